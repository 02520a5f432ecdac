"""The quantised-query decode over the planes (ops.attn_decode_pqv(query_bits=) -> spatten_attn_decode_pq_qint) against EXACT
math with the query the kernel exports (tests/pq_qint_exact.py): the case grid of tests/test_pq_qint_cpu.py — every criterion
of ``check_step`` at every threshold — head lists, the device-length form, a captured graph, split boundaries, a zero query,
the refusals and one launch at c5 geometry.  Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import pq_qint_exact as qx
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_pq_regimes import Inputs, _from_case
from tests.test_pq_qint_cpu import GRID, GRID_IDS, case, case_thresholds
from tests.util import TORCH_DT, dev, host

pytestmark = pytest.mark.gpu


def run(inp, bits, thr, heads=None, **kw):
    """One launch; a namespace of host arrays: out [B,H,d], need [B,H], stash, msb_logit [B,H,N], q_int [B,H,d], q_scale [B,H]."""
    from spatten_amd import ops
    B, H, d, N = inp.B, inp.H, inp.d, inp.N
    need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
    scores = torch.zeros(B, H, inp.cap, dtype=TORCH_DT[inp.dt], device="cuda")
    out = torch.zeros(B, H * d, dtype=TORCH_DT[inp.dt], device="cuda")
    q_int = torch.full((B, H, d), -128, dtype=torch.int8, device="cuda")
    q_scale = torch.full((B, H), -1.0, dtype=torch.float32, device="cuda")
    hid = None if heads is None else torch.tensor(heads, dtype=torch.int32, device="cuda")
    inp.pl.msb_logit.fill_(float("nan"))
    ops.attn_decode_pqv(inp.qd, inp.pl, N, inp.cos, inp.sin, N - 1, thr, out=out, need_lsb=need, scores=scores, head_ids=hid,
                        query_bits=bits, q_quant=(q_int, q_scale), **kw)
    torch.cuda.synchronize()
    return SimpleNamespace(out=host(out).reshape(B, H, d), need=need.cpu().numpy().reshape(B, H), stash=host(scores)[:, :, :N],
                           msb_logit=inp.pl.msb_logit[:, :, :N].cpu().numpy(), q_int=q_int.cpu().numpy().astype(np.int64),
                           q_scale=q_scale.cpu().numpy())


def check(inp, bits, thr, res, stats=None, **kw):
    return qx.check_step(inp.qr, inp.planes, inp.dt, bits, thr, res, stats=stats, **kw)


@pytest.mark.parametrize("regime,kb,vb,dt,d,Hkv,bits", GRID, ids=GRID_IDS)
def test_qint_grid(regime, kb, vb, dt, d, Hkv, bits):
    """The CPU test's grid: the exported query, msb_logit after an MSB-only launch, and stash / flags / band share / output at
    every threshold (picked on the CPU from the exact p1max alone)."""
    pc = case(regime, kb, vb, dt, d, Hkv)
    inp = _from_case(pc)
    stats = {}
    res = run(inp, bits, 0.0, msb_only=True)
    check(inp, bits, 0.0, res, stats=stats, msb_only=True, name=f"{regime} msb only")
    for thr in case_thresholds(pc, bits)[0]:
        res = run(inp, bits, thr)
        check(inp, bits, thr, res, stats=stats, name=f"{regime} thr={thr!r}")
    print(f"\n{regime} {kb} {dt} d{d} q{bits}: worst err / allowance {stats}")


def test_qint_head_list_leaves_pruned_heads_untouched():
    pc = case("sink24", 8, 8, "bf16", 64, 4)
    inp = _from_case(pc)
    heads = [1, 3]
    thr = case_thresholds(pc, 5)[0][2]
    res = run(inp, 5, thr, heads=heads)
    check(inp, 5, thr, res, heads=heads, name="head list")
    rest = [0, 2]
    assert not res.out[:, rest].any() and (res.need[:, rest] == -1).all() and not res.stash[:, rest].any()
    assert (res.q_int[:, rest] == -128).all() and (res.q_scale[:, rest] == -1.0).all()
    assert np.isnan(res.msb_logit[:, rest]).all()


@pytest.mark.parametrize("kb,dt,d", [(8, "bf16", 128), (4, "f16", 64)])
def test_qint_device_length_form_is_bit_identical(kb, dt, d):
    from spatten_amd import ops
    pc = case("flat", kb, 8, dt, d, 2 if dt == "f16" else 4)
    inp = _from_case(pc, extra=40)
    bits = 8
    thr = case_thresholds(pc, bits)[0][2]
    B, H, N, cap = inp.B, inp.H, inp.N, inp.cap
    cos_p, sin_p = oracle_table(cap, d, dt)
    res = []
    for dyn in (False, True):
        need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
        sc = torch.zeros(B, H, cap, dtype=TORCH_DT[dt], device="cuda")
        qq = (torch.zeros(B, H, d, dtype=torch.int8, device="cuda"), torch.zeros(B, H, dtype=torch.float32, device="cuda"))
        if dyn:
            st = ops.StepState(cos_p, sin_p)
            st.set(N - 1, N - 2)
            st.advance()
            o = ops.attn_decode_pqv(inp.qd, inp.pl, cap, cos_p, sin_p, 0, thr, scores=sc, need_lsb=need, step=st, query_bits=bits,
                                    q_quant=qq)
        else:
            o = ops.attn_decode_pqv(inp.qd, inp.pl, N, cos_p, sin_p, N - 1, thr, scores=sc, need_lsb=need, layout=cap,
                                    query_bits=bits, q_quant=qq)
        torch.cuda.synchronize()
        res.append((o.clone(), sc.clone(), need.clone(), qq[0].clone(), qq[1].clone(), inp.pl.msb_logit[:, :, :N].clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    o, sc, need, qi, qs, lg = res[1]
    r = SimpleNamespace(out=host(o).reshape(B, H, d), need=need.cpu().numpy().reshape(B, H), stash=host(sc)[:, :, :N],
                        msb_logit=lg.cpu().numpy(), q_int=qi.cpu().numpy().astype(np.int64), q_scale=qs.cpu().numpy())
    check(inp, bits, thr, r, name="device length")


def test_qint_captured_graph_replays_three_steps_like_the_eager_loop():
    """append (spatten_kv_append_planes, device length) + the quantised-query step, captured once and replayed three times,
    against the same three steps run eagerly: outputs, stash, flags and the exported query bit for bit."""
    from spatten_amd import ops
    dt, d, bits, steps = "bf16", 128, 8, 3
    pc = case("flat", 8, 8, dt, d, 4)
    cs = pc.cs
    B, H, Hkv, N0 = pc.B, pc.H, pc.Hkv, pc.N - steps
    cap = pc.N + 16
    tdt = TORCH_DT[dt]
    cos_p, sin_p = oracle_table(cap, d, dt)
    thr = case_thresholds(pc, bits)[0][2]
    # un-rotate nothing: the step's new rows are fresh random rows (the same in both runs)
    rng = np.random.default_rng(5)
    k_new = dev(orc.round_dt(rng.standard_normal((B, Hkv, d)).astype(np.float32), dt), dt)
    v_new = dev(orc.round_dt(rng.standard_normal((B, Hkv, d)).astype(np.float32), dt), dt)
    qd = dev(cs.q[:, :, 0], dt)

    def fresh():
        kr = torch.zeros(B, Hkv, cap, d, dtype=tdt, device="cuda")
        v = torch.zeros_like(kr)
        k = torch.zeros_like(kr)
        kr[:, :, :N0], v[:, :, :N0] = dev(cs.kr[:, :, :N0], dt), dev(cs.vc[:, :, :N0], dt)
        pl = ops.PQProfilePlanes(B, Hkv, H, cap, d, "cuda", key_bits=8, value_bits=8)
        ops.pq_pack_planes(kr, v, pl, 0, N0)
        st = ops.StepState(cos_p, sin_p)
        st.set(N0, N0 - 1)
        bufs = SimpleNamespace(out=torch.zeros(B, H * d, dtype=tdt, device="cuda"), sc=torch.zeros(B, H, cap, dtype=tdt, device="cuda"),
                               need=torch.zeros(B * H, dtype=torch.int32, device="cuda"),
                               qq=(torch.zeros(B, H, d, dtype=torch.int8, device="cuda"),
                                   torch.zeros(B, H, dtype=torch.float32, device="cuda")))
        return k, kr, v, pl, st, bufs

    def snap(b):
        return [t.clone() for t in (b.out, b.sc, b.need, b.qq[0], b.qq[1])]

    side = torch.cuda.Stream()
    ws = ops.DecodeWorkspace(B, H, d, "cuda")

    def step(k, kr, v, pl, st, b):
        st.advance()
        ops.kv_append_planes(k_new, v_new, k, kr, v, pl, 0, cos_p, sin_p, step=st)
        ops.attn_decode_pqv(qd, pl, cap, cos_p, sin_p, 0, thr, out=b.out, scores=b.sc, need_lsb=b.need, step=st, query_bits=bits,
                            q_quant=b.qq, workspace=ws)

    eager, replayed = [], []
    with torch.cuda.stream(side):
        A = fresh()
        for _ in range(steps):
            step(*A)
            side.synchronize()
            eager.append(snap(A[5]))
        Bf = fresh()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step(*Bf)
        for _ in range(steps):
            g.replay()
            side.synchronize()
            replayed.append(snap(Bf[5]))
    ws.check()
    for e, r in zip(eager, replayed):
        for x, y in zip(e, r):
            assert torch.equal(x, y)
    assert int(A[4].read()[0]) == int(Bf[4].read()[0]) == N0 + steps


@pytest.mark.parametrize("kb", [8, 4])
def test_qint_split_boundaries(kb):
    """kv_len not a multiple of the tile (2081 rows; tiles of 128 / 256 rows), n_splits forced to 1 and to 8."""
    pc = px.pq_case(1, 4, 4, 128, 2081, "bf16", "sink8", kb, 8)
    inp = _from_case(pc)
    ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, 8), pc.planes, 0.0)
    for thr in qx.thresholds(ex0)[1:3]:
        for ns in (1, 8):
            res = run(inp, 8, thr, n_splits=ns)
            check(inp, 8, thr, res, name=f"ns={ns} thr={thr!r}")


def test_qint_all_zero_query_head():
    pc = case("flat", 8, 8, "bf16", 128, 4)
    cs = pc.cs
    q = cs.q[:, :, 0].copy()
    q[:, 1] = 0
    qr = pc.qr.copy()
    qr[:, 1] = 0
    inp = Inputs(qr, q, cs.kr, cs.vc, 8, 8, "bf16")
    for thr in (0.0, 1.5):
        res = run(inp, 8, thr)
        assert (res.q_int[:, 1] == 0).all() and (res.q_scale[:, 1] == 0).all()
        assert (res.stash[:, 1] == 0).all() and (res.msb_logit[:, 1] == 0).all()
        check(inp, 8, thr, res, name=f"zero head thr={thr}")


def test_qint_refusals():
    from spatten_amd import ops
    pc = case("flat", 8, 8, "bf16", 128, 4)
    inp = _from_case(pc)
    args = (inp.qd, inp.pl, inp.N, inp.cos, inp.sin, inp.N - 1, 0.5)
    with pytest.raises(ValueError):
        ops.attn_decode_pqv(*args, query_bits=9)
    kr = torch.zeros(inp.B, inp.Hkv, inp.cap, inp.d, dtype=torch.bfloat16, device="cuda")
    kn = torch.zeros(inp.B, inp.Hkv, inp.d, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError, match="kv_append_planes"):
        ops.attn_decode_pqv(*args, query_bits=8, append=(kn, kn, None, kr, kr))
    p66 = _from_case(px.pq_case(1, 4, 4, 64, 300, "bf16", "flat", 6, 6))
    with pytest.raises(NotImplementedError):
        ops.attn_decode_pqv(p66.qd, p66.pl, p66.N, p66.cos, p66.sin, p66.N - 1, 0.5, query_bits=8)
    p32 = _from_case(px.pq_case(1, 4, 4, 64, 300, "f32", "flat", 8, 8))
    with pytest.raises(NotImplementedError):
        ops.attn_decode_pqv(p32.qd, p32.pl, p32.N, p32.cos, p32.sin, p32.N - 1, 0.5, query_bits=8)
    assert ops.pq_qint_supported(torch.bfloat16, 128, 8, 8, 8) and not ops.pq_qint_supported(torch.float32, 128, 8, 8, 8)
    # query_bits=None: the function is what it was
    o = ops.attn_decode_pqv(*args)
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()


def test_qint_c5_geometry():
    """40 heads x 8192 rows, d 128, (8, 8), bf16: flags and output criteria."""
    pc = px.pq_case(1, 40, 40, 128, 8192, "bf16", "sink8", 8, 8)
    inp = _from_case(pc)
    ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, 8), pc.planes, 0.0)
    for thr in qx.thresholds(ex0)[2:4]:
        res = run(inp, 8, thr)
        check(inp, 8, thr, res, only=("flags", "out"), name=f"c5 thr={thr!r}")
