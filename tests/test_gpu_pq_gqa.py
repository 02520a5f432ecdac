"""The grouped quantised-query decode (ops.attn_decode_pqv(query_bits=, grouped=True) -> spatten_attn_decode_pq_qint_gqa)
against EXACT math with the query the kernel exports (tests/pq_qint_exact.check_step, unchanged) and against the per-head form
(spatten_attn_decode_pq_qint) on the same inputs: q_int, q_scale, msb_logit and the MSB-only stash bit for bit — which is also the
exact-integer proof of the int8 MFMA operand maps.  Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import pq_qint_exact as qx
from tests import regimes as rg
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_pq_regimes import Inputs, _from_case
from tests.test_pq_gqa_cpu import GRID, GRID_IDS
from tests.test_pq_qint_cpu import case, case_thresholds
from tests.util import TORCH_DT, dev, host

pytestmark = pytest.mark.gpu


def run(inp, bits, thr, grouped=True, **kw):
    """One launch; a namespace of host arrays (tests/test_gpu_pq_qint.run) + the device tensors for bit comparisons."""
    from spatten_amd import ops
    B, H, d, N = inp.B, inp.H, inp.d, inp.N
    need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
    scores = torch.zeros(B, H, inp.cap, dtype=TORCH_DT[inp.dt], device="cuda")
    out = torch.zeros(B, H * d, dtype=TORCH_DT[inp.dt], device="cuda")
    q_int = torch.full((B, H, d), -128, dtype=torch.int8, device="cuda")
    q_scale = torch.full((B, H), -1.0, dtype=torch.float32, device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    inp.pl.msb_logit.fill_(float("nan"))
    ops.attn_decode_pqv(inp.qd, inp.pl, N, inp.cos, inp.sin, N - 1, thr, out=out, need_lsb=need, scores=scores, lse=lse,
                        query_bits=bits, q_quant=(q_int, q_scale), grouped=grouped, **kw)
    torch.cuda.synchronize()
    lg = inp.pl.msb_logit[:, :, :N].clone()
    return SimpleNamespace(out=host(out).reshape(B, H, d), need=need.cpu().numpy().reshape(B, H), stash=host(scores)[:, :, :N],
                           msb_logit=lg.cpu().numpy(), q_int=q_int.cpu().numpy().astype(np.int64), q_scale=q_scale.cpu().numpy(),
                           lse=lse.cpu().numpy(), t=SimpleNamespace(out=out, need=need, scores=scores, q_int=q_int, q_scale=q_scale, lg=lg))


def check(inp, bits, thr, res, stats=None, **kw):
    return qx.check_step(inp.qr, inp.planes, inp.dt, bits, thr, res, stats=stats, **kw)


def assert_msb_bits_equal(g, p, name=""):
    """q_int, q_scale, msb_logit and the stash of two launches, bit for bit."""
    for k in ("q_int", "q_scale", "lg", "scores"):
        assert torch.equal(getattr(g.t, k), getattr(p.t, k)), f"{name}: {k} differs from the per-head form"


@pytest.mark.parametrize("regime,dt,H,Hkv,bits", GRID, ids=GRID_IDS)
def test_gqa_grid(regime, dt, H, Hkv, bits):
    """Every regime: the MSB-only launch and every threshold by check_step; the MSB-only launch bit for bit against the per-head
    form; at every threshold q_int / q_scale / msb_logit still bit for bit (the stash then holds refetched rows of the heads each
    form flagged: judged by check_step)."""
    pc = case(regime, 8, 8, dt, 128, Hkv, H=H)
    inp = _from_case(pc)
    stats = {}
    res = run(inp, bits, 0.0, msb_only=True)
    check(inp, bits, 0.0, res, stats=stats, msb_only=True, name=f"{regime} msb only")
    ref = run(inp, bits, 0.0, grouped=False, msb_only=True)
    assert_msb_bits_equal(res, ref, f"{regime} msb only")
    for thr in case_thresholds(pc, bits)[0]:
        res = run(inp, bits, thr)
        check(inp, bits, thr, res, stats=stats, name=f"{regime} thr={thr!r}")
    print(f"\n{regime} {dt} {H}/{Hkv} q{bits}: worst err / allowance {stats}")


def test_gqa_device_length_form_is_bit_identical():
    from spatten_amd import ops
    dt, d, bits = "bf16", 128, 8
    pc = case("flat", 8, 8, dt, d, 2, H=8)
    inp = _from_case(pc, extra=40)
    thr = case_thresholds(pc, bits)[0][2]
    B, H, N, cap = inp.B, inp.H, inp.N, inp.cap
    cos_p, sin_p = oracle_table(cap, d, dt)
    res = []
    for dyn in (False, True):
        need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
        sc = torch.zeros(B, H, cap, dtype=TORCH_DT[dt], device="cuda")
        qq = (torch.zeros(B, H, d, dtype=torch.int8, device="cuda"), torch.zeros(B, H, dtype=torch.float32, device="cuda"))
        lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
        if dyn:
            st = ops.StepState(cos_p, sin_p)
            st.set(N - 1, N - 2)
            st.advance()
            o = ops.attn_decode_pqv(inp.qd, inp.pl, cap, cos_p, sin_p, 0, thr, scores=sc, need_lsb=need, lse=lse, step=st,
                                    query_bits=bits, q_quant=qq, grouped=True)
        else:
            o = ops.attn_decode_pqv(inp.qd, inp.pl, N, cos_p, sin_p, N - 1, thr, scores=sc, need_lsb=need, lse=lse, layout=cap,
                                    query_bits=bits, q_quant=qq, grouped=True)
        torch.cuda.synchronize()
        res.append((o.clone(), sc.clone(), need.clone(), qq[0].clone(), qq[1].clone(), lse.clone(), inp.pl.msb_logit[:, :, :N].clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    o, sc, need, qi, qs, _, lg = res[1]
    r = SimpleNamespace(out=host(o).reshape(B, H, d), need=need.cpu().numpy().reshape(B, H), stash=host(sc)[:, :, :N],
                        msb_logit=lg.cpu().numpy(), q_int=qi.cpu().numpy().astype(np.int64), q_scale=qs.cpu().numpy())
    check(inp, bits, thr, r, name="device length")


def test_gqa_multi_split_32_over_8_heads():
    """32 / 8 heads x 5003 rows (not a multiple of 32 nor of the chunk): automatic splits and forced 1 / 7 splits."""
    pc = px.pq_case(1, 32, 8, 128, 5003, "bf16", "sink8", 8, 8)
    inp = _from_case(pc)
    ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, 8), pc.planes, 0.0)
    ref = run(inp, 8, 0.0, grouped=False, msb_only=True)
    for ns in (0, 1, 7):
        res = run(inp, 8, 0.0, msb_only=True, n_splits=ns)
        assert_msb_bits_equal(res, ref, f"ns={ns}")
        check(inp, 8, 0.0, res, msb_only=True, name=f"ns={ns} msb only")
        for thr in qx.thresholds(ex0)[1:3]:
            res = run(inp, 8, thr, n_splits=ns)
            check(inp, 8, thr, res, name=f"ns={ns} thr={thr!r}")


def test_gqa_cache_shorter_than_one_tile_per_wave():
    for N in (5, 33, 100):
        pc = px.pq_case(2, 8, 2, 128, N, "f16", "flat", 8, 8)
        inp = _from_case(pc)
        ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, 8), pc.planes, 0.0)
        ref = run(inp, 8, 0.0, grouped=False, msb_only=True)
        res = run(inp, 8, 0.0, msb_only=True)
        assert_msb_bits_equal(res, ref, f"N={N}")
        for thr in qx.thresholds(ex0)[:2]:
            check(inp, 8, thr, run(inp, 8, thr), name=f"N={N} thr={thr!r}")


def test_gqa_all_zero_query_head():
    pc = case("flat", 8, 8, "bf16", 128, 2, H=8)
    cs = pc.cs
    q = cs.q[:, :, 0].copy()
    q[:, 5] = 0
    qr = pc.qr.copy()
    qr[:, 5] = 0
    inp = Inputs(qr, q, cs.kr, cs.vc, 8, 8, "bf16")
    for thr in (0.0, 1.5):
        res = run(inp, 8, thr)
        assert (res.q_int[:, 5] == 0).all() and (res.q_scale[:, 5] == 0).all()
        assert (res.stash[:, 5] == 0).all() and (res.msb_logit[:, 5] == 0).all()
        check(inp, 8, thr, res, name=f"zero head thr={thr}")


def test_gqa_refusals():
    from spatten_amd import _lib, ops
    import ctypes
    pc = case("flat", 8, 8, "bf16", 128, 2, H=8)
    inp = _from_case(pc)
    args = (inp.qd, inp.pl, inp.N, inp.cos, inp.sin, inp.N - 1, 0.5)
    with pytest.raises(ValueError):
        ops.attn_decode_pqv(*args, grouped=True)
    hid = torch.arange(8, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="head"):
        ops.attn_decode_pqv(*args, query_bits=8, grouped=True, head_ids=hid)
    with pytest.raises(NotImplementedError, match="head"):
        ops.attn_decode_pqv(*args, query_bits=8, grouped=True, head_abs=torch.zeros(inp.B * 8, device="cuda"))
    kr = torch.zeros(inp.B, inp.Hkv, inp.cap, inp.d, dtype=torch.bfloat16, device="cuda")
    kn = torch.zeros(inp.B, inp.Hkv, inp.d, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError, match="kv_append_planes"):
        ops.attn_decode_pqv(*args, query_bits=8, grouped=True, append=(kn, kn, None, kr, kr))
    for bad in (px.pq_case(1, 4, 4, 128, 300, "bf16", "flat", 8, 8),      # not grouped
                px.pq_case(1, 8, 2, 64, 300, "bf16", "flat", 8, 8),       # head_dim 64
                px.pq_case(1, 8, 2, 128, 300, "bf16", "flat", 4, 8),      # profile (4, 8)
                px.pq_case(1, 8, 2, 128, 300, "f32", "flat", 8, 8)):      # fp32
        bi = _from_case(bad)
        with pytest.raises(NotImplementedError):
            ops.attn_decode_pqv(bi.qd, bi.pl, bi.N, bi.cos, bi.sin, bi.N - 1, 0.5, query_bits=8, grouped=True)

    # the C entry point itself returns the documented codes (the ops layer raises before it gets there)
    lib = _lib.load()
    B, H, d, N = inp.B, inp.H, inp.d, inp.N
    out = torch.zeros(B, H * d, dtype=torch.bfloat16, device="cuda")
    need = torch.zeros(B * H, dtype=torch.int32, device="cuda")
    qi, qs = torch.zeros(B, H, d, dtype=torch.int8, device="cuda"), torch.zeros(B, H, dtype=torch.float32, device="cuda")
    ws = ops.DecodeWorkspace(B, H, d, "cuda")

    def call(planes=inp.pl, q=inp.qd, dtype=2, **over):
        a = _lib.PQDecodeArgs()
        a.struct_size, a.dtype = ctypes.sizeof(_lib.PQDecodeArgs), dtype
        a.q, a.q_sb, a.q_sh = q.data_ptr(), q.stride(0), q.stride(1)
        a.planes = ctypes.pointer(planes.desc)
        a.cos, a.sin, a.table_rows, a.pos_q = inp.cos.data_ptr(), inp.sin.data_ptr(), inp.cos.shape[0], N - 1
        a.out, a.out_sb = out.data_ptr(), out.stride(0)
        a.need_lsb, a.threshold = need.data_ptr(), 0.5
        a.workspace, a.workspace_splits = ws.buf.data_ptr(), ws.max_splits
        a.batch, a.heads, a.kv_heads, a.head_dim, a.kv_len = B, q.shape[1], planes.msb.shape[1], q.shape[2], N
        for k, v in over.items():
            setattr(a, k, v)
        qa = _lib.PQQintArgs()
        qa.struct_size, qa.query_bits, qa.step = ctypes.sizeof(_lib.PQQintArgs), 8, a
        qa.q_int, qa.qi_sb, qa.qi_sh, qa.q_scale = qi.data_ptr(), qi.stride(0), qi.stride(1), qs.data_ptr()
        return lib.spatten_attn_decode_pq_qint_gqa(ctypes.byref(qa), None)

    UNSUPPORTED = -2                                                     # SPATTEN_ERR_UNSUPPORTED
    assert call(head_ids=hid.data_ptr(), n_active_heads=8) == UNSUPPORTED
    assert call(head_abs_acc=torch.zeros(B * H, device="cuda").data_ptr()) == UNSUPPORTED
    assert call(k_new=kn.data_ptr(), v_new=kn.data_ptr(), kr_cache=kr.data_ptr(), v_cache=kr.data_ptr()) == UNSUPPORTED
    p48 = _from_case(px.pq_case(B, 8, 2, 128, N, "bf16", "flat", 4, 8))
    assert call(planes=p48.pl) == UNSUPPORTED
    assert call(dtype=0) == UNSUPPORTED                                  # fp32 (refused before anything is read)
    assert call(kv_heads=8) == UNSUPPORTED                               # heads == kv_heads
    torch.cuda.synchronize()
    assert call() == 0                                                    # and the untouched call is taken
    torch.cuda.synchronize()
    ws.check()


def test_gqa_captured_graph_replays_three_steps_like_the_eager_loop():
    """append (spatten_kv_append_planes, device length) + the grouped step, captured once and replayed three times, against the
    same three steps run eagerly: outputs, stash, flags, lse and the exported query bit for bit."""
    from spatten_amd import ops
    dt, d, bits, steps = "bf16", 128, 8, 3
    pc = case("flat", 8, 8, dt, d, 2, H=8)
    cs = pc.cs
    B, H, Hkv, N0 = pc.B, pc.H, pc.Hkv, pc.N - steps
    cap = pc.N + 16
    tdt = TORCH_DT[dt]
    cos_p, sin_p = oracle_table(cap, d, dt)
    thr = case_thresholds(pc, bits)[0][2]
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
                               lse=torch.zeros(B, H, 2, dtype=torch.float32, device="cuda"),
                               qq=(torch.zeros(B, H, d, dtype=torch.int8, device="cuda"),
                                   torch.zeros(B, H, dtype=torch.float32, device="cuda")))
        return k, kr, v, pl, st, bufs

    def snap(b):
        return [t.clone() for t in (b.out, b.sc, b.need, b.lse, b.qq[0], b.qq[1])]

    side = torch.cuda.Stream()
    ws = ops.DecodeWorkspace(B, H, d, "cuda")

    def step(k, kr, v, pl, st, b):
        st.advance()
        ops.kv_append_planes(k_new, v_new, k, kr, v, pl, 0, cos_p, sin_p, step=st)
        ops.attn_decode_pqv(qd, pl, cap, cos_p, sin_p, 0, thr, out=b.out, scores=b.sc, need_lsb=b.need, lse=b.lse, step=st,
                            query_bits=bits, q_quant=b.qq, workspace=ws, grouped=True)

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
    assert eager[0][0].float().abs().sum() > 0


def test_gqa_and_per_head_launches_alternate_on_one_workspace():
    """A per-head launch and a grouped launch alternating on ONE workspace (multi-split both): each repeats its own first
    result bit for bit, and the workspace reports no error."""
    from spatten_amd import ops
    pc = px.pq_case(1, 32, 8, 128, 3001, "bf16", "sink8", 8, 8)
    inp = _from_case(pc)
    ws = ops.DecodeWorkspace(inp.B, inp.H, inp.d, "cuda")
    ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, 8), pc.planes, 0.0)
    thr = qx.thresholds(ex0)[2]
    first = {}
    for rep in range(3):
        for grouped in (False, True):
            res = run(inp, 8, thr, grouped=grouped, workspace=ws)
            if rep == 0:
                first[grouped] = res
                check(inp, 8, thr, res, name=f"grouped={grouped}")
            else:
                for k in ("out", "need", "scores", "q_int", "q_scale", "lg"):
                    assert torch.equal(getattr(res.t, k), getattr(first[grouped].t, k)), (rep, grouped, k)
    ws.check()
