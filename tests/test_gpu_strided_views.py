"""Strided C-ABI arguments on padded views with guard bands (tests/strided.py).  Every case runs one call twice —
on fresh contiguous tensors, whose result the rest of the suite judges, and on views into larger parents with distinct strides —
and asserts equality of bits of every argument and result, and that no parent byte outside a view changed.  The guards of
inputs hold NaN / 0x7fffffff / 0xFF, so equality also shows none of them was read.  No tolerance anywhere.  Needs an MI355X."""
import math

import pytest
import torch

from oracle import spatten_oracle as orc
from tests.strided import PADS, Case
from tests.util import TORCH_DT, dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DTC = {"f32": 0, "f16": 1, "bf16": 2}


def R(seed, sid, shape, dt, scale=1.0):
    return dev(orc.synth_normal(seed, sid, shape, dt, scale), dt)


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cache(B, Hkv, cap, d, dt, seed):
    """K / shadow / V [B,Hkv,cap,d] with finite non-zero values in EVERY row (the device-length forms read rows up to the bound)
    and the rotary tables covering the capacity."""
    from spatten_amd import ops
    cos, sin = ops.rope_table(cap, d, TORCH_DT[dt], DEV)
    K, V = R(seed, 3, (B, Hkv, cap, d), dt), R(seed, 4, (B, Hkv, cap, d), dt)
    Kr = torch.zeros_like(K)
    ops.build_shadow(K, Kr, 0, cap, cos, sin)
    return K, Kr, V, cos, sin


def _cap(N):
    return (N + 64 + 127) // 128 * 128


def _lse_of(stash, n):
    x = stash[..., :n].float()
    m = x.max(-1).values
    return torch.stack([m, torch.exp(x - m[..., None]).sum(-1)], -1).contiguous()


def _mask(B, N, dt, seed):
    m = torch.zeros(B, N, dtype=TORCH_DT[dt], device=DEV)
    m[:, 3::17] = torch.finfo(TORCH_DT[dt]).min
    m[B - 1, :5] = -1.5
    return m


def _step(ops, cos, sin, N):
    st = ops.StepState(cos, sin)
    st.set(N - 1, N - 2)
    st.advance()           # the step that appends row N - 1: length N, query position N - 1
    return st


# ------------------------------------------------------------------------------------------------
# 1. the plain decode step (spatten_attn_decode_args)
# ------------------------------------------------------------------------------------------------
DECODE = [
    # B, H, Hkv, d, N, dtype, n_splits, variant
    (2, 4, 2, 128, 333, "bf16", 0, "mask"), (2, 4, 2, 128, 333, "bf16", 0, "cascade"),
    (2, 4, 2, 128, 2081, "bf16", 0, "mask"), (2, 4, 2, 128, 2081, "bf16", 0, "cascade"),
    (2, 4, 2, 128, 2081, "bf16", 7, "mask"), (2, 4, 2, 128, 2081, "bf16", 7, "cascade"),
    (2, 4, 2, 128, 333, "bf16", 0, "head_ids"), (2, 4, 2, 128, 333, "bf16", 0, "step"), (2, 4, 2, 128, 2081, "bf16", 0, "step"),
    (2, 4, 2, 64, 333, "bf16", 0, "mask"), (2, 4, 2, 128, 333, "f32", 0, "cascade"), (2, 4, 2, 128, 333, "f16", 0, "mask"),
    (1, 4, 2, 128, 333, "bf16", 0, "mask"),
    (2, 8, 2, 128, 2099, "bf16", 0, "gqa"),
    (1, 32, 32, 128, 300, "bf16", 0, "proj"),
]


@pytest.mark.parametrize("B,H,Hkv,d,N,dt,n_splits,variant", DECODE,
                         ids=[f"B{c[0]}-H{c[1]}-{c[2]}-d{c[3]}-n{c[4]}-{c[5]}-s{c[6]}-{c[7]}" for c in DECODE])
def test_plain_decode_step(B, H, Hkv, d, N, dt, n_splits, variant):
    """q, k_new / v_new, the three cache planes, mask, a stride-3 position vector, out, stash, lse, the cascade's accumulator and
    previous stash, the projection's weight and output — all views; mask and cascade exclude each other in the ABI, so each
    geometry runs both.  ``step``: the device-length form (bound = capacity).  ``gqa``: the matrix-core form, forced."""
    from spatten_amd import ops
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["decode"]
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 11)
    c = Case()
    c.arg("q", R(11, 0, (B, H, d), dt), P["q"]).arg("k_new", R(11, 1, (B, Hkv, d), dt), P["k_new"])
    c.arg("v_new", R(11, 2, (B, Hkv, d), dt), P["v_new"]).arg("K", K, P["K"]).arg("Kr", Kr, P["Kr"]).arg("V", V, P["V"])
    c.arg("out", _full((B, H * d), 0.5, tdt), P["out"]).arg("scores", _full((B, H, cap), 3.0, tdt), P["scores"])
    c.arg("lse", _full((B, H, 2), 7.0, torch.float32), "flat")
    if variant in ("mask", "head_ids"):
        c.arg("mask", _mask(B, N, dt, 11), P["mask"])
    if variant in ("mask", "head_ids", "cascade"):
        pos = torch.tensor([[N - 1], [N - 5]][:B], dtype=torch.int64, device=DEV)
        c.arg("pos", pos, P["pos"])                      # [B, 1] inside [B + 2, 3]: column 0 is a [B] vector of stride 3
    if variant == "cascade":
        prev = R(11, 5, (B, H, cap), dt)
        c.arg("prev", prev, P["prev"]).arg("prev_lse", _lse_of(prev, N - 1), "flat")
        c.arg("acc", torch.zeros(H, cap, dtype=torch.float32, device=DEV), P["acc"])      # zero: two atomic adds commute
    if variant == "head_ids":
        c.arg("head_ids", torch.tensor([1, 3], dtype=torch.int32, device=DEV), "flat")
    if variant == "proj":
        n_out = H * d + 24
        c.arg("W", R(11, 6, (n_out, H * d), dt, (H * d) ** -0.5), P["W"]).arg("bias", R(11, 7, (n_out,), dt), "flat")
        c.arg("y", _full((B, n_out), 0.25, tdt), P["y"])

    def fn(a):
        kw = dict(k_new=a.k_new, v_new=a.v_new, out=a.out, scores=a.scores, lse=a.lse, n_splits=n_splits)
        if hasattr(a, "mask"):
            kw["mask"] = a.mask
        if hasattr(a, "pos"):
            kw["position_ids"] = a.pos[:, 0]
            assert a.pos[:, 0].stride(0) == (3 if a.strided else 1)
        if variant == "cascade":
            kw["cascade"] = (a.acc, a.prev, a.prev_lse, N - 1)
        if variant == "head_ids":
            kw["head_ids"] = a.head_ids
        if variant == "proj":
            kw["proj"] = (a.W, a.bias, a.y)
        if variant == "step":
            ops.attn_decode(a.q, a.K, a.Kr, a.V, cap, cos, sin, 0, step=_step(ops, cos, sin, N), **kw)
        else:
            ops.attn_decode(a.q, a.K, a.Kr, a.V, N, cos, sin, N - 1, **kw)

    if variant == "gqa":
        prev_mode = ops.set_decode_gqa(1)
        try:
            assert ops.decode_gqa_selected(tdt, B, H, Hkv, d, N)
            c.run(fn)
        finally:
            ops.set_decode_gqa(prev_mode)
    else:
        c.run(fn)
    ops.check_workspaces()


# ------------------------------------------------------------------------------------------------
# 2. the chained decode launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["static", "step"])
def test_chained_decode(form):
    """Two layers; every layer's planes, k_new / v_new, out and stash are views of ONE padded geometry (the chain takes one set of
    strides for all layers); q is dense by the ABI and sits inside a 1-D parent."""
    from spatten_amd import ops
    L, B, H, d, N, dt = 2, 2, 4, 128, 333, "bf16"
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["decode"]
    c = Case()
    cos = sin = None
    for l in range(L):
        K, Kr, V, cos, sin = _cache(B, H, cap, d, dt, 20 + l)
        c.arg(f"q{l}", R(20 + l, 0, (B, H, d), dt), "flat").arg(f"k_new{l}", R(20 + l, 1, (B, H, d), dt), P["k_new"] if l == 0 else P["k_new"][0])
        c.arg(f"v_new{l}", R(20 + l, 2, (B, H, d), dt), P["v_new"]).arg(f"K{l}", K, P["K"] if l == 0 else P["K"][0])
        c.arg(f"Kr{l}", Kr, P["Kr"]).arg(f"V{l}", V, P["V"])
        c.arg(f"out{l}", _full((B, H * d), 0.5, tdt), P["out"] if l == 0 else P["out"][0])
        c.arg(f"scores{l}", _full((B, H, cap), 3.0, tdt), P["scores"] if l == 0 else P["scores"][0])

    def fn(a):
        g = lambda n: [getattr(a, f"{n}{l}") for l in range(L)]
        chain = ops.DecodeChain(g("q"), g("K"), g("Kr"), g("V"), g("out"), k_new=g("k_new"), v_new=g("v_new"), scores=g("scores"))
        if form == "step":
            chain(cap, cos, sin, 0, step=_step(ops, cos, sin, N))
        else:
            chain(N, cos, sin, N - 1)
        torch.cuda.synchronize()
        chain.check()

    c.run(fn)


# ------------------------------------------------------------------------------------------------
# 3. local V pruning in one launch (and its append form)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,N,form,append", [("bf16", 300, "static", False), ("bf16", 300, "step", True), ("bf16", 600, "static", True),
                                              ("bf16", 600, "step", False), ("f16", 600, "static", False), ("f32", 300, "static", True)])
def test_local_v(dt, N, form, append):
    """One split at 300 rows, two at 600 (a split holds at least 256); keep 30 %."""
    from spatten_amd import ops
    B, H, Hkv, d = 2, 4, 2, 128
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["decode"]
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 31)
    c = Case().arg("q", R(31, 0, (B, H, d), dt), P["q"]).arg("Kr", Kr, P["K"]).arg("V", V, P["V"])
    c.arg("out", _full((B, H * d), 0.5, tdt), P["out"]).arg("scores", _full((B, H, cap), 3.0, tdt), P["scores"])
    c.arg("lse", _full((B, H, 2), 7.0, torch.float32), "flat")
    if append:
        c.arg("K", K, P["Kr"]).arg("k_new", R(31, 1, (B, Hkv, d), dt), P["k_new"]).arg("v_new", R(31, 2, (B, Hkv, d), dt), P["v_new"])

    def fn(a):
        kw = dict(out=a.out, lse=a.lse, keep_fraction=0.3)
        if append:
            kw.update(k_new=a.k_new, v_new=a.v_new, k_cache=a.K)
        if form == "step":
            ops.attn_decode_local_v(a.q, a.Kr, a.V, cap, cos, sin, 0, 1, a.scores, step=_step(ops, cos, sin, N), **kw)
        else:
            ops.attn_decode_local_v(a.q, a.Kr, a.V, N, cos, sin, N - 1, math.ceil(0.3 * N), a.scores, **kw)

    c.run(fn)


# ------------------------------------------------------------------------------------------------
# 4. profiled planes: pack, append, decode (plain / in-launch append / cascade / quantised query / grouped), and the legacy planes
# ------------------------------------------------------------------------------------------------
PLANES = [
    # key bits, value bits, N, dtype, variant
    (8, 8, 333, "bf16", "plain"), (8, 8, 2081, "bf16", "append"), (6, 6, 333, "bf16", "append"), (6, 6, 2081, "bf16", "plain"),
    (4, 8, 333, "bf16", "plain"), (8, 8, 333, "bf16", "cascade"), (6, 6, 2081, "bf16", "cascade"), (8, 8, 2081, "bf16", "qint"),
    (4, 8, 333, "bf16", "qint"), (8, 8, 333, "bf16", "grouped"), (8, 8, 2081, "bf16", "grouped"), (8, 8, 333, "f16", "plain"),
    (6, 6, 333, "f32", "plain"), (8, 8, 333, "bf16", "step"),
]


@pytest.mark.parametrize("kb,vb,N,dt,variant", PLANES, ids=[f"k{c[0]}v{c[1]}-n{c[2]}-{c[3]}-{c[4]}" for c in PLANES])
def test_profiled_planes(kb, vb, N, dt, variant):
    """pq_pack_planes over rows [0, N - 1), the step's row through kv_append_planes (or inside the MSB pass: ``append``), then
    attn_decode_pqv — every plane of PQProfilePlanes a view with its own pads: byte strides for the key MSB / LSB and value
    planes, element strides for the two scales and msb_logit.  Threshold 1: every head refetches, so the LSB plane and msb_logit
    are read; the 333-row plain cases sit at 0.04, near the heads' largest probability."""
    from spatten_amd import ops
    B, H, Hkv, d = 2, 4, 2, 128
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["planes"]
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 41)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    c = Case().arg("q", R(41, 0, (B, H, d), dt), P["q"]).arg("k_new", R(41, 1, (B, Hkv, d), dt), P["k_new"])
    c.arg("v_new", R(41, 2, (B, Hkv, d), dt), P["v_new"]).arg("K", K, P["K"]).arg("Kr", Kr, P["Kr"]).arg("V", V, P["V"])
    c.arg("out", _full((B, H * d), 0.5, tdt), P["out"]).arg("scores", _full((B, H, cap), 3.0, tdt), P["scores"])
    c.arg("lse", _full((B, H, 2), 7.0, torch.float32), "flat").arg("need", _full((B * H,), -3, torch.int32), "flat")
    c.arg("msb", u8(B, Hkv, cap, d * kb // 8), P["msb"]).arg("lsb", u8(B, Hkv, cap, d // 2), P["lsb"])
    c.arg("vq", u8(B, Hkv, cap, d * vb // 8), P["vq"])
    c.arg("scale", _full((B, Hkv, cap), 1.0, torch.float32), P["scale"]).arg("vscale", _full((B, Hkv, cap), 1.0, torch.float32), P["vscale"])
    c.arg("lg", R(41, 8, (B, H, cap), "f32"), P["lg"])        # finite: the cascade fold reads the "previous step's" logits
    if variant == "cascade":
        c.arg("acc", torch.zeros(H, cap, dtype=torch.float32, device=DEV), P["acc"])       # zero: two atomic adds commute
        c.arg("prev_lse", torch.tensor([4.0, 50.0], device=DEV).repeat(B, H, 1).contiguous(), "flat")
    if variant in ("qint", "grouped"):
        c.arg("q_int", torch.full((B, H, d), 77, dtype=torch.int8, device=DEV), P["q_int"])
        c.arg("q_scale", _full((B, H), 9.0, torch.float32), "flat")
    thr = 0.04 if (variant == "plain" and N == 333) else 1.0

    def fn(a):
        planes = ops.PQProfilePlanes(B, Hkv, H, cap, d, DEV, kb, vb, tensors=(a.msb, a.lsb, a.scale, a.vq, a.vscale, a.lg))
        kw = dict(out=a.out, need_lsb=a.need, scores=a.scores, lse=a.lse)
        if variant == "step":
            st = _step(ops, cos, sin, N)
            ops.pq_pack_planes(a.Kr, a.V, planes, 0, N - 1)
            ops.kv_append_planes(a.k_new, a.v_new, a.K, a.Kr, a.V, planes, 0, cos, sin, step=st)
            ops.attn_decode_pqv(a.q, planes, cap, cos, sin, 0, thr, step=st, **kw)
            return
        ops.pq_pack_planes(a.Kr, a.V, planes, 0, N - 1)
        if variant == "append":
            kw["append"] = (a.k_new, a.v_new, a.K, a.Kr, a.V)
        else:
            ops.kv_append_planes(a.k_new, a.v_new, a.K, a.Kr, a.V, planes, N - 1, cos, sin)
        if variant == "cascade":
            kw["cascade"] = (a.acc, a.prev_lse, N - 1)
        if variant in ("qint", "grouped"):
            kw.update(query_bits=8, q_quant=(a.q_int, a.q_scale), grouped=variant == "grouped")
        ops.attn_decode_pqv(a.q, planes, N, cos, sin, N - 1, thr, **kw)

    if variant == "grouped":
        assert ops.pq_qint_gqa_supported(tdt, H, Hkv, d, kb, vb, 8)
    c.run(fn)
    ops.check_workspaces()


@pytest.mark.parametrize("form", ["static", "step"])
def test_legacy_planes(form):
    """pq_pack + attn_decode_pq (the pq_* fields of the decode argument block) over the nibble planes; ``step``: the row through
    kv_append_step with its planes, then the device-length decode."""
    from spatten_amd import ops
    B, H, Hkv, d, N, dt = 2, 4, 2, 128, 333, "bf16"
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["legacy_planes"]
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 43)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    c = Case().arg("q", R(43, 0, (B, H, d), dt), P["q"]).arg("k_new", R(43, 1, (B, Hkv, d), dt), P["k_new"])
    c.arg("v_new", R(43, 2, (B, Hkv, d), dt), P["v_new"]).arg("K", K, P["K"]).arg("Kr", Kr, P["Kr"]).arg("V", V, P["V"])
    c.arg("out", _full((B, H * d), 0.5, tdt), P["out"]).arg("scores", _full((B, H, cap), 3.0, tdt), P["scores"])
    c.arg("lse", _full((B, H, 2), 7.0, torch.float32), "flat").arg("need", _full((B * H,), -3, torch.int32), "flat")
    c.arg("msb", u8(B, Hkv, cap, d // 2), P["msb"]).arg("lsb", u8(B, Hkv, cap, d // 2), P["lsb"])
    c.arg("scale", _full((B, Hkv, cap), 1.0, torch.float32), P["scale"])

    def fn(a):
        planes = ops.PQPlanes(1, 1, 1, d, DEV)
        planes.msb, planes.lsb, planes.scale = a.msb, a.lsb, a.scale
        if form == "step":
            ops.pq_pack(a.Kr, planes, 0, cap)              # finite plane rows up to the bound
            st = _step(ops, cos, sin, N)
            ops.kv_append_step(a.k_new, a.v_new, a.K, a.Kr, a.V, st, planes=planes)
            ops.attn_decode(a.q, None, None, a.V, cap, cos, sin, 0, out=a.out, scores=a.scores, lse=a.lse, step=st,
                            pq=(planes, 1.0, a.need))
        else:
            ops.pq_pack(a.Kr, planes, 0, N)
            ops.attn_decode_pq(a.q, planes, a.V, N, cos, sin, N - 1, 1.0, out=a.out, need_lsb=a.need, lse=a.lse, scores=a.scores)

    c.run(fn)


# ------------------------------------------------------------------------------------------------
# 5. append and rotation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_append_and_rotation(dt):
    """kv_append of 5 rows from the transposed [B,n,Hkv,d] projection view (new_sn = a whole token), kv_append_step, build_shadow
    on cache views, rope_single with x and y padded differently and a padded position matrix."""
    from spatten_amd import ops
    B, H, Hkv, d, N, n = 2, 4, 2, 128, 77, 5
    tdt, cap = TORCH_DT[dt], 128
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 51)
    P = PADS["append"]
    c = Case().arg("k_new4", R(51, 1, (B, n, Hkv, d), dt), P["k_new4"]).arg("v_new4", R(51, 2, (B, n, Hkv, d), dt), P["v_new4"])
    c.arg("K", K, P["K"]).arg("Kr", torch.zeros_like(Kr), P["Kr"]).arg("V", V, P["V"])
    c.arg("k_new", R(51, 5, (B, Hkv, d), dt), PADS["decode"]["k_new"]).arg("v_new", R(51, 6, (B, Hkv, d), dt), PADS["decode"]["v_new"])

    def fn(a):
        ops.build_shadow(a.K, a.Kr, 3, N, cos, sin)
        kn, vn = a.k_new4.transpose(1, 2), a.v_new4.transpose(1, 2)
        assert kn.stride(2) > kn.stride(1)
        ops.kv_append(kn, vn, a.K, a.Kr, a.V, N, cos, sin)
        st = ops.StepState(cos, sin)
        st.set(N + n, N + n - 1)
        st.advance()
        ops.kv_append_step(a.k_new, a.v_new, a.K, a.Kr, a.V, st)

    c.run(fn)

    P = PADS["rope"]
    pos = torch.tensor([[0, 5, 2, 90, 17, 127, 64], [3, 3, 1, 0, 100, 9, 8]], dtype=torch.int64, device=DEV)
    c = Case().arg("x", R(52, 0, (B, H, 7, d), dt), P["x"]).arg("y", _full((B, H, 7, d), 0.5, tdt), P["y"]).arg("pos", pos, P["pos"])
    c.run(lambda a: ops.rope_single(a.x, cos, sin, position_ids=a.pos, out=a.y))


# ------------------------------------------------------------------------------------------------
# 6. prefill
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pl,ql,qpads", [(77, 130, False), (77, 130, True), (300, 9, False), (300, 9, True)])
def test_prefill(Pl, ql, qpads):
    """attn_prefill with q as the transposed projection view ([B,q,H*d] seen as [B,H,q,d]: q_sq = H*d, q_sh = d; ``qpads``: the
    same with pads behind the head and the row), mask, out, stash and positions padded; then importance_accumulate_prefill on the
    row statistics that call wrote, and attn_prefill_pq over padded nibble planes."""
    from spatten_amd import ops
    B, H, Hkv, d, dt = 2, 4, 2, 128, "bf16"
    N = Pl + ql
    tdt, cap, P = TORCH_DT[dt], _cap(N), PADS["prefill"]
    K, Kr, V, cos, sin = _cache(B, Hkv, cap, d, dt, 61)
    mask = torch.zeros(B, ql, N, dtype=tdt, device=DEV)
    mask[:, :, 2::13] = torch.finfo(tdt).min
    pos = (torch.arange(ql, device=DEV)[None] + torch.tensor([[Pl], [Pl - 2]], device=DEV)).to(torch.int64)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    c = Case().arg("qp", R(61, 0, (B, ql, H, d), dt), P["qp"] if qpads else ((1, 1, 0, 0), ()))
    c.arg("Kr", Kr, P["K"]).arg("V", V, P["V"]).arg("mask", mask, P["mask"]).arg("pos", pos, P["pos"])
    c.arg("out", _full((B, ql, H * d), 0.5, tdt), P["out"]).arg("stash", _full((B, H, ql, N), 3.0, tdt), P["stash"])
    c.arg("lse", _full((B, H, ql, 2), 7.0, torch.float32), "flat")
    c.arg("acc", torch.zeros(H, N, dtype=torch.float32, device=DEV), P["acc"])          # zero: two atomic adds commute
    c.arg("msb", u8(B, Hkv, cap, d // 2), P["msb"]).arg("lsb", u8(B, Hkv, cap, d // 2), P["lsb"])
    c.arg("scale", _full((B, Hkv, cap), 1.0, torch.float32), P["scale"])
    c.arg("out_pq", _full((B, ql, H * d), 0.5, tdt), ((1, 2, 24), ())).arg("need", _full((B, H, ql), -3, torch.int32), "flat")

    def fn(a):
        q = a.qp.transpose(1, 2)                       # [B,H,q,d] over the projection's [B,q,H,d]
        if not a.strided:
            q = q.contiguous()                         # what today's tests pass
        ops.attn_prefill(q, a.Kr, a.V, N, cos, sin, Pl, causal=True, position_ids=a.pos, mask=a.mask, out=a.out, scores=a.stash,
                         lse=a.lse)
        ops.importance_accumulate_prefill(a.acc, q, a.Kr, N, cos, sin, Pl, a.lse, causal=True, position_ids=a.pos)
        planes = ops.PQPlanes(1, 1, 1, d, DEV)
        planes.msb, planes.lsb, planes.scale = a.msb, a.lsb, a.scale
        ops.pq_pack(a.Kr, planes, 0, N)
        ops.attn_prefill_pq(q, planes, a.V, N, cos, sin, Pl, 1.0, causal=True, position_ids=a.pos, mask=a.mask, out=a.out_pq,
                            need_lsb=a.need)

    c.run(fn)


# ------------------------------------------------------------------------------------------------
# 7. importance and gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,ql", [("bf16", 1), ("bf16", 9), ("f32", 9)])
def test_importance_and_gather(dt, ql):
    """importance (out_sh through the C entry point: ops allocates its own output), row_lse, importance_accumulate with mask and
    causal, head_scores over a padded [B,q,H*d]; at q_len 1 also pv_gather with a padded kept-row list, with and without its
    workspace."""
    from spatten_amd import _lib, ops
    B, H, Hkv, d, L = 2, 4, 2, 128, 300
    tdt, P = TORCH_DT[dt], PADS["importance"]
    lib = _lib.load()
    mask = torch.zeros(B, ql, L, dtype=tdt, device=DEV)
    mask[:, :, 5::11] = torch.finfo(tdt).min
    c = Case().arg("stash", R(71, 0, (B, H, ql, L), dt), P["stash"]).arg("mask", mask, P["mask"])
    c.arg("acc", R(71, 1, (H, L), "f32"), P["acc"]).arg("imp", _full((H, L), 0.5, tdt), P["imp"])
    c.arg("out3", R(71, 2, (B, ql, H * d), dt), P["out3"]).arg("hs", _full((H,), 1.0, torch.float32), "flat")

    def fn(a):
        s = a.stash
        rc = lib.spatten_importance(_DTC[dt], s.data_ptr(), s.stride(0), s.stride(1), s.stride(2), a.imp.data_ptr(), a.imp.stride(0),
                                    B, H, ql, L, _stream())
        assert rc == 0
        lse = ops.row_lse(s, a.mask, causal=True)
        ops.importance_accumulate(a.acc, s, lse, mask=a.mask, causal=True)
        ops.head_scores(a.out3, H, a.hs)
        return lse

    c.run(fn)
    if ql != 1:
        return
    cap, k = 384, 90
    _, _, V, _, _ = _cache(B, Hkv, cap, d, dt, 72)
    stash3 = R(72, 0, (B, H, cap), dt)
    idx = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(u))[:k].sort().values for u in range(B * H)])
    mask2 = torch.zeros(B, L, dtype=tdt, device=DEV)
    mask2[:, 7::19] = torch.finfo(tdt).min
    for with_ws in (True, False):
        c = Case().arg("stash3", stash3, P["stash3"]).arg("mask2", mask2, P["mask2"]).arg("V", V, P["V"])
        c.arg("idx", idx.to(torch.int32).to(DEV), P["idx"]).arg("out", _full((B, H * d), 0.5, tdt), P["out"])
        c.arg("lse", _lse_of(stash3, L), "flat")

        def fn2(a):
            if with_ws:
                ops.pv_gather(a.stash3, a.lse, a.V, a.idx, mask=a.mask2, out=a.out)
            else:     # workspace NULL: one workgroup per (b, h)
                rc = lib.spatten_pv_gather(_DTC[dt], a.stash3.data_ptr(), a.stash3.stride(0), a.stash3.stride(1), a.lse.data_ptr(),
                                           a.mask2.data_ptr(), a.mask2.stride(0), a.V.data_ptr(), a.V.stride(0), a.V.stride(1),
                                           a.idx.data_ptr(), a.idx.stride(0), k, a.out.data_ptr(), a.out.stride(0), B, H, Hkv, d,
                                           None, 0, _stream())
                assert rc == 0

        c.run(fn2)


# ------------------------------------------------------------------------------------------------
# 8. prune
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_prune(dt):
    """topk_select (score_sh, idx_sh) and kv_compact (src and dst strides different, with the shadow) through the C entry points —
    ops allocates their outputs —, importance_compact, cascade_rank and gather_rows_i32 likewise; prune_layers over two layers of
    padded K / V / scores / destinations / accumulators."""
    from spatten_amd import _lib, ops
    B, H, d, L, lo, hi, k = 2, 4, 64, 96, 4, 80, 16
    tdt, P = TORCH_DT[dt], PADS["prune"]
    lib, code = _lib.load(), _DTC[dt]
    Lp = lo + k + (L - hi)
    cos, sin = ops.rope_table(L, d, tdt, DEV)
    i32 = lambda t: t.to(torch.int32).to(DEV)
    ids = i32(torch.stack([torch.randperm(400, generator=torch.Generator().manual_seed(h))[:L] for h in range(H)]))
    prev_ids = i32(torch.stack([ids[h].cpu()[torch.randperm(L, generator=torch.Generator().manual_seed(9 + h))[:24]].sort().values
                                for h in range(H)]))
    c = Case().arg("score", R(81, 0, (H, L), dt), P["score"]).arg("idx", _full((H, k), -7, torch.int32), P["idx"])
    c.arg("Ks", R(81, 1, (B, H, L, d), dt), P["Ks"]).arg("Vs", R(81, 2, (B, H, L, d), dt), P["Vs"])
    c.arg("Kd", _full((B, H, Lp + 8, d), 0.5, tdt), P["Kd"]).arg("Vd", _full((B, H, Lp + 8, d), 0.5, tdt), P["Vd"])
    c.arg("Krd", _full((B, H, Lp + 8, d), 0.5, tdt), P["Krd"])
    c.arg("acc", R(81, 3, (H, L), "f32"), P["acc"]).arg("acc_dst", _full((H, Lp + 8), 0.5, torch.float32), P["acc_dst"])
    c.arg("ids", ids, P["ids"]).arg("ids_dst", _full((H, Lp), -7, torch.int32), ((1, 64), ()))
    c.arg("prev_ids", prev_ids, P["prev_ids"]).arg("rank", _full((H, L), 0.5, torch.float32), P["rank"])

    def fn(a):
        st = _stream()
        assert lib.spatten_topk_select(code, a.score.data_ptr(), a.score.stride(0), H, lo, hi, k, a.idx.data_ptr(), a.idx.stride(0), st) == 0
        assert lib.spatten_kv_compact(code, a.Ks.data_ptr(), a.Vs.data_ptr(), a.Ks.stride(0), a.Ks.stride(1), a.Kd.data_ptr(),
                                      a.Vd.data_ptr(), a.Krd.data_ptr(), a.Kd.stride(0), a.Kd.stride(1), cos.data_ptr(), sin.data_ptr(),
                                      cos.shape[0], a.idx.data_ptr(), a.idx.stride(0), B, H, d, lo, k, hi, L - hi, st) == 0
        assert lib.spatten_importance_compact(a.acc.data_ptr(), a.acc.stride(0), a.acc_dst.data_ptr(), a.acc_dst.stride(0),
                                              a.idx.data_ptr(), a.idx.stride(0), H, lo, k, hi, L - hi, st) == 0
        # gather_rows_i32 is the same kernel over int32 rows
        assert lib.spatten_importance_compact(a.ids.data_ptr(), a.ids.stride(0), a.ids_dst.data_ptr(), a.ids_dst.stride(0),
                                              a.idx.data_ptr(), a.idx.stride(0), H, lo, k, hi, L - hi, st) == 0
        assert lib.spatten_cascade_rank(code, a.score.data_ptr(), a.score.stride(0), a.ids.data_ptr(), a.ids.stride(0),
                                        a.prev_ids.data_ptr(), a.prev_ids.stride(0), a.prev_ids.shape[1], a.rank.data_ptr(),
                                        a.rank.stride(0), H, L, st) == 0
        # the ops front ends on the same views (their outputs are their own allocations)
        return [ops.topk_select(a.score, lo, hi, k), ops.importance_compact(a.acc, a.idx, lo, hi, L),
                ops.cascade_rank(a.score, a.ids, a.prev_ids), ops.gather_rows_i32(a.ids, a.idx, lo, hi, L)]

    c.run(fn)

    nl = 2
    c = Case()
    for l in range(nl):
        first = l == 0
        e = lambda n: P[n] if first else P[n][0]
        c.arg(f"score{l}", R(82 + l, 0, (H, L), dt), e("score")).arg(f"Ks{l}", R(82 + l, 1, (B, H, L, d), dt), e("Ks"))
        c.arg(f"Vs{l}", R(82 + l, 2, (B, H, L, d), dt), P["Vs"])
        for n in ("Kd", "Vd", "Krd"):
            c.arg(f"{n}{l}", _full((B, H, Lp + 8, d), 0.5, tdt), e(n) if n == "Kd" else P[n])
        c.arg(f"acc{l}", R(82 + l, 3, (H, L), "f32"), e("acc")).arg(f"acc_dst{l}", _full((H, Lp + 8), 0.5, torch.float32), e("acc_dst"))
    c.arg("idx", _full((nl, H, k), -7, torch.int32), "flat")

    def fn_layers(a):
        g = lambda n: [getattr(a, f"{n}{l}") for l in range(nl)]
        ops.prune_layers(g("score"), g("Ks"), g("Vs"), L, lo, hi, k, dst=(g("Kd"), g("Vd"), g("Krd")), idx=a.idx, rope=(cos, sin),
                         acc=(g("acc"), g("acc_dst")))

    c.run(fn_layers)


# ------------------------------------------------------------------------------------------------
# 9. gemv
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_gemv(dt):
    """x, W and y padded at once (x_sm, w_sn, y_sm; x_sm and w_sn stay multiples of 8 as the header asks), M 2."""
    from spatten_amd import ops
    M, N, K = 2, 37, 520
    P = PADS["gemv"]
    c = Case().arg("x", R(91, 0, (M, K), dt), P["x"]).arg("W", R(91, 1, (N, K), dt, K ** -0.5), P["W"])
    c.arg("y", _full((M, N), 0.5, TORCH_DT[dt]), P["y"]).arg("bias", R(91, 2, (N,), dt), "flat")
    c.run(lambda a: ops.gemv(a.x, a.W, a.bias, out=a.y))
