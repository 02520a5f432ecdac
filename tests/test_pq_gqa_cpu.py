"""CPU side of the grouped quantised-query decode (spatten_attn_decode_pq_qint_gqa): the host rule, the option conflicts of the
Python layers, the documented P.V arithmetic (hi + lo bf16 weights on the bf16 matrix cores) under the unchanged criteria of
tests/pq_qint_exact.py — and the evidence that the criterion tells it from a single bf16 weight —, and the threshold condition the
GPU test starts from.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import pq_qint_exact as qx
from tests import regimes as rg
from tests.test_pq_qint_cpu import case, case_thresholds

# The grouped grid (shared with tests/test_gpu_pq_gqa.py): every regime at d = 128, profile (8, 8), N = 600, B = 2; dtype, the
# (H, Hkv) pair and query_bits rotate through the regimes so that every value of each meets every value of the others' pairs
# over the grid (a covering design, as tests/test_pq_qint_cpu.py's: the full product is 108 cases of float64 reference work)
_DT_HEADS_BITS = [("bf16", 8, 1, 8), ("f16", 8, 2, 5), ("bf16", 8, 4, 5), ("f16", 8, 1, 5), ("bf16", 8, 2, 8), ("f16", 8, 4, 8),
                  ("f16", 8, 1, 8), ("bf16", 8, 2, 5), ("f16", 8, 4, 5), ("bf16", 8, 1, 5), ("f16", 8, 2, 8), ("bf16", 8, 4, 8)]
GRID = [(r,) + _DT_HEADS_BITS[i % len(_DT_HEADS_BITS)] for i, r in enumerate(rg.REGIMES)]
GRID_IDS = [f"{r}-{dt}-h{H}-hkv{Hkv}-q{bits}" for r, dt, H, Hkv, bits in GRID]

F32, F16, BF16 = 0, 1, 2


def test_supported_rule_without_a_gpu():
    from spatten_amd import _lib
    lib = _lib.load()
    sup = lib.spatten_pq_qint_gqa_supported
    # every accepted corner
    for dt in (F16, BF16):
        for heads, kv in ((2, 1), (8, 4), (32, 8), (64, 8), (32, 1), (64, 2)):
            for qb in (4, 8):
                assert sup(dt, heads, kv, 128, 8, 8, qb) == 1, (dt, heads, kv, qb)
    # every documented refusal
    assert sup(F32, 32, 8, 128, 8, 8, 8) == 0                       # fp32 model dtype
    assert sup(BF16, 8, 8, 128, 8, 8, 8) == 0                       # heads == kv_heads: nothing to group
    assert sup(BF16, 33, 1, 128, 8, 8, 8) == 0                      # a group beyond the 32 columns of one B operand
    assert sup(BF16, 66, 2, 128, 8, 8, 8) == 0
    assert sup(BF16, 9, 2, 128, 8, 8, 8) == 0                       # heads not a multiple of kv_heads
    assert sup(BF16, 32, 8, 64, 8, 8, 8) == 0                       # head_dim 64
    assert sup(BF16, 32, 8, 256, 8, 8, 8) == 0
    assert sup(BF16, 32, 8, 128, 4, 8, 8) == 0                      # profile (4, 8)
    assert sup(BF16, 32, 8, 128, 6, 6, 8) == 0                      # profile (6, 6)
    assert sup(BF16, 32, 8, 128, 8, 6, 8) == 0
    assert sup(BF16, 32, 8, 128, 8, 8, 3) == 0 and sup(BF16, 32, 8, 128, 8, 8, 9) == 0
    assert sup(BF16, 0, 0, 128, 8, 8, 8) == 0 and sup(BF16, 8, -2, 128, 8, 8, 8) == 0
    # the whole rule, swept
    for dt in (F32, F16, BF16):
        for heads in (1, 2, 8, 12, 32, 64, 66):
            for kv in (1, 2, 8):
                for d in (64, 128):
                    for kb, vb in ((8, 8), (4, 8), (6, 6)):
                        for qb in (3, 4, 8, 9):
                            g = heads // kv if heads % kv == 0 else 0
                            want = dt in (F16, BF16) and 2 <= g <= 32 and d == 128 and (kb, vb) == (8, 8) and 4 <= qb <= 8
                            assert sup(dt, heads, kv, d, kb, vb, qb) == int(want), (dt, heads, kv, d, kb, vb, qb)
    # argument validation happens before anything touches a device
    a = _lib.PQQintArgs()
    call = lib.spatten_attn_decode_pq_qint_gqa
    assert call(None, None) == -1
    assert call(ctypes.byref(a), None) == -1                         # struct_size 0
    a.struct_size, a.query_bits = ctypes.sizeof(_lib.PQQintArgs), 8
    assert call(ctypes.byref(a), None) == -1                         # NULL outputs
    buf = (ctypes.c_char * 64)()
    a.q_int = a.q_scale = ctypes.addressof(buf)
    a.query_bits = 9
    assert call(ctypes.byref(a), None) == -1                         # query_bits outside [4, 8]


def test_abi_declares_the_grouped_entry_points():
    from tests.test_abi_exports import declared_functions
    names = declared_functions()
    assert "spatten_attn_decode_pq_qint_gqa" in names and "spatten_pq_qint_gqa_supported" in names


def test_ops_rule_and_option_conflicts():
    import torch

    from spatten_amd import ops
    from spatten_amd.extensions import SpattenExtensions
    assert ops.pq_qint_gqa_supported(torch.bfloat16, 32, 8, 128, 8, 8, 8)
    assert not ops.pq_qint_gqa_supported(torch.float32, 32, 8, 128, 8, 8, 8)
    assert not ops.pq_qint_gqa_supported(torch.float16, 8, 8, 128, 8, 8, 8)
    assert not ops.pq_qint_gqa_supported(torch.float16, 32, 8, 64, 8, 8, 8)
    with pytest.raises(ValueError, match="query_bits"):                  # grouped is a form of the quantised-query decode
        ops.attn_decode_pqv(None, None, 1, None, None, 0, 0.5, grouped=True)
    cache = type("C", (), {"important_size": 8})()
    ok = dict(pq_threshold=0.1, pq_profile=(8, 8), pq_query_bits=8, pq_grouped=True)
    assert SpattenExtensions(cache, 2, **ok).pq_grouped is True
    assert SpattenExtensions(cache, 2, pq_threshold=0.1, pq_profile=(8, 8), pq_query_bits=8).pq_grouped is False
    for bad in (dict(ok, pq_query_bits=None), dict(ok, pq_profile=(4, 8)), dict(ok, pq_profile=None), dict(ok, head_keep=4),
                dict(ok, local_v_keep=0.5)):
        with pytest.raises(ValueError):
            SpattenExtensions(cache, 2, **bad)


def emulate_gqa_out(pc, bits, thr, lo_term=True):
    """The documented grouped arithmetic on top of qx.emulate_qint's logits and flags: e_j = exp(z_j - m) (fp32), w_j = e_j
    val_scale_j (fp32), hi = bf16(w), lo = bf16(w - hi); out = (sum_j hi_j qv_j + sum_j lo_j qv_j) / l — exact products (an 8-bit qv
    and a bf16 weight: 16 significant bits), fp32 sums —, rounded to the model dtype.  ``lo_term=False``: the single-bf16-weight
    variant."""
    f32 = np.float32
    em = qx.emulate_qint(pc.qr, pc.planes, thr, pc.dt, bits, kb=pc.kb, q_unrotated=pc.cs.q[:, :, 0])
    H = pc.qr.shape[1]
    qv, vscale = px._rep(pc.planes[3], H), px._rep(pc.planes[4], H)
    m, l = px._softmax32(em.z)
    e = np.exp(em.z - m).astype(f32)
    w = (e * vscale[..., 0].astype(f32)).astype(f32)
    hi = orc.round_dt(w, "bf16").astype(f32)
    lo = orc.round_dt((w - hi).astype(f32), "bf16").astype(f32)
    acc = np.einsum("bhl,bhld->bhd", hi, qv.astype(f32)).astype(f32)
    if lo_term:
        acc = (acc + np.einsum("bhl,bhld->bhd", lo, qv.astype(f32)).astype(f32)).astype(f32)
    out = (acc / l.astype(f32)).astype(f32)
    return SimpleNamespace(q_int=em.q_int, q_scale=em.q_scale, msb_logit=em.msb_logit, z=em.z, stash=em.stash, need=em.need,
                           out=orc.round_dt(out, pc.dt))


def _out_passes(pc, bits, thr, **kw):
    try:
        qx.check_step(pc.qr, pc.planes, pc.dt, bits, thr, emulate_gqa_out(pc, bits, thr, **kw), only=("out",))
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("regime,dt,H,Hkv,bits", GRID, ids=GRID_IDS)
def test_hi_lo_weights_pass_the_output_criterion_and_thresholds_are_decided(regime, dt, H, Hkv, bits):
    pc = case(regime, 8, 8, dt, 128, Hkv, H=H)
    ths, ex0 = case_thresholds(pc, bits)
    for thr in ths:
        # the threshold condition: picked from the exact p1max alone, at most BAND_CAP of the heads inside the band
        assert qx.band_share(ex0, thr) <= px.BAND_CAP, (regime, thr)
        res = emulate_gqa_out(pc, bits, thr)
        qx.check_step(pc.qr, pc.planes, pc.dt, bits, thr, res, name=f"{regime} thr={thr!r}")


def test_a_single_bf16_weight_is_caught_in_f16():
    """The criterion tells the documented hi + lo pair from one bf16 weight (2^-9 relative per term): in an f16 model the
    single weight fails it on the grid, the pair passes everywhere."""
    caught = 0
    for regime, dt, H, Hkv, bits in GRID:
        if dt != "f16":
            continue
        pc = case(regime, 8, 8, dt, 128, Hkv, H=H)
        for thr in case_thresholds(pc, bits)[0]:
            assert _out_passes(pc, bits, thr), (regime, thr)
            caught += not _out_passes(pc, bits, thr, lo_term=False)
    assert caught > 0
