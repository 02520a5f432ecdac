"""CPU calibration of the exact-math criteria for the PQ-keyed prefill and the stash-free prefill importance
(tests/pq_exact.py), and the evidence that they catch faults today's checks let through.

* the vectorised float64 reference equals the per-row loop it replaced and agrees with the oracle at flat logits; the
  vectorised fp32 oracle equals orc.pq_prefill_attention where both are defined;
* the prefill regimes of tests/regimes.py survive 8-bit quantisation (asserted on the exact logits s2);
* numpy emulations of the two kernels' documented arithmetic pass EVERY criterion of tests/test_gpu_pq_prefill_regimes.py in
  every regime, bf16 and f16, d 64 and 128, Hkv < H, with and without a mask (the worst margin per criterion is printed);
* each seeded fault fails some criterion; ``OLD_CHECKS_CATCH`` records which of them the pre-existing checks (1e-4 absolute
  flag band, OUT_TOL on the rows decided alike, rtol 1e-2 / atol 2e-3 against the own stash, the row-sum rule) let through."""
import functools
import math

import numpy as np
import pytest

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import regimes as rg
from tests.util import OUT_TOL

PREFILL_REGIMES = tuple(r for r in rg.REGIMES if r not in rg.DECODE_ONLY)
# name -> (B, H, Hkv, d, P, ql, masked): one key range in pass 2 / the key-split pass (N >= 2048) / an explicit mask
SHAPES = {"unsplit": (1, 4, 4, 128, 300, 200, False), "split": (1, 4, 4, 64, 1900, 200, False),
          "masked": (2, 4, 2, 128, 300, 200, True), "gqa8": (1, 8, 1, 64, 140, 120, False)}


@functools.lru_cache(maxsize=None)
def _pc(shape, regime, dt):
    B, H, Hkv, d, P, ql, masked = SHAPES[shape]
    mask = rg.prefill_mask(B, ql, P + ql, dt, [0, 13][:B], 100, 228) if masked else None
    return px.prefill_case(B, H, Hkv, d, P, ql, dt, regime, mask=mask)


def _thresholds(pc):
    """The GPU test's thresholds + one that flags ~15 % of the rows (under a quarter: the key-split form where N allows)."""
    p = np.sort(pc.ex0.p1max.ravel())
    i = int(0.15 * p.size)
    return px.prefill_thresholds(pc.ex0) + [float((p[i] + p[i + 1]) / 2)]


def _loop_reference(qr, msb, lsb, scale, V, thr, past_len, need=None):
    """The per-row float64 loop pq_prefill_exact was before it was vectorised."""
    B, H, ql, d = qr.shape
    sc = px._rep(scale, H).astype(np.float64)
    m16 = 16.0 * px._rep(msb, H).astype(np.float64)
    k1, k2 = m16 * sc, (m16 + px._rep(lsb, H).astype(np.float64)) * sc
    V64 = px._rep(V, H).astype(np.float64)
    out = np.zeros((B, ql, H, d))
    flags = np.zeros((B, H, ql), bool)
    p1max = np.zeros((B, H, ql))
    for i in range(ql):
        vis = past_len + i + 1
        qi = np.asarray(qr[:, :, i], np.float64)
        s1 = np.einsum("bhd,bhld->bhl", qi, k1[:, :, :vis]) / math.sqrt(d)
        s2 = np.einsum("bhd,bhld->bhl", qi, k2[:, :, :vis]) / math.sqrt(d)
        p1max[:, :, i] = 1.0 / np.exp(s1 - s1.max(-1, keepdims=True)).sum(-1)
        flags[:, :, i] = p1max[:, :, i] < thr
        use = flags[:, :, i] if need is None else np.asarray(need, bool)[:, :, i]
        out[:, i] = np.einsum("bhl,bhld->bhd", px._softmax64(np.where(use[..., None], s2, s1)), V64[:, :, :vis])
    return out.reshape(B, ql, H * d), flags, p1max


# --------------------------------------------------------------------------------------------------------------------- #
# the references
# --------------------------------------------------------------------------------------------------------------------- #
def test_vectorised_reference_equals_the_row_loop_and_the_oracle():
    pc = _pc("gqa8", "flat", "bf16")
    for thr in (0.0, float(np.median(pc.ex0.p1max)), 2.0):
        o, f, p1 = px.pq_prefill_exact(pc.qr, *pc.planes, pc.V, thr, pc.P)
        o2, f2, p2 = _loop_reference(pc.qr, *pc.planes, pc.V, thr, pc.P)
        assert np.array_equal(f, f2)
        np.testing.assert_allclose(p1, p2, rtol=1e-12)
        np.testing.assert_allclose(o, o2, rtol=0, atol=1e-13)
        rep = [px._rep(x, pc.H) for x in pc.planes]
        want, need, pmax = orc.pq_prefill_attention(pc.qr, *rep, px._rep(pc.V, pc.H), thr, pc.P)
        np.testing.assert_allclose(pmax, p1, rtol=1e-5)
        ok = px.decided(p1, thr, 1e-4)
        assert np.array_equal(need[ok], f[ok])
        ex2 = px.prefill_exact(pc, thr, need=need)
        np.testing.assert_allclose(want, ex2.out, rtol=1e-4, atol=1e-5)
        # the vectorised fp32 oracle against the per-row one: fp32 summation order only
        np.testing.assert_allclose(px.pq_prefill_oracle(pc.qr, *pc.planes, pc.V, need, pc.P), want, rtol=0, atol=3e-6)


def test_reference_mask_and_causal_off():
    """A causal mask given explicitly = the causal flag; fully masked rows are the uniform average, as rg.attention_exact
    defines them; causal=False sees every key."""
    pc = _pc("masked", "sink8", "bf16")
    B, ql, N = pc.B, pc.ql, pc.N
    a = px.pq_prefill_exact(pc.qr, *pc.planes, pc.V, 0.1, pc.P, full=True)
    b = px.pq_prefill_exact(pc.qr, *pc.planes, pc.V, 0.1, pc.P, mask=orc.causal_mask(B, ql, N, pc.dt)[:, 0], causal=False, full=True)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.flags, b.flags)
    ex = px.prefill_exact(pc, 0.0)
    want = px._rep(pc.V, pc.H).astype(np.float64).mean(2)                              # [B,H,d]
    np.testing.assert_allclose(ex.out[1, :13].reshape(13, pc.H, pc.d), np.broadcast_to(want[1], (13, pc.H, pc.d)), rtol=1e-12)
    np.testing.assert_allclose(ex.p1max[1, :, :13], 1.0 / N)
    c = px.pq_prefill_exact(pc.qr, *pc.planes, pc.V, 0.0, pc.P, causal=False, full=True)
    assert c.vis.all() and np.isfinite(c.out).all()


@pytest.mark.parametrize("regime", PREFILL_REGIMES)
@pytest.mark.parametrize("shape", ["unsplit", "split"])
def test_prefill_regimes_survive_quantisation(shape, regime):
    """prefill_case asserts the regime on the exact logits of the dequantised keys (the ones the kernel sees)."""
    _pc(shape, regime, "bf16")


# --------------------------------------------------------------------------------------------------------------------- #
# the criteria applied to the emulated kernels
# --------------------------------------------------------------------------------------------------------------------- #
def judge(pc, thr, fault=None, stats=None):
    """(new criteria hold, old checks hold) for the emulated PQ prefill (with ``fault``) on case pc at threshold thr."""
    em = px.emulate_pq_prefill(pc.qr, *pc.planes, pc.V, thr, pc.P, pc.dt, mask=pc.mask, causal=pc.causal, fault=fault)
    new = old = True
    if not np.isfinite(em.out).all():
        return False, False
    try:
        px.check_pq_prefill(pc, thr, em.out, em.need, stats=stats)
    except AssertionError:
        new = False
    # today's checks (tests/test_gpu_fullsize.py): absolute flag band, OUT_TOL on the rows decided alike in every head
    ex = px.prefill_exact(pc, thr)
    o_need = ex.flags
    clear = np.abs(ex.p1max - thr) > 1e-4 * max(thr, 1e-3)
    if not np.array_equal(em.need[clear], o_need[clear]):
        old = False
    ok_rows = clear.all(axis=1)
    want = orc.round_dt(px.pq_prefill_oracle(pc.qr, *pc.planes, pc.V, o_need, pc.P, pc.mask, pc.causal, pc.dt), pc.dt)
    sh = (pc.B, pc.ql, pc.H, pc.d)
    if not np.allclose(em.out.reshape(sh)[ok_rows], want.reshape(sh)[ok_rows], **OUT_TOL[pc.dt]):
        old = False
    return new, old


def judge_colprob(cs, causal=True, fault=None, stats=None):
    acc, m, l = px.emulate_colprob(cs, causal, fault)
    new = old = True
    try:
        px.check_colprob(acc, cs, causal, stats=stats)
    except AssertionError:
        new = False
    # today's checks (tests/test_gpu_cascade.py): rtol 1e-2 / atol 2e-3 against the fault-free sum over the OWN logits, row sums
    own = px.emulate_colprob(cs, causal, None)[0]
    if not np.allclose(acc, own, rtol=1e-2, atol=2e-3) or not np.allclose(acc.sum(1), cs.B * cs.ql, rtol=1e-3):
        old = False
    return new, old


STATS = {}


@pytest.mark.parametrize("regime", PREFILL_REGIMES)
@pytest.mark.parametrize("shape,dt", [("unsplit", "bf16"), ("unsplit", "f16"), ("split", "bf16"), ("split", "f16"),
                                      ("masked", "bf16"), ("masked", "f16"), ("gqa8", "bf16")])
def test_emulated_pq_prefill_passes_every_criterion(shape, dt, regime):
    pc = _pc(shape, regime, dt)
    st = STATS.setdefault("pq prefill", {})
    for thr in _thresholds(pc):
        if px.band_share(pc.ex0, thr) > px.BAND_CAP:
            continue              # (the GPU test asserts the cap for its own parametrisations; here: a threshold of no use)
        new, _ = judge(pc, thr, stats=st)
        assert new, (shape, dt, regime, thr)
    print(f"\nemulated PQ prefill {shape} {dt} {regime}: worst err / allowance so far {st.get('out', 0):.3f}, "
          f"largest undecided share {st.get('band', 0):.4f}")


@functools.lru_cache(maxsize=None)
def _cs(regime, dt, causal=True, B=2, H=4, Hkv=2, d=128, P=200, ql=300):
    return rg.make_case(B, H, Hkv, d, P, ql, dt, regime, 23, mask=orc.causal_mask(B, ql, P + ql, dt) if causal else None)


@pytest.mark.parametrize("regime", ["flat", "sink24", "rising", "large12", "split_winner"])
@pytest.mark.parametrize("dt,d", [("bf16", 128), ("f16", 64)])
def test_emulated_colprob_passes_every_criterion(dt, d, regime):
    st = STATS.setdefault("importance", {})
    assert judge_colprob(_cs(regime, dt, d=d), stats=st)[0]
    assert judge_colprob(_cs(regime, dt, causal=False, d=d), causal=False, stats=st)[0]
    print(f"\nemulated prefill importance {dt} {regime}: worst err / allowance so far {st['importance']:.3f}")


def test_row_statistics_of_the_emulation_are_a_deferred_maximum():
    cs = _cs("rising", "bf16")
    _, m, l = px.emulate_colprob(cs)
    true = np.where(px.prefill_visibility(cs.B, cs.ql, cs.N, cs.P, True, None, cs.dt)[0], cs.stash, -np.inf).max(-1)
    assert (m <= true).all() and (m >= true - rg.DEFER_MAX).all() and (m < true).any()


# --------------------------------------------------------------------------------------------------------------------- #
# seeded faults
# --------------------------------------------------------------------------------------------------------------------- #
# does a pre-existing check fail at the flat logits and the shapes the old tests use (no mask, Hkv = H, causal)?
# False = the old checks let the fault through
OLD_CHECKS_CATCH = {
    "flag_from_run_max": True,           # (at the median threshold: the running maximum lags the true one in most flat rows)
    "flag_before_last_tile": True,
    "scale_of_previous_tile": True,
    "pass2_keeps_pass1_stats": True,
    "pass2_drops_last_range": False,     # the old thresholds (0, all, median) flag none or > 1/4 of a head: never the split pass
    "merge_stale_max": False,            # flat logits: a range's first-tile maximum is within e^8 of its last
    "causal_off_by_one": True,
    "kv_head_of_query_head": False,      # every old test builds K with H heads
    "mask_row_of_neighbour": False,      # no old test passes a mask
    "mask_add_rounded": False,           # (the parent commit's kernel: logit + mask rounded to the model dtype under a mask)
    "diag_off_by_one": True,
    "last_query_tile_dropped": True,
    "stats_of_neighbour_row": True,
    "first_q_clamped_wrong": True,
    "batch_row_0_only": True,
}

_SWEEP = [("unsplit", "flat", "bf16"), ("split", "flat", "bf16"), ("unsplit", "rising", "bf16"), ("split", "rising", "bf16"),
          ("split", "sink24", "f16"), ("split", "large12", "bf16"), ("masked", "sink8", "bf16"), ("masked", "flat", "f16"),
          ("gqa8", "flat", "bf16"), ("split", "split_winner", "bf16")]


def _fault_sweep(fault):
    """(some new criterion fails somewhere in the sweep, some old check fails at flat logits on the old tests' inputs)."""
    new_fail = old_fail = False
    if fault in px.COLPROB_FAULTS:
        for regime in ("flat", "rising", "sink24", "large12"):
            n, o = judge_colprob(_cs(regime, "bf16", P=300, ql=300), fault=fault)
            new_fail |= not n
            old_fail |= not o and regime == "flat"
        return new_fail, old_fail
    for shape, regime, dt in _SWEEP:
        pc = _pc(shape, regime, dt)
        for thr in _thresholds(pc):
            if px.band_share(pc.ex0, thr) > px.BAND_CAP:
                continue
            n, o = judge(pc, thr, fault)
            new_fail |= not n
            old_fail |= not o and regime == "flat" and shape in ("unsplit", "split") and thr in _thresholds(pc)[:4:2] + _thresholds(pc)[3:4]
    return new_fail, old_fail


@pytest.mark.parametrize("fault", px.PREFILL_FAULTS + px.COLPROB_FAULTS)
def test_seeded_fault_fails_the_new_criteria(fault):
    new_fail, old_fail = _fault_sweep(fault)
    assert new_fail, f"{fault}: passes every new criterion"
    assert old_fail == OLD_CHECKS_CATCH[fault], f"{fault}: old checks {'catch' if old_fail else 'let through'} it"
