"""CPU calibration of the exact-math criteria for progressive quantisation, local V pruning and cascade importance
(tests/pq_exact.py), and the evidence that they catch faults today's checks let through.

* the float64 references agree with the fp32 oracle at flat logits;
* the regimes of tests/regimes.py survive quantisation (asserted on the exact logits of the DEQUANTISED keys);
* the oracle's own errors sit well inside the calibrated bands (fp32 logit error, relative refetch-flag band);
* a numpy emulation of the PQ kernels' documented arithmetic passes every criterion in every regime;
* each seeded fault fails some criterion; ``OLD_CHECKS_CATCH`` records which of them the pre-existing checks (1e-4 absolute
  flag band, OUT_TOL outputs, stash within one 16-bit step, kept set against the kernel's own stash) let through."""
import functools
import math

import numpy as np
import pytest

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import regimes as rg
from tests.util import OUT_TOL

PROFILES = [(4, 8), (8, 8), (6, 6)]


@functools.lru_cache(maxsize=None)
def _pc(regime, kb, vb, dt="bf16", N=600, B=2, H=4, Hkv=4, d=128):
    return px.pq_case(B, H, Hkv, d, N, dt, regime, kb, vb)


def _thresholds(pc):
    """All heads refetch / none / about half (between two heads' exact p1max) / just above and just below head (0, 0)'s
    exact p1max, 2 tau away (both sides of the boundary, outside the band)."""
    p = np.sort(pc.p1max.ravel())
    i = p.size // 2
    tau = px.pq_exact(pc.qr, *pc.planes, 0.0).tau[0, 0]
    p0 = pc.p1max[0, 0]
    return (2.0, 0.0, float((p[i - 1] + p[i]) / 2), float(p0 * (1 + 2 * tau)), float(p0 * (1 - 2 * tau)))


# --------------------------------------------------------------------------------------------------------------------- #
# the references and the bands
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("kb,vb", PROFILES)
def test_exact_reference_agrees_with_the_oracle_at_flat_logits(kb, vb):
    pc = _pc("flat", kb, vb, Hkv=2)
    for thr in _thresholds(pc):
        ex = px.pq_exact(pc.qr, *pc.planes, thr)
        H = pc.H
        want, need, logits = orc.pq_decode_attention_profile(pc.qr, *[px._rep(x, H) for x in pc.planes], thr)
        assert np.array_equal(need, ex.flags)
        np.testing.assert_allclose(logits, ex.z, rtol=0, atol=2e-5)
        np.testing.assert_allclose(want, ex.out, rtol=1e-5, atol=1e-6)
        o2, l2 = px.pq_oracle(pc.qr, *pc.planes, need)
        assert np.array_equal(o2, want) and np.array_equal(l2, logits)


def test_prefill_reference_agrees_with_the_oracle():
    B, H, d, P, ql, dt = 1, 4, 64, 40, 24, "bf16"
    cs = rg.make_case(B, H, H, d, P, ql, dt, "sink8", 5, mask=orc.causal_mask(B, ql, P + ql, dt))
    msb, lsb, scale = orc.pq_quantize(cs.kr, bits=8)
    for thr in (0.0, 0.3, 2.0):
        want, need, pmax = orc.pq_prefill_attention(cs.qr, msb, lsb, scale, cs.vc, thr, P)
        ex, flags, p1 = px.pq_prefill_exact(cs.qr, msb, lsb, scale, cs.vc, thr, P)
        np.testing.assert_allclose(pmax, p1, rtol=1e-5)
        ok = px.decided(p1, thr, 1e-4)
        assert np.array_equal(need[ok], flags[ok])
        ex2, _, _ = px.pq_prefill_exact(cs.qr, msb, lsb, scale, cs.vc, thr, P, need=need)
        np.testing.assert_allclose(want, ex2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("regime", rg.REGIMES)
@pytest.mark.parametrize("kb,vb", PROFILES)
def test_regimes_survive_quantisation(regime, kb, vb):
    """pq_case asserts the regime on the exact logits of the dequantised keys (the ones the kernels see)."""
    pc = _pc(regime, kb, vb)
    if regime == "new_max":
        assert (pc.p1max > 0.999).all()


@pytest.mark.parametrize("regime", rg.REGIMES)
def test_calibration_of_the_bands(regime):
    """The fp32 oracle within a quarter of LOGIT_ERR's logit bound and of the flag band, at 600 and 2081 rows, 12 and 8
    MSB bits."""
    for kb, N in ((4, 2081), (8, 600), (6, 2081)):
        pc = _pc(regime, kb, 8, N=N)
        ex = px.pq_exact(pc.qr, *pc.planes, 2.0)
        B, H = pc.B, pc.H
        _, l1 = px.pq_oracle(pc.qr, *pc.planes, np.zeros((B, H), bool))
        _, l2 = px.pq_oracle(pc.qr, *pc.planes, np.ones((B, H), bool))
        bound = px.logit_err32(ex.absdot)
        assert (np.abs(l1 - ex.s1) <= bound / 4).all() and (np.abs(l2 - ex.s2) <= bound / 4).all()
        p1 = orc.softmax_probs(l1).max(-1)
        assert (np.abs(p1 - ex.p1max) <= ex.tau * ex.p1max / 4).all(), (np.abs(p1 - ex.p1max) / ex.p1max / ex.tau).max()
    # the band at unit-variance logits: < 1e-4 RELATIVE, i.e. ~1e-6 absolute at their p1max ~ 1e-2 (the old bar: 1e-4 absolute)
    pc = _pc("flat", 8, 8)
    assert pc.p1max.max() < 0.1 and px.pq_exact(pc.qr, *pc.planes, 0).tau.max() < 1e-4


# --------------------------------------------------------------------------------------------------------------------- #
# the criteria applied to an emulated kernel
# --------------------------------------------------------------------------------------------------------------------- #
def judge(pc, thr, keep=None, fault=None):
    """(new criteria hold, old checks hold) for the emulated kernel (with ``fault``) on case pc at threshold thr, full P.V
    (keep None) or local V over ``keep`` rows."""
    B, H, d, N, dt = pc.B, pc.H, pc.d, pc.N, pc.dt
    em = px.emulate_pq(pc.qr, *pc.planes, thr, dt, keep=keep, fault=fault)
    ex = px.pq_exact(pc.qr, *pc.planes, thr, need=em.need)
    o_out, o_lg = px.pq_oracle(pc.qr, *pc.planes, em.need)
    new, old = True, True
    # flags
    try:
        px.check_flags(em.need, ex.p1max, thr, ex.tau)
    except AssertionError:
        new = False
    o_flags = orc.softmax_probs(px.pq_oracle(pc.qr, *pc.planes, np.zeros((B, H), bool))[1]).max(-1)
    dec_old = np.abs(o_flags - thr) > 1e-4
    if not np.array_equal(em.need[dec_old], (o_flags < thr)[dec_old]):
        old = False
    same = em.need == (o_flags < thr)
    # stash (old bar: within one 16-bit step of the oracle's logits)
    tol = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 1e-6}[dt]
    if not np.all((np.abs(em.stash - o_lg) <= tol * np.maximum(np.abs(o_lg), 1.0) + 1e-6)[same]):
        old = False
    try:
        px.check_stash_exact(em.stash, ex.z, ex.absdot, dt)
    except AssertionError:
        new = False
    got = em.out.reshape(B, 1, H * d)
    if keep is None or keep >= N:
        want_old = orc.round_dt(orc.pq_decode_attention_profile(pc.qr, *[px._rep(x, H) for x in pc.planes], thr)[0], dt)
        if not np.allclose(em.out[same], want_old[same], **OUT_TOL[dt]):
            old = False
        try:
            rg.check_out_exact(got, orc.round_dt(o_out, dt).reshape(B, 1, H * d), ex.out.reshape(B, 1, H * d), dt, d)
        except AssertionError:
            new = False
        return new, old
    probs = orc.softmax_probs(o_lg)
    V32 = (px._rep(pc.planes[3], H).astype(np.float32) * px._rep(pc.planes[4], H))
    ref_o = np.zeros((B, H, d), np.float32)
    ref_x = np.zeros((B, H, d))
    slack = np.zeros((B, 1, H))
    for b in range(B):
        for h in range(H):
            k_ = em.kept[b, h]
            if not np.array_equal(np.sort(k_), orc.topk_window(em.stash[b, h:h + 1], 0, N, keep)[0]):
                old = False
            try:
                px.check_kept(k_, N, keep, ex.z[b, h], px.logit_err32(ex.absdot[b, h]), dt, stash=em.stash[b, h])
            except AssertionError:
                new = False
            ref_o[b, h] = probs[b, h, k_] @ V32[b, h, k_]
            ref_x[b, h] = px.local_v_exact(ex.p[b, h], ex.V[b, h], k_)
            slack[b, 0, h] = px.local_v_slack(ex.p[b, h], ex.V[b, h], k_, px.logit_err32(ex.absdot[b, h]))
    if not np.allclose(em.out, orc.round_dt(ref_o, dt), **OUT_TOL[dt]):
        old = False
    try:
        px.check_out_exact_slack(got, orc.round_dt(ref_o, dt).reshape(B, 1, H * d), ref_x.reshape(B, 1, H * d), slack, dt, d)
    except AssertionError:
        new = False
    return new, old


def _cascade_case(regime, kb, dt, T=8, N0=300, fault=None):
    """T decode steps over a growing cache (the query moves, one row more each step), thresholds alternating so the flagged
    set changes.  Returns (new holds, old holds)."""
    pc = _pc(regime, kb, 8, dt=dt, N=N0 + T)
    B, H = pc.B, pc.H
    rows, ex_sum, or_sum = [], np.zeros((H, pc.N)), np.zeros((H, pc.N), np.float32)
    for t in range(T):
        n = N0 + 1 + t
        pl = [x[:, :, :n] for x in pc.planes]
        qr = orc.round_dt(pc.qr * np.float32(1.0 + 0.05 * t), dt)
        thr = 2.0 if t % 3 == 0 else (0.0 if t % 3 == 1 else float(np.median(px.pq_exact(qr, *pl, 0).p1max)))
        em = px.emulate_pq(qr, *pl, thr, dt)
        ex = px.pq_exact(qr, *pl, thr, need=em.need)
        _, o_lg = px.pq_oracle(qr, *pl, em.need)
        rows.append(em.z)
        ex_sum[:, :n] += ex.p.sum(0)
        or_sum[:, :n] = (or_sum[:, :n] + orc.softmax_probs(o_lg).sum(0, dtype=np.float32)).astype(np.float32)
    acc = px.emulate_cascade(rows, fault=fault)
    try:
        px.check_cascade(acc, or_sum, ex_sum, T)
        new = True
    except AssertionError:
        new = False
    old = np.allclose(acc, or_sum, atol=2e-6, rtol=1e-4)
    return new, old


@pytest.mark.parametrize("regime", rg.REGIMES)
@pytest.mark.parametrize("kb,vb", PROFILES)
def test_emulated_kernel_passes_every_criterion(regime, kb, vb):
    pc = _pc(regime, kb, vb)
    for thr in _thresholds(pc):
        assert judge(pc, thr) == (True, True), (thr, "full")
        for keep in (1, 37, pc.N - 1, pc.N):
            assert judge(pc, thr, keep)[0], (thr, keep)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("regime", ["flat", "sink24", "rising", "large12", "split_winner"])
def test_emulated_kernel_passes_every_criterion_other_dtypes(dt, regime):
    pc = _pc(regime, 8, 8, dt=dt, d=64, Hkv=2)
    for thr in _thresholds(pc):
        assert judge(pc, thr)[0], thr
        for keep in (1, 150, pc.N - 1):
            assert judge(pc, thr, keep)[0], (thr, keep)


@pytest.mark.parametrize("regime", ["flat", "sink24", "rising", "large12"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_emulated_cascade_passes(regime, dt):
    assert _cascade_case(regime, 8, dt) == (True, True)


# --------------------------------------------------------------------------------------------------------------------- #
# seeded faults
# --------------------------------------------------------------------------------------------------------------------- #
# does a pre-existing check fail somewhere at the flat logits and (8, 8) planes the old tests use?  False = the old checks
# let the fault through
OLD_CHECKS_CATCH = {
    "gather_msb_logits": False,          # moves a flat (8, 8) output by < OUT_TOL; the stash is right (pass 2 wrote it)
    "flag_rounded_row": False,           # p1max off by ~1e-3 relative: inside the 1e-4 absolute band at p1max ~ 1e-2
    "flag_split_partial": True,
    "lsb_no_scale": True,
    "lsb_neighbour_scale": True,         # (by the stash alone: the flat output moves by less than an ulp)
    "vscale_prev_row": True,
    "renormalise_kept": True,
    "kept_per_split": True,
    "kept_without_new_row": True,
    "fold_prev_twice": True,
    "flush_skips_last": True,
}

_SWEEP = [("flat", 6, 6), ("flat", 8, 8), ("flat", 4, 8), ("sink24", 8, 8), ("rising", 6, 6), ("large12", 4, 8),
          ("new_max", 8, 8), ("split_winner", 6, 6), ("large4", 8, 8)]


def _fault_sweep(fault):
    """(some new criterion fails somewhere in _SWEEP, some old check fails at flat logits)."""
    new_fail = old_fail = False
    if fault in px.CASCADE_FAULTS:
        for regime in ("flat", "sink24", "large12"):
            kb = 8
            n, o = _cascade_case(regime, kb, "bf16", fault=fault)
            new_fail |= not n
            old_fail |= not o and (regime, kb) == ("flat", 8)
        return new_fail, old_fail
    local = fault in ("renormalise_kept", "kept_per_split", "kept_without_new_row")
    for regime, kb, vb in _SWEEP:
        pc = _pc(regime, kb, vb)
        for thr in _thresholds(pc):
            if local:
                for keep in (1, 37, 300):
                    n, o = judge(pc, thr, keep, fault)
                    new_fail |= not n
                    old_fail |= not o and (regime, kb) == ("flat", 8)
            else:
                n, o = judge(pc, thr, None, fault)
                new_fail |= not n
                old_fail |= not o and (regime, kb) == ("flat", 8)
    return new_fail, old_fail


@pytest.mark.parametrize("fault", px.FAULTS + px.CASCADE_FAULTS)
def test_seeded_fault_fails_the_new_criteria(fault):
    new_fail, old_fail = _fault_sweep(fault)
    assert new_fail, f"{fault}: passes every new criterion"
    assert old_fail == OLD_CHECKS_CATCH[fault], f"{fault}: old checks {'catch' if old_fail else 'let through'} it"
