"""Progressive quantisation, local V pruning and cascade importance against EXACT math (test infrastructure; may import
oracle/).

The oracle's PQ / local V / cascade functions are restatements (PARITY UNPINNED): comparing a kernel with them
at a fixed tolerance lets faults through whose effect is smaller than OUT_TOL (a gather that ignores the refetch moves a
(6,6) output by 0.0066 against |out| <= 0.23).  This module judges the kernels against float64 math over the planes the
kernels read (bit exact to orc.pq_quantize / orc.pq_quantize_values, so the dequantisation is exact):

* ``pq_exact``: k1 = 16 msb scale, k2 = (16 msb + lsb) scale, s1 / s2 = q.k / sqrt(d), the exact pass-1 max probability,
  the exact refetch flags, the final logits of a given decision, the probabilities and out = p . (qv vscale);
* ``check_flags``: need_lsb equals the exact flag wherever |p1max - thr| > tau p1max (``flag_band``: tau from the fp32
  logit error bound of the head, ~6e-5 at unit-variance logits);
* ``check_stash_exact``: the stash within 1 ulp of the dtype + the fp32 logit bound of the exact final logits;
* ``check_kept``: no dropped row's exact logit above the smallest kept one's by more than ``kept_delta``; exact ties lowest
  index first;
* ``check_cascade``: per head, max |acc - sum_t p_t| <= C max |acc_oracle - sum_t p_t| + T ulp_f32;
* outputs through ``regimes.check_out_exact`` (err <= C err(oracle) + 1 ulp); local V outputs in addition with the fp32
  logit error bound carried through the kept rows (``local_v_slack``);
* ``emulate_pq`` / ``emulate_cascade``: numpy restatement of the kernels' documented arithmetic with switchable faults —
  the CPU calibration of LOGIT_ERR / the flag band and the evidence that the criteria catch what today's checks let through
  (tests/test_pq_exact_cpu.py).
"""
import math
from types import SimpleNamespace

import numpy as np

from oracle import spatten_oracle as orc
from tests import regimes as rg

# fp32 logit error: |s_fp32 - s| <= LOGIT_ERR 2^-24 sum_i |q_i k_i| / sqrt(d).  The oracle stays below 4.1 in every regime
# (test_calibration_of_the_bands); the kernels sum offset-binary fields, q_i (m_i + 2^(KB-1)), and take the bias out through
# sum_i q_i: measured up to 22 on the GPU ((4, 8) planes, f16, split_winner), so 2x that
LOGIT_ERR = 48.0
# Refetch-flag band, relative to the pass-1 max probability, per head: p1max = 1 / sum_j exp(s_j - max) moves by the error of
# the logit differences (twice the fp32 logit bound at the head's largest sum |q_i k_i|) plus the rounding of the exps and
# their sum (TAU_FLOOR).  The oracle's own p1max stays within a quarter of it (8e-6 relative at the rising regime's logits
# of ~90, 4e-7 at flat ones, where tau is ~6e-5).  The old bar, 1e-4 ABSOLUTE, is a 10 % band at the p1max ~ 1e-3 of flat heads
TAU_FLOOR = 2.0 ** -18
# cascade importance is an fp32 sum of exp of fp32 logits in every form (the PQ planes' logits are fp32 whatever the model
# dtype): the f32 allowance of DESIGN §4 (the exp argument's ~|s| 2^-24 error the oracle's exp(s - m) does not have)
C_CASCADE = rg.C_EXACT_F32

EPS32 = 2.0 ** -24


# --------------------------------------------------------------------------------------------------------------------- #
# exact references
# --------------------------------------------------------------------------------------------------------------------- #
def _rep(x, H):
    return orc.repeat_kv(np.asarray(x), H // x.shape[1])


def _softmax64(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def pq_exact(qr, msb, lsb, scale, qv, vscale, thr, need=None):
    """Float64 progressive-quant decode.  qr [B,H,d] rotated (dtype-rounded) queries; msb / lsb [B,Hkv,N,d] integer planes,
    scale [B,Hkv,N,1], qv [B,Hkv,N,d], vscale [B,Hkv,N,1] (repeated for Hkv < H).  ``need`` [B,H] bool: the decision to
    evaluate (the kernel's); None = the exact flags.  Returns a namespace: s1, s2, z (final logits), p (probabilities),
    p1max, flags (exact), need (the decision used), out [B,H,d], V [B,H,N,d], absdot [B,H,N] (sum_i |q_i k_i| / sqrt(d),
    the larger of the two key views), tau [B,H] (flag_band)."""
    B, H, d = qr.shape
    q = np.asarray(qr, np.float64)
    sc = _rep(scale, H).astype(np.float64)
    m16 = 16.0 * _rep(msb, H).astype(np.float64)
    k1 = m16 * sc
    k2 = (m16 + _rep(lsb, H).astype(np.float64)) * sc
    V = _rep(qv, H).astype(np.float64) * _rep(vscale, H).astype(np.float64)
    rd = math.sqrt(d)
    s1 = np.einsum("bhd,bhld->bhl", q, k1) / rd
    s2 = np.einsum("bhd,bhld->bhl", q, k2) / rd
    p1max = 1.0 / np.exp(s1 - s1.max(-1, keepdims=True)).sum(-1)
    flags = p1max < thr
    use = flags if need is None else np.asarray(need, bool)
    z = np.where(use[..., None], s2, s1)
    p = _softmax64(z)
    out = np.einsum("bhl,bhld->bhd", p, V)
    absdot = np.einsum("bhd,bhld->bhl", np.abs(q), np.maximum(np.abs(k1), np.abs(k2))) / rd
    return SimpleNamespace(s1=s1, s2=s2, z=z, p=p, p1max=p1max, flags=flags, need=use, out=out, V=V, absdot=absdot,
                           tau=flag_band(absdot))


def pq_oracle(qr, msb, lsb, scale, qv, vscale, need):
    """orc.pq_decode_attention_profile with the decision given per head (the comparator of a kernel that took it):
    (out [B,H,d] fp32, logits [B,H,N] fp32)."""
    H = qr.shape[1]
    pl = [_rep(x, H) for x in (msb, lsb, scale, qv, vscale)]
    o0, _, l0 = orc.pq_decode_attention_profile(qr, *pl, 0.0)
    o1, _, l1 = orc.pq_decode_attention_profile(qr, *pl, 2.0)
    nd = np.asarray(need, bool)[..., None]
    return np.where(nd, o1, o0), np.where(nd, l1, l0)


def pq_prefill_exact(qr, msb, lsb, scale, V, thr, past_len, rows=None, need=None):
    """Float64 counterpart of orc.pq_prefill_attention (un-quantised V [B,H,N,d], HF causal rule: row i sees keys
    j <= past_len + i).  ``need`` [B,H,len(rows)]: the decision per query row (None = exact).  Returns (out [B,len(rows),H*d],
    flags [B,H,len(rows)], p1max [B,H,len(rows)])."""
    B, H, ql, d = qr.shape
    rows = list(range(ql)) if rows is None else list(rows)
    sc = _rep(scale, H).astype(np.float64)
    m16 = 16.0 * _rep(msb, H).astype(np.float64)
    k1, k2 = m16 * sc, (m16 + _rep(lsb, H).astype(np.float64)) * sc
    V64 = _rep(V, H).astype(np.float64)
    out = np.zeros((B, len(rows), H, d))
    flags = np.zeros((B, H, len(rows)), bool)
    p1max = np.zeros((B, H, len(rows)))
    for n, i in enumerate(rows):
        vis = past_len + i + 1
        qi = np.asarray(qr[:, :, i], np.float64)
        s1 = np.einsum("bhd,bhld->bhl", qi, k1[:, :, :vis]) / math.sqrt(d)
        s2 = np.einsum("bhd,bhld->bhl", qi, k2[:, :, :vis]) / math.sqrt(d)
        p1max[:, :, n] = 1.0 / np.exp(s1 - s1.max(-1, keepdims=True)).sum(-1)
        flags[:, :, n] = p1max[:, :, n] < thr
        use = flags[:, :, n] if need is None else np.asarray(need, bool)[:, :, n]
        p = _softmax64(np.where(use[..., None], s2, s1))
        out[:, n] = np.einsum("bhl,bhld->bhd", p, V64[:, :, :vis])
    return out.reshape(B, len(rows), H * d), flags, p1max


def local_v_exact(p, V, kept):
    """sum over the kept rows of p_j V_j (full-row denominator, no renormalisation).  p [n], V [n,d], kept [k] -> [d]."""
    idx = np.asarray(kept, np.int64)
    return np.asarray(p, np.float64)[idx] @ np.asarray(V, np.float64)[idx]


# --------------------------------------------------------------------------------------------------------------------- #
# criteria
# --------------------------------------------------------------------------------------------------------------------- #
def flag_band(absdot):
    """Relative band tau per head (absdot [..., N] of the pass-1 row: sum_i |q_i k_i| / sqrt(d))."""
    return TAU_FLOOR + 2.0 * logit_err32(np.asarray(absdot).max(-1))


def decided(p1max, thr, tau):
    """Heads whose exact flag is decided (outside the relative band around the threshold)."""
    return np.abs(p1max - thr) > tau * p1max


def check_flags(got_need, p1max, thr, tau, name=""):
    """need_lsb equal to the exact flag wherever |p1max - thr| > tau p1max (heads inside the band may go either way: their
    output is judged against the decision taken).  Returns the decision as bool."""
    got = np.asarray(got_need).astype(bool)
    dec = decided(p1max, thr, tau)
    bad = dec & (got != (p1max < thr))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: need_lsb {int(got[i])} at {i} where p1max {p1max[i]:.9g} vs threshold {thr:.9g} "
                             f"(relative gap {abs(p1max[i] - thr) / p1max[i]:.3g} > {tau[i]:.3g}); {int(bad.sum())} heads wrong")
    return got


def check_stash_exact(stash, z, absdot, dt, name=""):
    """The stash holds the final logits rounded to dt: |stash - z| <= 1 ulp(dt) + the fp32 logit bound, entry by entry."""
    st = np.asarray(stash, np.float64)
    z = np.asarray(z, np.float64)
    bound = rg.ulp(z, dt) + logit_err32(absdot)
    bad = np.abs(st - z) > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} stash entries off the exact final logits; {i}: {st[i]:.9g} vs {z[i]:.9g}")


def logit_err32(absdot):
    """Bound of the fp32 logit error at rows with sum |q_i k_i| / sqrt(d) = absdot."""
    return LOGIT_ERR * EPS32 * np.asarray(absdot, np.float64)


def kept_delta(zmag, err32, dt):
    """How far a dropped row's exact logit may lie above the smallest kept one: 2 ulp of the stash dtype at that magnitude
    (the select reads the rounded stash) plus both rows' fp32 error; f32: the fp32 error alone."""
    return (0.0 if dt == "f32" else 2.0 * rg.ulp(zmag, dt)) + 2.0 * err32


def check_kept(kept, n, k, z, err32, dt, stash=None, name=""):
    """One unit's kept list: k distinct rows in [0, n); (stash given) the top-k of the kernel's own stash, ties lowest index
    first; against exact math: max exact logit of a dropped row <= min over the kept rows + kept_delta; where exact logits
    tie across the boundary, the kept rows have the lower indices."""
    kept = np.asarray(kept[:k], np.int64)
    assert kept.size == k and len(set(kept.tolist())) == k and kept.min() >= 0 and kept.max() < n, \
        f"{name}: kept list not {k} distinct rows of [0, {n})"
    if stash is not None:
        want = orc.topk_window(np.asarray(stash[:n], np.float32)[None], 0, n, k)[0]
        assert np.array_equal(np.sort(kept), want), f"{name}: kept set is not the top-{k} of the stash"
    if k == n:
        return
    z = np.asarray(z[:n], np.float64)
    mask = np.zeros(n, bool)
    mask[kept] = True
    zmin = z[mask].min()
    zd = z[~mask].max()
    e = float(np.max(np.asarray(err32)[:n])) if np.ndim(err32) else float(err32)
    dl = float(kept_delta(max(abs(zmin), abs(zd)), e, dt))
    assert zd <= zmin + dl, f"{name}: dropped row {int(np.flatnonzero(~mask)[np.argmax(z[~mask])])} has exact logit " \
                            f"{zd:.9g} above the smallest kept {zmin:.9g} by {zd - zmin:.3g} > {dl:.3g}"
    tie_d = np.flatnonzero(~mask & (z == zmin))
    tie_k = np.flatnonzero(mask & (z == zmin))
    if tie_d.size and tie_k.size:
        assert tie_k.max() < tie_d.min(), f"{name}: exact tie at {zmin} not broken lowest index first"


def local_v_slack(p, V, kept, err32):
    """What the fp32 logit error alone moves a kept-row sum by: 2 max(err32) sum_K p_j max|V_j| (p_j's relative error is the
    error of z_j - lse).  Over a few kept rows nothing averages it out, and the oracle's own fp32 logits may land closer by
    chance: at keep = 1 the error is one probability's."""
    idx = np.asarray(kept, np.int64)
    return 2.0 * float(np.max(err32)) * float((np.asarray(p)[idx] * np.abs(np.asarray(V)[idx]).max(-1)).sum())


def check_out_exact_slack(got, oracle_out, exact, slack, dt, d, name=""):
    """regimes.check_out_exact with an extra allowance per (b, row, head) (local_v_slack)."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    ex = rg.exact_excess(got, oracle_out, exact, dt, d) - np.asarray(slack)
    if (ex > 0).any():
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        raise AssertionError(f"{name}: {int((ex > 0).sum())} of {ex.size} (b, row, head) exceed C*err(oracle)+ulp+slack; worst "
                             f"{i}: err {rg.row_err(got, exact, d)[i]:.3g} vs oracle err {rg.row_err(oracle_out, exact, d)[i]:.3g}, "
                             f"slack {np.asarray(slack)[i]:.3g}")


def cascade_slack(p, err32):
    """One step's share of the fp32 logit error in the importance: 2 max_j(err32) p_j, summed over batch rows -> [H, N]
    (p [B,H,N], err32 [B,H,N]).  The kernels' logits carry their own fp32 error into every probability they fold; the oracle's
    fp32 logits need not share it."""
    return (2.0 * np.asarray(err32).max(-1, keepdims=True) * np.asarray(p)).sum(0)


def check_cascade(acc, acc_oracle, acc_exact, T, name="", C=C_CASCADE, slack=None):
    """Per head row: max_j (|acc - exact| - slack_j) <= C max_j |acc_oracle - exact| + T ulp_f32(max_j exact).  acc* [H, L];
    slack [H, L] (sum over steps of cascade_slack) or None."""
    a, o, x = (np.asarray(t, np.float64) for t in (acc, acc_oracle, acc_exact))
    assert np.isfinite(a).all(), f"{name}: non-finite importance"
    ea, eo = (np.abs(a - x) - (0.0 if slack is None else np.asarray(slack))).max(-1), np.abs(o - x).max(-1)
    bound = C * eo + T * rg.ulp(np.abs(x).max(-1), "f32")
    bad = ea > bound
    if bad.any():
        h = int(np.argmax(ea - bound))
        raise AssertionError(f"{name}: importance of {int(bad.sum())} heads off; head {h}: err {ea[h]:.3g} vs oracle err "
                             f"{eo[h]:.3g} (C = {C}, T = {T})")


# --------------------------------------------------------------------------------------------------------------------- #
# regimes through the planes
# --------------------------------------------------------------------------------------------------------------------- #
def quantise(kr, v, kb, vb):
    """(msb, lsb, scale, qv, vscale) of rotated keys / values [B,Hkv,N,d], integers as int64."""
    msb, lsb, scale = orc.pq_quantize(kr, bits=kb + 4)
    qv, vscale = orc.pq_quantize_values(v, bits=vb)
    return msb.astype(np.int64), lsb.astype(np.int64), scale, qv.astype(np.int64), vscale


def pq_case(B, H, Hkv, d, N, dt, regime, kb, vb, seed=23):
    """A regime of tests/regimes.py (decode: one query row at position N - 1 over N keys) through the planes: the case's
    rotated q / keys / values quantised.  Asserts the regime on the EXACT logits of the dequantised keys (s2)."""
    cs = rg.make_case(B, H, Hkv, d, N - 1, 1, dt, regime if isinstance(regime, str) else list(regime), seed)
    pc = SimpleNamespace(cs=cs, B=B, H=H, Hkv=Hkv, d=d, N=N, dt=dt, kb=kb, vb=vb, regimes=cs.regimes)
    pc.qr = cs.qr[:, :, 0]
    pc.planes = quantise(cs.kr, cs.vc, kb, vb)
    ex = pq_exact(pc.qr, *pc.planes, 0.0)
    for b, r in enumerate(cs.regimes):
        rg.assert_regime(ex.s2[b][:, None, :], r, N)
    pc.p1max = ex.p1max
    return pc


# --------------------------------------------------------------------------------------------------------------------- #
# numpy emulation of the PQ kernels' documented arithmetic (+ switchable faults)
# --------------------------------------------------------------------------------------------------------------------- #
FAULTS = ("gather_msb_logits", "flag_rounded_row", "flag_split_partial", "lsb_no_scale", "lsb_neighbour_scale",
          "vscale_prev_row", "renormalise_kept", "kept_per_split", "kept_without_new_row")
CASCADE_FAULTS = ("fold_prev_twice", "flush_skips_last")


def _softmax32(s):
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m).astype(np.float32)
    l = e.sum(-1, keepdims=True, dtype=np.float32)
    return m, l


def emulate_pq(qr, msb, lsb, scale, qv, vscale, thr, dt, keep=None, n_splits=4, fault=None):
    """The kernels' arithmetic: fp32 MSB logit a * (scale 16 / sqrt(d)); need = 1 / l_tot < thr over the head's row;
    logit8 = logit_msb + (q . lsb) scale / sqrt(d); stash = final logit rounded to dt; P.V with exp(lg - m) / l x vscale_j
    over the qv fields; local V (keep): the top-keep of the stash, lowest index first, full-row denominator.
    Returns a namespace: need [B,H], z (final fp32 logits), stash, out [B,H,d] (rounded to dt; over the kept rows if
    keep), kept [B,H,k] or None."""
    B, H, d = qr.shape
    q = np.asarray(qr, np.float32)
    msb, lsb, scale, qv, vscale = (_rep(x, H) for x in (msb, lsb, scale, qv, vscale))
    N = msb.shape[2]
    sc = scale[..., 0].astype(np.float32)
    rsd = np.float32(1.0 / math.sqrt(d))
    a1 = np.einsum("bhd,bhld->bhl", q, msb.astype(np.float32)).astype(np.float32)
    s1 = (a1 * (sc * (np.float32(16.0) * rsd))).astype(np.float32)
    if fault == "flag_rounded_row":
        m1, l1 = _softmax32(orc.round_dt(s1, dt))
    elif fault == "flag_split_partial":
        chunk = -(-N // n_splits)
        m1, l1 = _softmax32(s1[..., :chunk])
    else:
        m1, l1 = _softmax32(s1)
    need = (np.float32(1.0) / l1[..., 0]) < np.float32(thr)
    a2 = np.einsum("bhd,bhld->bhl", q, lsb.astype(np.float32)).astype(np.float32)
    sc2 = sc
    if fault == "lsb_no_scale":
        sc2 = np.ones_like(sc)
    elif fault == "lsb_neighbour_scale":
        sc2 = np.concatenate([sc[..., :1], sc[..., :-1]], -1)
    s2 = (s1 + a2 * (sc2 * rsd)).astype(np.float32)
    z = np.where(need[..., None], s2, s1).astype(np.float32)
    m, l = _softmax32(z)
    lg = s1 if fault == "gather_msb_logits" else z        # the fault: P.V reads the MSB-pass logits, with pass 2's (max, sum)
    p =(np.exp(lg - m) / l).astype(np.float32)
    vs = vscale[..., 0].astype(np.float32)
    if fault == "vscale_prev_row":
        vs = np.concatenate([vs[..., :1], vs[..., :-1]], -1)
    w = (p * vs).astype(np.float32)
    stash = orc.round_dt(z, dt)
    kept = None
    if keep is not None and keep < N:
        kept = np.zeros((B, H, keep), np.int64)
        for b in range(B):
            for h in range(H):
                if fault == "kept_per_split":
                    chunk = -(-N // n_splits)
                    idx = []
                    for s0 in range(0, N, chunk):
                        s_hi = min(N, s0 + chunk)
                        ks = max(1, round(keep * (s_hi - s0) / N))
                        idx += (orc.topk_window(stash[b, h:h + 1, s0:s_hi], 0, s_hi - s0, min(ks, s_hi - s0))[0] + s0).tolist()
                    idx = sorted(idx)[:keep] + [i for i in range(N) if i not in idx][:max(0, keep - len(idx))]
                    kept[b, h] = np.sort(idx[:keep])
                elif fault == "kept_without_new_row":
                    kept[b, h] = orc.topk_window(stash[b, h:h + 1, :N - 1], 0, N - 1, keep)[0]
                else:
                    kept[b, h] = orc.topk_window(stash[b, h:h + 1], 0, N, keep)[0]
        sel = np.zeros((B, H, N), np.float32)
        np.put_along_axis(sel, kept, 1.0, -1)
        w = (w * sel).astype(np.float32)
        if fault == "renormalise_kept":
            w = (w / (p * sel).sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    out = np.einsum("bhl,bhld->bhd", w, qv.astype(np.float32)).astype(np.float32)
    return SimpleNamespace(need=need, z=z, stash=stash, out=orc.round_dt(out, dt), kept=kept, lse=(m[..., 0], l[..., 0]))


def emulate_cascade(logit_rows, fault=None):
    """Cascade importance as the kernels fold it: step t's launch adds step t-1's probabilities exp(lg - m) / l (its fp32
    logits and (max, sum)), the flush adds the last step's.  logit_rows: list over steps of fp32 logits [B,H,n_t] (growing).
    Returns acc [H, n_T] fp32."""
    H, L = logit_rows[-1].shape[1], logit_rows[-1].shape[2]
    acc = np.zeros((H, L), np.float32)
    T = len(logit_rows)
    for t, z in enumerate(logit_rows):
        if fault == "flush_skips_last" and t == T - 1:
            break
        m, l = _softmax32(z)
        p = (np.exp(z - m) / l).astype(np.float32).sum(0, dtype=np.float32)
        reps = 2 if (fault == "fold_prev_twice" and t == T // 2) else 1
        for _ in range(reps):
            acc[:, :z.shape[2]] = (acc[:, :z.shape[2]] + p).astype(np.float32)
    return acc
