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
  (tests/test_pq_exact_cpu.py);
* the PQ-keyed prefill and the stash-free prefill importance: ``pq_prefill_exact`` (every row, masks, causal off),
  ``pq_prefill_oracle``, the derived P-rounding allowance ``p_round_slack``, ``check_pq_prefill`` / ``check_colprob`` and the
  emulations ``emulate_pq_prefill`` / ``emulate_colprob`` with their faults (tests/test_pq_prefill_exact_cpu.py).
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


def prefill_visibility(B, ql, N, P, causal, mask, dt):
    """Which keys take part per query row.  causal: row i sees j <= P + i; mask additive [B,q,N] / [B,1,q,N]: entries at
    finfo_min (<= finfo_min / 2) are hard-masked, the others are added to the logit.  A row with no key left is the uniform
    average over the keys the causal flag leaves it (all N without it), as rg.attention_exact has it.
    Returns (vis [B,1,q,N] bool, add [B,1,q,N] float64 or None, dead [B,1,q,1] bool)."""
    rows = np.arange(ql)
    cv = (np.arange(N)[None, :] <= P + rows[:, None]) if causal else np.ones((ql, N), bool)
    cv = np.broadcast_to(cv[None, None], (B, 1, ql, N))
    if mask is None:
        return cv, None, np.zeros((B, 1, ql, 1), bool)
    m = np.asarray(mask, np.float64)
    m = m[:, None] if m.ndim == 3 else m
    hard = np.broadcast_to(m <= 0.5 * orc.finfo_min(dt), (B, 1, ql, N))
    vis = cv & ~hard
    dead = ~vis.any(-1, keepdims=True)
    return np.where(dead, cv, vis), np.where(hard | dead, 0.0, m), dead


def pq_prefill_exact(qr, msb, lsb, scale, V, thr, past_len, rows=None, need=None, mask=None, causal=True, dt="bf16",
                     full=False):
    """Float64 counterpart of orc.pq_prefill_attention (un-quantised V [B,Hkv,N,d], HF causal rule: row i sees keys
    j <= past_len + i), one [H,q,N] product per batch row.  ``need`` [B,H,len(rows)]: the decision per query row (None =
    exact); mask / causal: prefill_visibility.  Returns (out [B,len(rows),H*d], flags [B,H,len(rows)], p1max
    [B,H,len(rows)]); full=True: a namespace with, per (b, h, row), what pq_exact returns per head — s1, s2 [B,H,R,N] (raw
    logits), vis, p, p1max, flags, need, out, absdot [B,H,R] (max over the visible keys of sum_i |q_i k_i| / sqrt(d)), tau."""
    B, H, ql, d = qr.shape
    N = msb.shape[2]
    rows = np.arange(ql) if rows is None else np.asarray(list(rows), np.int64)
    R = len(rows)
    vis_a, add_a, dead_a = prefill_visibility(B, ql, N, past_len, causal, mask, dt)
    vis_a, dead_a = vis_a[:, :, rows], dead_a[:, :, rows]
    add_a = None if add_a is None else np.broadcast_to(add_a, (B, 1, ql, N))[:, :, rows]
    rd = math.sqrt(d)
    out = np.zeros((B, R, H, d))
    s1a, s2a = np.zeros((B, H, R, N)), np.zeros((B, H, R, N))
    absd = np.zeros((B, H, R))
    for b in range(B):
        sc = _rep(scale[b:b + 1], H)[0].astype(np.float64)
        m16 = 16.0 * _rep(msb[b:b + 1], H)[0].astype(np.float64)
        k1, k2 = m16 * sc, (m16 + _rep(lsb[b:b + 1], H)[0].astype(np.float64)) * sc
        q = np.asarray(qr[b][:, rows], np.float64)
        s1a[b] = q @ np.swapaxes(k1, 1, 2) / rd
        s2a[b] = q @ np.swapaxes(k2, 1, 2) / rd
        ad = np.abs(q) @ np.swapaxes(np.maximum(np.abs(k1), np.abs(k2)), 1, 2) / rd
        absd[b] = np.where(vis_a[b], ad, 0.0).max(-1)
    add = 0.0 if add_a is None else add_a

    def soft(s):
        z = np.where(vis_a, np.where(dead_a, 0.0, s + add), -np.inf)
        e = np.exp(z - z.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)
    p1 = soft(s1a)
    p1max = p1.max(-1)
    flags = p1max < thr
    use = flags if need is None else np.asarray(need, bool)
    pa = np.where(use[..., None], soft(s2a), p1) if use.any() else p1
    for b in range(B):
        out[b] = np.swapaxes(pa[b] @ _rep(V[b:b + 1], H)[0].astype(np.float64), 0, 1)
    out = out.reshape(B, R, H * d)
    if not full:
        return out, flags, p1max
    return SimpleNamespace(s1=s1a, s2=s2a, vis=vis_a, p=pa, p1max=p1max, flags=flags, need=use, out=out, absdot=absd,
                           tau=TAU_FLOOR + 2.0 * logit_err32(absd))


def pq_prefill_oracle(qr, msb, lsb, scale, V, need, past_len, mask=None, causal=True, dt="bf16"):
    """orc.pq_prefill_attention's arithmetic (fp32 dequantised keys, fp32 logits / softmax / P.V) with the decision given
    per (b, h, row), one matrix product per batch row instead of its per-row loop, and with the arguments it lacks: Hkv < H,
    an additive mask, causal=False.  (Equal to it up to fp32 summation order where both are defined:
    tests/test_pq_prefill_exact_cpu.py.)  Returns out [B,q,H*d] fp32."""
    B, H, ql, d = qr.shape
    N = msb.shape[2]
    vis, add, dead = prefill_visibility(B, ql, N, past_len, causal, mask, dt)
    nd = np.asarray(need, bool)
    out = np.zeros((B, ql, H, d), np.float32)
    for b in range(B):
        pl = [_rep(x[b:b + 1], H)[0] for x in (msb, lsb, scale)]
        q = qr[b].astype(np.float32)
        p = np.zeros((H, ql, N), np.float32)
        for use_lsb in (False, True):
            if not (nd[b] == use_lsb).any():
                continue
            k = orc.pq_dequant(pl[0], pl[1] if use_lsb else None, pl[2])
            s = (q @ np.swapaxes(k, 1, 2)) / np.float32(math.sqrt(d))
            if add is not None:
                s = np.where(dead[b], np.float32(0), s + add[b].astype(np.float32))
            p = np.where((nd[b] == use_lsb)[..., None], orc.softmax_probs(np.where(vis[b], s, np.float32(-np.inf))), p)
        out[b] = np.swapaxes(p @ _rep(V[b:b + 1], H)[0].astype(np.float32), 0, 1)
    return out.reshape(B, ql, H * d)


def p_round_slack(p, V, dt):
    """What rounding the un-normalised P to the model dtype before the matrix cores may cost an output element: the prefill
    kernel hands P = exp(s - m_run) to the MFMA as dt (round to nearest: relative error u = 2^-9 bf16 / 2^-12 f16) while l sums
    the unrounded values, so |delta out_d| <= u sum_j p_j |V_jd|.  p [B,H,R,N], V [B,Hkv,N,d] -> [B,R,H] (max over d)."""
    u = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12, "f32": 0.0}[dt]
    H = p.shape[1]
    av = np.abs(_rep(np.asarray(V), H).astype(np.float64))
    return u * np.swapaxes(np.matmul(p, av).max(-1), 1, 2)


def prefill_logit_slack(p, V, absdot):
    """local_v_slack's form over all visible keys: 2 max_j logit_err32 * sum_j p_j max_d |V_j|.  absdot [B,H,R] -> [B,R,H]."""
    H = p.shape[1]
    vm = np.abs(_rep(np.asarray(V), H).astype(np.float64)).max(-1)                     # [B,H,N]
    return np.swapaxes(2.0 * logit_err32(absdot) * np.einsum("bhrn,bhn->bhr", p, vm), 1, 2)


def prefill_out_slack(ex, V, dt):
    """The allowance of a PQ prefill output beyond C err(oracle) + 1 ulp: P rounding + fp32 logit error."""
    return p_round_slack(ex.p, V, dt) + prefill_logit_slack(ex.p, V, ex.absdot)


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


# --------------------------------------------------------------------------------------------------------------------- #
# the PQ prefill and the stash-free prefill importance: cases and criteria
# --------------------------------------------------------------------------------------------------------------------- #
BAND_CAP = 0.01           # share of (b, h, row) a threshold may leave undecided (inside the flag band): a condition on the INPUTS


def prefill_case(B, H, Hkv, d, P, ql, dt, regime, seed=23, mask=None, causal=True):
    """A prefill regime of tests/regimes.py (ql query rows at positions P .. N-1) through 8-bit planes: rotated q, the
    planes of the rotated keys (orc.pq_quantize), values.  mask None: the causal mask (or none at all with causal=False).
    Asserts the regime on the EXACT logits of the dequantised keys (s2) and keeps the exact reference at threshold 0."""
    N = P + ql
    mk = mask if mask is not None else (orc.causal_mask(B, ql, N, dt) if causal else None)
    cs = rg.make_case(B, H, Hkv, d, P, ql, dt, regime if isinstance(regime, str) else list(regime), seed, mask=mk)
    pc = SimpleNamespace(cs=cs, B=B, H=H, Hkv=Hkv, d=d, P=P, ql=ql, N=N, dt=dt, mask=mask, causal=causal and mask is None,
                         regimes=cs.regimes, qr=cs.qr, V=cs.vc)
    msb, lsb, scale = orc.pq_quantize(cs.kr, bits=8)
    pc.planes = (msb.astype(np.int64), lsb.astype(np.int64), scale)
    pc.ex0 = prefill_exact(pc, 0.0)
    for b, r in enumerate(cs.regimes):
        rg.assert_regime(pc.ex0.s2[b], r, N)
    return pc


def prefill_exact(pc, thr, need=None):
    return pq_prefill_exact(pc.qr, *pc.planes, pc.V, thr, pc.P, need=need, mask=pc.mask, causal=pc.causal, dt=pc.dt, full=True)


def band_share(ex0, thr):
    """Share of (b, h, row) whose exact flag is undecided at this threshold (from the float64 reference alone)."""
    return float((~decided(ex0.p1max, thr, ex0.tau)).mean())


def prefill_thresholds(ex0):
    """0, 1 (moved to 1 + 2 max tau where more than BAND_CAP of the rows saturate at p1max = 1 within the band: large logits),
    1.5, the median exact p1max (moved to the middle of the widest gap among the 9 values around it) and 2 tau
    above / below the exact p1max of two fixed rows: (0, 0, row q/8) of the first block and (B-1, H-1, row q - 1 - q/8)
    (or the next row after them whose threshold meets BAND_CAP)."""
    p = np.sort(ex0.p1max.ravel())
    i = p.size // 2
    w = p[max(0, i - 4): i + 5]
    g = int(np.argmax(np.diff(w))) if w.size > 1 else 0
    one = 1.0 if band_share(ex0, 1.0) <= BAND_CAP else 1.0 + 2.0 * float(ex0.tau.max())
    out = [0.0, one, 1.5, float((w[g] + w[min(g + 1, w.size - 1)]) / 2)]
    B, H, ql = ex0.p1max.shape
    for b, h, r0 in ((0, 0, ql // 8), (B - 1, H - 1, ql - 1 - ql // 8)):
        for sign in (1.0, -1.0):
            # the anchor row; where its threshold leaves more than BAND_CAP of the rows undecided (it sits among rows that
            # saturate at the same p1max), the next row of the block that does not — decided from the reference alone
            for r in list(range(r0, ql)) + list(range(r0)):
                t = float(ex0.p1max[b, h, r] * (1 + sign * 2 * ex0.tau[b, h, r]))
                if band_share(ex0, t) <= BAND_CAP:
                    break
            out.append(t)
    return out


def check_pq_prefill(pc, thr, out, need, name="", stats=None):
    """One attn_prefill_pq launch against exact math, every (b, h, row): the undecided share of the INPUTS <= BAND_CAP
    (from the reference alone); flags exact outside the relative band; outputs — rows inside the band judged against the
    decision the kernel took, nothing skipped — err <= C err(oracle) + 1 ulp + P-rounding + fp32-logit allowance.
    Returns the exact namespace of the decision taken; ``stats`` (a dict) collects the worst err / allowance."""
    share = band_share(pc.ex0, thr)
    assert share <= BAND_CAP, f"{name}: {share:.3%} of the rows lie inside the flag band at threshold {thr!r}: move the threshold"
    got = check_flags(need, pc.ex0.p1max, thr, pc.ex0.tau, name)
    ex = prefill_exact(pc, thr, need=got)
    o_out = orc.round_dt(pq_prefill_oracle(pc.qr, *pc.planes, pc.V, got, pc.P, pc.mask, pc.causal, pc.dt), pc.dt)
    slack = prefill_out_slack(ex, pc.V, pc.dt)
    if stats is not None:
        err = rg.row_err(np.asarray(out, np.float64), ex.out, pc.d)
        allow = rg.exact_bound(o_out, ex.out, pc.dt, pc.d, rg.C_EXACT) + slack
        stats["out"] = max(stats.get("out", 0.0), float((err / allow).max()))
        und = ~decided(pc.ex0.p1max, thr, pc.ex0.tau)
        stats["band"] = max(stats.get("band", 0.0), share)
        wrong = (got != (pc.ex0.p1max < thr)) & und
        stats["undecided_flipped"] = stats.get("undecided_flipped", 0) + int(wrong.sum())
    check_out_exact_slack(out, o_out, ex.out, slack, pc.dt, pc.d, name)
    return ex


def colprob_refs(cs, causal=True, acc0=None):
    """(exact [H,N] float64, oracle [H,N] fp32) column sums of the softmax probabilities of a regimes.Case: exact from
    rg.attention_exact's float64 logits with the causal rule, oracle = orc.cascade_importance_accumulate over the ORACLE's
    stash (its two 16-bit roundings).  acc0 [H,>=N]: what the accumulator held before."""
    B, H, ql, N, P = cs.B, cs.H, cs.ql, cs.N, cs.P
    vis = prefill_visibility(B, ql, N, P, causal, None, cs.dt)[0]
    z = np.where(vis, cs.logits, -np.inf)
    e = np.exp(z - z.max(-1, keepdims=True))
    a0 = np.zeros((H, N), np.float32) if acc0 is None else np.asarray(acc0, np.float32)[:, :N]
    exact = a0.astype(np.float64) + (e / e.sum(-1, keepdims=True)).sum((0, 2))
    m = np.where(vis, 0.0, -np.inf).astype(np.float32)
    oracle = orc.cascade_importance_accumulate(a0.copy(), cs.stash, m)
    return exact, oracle


def check_colprob(acc, cs, causal=True, acc0=None, calls=1, name="", stats=None):
    """The stash-free prefill importance against exact math, per head: max_j |acc - exact| <= C err(oracle) + T ulp_f32 with
    T = B q_len (the worst-case fp32 growth of a column sum of that many addends: each add rounds at most half an ulp of the
    running sum, which the column's final magnitude bounds — derived, not measured), C = rg.C_EXACT; the row-sum rule
    (sum_j acc[h, j] = the number of (b, i) pairs, plus what the accumulator held) inside the same bound.
    ``calls``: how many times the contribution was added."""
    H, N = cs.H, cs.N
    T = cs.B * cs.ql * calls
    exact, oracle = colprob_refs(cs, causal, acc0)
    for _ in range(calls - 1):
        e2, o2 = colprob_refs(cs, causal, None)
        exact, oracle = exact + e2, (oracle + o2).astype(np.float32)
    a = np.asarray(acc, np.float64)[:, :N]
    if stats is not None:
        eo = np.abs(oracle - exact).max(-1)
        bound = rg.C_EXACT * eo + T * rg.ulp(np.abs(exact).max(-1), "f32")
        stats["importance"] = max(stats.get("importance", 0.0), float((np.abs(a - exact).max(-1) / bound).max()))
    check_cascade(a, oracle, exact, T, name=name, C=rg.C_EXACT)
    check_cascade(a.sum(-1, keepdims=True), oracle.astype(np.float64).sum(-1, keepdims=True), exact.sum(-1, keepdims=True), T,
                  name=f"{name} row sums", C=rg.C_EXACT)


# --------------------------------------------------------------------------------------------------------------------- #
# numpy emulation of the PQ prefill and of the stash-free prefill importance (+ switchable faults)
# --------------------------------------------------------------------------------------------------------------------- #
KT = 128                  # keys per tile of prefill_pp128_kernel
PREFILL_FAULTS = ("flag_from_run_max", "flag_before_last_tile", "scale_of_previous_tile", "pass2_keeps_pass1_stats",
                  "pass2_drops_last_range", "merge_stale_max", "causal_off_by_one", "kv_head_of_query_head",
                  "mask_row_of_neighbour", "mask_add_rounded")
COLPROB_FAULTS = ("diag_off_by_one", "last_query_tile_dropped", "stats_of_neighbour_row", "first_q_clamped_wrong",
                  "batch_row_0_only")


def pq_pass2_ksplit(kv_len):
    """Key ranges of the split refetch pass (prefill_attn.hip, pq_pass2_ksplit)."""
    tiles = -(-kv_len // KT)
    ks = max(1, min(8, tiles // 8))
    per = -(-tiles // ks)
    return -(-tiles // per)


def _flash_pass(s, vis, edge_from, V, dt, lo, hi, group=32):
    """Online softmax over 128-key tiles [lo, hi) per row (lo / hi [B,H,R] tile indices).  s [B,H,R,N] fp32 logits, vis
    [B,H,R,N]; a tile whose end lies beyond edge_from [R] (the first key some row of the 32-row wave does not see; 0 under a
    mask) takes the per-element path (the maximum moves at once), the others the deferred maximum: it moves only when a row
    of the group outgrew it by more than rg.DEFER_MAX.  P rounded to dt for P.V (V [B,H,N,d] fp32 or None), fp32 sums.
    Returns a namespace of m, l, acc, m_true, m_first and the (m, l, m_true) as they stood before each row's last tile."""
    B, H, R, N = s.shape
    f32 = np.float32
    m = np.full((B, H, R), -np.inf, f32)
    mt = m.copy()
    mfirst = np.full((B, H, R), np.nan, f32)
    l = np.zeros((B, H, R), f32)
    acc = None if V is None else np.zeros((B, H, R, V.shape[-1]), f32)
    prev = None
    Rp = -(-R // group) * group
    for t in range(-(-N // KT)):
        a, e = t * KT, min(N, t * KT + KT)
        act = (t >= lo) & (t < hi)
        if not act.any():
            continue
        st = np.where(vis[..., a:e], s[..., a:e], f32(-np.inf))
        m_tile = st.max(-1)
        edge = np.broadcast_to((t * KT + KT > edge_from)[None, None], m.shape)
        with np.errstate(invalid="ignore"):
            out = (m_tile - m > rg.DEFER_MAX) | (np.isinf(m) & ~np.isinf(m_tile))
        pad = np.zeros((B, H, Rp), bool)
        pad[..., :R] = out & act & ~edge
        move = np.repeat(pad.reshape(B, H, Rp // group, group).any(-1), group, -1)[..., :R]
        m_new = np.where(edge | move, np.maximum(m, m_tile), m)
        last = act & (t + 1 >= hi)
        if prev is None:
            prev = [m.copy(), l.copy(), mt.copy()]
        for x, y in zip(prev, (m, l, mt)):
            x[last] = y[last]
        base = np.where(np.isinf(m_new), f32(0), m_new)
        with np.errstate(invalid="ignore", over="ignore"):
            pe = np.where(vis[..., a:e], np.exp(st - base[..., None]), 0).astype(f32)
            alpha = np.where(m_new != m, np.exp(m - base), 1).astype(f32)
        alpha = np.where(np.isnan(alpha), f32(0), alpha)
        l_n = (l * alpha + pe.sum(-1, dtype=f32)).astype(f32)
        l = np.where(act, l_n, l)
        if acc is not None:
            a_n = (acc * alpha[..., None] + np.matmul(orc.round_dt(pe, dt), V[:, :, a:e])).astype(f32)
            acc = np.where(act[..., None], a_n, acc)
        mt = np.where(act, np.maximum(mt, m_tile), mt)
        m = np.where(act, m_new, m)
        mfirst = np.where(act & np.isnan(mfirst), m, mfirst)
    return SimpleNamespace(m=m, l=l, acc=acc, m_true=mt, m_first=mfirst, prev=prev)


def _edge_from(ql, N, P, causal, masked):
    if masked:
        return np.zeros(ql, np.int64)
    if not causal:
        return np.full(ql, N, np.int64)
    return np.minimum(N, P + (np.arange(ql) // 32) * 32 + 1)


def emulate_pq_prefill(qr, msb, lsb, scale, V, thr, past_len, dt, mask=None, causal=True, fault=None, need=None):
    """The PQ prefill's documented arithmetic: integer-valued keys (exact in dt), fp32 dot, * (scale / sqrt(d)) in fp32, no
    16-bit logit rounding (also under a mask: hard-masked keys sit at finfo_min, the others take the fp32 sum), 128-key tiles,
    deferred maximum, m_true beside m_run, need = exp(m_true - m_run) / l < thr, P rounded to dt, fp32 sums; pass 2 over the
    8-bit keys for the flagged rows — one key range when more than a quarter of the head's rows is flagged, pq_pass2_ksplit
    ranges + the merge otherwise — output rounded to dt.  Returns a namespace: need [B,H,q], out [B,q,H*d]."""
    B, H, ql, d = qr.shape
    Hkv, N = msb.shape[1], msb.shape[2]
    f32 = np.float32
    P = past_len
    if fault == "kv_head_of_query_head" and Hkv < H:
        rep = lambda x: np.asarray(x)[:, np.arange(H) % Hkv]
    else:
        rep = lambda x: _rep(x, H)
    q = np.asarray(qr, f32)
    sc = (rep(scale)[..., 0].astype(f32) * f32(1.0 / math.sqrt(d))).astype(f32)
    if fault == "scale_of_previous_tile":
        sc = np.concatenate([sc[..., :KT], sc[..., :-KT]], -1) if N > KT else sc
    k1 = 16.0 * rep(msb).astype(f32)
    k8 = (k1 + rep(lsb).astype(f32)).astype(f32)
    V32 = rep(V).astype(f32)
    mk = mask
    if mk is not None and fault == "mask_row_of_neighbour":
        mk = np.asarray(mk)
        mk = np.concatenate([mk[..., 1:, :], mk[..., -1:, :]], -2)
    Pv = P - 1 if fault == "causal_off_by_one" else P
    vis, add, dead = prefill_visibility(B, ql, N, Pv, causal, mk, dt)
    if fault == "causal_off_by_one":
        vis = vis.copy()
        vis[..., 0] |= ~vis.any(-1)
    vis = np.broadcast_to(vis, (B, H, ql, N))
    fm = f32(orc.finfo_min(dt))

    def logits(k):
        s = (np.matmul(q, np.swapaxes(k, 2, 3)).astype(f32) * sc[:, :, None, :]).astype(f32)
        if mk is not None:
            if fault == "mask_add_rounded":
                m4 = np.asarray(mk, f32)
                s = orc.round_dt(s + (m4[:, None] if m4.ndim == 3 else m4), dt).astype(f32)
            else:
                s = (s + add.astype(f32)).astype(f32)
            s = np.where(np.broadcast_to(dead, s.shape), fm, s)
        return s
    ef = _edge_from(ql, N, P, causal, mk is not None)
    tiles_all = -(-N // KT)
    zero = np.zeros((B, H, ql), np.int64)
    p1 = _flash_pass(logits(k1), vis, ef, V32, dt, zero, zero + tiles_all)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pmax = np.exp(p1.m_true - p1.m) / p1.l
        if fault == "flag_from_run_max":
            pmax = f32(1.0) / p1.l
        elif fault == "flag_before_last_tile":
            pm, pl, pt = p1.prev
            pmax = np.where(pl > 0, np.exp(pt - pm) / pl, f32(1.0))
    flag = (pmax < f32(thr)) if need is None else np.asarray(need, bool)
    out = (p1.acc / p1.l[..., None]).astype(f32)
    if flag.any():
        s8 = logits(k8)
        ks2 = pq_pass2_ksplit(N)
        split = (flag.sum(-1) * 4 <= ql) & (ks2 > 1)                                   # [B,H]: the compacted, key-split form
        # the tiles a row's workgroup walks: up to the last row of its block of 256 list entries
        att = np.full((B, H, ql), tiles_all, np.int64)
        if causal:
            for b in range(B):
                for h in range(H):
                    lst = np.flatnonzero(flag[b, h])
                    for c in range(0, lst.size, 256):
                        blk = lst[c:c + 256]
                        att[b, h, blk] = -(-min(N, P + int(blk[-1]) + 1) // KT)
        ksb = np.where(split, ks2, 1)[..., None]
        per = -(-att // ksb)
        parts = []
        for sidx in range(int(ksb.max())):
            lo = np.minimum(sidx * per, att)
            hi = np.where(sidx < ksb, np.minimum(lo + per, att), lo)
            parts.append(_flash_pass(s8, vis, ef if mk is not None or not causal else np.minimum(N, P + np.arange(ql) + 1),
                                     V32, dt, lo, hi, group=1))
        if fault == "pass2_drops_last_range" and len(parts) > 1:
            keep_all = ~split[..., None]
            last = parts[-1]
            last.l = np.where(keep_all, last.l, f32(0))
            last.m = np.where(keep_all, last.m, f32(-np.inf))
        M = np.max(np.stack([p_.m for p_ in parts]), 0)
        L = np.zeros_like(parts[0].l)
        O = np.zeros_like(parts[0].acc)
        for i, p_ in enumerate(parts):
            with np.errstate(invalid="ignore"):
                w = np.where(np.isinf(p_.m), f32(0), np.exp(p_.m - M)).astype(f32)
                if fault == "merge_stale_max" and len(parts) > 1 and i == len(parts) // 2:
                    w = np.where(np.isnan(p_.m_first) | np.isinf(p_.m), f32(0), np.exp(np.minimum(p_.m_first - M, 0))).astype(f32)
            L = (L + w * p_.l).astype(f32)
            O = (O + w[..., None] * p_.acc).astype(f32)
        if fault == "pass2_keeps_pass1_stats":
            L = p1.l
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(flag[..., None], (O / L[..., None]).astype(f32), out)
    out = orc.round_dt(out, dt)
    return SimpleNamespace(need=flag, out=np.swapaxes(out, 1, 2).reshape(B, ql, H * d), pmax=pmax)


def emulate_colprob(cs, causal=True, fault=None, acc0=None):
    """prefill_colprob_kernel's arithmetic on a regimes.Case: acc[h, j] += sum_{b, i visible} exp2(v_ij log2e - (m_i log2e +
    log2 l_i)) with v_ij the logit after the reference's two 16-bit roundings and (m_i, l_i) from an emulated
    reference-numerics flash pass with a deferred maximum.  Returns (acc [H,N] fp32, m [B,H,q], l [B,H,q])."""
    import copy
    c2 = copy.copy(cs)
    c2.mask = None
    f32 = np.float32
    B, H, ql, N, P = cs.B, cs.H, cs.ql, cs.N, cs.P
    v = rg.emulate_logits(c2, "reference")
    vis = np.broadcast_to(prefill_visibility(B, ql, N, P, causal, None, cs.dt)[0], v.shape)
    zero = np.zeros((B, H, ql), np.int64)
    fp = _flash_pass(v, vis, _edge_from(ql, N, P, causal, False), None, cs.dt, zero, zero + (-(-N // KT)))
    m, l = fp.m, fp.l
    if fault == "stats_of_neighbour_row":
        m, l = (np.concatenate([x[..., 1:], x[..., -1:]], -1) for x in (m, l))
    log2e = f32(1.4426950408889634)
    st = (m * log2e + np.log2(l).astype(f32)).astype(f32)
    with np.errstate(over="ignore"):
        pr = np.exp2((v.astype(np.float64) * float(log2e) - st[..., None]).astype(f32)).astype(f32)     # one fma
    i, j = np.arange(ql)[:, None], np.arange(N)[None, :]
    take = np.broadcast_to(vis, pr.shape).copy()
    if fault == "diag_off_by_one" and causal:
        take &= (j < P + i)
    if fault == "last_query_tile_dropped":
        take[:, :, (ql - 1) // 128 * 128:] = False
    if fault == "first_q_clamped_wrong" and causal:
        first_q = np.maximum(0, (j // 256) * 256 - P)                           # per key block of 256
        t_lo = first_q // 128
        take &= ~((first_q > 0) & (i // 128 == t_lo))
    if fault == "batch_row_0_only":
        take[1:] = False
    acc = np.zeros((H, N), f32) if acc0 is None else np.asarray(acc0, f32)[:, :N].copy()
    acc = (acc + np.where(take, pr, f32(0)).sum((0, 2), dtype=f32)).astype(f32)
    return acc, fp.m, fp.l
