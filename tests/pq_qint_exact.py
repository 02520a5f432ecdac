"""The quantised-query decode over the planes (spatten_attn_decode_pq_qint, include/spatten.h "Quantised query") against EXACT
math (test infrastructure; may import oracle/).

Integer arithmetic is exact: with the query the kernel EXPORTS (q_int, q_scale) a logit is a known integer times two known
scales, so the criteria are far tighter than tests/pq_exact.py's fp32 ones (LOGIT_ERR = 48 epsilons of sum |q_i k_i|):

* ``check_query_quant``: q_scale within 1 fp32 ulp of amax / Q, |q_int| <= Q, q_int a nearest rounding of qr / q_scale;
* ``qint_exact``: ``pq_exact`` with the query q_int * float64(q_scale), plus the exact integers A1, A2;
* ``logit_bound``: R 2^-24 (|s1| + |s2 - s1|) with R = 8, the number of fp32 roundings of the documented chain — 16 / sqrt(d)
  (2: the square root and the reciprocal; the scaling by 16 is exact), cq, key_scale * cq, the product (5 on s1); the LSB term
  shares the four scale roundings (cq / 16 is exact) and adds its product, and the final add rounds once at a magnitude
  <= |s1| + |s2 - s1|: at most 6 on either term.  R = 8 leaves two to spare;
* ``check_step``: every criterion of one decode step (the GPU test and the CPU emulation are judged by the same code);
* ``emulate_qint``: a numpy restatement of the arithmetic with switchable faults (tests/test_pq_qint_cpu.py).
"""
import math
from types import SimpleNamespace

import numpy as np

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import regimes as rg

R_ROUNDINGS = 8
FAULTS = ("bias_not_removed", "lsb_odd_even_swapped", "q_scale_of_neighbour_head", "msb_term_not_x16", "q_not_rotated",
          "refetch_rereads_unscaled_lsb", "q_int_piece_order_exported")


def qmax(bits):
    return 2 ** (bits - 1) - 1


def quantise_query(qr, bits):
    """The documented query quantisation: (q_int int64 [B,H,d], q_scale fp32 [B,H])."""
    Q = qmax(bits)
    amax = np.abs(np.asarray(qr, np.float32)).max(-1)
    q_scale = (amax / np.float32(Q)).astype(np.float32)
    safe = np.where(q_scale > 0, q_scale, np.float32(1)).astype(np.float64)
    q_int = np.clip(np.rint(np.asarray(qr, np.float64) / safe[..., None]), -Q, Q).astype(np.int64)
    q_int[q_scale == 0] = 0
    return q_int, q_scale


def query64(q_int, q_scale):
    return np.asarray(q_int, np.float64) * np.asarray(q_scale, np.float64)[..., None]


def qint_exact(q_int, q_scale, planes, thr, need=None):
    """``pq_exact`` with the query q_int * float64(q_scale); also the exact integers A1 = sum_i q_int_i msb_ij and
    A2 = sum_i q_int_i lsb_ij ([B,H,N] int64)."""
    ex = px.pq_exact(query64(q_int, q_scale), *planes, thr, need=need)
    H = q_int.shape[1]
    qi = np.asarray(q_int, np.int64)
    ex.A1 = np.einsum("bhd,bhld->bhl", qi, px._rep(planes[0], H).astype(np.int64))
    ex.A2 = np.einsum("bhd,bhld->bhl", qi, px._rep(planes[1], H).astype(np.int64))
    # the logits from the exact integers (a float64 sum of the products leaves ~1e-16 where the integer sum cancels to 0)
    f = np.asarray(q_scale, np.float64)[..., None] * px._rep(planes[2], H)[..., 0].astype(np.float64) / math.sqrt(q_int.shape[2])
    ex.s1 = 16.0 * ex.A1 * f
    ex.s2 = (16.0 * ex.A1 + ex.A2) * f
    ex.z = np.where(ex.need[..., None], ex.s2, ex.s1)
    return ex


def logit_bound(s1, s2):
    """R 2^-24 (|s1| + |s2 - s1|), R = R_ROUNDINGS = 8 (the module docstring counts them)."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    return R_ROUNDINGS * px.EPS32 * (np.abs(s1) + np.abs(s2 - s1))


def check_query_quant(qr, q_int, q_scale, bits, name=""):
    """q_scale within 1 fp32 ulp of amax / Q; |q_int| <= Q; |q_int_i - qr_i / q_scale| <= 0.5 + 2^-20 in float64 (a nearest
    rounding; which way a tie goes is left free); an all-zero query: q_scale = 0 and q_int = 0."""
    Q = qmax(bits)
    qr64 = np.asarray(qr, np.float64)
    qs = np.asarray(q_scale, np.float64)
    qi = np.asarray(q_int, np.int64)
    want = np.abs(qr64).max(-1) / Q
    assert (np.abs(qs - want) <= rg.ulp(want, "f32") * (want > 0)).all(), \
        f"{name}: q_scale off amax / Q by {np.abs(qs - want).max():.3g}"
    assert (np.abs(qi) <= Q).all(), f"{name}: |q_int| above {Q}"
    zero = want == 0
    assert (qi[zero] == 0).all() and (qs[zero] == 0).all(), f"{name}: an all-zero query must give q_scale = 0, q_int = 0"
    quo = qr64 / np.where(zero, 1.0, qs)[..., None]
    err = np.abs(qi - quo)[~zero]
    assert err.size == 0 or err.max() <= 0.5 + 2.0 ** -20, f"{name}: q_int is not a nearest rounding (off by {err.max():.9g})"


def thresholds(ex0, n_gaps=2):
    """From the exact reference alone (as px.prefill_thresholds): 0, 1.5 and the midpoints of the widest gaps between the
    heads' sorted p1max — widest first, a midpoint that leaves more than BAND_CAP of the heads inside the flag band (heads
    that saturate at the same p1max: new_max) is passed over."""
    p = np.sort(np.asarray(ex0.p1max).ravel())
    out = [0.0, 1.5]
    if p.size > 1:
        gaps = np.diff(p)
        for g in np.argsort(-gaps, kind="stable"):
            t = float((p[g] + p[g + 1]) / 2)
            if band_share(ex0, t) <= px.BAND_CAP:
                out.append(t)
            if len(out) == 2 + n_gaps:
                break
    return out


def flag_tau(ex0):
    """TAU_FLOOR + 2 logit_bound at the head's largest pass-1 logit ([B,H])."""
    return px.TAU_FLOOR + 2.0 * logit_bound(np.abs(ex0.s1).max(-1), np.abs(ex0.s1).max(-1))


def band_share(ex0, thr):
    return float((~px.decided(ex0.p1max, thr, flag_tau(ex0))).mean())


def out_slack(ex, lb):
    """px.local_v_slack's form over ALL rows with logit_bound: 2 max_j lb_j sum_j p_j max_d |V_jd| -> [B,1,H]."""
    vm = np.abs(ex.V).max(-1)
    return (2.0 * lb.max(-1) * (ex.p * vm).sum(-1))[:, None, :]


def check_step(qr, planes, dt, bits, thr, res, heads=None, msb_only=False, only=None, stats=None, name=""):
    """Every criterion of one step.  res: q_int [B,H,d], q_scale [B,H], msb_logit [B,H,N] fp32 (of an MSB-only launch, or
    None), stash [B,H,N], need [B,H], out [B,H,d].  ``only``: a subset of {"quant", "msb_logit", "stash", "flags", "out"}.
    Heads inside the flag band are judged against the decision taken; nothing is skipped.  Returns the exact namespace."""
    B, H, d = qr.shape
    hs = list(range(H)) if heads is None else list(heads)
    want = (lambda k: only is None or k in only)
    qi, qs = np.asarray(res.q_int)[:, hs], np.asarray(res.q_scale)[:, hs]
    if want("quant"):
        check_query_quant(qr[:, hs], qi, qs, bits, name)
    # (the exact reference needs every head's query: pruned heads take the documented quantisation of their own query)
    qi_all, qs_all = quantise_query(qr, bits)
    qi_all[:, hs], qs_all[:, hs] = qi, qs
    ex0 = qint_exact(qi_all, qs_all, planes, thr)
    if want("msb_logit") and res.msb_logit is not None:
        lb1 = logit_bound(ex0.s1, ex0.s1)
        err = np.abs(np.asarray(res.msb_logit, np.float64) - ex0.s1)[:, hs]
        if stats is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                stats["msb_logit"] = max(stats.get("msb_logit", 0.0), float(np.nan_to_num(err / lb1[:, hs]).max()))
        assert (err <= lb1[:, hs]).all(), f"{name}: msb_logit off s1(q_int, q_scale) by {err.max():.3g} (bound {lb1[:, hs].max():.3g})"
    tau = flag_tau(ex0)
    got = np.asarray(res.need).astype(bool)
    if want("flags"):
        share = float((~px.decided(ex0.p1max, thr, tau))[:, hs].mean())
        assert share <= px.BAND_CAP, f"{name}: {share:.2%} of the heads inside the flag band at threshold {thr!r}"
        px.check_flags(got[:, hs], ex0.p1max[:, hs], thr, tau[:, hs], name)
    use = np.zeros((B, H), bool)
    use[:, hs] = False if msb_only else got[:, hs]
    ex = qint_exact(qi_all, qs_all, planes, thr, need=use)
    lb = logit_bound(ex.s1, ex.z)
    if want("stash"):
        z = ex.z[:, hs]
        st = np.asarray(res.stash, np.float64)[:, hs]
        bound = rg.ulp(z, dt) + lb[:, hs]
        if stats is not None:
            stats["stash"] = max(stats.get("stash", 0.0), float((np.abs(st - z) / bound).max()))
        bad = np.abs(st - z) > bound
        assert not bad.any(), f"{name}: {int(bad.sum())} stash entries off the exact final logits (worst {np.abs(st - z).max():.3g})"
    if want("out"):
        o_out, _ = px.pq_oracle(query64(qi_all, qs_all).astype(np.float32), *planes, use)
        sel = (lambda x: np.asarray(x)[:, hs].reshape(B, 1, -1))
        slack = out_slack(ex, lb)[:, :, hs]
        if stats is not None:
            allow = rg.exact_bound(sel(orc.round_dt(o_out, dt)), sel(ex.out), dt, d) + slack
            stats["out"] = max(stats.get("out", 0.0), float((rg.row_err(sel(res.out), sel(ex.out), d) / allow).max()))
        px.check_out_exact_slack(sel(res.out), sel(orc.round_dt(o_out, dt)), sel(ex.out), slack, dt, d, name)
    return ex


# --------------------------------------------------------------------------------------------------------------------- #
# numpy emulation of the documented arithmetic (+ switchable faults)
# --------------------------------------------------------------------------------------------------------------------- #
def _piece_order(d):
    """Element index held by position p of the piece-ordered row (piece c = elements 8c .. 8c+7, d/2 + 8c .. d/2 + 8c+7)."""
    idx = []
    for c in range(d // 16):
        idx += list(range(8 * c, 8 * c + 8)) + list(range(d // 2 + 8 * c, d // 2 + 8 * c + 8))
    return np.asarray(idx)


def emulate_qint(qr, planes, thr, dt, bits, kb=8, fault=None, q_unrotated=None, msb_only=False):
    """The documented arithmetic: query quantisation; int64 dots; fp32 scale chain (cq = q_scale (16 / sqrt(d)); s1 = float(A1)
    (key_scale cq); s2 = s1 + float(A2) (key_scale cq / 16)); fp32 softmax; need = 1 / l < thr; P.V as px.emulate_pq.
    Returns a namespace: q_int, q_scale (as exported), msb_logit (s1 fp32), z, stash, need, out [B,H,d] (rounded to dt)."""
    f32 = np.float32
    B, H, d = qr.shape
    msb, lsb, scale, qv, vscale = (px._rep(x, H) for x in planes)
    src = q_unrotated if fault == "q_not_rotated" else qr
    q_int, q_scale = quantise_query(src, bits)
    rsd = f32(1.0) / np.sqrt(f32(d))
    c16 = f32(16.0) * rsd
    if fault == "msb_term_not_x16":
        c16 = rsd
    qs_used = np.roll(q_scale, 1, axis=1) if fault == "q_scale_of_neighbour_head" else q_scale
    cq = (qs_used * c16).astype(f32)                                                   # [B,H]
    m_fields = msb.astype(np.int64) + ((1 << (kb - 1)) if fault == "bias_not_removed" else 0)
    A1 = np.einsum("bhd,bhld->bhl", q_int, m_fields)
    l_fields = lsb.astype(np.int64)
    if fault == "lsb_odd_even_swapped":
        l_fields = l_fields[..., np.arange(d) ^ 1]
    A2 = np.einsum("bhd,bhld->bhl", q_int, l_fields)
    ks = scale[..., 0].astype(f32)
    s1 = (A1.astype(f32) * (ks * cq[..., None]).astype(f32)).astype(f32)
    cq2 = cq if fault == "refetch_rereads_unscaled_lsb" else (cq * f32(0.0625)).astype(f32)
    s2 = (s1 + (A2.astype(f32) * (ks * cq2[..., None]).astype(f32)).astype(f32)).astype(f32)
    _, l1 = px._softmax32(s1)
    need = (f32(1.0) / l1[..., 0]) < f32(thr)
    z = np.where((need & (not msb_only))[..., None], s2, s1).astype(f32)
    m, l = px._softmax32(z)
    p = (np.exp(z - m) / l).astype(f32)
    w = (p * vscale[..., 0].astype(f32)).astype(f32)
    out = np.einsum("bhl,bhld->bhd", w, qv.astype(f32)).astype(f32)
    exp_q = q_int[..., _piece_order(d)] if fault == "q_int_piece_order_exported" else q_int
    return SimpleNamespace(q_int=exp_q, q_scale=q_scale, msb_logit=s1, z=z, stash=orc.round_dt(z, dt), need=need,
                           out=orc.round_dt(out, dt))


def method_bound(q_scale, planes, H, d):
    """Derived, not measured: against the unquantised query every |q_i - q_int_i q_scale| <= q_scale / 2, so for every key
    |s_q - s| <= (q_scale / 2) sum_i |k_i| / sqrt(d).  Returns ([B,H,N] for the MSB keys, [B,H,N] for the 8-bit keys)."""
    sc = px._rep(planes[2], H).astype(np.float64)
    m16 = 16.0 * px._rep(planes[0], H).astype(np.float64)
    k1 = np.abs(m16 * sc).sum(-1)
    k2 = np.abs((m16 + px._rep(planes[1], H).astype(np.float64)) * sc).sum(-1)
    half = np.asarray(q_scale, np.float64)[..., None] / 2.0 / math.sqrt(d)
    return half * k1, half * k2
