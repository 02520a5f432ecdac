"""Logit regimes and the exact-softmax criterion (test infrastructure; may import oracle/).

The suite's fixed output tolerance (tests/util.py OUT_TOL) is loose where outputs are small (flat, unit-variance logits: the
output is an average of ~N/e value rows) and unfair where logits are large (the reference's own 16-bit logit roundings move
its output far from exact math).  This module judges a kernel against EXACT attention instead, relative to how far the
oracle itself sits from it:

* ``attention_exact``: float64 softmax attention of the reference's own dtype-rounded ROTATED q / k (what the kernels
  reproduce bit for bit), no intermediate rounding;
* ``check_out_exact``: per (batch, query row, head), ``err(got) <= C * err(oracle) + 1 ulp`` of the row's largest exact
  output element (err = max-abs over the head's d-vector against the exact output);
* seeded generators of the regimes real Llama attention has (sinks, large spreads, a moving maximum, a winning split whose
  neighbours underflow, masks), built in rotated space and checked against the oracle's stash;
* ``emulate_kernel``: numpy restatement of the kernels' documented arithmetic (online softmax over 64-row tiles, unnormalised
  P rounded to the model dtype, fp32 accumulation, the split merge) with switchable faults — the CPU calibration of C and the
  evidence that the criterion catches what OUT_TOL lets through (tests/test_logit_regimes_cpu.py).
"""
import math

import numpy as np

from oracle import spatten_oracle as orc

# C of the criterion: calibrated on the CPU with emulate_kernel (test_the_calibration_of_c) — reference-numerics
# arithmetic stays within 1.0x the oracle's own error beyond the ulp, fp32 logits below it; 2x leaves room for the kernels'
# other summation orders
C_EXACT = 2.0
# f32: the kernels take exp2 of log2e-prescaled fp32 logits (one fma + v_exp_f32 per logit), an argument error of ~|s| 2^-24 the
# oracle's exp(s - m) does not have; next to the oracle's tiny fp32 error that is a measured 6.4x at logit std 12 (2.5e-6
# absolute, an eighth of OUT_TOL's 2e-5)
C_EXACT_F32 = 8.0


def c_for(dt):
    return C_EXACT_F32 if dt == "f32" else C_EXACT
TILE = 64                 # rows per online-softmax tile of the decode / flash kernels
DEFER_MAX = 8.0           # prefill_attn.hip kDeferMax: the running maximum moves only past this margin
SPLIT_GAP = 120.0         # split_winner: every other split sits this far below (> 104: its fp32 partial underflows to 0)

REGIMES = ("flat", "sink8", "sink24", "new_max", "new_min", "rising", "split_winner", "large4", "large12")
DECODE_ONLY = ("new_max", "new_min")


# --------------------------------------------------------------------------------------------------------------------- #
# the exact reference and the criterion
# --------------------------------------------------------------------------------------------------------------------- #
def attention_exact(qr, kr, v, mask=None, dt="bf16"):
    """Float64 attention of rotated q [B,H,q,d] over rotated keys kr / values v [B,Hkv,N,d] (repeat_kv as in the reference),
    additive mask [B,1,q,N] (or broadcastable) as orc.attention_core takes it.  Entries at finfo_min are masked out; a query
    row with EVERY key masked is the uniform average over the keys (its logits all round to finfo_min in the reference).
    Returns (out [B,q,H*d] float64, logits [B,H,q,N] float64 before the mask)."""
    B, H, ql, d = qr.shape
    rep = H // kr.shape[1]
    k64 = orc.repeat_kv(np.asarray(kr, np.float64), rep)
    v64 = orc.repeat_kv(np.asarray(v, np.float64), rep)
    logits = np.matmul(np.asarray(qr, np.float64), np.swapaxes(k64, 2, 3)) / math.sqrt(d)
    s = logits
    if mask is not None:
        m = np.broadcast_to(np.asarray(mask, np.float64), logits.shape)
        hard = m <= 0.5 * orc.finfo_min(dt)
        s = np.where(hard, -np.inf, logits + np.where(hard, 0.0, m))
        s = np.where(hard.all(-1, keepdims=True), 0.0, s)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    o = np.matmul(p, v64)
    return np.swapaxes(o, 1, 2).reshape(B, ql, H * d), logits


def ulp(x, dt):
    """One unit in the last place of |x| in dtype dt (the smallest normal's for 0)."""
    mant = {"f32": 23, "f16": 10, "bf16": 7}[dt]
    tiny = {"f32": 2.0 ** -126, "f16": 2.0 ** -14, "bf16": 2.0 ** -126}[dt]
    x = np.maximum(np.abs(np.asarray(x, np.float64)), tiny)
    return 2.0 ** (np.floor(np.log2(x)) - mant)


def row_err(got, exact, d):
    """max-abs error over each head's d-vector: [B,q,H*d] -> [B,q,H]."""
    g = np.asarray(got, np.float64)
    return np.abs(g - exact).reshape(*g.shape[:-1], -1, d).max(-1)


def exact_bound(oracle_out, exact, dt, d, C=None):
    """The allowance per (batch, query row, head): C * err(oracle) + 1 ulp at the row's max |exact| (C: c_for(dt))."""
    C = c_for(dt) if C is None else C
    amax = np.abs(exact).reshape(*exact.shape[:-1], -1, d).max(-1)
    return C * row_err(oracle_out, exact, d) + ulp(amax, dt)


def exact_excess(got, oracle_out, exact, dt, d, C=None):
    """err(got) - allowance per row (<= 0 where the criterion holds)."""
    return row_err(got, exact, d) - exact_bound(oracle_out, exact, dt, d, C)


def check_out_exact(got, oracle_out, exact, dt, d, C=None, name=""):
    """Assert err(got, exact) <= C * err(oracle_out, exact) + 1 ulp(dt) at the row's max |exact|, for every (b, row, head).
    got / oracle_out / exact [B,q,H*d]."""
    C = c_for(dt) if C is None else C
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    ex = exact_excess(got, oracle_out, exact, dt, d, C)
    if (ex > 0).any():
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        e = row_err(got, exact, d)[i]
        o = row_err(oracle_out, exact, d)[i]
        raise AssertionError(f"{name}: {int((ex > 0).sum())} of {ex.size} (b, row, head) exceed C*err(oracle)+ulp; worst {i}: "
                             f"err {e:.3g} vs oracle err {o:.3g} (C = {C})")


def check_fast_vs_reference(got_fast, got_ref, exact, dt, d, name=""):
    """fp32-logit forms: err(fast, exact) <= err(reference-numerics kernel, exact) + 1 ulp per (b, row, head)."""
    amax = np.abs(exact).reshape(*exact.shape[:-1], -1, d).max(-1)
    ef, er = row_err(got_fast, exact, d), row_err(got_ref, exact, d)
    bad = ef > er + ulp(amax, dt)
    assert not bad.any(), f"{name}: fp32 logits further from exact than the reference numerics at {int(bad.sum())} rows, " \
                          f"worst {float((ef - er).max()):.3g}"


# --------------------------------------------------------------------------------------------------------------------- #
# regimes, built in rotated space
# --------------------------------------------------------------------------------------------------------------------- #
def _tables64(n, d):
    c, s = orc.rope_table(n, d, "f32")
    return c.astype(np.float64), s.astype(np.float64)


def unrotate(xr, cos, sin, pos):
    """Inverse of apply_rotary_pos_emb_single in float64: x = xr*cos - rotate_half(xr)*sin.  pos [B or 1, n]."""
    c = cos[pos][:, None]
    s = sin[pos][:, None]
    return xr * c - orc.rotate_half(xr) * s


def _offsets(regime, N, ql, rng):
    """(per-key logit offset c [N], base spread sigma) of one batch row."""
    c = np.zeros(N)
    sigma = 1.0
    if regime == "flat":
        pass
    elif regime.startswith("sink"):
        c[:4] = float(regime[4:])
    elif regime == "new_max":
        c[N - 1] = 30.0
    elif regime == "new_min":
        c[N - 1] = -60.0
    elif regime == "rising":
        R = min(96.0, max(24.0, N / 32.0))
        c = R * np.arange(N) / N
    elif regime == "split_winner":
        w = split_winner_rows(N)
        c[:] = -SPLIT_GAP
        c[w[0]:w[1]] = 0.0
    elif regime.startswith("large"):
        sigma = float(regime[5:])
    else:
        raise ValueError(regime)
    return c, sigma


def split_winner_rows(N):
    """The 8 rows (8-aligned: inside one split for every split count, splits are whole multiples of 8 rows) that win."""
    w = (N // 2) // 8 * 8
    return w, min(N, w + 8)


class Case:
    """Inputs (orc.attention_core's: q [B,H,ql,d], k / v [B,Hkv,ql,d], past = (pk, pv) [B,Hkv,P,d] or None, mask or None),
    the oracle's (out, stash) and the exact (out, logits)."""


def make_case(B, H, Hkv, d, P, ql, dt, regime, seed, mask=None):
    """Regime(s) per batch row (a name or a list of B names).  Keys, values and queries are chosen so the logits are
    base_ij + c_j: q_i = n_i + sqrt(d) e, k_j = sigma n_j + c_j e with n _|_ e (e one fixed unit vector per kv head), in
    ROTATED space; q / k are then un-rotated in float64 at their positions and rounded to dt.  The regime is asserted
    from the oracle's stash.  mask: additive [B,1,ql,N] (finfo_min entries) or None; decode (ql = 1) builds no causal mask."""
    regimes = [regime] * B if isinstance(regime, str) else list(regime)
    assert len(regimes) == B
    N = P + ql
    rng = np.random.default_rng([seed, B, H, Hkv, d, P, ql, {"f32": 0, "f16": 1, "bf16": 2}[dt]])
    cos, sin = _tables64(N, d)
    if all(r == "flat" for r in regimes):
        from tests.util import attn_inputs
        q, k, v, past = attn_inputs(B, H, Hkv, d, P, ql, dt, seed)
    else:
        rep = H // Hkv
        e = rng.standard_normal((B, Hkv, 1, d))
        e /= np.linalg.norm(e, axis=-1, keepdims=True)
        perp = lambda x, e_: x - (x * e_).sum(-1, keepdims=True) * e_
        eq = np.repeat(e, rep, 1)
        qr = perp(rng.standard_normal((B, H, ql, d)), eq) + math.sqrt(d) * eq
        kr = np.empty((B, Hkv, N, d))
        for b, r in enumerate(regimes):
            if r in DECODE_ONLY:
                assert ql == 1, f"{r} is a decode regime"
            c, sigma = _offsets(r, N, ql, rng)
            # logit = (n_i . sigma n_j) / sqrt(d) + c_j: |n|^2 ~ d so the base spread is ~sigma
            kr[b] = sigma * perp(rng.standard_normal((Hkv, N, d)), e[b]) + c[None, :, None] * e[b]
        q = orc.round_dt(unrotate(qr, cos, sin, np.arange(P, N)[None]), dt)
        kc = orc.round_dt(unrotate(kr, cos, sin, np.arange(N)[None]), dt)
        vall = orc.synth_normal(seed, 2, (B, Hkv, N, d), dt)
        k, v = kc[:, :, P:], vall[:, :, P:]
        past = (kc[:, :, :P], vall[:, :, :P]) if P else None
    cs = case_from_inputs(q, k, v, past, mask, dt)
    cs.regimes = regimes
    for b, r in enumerate(regimes):
        assert_regime(cs.stash[b], r, N)
    return cs


def case_from_inputs(q, k, v, past, mask, dt):
    """A Case of given inputs (orc.attention_core's layout; query rows at positions P.. N-1)."""
    B, H, ql, d = q.shape
    Hkv = k.shape[1]
    P = 0 if past is None else past[0].shape[2]
    N = P + ql
    cs = Case()
    cs.q, cs.k, cs.v, cs.past, cs.mask, cs.dt, cs.regimes = q, k, v, past, mask, dt, None
    cs.B, cs.H, cs.Hkv, cs.d, cs.P, cs.ql, cs.N = B, H, Hkv, d, P, ql, N
    pos = np.tile(np.arange(P, N)[None], (B, 1))
    pk, pv = (None, None) if past is None else past
    cs.out, cs.stash, (kc_o, vc_o) = orc.attention_core(q, k, v, pk, pv, pos, mask, dt)
    c32, s32 = orc.rope_table(N, d, dt)
    cs.qr = orc.apply_rotary_pos_emb_single(q, c32, s32, pos, dt)
    cs.kr = orc.apply_rotary_pos_emb_single(kc_o, c32, s32, np.arange(N)[None], dt)
    cs.vc = vc_o
    cs.exact, cs.logits = attention_exact(cs.qr, cs.kr, vc_o, mask, dt)
    return cs


def assert_regime(st, regime, N):
    """The regime is really in the oracle's stash st [H,q,N] of one batch row."""
    st = st.astype(np.float64)
    if regime == "flat":
        assert 0.75 < st.std() < 1.3, st.std()
    elif regime.startswith("sink"):
        D = float(regime[4:])
        gap = st[..., :4].mean(-1) - st[..., 4:].mean(-1)
        assert (gap > D - 2.5).all() and (gap < D + 2.5).all(), (regime, gap.min(), gap.max())
    elif regime == "new_max":
        assert (st[..., -1] - st[..., :-1].max(-1) > 20).all()
    elif regime == "new_min":
        assert (st[..., :-1].min(-1) - st[..., -1] > 40).all()
    elif regime == "rising":
        R = min(96.0, max(24.0, N / 32.0))
        assert (st[..., -N // 4:].max(-1) > st[..., :N // 2].max(-1) + R / 4).all()
        assert (np.argmax(st, -1) >= N - N // 8).mean() > 0.9        # the maximum lands in the last split
    elif regime == "split_winner":
        a, b = split_winner_rows(N)
        rest = np.concatenate([st[..., :a], st[..., b:]], -1)
        assert (st[..., a:b].max(-1) - rest.max(-1) > 104).all()
    elif regime.startswith("large"):
        sg = float(regime[5:])
        assert 0.8 * sg < st.std() < 1.25 * sg, (regime, st.std())
    else:
        raise ValueError(regime)


def decode_mask(B, N, dt, kinds):
    """Additive decode masks [B,1,1,N]: per batch row 'range' (keys [N/4, 3N/4) at finfo_min: whole splits masked for every
    split count >= 3), 'full' (every key masked, as left padding leaves a row) or 'none'."""
    m = np.zeros((B, 1, 1, N), np.float32)
    fm = np.float32(orc.finfo_min(dt))
    for b, kd in enumerate(kinds):
        if kd == "range":
            m[b, ..., N // 4: 3 * N // 4] = fm
        elif kd == "full":
            m[b] = fm
    return m


def prefill_mask(B, ql, N, dt, pad, lo=None, hi=None):
    """Causal + left padding of `pad` tokens per batch row (query rows < pad see no key at all) + keys [lo, hi) masked."""
    m = orc.causal_mask(B, ql, N, dt).copy()
    fm = np.float32(orc.finfo_min(dt))
    P = N - ql
    for b in range(B):
        if pad[b]:
            m[b, :, :, P:P + pad[b]] = fm               # the padded prompt tokens are nobody's keys
            m[b, :, :pad[b], :] = fm                    # and their own query rows see nothing
    if lo is not None:
        m[..., lo:hi] = fm
    return m


# --------------------------------------------------------------------------------------------------------------------- #
# numpy emulation of the kernels' documented arithmetic (+ switchable faults)
# --------------------------------------------------------------------------------------------------------------------- #
FAULTS = ("drop_new_row", "merge_weight_0p8", "merge_stale_max", "defer_without_correction", "masked_row_zeros")


def emulate_logits(cs, numerics):
    """[B,H,q,N] float32 logits as the kernels form them: 'reference' = the two 16-bit roundings + the rounded mask add,
    'fast' = fp32 logits (+ mask in fp32)."""
    rep = cs.H // cs.Hkv
    qr = cs.qr.astype(np.float32)
    kr = orc.repeat_kv(cs.kr, rep).astype(np.float32)
    dot = np.matmul(qr, np.swapaxes(kr, 2, 3)).astype(np.float32)
    if numerics == "reference":
        s = orc.round_dt(orc.round_dt(dot, cs.dt) / np.float32(math.sqrt(cs.d)), cs.dt)
        if cs.mask is not None:
            s = orc.round_dt(s + cs.mask, cs.dt)
    else:
        s = (dot / np.float32(math.sqrt(cs.d))).astype(np.float32)
        if cs.mask is not None:
            s = np.maximum(s + cs.mask.astype(np.float32), np.float32(orc.finfo_min("f32")))
    return s.astype(np.float32)


def emulate_kernel(cs, numerics="reference", n_splits=1, fault=None, defer=False):
    """Online softmax over 64-row tiles per split, unnormalised P = exp(s - running max) rounded to dt for P.V, fp32 sums,
    then the split merge (max of the split maxima, weights exp(m_s - M)).  defer: the running maximum only moves when a tile
    outgrows it by more than DEFER_MAX (P then carries up to e^DEFER_MAX, exact once divided by l).  Returns [B,q,H*d]."""
    B, H, ql, d, N, dt = cs.B, cs.H, cs.ql, cs.d, cs.N, cs.dt
    s = emulate_logits(cs, numerics)
    V = orc.repeat_kv(cs.vc, H // cs.Hkv).astype(np.float32)                     # [B,H,N,d]
    S = max(1, min(n_splits, N))
    chunk = -(-(-(-N // S)) // 8) * 8
    bounds = [(a, min(N, a + chunk)) for a in range(0, N, chunk)]
    parts = []
    for (a, b) in bounds:
        m = np.full((B, H, ql, 1), -np.inf, np.float32)
        m_first = None
        l = np.zeros((B, H, ql, 1), np.float32)
        acc = np.zeros((B, H, ql, d), np.float32)
        for t in range(a, b, TILE):
            u = min(b, t + TILE)
            st = s[..., t:u]
            mt = st.max(-1, keepdims=True)
            if defer or fault == "defer_without_correction":
                move = (mt - m > DEFER_MAX) | ~np.isfinite(m)
                m_new = np.where(move, np.maximum(m, mt), m) if fault != "defer_without_correction" else np.maximum(m, mt)
                # the fault: a small move of the maximum is taken for P but acc / l are not rescaled by it
                scale = np.where(np.isfinite(m), np.exp(m - m_new), 0).astype(np.float32)
                if fault == "defer_without_correction":
                    scale = np.where(move, scale, np.float32(1.0)).astype(np.float32)
            else:
                m_new = np.maximum(m, mt)
                scale = np.where(np.isfinite(m), np.exp(m - m_new), 0).astype(np.float32)
            p = np.exp(st - m_new).astype(np.float32)
            p16 = orc.round_dt(p, dt)
            if fault == "drop_new_row" and u == N and ql == 1:
                p16 = p16.copy()
                p16[..., -1] = 0                                                 # scored (in l) but left out of P.V
            l = (l * scale + p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
            acc = (acc * scale + np.matmul(p16, V[:, :, t:u, :])).astype(np.float32)
            m = m_new
            if m_first is None:
                m_first = m.copy()
        parts.append((m, l, acc, m_first))
    M = np.max(np.stack([p_[0] for p_ in parts]), 0)
    L = np.zeros_like(parts[0][1])
    O = np.zeros_like(parts[0][2])
    for i, (m, l, acc, m_first) in enumerate(parts):
        w = np.exp(m - M).astype(np.float32)
        if fault == "merge_weight_0p8" and i == len(parts) // 2:                # (the middle split: split_winner's)
            w = (w * np.float32(0.8)).astype(np.float32)
        if fault == "merge_stale_max" and i == len(parts) // 2:
            w = np.exp(np.minimum(m_first - M, 0)).astype(np.float32)           # the split's first-tile maximum
        L = (L + w * l).astype(np.float32)
        O = (O + w * acc).astype(np.float32)
    o = (O / L).astype(np.float32)
    if fault == "masked_row_zeros" and cs.mask is not None:
        full = (cs.mask <= 0.5 * orc.finfo_min(dt)).all(-1)[..., None]        # [B,1,q,1]
        o = np.where(np.broadcast_to(full, o.shape), np.float32(0), o)
    o = orc.round_dt(o, dt)
    return np.swapaxes(o, 1, 2).reshape(B, ql, H * d)
