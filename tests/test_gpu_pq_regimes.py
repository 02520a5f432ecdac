"""Progressive quantisation, local V pruning and cascade importance against EXACT math (tests/pq_exact.py), in the
logit regimes of tests/regimes.py built in rotated space and packed into the planes, and in PQ-specific cases: peaked and flat
heads in one launch, thresholds at 0 / 1 / above 1 and 2 tau either side of a head's max probability, all-zero key / value
rows, rows with one dominant field, zero queries (exact ties across every split), short and tile-edge lengths.

Criteria: need_lsb equals the exact flag outside the relative band tau (check_flags); the stash within 1 ulp + the fp32 logit
bound of the exact final logits of the decision taken; outputs err <= C err(oracle) + 1 ulp (local V: + the fp32 logit bound
through the kept rows); kept sets the top-k of the kernel's own stash and no dropped row's exact logit above the smallest kept
one's by more than delta; cascade importance per head within C err(oracle) + T ulp of the exact sum of probabilities.
Needs an MI355X."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import regimes as rg
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_pq_local_v import _kept_lists
from tests.util import TORCH_DT, dev, host

pytestmark = pytest.mark.gpu

PROFILES = [(4, 8), (8, 8), (6, 6)]


@functools.lru_cache(maxsize=None)
def _pc(B, H, Hkv, d, N, dt, regime, kb, vb, seed=23):
    return px.pq_case(B, H, Hkv, d, N, dt, regime, kb, vb, seed)


class Inputs:
    """Host planes + exact reference inputs and their device form (planes packed by the library, asserted bit exact)."""

    def __init__(self, qr, q, kr, v, kb, vb, dt, extra=9):
        from spatten_amd import ops
        self.B, self.Hkv, self.N, self.d = kr.shape
        self.H = qr.shape[1]
        self.dt, self.kb, self.vb = dt, kb, vb
        self.qr = qr
        self.planes = px.quantise(kr, v, kb, vb)
        B, Hkv, N, d = self.B, self.Hkv, self.N, self.d
        self.cap = N + extra
        krd = torch.zeros(B, Hkv, self.cap, d, dtype=TORCH_DT[dt], device="cuda")
        vd = torch.zeros_like(krd)
        krd[:, :, :N], vd[:, :, :N] = dev(kr, dt), dev(v, dt)
        self.pl = ops.PQProfilePlanes(B, Hkv, self.H, self.cap, d, "cuda", key_bits=kb, value_bits=vb)
        ops.pq_pack_planes(krd, vd, self.pl, 0, N)
        got = self.pl.unpack(N)
        for g, w in zip(got, self.planes):
            assert np.array_equal(g, w), "planes not bit exact to the oracle's quantiser"
        self.qd = dev(q, dt)
        self.cos, self.sin = oracle_table(self.cap + 1, d, dt)


def _from_case(pc, extra=9):
    cs = pc.cs
    return Inputs(pc.qr, cs.q[:, :, 0], cs.kr, cs.vc, pc.kb, pc.vb, pc.dt, extra)


def _sel(x, heads):
    """[B,H,...] -> the listed heads, as [B,1,len(heads)*d] when x is [B,H,d]."""
    y = np.asarray(x)[:, heads]
    return y.reshape(y.shape[0], 1, -1) if y.ndim == 3 else y


def check_decode(inp, thr, out, need, st, heads=None, msb_only=False, name=""):
    """Flags, stash and output of one attn_decode_pqv launch against exact math.  out [B,H,d], need [B,H], st [B,H,N]."""
    B, H, d, dt = inp.B, inp.H, inp.d, inp.dt
    hs = list(range(H)) if heads is None else list(heads)
    ex0 = px.pq_exact(inp.qr, *inp.planes, thr)
    got = px.check_flags(need[:, hs], ex0.p1max[:, hs], thr, ex0.tau[:, hs], name)
    use = np.zeros((B, H), bool)
    use[:, hs] = False if msb_only else got
    ex = px.pq_exact(inp.qr, *inp.planes, thr, need=use)
    o_out, _ = px.pq_oracle(inp.qr, *inp.planes, use)
    px.check_stash_exact(st[:, hs], ex.z[:, hs], ex.absdot[:, hs], dt, name)
    rg.check_out_exact(_sel(out, hs), _sel(orc.round_dt(o_out, dt), hs), _sel(ex.out, hs), dt, d, name=name)
    return ex


def run_pqv(inp, thr, heads=None, **kw):
    from spatten_amd import ops
    B, H, d, N = inp.B, inp.H, inp.d, inp.N
    need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
    scores = torch.zeros(B, H, inp.cap, dtype=TORCH_DT[inp.dt], device="cuda")
    out = torch.zeros(B, H * d, dtype=TORCH_DT[inp.dt], device="cuda")
    hid = None if heads is None else torch.tensor(heads, dtype=torch.int32, device="cuda")
    ops.attn_decode_pqv(inp.qd, inp.pl, N, inp.cos, inp.sin, N - 1, thr, out=out, need_lsb=need, scores=scores, head_ids=hid,
                        **kw)
    torch.cuda.synchronize()
    return host(out).reshape(B, H, d), need.cpu().numpy().reshape(B, H), host(scores)[:, :, :N]


def thresholds(inp):
    """0, exactly 1, above 1, between two heads' exact p1max, and 2 tau above / below heads 0 and 1's exact p1max."""
    ex = px.pq_exact(inp.qr, *inp.planes, 0.0)
    p = np.sort(ex.p1max.ravel())
    i = p.size // 2
    out = [0.0, 1.0, 1.5, float((p[i - 1] + p[i]) / 2) if p.size > 1 else 0.5]
    for h in range(min(2, inp.H)):
        out += [float(ex.p1max[0, h] * (1 + 2 * ex.tau[0, h])), float(ex.p1max[0, h] * (1 - 2 * ex.tau[0, h]))]
    return out


# ---- 1. attn_decode_pqv ----------------------------------------------------------------------------------------------
_REGIME_SETS = {(8, 8): rg.REGIMES, (4, 8): ("flat", "sink24", "rising", "split_winner", "large12"),
                (6, 6): ("flat", "sink8", "new_max", "large4", "large12")}


@pytest.mark.parametrize("kb,vb,regime", [(kb, vb, r) for (kb, vb) in PROFILES for r in _REGIME_SETS[(kb, vb)]])
def test_pqv_regimes(kb, vb, regime):
    """2081 rows, 8 heads, d 128, bf16: every threshold of ``thresholds``; auto / 1 / 7 splits at the median threshold."""
    inp = _from_case(_pc(1, 8, 8, 128, 2081, "bf16", regime, kb, vb))
    for thr in thresholds(inp):
        out, need, st = run_pqv(inp, thr)
        check_decode(inp, thr, out, need, st, name=f"{regime} thr={thr!r}")
    thr = thresholds(inp)[3]
    for ns in (1, 7):
        out, need, st = run_pqv(inp, thr, n_splits=ns)
        check_decode(inp, thr, out, need, st, name=f"{regime} ns={ns}")


@pytest.mark.parametrize("dt,d,H,Hkv,N,regime,prof", [
    ("f16", 64, 8, 4, 2081, "sink24", (8, 8)), ("f32", 128, 8, 2, 2081, "large12", (8, 8)),
    ("f32", 64, 4, 4, 1500, "rising", (6, 6)), ("f16", 128, 8, 8, 700, "split_winner", (4, 8)),
    ("bf16", 64, 8, 2, 2081, "new_max", (6, 6)), ("f32", 128, 4, 4, 700, "flat", (4, 8)),
    ("bf16", 128, 8, 4, 5000, "sink8", (4, 8)), ("f16", 64, 4, 2, 300, "new_min", (8, 8))])
def test_pqv_dtypes_dims_gqa_heads_and_forms(dt, d, H, Hkv, N, regime, prof):
    """f16 / f32 / bf16, d 64 / 128, Hkv < H; a head list; msb_only (flags from pass 1, output from the MSB logits); the
    device-length form (bit-identical to the host form laid out for the capacity, and exact)."""
    from spatten_amd import ops
    kb, vb = prof
    inp = _from_case(_pc(2, H, Hkv, d, N, dt, regime, kb, vb), extra=40)
    ths = thresholds(inp)
    for thr in ths:
        out, need, st = run_pqv(inp, thr)
        check_decode(inp, thr, out, need, st, name=f"thr={thr!r}")
    heads = [1, H - 1]
    thr = ths[3]
    out, need, st = run_pqv(inp, thr, heads=heads)
    check_decode(inp, thr, out, need, st, heads=heads, name="head list")
    rest = [h for h in range(H) if h not in heads]
    assert not out[:, rest].any() and (need[:, rest] == -1).all()
    out, need, st = run_pqv(inp, thr, msb_only=True)
    check_decode(inp, thr, out, need, st, msb_only=True, name="msb_only")
    # device length: bound = capacity, length N from the step state
    B, cap = inp.B, inp.cap
    cos_p, sin_p = oracle_table(cap, d, dt)
    res = []
    for dyn in (False, True):
        need_d = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
        sc = torch.zeros(B, H, cap, dtype=TORCH_DT[dt], device="cuda")
        if dyn:
            st_ = ops.StepState(cos_p, sin_p)
            st_.set(N - 1, N - 2)
            st_.advance()
            o = ops.attn_decode_pqv(inp.qd, inp.pl, cap, cos_p, sin_p, 0, thr, scores=sc, need_lsb=need_d, step=st_)
        else:
            o = ops.attn_decode_pqv(inp.qd, inp.pl, N, cos_p, sin_p, N - 1, thr, scores=sc, need_lsb=need_d, layout=cap)
        torch.cuda.synchronize()
        res.append((o.clone(), sc.clone(), need_d.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    check_decode(inp, thr, host(res[1][0]).reshape(B, H, d), res[1][2].cpu().numpy().reshape(B, H),
                 host(res[1][1])[:, :, :N], name="device length")


@pytest.mark.parametrize("regime", ["rising", "large12", "flat"])
def test_pqv_f32_six_bit_fields_keep_fp32_precision(regime):
    """Regression: the (6, 6) fields went through the mantissa forms for every output dtype — values 4096 + f (6 bits of the
    fp32 accumulator, ~2^-17 of full scale: 12x the oracle's error at rising), keys 64 + f with 96 qsum taken out (15x at
    large12).  f32 outputs now take extract + convert (pq_decode.hip fma_piece / dot_piece)."""
    inp = _from_case(_pc(1, 4, 4, 64, 1500, "f32", regime, 6, 6))
    for thr in (0.0, 2.0):
        out, need, st = run_pqv(inp, thr)
        check_decode(inp, thr, out, need, st, name=f"{regime} thr={thr}")


def _constructed(kind, kb, vb, dt="bf16", B=1, H=4, d=128, N=2081, seed=7):
    """PQ-specific inputs (rotated keys built around the reference's rotated query):
    'mixed'    head 0's newest key = 2 x its query (p1max ~ 1), head 1 flat at 1 / N (zero query), heads 2.. normal;
    'zero'     rows of all-zero keys and values (scale 1) every 7th row, the newest one among them;
    'dominant' every key row one large field, the others quantising to -1 / 0 / 1 (msb = -1, lsb = 15: the largest MSB-only
               error), values likewise;
    'ties'     a zero query: every logit exactly 0, ties across every split."""
    rng = np.random.default_rng([seed, N, d, kb, {"bf16": 0, "f16": 1, "f32": 2}[dt]])
    q = orc.round_dt(rng.standard_normal((B, H, d)).astype(np.float32), dt)
    c, s = orc.rope_table(N + 9 + 1, d, dt)
    if kind in ("mixed", "ties"):
        q[:, 1 if kind == "mixed" else slice(None)] = 0
    qr = orc.apply_rotary_pos_emb_single(q[:, :, None], c, s, np.full((B, 1), N - 1), dt)[:, :, 0]
    kr = rng.standard_normal((B, H, N, d)).astype(np.float32)
    v = rng.standard_normal((B, H, N, d)).astype(np.float32)
    if kind == "mixed":
        kr[:, 0, N - 1] = 2.0 * qr[:, 0]
    elif kind == "zero":
        kr[:, :, ::7] = 0
        v[:, :, ::7] = 0
        kr[:, :, N - 1] = 0
        v[:, :, N - 1] = 0
    elif kind == "dominant":
        for x in (kr, v):
            big = 8.0 * np.sign(rng.standard_normal((B, H, N)))
            qmax = 2.0 ** (kb + 3) - 1
            x[:] = rng.uniform(-1.4, 1.4, (B, H, N, d)) * (8.0 / qmax)
            x[..., 5] = big
    kr, v = orc.round_dt(kr, dt), orc.round_dt(v, dt)
    return Inputs(qr, q, kr, v, kb, vb, dt)


@pytest.mark.parametrize("kind", ["mixed", "zero", "dominant", "ties"])
@pytest.mark.parametrize("kb,vb", PROFILES)
def test_pqv_constructed_cases(kind, kb, vb):
    inp = _constructed(kind, kb, vb)
    if kind == "dominant":      # the case is what it claims: msb = -1 with lsb = 15 in every row
        m, l = inp.planes[0], inp.planes[1]
        assert ((m == -1) & (l == 15)).any(-1).all()
    if kind == "mixed":
        ex = px.pq_exact(inp.qr, *inp.planes, 0.0)
        assert ex.p1max[0, 0] > 0.999 and abs(ex.p1max[0, 1] * inp.N - 1) < 1e-9
    for thr in thresholds(inp):
        out, need, st = run_pqv(inp, thr)
        check_decode(inp, thr, out, need, st, name=f"{kind} thr={thr!r}")


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 129, 1023, 1025, 4097])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_pqv_lengths(N, dt):
    inp = _constructed("mixed", 8, 8, dt=dt, H=4, d=64, N=N)
    for thr in thresholds(inp):
        for ns in (0, 3):
            out, need, st = run_pqv(inp, thr, n_splits=ns)
            check_decode(inp, thr, out, need, st, name=f"N={N} thr={thr!r} ns={ns}")


# ---- 2. the composed step (attn_decode_pq_local_v) -------------------------------------------------------------------
def run_pq_local_v(inp, thr, keep, heads=None, dyn=False, frac=0.0):
    from spatten_amd import ops
    B, H, d, N, dt = inp.B, inp.H, inp.d, inp.N, inp.dt
    need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
    scores = torch.zeros(B, H, inp.cap, dtype=TORCH_DT[dt], device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    out = torch.zeros(B, H * d, dtype=TORCH_DT[dt], device="cuda")
    hid = None if heads is None else torch.tensor(heads, dtype=torch.int32, device="cuda")
    if dyn:
        cos_p, sin_p = oracle_table(inp.cap, d, dt)
        st = ops.StepState(cos_p, sin_p)
        st.set(N - 1, N - 2)
        st.advance()
        ops.attn_decode_pq_local_v(inp.qd, inp.pl, inp.cap, cos_p, sin_p, 0, thr, 1, scores, lse, out=out, need_lsb=need,
                                   head_ids=hid, keep_fraction=frac, step=st)
    else:
        ops.attn_decode_pq_local_v(inp.qd, inp.pl, N, inp.cos, inp.sin, N - 1, thr, keep, scores, lse, out=out, need_lsb=need,
                                   head_ids=hid)
    torch.cuda.synchronize()
    return host(out).reshape(B, H, d), need.cpu().numpy().reshape(B, H), host(scores)[:, :, :N], _kept_lists(B, H, d)


def check_local_v(inp, thr, keep, out, need, st, kept, heads=None, name=""):
    """Flags and stash as check_decode; the kept set (own stash + exact logits); out = sum over the kernel's kept rows of
    p_exact V (full-row denominator) against the same sum in fp32 over the oracle's probabilities."""
    B, H, d, N, dt = inp.B, inp.H, inp.d, inp.N, inp.dt
    hs = list(range(H)) if heads is None else list(heads)
    ex0 = px.pq_exact(inp.qr, *inp.planes, thr)
    got = px.check_flags(need[:, hs], ex0.p1max[:, hs], thr, ex0.tau[:, hs], name)
    use = np.zeros((B, H), bool)
    use[:, hs] = got
    ex = px.pq_exact(inp.qr, *inp.planes, thr, need=use)
    _, o_lg = px.pq_oracle(inp.qr, *inp.planes, use)
    px.check_stash_exact(st[:, hs], ex.z[:, hs], ex.absdot[:, hs], dt, name)
    probs = orc.softmax_probs(o_lg)
    V32 = px._rep(inp.planes[3], H).astype(np.float32) * px._rep(inp.planes[4], H)
    ref_o = np.zeros((B, H, d), np.float32)
    ref_x = np.zeros((B, H, d))
    slack = np.zeros((B, 1, H))
    for b in range(B):
        for h in hs:
            k_ = np.sort(kept[b, h, :keep])
            err = px.logit_err32(ex.absdot[b, h])
            px.check_kept(k_, N, keep, ex.z[b, h], err, dt, stash=st[b, h], name=f"{name} ({b}, {h})")
            ref_o[b, h] = probs[b, h, k_] @ V32[b, h, k_]
            ref_x[b, h] = px.local_v_exact(ex.p[b, h], ex.V[b, h], k_)
            slack[b, 0, h] = px.local_v_slack(ex.p[b, h], ex.V[b, h], k_, err)
    px.check_out_exact_slack(_sel(out, hs), _sel(orc.round_dt(ref_o, dt), hs), _sel(ref_x, hs), slack[:, :, hs], dt, d,
                             name=name)


@pytest.mark.parametrize("prof,dt,d,regime", [
    ((8, 8), "bf16", 128, "flat"), ((8, 8), "bf16", 128, "sink24"), ((6, 6), "bf16", 64, "rising"),
    ((4, 8), "f16", 128, "split_winner"), ((8, 8), "f32", 128, "large12"), ((6, 6), "f32", 64, "new_max"),
    ((4, 8), "bf16", 128, "large4"), ((8, 8), "f16", 64, "new_min")])
def test_pq_local_v_regimes(prof, dt, d, regime):
    """keep 1 / 30 % / n - 1 / n, with and without a head list, host- and device-length forms."""
    kb, vb = prof
    H, N = 8, 2081
    inp = _from_case(_pc(2, H, H, d, N, dt, regime, kb, vb), extra=31)
    ths = thresholds(inp)
    for thr in (ths[0], ths[2], ths[3], ths[4]):
        for keep in (1, math.ceil(0.3 * N), N - 1, N):
            out, need, st, kept = run_pq_local_v(inp, thr, keep)
            check_local_v(inp, thr, keep, out, need, st, kept, name=f"{regime} thr={thr!r} keep={keep}")
    heads = [0, 3, 6]
    thr = ths[3]
    out, need, st, kept = run_pq_local_v(inp, thr, 100, heads=heads)
    check_local_v(inp, thr, 100, out, need, st, kept, heads=heads, name="head list")
    rest = [h for h in range(H) if h not in heads]
    assert not out[:, rest].any() and (need[:, rest] == -1).all()
    frac = 0.3
    for hl in (None, heads):
        out, need, st, kept = run_pq_local_v(inp, thr, 0, heads=hl, dyn=True, frac=frac)
        check_local_v(inp, thr, math.ceil(frac * N), out, need, st, kept, heads=hl, name=f"device length heads={hl}")


@pytest.mark.parametrize("kb,vb", PROFILES)
def test_pq_local_v_ties_and_constructed(kb, vb):
    """A zero query (every logit 0: the plateau covers every split; keep 777 lands inside it) and the mixed / dominant cases."""
    inp = _constructed("ties", kb, vb, N=3001)
    for keep in (1, 777, 3000):
        out, need, st, kept = run_pq_local_v(inp, 0.5, keep)
        for h in range(inp.H):
            assert np.array_equal(kept[0, h, :keep], np.arange(keep))
        check_local_v(inp, 0.5, keep, out, need, st, kept, name=f"ties keep={keep}")
    for kind in ("mixed", "dominant", "zero"):
        inp = _constructed(kind, kb, vb)
        for thr in thresholds(inp)[:4]:
            out, need, st, kept = run_pq_local_v(inp, thr, 300)
            check_local_v(inp, thr, 300, out, need, st, kept, name=f"{kind} thr={thr!r}")


def test_pq_local_v_c5_scale():
    """40 heads x 8192 rows, (8, 8), bf16: flags at the median threshold and 2 tau around two heads, 30 % kept."""
    inp = _from_case(_pc(1, 40, 40, 128, 8192, "bf16", "sink8", 8, 8))
    ths = thresholds(inp)
    for thr in (ths[3], ths[4], ths[5]):
        out, need, st, kept = run_pq_local_v(inp, thr, 2458)
        check_local_v(inp, thr, 2458, out, need, st, kept, name=f"C5 thr={thr!r}")


def test_pq_local_v_grouped_query_is_refused():
    from spatten_amd import ops
    inp = _from_case(_pc(1, 8, 2, 64, 300, "bf16", "flat", 8, 8))
    sc = torch.zeros(1, 8, inp.cap, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(1, 8, 2, dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.attn_decode_pq_local_v(inp.qd, inp.pl, inp.N, inp.cos, inp.sin, inp.N - 1, 0.5, 10, sc, lse)


# ---- 3. local V over the un-quantised cache (attn_decode_local_v, cascade.local_v_decode) ------------------------------
@functools.lru_cache(maxsize=None)
def _case(B, H, Hkv, d, P, dt, regime, seed=17):
    return rg.make_case(B, H, Hkv, d, P, 1, dt, regime, seed)


@pytest.mark.parametrize("dt,d,H,Hkv,regime", [
    ("bf16", 128, 8, 8, "sink24"), ("bf16", 128, 8, 8, "rising"), ("f16", 64, 8, 4, "split_winner"),
    ("f32", 128, 4, 4, "large12"), ("f32", 64, 4, 2, "new_max"), ("bf16", 64, 8, 2, "flat"), ("f32", 128, 8, 8, "sink8")])
def test_local_v_regimes(dt, d, H, Hkv, regime):
    """One launch and the three-launch form; keep 1 / 30 % / n - 1; the kept set is the top-k of the kernel's own stash
    (asserted by test_gpu_local_v), judged here against the exact logits; out against sum_K p_exact V."""
    from spatten_amd.cascade import local_v_decode
    cs = _case(1, H, Hkv, d, 2080, dt, regime)
    B, N = cs.B, cs.N
    krd, vd = dev(cs.kr, dt), dev(cs.vc, dt)
    cos, sin = oracle_table(N + 5, d, dt)
    qd = dev(cs.q[:, :, 0], dt)
    z = cs.logits[:, :, 0]                                            # exact logits [B,H,N]
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    V = orc.repeat_kv(cs.vc, H // Hkv).astype(np.float64)
    absdot = np.einsum("bhd,bhld->bhl", np.abs(cs.qr[:, :, 0].astype(np.float64)),
                       np.abs(orc.repeat_kv(cs.kr, H // Hkv).astype(np.float64))) / math.sqrt(d)
    probs = orc.softmax_probs(cs.stash[:, :, 0])
    V32 = V.astype(np.float32)
    for three in (False, True):
        for keep in (1, math.ceil(0.3 * N), N - 1):
            lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
            out, stash = local_v_decode(qd, krd, vd, N, cos, sin, N - 1, keep, lse=lse, three_launches=three)
            torch.cuda.synchronize()
            st = host(stash)[:, :, :N]
            o = host(out).reshape(B, H, d)
            name = f"{regime} three={three} keep={keep}"
            ref_o = np.zeros((B, H, d), np.float32)
            ref_x = np.zeros((B, H, d))
            slack = np.zeros((B, 1, H))
            for b in range(B):
                k_all = orc.topk_window(st[b], 0, N, keep)
                for h in range(H):
                    k_ = k_all[h]
                    err = px.logit_err32(absdot[b, h])
                    # the reference-numerics stash rounds twice (dot, then / sqrt(d)): up to 1.2 ulp per entry
                    px.check_kept(k_, N, keep, z[b, h], err + (0 if dt == "f32" else 0.5 * rg.ulp(np.abs(z[b, h]).max(), dt)),
                                  dt, name=f"{name} ({b}, {h})")
                    ref_o[b, h] = probs[b, h, k_] @ V32[b, h, k_]
                    ref_x[b, h] = px.local_v_exact(p[b, h], V[b, h], k_)
                    slack[b, 0, h] = px.local_v_slack(p[b, h], V[b, h], k_, err)
            px.check_out_exact_slack(o.reshape(B, 1, H * d), orc.round_dt(ref_o, dt).reshape(B, 1, H * d),
                                     ref_x.reshape(B, 1, H * d), slack, dt, d, name=name)


# ---- 4. cascade importance over T steps ------------------------------------------------------------------------------
T_STEPS = 32


@pytest.mark.parametrize("dt,regime", [("bf16", "sink24"), ("f32", "large12"), ("f16", "flat")])
def test_cascade_fused_fold_against_exact(dt, regime):
    """attn_decode(..., cascade=) over T = 32 steps of a growing cache (the query of the case at each step's position), the
    last step folded by the flush: acc per head within C err(oracle) + T ulp of sum_t p_exact,t."""
    from spatten_amd import ops
    H, d, P0 = 4, 128, 1200
    cs = _case(1, H, H, d, P0 + T_STEPS - 1, dt, regime)
    B, N = cs.B, cs.N
    cap = N + 3
    tdt = TORCH_DT[dt]
    krc = torch.zeros(B, H, cap, d, dtype=tdt, device="cuda")
    vc = torch.zeros_like(krc)
    krc[:, :, :N], vc[:, :, :N] = dev(cs.kr, dt), dev(cs.vc, dt)
    cos, sin = oracle_table(cap, d, dt)
    c32, s32 = orc.rope_table(cap, d, dt)
    acc = torch.zeros(H, cap, dtype=torch.float32, device="cuda")
    stash = [torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(2)]
    lse = [torch.zeros(B, H, 2, dtype=torch.float32, device="cuda") for _ in range(2)]
    ex_sum = np.zeros((H, cap))
    or_sum = np.zeros((H, cap), np.float32)
    kr64 = cs.kr.astype(np.float64)
    qd = dev(cs.q[:, :, 0], dt)
    for t in range(T_STEPS):
        n = P0 + 1 + t
        cur, prv = t & 1, (t & 1) ^ 1
        ops.attn_decode(qd, None, krc, vc, n, cos, sin, n - 1, scores=stash[cur], lse=lse[cur],
                        cascade=(acc, stash[prv], lse[prv], n - 1) if t > 0 else None)
        qr = orc.apply_rotary_pos_emb_single(cs.q, c32, s32, np.full((B, 1), n - 1), dt)[:, :, 0]
        z = np.einsum("bhd,bhld->bhl", qr.astype(np.float64), kr64[:, :, :n]) / math.sqrt(d)
        p = np.exp(z - z.max(-1, keepdims=True))
        ex_sum[:, :n] += (p / p.sum(-1, keepdims=True)).sum(0)
        st_o = orc.round_dt(orc.round_dt(np.matmul(qr[:, :, None], np.swapaxes(cs.kr[:, :, :n], 2, 3)), dt)
                            / np.float32(math.sqrt(d)), dt)[:, :, 0]
        or_sum[:, :n] = (or_sum[:, :n] + orc.softmax_probs(st_o).sum(0, dtype=np.float32)).astype(np.float32)
    n = P0 + T_STEPS
    ops.importance_accumulate(acc, stash[(T_STEPS - 1) & 1][:, :, None, :n], lse[(T_STEPS - 1) & 1][:, :, None, :])
    torch.cuda.synchronize()
    px.check_cascade(acc.cpu().numpy()[:, :n], or_sum[:, :n], ex_sum[:, :n], T_STEPS, name=f"{dt} {regime}",
                     C=rg.c_for(dt))


@pytest.mark.parametrize("dt,prof,regime", [("bf16", (8, 8), "sink24"), ("f32", (6, 6), "flat"), ("f16", (4, 8), "large4")])
def test_cascade_composed_pq_step_against_exact(dt, prof, regime):
    """attn_decode_pq_local_v(..., cascade=) over T = 32 steps, thresholds cycling through all / none / the median / 2 tau
    below a head's p1max so the flagged set changes between steps; the last step folded by the flush from planes.msb_logit.
    Every step's flags against exact math; acc against sum_t p_exact,t of the decisions taken."""
    from spatten_amd import ops
    kb, vb = prof
    H, d, P0 = 6, 64, 900
    pc = _pc(1, H, H, d, P0 + T_STEPS, dt, regime, kb, vb)
    inp = _from_case(pc)
    B, N = inp.B, inp.N
    c32, s32 = orc.rope_table(inp.cap + 1, d, dt)
    acc = torch.zeros(H, inp.cap, dtype=torch.float32, device="cuda")
    scores = torch.zeros(B, H, inp.cap, dtype=TORCH_DT[dt], device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    prev_lse = torch.zeros_like(lse)
    need_d = torch.zeros(B * H, dtype=torch.int32, device="cuda")
    ex_sum = np.zeros((H, inp.cap))
    or_sum = np.zeros((H, inp.cap), np.float32)
    slack = np.zeros((H, inp.cap))
    flagged = set()
    for t in range(T_STEPS):
        n = P0 + 1 + t
        pl = [x[:, :, :n] for x in inp.planes]
        qr = orc.apply_rotary_pos_emb_single(pc.cs.q, c32, s32, np.full((B, 1), n - 1), dt)[:, :, 0]
        ex0 = px.pq_exact(qr, *pl, 0.0)
        thr = [2.0, 0.0, float(np.median(ex0.p1max)), float(ex0.p1max[0, t % H] * (1 - 2 * ex0.tau[0, t % H]))][t % 4]
        ops.attn_decode_pq_local_v(inp.qd, inp.pl, n, inp.cos, inp.sin, n - 1, thr, max(1, n // 3), scores, lse,
                                   need_lsb=need_d, cascade=(acc, prev_lse, 0 if t == 0 else n - 1))
        torch.cuda.synchronize()
        got = px.check_flags(need_d.cpu().numpy().reshape(B, H), ex0.p1max, thr, ex0.tau, f"step {t}")
        flagged.add(tuple(got.ravel().tolist()))
        ex = px.pq_exact(qr, *pl, thr, need=got)
        _, o_lg = px.pq_oracle(qr, *pl, got)
        ex_sum[:, :n] += ex.p.sum(0)
        slack[:, :n] += px.cascade_slack(ex.p, px.logit_err32(ex.absdot))
        or_sum[:, :n] = (or_sum[:, :n] + orc.softmax_probs(o_lg).sum(0, dtype=np.float32)).astype(np.float32)
    assert len(flagged) >= 3                                                  # the flagged set did change
    n = P0 + T_STEPS
    ops.importance_accumulate(acc, inp.pl.msb_logit[:, :, None, :n], lse[:, :, None, :])       # the flush
    torch.cuda.synchronize()
    px.check_cascade(acc.cpu().numpy()[:, :n], or_sum[:, :n], ex_sum[:, :n], T_STEPS, name=f"{dt} {prof} {regime}",
                     slack=slack[:, :n])
