"""The PQ-keyed prefill (spatten_attn_prefill_pq) and the stash-free prefill importance
(spatten_importance_accumulate_prefill) against EXACT math (tests/pq_exact.py), in the prefill regimes of
tests/regimes.py built in rotated space and packed into the planes by the library.

PQ prefill, every query row of every head: the refetch flag equals the exact one outside the relative band tau (at most 1 % of
the rows inside it, asserted from the float64 reference alone); outputs err <= C err(oracle) + 1 ulp + the P-rounding and fp32
logit allowances, rows inside the band judged against the decision the kernel took; un-flagged rows bit-equal to the
threshold-0 launch, flagged rows bit-equal to the threshold-2 launch in the heads where both walk the same row list (every row flagged, one key range).  Each case
asserts from the flags which pass-2 form its heads took (one key range: more than a quarter of a head's rows flagged;
compacted + key-split + merge: fewer, on kv_len >= 2048).
Importance: per head within C err(oracle) + T ulp of the float64 column sums, the row-sum rule, accumulation onto a non-zero
accumulator, untouched columns beyond kv_len.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests import regimes as rg
from tests.test_gpu_decode import oracle_table
from tests.util import TORCH_DT, dev, host

pytestmark = pytest.mark.gpu

STATS = {}           # worst err / allowance per criterion over the session (printed by every test: run with -s to see it)


def _report(name):
    print(f"\n[{name}] worst err / allowance so far: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(STATS.items())))


@functools.lru_cache(maxsize=None)
def _pc(B, H, Hkv, d, P, ql, dt, regime, causal=True, masked=False, seed=23):
    mask = rg.prefill_mask(B, ql, P + ql, dt, [0, 13, 0][:B], 100, 228) if masked else None
    return px.prefill_case(B, H, Hkv, d, P, ql, dt, regime, seed, mask=mask, causal=causal)


class Inputs:
    """Device form of a px.prefill_case: un-rotated q, values, the planes packed by the LIBRARY from the rotated keys (asserted
    bit exact to orc.pq_quantize), the oracle's rotary table."""

    def __init__(self, pc, extra=5):
        from spatten_amd import ops
        cs, B, Hkv, N, d, dt = pc.cs, pc.B, pc.Hkv, pc.N, pc.d, pc.dt
        self.pc, self.cap = pc, N + extra
        krd = torch.zeros(B, Hkv, self.cap, d, dtype=TORCH_DT[dt], device="cuda")
        self.vd = torch.zeros_like(krd)
        krd[:, :, :N], self.vd[:, :, :N] = dev(cs.kr, dt), dev(cs.vc, dt)
        self.planes = ops.PQPlanes(B, Hkv, self.cap, d, "cuda")
        ops.pq_pack(krd, self.planes, 0, N)
        for g, w in zip(self.planes.unpack(N), pc.planes):
            assert np.array_equal(np.asarray(g).reshape(w.shape), w), "planes not bit exact to the oracle's quantiser"
        self.qd = dev(cs.q, dt)
        self.cos, self.sin = oracle_table(self.cap + 8, d, dt)
        self.mask = None if pc.mask is None else dev(np.ascontiguousarray(pc.mask[:, 0]), dt)

    def run(self, thr, **kw):
        from spatten_amd import ops
        pc = self.pc
        out, need = ops.attn_prefill_pq(self.qd, self.planes, self.vd, pc.N, self.cos, self.sin, pc.P, thr, causal=pc.causal,
                                        mask=self.mask, **kw)
        torch.cuda.synchronize()
        return host(out), need.cpu().numpy().astype(bool)


def _judge_all(inp, ths, name):
    """Every threshold against exact math + the pass structure.  Returns {thr: need}."""
    pc = inp.pc
    sh = (pc.B, pc.ql, pc.H, pc.d)
    o0, n0 = inp.run(0.0)
    o2, n2 = inp.run(2.0)
    assert not n0.any() and n2.all()
    needs = {}
    for thr in ths:
        out, need = inp.run(thr)
        px.check_pq_prefill(pc, thr, out, need, name=f"{name} thr={thr!r}", stats=STATS)
        keep = np.swapaxes(~need, 1, 2)                                         # [B,q,H]
        assert np.array_equal(out.reshape(sh)[keep], o0.reshape(sh)[keep]), f"{name}: pass 2 touched un-flagged rows"
        # a head whose EVERY row is flagged walks the same row list, in the same waves, over the same single key range as the
        # all-flagged launch: bit for bit.  (Partly flagged heads are not comparable bit for bit in either form: pass 2 packs
        # 32 LIST entries into a wave and the deferred maximum moves per wave, so a row's rounding depends on its list neighbours)
        one = need.all(-1)                                                      # [B,H]
        same = np.swapaxes(need & one[..., None], 1, 2)
        assert np.array_equal(out.reshape(sh)[same], o2.reshape(sh)[same]), f"{name}: a flagged row differs from the thr=2 launch"
        needs[thr] = need
    return needs


def _quantile_thr(pc, head, frac):
    """A threshold that flags about ``frac`` of head ``head``'s rows (batch row 0), centred in a gap of its exact p1max."""
    p = np.sort(pc.ex0.p1max[0, head])
    i = max(1, int(frac * p.size))
    return float((p[i - 1] + p[i]) / 2)


REGIMES7 = ("flat", "sink8", "sink24", "rising", "split_winner", "large4", "large12")


@pytest.mark.parametrize("regime", REGIMES7)
def test_pq_prefill_regimes_one_key_range(regime):
    """8 heads, d 128, bf16, 520 query rows (not a multiple of 32) on 300 past keys (not a multiple of 128): kv_len < 2048, so
    pass 2 never splits.  Every threshold of px.prefill_thresholds."""
    pc = _pc(1, 8, 8, 128, 300, 520, "bf16", regime)
    assert px.pq_pass2_ksplit(pc.N) == 1
    _judge_all(Inputs(pc), px.prefill_thresholds(pc.ex0), regime)
    _report(f"one range {regime}")


@pytest.mark.parametrize("regime", ["flat", "sink24", "rising", "large12", "split_winner"])
def test_pq_prefill_regimes_split_refetch_pass(regime):
    """kv_len 2200 (two key ranges), 300 query rows, Hkv 2 of 8: the thresholds of px.prefill_thresholds + one that flags ~12 %
    of head 3's rows — asserted from the flags: head 3 takes the compacted, key-split pass and the merge."""
    pc = _pc(1, 8, 2, 128, 1900, 300, "bf16", regime)
    assert px.pq_pass2_ksplit(pc.N) >= 2
    tq = _quantile_thr(pc, 3, 0.12)
    needs = _judge_all(Inputs(pc), px.prefill_thresholds(pc.ex0) + [tq], regime)
    share = needs[tq][0, 3].mean()
    assert 0 < share < 0.25, share
    _report(f"split {regime}")


def test_pq_prefill_heads_of_every_kind_in_one_launch():
    """5 heads (not a multiple of 8), B 2, q 2000 on kv_len 2300 (the largest case): the queries of head 0 scaled by 8 (confident:
    NO flagged row), of head 1 by 1/2 (flat: every row flagged, one key range), heads 2-4 as they are, the threshold at head
    2's 12 % quantile (compacted + key-split + merge) — one launch, paths asserted from the flags."""
    B, H, d, P, ql, dt = 2, 5, 128, 300, 2000, "bf16"
    base = _pc(B, H, H, d, P, ql, dt, "flat")
    import copy
    pc = copy.copy(base)
    sc = np.array([8, 0.5, 1, 1, 1], np.float32)[None, :, None, None]
    pc.cs = copy.copy(base.cs)
    pc.cs.q, pc.qr = base.cs.q * sc, base.qr * sc            # powers of two: the rotation's roundings commute with them
    pc.ex0 = px.prefill_exact(pc, 0.0)
    thr = _quantile_thr(pc, 2, 0.12)
    needs = _judge_all(Inputs(pc), [thr], "mixed heads")
    share = needs[thr].mean(-1)                              # [B,H]
    assert (share[:, 0] == 0).all() and (share[:, 1] > 0.25).all() and (0 < share[:, 2]).all() and (share[:, 2] < 0.25).all(), share
    _report("mixed heads")


# name: (B, H, Hkv, d, P, ql, dt, regime, causal, masked)
CASES = {
    "mask_bf16_gqa4": (2, 4, 1, 128, 300, 200, "bf16", "sink8", True, True),
    "mask_f16_d64_split": (2, 4, 2, 64, 1900, 200, "f16", "sink24", True, True),
    "gqa8_f16_d64": (1, 8, 1, 64, 140, 330, "f16", "rising", True, False),
    "f16_d64_split_refetch": (1, 4, 4, 64, 1900, 300, "f16", "large12", True, False),
    "causal_off_block_on_past": (1, 4, 2, 128, 333, 200, "bf16", "sink8", False, False),
    "q9": (1, 4, 4, 128, 300, 9, "bf16", "flat", True, False),
    "kv_2047": (1, 4, 4, 128, 1747, 300, "bf16", "flat", True, False),
    "kv_2049": (1, 4, 4, 128, 1749, 300, "bf16", "rising", True, False),
    "first_prompt_q256": (1, 8, 8, 128, 0, 256, "bf16", "sink8", True, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pq_prefill_arguments_and_shapes(name):
    """Arguments and shapes no other test runs.  Explicit mask (causal + keys [100, 228) masked + 13 tokens of left padding
    in batch row 1, passed with causal=False as the plain prefill's tests do): hard-masked entries (finfo_min) take no part, the
    fully masked rows are the uniform average over all keys (max probability 1 / kv_len) — the PQ entry point keeps its logits in
    fp32 under a mask too.  Hkv < H at 4:1 and 8:1; causal=False on a block with P > 0; d 64 and f16, also through the split
    refetch pass; q_len 9 (the plain prefill's flash leg starts there, rows_leg; the PQ entry point has no rows leg: every q_len
    >= 1 takes the flash kernel); kv_len = 2048 -+ 1; a first prompt of one whole 256-row block (row 0 has p1max = 1
    exactly: undecided at threshold 1.0, 1 of 256 rows)."""
    B, H, Hkv, d, P, ql, dt, regime, causal, masked = CASES[name]
    pc = _pc(B, H, Hkv, d, P, ql, dt, regime, causal, masked)
    ths = px.prefill_thresholds(pc.ex0)
    if px.pq_pass2_ksplit(pc.N) >= 2:
        ths.append(_quantile_thr(pc, H - 1, 0.12))
    needs = _judge_all(Inputs(pc), ths, name)
    if px.pq_pass2_ksplit(pc.N) >= 2:
        assert 0 < needs[ths[-1]][0, H - 1].mean() < 0.25
    if masked:
        out, need = Inputs(pc).run(1.5)
        assert np.isfinite(out).all()
        assert need[1, :, :13].all()              # 1 / kv_len < 1.5; their outputs were judged above: the uniform average
    _report(name)


def test_pq_prefill_position_ids():
    """position_ids equal to pos_q0 + arange give the pos_q0 launch bit for bit; shifted by 7 they match the reference built
    for the shifted rotation (the causal rule does not move: it is kv_len - q_len + i)."""
    import copy
    from spatten_amd import ops
    B, H, Hkv, d, P, ql, dt = 2, 4, 2, 128, 300, 200, "bf16"
    pc = _pc(B, H, Hkv, d, P, ql, dt, "sink8")
    inp = Inputs(pc)
    thr = px.prefill_thresholds(pc.ex0)[3]
    o, n = inp.run(thr)
    pos = torch.arange(P, P + ql, device="cuda", dtype=torch.int64)[None].repeat(B, 1)
    o1, n1 = inp.run(thr, position_ids=pos)
    assert np.array_equal(o, o1) and np.array_equal(n, n1)
    c, s = orc.rope_table(inp.cap + 8, d, dt)
    pc2 = copy.copy(pc)
    pc2.qr = orc.apply_rotary_pos_emb_single(pc.cs.q, c, s, np.tile(np.arange(P, P + ql)[None] + 7, (B, 1)), dt)
    pc2.ex0 = px.prefill_exact(pc2, 0.0)
    inp.pc = pc2
    for thr in px.prefill_thresholds(pc2.ex0)[3:6]:
        o2, n2 = inp.run(thr, position_ids=pos + 7)
        px.check_pq_prefill(pc2, thr, o2, n2, name=f"shifted positions thr={thr!r}", stats=STATS)
    _report("position_ids")


# ---- the stash-free prefill importance ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cs(B, H, Hkv, d, P, ql, dt, regime, causal=True):
    return rg.make_case(B, H, Hkv, d, P, ql, dt, regime, 23, mask=orc.causal_mask(B, ql, P + ql, dt) if causal else None)


def _importance(cs, causal, acc, pos=None, stash=False):
    from spatten_amd import ops
    B, H, Hkv, d, P, ql, N, dt = cs.B, cs.H, cs.Hkv, cs.d, cs.P, cs.ql, cs.N, cs.dt
    krd = torch.zeros(B, Hkv, N + 3, d, dtype=TORCH_DT[dt], device="cuda")
    vd = torch.zeros_like(krd)
    krd[:, :, :N], vd[:, :, :N] = dev(cs.kr, dt), dev(cs.vc, dt)
    cos, sin = oracle_table(N + 16, d, dt)
    qd = dev(cs.q, dt)
    lse = torch.zeros(B, H, ql, 2, dtype=torch.float32, device="cuda")
    st = torch.zeros(B, H, ql, N, dtype=TORCH_DT[dt], device="cuda") if stash else None
    ops.attn_prefill(qd, krd, vd, N, cos, sin, P, causal=causal, position_ids=pos, lse=lse, scores=st, numerics="reference")
    run = lambda: ops.importance_accumulate_prefill(acc, qd, krd, N, cos, sin, P, lse, causal=causal, position_ids=pos)
    run()
    torch.cuda.synchronize()
    return run, host(lse), (None if st is None else host(st))


IMP_CASES = [("bf16", 128, 3, 4, 2, 300, 700, "flat", True), ("bf16", 128, 3, 4, 2, 300, 700, "rising", True),
             ("bf16", 128, 2, 8, 2, 300, 700, "sink24", True), ("f16", 64, 3, 4, 1, 300, 700, "large12", True),
             ("f16", 64, 2, 4, 2, 300, 700, "split_winner", True), ("bf16", 64, 2, 4, 2, 333, 200, "sink24", False),
             ("f16", 128, 3, 4, 4, 0, 333, "flat", True), ("bf16", 128, 2, 4, 2, 300, 700, "large12", False)]


@pytest.mark.parametrize("dt,d,B,H,Hkv,P,ql,regime,causal", IMP_CASES)
def test_prefill_importance_against_exact_math(dt, d, B, H, Hkv, P, ql, regime, causal):
    """q 700 on 300 past keys: the 256-key blocks lie wholly below the diagonal (block 0), across it (block 1) and above it
    (blocks 2, 3: the first_q clamp starts them at query tiles 1 and 3); q_len not a multiple of 128 / 32, kv_len 1000 not of
    256 / 32.  The accumulator starts NON-zero, with sentinels beyond kv_len (bit for bit untouched); a second call adds the
    same contribution again."""
    cs = _cs(B, H, Hkv, d, P, ql, dt, regime, causal)
    N = cs.N
    rng = np.random.default_rng(7)
    acc0 = rng.uniform(0.0, 3.0, (H, N + 9)).astype(np.float32)
    acc0[:, N:] = np.float32(-12345.678)
    acc = torch.from_numpy(acc0.copy()).cuda()
    run, _, _ = _importance(cs, causal, acc)
    got = host(acc)
    assert np.array_equal(got[:, N:], acc0[:, N:])
    px.check_colprob(got, cs, causal, acc0=acc0, name=f"{regime} {dt}", stats=STATS)
    run()
    torch.cuda.synchronize()
    got2 = host(acc)
    assert np.array_equal(got2[:, N:], acc0[:, N:])
    px.check_colprob(got2, cs, causal, acc0=acc0, calls=2, name=f"{regime} {dt} twice", stats=STATS)
    # a zero accumulator: the plain column sums
    z = torch.zeros(H, N, dtype=torch.float32, device="cuda")
    _importance(cs, causal, z)
    px.check_colprob(host(z), cs, causal, name=f"{regime} {dt} from zero", stats=STATS)
    _report(f"importance {regime} {dt}")


def test_prefill_importance_position_ids():
    cs = _cs(2, 4, 2, 128, 300, 200, "bf16", "sink24")
    pos = torch.arange(cs.P, cs.N, device="cuda", dtype=torch.int64)[None].repeat(cs.B, 1)
    z = torch.zeros(cs.H, cs.N, dtype=torch.float32, device="cuda")
    _importance(cs, True, z, pos=pos)
    px.check_colprob(host(z), cs, True, name="position_ids", stats=STATS)


@pytest.mark.parametrize("dt,d", [("bf16", 128), ("f16", 64)])
def test_prefill_row_statistics_handed_to_the_importance(dt, d):
    """The (m, l) the importance kernel reads are the flash kernel's own: exp(stash - m) / l of the same launch's stash sums to 1
    per row and equals the softmax of the stash; m may be a DEFERRED maximum (up to rg.DEFER_MAX below the row's true maximum),
    never above it."""
    cs = _cs(2, 4, 2, d, 100, 150, dt, "rising")
    z = torch.zeros(cs.H, cs.N, dtype=torch.float32, device="cuda")
    _, lse, st = _importance(cs, True, z, stash=True)
    vis = px.prefill_visibility(cs.B, cs.ql, cs.N, cs.P, True, None, dt)[0]
    s = np.where(vis, st.astype(np.float64), -np.inf)
    m, l = lse[..., 0].astype(np.float64), lse[..., 1].astype(np.float64)
    true = s.max(-1)
    assert (m <= true).all() and (m >= true - rg.DEFER_MAX).all()
    p = np.exp(s - m[..., None]) / l[..., None]
    np.testing.assert_allclose(p.sum(-1), 1.0, rtol=2e-6 * 16)
    want = orc.softmax_probs(np.where(vis, st, -np.inf).astype(np.float32))
    np.testing.assert_allclose(p, want, rtol=2e-3, atol=1e-6)
