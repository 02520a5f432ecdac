"""The cascade step of a RAGGED batch over the profiled planes (spatten_attn_decode_pq_cascade_ragged,
ops.attn_decode_pqv(step=StepState(batch=B), cascade=(acc [B,H,L], prev_lse, _))): progressive quantisation and the cumulative
token importance in one step, one step state and one accumulator per sequence.

Yardsticks.  (1) The fold does not disturb the step: out, stash, lse, need_lsb, head_abs equal to the ragged plain step on clones,
bit for bit.  (2) Sequence b of every step equals today's shared-state spatten_attn_decode_pq_cascade at batch 1 on sequence b's
slices (its own StepState at the same length and position, same splits, laid out for the bound): out row, stash, lse, prev_lse,
need_lsb, msb_logit and acc[b], bit for bit.  (3) acc[b] equals the library's own fold (ops.importance_accumulate of the fp32 logit
rows and lse) of sequence b's earlier steps, one call per step, and again after the flush through
ops.importance_accumulate_step(acc, msb_logit, lse, msb_logit, lse); the first step after a set folds nothing.  (4) acc[b] against
float64 exact math (pq_exact.check_cascade with the slack rule of tests/pq_cascade_case.py, per sequence), flags by
pq_exact.check_flags.  (5) Sentinels: accumulator entries at or past the folded rows, rows of pruned heads, stash / msb_logit
entries [len_b, bound), and the guard bands of a padded accumulator view.  (6) One captured graph of a token.  (7) A whole turn:
steps, flush, ragged prune event, repack of the planes, set from device lengths, more steps — against the per-sequence schedule
driven from host integers.

Shapes: bound 704, three steps, lengths after step t = (702 + t, 351 + t, 350 + t, 234 + t, 1 + t): the rows the fold reads end on
the 352 | 353 chunk edge of two splits, one past it, beside a three-split edge (235 | 236), inside a tile, and one sequence starts
from the appended row alone.  Thresholds 0.0, 2.0 and one in between picked on the CPU so that over the (step, sequence) pairs
one has more than half of its launched heads flagged and one some but at most half (the compact refetch pass's two layouts) and
every |p1max - thr| > 1e-3.  Needs an MI355X."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_exact as px
from tests.strided import Guards, padded
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_ragged_pq import (BAND, CAP, LOGIT_FILL, OUT_FILL, POS_OFF, STASH_FILL, TABLE_ROWS, Buffers, oracle_sequence,
                                      rotated)
from tests.util import OUT_TOL, TORCH_DT, dev, host

pytestmark = pytest.mark.gpu

T = 3
START = (701, 350, 349, 233, 0)           # cache lengths before the first token
ACC_FILL, PREV_FILL = -3.0, 3.0

# (name, key bits, value bits, dtype, d, H, Hkv, head list, head_abs, query_bits, seed): tests/test_gpu_ragged_pq.py's tuple
ROUTES = [
    ("p88-bf16", 8, 8, "bf16", 128, 4, 4, None, False, None, 0),
    ("p48-f16-d64", 4, 8, "f16", 64, 8, 4, None, False, None, 0),
    ("p66-bf16-gqa", 6, 6, "bf16", 128, 8, 2, None, False, None, 0),
    ("p88-f32", 8, 8, "f32", 128, 4, 2, None, False, None, 0),
    ("p88-head-list", 8, 8, "bf16", 128, 4, 4, (0, 2, 3), True, None, 0),
]
ROUTE_IDS = [r[0] for r in ROUTES]


def lens_at(t):
    """cache lengths after step t's append"""
    return tuple(n + t + 1 for n in START)


def pick_mid_threshold(p1max):
    """p1max [rows, launched heads]: a midpoint between neighbouring values that meets the docstring's conditions, or None."""
    vals = np.unique(p1max)
    half = p1max.shape[1]
    for thr in (vals[:-1] + vals[1:]) / 2:
        cnt = (p1max < thr).sum(1)
        if np.abs(p1max - thr).min() > BAND and (2 * cnt > half).any() and ((cnt > 0) & (2 * cnt <= half)).any():
            return float(thr)
    return None


_CASES = {}


def case(route):
    """Host inputs of a route and the oracle's view of every (step, sequence), computed once and shared (never modified)."""
    name, kb, vb, dt, d, H, Hkv, hlist, _, _, seed = route
    if name in _CASES:
        return _CASES[name]
    B, G = len(START), H // Hkv
    s = 9800 + 7 * H + Hkv + d + kb + 1000 * seed
    full = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n + T, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n + T, d), dt))
            for b, n in enumerate(START)]
    live = list(range(H)) if hlist is None else list(hlist)
    toks, seqs = [], []
    for t in range(T):
        q = orc.synth_normal(s, 200 + t, (B, H, d), dt)
        kn = np.stack([full[b][0][:, START[b] + t] for b in range(B)])
        vn = np.stack([full[b][1][:, START[b] + t] for b in range(B)])
        toks.append((q, kn, vn))
        seqs.append([oracle_sequence(q[b], full[b][0][:, :n], full[b][1][:, :n], n - 1 + POS_OFF[b], kb, vb, G, dt, None)
                     for b, n in enumerate(lens_at(t))])
    p1max = np.stack([np.stack([sq[2] for sq in row]) for row in seqs])            # [T, B, H]
    c = dict(full=full, toks=toks, seqs=seqs, live=live, p1max=p1max, mid=pick_mid_threshold(p1max[:, :, live].reshape(T * B, -1)),
             logits={}, refs={})
    _CASES[name] = c
    return c


def exact_step(c, t, b, need):
    """One (step, sequence) at the decision taken: (exact probabilities [H, n] f64, the oracle's fp32 probabilities [H, n], the slack
    of tests/pq_cascade_case.references [H, n]) and the exact view at threshold 0 (for the flags)."""
    key = (t, b, need.tobytes())
    if key not in c["refs"]:
        planes, qr, _ = c["seqs"][t][b]
        if (t, b) not in c["logits"]:
            c["logits"][(t, b)] = (orc.pq_decode_attention_profile(qr, *planes, 0.0)[2], orc.pq_decode_attention_profile(qr, *planes, 2.0)[2],
                                   px.pq_exact(qr, *planes, 0.0))
        l0, l1, ex0 = c["logits"][(t, b)]
        ex = px.pq_exact(qr, *planes, 0.0, need=need[None])
        o_lg = np.where(need[None, :, None], l1, l0)
        c["refs"][key] = (ex.p.sum(0), orc.softmax_probs(o_lg).sum(0, dtype=np.float32),
                          px.cascade_slack(ex.p, px.logit_err32(ex.absdot)), ex0)
    return c["refs"][key]


def check_exact(c, needs, acc, msg):
    """acc [B, H, CAP] after the flush against float64 exact math, per sequence: pq_cascade_case.references' sums and slack."""
    live = c["live"]
    H = acc.shape[1]
    for b in range(len(START)):
        N = lens_at(T - 1)[b]
        ex_sum, or_sum, slack = np.zeros((H, N)), np.zeros((H, N), np.float32), np.zeros((H, N))
        for t in range(T):
            n = lens_at(t)[b]
            p, po, sl, _ = exact_step(c, t, b, needs[t][b])
            ex_sum[:, :n] += p
            slack[:, :n] += sl
            or_sum[:, :n] = (or_sum[:, :n] + po).astype(np.float32)
        px.check_cascade(acc[b][live, :N], or_sum[live], ex_sum[live], T, name=f"{msg} b={b}", slack=slack[live])


def check_flags(c, t, thr, need, msg):
    for b in range(len(START)):
        planes, qr, _ = c["seqs"][t][b]
        if (t, b) not in c["logits"]:
            exact_step(c, t, b, need[b])
        ex0 = c["logits"][(t, b)][2]
        live = c["live"]
        px.check_flags(need[b][None][:, live], ex0.p1max[:, live], thr, ex0.tau[:, live], f"{msg} b={b}")


class Casc:
    """The cascade buffers of a ragged batch: acc [B, H, CAP] fp32 (zero where a fold may land, ACC_FILL from the last step's length on
    and in every row of a pruned head) and prev_lse [B, H, 2]."""

    def __init__(self, B, H, dead, final_lens):
        self.acc = torch.zeros(B, H, CAP, dtype=torch.float32, device="cuda")
        for b, n in enumerate(final_lens):
            self.acc[b, :, n:] = ACC_FILL
        if dead:
            self.acc[:, dead] = ACC_FILL
        self.prev = torch.full((B, H, 2), PREV_FILL, dtype=torch.float32, device="cuda")


def plain_step(buf, route, q, cos, sin, ws, n_splits, thr, ids, step):
    from spatten_amd import ops
    ops.attn_decode_pqv(q, buf.planes(), CAP, cos, sin, 0, thr, out=buf.out, need_lsb=buf.need, scores=buf.st, lse=buf.lse,
                        head_ids=ids, head_abs=buf.habs if route[8] else None, step=step, n_splits=n_splits, workspace=ws)


def cascade_step(buf, route, q, cos, sin, ws, n_splits, thr, ids, step, acc, prev, b=None):
    """The ragged launch (b None: acc [B, H, CAP]) or today's shared-state call on sequence b's slices (acc [H, CAP])."""
    from spatten_amd import ops
    B, H = buf.lse.shape[:2]
    sl = slice(None) if b is None else slice(b, b + 1)
    need = buf.need if b is None else buf.need.view(B, H)[b]
    habs = None if not route[8] else buf.habs if b is None else buf.habs.view(B, H)[b]
    ops.attn_decode_pqv(q[sl], buf.planes(b), CAP, cos, sin, 0, thr, out=buf.out[sl], need_lsb=need, scores=buf.st[sl], lse=buf.lse[sl],
                        head_ids=ids, head_abs=habs, step=step, n_splits=n_splits, workspace=ws, cascade=(acc, prev[sl], 0))


def fold_reference(ref_b, lg, lse, live, all_heads):
    """The library's fold of one step of one sequence into ref_b [H, CAP]: lg [1, H, n] fp32 logits, lse [1, H, 2]."""
    from spatten_amd import ops
    if all_heads:
        ops.importance_accumulate(ref_b, lg[:, :, None, :], lse[:, :, None, :])
        return
    # a head list: the launched heads alone (0 + p = p exactly, then the one add the kernel makes)
    tmp = torch.zeros(len(live), ref_b.shape[1], dtype=torch.float32, device="cuda")
    ops.importance_accumulate(tmp, lg[:, live][:, :, None, :].contiguous(), lse[:, live][:, :, None, :].contiguous())
    ref_b[live] += tmp


@pytest.mark.parametrize("n_splits", [1, 2, 3])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_ragged_cascade_steps(route, n_splits):
    from spatten_amd import ops
    name, kb, vb, dt, d, H, Hkv, hlist, use_habs, _, _ = route
    c = case(route)
    B, live = len(START), c["live"]
    # ---- the condition on the inputs, on CPU values, before anything is launched
    assert c["mid"] is not None, f"{name}: no threshold meets the conditions — pick another seed"
    p1 = c["p1max"][:, :, live].reshape(T * B, -1)
    for thr in (0.0, 2.0, c["mid"]):
        assert np.abs(p1 - thr).min() > BAND, (name, thr)
    cnt = (p1 < c["mid"]).sum(1)
    assert (2 * cnt > len(live)).any() and ((cnt > 0) & (2 * cnt <= len(live))).any(), (name, cnt)

    dead = [h for h in range(H) if h not in live]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    ids = None if hlist is None else torch.tensor(hlist, dtype=torch.int32, device="cuda")
    ws, ws1 = ops.DecodeWorkspace(B, H, d, "cuda"), ops.DecodeWorkspace(1, H, d, "cuda")
    base = Buffers(kb, vb, dt, d, H, Hkv, B)
    base.fill_past(c["full"], lens_at(0), dt, cos, sin)                         # rows [0, START[b]) of sequence b
    pos0 = [n + o - 1 for n, o in zip(START, POS_OFF)]
    toks = [tuple(dev(x, dt) for x in tk) for tk in c["toks"]]
    for thr in (0.0, 2.0, c["mid"]):
        rag, seq = base.clone(), base.clone()
        init = Casc(B, H, dead, lens_at(T - 1))
        acc, parent, mask = padded(init.acc, (1, 2, 24))                        # a non-trivial acc_batch_stride and acc_sh
        assert acc.stride(0) != H * CAP and acc.stride(1) != CAP and acc.stride(2) == 1
        guards = Guards()
        guards.add("acc", parent, mask)
        guards.snapshot()
        prev = init.prev.clone()
        one = Casc(B, H, dead, lens_at(T - 1))                                  # the per-sequence schedule's buffers (dense)
        ref = init.acc.clone()                                                  # the library's fold
        step = ops.StepState(cos, sin, batch=B)
        step.set(list(START), pos0)
        ones = [ops.StepState(cos, sin) for _ in range(B)]
        for b in range(B):
            ones[b].set(START[b], pos0[b])
        pend, needs = [None] * B, []
        for t in range(T):
            q, kn, vn = toks[t]
            lens = lens_at(t)
            msg = f"{name} S={n_splits} thr={thr} t={t}"
            step.advance()
            ops.kv_append_planes(kn, vn, rag.kc, rag.krc, rag.vc, rag.planes(), 0, cos, sin, step=step)
            plain = rag.clone()
            plain_step(plain, route, q, cos, sin, ws, n_splits, thr, ids, step)
            cascade_step(rag, route, q, cos, sin, ws, n_splits, thr, ids, step, acc, prev)
            for b in range(B):
                ones[b].advance()
                ops.kv_append_planes(kn[b:b + 1], vn[b:b + 1], seq.kc[b:b + 1], seq.krc[b:b + 1], seq.vc[b:b + 1], seq.planes(b), 0,
                                     cos, sin, step=ones[b])
                cascade_step(seq, route, q, cos, sin, ws1, n_splits, thr, ids, ones[b], one.acc[b], one.prev, b)
                if pend[b] is not None:
                    fold_reference(ref[b], *pend[b], live, hlist is None)
            torch.cuda.synchronize()
            ws.check()
            ws1.check()
            # (1) the step is undisturbed
            for k in ("out", "st", "lse", "need", "habs"):
                assert torch.equal(getattr(rag, k), getattr(plain, k)), (msg, k)
            # (2) every sequence is the shared-state call's: every buffer whole (the sentinels are the same on both sides)
            for k in Buffers.NAMES:
                assert torch.equal(getattr(rag, k), getattr(seq, k)), (msg, k)
            assert torch.equal(acc, one.acc) and torch.equal(prev, one.prev), msg
            words = step.read(all_words=True)
            assert [w[:4] for w in words] == [ones[b].read(all_words=True)[:4] for b in range(B)], msg
            assert [w[0] for w in words] == list(lens) and [w[3] for w in words] == ([0] * B if t == 0 else list(lens_at(t - 1))), msg
            # (3) the accumulator is the library's fold of the earlier steps (t = 0: of nothing)
            assert torch.equal(acc, ref), msg
            assert torch.equal(prev[:, live], rag.lse[:, live]), msg
            # (5) untouched: past the folded rows, past the lengths, pruned heads
            for b, n in enumerate(lens):
                folded = 0 if t == 0 else lens_at(t - 1)[b]
                assert torch.equal(acc[b, :, folded:], init.acc[b, :, folded:]), (msg, b)
                assert (rag.st[b, :, n:] == STASH_FILL).all() and (rag.lg[b, :, n:] == LOGIT_FILL).all(), (msg, b)
                assert (acc[b, :, lens_at(T - 1)[b]:] == ACC_FILL).all(), (msg, b)
            if dead:
                assert (acc[:, dead] == ACC_FILL).all() and (prev[:, dead] == PREV_FILL).all(), msg
                assert (rag.out.view(B, H, d)[:, dead] == OUT_FILL).all() and (rag.st[:, dead] == STASH_FILL).all(), msg
                assert (rag.lg[:, dead] == LOGIT_FILL).all() and (rag.lse[:, dead] == -1.0).all(), msg
            need = rag.need.view(B, H).cpu().numpy().astype(bool)
            check_flags(c, t, thr, need, msg)                                   # (4) the flags
            differs = (rag.lg != plain.lg).any(-1)                              # only flagged heads may differ from the plain step's
            assert not differs[~torch.from_numpy(need).cuda()].any(), msg       # MSB-only logits: they hold their FINAL logits
            needs.append(need)
            pend = [(rag.lg[b:b + 1, :, :n].clone(), rag.lse[b:b + 1].clone()) for b, n in enumerate(lens)]
        guards.check()
        # ---- the flush: msb_logit / lse as both buffer pairs
        msg = f"{name} S={n_splits} thr={thr} flush"
        ops.importance_accumulate_step(acc, rag.lg, rag.lse, rag.lg, rag.lse, step, CAP)
        for b in range(B):
            fold_reference(ref[b], *pend[b], live, hlist is None)
        torch.cuda.synchronize()
        guards.check()
        assert torch.equal(acc[:, live], ref[:, live]), msg
        for b, n in enumerate(lens_at(T - 1)):
            assert (acc[b, :, n:] == ACC_FILL).all(), (msg, b)
        check_exact(c, needs, acc.cpu().numpy(), msg)                           # (4) exact math
    ops.check_workspaces()


GRAPH_ROUTE = ROUTES[0]


def test_a_token_of_the_ragged_cascade_as_one_captured_graph():
    """[advance, kv_append_planes (ragged), the cascade step] captured ONCE, replayed for the three steps with fresh q / k_new /
    v_new: every buffer, the accumulator, prev_lse and the state words equal the same calls issued eagerly, bit for bit."""
    from spatten_amd import ops
    route = GRAPH_ROUTE
    name, kb, vb, dt, d, H, Hkv = route[:7]
    c = case(route)
    assert c["mid"] is not None, "no threshold meets the conditions — pick another seed"
    B, n_splits, thr = len(START), 2, c["mid"]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    base = Buffers(kb, vb, dt, d, H, Hkv, B)
    base.fill_past(c["full"], lens_at(0), dt, cos, sin)
    init = Casc(B, H, [], lens_at(T - 1))
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    tdt = TORCH_DT[dt]
    q, kn, vn = (torch.zeros(B, H, d, dtype=tdt, device="cuda"), torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"),
                 torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"))
    sets = {kind: (base.clone(), ops.StepState(cos, sin, batch=B), Casc(B, H, [], lens_at(T - 1))) for kind in ("graph", "eager")}
    pos0 = [n + o - 1 for n, o in zip(START, POS_OFF)]

    def token(kind):
        buf, step, cs = sets[kind]
        step.advance()
        ops.kv_append_planes(kn, vn, buf.kc, buf.krc, buf.vc, buf.planes(), 0, cos, sin, step=step)
        cascade_step(buf, route, q, cos, sin, ws, n_splits, thr, None, step, cs.acc, cs.prev)

    def reset(kind):
        buf, step, cs = sets[kind]
        buf.copy_from(base)
        cs.acc.copy_(init.acc)
        cs.prev.copy_(init.prev)
        step.set(list(START), pos0)

    reset("graph")
    token("graph")                                         # warm-up outside the capture
    torch.cuda.synchronize()
    reset("graph"); reset("eager")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        token("graph")
    reset("graph")                                         # (nothing ran during the capture; states as set)
    flagged = 0
    for t in range(T):
        for dst, src in zip((q, kn, vn), c["toks"][t]):
            dst.copy_(dev(src, dt))
        gr.replay()
        token("eager")
        torch.cuda.synchronize()
        ws.check()
        (g_, gs, gc), (e_, es, ec) = sets["graph"], sets["eager"]
        assert gs.read(all_words=True) == es.read(all_words=True), t
        assert [w[0] for w in gs.read(all_words=True)] == list(lens_at(t)), t
        for k in Buffers.NAMES:
            assert torch.equal(getattr(g_, k), getattr(e_, k)), (t, k)
        assert torch.equal(gc.acc, ec.acc) and torch.equal(gc.prev, ec.prev), t
        assert bool((gc.acc[:, :, :1] != 0).any()) == (t > 0)   # (the replay did fold)
        flagged += int(g_.need.sum())
    assert 0 < flagged < T * B * H
    ops.check_workspaces()


# ------------------------------------------------------------------------------------------------
# A whole turn: three steps, the flush, ONE ragged prune event for both layers, the planes repacked, the states set from device
# lengths, two more steps — against the same schedule per sequence from host integers through today's single-sequence calls
# ------------------------------------------------------------------------------------------------
E_START, E_RECENT, E_K, E_NC = 4, 8, 16, 1                   # keep_rows 27: lengths 63 and 36 prune, 19 does not
E_BOUND, E_CAP2 = 96, 32                                     # rows of the planes before / after the event
E_LENS0 = (60, 33, 16)                                       # cache lengths before the first token
E_LAYERS, E_H, E_D, E_STEPS1, E_STEPS2 = 2, 4, 128, 3, 2
E_THR = 0.12


class Layer:
    """One layer's caches, planes and step outputs for `B` sequences and `rows` rows."""

    def __init__(self, B, rows, tdt, seed=None, lens=None, cos=None, sin=None):
        from spatten_amd import ops
        z = lambda *s, dtype=tdt: torch.zeros(*s, dtype=dtype, device="cuda")
        self.B, self.rows = B, rows
        self.kc, self.krc, self.vc = z(B, E_H, rows, E_D), z(B, E_H, rows, E_D), z(B, E_H, rows, E_D)
        self.planes = ops.PQProfilePlanes(B, E_H, E_H, rows, E_D, "cuda", key_bits=8, value_bits=8)
        self.st, self.out = z(B, E_H, rows), z(B, E_H * E_D)
        self.lse, self.prev = z(B, E_H, 2, dtype=torch.float32), z(B, E_H, 2, dtype=torch.float32)
        self.acc = z(B, E_H, rows, dtype=torch.float32)
        self.need = torch.full((B * E_H,), -1, dtype=torch.int32, device="cuda")
        self.ws = ops.DecodeWorkspace(B, E_H, E_D, "cuda")
        if seed is not None:
            g = torch.Generator(device="cuda").manual_seed(seed)
            for b, n in enumerate(lens):
                self.kc[b, :, :n] = torch.randn(E_H, n, E_D, device="cuda", generator=g).to(tdt)
                self.vc[b, :, :n] = torch.randn(E_H, n, E_D, device="cuda", generator=g).to(tdt)
                ops.build_shadow(self.kc[b:b + 1], self.krc[b:b + 1], 0, n, cos, sin)
            ops.pq_pack_planes(self.krc, self.vc, self.planes, 0, rows)

    PLANES = ("msb", "lsb", "scale", "vq", "vscale", "msb_logit")

    def sequence(self, b):
        """a copy of sequence b alone"""
        from spatten_amd import ops
        c = Layer(1, self.rows, self.kc.dtype)
        for k in ("kc", "krc", "vc", "st", "out", "lse", "prev", "acc"):
            getattr(c, k).copy_(getattr(self, k)[b:b + 1])
        for k in self.PLANES:
            getattr(c.planes, k).copy_(getattr(self.planes, k)[b:b + 1])
        return c

    def clone(self):
        c = Layer(self.B, self.rows, self.kc.dtype)
        for k in ("kc", "krc", "vc", "st", "out", "lse", "prev", "acc", "need"):
            getattr(c, k).copy_(getattr(self, k))
        for k in self.PLANES:
            getattr(c.planes, k).copy_(getattr(self.planes, k))
        return c


def layer_step(L, q, kn, vn, step, bound, cos, sin, acc):
    from spatten_amd import ops
    ops.kv_append_planes(kn, vn, L.kc, L.krc, L.vc, L.planes, 0, cos, sin, step=step)
    ops.attn_decode_pqv(q, L.planes, bound, cos, sin, 0, E_THR, out=L.out, need_lsb=L.need, scores=L.st, lse=L.lse, step=step,
                        n_splits=2, workspace=L.ws, cascade=(acc, L.prev, 0))


@contextlib.contextmanager
def no_host_reads():
    """torch.Tensor.item / .cpu / .tolist raise inside: the ragged turn has no host value of a length."""
    def refuse(*a, **k):
        raise AssertionError("the ragged turn read a device value on the host")
    names = ("item", "cpu", "tolist")
    own = {n: torch.Tensor.__dict__[n] for n in names if n in torch.Tensor.__dict__}
    for n in names:
        setattr(torch.Tensor, n, refuse)
    try:
        yield
    finally:
        for n in names:
            if n in own:
                setattr(torch.Tensor, n, own[n])
            else:
                delattr(torch.Tensor, n)                     # (inherited from the C base class again)


def test_a_whole_cascade_pruned_turn_of_a_ragged_batch_over_the_planes():
    from spatten_amd import ops
    dt, B = "bf16", len(E_LENS0)
    tdt = TORCH_DT[dt]
    cos, sin = oracle_table(E_BOUND + 8, E_D, dt)
    keep = E_START + E_K + E_RECENT - E_NC
    g = torch.Generator(device="cuda").manual_seed(91)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(tdt)
    toks = [[(rnd(B, E_H, E_D), rnd(B, E_H, E_D), rnd(B, E_H, E_D)) for _ in range(E_LAYERS)] for _ in range(E_STEPS1 + E_STEPS2)]
    layers0 = [Layer(B, E_BOUND, tdt, seed=15 + i, lens=E_LENS0, cos=cos, sin=sin) for i in range(E_LAYERS)]
    lens1 = [n + E_STEPS1 for n in E_LENS0]
    want_lens = [keep if n + E_NC > E_START + E_K + E_RECENT else n for n in lens1]
    assert sum(n == keep for n in want_lens) == 2 and want_lens[2] == lens1[2]

    # ---------------- the ragged schedule ----------------
    rag = [L.clone() for L in layers0]
    step = ops.StepState(cos, sin, batch=B)
    step.set(list(E_LENS0), [n - 1 for n in E_LENS0])
    outs = []
    with no_host_reads():
        for t in range(E_STEPS1):
            step.advance()
            for L, (q, kn, vn) in zip(rag, toks[t]):
                layer_step(L, q, kn, vn, step, E_BOUND, cos, sin, L.acc)
        for L in rag:
            ops.importance_accumulate_step(L.acc, L.planes.msb_logit, L.lse, L.planes.msb_logit, L.lse, step, E_BOUND)
        Kn, Vn, Krn, idx, new_lens, accs = ops.prune_ragged([L.acc for L in rag], [L.kc for L in rag], [L.vc for L in rag], step.lengths(),
                                                            E_BOUND, E_START, E_RECENT, E_K, E_NC, E_CAP2, (cos, sin),
                                                            acc=[L.acc for L in rag])
        rag2 = []
        for l in range(E_LAYERS):
            L2 = Layer(B, E_CAP2, tdt)
            L2.kc, L2.vc, L2.krc, L2.acc = Kn[l], Vn[l], Krn[l], accs[l]
            ops.pq_pack_planes(L2.krc, L2.vc, L2.planes, 0, E_CAP2)       # (zero rows behind the new lengths pack with scale 1.0)
            rag2.append(L2)
        event = [L2.clone() for L2 in rag2]                               # what the event left, before the next steps write rows
        step.set(new_lens, new_lens - 1)                                  # device tensors: no host value of a length
        for t in range(E_STEPS1, E_STEPS1 + E_STEPS2):
            step.advance()
            for L, (q, kn, vn) in zip(rag2, toks[t]):
                layer_step(L, q, kn, vn, step, E_CAP2, cos, sin, L.acc)
            outs.append([L.out.clone() for L in rag2])
    torch.cuda.synchronize()
    for L in rag + rag2:
        L.ws.check()
    assert new_lens.tolist() == want_lens
    assert [r[0] for r in step.read()] == [n + E_STEPS2 for n in want_lens]

    # ---------------- the same schedule per sequence, from host integers ----------------
    for b in range(B):
        sl = slice(b, b + 1)
        S = [L0.sequence(b) for L0 in layers0]
        one = ops.StepState(cos, sin)
        one.set(E_LENS0[b], E_LENS0[b] - 1)
        for t in range(E_STEPS1):
            one.advance()
            for L, (q, kn, vn) in zip(S, toks[t]):
                layer_step(L, q[sl], kn[sl], vn[sl], one, E_BOUND, cos, sin, L.acc[0])
        n = lens1[b]
        for L in S:
            ops.importance_accumulate(L.acc[0], L.planes.msb_logit[:, :, None, :n], L.lse[:, :, None, :])
        accs_b = [L.acc[0] for L in S]
        if n + E_NC > E_START + E_K + E_RECENT:
            m, hi = keep, n - E_RECENT + E_NC
            acc_n = [torch.zeros(E_H, E_CAP2, dtype=torch.float32, device="cuda") for _ in S]
            Kb, Vb, Krb, _ = ops.prune_layers(accs_b, [L.kc for L in S], [L.vc for L in S], n, E_START, hi, E_K, capacity=E_CAP2,
                                              rope=(cos, sin), acc=(accs_b, acc_n))
        else:
            m = n
            empty = torch.empty(E_H, 0, dtype=torch.int32, device="cuda")
            res = [ops.kv_compact(L.kc, L.vc, empty, n, n, L=n, capacity=E_CAP2, rope=(cos, sin)) for L in S]
            Kb, Vb, Krb, acc_n = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], accs_b
        S2 = []
        for l in range(E_LAYERS):
            P2 = Layer(1, E_CAP2, tdt)
            P2.kc[:, :, :m], P2.vc[:, :, :m], P2.krc[:, :, :m] = Kb[l][:, :, :m], Vb[l][:, :, :m], Krb[l][:, :, :m]
            P2.acc[0, :, :m] = acc_n[l][:, :m]
            ops.pq_pack_planes(P2.krc, P2.vc, P2.planes, 0, E_CAP2)
            S2.append(P2)
        torch.cuda.synchronize()
        for l in range(E_LAYERS):                                         # the event and the repack
            msg = f"event layer {l} b={b}"
            for k in ("kc", "vc", "krc", "acc"):
                assert torch.equal(getattr(event[l], k)[sl], getattr(S2[l], k)), (msg, k)
            for k in Layer.PLANES[:5]:
                assert torch.equal(getattr(event[l].planes, k)[sl], getattr(S2[l].planes, k)), (msg, k)
            assert torch.isfinite(event[l].planes.scale).all() and torch.isfinite(event[l].planes.vscale).all(), msg
        one.set(m, m - 1)
        for t in range(E_STEPS1, E_STEPS1 + E_STEPS2):
            one.advance()
            for l, (L, (q, kn, vn)) in enumerate(zip(S2, toks[t])):
                layer_step(L, q[sl], kn[sl], vn[sl], one, E_CAP2, cos, sin, L.acc[0])
                torch.cuda.synchronize()
                msg = f"step {t} layer {l} b={b}"
                assert torch.equal(outs[t - E_STEPS1][l][sl], L.out), msg
                # ---- the oracle on the repacked planes of this sequence: out within the profiled step's tolerance
                n_t = m + t - E_STEPS1 + 1
                planes = L.planes.unpack(n_t)
                qr = rotated(host(q[b])[:, None], [n_t - 1], E_D, dt)[:, 0][None]
                o_ref, need_ref, _ = orc.pq_decode_attention_profile(qr, *planes, E_THR)
                p1 = orc.softmax_probs(np.einsum("bhd,bhld->bhl", qr.astype(np.float32), orc.pq_dequant(planes[0], None, planes[2]))
                                       / np.float32(np.sqrt(E_D))).max(-1)
                got_need = L.need.cpu().numpy().reshape(1, E_H).astype(bool)
                decided = np.abs(p1 - E_THR) > 1e-4
                assert np.array_equal(got_need[decided], need_ref[decided]), msg
                ok = got_need == need_ref
                np.testing.assert_allclose(host(L.out).reshape(1, E_H, E_D)[ok], orc.round_dt(o_ref, dt)[ok], err_msg=msg, **OUT_TOL[dt])
        for l in range(E_LAYERS):                                         # the end of the turn
            msg = f"end layer {l} b={b}"
            for k in ("kc", "vc", "krc", "acc", "out", "lse", "prev"):
                assert torch.equal(getattr(rag2[l], k)[sl], getattr(S2[l], k)), (msg, k)
            for k in Layer.PLANES[:5]:
                assert torch.equal(getattr(rag2[l].planes, k)[sl], getattr(S2[l].planes, k)), (msg, k)
            n_e = m + E_STEPS2
            assert torch.equal(rag2[l].st[sl, :, :n_e], S2[l].st[:, :, :n_e]), msg
            assert torch.equal(rag2[l].planes.msb_logit[sl, :, :n_e], S2[l].planes.msb_logit[:, :, :n_e]), msg
        for L in S + S2:
            L.ws.check()
    ops.check_workspaces()


def test_ops_routes_by_the_accumulators_batch_axis():
    """A 2-D accumulator with a batched state keeps today's refusal, a 3-D one of another batch or shape is a ValueError — nothing is
    launched either way."""
    from spatten_amd import ops
    dt, d, H, Hkv, B = "bf16", 128, 4, 2, 2
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    buf = Buffers(8, 8, dt, d, H, Hkv, B)
    q = torch.zeros(B, H, d, dtype=TORCH_DT[dt], device="cuda")
    step = ops.StepState(cos, sin, batch=B)
    step.set([9, 4], [9, 4])
    step.advance()
    args = (q, buf.planes(), CAP, cos, sin, 0, 0.5)
    prev = torch.zeros(B, H, 2, device="cuda")
    with pytest.raises(NotImplementedError, match="batch axis"):
        ops.attn_decode_pqv(*args, step=step, lse=buf.lse, cascade=(torch.zeros(H, CAP, device="cuda"), prev, 0))
    for shape in ((B + 1, H, CAP), (B, H + 1, CAP), (B, H, CAP - 1)):
        with pytest.raises(ValueError):
            ops.attn_decode_pqv(*args, step=step, lse=buf.lse, cascade=(torch.zeros(*shape, device="cuda"), prev, 0))
    with pytest.raises(ValueError):
        ops.attn_decode_pqv(*args, step=step, lse=buf.lse, cascade=(torch.zeros(B, H, 2 * CAP, device="cuda")[:, :, ::2], prev, 0))
    with pytest.raises(NotImplementedError, match="append"):
        ops.attn_decode_pqv(*args, step=step, lse=buf.lse, cascade=(torch.zeros(B, H, CAP, device="cuda"), prev, 0),
                            append=(None,) * 5)
    torch.cuda.synchronize()
    assert (buf.out == OUT_FILL).all() and (buf.need == -1).all() and (buf.lg == LOGIT_FILL).all()
