"""The device-length decode step with ONE STATE PER SEQUENCE (spatten_decode_args_t::step_state_sb, ops.StepState(batch=B)): a ragged
batch — every sequence its own cache length, query position and append slot — on every route of the plain step.

Two yardsticks per case.  Independent: oracle.spatten_oracle.attention_core on each sequence alone.  Bit exact: for each sequence b
today's uniform-length static launch of the same batch (kv_len = length_b, pos_q = pos_b, laid out for the bound, same splits, team
and grouped-query mode) — same grid, same route, same merge — whose row b the ragged launch must reproduce bit for bit.

Shapes: bound 704, lengths after the append (704, 353, 352, 236, 1): 352 | 353 is the split boundary of two splits, 235 | 236 lies
around that of three; 352-row chunks are longer than the 320-row single-shot tile (pipelined instantiation), three splits take the
single-shot one; every length but 704 ends inside a 32-row tile of the grouped kernel; length 1 is the appended row alone.
Needs an MI355X."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_gqa import check_stash as check_stash_mfma
from tests.util import OUT_TOL, TORCH_DT, check_stash, dev, host

pytestmark = pytest.mark.gpu

CAP = 704
LENS = (704, 353, 352, 236, 1)            # cache lengths AFTER the step's append
POS_OFF = (0, 3, 0, 9, 5)                 # query position = length - 1 + offset (independent of the length after a prune)
TABLE_ROWS = 724
PLANE_FILL, STASH_FILL, OUT_FILL = 7.0, 5.0, 3.0


@contextlib.contextmanager
def long_oracle_table(rows):
    """attention_core builds its rotary table for the cache length only; a query position beyond it (a pruned sequence) needs more
    rows.  The oracle's own rope_table, asked for at least `rows` rows: the rows it had are unchanged."""
    real = orc.rope_table
    orc.rope_table = lambda n, d, dt, base=10000.0: real(max(n, rows), d, dt, base)
    try:
        yield
    finally:
        orc.rope_table = real


def oracle_rows(q, kn, vn, pasts, lens, pos, dt):
    """attention_core per sequence: [(out [H*d], stash [H, len], max prob [H])]."""
    res = []
    with long_oracle_table(TABLE_ROWS):
        for b, n in enumerate(lens):
            pk, pv = (None, None) if n == 1 else (pasts[b][0][None], pasts[b][1][None])
            o, st, _ = orc.attention_core(q[b][None, :, None], kn[b][None, :, None], vn[b][None, :, None], pk, pv,
                                          np.array([[pos[b]]]), None, dt)
            res.append((o[0, 0], st[0, :, 0], orc.softmax_probs(st)[0, :, 0].max(-1)))
    return res


_INPUTS = {}


def inputs(dt, H, Hkv, d, lens=LENS, seed=0, pos_off=POS_OFF):
    """Host inputs of a case and its oracle, computed once per geometry and shared (never modified)."""
    key = (dt, H, Hkv, d, lens, seed, pos_off)
    if key not in _INPUTS:
        B = len(lens)
        s = 9100 + 7 * H + Hkv + d + seed
        q = orc.synth_normal(s, 0, (B, H, d), dt)
        kn = orc.synth_normal(s, 1, (B, Hkv, d), dt)
        vn = orc.synth_normal(s, 2, (B, Hkv, d), dt)
        pasts = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n - 1, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n - 1, d), dt))
                 for b, n in enumerate(lens)]
        pos = [n - 1 + o for n, o in zip(lens, pos_off)]
        _INPUTS[key] = dict(q=q, kn=kn, vn=vn, pasts=pasts, pos=pos, oracle=oracle_rows(q, kn, vn, pasts, lens, pos, dt))
    return _INPUTS[key]


class Planes:
    """Device tensors of one launch: planes [B, Hkv, CAP, d] holding each sequence's past rows, the rest a finite sentinel."""

    def __init__(self, inp, dt, H, Hkv, d, lens, cos, sin):
        from spatten_amd import ops
        tdt, B = TORCH_DT[dt], len(lens)
        self.kc = torch.full((B, Hkv, CAP, d), PLANE_FILL, dtype=tdt, device="cuda")
        self.vc, self.krc = self.kc.clone(), self.kc.clone()
        for b, n in enumerate(lens):
            if n > 1:
                self.kc[b, :, :n - 1] = dev(inp["pasts"][b][0], dt)
                self.vc[b, :, :n - 1] = dev(inp["pasts"][b][1], dt)
                ops.build_shadow(self.kc[b:b + 1], self.krc[b:b + 1], 0, n - 1, cos, sin)
        self.out = torch.full((B, H * d), OUT_FILL, dtype=tdt, device="cuda")
        self.st = torch.full((B, H, CAP), STASH_FILL, dtype=tdt, device="cuda")
        self.lse = torch.full((B, H, 2), -1.0, dtype=torch.float32, device="cuda")
        self.habs = torch.zeros(B * H, dtype=torch.float32, device="cuda")

    def clone(self):
        c = object.__new__(Planes)
        c.__dict__ = {k: v.clone() for k, v in self.__dict__.items()}
        return c


def launch(pl, q, kn, vn, cos, sin, ws, n_splits, head_ids=None, grouped_heads=False, use_habs=False, **how):
    from spatten_amd import ops
    kw = dict(k_new=kn, v_new=vn, scores=pl.st, lse=pl.lse, out=pl.out, workspace=ws, n_splits=n_splits)
    if head_ids is not None:
        kw.update(head_ids=head_ids)
    if use_habs:
        kw.update(head_abs=pl.habs)
    if grouped_heads:
        kw.update(grouped_heads=True)
    kw.update(how)
    kv_len = kw.pop("kv_len")
    pos_q = kw.pop("pos_q", 0)
    args = (q, pl.kc, pl.krc, pl.vc, kv_len, cos, sin, pos_q)
    form = ops.decode_gqa_form(*args, **kw)
    ops.attn_decode(*args, **kw)
    return form


# (name, H, Hkv, d, dt, gqa mode, team, head list, head_abs, grouped_heads)
ROUTES = [
    ("mha-lean-bf16", 4, 4, 128, "bf16", 0, 512, None, False, False),
    ("mha-lean-f16", 4, 4, 128, "f16", 0, 512, None, False, False),
    ("mha-head-list", 4, 4, 128, "bf16", 0, 512, (0, 2, 3), True, False),
    ("gqa-per-query-head", 8, 2, 128, "bf16", 0, 512, None, False, False),
    ("gqa-grouped", 8, 2, 128, "bf16", 1, 512, None, False, False),
    ("gqa-grouped-f16", 8, 2, 128, "f16", 1, 512, None, False, False),
    ("gqa-grouped-head-list", 8, 2, 128, "bf16", 1, 512, (0, 2, 3), True, True),     # heads 4..7: kv head 1's group is empty
    ("mha-lean-team256", 4, 4, 128, "bf16", 0, 256, None, False, False),
    ("mha-f32-d64", 4, 4, 64, "f32", 0, 512, None, False, False),
]


@pytest.mark.parametrize("n_splits", [1, 2, 3])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_ragged_step_vs_oracle_and_vs_the_static_launch_of_each_length(route, n_splits):
    from spatten_amd import ops
    name, H, Hkv, d, dt, mode, team, hlist, use_habs, grouped_heads = route
    inp = inputs(dt, H, Hkv, d)
    B, G, tdt = len(LENS), H // Hkv, TORCH_DT[dt]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    q, kn, vn = dev(inp["q"], dt), dev(inp["kn"], dt), dev(inp["vn"], dt)
    ids = None if hlist is None else torch.tensor(hlist, dtype=torch.int32, device="cuda")
    live = list(range(H)) if hlist is None else list(hlist)
    dead = [h for h in range(H) if h not in live]
    live_kv = sorted({h // G for h in live})               # kv heads with a launched query head: only those append
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    base = Planes(inp, dt, H, Hkv, d, LENS, cos, sin)
    prev_mode, prev_team = ops.set_decode_gqa(mode), ops.set_decode_team(team)
    try:
        rag = base.clone()
        step = ops.StepState(cos, sin, batch=B)
        assert step.stride >= 64 + 2 * d * (4 if dt == "f32" else 2) and step.stride % 256 == 0
        step.set([n - 1 for n in LENS], [p - 1 for p in inp["pos"]])
        step.advance()
        assert step.read() == list(zip(LENS, inp["pos"]))
        common = dict(head_ids=ids, grouped_heads=grouped_heads, use_habs=use_habs)
        form = launch(rag, q, kn, vn, cos, sin, ws, n_splits, kv_len=CAP, step=step, **common)
        assert form == (mode == 1), name
        torch.cuda.synchronize()
        ws.check()
        out, st, lse = host(rag.out).reshape(B, H, d), host(rag.st), host(rag.lse)
        for b, n in enumerate(LENS):
            o_ref, st_ref, pmax = inp["oracle"][b]
            msg = f"{name} S={n_splits} b={b} len={n}"
            # ---- the oracle on this sequence alone
            np.testing.assert_allclose(out[b, live], o_ref.reshape(H, d)[live], err_msg=msg, **OUT_TOL[dt])
            (check_stash_mfma if mode == 1 else check_stash)(st[b, live, :n], st_ref[live], dt, msg)
            np.testing.assert_allclose(1.0 / lse[b, live, 1], pmax[live], rtol=2e-2, err_msg=msg)
            # ---- nothing past the sequence's length, nothing of a pruned head
            assert (rag.st[b, :, n:] == STASH_FILL).all(), msg
            for plane in (rag.kc, rag.krc, rag.vc):
                assert (plane[b, :, n:] == PLANE_FILL).all(), msg
            assert torch.equal(rag.kc[b, live_kv, n - 1], kn[b, live_kv]) and torch.equal(rag.vc[b, live_kv, n - 1], vn[b, live_kv]), msg
            if dead:
                assert (rag.st[b, dead] == STASH_FILL).all() and (rag.out.view(B, H, d)[b, dead] == OUT_FILL).all(), msg
                assert (rag.lse[b, dead] == -1.0).all() and (rag.habs.view(B, H)[b, dead] == 0).all(), msg
            # ---- today's static launch of the whole batch at THIS sequence's length and position: row b, bit for bit
            sta = base.clone()
            form_s = launch(sta, q, kn, vn, cos, sin, ws, n_splits, kv_len=n, pos_q=inp["pos"][b], layout=CAP, **common)
            assert form_s == form, msg
            torch.cuda.synchronize()
            assert torch.equal(rag.out[b], sta.out[b]), msg
            assert torch.equal(rag.st[b, :, :n], sta.st[b, :, :n]), msg
            assert torch.equal(rag.lse[b], sta.lse[b]), msg
            for a_, s_ in ((rag.kc, sta.kc), (rag.krc, sta.krc), (rag.vc, sta.vc)):
                assert torch.equal(a_[b, :, :n], s_[b, :, :n]), msg
            if use_habs:
                assert torch.equal(rag.habs.view(B, H)[b], sta.habs.view(B, H)[b]), msg
        ws.check()
    finally:
        ops.set_decode_gqa(prev_mode)
        ops.set_decode_team(prev_team)


GRAPH_START = (700, 350, 351, 233, 1)     # cache lengths BEFORE the first token: split boundaries are crossed while the steps run


@pytest.mark.parametrize("route", [("mha-lean", 4, 4, 0, 2), ("mha-lean-single-shot", 4, 4, 0, 3), ("gqa-grouped", 8, 2, 1, 2)],
                         ids=lambda r: r[0])
def test_three_tokens_of_a_ragged_batch_as_one_captured_graph(route):
    """advance + launch captured ONCE (a linear graph), replayed for three tokens with fresh q / k_new / v_new: equal to the eager
    ragged launches bit for bit, and to the oracle on the last token."""
    from spatten_amd import ops
    name, H, Hkv, mode, n_splits = route
    dt, d, B, T = "bf16", 128, len(GRAPH_START), 3
    tdt = TORCH_DT[dt]
    final = tuple(n + T for n in GRAPH_START)
    # the final state of every sequence as ONE host case: its past rows = the starting rows + the first T - 1 appended tokens
    s = 9900 + H
    pasts = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n - 1, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n - 1, d), dt))
             for b, n in enumerate(final)]
    toks = []                                              # (q, k_new, v_new) of token t: rows GRAPH_START[b] + t of the final caches
    for t in range(T):
        if t < T - 1:
            tk = np.stack([pasts[b][0][:, GRAPH_START[b] + t] for b in range(B)])
            tv = np.stack([pasts[b][1][:, GRAPH_START[b] + t] for b in range(B)])
        else:
            tk, tv = orc.synth_normal(s, 101, (B, Hkv, d), dt), orc.synth_normal(s, 102, (B, Hkv, d), dt)
        toks.append((orc.synth_normal(s, 200 + t, (B, H, d), dt), tk, tv))
    pos_last = [n - 1 + o for n, o in zip(final, POS_OFF)]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    start_inp = dict(pasts=[(pk[:, :n0], pv[:, :n0]) for (pk, pv), n0 in zip(pasts, GRAPH_START)])
    start_lens = tuple(n0 + 1 for n0 in GRAPH_START)       # (Planes takes lengths after an append: rows [0, n0) are the past)
    base = Planes(start_inp, dt, H, Hkv, d, start_lens, cos, sin)
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    q, kn, vn = (torch.zeros(B, H, d, dtype=tdt, device="cuda"), torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"),
                 torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"))
    prev_mode = ops.set_decode_gqa(mode)
    try:
        sets = {}
        for kind in ("graph", "eager"):
            pl, step = base.clone(), ops.StepState(cos, sin, batch=B)
            sets[kind] = (pl, step)

        def token(kind):
            pl, step = sets[kind]
            step.advance()
            return launch(pl, q, kn, vn, cos, sin, ws, n_splits, kv_len=CAP, step=step)

        def reset(kind):
            pl, step = sets[kind]
            for k, v in base.__dict__.items():
                getattr(pl, k).copy_(v)
            step.set(list(GRAPH_START), [n0 - 1 + o for n0, o in zip(GRAPH_START, POS_OFF)])

        reset("graph")
        assert token("graph") == (mode == 1)               # warm-up outside the capture
        torch.cuda.synchronize()
        reset("graph"); reset("eager")
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            token("graph")
        reset("graph")                                     # (nothing ran during the capture; states as set)
        for t in range(T):
            q.copy_(dev(toks[t][0], dt)); kn.copy_(dev(toks[t][1], dt)); vn.copy_(dev(toks[t][2], dt))
            gr.replay()
            token("eager")
            torch.cuda.synchronize()
            ws.check()
            g_, e_ = sets["graph"][0], sets["eager"][0]
            lens = [n0 + t + 1 for n0 in GRAPH_START]
            assert sets["graph"][1].read() == sets["eager"][1].read() == [(n, n - 1 + o) for n, o in zip(lens, POS_OFF)], t
            for k in ("out", "st", "lse", "kc", "krc", "vc"):
                assert torch.equal(getattr(g_, k), getattr(e_, k)), (name, t, k)
            for b, n in enumerate(lens):
                assert (g_.st[b, :, n:] == STASH_FILL).all() and (g_.vc[b, :, n:] == PLANE_FILL).all(), (name, t, b)
        ref = oracle_rows(toks[-1][0], toks[-1][1], toks[-1][2], pasts, final, pos_last, dt)
        g_ = sets["graph"][0]
        out, st, lse = host(g_.out).reshape(B, H, d), host(g_.st), host(g_.lse)
        for b, n in enumerate(final):
            o_ref, st_ref, pmax = ref[b]
            np.testing.assert_allclose(out[b], o_ref.reshape(H, d), err_msg=f"{name} b={b}", **OUT_TOL[dt])
            (check_stash_mfma if mode == 1 else check_stash)(st[b, :, :n], st_ref, dt, f"{name} b={b}")
            np.testing.assert_allclose(1.0 / lse[b, :, 1], pmax, rtol=2e-2)
    finally:
        ops.set_decode_gqa(prev_mode)


def test_advance_with_a_delta_per_sequence():
    """deltas = (1, 0, 1, 1, 0): sequences with delta 0 keep length and position, the others move — as host values and as a device
    tensor; every state's staged rotary rows are those a scalar state holds for the same (length, position)."""
    from spatten_amd import ops
    d, dt = 128, "bf16"
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    B = len(LENS)
    lens0 = [n - 1 for n in LENS]
    pos0 = [max(n - 2 + o, 0) for n, o in zip(LENS, POS_OFF)]
    step = ops.StepState(cos, sin, batch=B)
    step.set(torch.tensor(lens0, dtype=torch.int32, device="cuda"), torch.tensor(pos0, dtype=torch.int32, device="cuda"))
    assert step.read() == list(zip(lens0, pos0))
    deltas = [1, 0, 1, 1, 0]
    step.advance(deltas=deltas)
    want = [(n + dl, p + dl) for n, p, dl in zip(lens0, pos0, deltas)]
    assert step.read() == want
    step.advance(deltas=torch.tensor(deltas, dtype=torch.int32, device="cuda"))
    want = [(n + dl, p + dl) for (n, p), dl in zip(want, deltas)]
    assert step.read() == want
    assert [w[2] for w in step.read(all_words=True)] == [2] * B      # words 2 / 3 as in the scalar calls: two steps since the set
    step.advance(2)
    want = [(n + 2, p + 2) for n, p in want]
    assert step.read() == want
    rows = step.buf.view(B, step.stride)[:, 64:]
    one = ops.StepState(cos, sin)
    for b, (n, p) in enumerate(want):
        one.set(n, p)
        assert torch.equal(rows[b], one.buf[64:]), b
    with pytest.raises(ValueError):
        step.advance(deltas=[1, 2])
    with pytest.raises(ValueError):
        one.advance(deltas=[1])


def test_a_batch_of_one_state_is_the_scalar_state_and_a_strided_launch_of_one_sequence_the_shared_one():
    from spatten_amd import ops
    dt, H, Hkv, d, n, off = "bf16", 8, 2, 128, 353, 3
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    one, bat = ops.StepState(cos, sin), ops.StepState(cos, sin, batch=1)
    assert bat.stride == one.buf.numel() == bat.buf.numel()
    one.set(n - 1, n - 2 + off); bat.set(n - 1, n - 2 + off)
    assert torch.equal(one.buf, bat.buf)
    one.advance(); bat.advance()
    assert torch.equal(one.buf, bat.buf) and bat.read() == [one.read()] == [(n, n - 1 + off)]
    one.advance(3); bat.advance(3)
    one.advance(-3); bat.advance(deltas=[-3])
    assert torch.equal(one.buf, bat.buf) and bat.read(all_words=True) == [one.read(all_words=True)]
    inp = inputs(dt, H, Hkv, d, lens=(n,), seed=1, pos_off=(off,))
    q, kn, vn = dev(inp["q"], dt), dev(inp["kn"], dt), dev(inp["vn"], dt)
    ws = ops.DecodeWorkspace(1, H, d, "cuda")
    base = Planes(inp, dt, H, Hkv, d, (n,), cos, sin)
    prev = ops.set_decode_gqa(0)
    try:
        for mode in (0, 1):
            ops.set_decode_gqa(mode)
            for ns in (1, 2, 3):
                a, b_ = base.clone(), base.clone()
                fa = launch(a, q, kn, vn, cos, sin, ws, ns, kv_len=CAP, step=one)
                fb = launch(b_, q, kn, vn, cos, sin, ws, ns, kv_len=CAP, step=bat)
                torch.cuda.synchronize()
                assert fa == fb == (mode == 1)
                for k in ("out", "st", "lse", "kc", "krc", "vc"):
                    assert torch.equal(getattr(a, k), getattr(b_, k)), (mode, ns, k)
                np.testing.assert_allclose(host(a.out)[0], inp["oracle"][0][0], **OUT_TOL[dt])
        ws.check()
    finally:
        ops.set_decode_gqa(prev)


def test_what_a_strided_step_refuses():
    from spatten_amd import ops
    dt, H, Hkv, d = "bf16", 4, 4, 128
    tdt = TORCH_DT[dt]
    inp = inputs(dt, H, Hkv, d)
    B = len(LENS)
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    q, kn, vn = dev(inp["q"], dt), dev(inp["kn"], dt), dev(inp["vn"], dt)
    pl = Planes(inp, dt, H, Hkv, d, LENS, cos, sin)
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    step = ops.StepState(cos, sin, batch=B)
    step.set(list(LENS), inp["pos"])
    args = (q, pl.kc, pl.krc, pl.vc, CAP, cos, sin, 0)
    acc = torch.zeros(H, CAP, dtype=torch.float32, device="cuda")
    prev_st, prev_lse = torch.zeros_like(pl.st), torch.ones_like(pl.lse)
    with pytest.raises(RuntimeError, match=r"status -2"):  # SPATTEN_ERR_UNSUPPORTED: the accumulator [H, L] has no batch axis
        ops.attn_decode(*args, k_new=kn, v_new=vn, scores=pl.st, lse=pl.lse, out=pl.out, workspace=ws, step=step,
                        cascade=(acc, prev_st, prev_lse, 0))
    planes = ops.PQPlanes(B, Hkv, CAP, d, "cuda")
    need = torch.zeros(B * H, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"status -2"):  # the quantised-key passes keep the shared state
        ops.attn_decode(*args, scores=pl.st, lse=pl.lse, out=pl.out, workspace=ws, step=step, pq=(planes, 0.1, need))
    with pytest.raises(ValueError, match="sequences"):     # a state array of another batch size
        ops.attn_decode(*args, k_new=kn, v_new=vn, out=pl.out, workspace=ws, step=ops.StepState(cos, sin, batch=B + 1))
    mask = torch.zeros(B, CAP, dtype=tdt, device="cuda")
    with pytest.raises(RuntimeError, match=r"status -1"):  # a mask stays refused with a state (SPATTEN_ERR_INVALID)
        ops.attn_decode(*args, k_new=kn, v_new=vn, out=pl.out, workspace=ws, step=step, mask=mask)
    torch.cuda.synchronize()
    assert (pl.out == OUT_FILL).all()                      # nothing was launched


def test_a_sequence_with_delta_zero_repeats_its_step_in_place():
    """advance(deltas=...) with a 0 leaves that sequence's state alone, but the launch still runs it: its k_new / v_new go to row
    length_b - 1 again.  Handed the rows of its last step once more, an idle sequence keeps every bit — out, stash, (max, sum), planes
    — while the others append their next row."""
    from spatten_amd import ops
    dt, H, Hkv, d = "bf16", 8, 2, 128
    starts, deltas = (699, 351, 235, 1), (1, 0, 1, 0)
    B = len(starts)
    lens1 = tuple(n + 1 for n in starts)
    inp = inputs(dt, H, Hkv, d, lens=lens1, seed=2, pos_off=(0, 3, 9, 5))
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    prev = ops.set_decode_gqa(0)
    try:
        for mode in (0, 1):
            ops.set_decode_gqa(mode)
            pl = Planes(inp, dt, H, Hkv, d, lens1, cos, sin)
            q, kn, vn = dev(inp["q"], dt), dev(inp["kn"], dt), dev(inp["vn"], dt)
            step = ops.StepState(cos, sin, batch=B)
            step.set(list(starts), [p - 1 for p in inp["pos"]])
            step.advance()
            launch(pl, q, kn, vn, cos, sin, ws, 2, kv_len=CAP, step=step)
            torch.cuda.synchronize()
            first = pl.clone()
            # the moving sequences get a new token; the idle ones are handed their last rows again
            g = torch.Generator(device="cuda").manual_seed(5)
            move = [b for b in range(B) if deltas[b]]
            idle = [b for b in range(B) if not deltas[b]]
            for t in (q, kn, vn):
                t[move] = torch.randn(t[move].shape, device="cuda", generator=g).to(t.dtype)
            step.advance(deltas=list(deltas))
            assert step.read() == [(n + dl, p + dl) for n, p, dl in zip(lens1, inp["pos"], deltas)]
            launch(pl, q, kn, vn, cos, sin, ws, 2, kv_len=CAP, step=step)
            torch.cuda.synchronize()
            ws.check()
            for b in idle:
                for k in ("out", "st", "lse", "kc", "krc", "vc"):
                    assert torch.equal(getattr(pl, k)[b], getattr(first, k)[b]), (mode, b, k)
            for b in move:
                n = lens1[b] + 1
                assert torch.equal(pl.kc[b, :, n - 1], kn[b]) and torch.equal(pl.vc[b, :, n - 1], vn[b]), (mode, b)
                for k in ("kc", "krc", "vc"):
                    assert torch.equal(getattr(pl, k)[b, :, :n - 1], getattr(first, k)[b, :, :n - 1]), (mode, b, k)
                    assert (getattr(pl, k)[b, :, n:] == PLANE_FILL).all(), (mode, b, k)
                assert (pl.st[b, :, n:] == STASH_FILL).all() and not torch.equal(pl.out[b], first.out[b]), (mode, b)
    finally:
        ops.set_decode_gqa(prev)
