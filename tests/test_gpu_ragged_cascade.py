"""Cascade importance on a ragged batch: one accumulator PER SEQUENCE (spatten_decode_args_t::acc_sb, a 3-D ``acc`` in
ops.attn_decode), the fold of the pending step (spatten_importance_accumulate_step) and the whole turn — accumulate, fold, prune every
sequence at its own length, hand the lengths on — without one host value of a length.

Shapes are those of tests/test_gpu_ragged_step.py: bound 704; three consecutive steps whose LAST one runs at the lengths
(704, 353, 352, 236, 3) — 352 | 353 the boundary of two splits, 235 | 236 around that of three, 704 the bound — and whose FIRST one
has a sequence of length 1 (the appended row alone).  Bit-exact yardstick, that file's own: for each sequence b the uniform-length
static launch of the same batch at kv_len = len_b with the same acc_sb — row b of accumulator, stash, (max, sum) and out.
Independent: orc.cascade_importance_accumulate per sequence, at tests/test_gpu_gqa_cascade.py's tolerance.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_ragged_step import CAP, POS_OFF, TABLE_ROWS, Planes, launch
from tests.util import OUT_TOL, TORCH_DT, dev, host

pytestmark = pytest.mark.gpu

T = 3
LAST = (704, 353, 352, 236, 3)               # lengths after the append of the last step
ACC_TOL = dict(rtol=2e-3, atol=2e-5)         # tests/test_gpu_gqa_cascade.py, the same quantity


def step_len(b, t):
    return LAST[b] - (T - 1) + t


class Turn:
    """Everything one token stream owns on the device: planes, the two swapping stash / (max, sum) buffers, the accumulators."""

    def __init__(self, pl, B, H):
        self.pl = pl
        self.st = [pl.st, pl.st.clone()]
        self.lse = [pl.lse, pl.lse.clone()]
        self.acc = torch.zeros(B, H, CAP, dtype=torch.float32, device="cuda")

    def clone(self):
        c = object.__new__(Turn)
        c.pl = self.pl.clone()
        c.st = [c.pl.st, self.st[1].clone()]
        c.lse = [c.pl.lse, self.lse[1].clone()]
        c.acc = self.acc.clone()
        return c


def host_inputs(dt, H, Hkv, d, seed):
    B = len(LAST)
    pasts = [(orc.synth_normal(seed, 10 + 2 * b, (Hkv, max(step_len(b, 0) - 1, 1), d), dt)[:, :step_len(b, 0) - 1],
              orc.synth_normal(seed, 11 + 2 * b, (Hkv, max(step_len(b, 0) - 1, 1), d), dt)[:, :step_len(b, 0) - 1]) for b in range(B)]
    toks = [(orc.synth_normal(seed, 100 + 3 * t, (B, H, d), dt), orc.synth_normal(seed, 101 + 3 * t, (B, Hkv, d), dt),
             orc.synth_normal(seed, 102 + 3 * t, (B, Hkv, d), dt)) for t in range(T)]
    return pasts, toks


# (name, H, Hkv, d, dt, gqa mode)
ROUTES = [
    ("mha-lean-bf16", 4, 4, 128, "bf16", 0),
    ("gqa-per-query-head", 8, 2, 128, "bf16", 0),
    ("gqa-grouped", 8, 2, 128, "bf16", 1),
    ("mha-f32-d64", 4, 4, 64, "f32", 0),
]


@pytest.mark.parametrize("n_splits", [1, 2, 3])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_three_ragged_steps_accumulate_per_sequence(route, n_splits):
    from spatten_amd import ops
    name, H, Hkv, d, dt, mode = route
    B = len(LAST)
    pasts, toks = host_inputs(dt, H, Hkv, d, 9300 + H + d)
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    lens0 = tuple(step_len(b, 0) for b in range(B))
    rag = Turn(Planes(dict(pasts=pasts), dt, H, Hkv, d, lens0, cos, sin), B, H)
    pos0 = [n - 1 + o for n, o in zip(lens0, POS_OFF)]
    prev_mode = ops.set_decode_gqa(mode)
    try:
        step = ops.StepState(cos, sin, batch=B)
        step.set([n - 1 for n in lens0], [p - 1 for p in pos0])
        # right after the set nothing is pending: the fold is a no-op
        ops.importance_accumulate_step(rag.acc, rag.st[0], rag.lse[0], rag.st[1], rag.lse[1], step, CAP)
        torch.cuda.synchronize()
        assert not rag.acc.any()
        want = np.zeros((B, H, CAP), np.float32)             # the oracle's running sum from the kernel's own stash
        for t in range(T):
            q, kn, vn = (dev(x, dt) for x in toks[t])
            before = rag.clone()
            step.advance()
            cur, prv = t & 1, (t & 1) ^ 1
            # (the device-length form takes the two buffers in a FIXED order and swaps by the state's parity)
            form = launch(rag.pl, q, kn, vn, cos, sin, ws, n_splits, kv_len=CAP, step=step, scores=rag.st[0], lse=rag.lse[0],
                          cascade=(rag.acc, rag.st[1], rag.lse[1], 0))
            assert form == (mode == 1), name
            torch.cuda.synchronize()
            ws.check()
            for b in range(B):
                n, msg = step_len(b, t), f"{name} S={n_splits} t={t} b={b}"
                # ---- the static launch of the whole batch at THIS sequence's length, same acc_sb: row b, bit for bit
                sta = before.clone()
                form_s = launch(sta.pl, q, kn, vn, cos, sin, ws, n_splits, kv_len=n, pos_q=pos0[b] + t, layout=CAP,
                                scores=sta.st[cur], lse=sta.lse[cur],
                                cascade=(sta.acc, sta.st[prv], sta.lse[prv], n - 1) if t > 0 else None)
                assert form_s == form, msg
                torch.cuda.synchronize()
                assert torch.equal(rag.pl.out[b], sta.pl.out[b]), msg
                assert torch.equal(rag.st[cur][b, :, :n], sta.st[cur][b, :, :n]) and torch.equal(rag.st[prv][b], before.st[prv][b]), msg
                assert torch.equal(rag.lse[cur][b], sta.lse[cur][b]) and torch.equal(rag.lse[prv][b], before.lse[prv][b]), msg
                assert torch.equal(rag.acc[b], sta.acc[b]), msg
                assert torch.equal(rag.acc[b, :, max(n - 1, 0) if t else 0:], before.acc[b, :, max(n - 1, 0) if t else 0:]), msg
                # ---- the oracle: everything up to the previous step is in the accumulator
                np.testing.assert_allclose(host(rag.acc[b]), want[b], err_msg=msg, **ACC_TOL)
                want[b, :, :n] = orc.cascade_importance_accumulate(want[b, :, :n], host(rag.st[cur][b:b + 1, :, :n])[:, :, None, :])
            # ---- the pending step folded: spatten_importance_accumulate on each slice, bit for bit (after an odd count, t = 0 / 2,
            # and an even one, t = 1); the turn's own accumulator is left alone
            folded = rag.acc.clone()
            ops.importance_accumulate_step(folded, rag.st[0], rag.lse[0], rag.st[1], rag.lse[1], step, CAP)
            ref = rag.acc.clone()
            for b in range(B):
                n = step_len(b, t)
                ops.importance_accumulate(ref[b], rag.st[cur][b:b + 1, :, None, :n], rag.lse[cur][b:b + 1, :, None, :])
            torch.cuda.synchronize()
            assert torch.equal(folded, ref), (name, n_splits, t)
            for b in range(B):
                np.testing.assert_allclose(host(folded[b]), want[b], err_msg=f"{name} fold t={t} b={b}", **ACC_TOL)
        ws.check()
    finally:
        ops.set_decode_gqa(prev_mode)


def test_what_the_accumulator_stride_refuses():
    from spatten_amd import ops
    dt, H, Hkv, d, B = "bf16", 4, 4, 128, len(LAST)
    pasts, toks = host_inputs(dt, H, Hkv, d, 9300 + H + d)
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    lens0 = tuple(step_len(b, 0) for b in range(B))
    tr = Turn(Planes(dict(pasts=pasts), dt, H, Hkv, d, lens0, cos, sin), B, H)
    q, kn, vn = (dev(x, dt) for x in toks[0])
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    step = ops.StepState(cos, sin, batch=B)
    step.set(list(lens0), [n - 1 for n in lens0])
    args = (q, tr.pl.kc, tr.pl.krc, tr.pl.vc, CAP, cos, sin, 0)
    kw = dict(k_new=kn, v_new=vn, scores=tr.st[0], lse=tr.lse[0], out=tr.pl.out, workspace=ws, step=step)
    with pytest.raises(ValueError, match="cascade"):           # an accumulator of another batch size
        ops.attn_decode(*args, cascade=(tr.acc[:B - 1], tr.st[1], tr.lse[1], 0), **kw)
    with pytest.raises(ValueError, match="cascade"):
        ops.attn_decode(*args, cascade=(tr.acc.expand(2, B, H, CAP), tr.st[1], tr.lse[1], 0), **kw)
    with pytest.raises(ValueError, match="acc"):               # the fold of a batch needs the batch axis too
        ops.importance_accumulate_step(tr.acc[0], tr.st[0], tr.lse[0], tr.st[1], tr.lse[1], step, CAP)
    planes = ops.PQPlanes(B, Hkv, CAP, d, "cuda")
    need = torch.zeros(B * H, dtype=torch.int32, device="cuda")
    one = ops.StepState(cos, sin)
    one.set(300, 299)
    with pytest.raises(RuntimeError, match=r"status -2"):      # the quantised-key passes keep their own accumulator argument
        ops.attn_decode(*args, scores=tr.st[0], lse=tr.lse[0], out=tr.pl.out, workspace=ws, step=one, pq=(planes, 0.1, need),
                        cascade=(tr.acc, tr.st[1], tr.lse[1], 0))
    torch.cuda.synchronize()
    assert not tr.acc.any()


# ------------------------------------------------------------------------------------------------
# End to end: four captured tokens, fold, ragged prune, hand the lengths on, one more step
# ------------------------------------------------------------------------------------------------
E_START, E_RECENT, E_K, E_NC = 4, 8, 16, 1                   # keep_rows 27: lengths 40 and 30 prune, 20 does not
E_BOUND, E_CAP2 = 64, 32                                     # rows of the planes before / after the event
E_LENS0 = (36, 26, 16)                                       # cache lengths before the first token
E_TOKENS = 4
E_MODELS = (("grouped", 8, 2, 1), ("lean", 4, 4, 0))         # (name, H, Hkv, gqa mode): two "layers" of one token stream


class Layer:
    def __init__(self, H, Hkv, mode, B, d, tdt, rows, seed=None, lens=None, cos=None, sin=None):
        from spatten_amd import ops
        self.H, self.Hkv, self.mode = H, Hkv, mode
        z = lambda *s, dtype=tdt: torch.zeros(*s, dtype=dtype, device="cuda")
        self.kc, self.krc, self.vc = z(B, Hkv, rows, d), z(B, Hkv, rows, d), z(B, Hkv, rows, d)
        self.st, self.lse = [z(B, H, rows), z(B, H, rows)], [z(B, H, 2, dtype=torch.float32), z(B, H, 2, dtype=torch.float32)]
        self.acc = z(B, H, rows, dtype=torch.float32)
        self.out = z(B, H * d)
        self.ws = ops.DecodeWorkspace(B, H, d, "cuda")
        if seed is not None:
            g = torch.Generator(device="cuda").manual_seed(seed)
            for b, n in enumerate(lens):
                self.kc[b, :, :n] = torch.randn(Hkv, n, d, device="cuda", generator=g).to(tdt)
                self.vc[b, :, :n] = torch.randn(Hkv, n, d, device="cuda", generator=g).to(tdt)
                ops.build_shadow(self.kc[b:b + 1], self.krc[b:b + 1], 0, n, cos, sin)

    def clone(self):
        c = object.__new__(Layer)
        c.__dict__ = {k: ([x.clone() for x in v] if isinstance(v, list) else v.clone() if isinstance(v, torch.Tensor) else v)
                      for k, v in self.__dict__.items()}
        return c


def kv_scores(layer):
    """group-summed importance [B, Hkv, rows] for the per-KV-head row map"""
    B, H, rows = layer.acc.shape
    return layer.acc.view(B, layer.Hkv, H // layer.Hkv, rows).sum(2)


def test_a_captured_ragged_turn_then_fold_prune_and_one_more_step():
    """The ragged schedule (one graph per token; fold, ONE prune event per model geometry, set from device lengths) against the same
    schedule driven per sequence from host integers through today's calls (B = 1 states, importance_accumulate,
    prune_layers): caches, accumulators and lengths bit for bit; the last step's out against the oracle."""
    from spatten_amd import ops
    dt, d, B = "bf16", 128, len(E_LENS0)
    tdt = TORCH_DT[dt]
    cos, sin = oracle_table(E_BOUND + 8, d, dt)
    keep = E_START + E_K + E_RECENT - E_NC
    g = torch.Generator(device="cuda").manual_seed(77)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(tdt)
    toks = [[(rnd(B, H, d), rnd(B, Hkv, d), rnd(B, Hkv, d)) for _, H, Hkv, _ in E_MODELS] for _ in range(E_TOKENS + 1)]
    layers0 = [Layer(H, Hkv, mode, B, d, tdt, E_BOUND, seed=5 + i, lens=E_LENS0, cos=cos, sin=sin) for i, (_, H, Hkv, mode) in enumerate(E_MODELS)]
    prev_mode = ops.set_decode_gqa(0)

    def decode(L, q, kn, vn, step, bound, sl=slice(None), **how):
        ops.set_decode_gqa(L.mode)
        args = (q, L.kc[sl], L.krc[sl], L.vc[sl], bound, cos, sin, 0)
        kw = dict(k_new=kn, v_new=vn, scores=L.st[0][sl], lse=L.lse[0][sl], out=L.out[sl], workspace=how.pop("ws", L.ws), step=step,
                  cascade=(L.acc[sl], L.st[1][sl], L.lse[1][sl], 0), n_splits=2)
        assert ops.decode_gqa_form(*args, **kw) == (L.mode == 1)
        ops.attn_decode(*args, **kw)

    try:
        # ---------------- the ragged schedule ----------------
        rag = [L.clone() for L in layers0]
        qb = [[torch.zeros_like(x) for x in m] for m in toks[0]]
        step = ops.StepState(cos, sin, batch=B)

        def token():
            step.advance()
            for L, (q, kn, vn) in zip(rag, qb):
                decode(L, q, kn, vn, step, E_BOUND)

        def reset():
            for L, L0 in zip(rag, layers0):
                for k_, v in L0.__dict__.items():
                    if isinstance(v, torch.Tensor):
                        getattr(L, k_).copy_(v)
                    elif isinstance(v, list):
                        for x, y in zip(getattr(L, k_), v):
                            x.copy_(y)
            step.set(list(E_LENS0), [n - 1 for n in E_LENS0])

        reset()
        token()                                              # warm-up outside the capture
        torch.cuda.synchronize()
        reset()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            token()
        reset()
        for t in range(E_TOKENS):
            for dst, src in zip(qb, toks[t]):
                for x, y in zip(dst, src):
                    x.copy_(y)
            gr.replay()
        lens1 = [n + E_TOKENS for n in E_LENS0]
        torch.cuda.synchronize()
        assert [r[0] for r in step.read()] == lens1
        new_lens, rag2 = None, []
        for L in rag:
            ops.importance_accumulate_step(L.acc, L.st[0], L.lse[0], L.st[1], L.lse[1], step, E_BOUND)
            L.ws.check()
            Kn, Vn, Krn, idx, nl, accs = ops.prune_ragged([kv_scores(L)], [L.kc], [L.vc], step.lengths(), E_BOUND, E_START, E_RECENT, E_K,
                                                          E_NC, E_CAP2, (cos, sin), acc=[L.acc])
            assert new_lens is None or torch.equal(new_lens, nl)
            new_lens = nl
            L2 = Layer(L.H, L.Hkv, L.mode, B, d, tdt, E_CAP2)
            L2.kc, L2.vc, L2.krc, L2.acc = Kn[0], Vn[0], Krn[0], accs[0]
            rag2.append(L2)
        step.set(new_lens, new_lens - 1)                     # device tensors: no host value of a length
        step.advance()
        for L, (q, kn, vn) in zip(rag2, toks[E_TOKENS]):
            decode(L, q, kn, vn, step, E_CAP2)
        torch.cuda.synchronize()
        want_lens = [keep if n + E_NC > E_START + E_K + E_RECENT else n for n in lens1]
        assert new_lens.tolist() == want_lens and sum(n == keep for n in want_lens) == 2 and want_lens[2] == lens1[2]
        assert [r[0] for r in step.read()] == [n + 1 for n in want_lens]

        # ---------------- the same schedule per sequence, from host integers ----------------
        for i, (L0, R2) in enumerate(zip(layers0, rag2)):
            for b in range(B):
                sl = slice(b, b + 1)
                S = L0.clone()
                one = ops.StepState(cos, sin)
                one.set(E_LENS0[b], E_LENS0[b] - 1)
                ws1 = ops.DecodeWorkspace(1, S.H, d, "cuda")
                for t in range(E_TOKENS):
                    one.advance()
                    q, kn, vn = (x[sl] for x in toks[t][i])
                    decode(S, q, kn, vn, one, E_BOUND, sl, ws=ws1)
                n = lens1[b]
                last = (E_TOKENS - 1) & 1
                acc_b = S.acc[b]
                ops.importance_accumulate(acc_b, S.st[last][sl, :, None, :n], S.lse[last][sl, :, None, :])
                if n + E_NC > E_START + E_K + E_RECENT:
                    hi, G = n - E_RECENT + E_NC, S.H // S.Hkv
                    sc = kv_scores(S)[b]                     # (the batch's own reduction: the same bits as the ragged event ranked)
                    Kn = Vn = Krn = None
                    acc_n = torch.zeros(S.H, E_CAP2, dtype=torch.float32, device="cuda")
                    for j in range(G):
                        Kn, Vn, Krn, _ = ops.prune_layers([sc], [S.kc[sl]], [S.vc[sl]], n, E_START, hi, E_K, capacity=E_CAP2, rope=(cos, sin),
                                                          acc=([acc_b[j::G]], [acc_n[j::G]]))
                    m = keep
                    Kn, Vn, Krn = Kn[0], Vn[0], Krn[0]
                else:
                    m = n
                    empty = torch.empty(S.Hkv, 0, dtype=torch.int32, device="cuda")
                    Kn, Vn, Krn = ops.kv_compact(S.kc[sl], S.vc[sl], empty, n, n, L=n, capacity=E_CAP2, rope=(cos, sin))
                    acc_n = acc_b
                torch.cuda.synchronize()
                msg = f"{E_MODELS[i][0]} b={b}"
                # the event's output, before the last step touched row m: rows [0, m) moved, the rest zero
                P2 = Layer(S.H, S.Hkv, S.mode, 1, d, tdt, E_CAP2)
                P2.kc[:, :, :m], P2.vc[:, :, :m], P2.krc[:, :, :m], P2.acc[0, :, :m] = Kn[:, :, :m], Vn[:, :, :m], Krn[:, :, :m], acc_n[:, :m]
                one.set(m, m - 1)
                one.advance()
                q, kn, vn = (x[sl] for x in toks[E_TOKENS][i])
                decode(P2, q, kn, vn, one, E_CAP2, ws=ws1)
                torch.cuda.synchronize()
                ws1.check()
                for name in ("kc", "vc", "krc", "acc", "out"):
                    assert torch.equal(getattr(R2, name)[sl], getattr(P2, name)), (msg, name)
                assert torch.equal(R2.st[0][sl, :, :m + 1], P2.st[0][:, :, :m + 1]) and torch.equal(R2.lse[0][sl], P2.lse[0]), msg
                # ---- the oracle on the new cache: out within OUT_TOL
                o, _, _ = orc.attention_core(host(q)[:, :, None], host(kn)[:, :, None], host(vn)[:, :, None], host(Kn[:, :, :m]),
                                             host(Vn[:, :, :m]), np.array([[m]]), None, dt)
                np.testing.assert_allclose(host(R2.out[b]), o[0, 0], err_msg=msg, **OUT_TOL[dt])
        for L in rag2:
            L.ws.check()
    finally:
        ops.set_decode_gqa(prev_mode)
