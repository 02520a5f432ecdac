"""The prune event of a ragged batch (spatten_prune_ragged / ops.prune_ragged): every sequence pruned by the reference's rule at its
own DEVICE length, all layers and sequences in one event.  Everything is compared bit for bit, no tolerance:

1. against tests/ragged_prune_case.py (the rule restated in numpy from the oracle's pieces): K, V, shadow, accumulators, idx of
   pruned sequences, new_lens;
2. against today's single-sequence calls on slice b with host integers: ops.prune_layers(..., acc=...) for a pruned sequence,
   spatten_kv_compact(start = len_b, k = 0) for an unpruned one;
3. sentinels survive beyond out_rows / acc_cols, in the idx rows of unpruned sequences and in the guard bands of padded views.

start 4 / recent 8 / k 16 / 1 coming: keep_rows 27, threshold 28.  Lengths (28, 27, 300, 1, 0, 5) under bound 320: 28 = a window of
k + 1; 27 = the longest unpruned length; 300 = a window longer than one 256-thread pass; 1 and 5 unpruned; 0 an empty slot.
(1100, 28, 27) under bound 1152: the select's next register instantiation.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import ragged_prune_case as rpc
from tests.strided import Guards, bits, padded
from tests.test_gpu_decode import oracle_table
from tests.util import TORCH_DT, dev

pytestmark = pytest.mark.gpu

START, RECENT, K, NC = 4, 8, 16, 1
KEEP = 27
LAYERS, HEADS = 2, 2
OUT_ROWS, ACC_COLS = 40, 48
CAPACITY, ACC_CAP = 44, 56                   # rows / columns of the destinations: the event defines the first OUT_ROWS / ACC_COLS
LENGTHS = {320: (28, 27, 300, 1, 0, 5), 1152: (1100, 28, 27)}
PLANE_SENT, ACC_SENT, IDX_SENT = 7.0, -3.0, -7

_CASES = {}


def case(bound, dt, d, acc_heads):
    """Host inputs and the helper's answer, computed once per geometry and shared (never modified)."""
    key = (bound, dt, d, acc_heads)
    if key not in _CASES:
        lens = LENGTHS[bound]
        B = len(lens)
        seed = 700 + bound + d + acc_heads
        Ks = [orc.synth_normal(seed, 2 * l, (B, HEADS, bound, d), dt) for l in range(LAYERS)]
        Vs = [orc.synth_normal(seed, 2 * l + 1, (B, HEADS, bound, d), dt) for l in range(LAYERS)]
        scores = rpc.make_scores(seed, LAYERS, B, HEADS, bound, lens, START, RECENT, K, NC)
        accs = [np.abs(orc.synth_normal(seed, 20 + l, (B, acc_heads, bound), "f32")) for l in range(LAYERS)]
        want = rpc.reference(scores, Ks, Vs, lens, START, RECENT, K, NC, OUT_ROWS, dt, accs=accs, acc_cols=ACC_COLS)
        _CASES[key] = dict(lens=lens, Ks=Ks, Vs=Vs, scores=scores, accs=accs, want=want)
    return _CASES[key]


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def same(t, a, dt=None):
    """device tensor == host array, bit for bit"""
    w = f32(a) if dt is None else dev(a, dt)
    return torch.equal(bits(t), bits(w))


class Device:
    def __init__(self, c, dt, d, acc_heads, bound):
        tdt = TORCH_DT[dt]
        B = len(c["lens"])
        self.B, self.dt, self.tdt = B, dt, tdt
        self.Ks, self.Vs = [dev(x, dt) for x in c["Ks"]], [dev(x, dt) for x in c["Vs"]]
        self.scores, self.accs = [f32(x) for x in c["scores"]], [f32(x) for x in c["accs"]]
        self.lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        self.cos, self.sin = oracle_table(CAPACITY + 4, d, dt)
        mk = lambda: [torch.full((B, HEADS, CAPACITY, d), PLANE_SENT, dtype=tdt, device="cuda") for _ in range(LAYERS)]
        self.Kd, self.Vd, self.Krd = mk(), mk(), mk()
        self.acc_dst = [torch.full((B, acc_heads, ACC_CAP), ACC_SENT, dtype=torch.float32, device="cuda") for _ in range(LAYERS)]
        self.idx = torch.full((LAYERS, B, HEADS, K), IDX_SENT, dtype=torch.int32, device="cuda")
        self.new_lens = torch.full((B,), IDX_SENT, dtype=torch.int32, device="cuda")

    def run(self, bound, lens=None):
        from spatten_amd import ops
        return ops.prune_ragged(self.scores, self.Ks, self.Vs, self.lens if lens is None else lens, bound, START, RECENT, K, NC,
                                CAPACITY, (self.cos, self.sin), acc=self.accs, out_rows=OUT_ROWS, acc_cols=ACC_COLS,
                                dst=(self.Kd, self.Vd, self.Krd), idx=self.idx, new_lens=self.new_lens, acc_dst=self.acc_dst)


def check_against_the_helper(dv, c):
    want, lens = c["want"], c["lens"]
    assert dv.new_lens.tolist() == want["new_lens"].tolist()
    for l in range(LAYERS):
        for name, got in (("K", dv.Kd), ("V", dv.Vd), ("Kr", dv.Krd)):
            assert same(got[l][:, :, :OUT_ROWS], want[name][l], dv.dt), (name, l)
            assert (got[l][:, :, OUT_ROWS:] == PLANE_SENT).all(), (name, l)            # beyond out_rows: untouched
        assert same(dv.acc_dst[l][:, :, :ACC_COLS], want["acc"][l]), l
        assert (dv.acc_dst[l][:, :, ACC_COLS:] == ACC_SENT).all(), l
        for b, n in enumerate(lens):
            if rpc.needs_pruning(n, START, RECENT, K, NC):
                assert dv.idx[l, b].tolist() == want["idx"][(l, b)].tolist(), (l, b)
            else:
                assert (dv.idx[l, b] == IDX_SENT).all(), (l, b)                        # an unpruned sequence's idx rows: untouched


def check_against_the_single_sequence_calls(dv, c, acc_heads):
    """Today's calls on slice b, driven by host integers."""
    from spatten_amd import ops
    g = acc_heads // HEADS
    rope = (dv.cos, dv.sin)
    for b, n in enumerate(c["lens"]):
        Kb, Vb = [x[b:b + 1] for x in dv.Ks], [x[b:b + 1] for x in dv.Vs]
        if rpc.needs_pruning(n, START, RECENT, K, NC):
            hi = n - RECENT + NC
            for j in range(g):                           # accumulator rows j, j + g, ...: one per KV head, in KV-head order
                a_src = [x[b, j::g] for x in dv.accs]
                a_dst = [torch.zeros(HEADS, KEEP, dtype=torch.float32, device="cuda") for _ in range(LAYERS)]
                Kn, Vn, Krn, idx = ops.prune_layers([s[b] for s in dv.scores], Kb, Vb, n, START, hi, K, capacity=CAPACITY, rope=rope,
                                                    acc=(a_src, a_dst))
                for l in range(LAYERS):
                    assert torch.equal(dv.acc_dst[l][b, j::g, :KEEP], a_dst[l]), (b, l, j)
            m = KEEP
            for l in range(LAYERS):
                assert torch.equal(dv.idx[l, b], idx[l]), (b, l)
        else:
            m = n
            empty = torch.empty(HEADS, 0, dtype=torch.int32, device="cuda")
            res = [ops.kv_compact(Kb[l], Vb[l], empty, n, n, L=n, capacity=CAPACITY, rope=rope) for l in range(LAYERS)]
            Kn, Vn, Krn = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
            for l in range(LAYERS):
                assert torch.equal(dv.acc_dst[l][b, :, :n], dv.accs[l][b, :, :n]), (b, l)
        for l in range(LAYERS):
            for got, ref in ((dv.Kd, Kn), (dv.Vd, Vn), (dv.Krd, Krn)):
                assert ref[l].shape[2] == m and torch.equal(bits(got[l][b:b + 1, :, :m]), bits(ref[l])), (b, l)
                assert not got[l][b, :, m:OUT_ROWS].any(), (b, l)
            assert not dv.acc_dst[l][b, :, m:ACC_COLS].any(), (b, l)


@pytest.mark.parametrize("acc_heads", [2, 4])
@pytest.mark.parametrize("dt,d", [("bf16", 128), ("f16", 128), ("f32", 64)])
@pytest.mark.parametrize("bound", [320, 1152])
def test_ragged_prune_event(bound, dt, d, acc_heads):
    c = case(bound, dt, d, acc_heads)
    dv = Device(c, dt, d, acc_heads, bound)
    Kn, Vn, Krn, idx, new_lens, new_accs = dv.run(bound)
    torch.cuda.synchronize()
    assert Kn[0] is dv.Kd[0] and new_accs[0] is dv.acc_dst[0] and idx is dv.idx and new_lens is dv.new_lens
    check_against_the_helper(dv, c)
    check_against_the_single_sequence_calls(dv, c, acc_heads)


def test_ragged_prune_event_allocates_its_own_destinations_and_skips_optional_outputs():
    """Without dst / acc / rope: fresh [B, H, capacity, d] planes of which every row is defined, no shadow, no accumulators."""
    from spatten_amd import ops
    c = case(320, "bf16", 128, 2)
    dv = Device(c, "bf16", 128, 2, 320)
    Kn, Vn, Krn, idx, new_lens, new_accs = ops.prune_ragged(dv.scores, dv.Ks, dv.Vs, dv.lens, 320, START, RECENT, K, NC, OUT_ROWS)
    torch.cuda.synchronize()
    assert Krn is None and new_accs is None and new_lens.tolist() == c["want"]["new_lens"].tolist()
    for l in range(LAYERS):
        assert Kn[l].shape == (dv.B, HEADS, OUT_ROWS, 128)
        assert same(Kn[l], c["want"]["K"][l], "bf16") and same(Vn[l], c["want"]["V"][l], "bf16")


def test_ragged_prune_event_on_padded_views_with_guard_bands():
    """Every strided argument a padded view with pairwise distinct strides inside a guarded parent: the helper's bits in the views,
    not one byte outside them."""
    bound, dt, d, acc_heads = 320, "bf16", 128, 4
    c = case(bound, dt, d, acc_heads)
    dv = Device(c, dt, d, acc_heads, bound)
    g = Guards()

    def pad_all(name, ts, pads, guard=None):
        out = []
        for l, t in enumerate(ts):
            view, parent, mask = padded(t, pads, guard)
            g.add(f"{name}[{l}]", parent, mask)
            out.append(view)
        return out

    dv.scores = pad_all("scores", dv.scores, (1, 2, 24))
    dv.Ks, dv.Vs = pad_all("K", dv.Ks, (1, 1, 8, 0)), pad_all("V", dv.Vs, (1, 1, 8, 0))
    dv.Kd, dv.Vd, dv.Krd = (pad_all(n, t, (1, 2, 16, 0), PLANE_SENT) for n, t in (("Kd", dv.Kd), ("Vd", dv.Vd), ("Krd", dv.Krd)))
    dv.accs = pad_all("acc", dv.accs, (1, 1, 16))
    dv.acc_dst = pad_all("acc_dst", dv.acc_dst, (1, 3, 8), ACC_SENT)
    (dv.idx,) = pad_all("idx", [dv.idx], "flat", IDX_SENT)
    (dv.new_lens,) = pad_all("new_lens", [dv.new_lens], "flat", IDX_SENT)
    lens_view = pad_all("lens", [dv.lens], (3,))[0]
    strides = [dv.scores[0].stride(0), dv.scores[0].stride(1), dv.Ks[0].stride(0), dv.Ks[0].stride(1), dv.Kd[0].stride(0),
               dv.Kd[0].stride(1), dv.accs[0].stride(0), dv.accs[0].stride(1), dv.acc_dst[0].stride(0), dv.acc_dst[0].stride(1)]
    assert len(set(strides)) == len(strides), strides
    g.snapshot()
    dv.run(bound, lens=lens_view)
    torch.cuda.synchronize()
    g.check()
    check_against_the_helper(dv, c)


def test_ragged_prune_event_reads_the_lengths_in_place_from_the_step_states():
    from spatten_amd import ops
    bound, dt, d, acc_heads = 320, "f16", 128, 2
    c = case(bound, dt, d, acc_heads)
    dv = Device(c, dt, d, acc_heads, bound)
    cos, sin = oracle_table(bound + 4, d, dt)
    step = ops.StepState(cos, sin, batch=dv.B)
    step.set(list(c["lens"]), [max(n - 1, 0) for n in c["lens"]])
    lens = step.lengths()
    assert lens.dtype == torch.int32 and lens.shape == (dv.B,) and lens.stride(0) == step.stride // 4
    assert lens.data_ptr() == step.data_ptr() and lens.tolist() == list(c["lens"])
    before = step.buf.clone()
    dv.run(bound, lens=lens)
    torch.cuda.synchronize()
    assert torch.equal(step.buf, before)
    check_against_the_helper(dv, c)
    # ... and hands the new lengths on: a pure stream operation over device tensors
    step.set(dv.new_lens, torch.clamp(dv.new_lens - 1, min=0))
    assert [r[0] for r in step.read()] == c["want"]["new_lens"].tolist()
