"""The fused cascade accumulation on the matrix-core grouped-query decode step (csrc/decode_gqa.hip, CASC): while a KV head's rows
stream once for its query group, the previous step's probabilities are added to the cumulative importance — the same bits the
per-query-head kernel adds (decode_body.h), the step itself untouched, in the static and the device-length form.  Every case
asserts through ops.decode_gqa_form that the grouped form is the one the call takes.  Needs an MI355X.

Geometry behind the shapes: tiles of 32 rows go round-robin to four waves, a split holds at least 128 rows; the previous rows
arrive in 16-byte pieces (8 keys), the piece the bound cuts by ordinary loads."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.util import TORCH_DT, host

pytestmark = pytest.mark.gpu
D = 128


@pytest.fixture
def gqa_forced():
    from spatten_amd import ops
    prev = ops.set_decode_gqa(1)
    yield
    ops.set_decode_gqa(prev)


class Step:
    """One appending step at cached length N (row N - 1 is the new token) with the previous step's stash / (max, sum), produced
    once by the per-query-head kernel at length N - 1 and never changed."""

    def __init__(self, B, H, Hkv, N, dt, d=D, seed=0, extra=9):
        from spatten_amd import ops
        self.B, self.H, self.Hkv, self.N, self.d, self.tdt = B, H, Hkv, N, d, TORCH_DT[dt]
        self.cap = cap = (N + extra + 7) // 8 * 8          # stash rows 16-byte aligned: what the grouped fold asks for
        g = torch.Generator(device="cuda").manual_seed(1000 + seed + N + H)
        rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(self.tdt)
        self.cos, self.sin = ops.rope_table(cap + 8, d, self.tdt, "cuda")
        self.kc = torch.zeros(B, Hkv, cap, d, dtype=self.tdt, device="cuda")
        self.vc, self.krc = torch.zeros_like(self.kc), torch.zeros_like(self.kc)
        self.kc[:, :, :N - 1], self.vc[:, :, :N - 1] = rnd(B, Hkv, N - 1, d), rnd(B, Hkv, N - 1, d)
        ops.build_shadow(self.kc, self.krc, 0, N - 1, self.cos, self.sin)
        self.q, self.kn, self.vn = rnd(B, H, d), rnd(B, Hkv, d), rnd(B, Hkv, d)
        self.prev = torch.zeros(B, H, cap, dtype=self.tdt, device="cuda")
        self.plse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
        mode = ops.set_decode_gqa(0)
        try:
            ops.attn_decode(rnd(B, H, d), None, self.krc, self.vc, N - 1, self.cos, self.sin, N - 2, scores=self.prev, lse=self.plse)
        finally:
            ops.set_decode_gqa(mode)
        torch.cuda.synchronize()

    def run(self, mode, acc=None, prev_len=None, n_splits=0, head_ids=None, expect_form=None):
        """The step on private copies of the caches: (out, stash, lse, appended k / kr / v rows)."""
        from spatten_amd import ops
        N = self.N
        kc, krc, vc = self.kc.clone(), self.krc.clone(), self.vc.clone()
        stash = torch.zeros(self.B, self.H, self.cap, dtype=self.tdt, device="cuda")
        lse = torch.zeros(self.B, self.H, 2, dtype=torch.float32, device="cuda")
        out = torch.zeros(self.B, self.H * self.d, dtype=self.tdt, device="cuda")
        kw = dict(k_new=self.kn, v_new=self.vn, out=out, scores=stash, lse=lse, n_splits=n_splits, head_ids=head_ids,
                  cascade=None if acc is None else (acc, self.prev, self.plse, N - 1 if prev_len is None else prev_len))
        old = ops.set_decode_gqa(mode)
        try:
            if expect_form is not None:
                assert ops.decode_gqa_form(self.q, kc, krc, vc, N, self.cos, self.sin, N - 1, **kw) is expect_form
            ops.attn_decode(self.q, kc, krc, vc, N, self.cos, self.sin, N - 1, **kw)
        finally:
            ops.set_decode_gqa(old)
        torch.cuda.synchronize()
        return out, stash, lse, kc[:, :, N - 1].clone(), krc[:, :, N - 1].clone(), vc[:, :, N - 1].clone()


CASES = [("bf16", 1, 4, 2), ("bf16", 1, 12, 4), ("bf16", 1, 64, 2), ("bf16", 2, 8, 2), ("f16", 1, 12, 4)]


@pytest.mark.parametrize("n_splits", [1, 4])
@pytest.mark.parametrize("N", [5, 130, 600, 1031])
@pytest.mark.parametrize("dt,B,H,Hkv", CASES)
def test_grouped_fold_adds_the_per_head_bits_and_leaves_the_step_alone(dt, B, H, Hkv, N, n_splits):
    from spatten_amd import ops
    s = Step(B, H, Hkv, N, dt)
    acc0 = torch.zeros(H, s.cap, dtype=torch.float32, device="cuda")
    acc1 = torch.zeros_like(acc0)
    s.run(0, acc=acc0, n_splits=n_splits, expect_form=False)
    casc = s.run(1, acc=acc1, n_splits=n_splits, expect_form=True)
    # 1. the same bits as the per-head fold (B = 2: two adds from zero commute)
    assert torch.equal(acc0, acc1)
    np.testing.assert_allclose(host(acc1)[:, :N - 1].sum(1), np.full(H, B), rtol=2e-3)     # probabilities of B rows per head
    guard = torch.full_like(acc0, 7.0)
    s.run(1, acc=guard, n_splits=n_splits, expect_form=True)
    assert bool((guard[:, N - 1:] == 7.0).all()), "touched at or past prev_len"
    assert bool((guard[:, :N - 1] != 7.0).any())
    # 2. the fold leaves the step alone: the plain grouped step on the same inputs
    plain = s.run(1, n_splits=n_splits, expect_form=True)
    for name, a, b in zip(("out", "stash", "lse", "k row", "kr row", "v row"), casc, plain):
        assert torch.equal(a, b), name
    ops.check_workspaces()


@pytest.mark.parametrize("prev_len", [0, 7, 32, 128, 160, 599])
def test_partial_prev_len(prev_len):
    """N = 600 in four splits of 160 rows (tiles 0..4 each): nothing; inside the first tile (and inside a cut 16-byte piece); a
    tile boundary; wave 0's second tile (row 128); a split boundary (160); N - 1."""
    B, H, Hkv, N = 1, 12, 4, 600
    s = Step(B, H, Hkv, N, "bf16", seed=3)
    acc0 = torch.full((H, s.cap), 3.0, dtype=torch.float32, device="cuda")
    acc1 = acc0.clone()
    s.run(0, acc=acc0, prev_len=prev_len, n_splits=4, expect_form=False)
    s.run(1, acc=acc1, prev_len=prev_len, n_splits=4, expect_form=True)
    assert torch.equal(acc0, acc1)
    assert bool((acc1[:, prev_len:] == 3.0).all())
    if prev_len:
        assert bool((acc1[:, :prev_len] > 3.0).all())
        want = 3.0 + orc.softmax_probs(host(s.prev[:, :, :N - 1])[:, :, None, :]).sum(axis=(0, 2))[:, :prev_len]
        np.testing.assert_allclose(host(acc1)[:, :prev_len], want, rtol=2e-3, atol=2e-5)


@pytest.mark.parametrize("dt,B,H,Hkv", [("bf16", 2, 8, 2), ("f16", 1, 12, 4)])
def test_running_sum_over_five_appended_steps(gqa_forced, dt, B, H, Hkv):
    """tests/test_gpu_cascade.py::test_cascade_accumulation_fused_into_the_decode_step on the grouped form: ping-pong stash
    buffers, the oracle accumulates from the kernel's own stash, the last step is flushed by importance_accumulate."""
    from spatten_amd import ops
    P, steps, tdt = 250, 5, TORCH_DT[dt]
    cap = (P + steps + 3 + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(17)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    cos, sin = ops.rope_table(cap + 8, D, tdt, "cuda")
    kc = torch.zeros(B, Hkv, cap, D, dtype=tdt, device="cuda")
    krc, vc = torch.zeros_like(kc), torch.zeros_like(kc)
    kc[:, :, :P], vc[:, :, :P] = rnd(B, Hkv, P, D), rnd(B, Hkv, P, D)
    ops.build_shadow(kc, krc, 0, P, cos, sin)
    acc = torch.zeros(H, cap, dtype=torch.float32, device="cuda")
    want = np.zeros((H, cap), np.float32)
    stash = [torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(2)]
    lse = [torch.zeros(B, H, 2, dtype=torch.float32, device="cuda") for _ in range(2)]
    for t in range(steps):
        n = P + t + 1
        cur, prv = t & 1, (t & 1) ^ 1
        args = (rnd(B, H, D), kc, krc, vc, n, cos, sin, n - 1)
        kw = dict(k_new=rnd(B, Hkv, D), v_new=rnd(B, Hkv, D), scores=stash[cur], lse=lse[cur],
                  cascade=(acc, stash[prv], lse[prv], n - 1) if t > 0 else None)
        assert ops.decode_gqa_form(*args, **kw)
        ops.attn_decode(*args, **kw)
        torch.cuda.synchronize()
        want[:, :n] = orc.cascade_importance_accumulate(want[:, :n], host(stash[cur][:, :, :n])[:, :, None, :])
        if t > 0:     # everything up to the previous step is in the accumulator after this launch
            prev_want = want[:, :n].copy()
            prev_want -= orc.softmax_probs(host(stash[cur][:, :, :n])[:, :, None, :]).sum(axis=(0, 2))
            np.testing.assert_allclose(host(acc)[:, :n], prev_want, rtol=2e-3, atol=2e-5)
    n = P + steps
    ops.importance_accumulate(acc, stash[(steps - 1) & 1][:, :, None, :n], lse[(steps - 1) & 1][:, :, None, :])   # the flush
    np.testing.assert_allclose(host(acc)[:, :n], want[:, :n], rtol=2e-3, atol=2e-5)
    assert float(host(acc)[:, n:].max()) == 0.0


def test_device_length_form_and_captured_graph(gqa_forced):
    """StepState with the bound above the length: eight steps in the host form laid out for the bound, the same eight in the
    device-length form, and one captured step replayed eight times agree bit for bit in out, both stash buffers, both (max, sum)
    buffers and the accumulator (tests/test_gpu_pq_cascade.py::test_device_length_form_and_captured_graph is the pattern)."""
    from spatten_amd import ops
    # (B = 1: one add per accumulator entry and step — with two sequences the order of their adds onto a NON-zero sum is not fixed)
    B, H, Hkv, P, T, bound, cap, tdt = 1, 8, 2, 250, 8, 300, 304, torch.bfloat16   # the bound cuts a 16-byte piece of the stash rows
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    cos, sin = ops.rope_table(cap + 8, D, tdt, "cuda")
    k0, v0 = rnd(B, Hkv, P, D), rnd(B, Hkv, P, D)
    toks = [(rnd(B, H, D), rnd(B, Hkv, D), rnd(B, Hkv, D)) for _ in range(T)]

    class Bufs:
        def __init__(self):
            self.kc = torch.zeros(B, Hkv, cap, D, dtype=tdt, device="cuda")
            self.krc, self.vc = torch.zeros_like(self.kc), torch.zeros_like(self.kc)
            self.kc[:, :, :P], self.vc[:, :, :P] = k0, v0
            ops.build_shadow(self.kc, self.krc, 0, P, cos, sin)
            self.q, self.kn, self.vn = torch.zeros(B, H, D, dtype=tdt, device="cuda"), torch.zeros(B, Hkv, D, dtype=tdt, device="cuda"), \
                torch.zeros(B, Hkv, D, dtype=tdt, device="cuda")
            self.out = torch.zeros(B, H * D, dtype=tdt, device="cuda")
            self.stash = [torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(2)]
            self.lse = [torch.zeros(B, H, 2, dtype=torch.float32, device="cuda") for _ in range(2)]
            self.acc = torch.zeros(H, cap, dtype=torch.float32, device="cuda")

        def feed(self, t):
            for dst, src in zip((self.q, self.kn, self.vn), toks[t]):
                dst.copy_(src)

        def record(self):
            return [x.clone() for x in (self.out, *self.stash, *self.lse, self.acc, self.kc, self.krc, self.vc)]

    bf, eager = Bufs(), []
    for t in range(T):
        n = P + 1 + t
        bf.feed(t)
        cur, prv = t & 1, (t & 1) ^ 1
        args = (bf.q, bf.kc, bf.krc, bf.vc, n, cos, sin, n - 1)
        kw = dict(k_new=bf.kn, v_new=bf.vn, out=bf.out, scores=bf.stash[cur], lse=bf.lse[cur],
                  cascade=(bf.acc, bf.stash[prv], bf.lse[prv], 0 if t == 0 else n - 1), layout=bound)
        assert ops.decode_gqa_form(*args, **kw)
        ops.attn_decode(*args, **kw)
        torch.cuda.synchronize()
        eager.append(bf.record())
    assert float(eager[-1][5][:, :P + T - 1].min()) > 0.0 and float(eager[-1][5][:, P + T - 1:].max()) == 0.0

    st = ops.StepState(cos, sin)

    def step(b):
        st.advance()
        ops.attn_decode(b.q, b.kc, b.krc, b.vc, bound, cos, sin, 0, k_new=b.kn, v_new=b.vn, out=b.out, scores=b.stash[0], lse=b.lse[0],
                        cascade=(b.acc, b.stash[1], b.lse[1], 0), step=st)

    bf2 = Bufs()
    st.set(P, P - 1)
    assert ops.decode_gqa_form(bf2.q, bf2.kc, bf2.krc, bf2.vc, bound, cos, sin, 0, k_new=bf2.kn, v_new=bf2.vn, out=bf2.out,
                               scores=bf2.stash[0], lse=bf2.lse[0], cascade=(bf2.acc, bf2.stash[1], bf2.lse[1], 0), step=st)
    for t in range(T):
        bf2.feed(t)
        step(bf2)
        torch.cuda.synchronize()
        for i, (got, w) in enumerate(zip(bf2.record(), eager[t])):
            assert torch.equal(got, w), f"device-length step {t}, buffer {i}"
    # one captured step, replayed
    bf3 = Bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        st.set(P, P - 1)
        bf3.feed(0)
        step(bf3)                       # warm-up outside the capture (the side stream's workspace), then back to the start
        side.synchronize()
        for x in (bf3.out, *bf3.stash, *bf3.lse, bf3.acc):
            x.zero_()
        for x in (bf3.kc, bf3.krc, bf3.vc):
            x[:, :, P:].zero_()
        st.set(P, P - 1)
        side.synchronize()
        pins = ops.set_ws_pins([])
        try:
            with torch.cuda.graph(gr, stream=side):
                step(bf3)
        finally:
            ops.set_ws_pins(pins)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in range(T):
        bf3.feed(t)
        gr.replay()
        torch.cuda.synchronize()
        for i, (got, w) in enumerate(zip(bf3.record(), eager[t])):
            assert torch.equal(got, w), f"replay {t}, buffer {i}"
    ops.check_workspaces()


def test_steps_the_form_does_not_serve_still_work():
    """A cascade step with a head list, and one at d = 64, under mode 1: the predicate says no, the results are mode 0's."""
    B, H, Hkv, N = 1, 8, 2, 300
    s = Step(B, H, Hkv, N, "bf16", seed=8)
    ids = torch.tensor([0, 3, 4, 6], dtype=torch.int32, device="cuda")
    s64 = Step(B, H, Hkv, N, "bf16", d=64, seed=9)
    for step, kw in ((s, dict(head_ids=ids)), (s64, {})):
        accs, res = [], []
        for mode in (0, 1):
            acc = torch.zeros(H, step.cap, dtype=torch.float32, device="cuda")
            res.append(step.run(mode, acc=acc, expect_form=False, **kw))
            accs.append(acc)
        assert torch.equal(accs[0], accs[1]) and float(accs[1].sum()) > 0.0
        for a, b in zip(res[0], res[1]):
            assert torch.equal(a, b)
