"""The profiled decode step with the cascade importance folded into its launches (ops.attn_decode_pqv(cascade=) ->
spatten_attn_decode_pq_cascade) on the cases of tests/pq_cascade_case.py:

1. the fold does not disturb the step: out, stash, lse, need_lsb bit-identical to spatten_attn_decode_pq; msb_logit rows of
   confident heads too, rows of flagged heads bit-identical to what the composed step (spatten_attn_decode_pq_local_v) leaves;
2. the accumulator bit-identical to spatten_importance_accumulate(SPATTEN_F32) folding the fp32 logit rows and lse of the
   earlier steps, one call per step (B = 1: one add per element and step), and again after the flush;
3. the accumulator against float64 exact math (pq_exact.check_cascade with cascade_slack);
4. prev_len = 0, partial prev_len inside a split and on a split boundary; 5. prev_lse and the untouched rows of unlaunched
   heads; 6. B = 2; 7. the device-length form and a captured graph; 8. refusals.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pq_cascade_case as pcc
from tests import pq_exact as px
from tests.test_gpu_pq_regimes import Inputs
from tests.util import TORCH_DT, host

pytestmark = pytest.mark.gpu

H = 4


def _inputs(pc, mha=False, extra=9):
    """Device planes of the case (every row packed); mha: the kv heads repeated (the composed step takes no grouped caches — a
    query head reads the same plane rows either way)."""
    from oracle import spatten_oracle as orc
    kr, v = pc.cs.kr, pc.cs.vc
    if mha and pc.Hkv != pc.H:
        kr, v = orc.repeat_kv(kr, pc.H // pc.Hkv), orc.repeat_kv(v, pc.H // pc.Hkv)
    return Inputs(pc.qr, pc.cs.q[:, :, 0], kr, v, pc.kb, pc.vb, pc.dt, extra)


class Bufs:
    def __init__(self, inp, guard=0.0):
        B, d, cap, tdt = inp.B, inp.d, inp.cap, TORCH_DT[inp.dt]
        f = lambda *s, dt=torch.float32: torch.full(s, guard, dtype=dt, device="cuda")
        self.out, self.scores = f(B, H * d, dt=tdt), f(B, H, cap, dt=tdt)
        self.lse, self.prev, self.acc = f(B, H, 2), f(B, H, 2), f(H, cap)
        self.need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")


def _cascade(inp, bf, n, thr, prev_len, ns=0, **kw):
    from spatten_amd import ops
    ops.attn_decode_pqv(inp.qd, inp.pl, n, inp.cos, inp.sin, n - 1, thr, out=bf.out, need_lsb=bf.need, scores=bf.scores,
                        lse=bf.lse, n_splits=ns, cascade=(bf.acc, bf.prev, prev_len), **kw)


def _run_steps(pc, inp, bf, thr, ns):
    """The case's steps with prev_len = kv_len - 1 (0 at the first); after each: prev_lse == lse, and the accumulator equal to
    the library's own fold of the earlier steps' rows.  Returns the decisions per step."""
    from spatten_amd import ops
    ref = torch.zeros_like(bf.acc)
    needs, pend = [], None
    for t, n in enumerate(pcc.lengths(pc)):
        _cascade(inp, bf, n, thr, 0 if t == 0 else n - 1, ns)
        if pend is not None:
            ops.importance_accumulate(ref, pend[0][:, :, None, :], pend[1][:, :, None, :])
        torch.cuda.synchronize()
        assert torch.equal(bf.prev, bf.lse), f"step {t}: prev_lse is not this step's lse"
        if inp.B == 1:
            assert torch.equal(bf.acc, ref), f"step {t}: accumulator differs from the library's fold of steps 0..{t - 1}"
        pend = (inp.pl.msb_logit[:, :, :n].clone(), bf.lse.clone())
        needs.append(bf.need.cpu().numpy().reshape(inp.B, H).astype(bool))
    n = pcc.lengths(pc)[-1]
    ops.importance_accumulate(bf.acc, inp.pl.msb_logit[:, :, None, :n], bf.lse[:, :, None, :])          # the flush
    ops.importance_accumulate(ref, pend[0][:, :, None, :], pend[1][:, :, None, :])
    torch.cuda.synchronize()
    if inp.B == 1:
        assert torch.equal(bf.acc, ref), "accumulator differs after the flush"
    return needs


def _check_exact(pc, thr, needs, acc, name):
    for n, need in zip(pcc.lengths(pc), needs):
        qr, pl = pcc.step_inputs(pc, n)
        ex0 = px.pq_exact(qr, *pl, 0.0)
        px.check_flags(need, ex0.p1max, thr, ex0.tau, f"{name} n={n}")
    ex_sum, or_sum, slack = pcc.references(pc, thr, needs)
    px.check_cascade(acc.cpu().numpy()[:, :pc.N], or_sum, ex_sum, len(needs), name=name, slack=slack)


@pytest.mark.parametrize("dt,prof,d,Hkv,N,ns", pcc.GPU_CASES)
def test_fold_leaves_the_step_alone_and_accumulates_exactly(dt, prof, d, Hkv, N, ns):
    from spatten_amd import ops
    pc = pcc.case(dt, prof[0], prof[1], d, H, Hkv, N)
    thr = pcc.threshold(pc)                                  # (asserts the band share on the oracle)
    inp, bf = _inputs(pc), None
    bf = Bufs(inp)
    needs = _run_steps(pc, inp, bf, thr, ns)                 # checks 2 and 5 (prev_lse)
    need = needs[-1][0]
    assert need.any() and not need.all(), "the threshold must leave confident and flagged heads"
    _check_exact(pc, thr, needs, bf.acc, f"{dt} {prof} d{d} Hkv{Hkv} N{N} ns{ns}")           # check 3
    # check 1, at the last step: the plain step and the composed step on planes of their own
    plain, pb = _inputs(pc), None
    pb = Bufs(plain)
    ops.attn_decode_pqv(plain.qd, plain.pl, N, plain.cos, plain.sin, N - 1, thr, out=pb.out, need_lsb=pb.need, scores=pb.scores,
                        lse=pb.lse, n_splits=ns)
    comp = _inputs(pc, mha=True)
    cb = Bufs(comp)
    ops.attn_decode_pq_local_v(comp.qd, comp.pl, N, comp.cos, comp.sin, N - 1, thr, N, cb.scores, cb.lse, out=cb.out,
                               need_lsb=cb.need, n_splits=ns)
    torch.cuda.synchronize()
    assert torch.equal(bf.out, pb.out) and torch.equal(bf.scores[:, :, :N], pb.scores[:, :, :N])
    assert torch.equal(bf.lse, pb.lse) and torch.equal(bf.need, pb.need) and torch.equal(cb.need, pb.need)
    lg, lg_p, lg_c = (x.pl.msb_logit[0, :, :N] for x in (inp, plain, comp))
    conf = torch.from_numpy(~need).cuda()
    assert torch.equal(lg[conf], lg_p[conf]), "confident heads: msb_logit differs from the plain step's"
    assert torch.equal(lg[~conf], lg_c[~conf]), "flagged heads: msb_logit differs from the composed step's final logits"
    assert not torch.equal(lg[~conf], lg_p[~conf])           # (the plain step leaves their MSB-only logits)
    ops.check_workspaces()


def test_first_step_and_partial_prev_len():
    """N = 600 at 4 splits (chunks of 152 rows): prev_len 0, inside the first split, on a split boundary, inside the third
    split, one short of the length.  The rows below prev_len gain exactly the library's fold, the others keep their guard."""
    from spatten_amd import ops
    pc = pcc.case("bf16", 8, 8, 128, H, H, 600)
    thr = pcc.threshold(pc)
    inp = _inputs(pc)
    bf = Bufs(inp)
    _cascade(inp, bf, 599, thr, 0, 4)
    torch.cuda.synchronize()
    assert not bf.acc.any(), "prev_len = 0 must fold nothing"
    lg0, lse0 = inp.pl.msb_logit.clone(), bf.lse.clone()
    for prev_len in (0, 100, 152, 304, 400, 599):
        inp.pl.msb_logit.copy_(lg0)
        bf.prev.copy_(lse0)
        bf.acc.fill_(7.0)
        want = torch.full_like(bf.acc, 7.0)
        if prev_len:
            ops.importance_accumulate(want, lg0[:, :, None, :prev_len], lse0[:, :, None, :])
        _cascade(inp, bf, 600, thr, prev_len, 4)
        torch.cuda.synchronize()
        assert torch.equal(bf.acc, want), prev_len
        assert (bf.acc[:, prev_len:] == 7.0).all() and (prev_len == 0 or (bf.acc[:, :prev_len] > 7.0).all()), prev_len


def test_head_list_leaves_unlaunched_heads_untouched():
    from spatten_amd import ops
    pc = pcc.case("bf16", 8, 8, 128, H, H, 600)
    thr = pcc.threshold(pc)
    inp, plain = _inputs(pc), _inputs(pc)
    bf, pb = Bufs(inp, guard=3.0), Bufs(plain, guard=3.0)
    hid = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    ha, ha_p = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    ref = torch.full_like(bf.acc, 3.0)
    for t, n in enumerate((599, 600)):
        _cascade(inp, bf, n, thr, 0 if t == 0 else n - 1, 4, head_ids=hid, head_abs=ha)
        ops.attn_decode_pqv(plain.qd, plain.pl, n, plain.cos, plain.sin, n - 1, thr, out=pb.out, need_lsb=pb.need,
                            scores=pb.scores, lse=pb.lse, n_splits=4, head_ids=hid, head_abs=ha_p)
        torch.cuda.synchronize()
        assert torch.equal(bf.prev[:, [0, 2]], bf.lse[:, [0, 2]]) and (bf.prev[:, [1, 3]] == 3.0).all()
        assert torch.equal(bf.out, pb.out) and torch.equal(bf.scores, pb.scores) and torch.equal(bf.lse, pb.lse)
        assert torch.equal(bf.need, pb.need) and torch.equal(ha, ha_p)
        assert (bf.out.view(1, H, -1)[:, [1, 3]] == 3.0).all() and (bf.scores[:, [1, 3]] == 3.0).all()
        if t == 0:
            lg0, lse0 = inp.pl.msb_logit[:, [0, 2], :599].clone(), bf.lse[:, [0, 2]].clone()
    tmp = torch.zeros(2, bf.acc.shape[1], device="cuda")
    ops.importance_accumulate(tmp, lg0[:, :, None, :], lse0[:, :, None, :])
    ref[[0, 2]] += tmp
    # (3.0 + p in one add on both sides: the kernel adds p to the guard, the reference adds the same p to the same guard)
    torch.cuda.synchronize()
    assert torch.equal(bf.acc[[1, 3]], ref[[1, 3]]), "accumulator rows of unlaunched heads were touched"
    assert torch.equal(bf.acc[[0, 2]], ref[[0, 2]])


def test_batch_two_against_exact_math():
    pc = pcc.case("bf16", 8, 8, 128, H, H, 600, B=2)
    thr = pcc.threshold(pc)
    inp = _inputs(pc)
    bf = Bufs(inp)
    needs = _run_steps(pc, inp, bf, thr, 4)
    _check_exact(pc, thr, needs, bf.acc, "B=2")


def test_device_length_form_and_captured_graph():
    """step_state with the bound above the length: bit-identical to the host form laid out for the bound; one captured step
    replayed eight times equals the eager loop bit for bit."""
    from spatten_amd import ops
    T, P = 8, 592
    pc = pcc.case("bf16", 8, 8, 128, H, H, P + T)
    thr = pcc.threshold(pc)
    flagged = 0

    def record(bf, inp, n):
        return [x.clone() for x in (bf.out, bf.scores[:, :, :n], bf.lse, bf.prev, bf.need, bf.acc, inp.pl.msb_logit[:, :, :n])]

    inp = _inputs(pc, extra=40)
    cap, bf, eager = inp.cap, Bufs(inp), []
    for t in range(T):
        n = P + 1 + t
        _cascade(inp, bf, n, thr, 0 if t == 0 else n - 1, 0, layout=cap)
        eager.append(record(bf, inp, n))
        flagged += int(bf.need.sum().item())
    assert 0 < flagged < T * H
    # the device-length form, eager
    inp2 = _inputs(pc, extra=40)
    bf2 = Bufs(inp2)
    st = ops.StepState(inp2.cos, inp2.sin)
    st.set(P, P - 1)

    def step(i, b):
        st.advance()
        ops.attn_decode_pqv(i.qd, i.pl, cap, i.cos, i.sin, 0, thr, out=b.out, need_lsb=b.need, scores=b.scores, lse=b.lse,
                            cascade=(b.acc, b.prev, 0), step=st)

    for t in range(T):
        step(inp2, bf2)
        torch.cuda.synchronize()
        for g, w in zip(record(bf2, inp2, P + 1 + t), eager[t]):
            assert torch.equal(g, w), f"device-length step {t}"
    # one captured step, replayed
    inp3 = _inputs(pc, extra=40)
    bf3 = Bufs(inp3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        st.set(P, P - 1)
        step(inp3, bf3)                 # warm-up outside the capture (the side stream's workspace), then back to the start
        side.synchronize()
        for x in (bf3.out, bf3.scores, bf3.lse, bf3.prev, bf3.acc, inp3.pl.msb_logit):
            x.zero_()
        st.set(P, P - 1)
        side.synchronize()
        pins = ops.set_ws_pins([])
        try:
            with torch.cuda.graph(g, stream=side):
                step(inp3, bf3)
        finally:
            ops.set_ws_pins(pins)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in range(T):
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip(record(bf3, inp3, P + 1 + t), eager[t]):
            assert torch.equal(got, w), f"replay {t}"
    ops.check_workspaces()


def test_refusals_launch_nothing(monkeypatch):
    """The documented status of every refused call; the guard values of every output show that nothing ran."""
    from spatten_amd import _lib, ops
    pc = pcc.case("bf16", 8, 8, 128, H, 2, 130)
    inp = _inputs(pc)
    bf = Bufs(inp, guard=5.0)
    lg0 = inp.pl.msb_logit.clone()
    lib = _lib.load()
    grabbed = []

    class Grab:                          # the argument block ops builds, taken in front of the library
        def __getattr__(self, name):
            return getattr(lib, name)

        def spatten_attn_decode_pq_cascade(self, ref, stream):
            blk = _lib.PQCascadeArgs()
            ctypes.memmove(ctypes.byref(blk), ref, ctypes.sizeof(blk))
            grabbed.append((blk, stream))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Grab())
    _cascade(inp, bf, 130, 0.05, 129, 4)
    monkeypatch.undo()
    good, stream = grabbed[0]

    def call(**edit):
        blk = _lib.PQCascadeArgs()
        ctypes.memmove(ctypes.byref(blk), ctypes.byref(good), ctypes.sizeof(blk))
        for k, v in edit.items():
            obj = blk.step if k.startswith("step_") else blk
            setattr(obj, k[5:] if k.startswith("step_") else k, v)
        return lib.spatten_attn_decode_pq_cascade(ctypes.byref(blk), stream)

    INVALID, UNSUPPORTED = -1, -2
    assert call(importance_acc=None) == INVALID and call(prev_lse=None) == INVALID and call(step_lse=None) == INVALID
    assert call(prev_len=-1) == INVALID and call(prev_len=131) == INVALID
    assert call(struct_size=good.struct_size - 8) == INVALID
    kn = torch.zeros(1, 2, 128, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(1, 2, inp.cap, 128, dtype=torch.bfloat16, device="cuda")
    assert call(step_k_new=kn.data_ptr(), step_v_new=kn.data_ptr(), step_kr_cache=kc.data_ptr(), step_v_cache=kc.data_ptr(),
                step_new_sb=256, step_new_sh=128, step_kv_sb=kc.stride(0), step_kv_sh=kc.stride(1)) == UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _cascade(inp, bf, 130, 0.05, 129, 4, append=(kn, kn, None, kc, kc))
    with pytest.raises(NotImplementedError):
        _cascade(inp, bf, 130, 0.05, 129, 4, query_bits=8)
    with pytest.raises(NotImplementedError):
        _cascade(inp, bf, 130, 0.05, 129, 4, query_bits=8, grouped=True)
    with pytest.raises(ValueError):
        ops.attn_decode_pqv(inp.qd, inp.pl, 130, inp.cos, inp.sin, 129, 0.05, out=bf.out, need_lsb=bf.need, scores=bf.scores,
                            lse=bf.lse, cascade=(bf.acc[:, :100], bf.prev, 129))
    torch.cuda.synchronize()
    for x in (bf.out, bf.scores, bf.lse, bf.prev, bf.acc):
        assert (x == 5.0).all()
    assert (bf.need == -1).all() and torch.equal(inp.pl.msb_logit, lg0) and not (kc != 0).any()
    assert call() == 0                   # the unedited block runs
    torch.cuda.synchronize()
    assert torch.equal(bf.prev, bf.lse) and (bf.need >= 0).all()
