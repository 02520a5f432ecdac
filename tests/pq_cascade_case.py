"""The multi-step case of the profiled decode step with the folded cascade importance (spatten_attn_decode_pq_cascade), shared
by tests/test_pq_cascade_cpu.py (the criterion tells a wrong kernel from a right one) and tests/test_gpu_pq_cascade.py (the
kernel).  Test infrastructure; may import oracle/.

A case is ``pq_exact.pq_case`` at the final length N in a regime of tests/regimes.py.  T_STEPS consecutive decode steps run over
its planes: step t sees the first n_t = N - (T_STEPS - 1) + t rows and the case's query rotated at position n_t - 1.  ONE
threshold per case: the midpoint between two neighbouring exact pass-1 max probabilities of the LAST step, so that confident
and flagged heads both occur there; the share of (step, b, h) inside ``pq_exact.flag_band`` is asserted within BAND_CAP."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import spatten_oracle as orc
from tests import pq_exact as px

T_STEPS = 5


@functools.lru_cache(maxsize=None)
def case(dt, kb, vb, d, H, Hkv, N, B=1, regime="flat", seed=23):
    pc = px.pq_case(B, H, Hkv, d, N, dt, regime, kb, vb, seed)
    pc.c32, pc.s32 = orc.rope_table(N + 1, d, dt)
    return pc


def lengths(pc, T=T_STEPS):
    return [max(1, pc.N - (T - 1) + t) for t in range(T)] if pc.N >= T else list(range(1, pc.N + 1))


def step_inputs(pc, n):
    """(rotated query [B,H,d] at position n - 1, the planes' first n rows)."""
    qr = orc.apply_rotary_pos_emb_single(pc.cs.q, pc.c32, pc.s32, np.full((pc.B, 1), n - 1), pc.dt)[:, :, 0]
    return qr, [x[:, :, :n] for x in pc.planes]


def threshold(pc):
    """The case's threshold (see the module docstring) — asserts the band share on the oracle's side, before any comparison."""
    ns = lengths(pc)
    qr, pl = step_inputs(pc, ns[-1])
    p = np.unique(px.pq_exact(qr, *pl, 0.0).p1max.ravel())
    assert p.size >= 2, "every head has the same max probability: no threshold separates them"
    i = int(np.argmax(np.diff(np.log(p))))                  # the widest relative gap
    thr = float(np.sqrt(p[i] * p[i + 1]))
    inside = total = 0
    for n in ns:
        qr, pl = step_inputs(pc, n)
        ex = px.pq_exact(qr, *pl, 0.0)
        inside += int((~px.decided(ex.p1max, thr, ex.tau)).sum())
        total += ex.p1max.size
    assert inside <= px.BAND_CAP * total, f"{inside} of {total} (step, b, h) inside the flag band at threshold {thr!r}"
    return thr


def references(pc, thr, needs):
    """Float64 exact sums, the oracle's fp32 sums and the fp32-logit slack of the steps, for the decisions taken.
    needs: list over steps of [B,H] bool.  Returns (ex_sum [H,N] f64, or_sum [H,N] f32, slack [H,N])."""
    H, N = pc.H, pc.N
    ex_sum, or_sum, slack = np.zeros((H, N)), np.zeros((H, N), np.float32), np.zeros((H, N))
    for n, need in zip(lengths(pc), needs):
        qr, pl = step_inputs(pc, n)
        ex = px.pq_exact(qr, *pl, thr, need=need)
        _, o_lg = px.pq_oracle(qr, *pl, need)
        ex_sum[:, :n] += ex.p.sum(0)
        slack[:, :n] += px.cascade_slack(ex.p, px.logit_err32(ex.absdot))
        or_sum[:, :n] = (or_sum[:, :n] + orc.softmax_probs(o_lg).sum(0, dtype=np.float32)).astype(np.float32)
    return ex_sum, or_sum, slack


def emulated_steps(pc, thr):
    """The kernels' documented arithmetic on the CPU (pq_exact.emulate_pq) for every step: (fp32 logit rows, decisions)."""
    rows, needs = [], []
    for n in lengths(pc):
        qr, pl = step_inputs(pc, n)
        em = px.emulate_pq(qr, *pl, thr, pc.dt)
        rows.append(em.z)
        needs.append(em.need)
    return SimpleNamespace(rows=rows, needs=needs)


# the cases of tests/test_gpu_pq_cascade.py: (dtype, (key bits, value bits), head_dim, kv heads of 4 query heads, N, n_splits) —
# every N x n_splits pair at (8, 8) / d 128 / bf16, and every value of every other axis at least once
GPU_CASES = [("bf16", (8, 8), 128, 4, N, ns) for N in (5, 130, 600, 1031) for ns in (1, 4)] + [
    ("f32", (4, 8), 64, 2, 130, 4), ("f32", (6, 6), 128, 4, 600, 1), ("bf16", (6, 6), 64, 4, 1031, 4),
    ("bf16", (4, 8), 128, 2, 600, 4), ("f32", (8, 8), 64, 2, 1031, 1)]
