"""The CASCADE step over the profiled planes on a RAGGED batch: ONE launch with one step state and one accumulator per sequence
(spatten_attn_decode_pq_cascade_ragged, ops.attn_decode_pqv(step=StepState(batch=B), cascade=(acc [B,H,L], prev_lse, 0))) against
what serves that batch without it — B launches of the batch-1 shared-state cascade step (spatten_attn_decode_pq_cascade) with B
states, each laid out for the same bound — and against the ragged PLAIN profiled step (no fold), which shows what the fold costs.

B = 4, lengths 4096 / 2048 / 1024 / 512 under a 4096-row bound, 32 heads, d 128, (8, 8) planes, bf16; no route appends (the
cascade forms take the row from spatten_kv_append_planes[_ragged]).  Every route streams the bound for every sequence, so the plane
bytes are the same; the cascade routes add the read of the previous logits and one add per folded row (every state has taken two
steps since its set: word 3 = length - 1 rows are folded per step).  Two thresholds: 0.0 (no head flagged) and 2.0 (every head).

Method (ragged_pq_bench.py's): graphs of 20 steps rotating over enough layer planes to defeat the Infinity Cache, median and
min .. max of 7 timings per route, the routes alternating in one process on the same planes.
usage: ragged_pq_cascade_bench.py"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("SPATTEN_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from spatten_amd import ops

d, tdt, STEPS, RUNS = 128, torch.bfloat16, 20, 7
KB, VB = 8, 8


def time_routes(routes, label):
    """routes: name -> function issuing STEPS steps.  Captured once each, then RUNS alternating timings of 5 replays."""
    graphs = {}
    for name, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs[name] = gr
    for gr in graphs.values():
        for _ in range(3):
            gr.replay()
    torch.cuda.synchronize()
    times = {n: [] for n in graphs}
    for _ in range(RUNS):
        for n, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / (5 * STEPS))
    for n, t in times.items():
        print(f"{label} route {n}: median {statistics.median(t):7.2f} us/step  ({min(t):.2f} .. {max(t):.2f} of {RUNS})", flush=True)
    return {n: statistics.median(t) for n, t in times.items()}


def ragged(H, lens, bound):
    B = len(lens)
    per_layer = B * H * bound * (d * KB // 8 + d // 2 + d * VB // 8 + 12 + 4)
    L = max(2, int(600e6 // per_layer) + 1)
    cos, sin = ops.rope_table(bound + 8, d, tdt, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    layers = []
    for _ in range(L):
        kr, v = rnd(B, H, bound, d), rnd(B, H, bound, d)
        pl = ops.PQProfilePlanes(B, H, H, bound, d, "cuda", key_bits=KB, value_bits=VB)
        ops.pq_pack_planes(kr, v, pl, 0, bound)
        views = [ops.PQProfilePlanes(1, H, H, bound, d, "cuda", key_bits=KB, value_bits=VB,
                                     tensors=tuple(x[b:b + 1] for x in (pl.msb, pl.lsb, pl.scale, pl.vq, pl.vscale, pl.msb_logit)))
                 for b in range(B)]
        layers.append((pl, views, torch.zeros(B, H, bound, dtype=torch.float32, device="cuda")))
        del kr, v
    q = rnd(B, H, d)
    out = torch.zeros(B, H * d, dtype=tdt, device="cuda")
    st = torch.zeros(B, H, bound, dtype=tdt, device="cuda")
    need = torch.zeros(B * H, dtype=torch.int32, device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    prev = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    prev[..., 1] = 1.0                                       # (max 0, sum 1: the first fold of the zero-filled logits stays finite)
    ws, ws1 = ops.DecodeWorkspace(B, H, d, "cuda"), ops.DecodeWorkspace(1, H, d, "cuda")
    step = ops.StepState(cos, sin, batch=B)
    step.set([n - 2 for n in lens], [n - 3 for n in lens])
    step.advance()
    step.advance()                                           # two steps since the set: word 3 = length - 1 rows to fold
    singles = []
    for n in lens:
        s1 = ops.StepState(cos, sin)
        s1.set(n - 2, n - 3)
        s1.advance()
        s1.advance()
        singles.append(s1)
    torch.cuda.synchronize()
    assert [w[0] for w in step.read(all_words=True)] == list(lens) and [w[3] for w in step.read(all_words=True)] == [n - 1 for n in lens]
    for thr in (0.0, 2.0):
        def ragged_cascade():
            for i in range(STEPS):
                pl, _, acc = layers[i % L]
                ops.attn_decode_pqv(q, pl, bound, cos, sin, 0, thr, out=out, need_lsb=need, scores=st, lse=lse, step=step, workspace=ws,
                                    cascade=(acc, prev, 0))

        def cascade_per_sequence():
            for i in range(STEPS):
                _, views, acc = layers[i % L]
                for b in range(B):
                    ops.attn_decode_pqv(q[b:b + 1], views[b], bound, cos, sin, 0, thr, out=out[b:b + 1], need_lsb=need[b * H:(b + 1) * H],
                                        scores=st[b:b + 1], lse=lse[b:b + 1], step=singles[b], workspace=ws1,
                                        cascade=(acc[b], prev[b:b + 1], 0))

        def ragged_plain():
            for i in range(STEPS):
                pl, _, _ = layers[i % L]
                ops.attn_decode_pqv(q, pl, bound, cos, sin, 0, thr, out=out, need_lsb=need, scores=st, lse=lse, step=step, workspace=ws)

        names = ("one ragged cascade launch", f"{B} cascade launches of batch 1", "one ragged plain launch")
        med = time_routes(dict(zip(names, (ragged_cascade, cascade_per_sequence, ragged_plain))),
                          f"H={H} bound={bound} lengths={lens} ({KB},{VB}) thr={thr} layers={L}")
        print(f"    ragged cascade / per-sequence cascade = {med[names[0]] / med[names[1]]:.3f}; "
              f"ragged cascade / ragged plain = {med[names[0]] / med[names[2]]:.3f}", flush=True)
        ws.check()
        ws1.check()


ragged(32, (4096, 2048, 1024, 512), 4096)
