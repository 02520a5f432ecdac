#!/usr/bin/env python3
"""Device time of the profiled decode step with the cascade importance folded into its launches (attn_decode_pqv(cascade=) ->
spatten_attn_decode_pq_cascade) next to the plain profiled step (attn_decode_pqv) and the composed step at keep 1.0
(attn_decode_pq_local_v with cascade=: four launches).  The routes ALTERNATE in one process on the same planes: each is captured
once in a HIP graph of `--reps` steps, then `--runs` rounds time one replay batch of every route in turn with HIP events; the
line of a route is the median and min..max of its rounds, per step.

    python tools/probe_pq_cascade.py [--shapes 40x8192 32x4096] [--confidence trace all] [--profile 8 8] [--runs 7]
    python tools/probe_pq_cascade.py --single fused --shapes 40x8192 --confidence trace      # one route, for a profiler

Confidence as bench.py --pq-confidence builds it: "trace" = ~7 % of the heads flagged for the LSB refetch (a confident head's
newest key is 0.9 x its query), "all" = every head flagged (threshold 2.0).  The fused and the composed route fold a full row
(prev_len = rows - 1) on every step."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatten_amd import ops  # noqa: E402

ROUTES = ("plain", "fused", "composed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["40x8192", "32x4096"], help="HEADSxROWS")
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--profile", type=int, nargs=2, default=(8, 8))
    ap.add_argument("--confidence", nargs="+", choices=["trace", "all"], default=["trace", "all"])
    ap.add_argument("--reps", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--single", choices=ROUTES, default=None, help="run only this route")
    args = ap.parse_args()
    print(f"# probe_pq_cascade: graphs of {args.reps} steps, median [min .. max] of {args.runs} alternating rounds, us per step")
    for shape in args.shapes:
        H, N = (int(x) for x in shape.split("x"))
        for conf in args.confidence:
            measure(args, H, N, conf)
    ops.check_workspaces()


def measure(args, H, N, confidence):
    d = args.head_dim
    kb, vb = args.profile
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
    cos, sin = ops.rope_table(N + 64, d, dt, dev)
    K, V, q = rnd(1, H, N, d), rnd(1, H, N, d), rnd(1, H, d)
    thr = 0.05
    if confidence == "trace":
        conf = torch.rand(1, H, device=dev, generator=g) < 0.93
        K[:, :, N - 1] = torch.where(conf[:, :, None], (0.9 * q.float()).to(dt), K[:, :, N - 1])
    else:
        thr = 2.0
    Kr = ops.rope_single(K, cos, sin)
    planes = ops.PQProfilePlanes(1, H, H, N, d, dev, key_bits=kb, value_bits=vb)
    ops.pq_pack_planes(Kr, V, planes, 0, N)
    out = torch.empty(1, H * d, dtype=dt, device=dev)
    scores = torch.empty(1, H, N, dtype=dt, device=dev)
    lse = torch.zeros(1, H, 2, dtype=torch.float32, device=dev)
    prev = torch.zeros(1, H, 2, dtype=torch.float32, device=dev)
    acc = torch.zeros(H, N, dtype=torch.float32, device=dev)
    need = torch.zeros(H, dtype=torch.int32, device=dev)
    ws = ops.DecodeWorkspace(1, H, d, dev)
    common = dict(out=out, need_lsb=need, workspace=ws)
    fns = {
        "plain": lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, scores=scores, lse=lse, **common),
        "fused": lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, scores=scores, lse=lse,
                                             cascade=(acc, prev, N - 1), **common),
        "composed": lambda: ops.attn_decode_pq_local_v(q, planes, N, cos, sin, N - 1, thr, N, scores, lse, keep_fraction=1.0,
                                                       cascade=(acc, prev, N - 1), **common),
    }
    routes = [args.single] if args.single else list(ROUTES)
    fns["plain"]()
    torch.cuda.synchronize()
    print(f"== {H} heads x {N} rows, d = {d}, bf16, profile {(kb, vb)}, confidence {confidence}: {int(need.sum().item())} of {H} "
          f"heads refetch the LSB plane", flush=True)
    side = torch.cuda.Stream(device=dev)
    graphs = {}
    with torch.cuda.stream(side):
        for r in routes:
            fns[r]()                      # (the side stream's workspaces; the fused / composed routes leave logits to fold)
            side.synchronize()
            graphs[r] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[r], stream=side):
                for _ in range(args.reps):
                    fns[r]()
            graphs[r].replay()
            side.synchronize()
        times = {r: [] for r in routes}
        for _ in range(args.runs):
            for r in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(5):
                    graphs[r].replay()
                e1.record(side)
                side.synchronize()
                times[r].append(e0.elapsed_time(e1) * 1e3 / (5 * args.reps))
    for r in routes:
        t = times[r]
        print(f"{r:<9}: {statistics.median(t):8.2f} us   [{min(t):.2f} .. {max(t):.2f}]", flush=True)
    if not args.single:
        m = {r: statistics.median(times[r]) for r in routes}
        print(f"fused / composed = {m['fused'] / m['composed']:.3f}   fused / plain = {m['fused'] / m['plain']:.3f}", flush=True)


if __name__ == "__main__":
    main()
