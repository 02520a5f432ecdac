#!/usr/bin/env python3
"""Device time of the quantised-query decode over the planes (attn_decode_pqv(query_bits=8) -> spatten_attn_decode_pq_qint:
integer dot products) next to attn_decode_pqv with the model-dtype query (spatten_attn_decode_pq), ALTERNATED in the same
process, at the c5 geometry.  Three legs per profile: the MSB pass alone, the traces' refetch rate (~7.5 % of the heads
flagged) and every head flagged.  Each variant is captured in a HIP graph of `reps` steps and timed with HIP events around
its replays; `repeats` such measurements per variant, taken in turns (A B A B ...): the median and the spread (min .. max)
are printed.  Every profile is a child process under `timeout -k 10 <s>`; a failed step ends the probe with its exit status.

    python tools/probe_pq_qint.py [--heads 40] [--rows 8192] [--profiles 8 4] [--query-bits 8] [--repeats 7]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatten_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--profiles", type=int, nargs="+", default=(8, 4), help="key MSB bits (value bits 8)")
    ap.add_argument("--query-bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return measure(args, args.child)
    for kb in args.profiles:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(kb), "--heads", str(args.heads), "--rows", str(args.rows),
               "--head-dim", str(args.head_dim), "--query-bits", str(args.query_bits), "--reps", str(args.reps),
               "--repeats", str(args.repeats)]
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd)
        if r.returncode != 0:
            print(f"step failed (exit {r.returncode}): {' '.join(cmd)}", flush=True)
            sys.exit(r.returncode)


def measure(args, kb):
    H, N, d = args.heads, args.rows, args.head_dim
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
    cos, sin = ops.rope_table(N + 64, d, dt, dev)
    V, q = rnd(1, H, N, d), rnd(1, H, d)
    out = torch.empty(1, H * d, dtype=dt, device=dev)
    scores = torch.empty(1, H, N, dtype=dt, device=dev)
    need = torch.zeros(H, dtype=torch.int32, device=dev)
    qq = (torch.zeros(1, H, d, dtype=torch.int8, device=dev), torch.zeros(1, H, dtype=torch.float32, device=dev))
    ws = ops.DecodeWorkspace(1, H, d, dev)
    side = torch.cuda.Stream(device=dev)

    def graph_of(fn):
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(args.reps):
                    fn()
            gr.replay()
            side.synchronize()
        return gr

    def once(gr):
        with torch.cuda.stream(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(5):
                gr.replay()
            e1.record(side)
            side.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (5 * args.reps)

    print(f"geometry: {H} heads x {N} rows, d = {d}, profile ({kb}, 8), query_bits {args.query_bits}; us per step, median of "
          f"{args.repeats} (min .. max), the two entry points alternated")
    for leg in ("msb pass only", "trace refetch rate", "every head flagged"):
        K = rnd(1, H, N, d)
        thr, msb_only = 0.05, leg == "msb pass only"
        if leg == "every head flagged":
            thr = 2.0
        else:   # a confident head's newest key is 0.9 x its query: max probability ~ 0.6 >> the threshold (bench.py --pq-confidence trace)
            conf = torch.rand(1, H, device=dev, generator=g) < 0.925
            K[:, :, N - 1] = torch.where(conf[:, :, None], (0.9 * q.float()).to(dt), K[:, :, N - 1])
        planes = ops.PQProfilePlanes(1, H, H, N, d, dev, key_bits=kb, value_bits=8)
        ops.pq_pack_planes(ops.rope_single(K, cos, sin), V, planes, 0, N)
        kw = dict(out=out, need_lsb=need, scores=scores, workspace=ws, msb_only=msb_only)
        f16 = lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, **kw)
        fqi = lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, query_bits=args.query_bits, q_quant=qq, **kw)
        flags = []
        for fn in (f16, fqi):
            fn()
            torch.cuda.synchronize()
            flags.append(int(need.sum().item()))
        ga, gb = graph_of(f16), graph_of(fqi)
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(once(ga))
            tb.append(once(gb))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"  {leg:<19} flagged {flags[0]:2d} / {flags[1]:2d} of {H}:  16-bit query {ma:7.2f} ({min(ta):.2f} .. {max(ta):.2f})   "
              f"integer dot {mb:7.2f} ({min(tb):.2f} .. {max(tb):.2f})   ratio {mb / ma:.3f}", flush=True)
    ops.check_workspaces()


if __name__ == "__main__":
    main()
