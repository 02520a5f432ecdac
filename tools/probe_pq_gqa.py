#!/usr/bin/env python3
"""Device time of the GROUPED quantised-query decode over the planes (attn_decode_pqv(query_bits=8, grouped=True) ->
spatten_attn_decode_pq_qint_gqa: one plane stream per KV head, int8 MFMA) next to the per-head form (grouped=False ->
spatten_attn_decode_pq_qint), ALTERNATED in the same process on the same planes.  Three legs per shape: the MSB pass alone, the
traces' refetch rate (~7.5 % of the heads flagged) and every head flagged.  Each variant is captured in a HIP graph of `reps`
steps and timed with HIP events around its replays; `repeats` such measurements per variant, taken in turns (A B A B ...): the
median and the spread (min .. max) are printed, with the TB/s of UNIQUE plane bytes of the MSB pass (MSB + value planes + both
scales: 264 bytes per kv row).  Every shape is a child process under `timeout -k 10 <s>`; a failed step ends the probe with its
exit status.

    python tools/probe_pq_gqa.py [--shapes 32/8 64/8] [--rows 4096 8192 16384] [--query-bits 8] [--repeats 7]
    python tools/probe_pq_gqa.py --single 32/8 --rows 16384 --form grouped     # one form, eager steps: for a profiler
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
    ap.add_argument("--shapes", nargs="+", default=("32/8", "64/8"), help="query heads / kv heads")
    ap.add_argument("--rows", type=int, nargs="+", default=(4096, 8192, 16384))
    ap.add_argument("--query-bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--single", default=None, help="H/Hkv: run --steps eager steps of --form at --rows[0] and exit")
    ap.add_argument("--form", default="grouped", choices=("grouped", "per-head"))
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if args.single is not None:
        return single(args)
    if args.child is not None:
        return measure(args, args.child)
    for shape in args.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--rows"] + [str(r) for r in args.rows] + \
              ["--query-bits", str(args.query_bits), "--reps", str(args.reps), "--repeats", str(args.repeats)]
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd)
        if r.returncode != 0:
            print(f"step failed (exit {r.returncode}): {' '.join(cmd)}", flush=True)
            sys.exit(r.returncode)


def setup(H, Hkv, N, leg, dev, g):
    d, dt = 128, torch.bfloat16
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
    cos, sin = ops.rope_table(N + 64, d, dt, dev)
    V, q, K = rnd(1, Hkv, N, d), rnd(1, H, d), rnd(1, Hkv, N, d)
    thr = 2.0 if leg == "every head flagged" else 0.05
    if leg != "every head flagged":
        # a kv row serves G heads: the heads of a confident group share one query and the newest key is 0.9 x that query
        # (max probability ~ 0.6 >> the threshold: bench.py --pq-confidence trace); the other groups keep their own queries
        G = H // Hkv
        conf = torch.rand(1, Hkv, device=dev, generator=g) < 0.925
        q0 = q.view(1, Hkv, G, d)[:, :, :1].expand(1, Hkv, G, d)
        q = torch.where(conf[:, :, None, None], q0, q.view(1, Hkv, G, d)).reshape(1, H, d).contiguous()
        K[:, :, N - 1] = torch.where(conf[:, :, None], (0.9 * q.view(1, Hkv, G, d)[:, :, 0].float()).to(dt), K[:, :, N - 1])
    planes = ops.PQProfilePlanes(1, Hkv, H, N, d, dev, key_bits=8, value_bits=8)
    kr = ops.rope_single(K, cos, sin)
    ops.pq_pack_planes(kr, V, planes, 0, N)
    return q, planes, cos, sin, thr


def measure(args, shape):
    H, Hkv = (int(x) for x in shape.split("/"))
    d, dt, dev = 128, torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
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

    for N in args.rows:
        out = torch.empty(1, H * d, dtype=dt, device=dev)
        scores = torch.empty(1, H, N, dtype=dt, device=dev)
        need = torch.zeros(H, dtype=torch.int32, device=dev)
        qq = (torch.zeros(1, H, d, dtype=torch.int8, device=dev), torch.zeros(1, H, dtype=torch.float32, device=dev))
        ws = ops.DecodeWorkspace(1, H, d, dev)
        unique = Hkv * N * (128 + 128 + 8)
        print(f"geometry: {H} / {Hkv} heads x {N} rows, d = {d}, profile (8, 8), query_bits {args.query_bits}; us per step, median of "
              f"{args.repeats} (min .. max), the two forms alternated; unique plane bytes of the MSB pass {unique / 1e6:.2f} MB")
        for leg in ("msb pass only", "trace refetch rate", "every head flagged"):
            q, planes, cos, sin, thr = setup(H, Hkv, N, leg, dev, g)
            kw = dict(out=out, need_lsb=need, scores=scores, workspace=ws, msb_only=leg == "msb pass only",
                      query_bits=args.query_bits, q_quant=qq)
            fa = lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, **kw)
            fb = lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, grouped=True, **kw)
            flags = []
            for fn in (fa, fb):
                fn()
                torch.cuda.synchronize()
                flags.append(int(need.sum().item()))
            ga, gb = graph_of(fa), graph_of(fb)
            ta, tb = [], []
            for _ in range(args.repeats):
                ta.append(once(ga))
                tb.append(once(gb))
            ma, mb = statistics.median(ta), statistics.median(tb)
            tbs = (lambda us: unique / us * 1e-6)
            print(f"  {leg:<19} flagged {flags[0]:2d} / {flags[1]:2d} of {H}:  per-head {ma:7.2f} ({min(ta):.2f} .. {max(ta):.2f}) "
                  f"{tbs(ma):5.2f} TB/s   grouped {mb:7.2f} ({min(tb):.2f} .. {max(tb):.2f}) {tbs(mb):5.2f} TB/s   ratio {mb / ma:.3f}",
                  flush=True)
        ops.check_workspaces()


def single(args):
    H, Hkv = (int(x) for x in args.single.split("/"))
    N, d, dt, dev = args.rows[0], 128, torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    q, planes, cos, sin, thr = setup(H, Hkv, N, "trace refetch rate", dev, g)
    out = torch.empty(1, H * d, dtype=dt, device=dev)
    scores = torch.empty(1, H, N, dtype=dt, device=dev)
    need = torch.zeros(H, dtype=torch.int32, device=dev)
    qq = (torch.zeros(1, H, d, dtype=torch.int8, device=dev), torch.zeros(1, H, dtype=torch.float32, device=dev))
    ws = ops.DecodeWorkspace(1, H, d, dev)
    for _ in range(args.steps):
        ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, out=out, need_lsb=need, scores=scores, workspace=ws,
                            query_bits=args.query_bits, q_quant=qq, grouped=args.form == "grouped")
    torch.cuda.synchronize()
    ops.check_workspaces()
    print(f"{args.form}: {args.steps} steps, {H} / {Hkv} heads x {N} rows, flagged {int(need.sum().item())} of {H}; unique plane bytes "
          f"of the MSB pass {Hkv * N * 264} per step")


if __name__ == "__main__":
    main()
