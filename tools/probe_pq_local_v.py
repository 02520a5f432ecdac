#!/usr/bin/env python3
"""Device time of the composed step over the quantised planes (spatten_attn_decode_pq_local_v: MSB pass + refetch pass, both
scores only, kept-row select, P.V gather over the kept rows of the quantised V plane) next to attn_decode_pqv (the profiled step
that streams the whole V plane) and the 16-bit one-launch local-V step (attn_decode_local_v).  Every variant is captured in a
HIP graph of `reps` steps and timed with HIP events around its replays: one line each.  Then one line per launch of the composed
step, from `rocprofv3 --kernel-trace --stats` over a run of the composed step alone (skipped, with a note, where rocprofv3 is not
installed).  Every GPU step is a child process under `timeout -k 10 <s>`; a failed step ends the probe with its exit status.

    python tools/probe_pq_local_v.py [--heads 40] [--rows 8192] [--profile 8 8] [--confidence trace|all]

Confidence as bench.py --pq-confidence builds it: "trace" = ~7 % of the heads flagged for the LSB refetch (a confident head's
newest key is 0.9 x its query: max probability ~ 0.6 >> the 0.05 threshold), "all" = every head flagged (threshold 2.0)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatten_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--profile", type=int, nargs=2, default=(8, 8))
    ap.add_argument("--confidence", choices=["trace", "all"], default="trace")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--child", choices=["all", "composed"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args)
    else:
        drive(args)


def _child_cmd(args, what):
    return [sys.executable, os.path.abspath(__file__), "--child", what, "--heads", str(args.heads), "--rows", str(args.rows),
            "--head-dim", str(args.head_dim), "--profile", *map(str, args.profile), "--confidence", args.confidence,
            "--reps", str(args.reps)]


def _run_step(cmd, seconds, **kw):
    """One GPU step under `timeout -k 10 <seconds>`; a failure ends the probe with the step's exit status."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, **kw)
    if r.returncode != 0:
        print(f"step failed (exit {r.returncode}): {' '.join(cmd)}", flush=True)
        sys.exit(r.returncode)
    return r


def drive(args):
    _run_step(_child_cmd(args, "all"), args.timeout)
    prof = shutil.which("rocprofv3")
    if prof is None:
        print("per launch: rocprofv3 not found — no per-launch lines")
        return
    with tempfile.TemporaryDirectory() as td:
        _run_step([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "run", "--"]
                  + _child_cmd(args, "composed"), args.timeout + 60, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            print("per launch: rocprofv3 wrote no kernel_stats.csv")
            return
        names = {"pqv_decode_kernel": None, "pqlv_select_kernel": "kept-row select", "pqlv_gather_kernel": "P.V gather"}
        with open(stats[0], newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Name"]
                kind = next((k for k in names if k in name), None)
                if kind is None or (kind == "pqv_decode_kernel" and "Lb1EEEv" not in name):   # (the scores-only instantiations)
                    continue
                label = names[kind] or ("MSB pass (scores only)" if "ELi1ELb" in name else "refetch pass (scores only)")
                print(f"  launch {label:<27}: {float(row['AverageNs']) / 1e3:8.2f} us average over {row['Calls']} calls "
                      f"(keep 0.3 and 1.0, rocprofv3)")


def measure(args):
    H, N, d = args.heads, args.rows, args.head_dim
    kb, vb = args.profile
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
    cos, sin = ops.rope_table(N + 64, d, dt, dev)
    K, V, q = rnd(1, H, N, d), rnd(1, H, N, d), rnd(1, H, d)
    thr = 0.05
    if args.confidence == "trace":
        conf = torch.rand(1, H, device=dev, generator=g) < 0.93
        K[:, :, N - 1] = torch.where(conf[:, :, None], (0.9 * q.float()).to(dt), K[:, :, N - 1])
    else:
        thr = 2.0
    Kr = ops.rope_single(K, cos, sin)
    planes = ops.PQProfilePlanes(1, H, H, N, d, dev, key_bits=kb, value_bits=vb)
    ops.pq_pack_planes(Kr, V, planes, 0, N)
    out = torch.empty(1, H * d, dtype=dt, device=dev)
    scores = torch.empty(1, H, N, dtype=dt, device=dev)
    lse = torch.empty(1, H, 2, dtype=torch.float32, device=dev)
    need = torch.zeros(H, dtype=torch.int32, device=dev)
    ws = ops.DecodeWorkspace(1, H, d, dev)

    def timed(fn):
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(args.reps):
                    fn()
            gr.replay()
            side.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(5):
                gr.replay()
            e1.record(side)
            side.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (5 * args.reps)

    pqv = lambda: ops.attn_decode_pqv(q, planes, N, cos, sin, N - 1, thr, out=out, need_lsb=need, scores=scores, lse=lse,
                                      workspace=ws)
    pqv()
    torch.cuda.synchronize()
    flagged = int(need.sum().item())
    print(f"geometry: {H} heads x {N} rows, d = {d}, profile {(kb, vb)}, confidence {args.confidence}: {flagged} of {H} heads "
          f"refetch the LSB plane")
    if args.child == "all":
        print(f"attn_decode_pqv                     : {timed(pqv):8.2f} us")
    for f in (0.3, 1.0):
        keep = max(1, min(N, -(-int(f * N * 1000) // 1000)))
        t = timed(lambda: ops.attn_decode_pq_local_v(q, planes, N, cos, sin, N - 1, thr, keep, scores, lse, out=out, need_lsb=need,
                                                     keep_fraction=f, workspace=ws))
        print(f"attn_decode_pq_local_v keep {f:.1f}       : {t:8.2f} us", flush=True)
    if args.child == "all":
        lv_scores = torch.empty(1, H, N, dtype=dt, device=dev)
        for f in (0.3, 1.0):
            keep = max(1, min(N, -(-int(f * N * 1000) // 1000)))
            t = timed(lambda: ops.attn_decode_local_v(q, Kr, V, N, cos, sin, N - 1, keep, lv_scores, out=out))
            print(f"attn_decode_local_v (16-bit) keep {f:.1f} : {t:8.2f} us")
    ops.check_workspaces()


if __name__ == "__main__":
    main()
