"""Grouped-query decode step WITH a head list and head importance (head pruning): (a) the per-query-head step over the list, (b) the
matrix-core step with the list (grouped_heads=True), (c) the plain matrix-core step of the same shape — alternating in one process on
the same planes (gqa_bench.py's method): graphs of 20 steps rotating over enough layer planes to defeat the Infinity Cache, median
and min .. max of 7 timings per route.  24 of 32 heads alive, once spread over all groups (every group keeps 3 of 4) and once with
two groups empty, at 4096 and 16384 rows.
usage: gqa_heads_bench.py [H Hkv [B]]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from spatten_amd import ops

argv = sys.argv[1:]
H, Hkv = (int(x) for x in (argv[:2] if len(argv) >= 2 else (32, 8)))
B = int(argv[2]) if len(argv) > 2 else 1
d, tdt, STEPS, RUNS = 128, torch.bfloat16, 20, 7
G = H // Hkv
MODE0 = ops.set_decode_gqa(-1)              # the mode the process started with: restored at the end
LISTS = {"spread": [h for h in range(H) if h % G != G - 1],                 # every group loses its last head
         "two groups empty": [h for h in range(H) if h // G < Hkv - 2]}     # the last two groups lose every head


def bench(N, list_name):
    ids = torch.tensor(LISTS[list_name], dtype=torch.int32, device="cuda")
    cap = (N + 64 + 7) // 8 * 8
    plane = B * Hkv * cap * d * 2
    L = max(4, int(600e6 // (2 * plane)) + 1)
    cos, sin = ops.rope_table(cap + 8, d, tdt, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    planes = []
    for l in range(L):
        kr, v = rnd(B, Hkv, cap, d), rnd(B, Hkv, cap, d)
        planes.append((torch.zeros_like(kr), kr, v))
    q, kn, vn = rnd(B, H, d), rnd(B, Hkv, d), rnd(B, Hkv, d)
    out = torch.zeros(B, H * d, dtype=tdt, device="cuda")
    st = torch.zeros(B, H, cap, dtype=tdt, device="cuda")
    lse = torch.zeros(B, H, 2, device="cuda")
    habs = torch.zeros(B * H, device="cuda")
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    routes = {"a per-head list": (0, True), "b grouped list": (1, True), "c plain grouped": (1, False)}
    graphs = {}
    for name, (mode, lst) in routes.items():
        ops.set_decode_gqa(mode)

        def steps():
            for i in range(STEPS):
                kc, krc, vc = planes[i % L]
                args = (q, kc, krc, vc, N, cos, sin, N - 1)
                kw = dict(k_new=kn, v_new=vn, scores=st, lse=lse, out=out, workspace=ws)
                if lst:
                    kw.update(head_ids=ids, head_abs=habs, grouped_heads=bool(mode))
                if i == 0:
                    assert ops.decode_gqa_form(*args, **kw) == bool(mode), name
                ops.attn_decode(*args, **kw)

        steps()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            steps()
        graphs[name] = gr
    times = {n: [] for n in graphs}
    for n, gr in graphs.items():
        for _ in range(3):
            gr.replay()
    torch.cuda.synchronize()
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
        print(f"H={H} Hkv={Hkv} N={N} B={B} alive={ids.numel()} ({list_name}) planes={L} route {n}: median {statistics.median(t):7.2f} us/step  ({min(t):.2f} .. {max(t):.2f} of {RUNS})", flush=True)
    ws.check()

for n_rows in (4096, 16384):
    for name in LISTS:
        bench(n_rows, name)
ops.set_decode_gqa(MODE0)
