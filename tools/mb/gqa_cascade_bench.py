"""Grouped-query decode step WITH the fused cascade accumulation: (a) the per-query-head cascade step, (b) the matrix-core cascade
step, (c) the plain matrix-core step — alternating in one process on the same planes (gqa_bench.py's method): graphs of 20 steps
rotating over enough layer planes to defeat the Infinity Cache, median and min .. max of 7 timings per route.
usage: gqa_cascade_bench.py [H Hkv N [B]] [--single]      (--single: route (c) only — the untouched instantiations)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from spatten_amd import ops

argv = [a for a in sys.argv[1:] if a != "--single"]
single = "--single" in sys.argv
H, Hkv, N = (int(x) for x in (argv[:3] if len(argv) >= 3 else (32, 8, 16384)))
B = int(argv[3]) if len(argv) > 3 else 1
d, tdt, STEPS, RUNS = 128, torch.bfloat16, 20, 7
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
prev = rnd(B, H, cap)
lse, plse = torch.zeros(B, H, 2, device="cuda"), torch.zeros(B, H, 2, device="cuda")
plse[..., 0], plse[..., 1] = 4.0, float(N)
acc = torch.zeros(H, cap, device="cuda")
ws = ops.DecodeWorkspace(B, H, d, "cuda")
routes = {"c plain grouped": (1, False)} if single else \
    {"a per-head cascade": (0, True), "b grouped cascade": (1, True), "c plain grouped": (1, False)}
graphs = {}
for name, (mode, casc) in routes.items():
    ops.set_decode_gqa(mode)

    def steps():
        for i in range(STEPS):
            kc, krc, vc = planes[i % L]
            args = (q, kc, krc, vc, N, cos, sin, N - 1)
            kw = dict(k_new=kn, v_new=vn, scores=st, lse=lse, out=out, workspace=ws, cascade=(acc, prev, plse, N - 1) if casc else None)
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
    print(f"H={H} Hkv={Hkv} N={N} B={B} planes={L} route {n}: median {statistics.median(t):7.2f} us/step  ({min(t):.2f} .. {max(t):.2f} of {RUNS})", flush=True)
ws.check()
