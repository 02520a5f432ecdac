"""The device-length decode step (a) with ONE shared state — the form every captured decode graph uses; timed on this tree and on
the parent's to show that the per-sequence stride (spatten_decode_args_t::step_state_sb = 0 here) costs it nothing — and (b) with one
state per sequence on a ragged batch against the same batch padded to the bound with a -inf mask on the general kernel.

Method (gqa_bench.py's): graphs of 20 steps rotating over enough layer planes to defeat the Infinity Cache, median and min .. max of
7 timings per route; the routes of (b) alternate in one process on the same planes.  (a) is one route: alternate PROCESSES of the two
trees — SPATTEN_TREE names the tree whose spatten_amd package is imported (default: this one); it uses nothing the parent lacks.
usage: ragged_step_bench.py shared | ragged"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("SPATTEN_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from spatten_amd import ops

d, tdt, STEPS, RUNS = 128, torch.bfloat16, 20, 7
MODE0 = ops.set_decode_gqa(-1)              # the mode the process started with: restored at the end


def setup(B, H, Hkv, bound):
    plane = B * Hkv * bound * d * 2
    L = max(4, int(600e6 // (2 * plane)) + 1)
    cos, sin = ops.rope_table(bound + 8, d, tdt, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    planes = []
    for l in range(L):
        kr, v = rnd(B, Hkv, bound, d), rnd(B, Hkv, bound, d)
        planes.append((torch.zeros_like(kr), kr, v))
    t = dict(q=rnd(B, H, d), kn=rnd(B, Hkv, d), vn=rnd(B, Hkv, d), out=torch.zeros(B, H * d, dtype=tdt, device="cuda"),
             st=torch.zeros(B, H, bound, dtype=tdt, device="cuda"), lse=torch.zeros(B, H, 2, device="cuda"),
             ws=ops.DecodeWorkspace(B, H, d, "cuda"))
    return cos, sin, planes, t


def time_routes(routes, label):
    """routes: name -> function issuing STEPS launches.  Captured once each, then RUNS alternating timings of 5 replays."""
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


def shared(H, Hkv, bound, length, mode, want_form):
    """(a): B = 1, the shared state at `length` under `bound`."""
    cos, sin, planes, t = setup(1, H, Hkv, bound)
    step = ops.StepState(cos, sin)
    step.set(length, length - 1)
    ops.set_decode_gqa(mode)

    def steps():
        for i in range(STEPS):
            kc, krc, vc = planes[i % len(planes)]
            args = (t["q"], kc, krc, vc, bound, cos, sin, 0)
            kw = dict(k_new=t["kn"], v_new=t["vn"], scores=t["st"], lse=t["lse"], out=t["out"], workspace=t["ws"], step=step)
            if i == 0:
                assert ops.decode_gqa_form(*args, **kw) == want_form
            ops.attn_decode(*args, **kw)

    time_routes({"shared state": steps}, f"H={H} Hkv={Hkv} bound={bound} length={length} B=1 planes={len(planes)}")
    t["ws"].check()


def ragged(H, Hkv, lens, bound):
    """(b): one state per sequence against the padded batch with a -inf mask (the general per-query-head kernel)."""
    B = len(lens)
    cos, sin, planes, t = setup(B, H, Hkv, bound)
    step = ops.StepState(cos, sin, batch=B)
    step.set(list(lens), [n - 1 for n in lens])
    mask = torch.zeros(B, bound, dtype=tdt, device="cuda")
    for b, n in enumerate(lens):
        mask[b, n:] = float("-inf")
    kw0 = dict(k_new=t["kn"], v_new=t["vn"], scores=t["st"], lse=t["lse"], out=t["out"], workspace=t["ws"])
    forms = {}

    def make(name, **kw):
        def steps():
            for i in range(STEPS):
                kc, krc, vc = planes[i % len(planes)]
                args = (t["q"], kc, krc, vc, bound, cos, sin, bound - 1)
                if i == 0:
                    forms[name] = ops.decode_gqa_form(*args, **kw0, **kw)
                ops.attn_decode(*args, **kw0, **kw)
        return steps

    ops.set_decode_gqa(-1)
    med = time_routes({"padded + mask": make("padded + mask", mask=mask), "ragged (state per sequence)": make("ragged (state per sequence)", step=step)},
                      f"H={H} Hkv={Hkv} bound={bound} lengths={lens} planes={len(planes)}")
    print(f"    grouped form: {forms}   ragged / padded = {med['ragged (state per sequence)'] / med['padded + mask']:.3f}", flush=True)
    t["ws"].check()


what = sys.argv[1] if len(sys.argv) > 1 else "shared"
if what == "shared":
    shared(32, 32, 2304, 2080, -1, False)
    shared(32, 8, 16384 + 64, 16384, -1, True)
else:
    ragged(32, 32, (4096, 2048, 1024, 512), 4096)
    ragged(32, 8, (4096, 2048, 1024, 512), 4096)
ops.set_decode_gqa(MODE0)
