"""(a) The ragged prune event (spatten_prune_ragged: every sequence at its own device length, one event) against what a caller does
without it: one spatten_prune_layers_scored event per sequence on that sequence's slice, driven by host integers — with the
read-back of the lengths, and any copy of the sequences that are NOT pruned, left out in the baseline's favour (the ragged event
copies those and zero-fills the defined region).  Llama-2-7B geometry: 32 layers, 32 heads, d = 128, bf16, B = 4, lengths
4096 / 2048 / 1024 / 512, start 4 / recent 1020 / k 1020, one token coming: the two longest sequences prune.
(b) The shared-state cascade step (importance_acc with acc_sb = 0), timed on this tree and on the parent's: what the run-time field
costs the accumulation kernels that do not use it.  Alternate PROCESSES of the two trees — SPATTEN_TREE names the tree whose
spatten_amd package is imported (default: this one); (b) uses nothing the parent lacks.

Method (ragged_step_bench.py's): median and min .. max of 7 timings per route, routes alternating.
usage: ragged_prune_bench.py prune | step"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("SPATTEN_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from spatten_amd import ops

d, tdt, RUNS = 128, torch.bfloat16, 7


def timed(routes, label, reps, unit):
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in routes}
    for _ in range(RUNS):
        for n, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    for n, t in times.items():
        print(f"{label} route {n}: median {statistics.median(t):9.2f} us/{unit}  ({min(t):.2f} .. {max(t):.2f} of {RUNS})", flush=True)
    return {n: statistics.median(t) for n, t in times.items()}


def prune(layers=32, H=32, lens=(4096, 2048, 1024, 512), start=4, recent=1020, k=1020, nc=1):
    B, bound = len(lens), max(lens)
    keep = start + k + recent - nc
    cap = (keep + 1 + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g)
    cos, sin = ops.rope_table(cap + 8, d, tdt, "cuda")
    Ks = [rnd(B, H, bound, d).to(tdt) for _ in range(layers)]
    Vs = [rnd(B, H, bound, d).to(tdt) for _ in range(layers)]
    accs = [rnd(B, H, bound).abs() for _ in range(layers)]
    mk = lambda: [torch.zeros(B, H, cap, d, dtype=tdt, device="cuda") for _ in range(layers)]
    Kd, Vd, Krd = mk(), mk(), mk()
    acc_d = [torch.zeros(B, H, cap, device="cuda") for _ in range(layers)]
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    idx = torch.zeros(layers, B, H, k, dtype=torch.int32, device="cuda")
    new_lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    plan = ops.PrunePlan(accs, Ks, Vs, Kd, Vd, Krd, accs, acc_d)

    def ragged():
        ops.prune_ragged(accs, Ks, Vs, lens_d, bound, start, recent, k, nc, cap, (cos, sin), acc=accs, dst=(Kd, Vd, Krd), idx=idx,
                         new_lens=new_lens, acc_dst=acc_d, plan=plan)

    pruned = [b for b, n in enumerate(lens) if n + nc > start + k + recent]
    per_seq = []
    for b in pruned:
        sl = slice(b, b + 1)
        a = dict(scores=[x[b] for x in accs], Ks=[x[sl] for x in Ks], Vs=[x[sl] for x in Vs], dst=([x[sl] for x in Kd], [x[sl] for x in Vd],
                 [x[sl] for x in Krd]), acc=([x[b] for x in accs], [x[b] for x in acc_d]), idx=torch.zeros(layers, H, k, dtype=torch.int32, device="cuda"))
        a["plan"] = ops.PrunePlan(a["scores"], a["Ks"], a["Vs"], *a["dst"], *a["acc"])
        per_seq.append((lens[b], a))

    def slices():
        for n, a in per_seq:
            ops.prune_layers(a["scores"], a["Ks"], a["Vs"], n, start, n - recent + nc, k, capacity=cap, dst=a["dst"], plan=a["plan"],
                             idx=a["idx"], rope=(cos, sin), acc=a["acc"])

    ragged(); slices()
    torch.cuda.synchronize()
    assert new_lens.tolist() == [keep if b in pruned else n for b, n in enumerate(lens)]
    for (n, a), b in zip(per_seq, pruned):
        assert torch.equal(idx[:, b], a["idx"])
    med = timed({f"{len(pruned)} single-sequence events (pruned sequences only)": slices, "one ragged event (all sequences)": ragged},
                f"layers={layers} H={H} lengths={lens} start/recent/k={start}/{recent}/{k}", 3, "event")
    vals = list(med.values())
    print(f"    ragged / per-sequence = {vals[1] / vals[0]:.3f}", flush=True)


def step(H, Hkv, bound, length, mode, want_form, STEPS=20):
    """the shared-state cascade step at `length` under `bound`, B = 1, acc [H, bound] (acc_sb = 0)"""
    plane = Hkv * bound * d * 2
    L = max(4, int(600e6 // (2 * plane)) + 1)
    cos, sin = ops.rope_table(bound + 8, d, tdt, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    planes = [(torch.zeros(1, Hkv, bound, d, dtype=tdt, device="cuda"), rnd(1, Hkv, bound, d), rnd(1, Hkv, bound, d)) for _ in range(L)]
    q, kn, vn = rnd(1, H, d), rnd(1, Hkv, d), rnd(1, Hkv, d)
    out = torch.zeros(1, H * d, dtype=tdt, device="cuda")
    st = [torch.zeros(1, H, bound, dtype=tdt, device="cuda") for _ in range(2)]
    lse = [torch.ones(1, H, 2, device="cuda") for _ in range(2)]
    acc = torch.zeros(H, bound, device="cuda")
    ws = ops.DecodeWorkspace(1, H, d, "cuda")
    state = ops.StepState(cos, sin)
    state.set(length, length - 1)
    state.advance(0)
    state.advance(0)                            # word 3 = length: every step folds `length` rows of the other buffer
    prev = ops.set_decode_gqa(mode)

    def steps():
        for i in range(STEPS):
            kc, krc, vc = planes[i % L]
            args = (q, kc, krc, vc, bound, cos, sin, 0)
            kw = dict(k_new=kn, v_new=vn, scores=st[0], lse=lse[0], out=out, workspace=ws, step=state, cascade=(acc, st[1], lse[1], 0))
            if i == 0:
                assert ops.decode_gqa_form(*args, **kw) == want_form
            ops.attn_decode(*args, **kw)

    steps()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        steps()
    timed({"shared-state cascade step": lambda: gr.replay()}, f"H={H} Hkv={Hkv} bound={bound} length={length} B=1 planes={L}", 5 , f"{STEPS} steps")
    ws.check()
    ops.set_decode_gqa(prev)


what = sys.argv[1] if len(sys.argv) > 1 else "prune"
if what == "prune":
    prune()
else:
    step(32, 32, 2304, 2080, 0, False)
    step(32, 8, 16384 + 64, 16384, 1, True)
