"""The composed decode step over the profiled planes (spatten_attn_decode_pq_local_v): MSB scores, LSB refetch for the flagged
heads, local V pruning over the quantised V plane, fused cascade importance.  PARITY UNPINNED: the reference is the composition
of the oracle's pieces (oracle/spatten_oracle.py: pq_quantize / pq_quantize_values -> pq_decode_attention_profile ->
local_value_prune(softmax_probs(logits), qv * vscale, keep) -> cascade_importance_accumulate; SpAttenController.scala:402,546-558,
591-612, RequantDecision.scala:44-72, TopK.scala:193-212).  Bars: need_lsb equal to the oracle's (the threshold is placed between
two heads' max probabilities); kept set exact on the kernel's own stash; out within the output tolerance; stash and need_lsb
bit-identical to attn_decode_pqv on the same inputs."""
import math

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.test_gpu_pq_profiles import _build
from tests.util import OUT_TOL, TORCH_DT, host

pytestmark = pytest.mark.gpu


def _kept_lists(B, H, d):
    """The kept-row lists the last call left in its workspace (include/spatten.h: counters | partials | kept lists)."""
    from spatten_amd import ops
    ws, rows = ops._pq_local_v_workspace(B, H, d, 1, torch.device("cuda", torch.cuda.current_device()))
    units = B * H
    off = (units * 4 + 255) // 256 * 256 + units * 64 * d * 4
    return ws[off:off + units * rows * 4].view(torch.int32).view(B, H, rows).cpu().numpy()


def _oracle(planes_host, qr, thr, H, Hkv):
    msb, lsb, scale, qv, vscale = planes_host
    rep = lambda a: orc.repeat_kv(a, H // Hkv)
    return orc.pq_decode_attention_profile(qr, rep(msb), rep(lsb), rep(scale), rep(qv), rep(vscale), thr)


def _split_threshold(planes_host, qr, d):
    """A threshold between two heads' pass-1 max probabilities (the widest gap near the middle): need_lsb is then decided."""
    msb, _, scale, _, _ = planes_host
    p1max = np.sort(orc.softmax_probs(np.einsum("bhd,bhld->bhl", qr.astype(np.float32), orc.pq_dequant(msb, None, scale))
                                      / np.float32(np.sqrt(d))).max(-1).ravel())
    n = p1max.size
    lo, hi = max(0, n // 4 - 1), min(n - 1, 3 * n // 4)
    i = lo + int(np.argmax(np.diff(p1max[lo:hi + 1])))
    return float((p1max[i] + p1max[i + 1]) / 2)


def _check_kept(kept, stash, n, k, units):
    for b, h in units:
        want = orc.topk_window(stash[b, h:h + 1, :n].astype(np.float32), 0, n, k)[0]
        assert np.array_equal(np.sort(kept[b, h, :k]), want), (b, h)


CASES = [  # (kb, vb), dt, d, B, H, P, keep, head list
    ((8, 8), "bf16", 128, 1, 40, 8191, 0.3, False),
    ((8, 8), "bf16", 128, 2, 8, 700, 0.1, True),
    ((4, 8), "f16", 64, 2, 12, 40, 1.0, False),
    ((4, 8), "bf16", 128, 1, 16, 2999, 0.3, True),
    ((6, 6), "f32", 128, 1, 8, 1500, 0.1, False),
    ((6, 6), "bf16", 64, 2, 6, 300, 0.3, True),
    ((8, 8), "f32", 64, 1, 4, 16383, 0.1, False),
    ((6, 6), "f16", 128, 1, 32, 4095, 1.0, True),
]


@pytest.mark.parametrize("prof,dt,d,B,H,P,keep_f,use_heads", CASES)
def test_pq_local_v_vs_composed_oracle(prof, dt, d, B, H, P, keep_f, use_heads):
    from spatten_amd import ops
    kb, vb = prof
    planes, ph, qr, qd, krd, vd, cos, sin, N = _build(B, H, H, d, P, dt, 61 + H, kb, vb)
    thr = _split_threshold(ph, qr, d)
    want_full, need, logits = _oracle(ph, qr, thr, H, H)
    keep = max(1, min(N, math.ceil(keep_f * N)))
    heads = list(range(0, H, 2)) if use_heads else list(range(H))
    hid = torch.tensor(heads, dtype=torch.int32, device="cuda") if use_heads else None
    need_dev = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
    scores = torch.zeros(B, H, N + 9, dtype=TORCH_DT[dt], device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    out = torch.zeros(B, H * d, dtype=TORCH_DT[dt], device="cuda")
    ops.attn_decode_pq_local_v(qd, planes, N, cos, sin, N - 1, thr, keep, scores, lse, out=out, need_lsb=need_dev, head_ids=hid)
    torch.cuda.synchronize()
    units = [(b, h) for b in range(B) for h in heads]
    got_need = need_dev.cpu().numpy().reshape(B, H)
    for b, h in units:
        assert bool(got_need[b, h]) == bool(need[b, h]), (b, h)
    st = host(scores)
    kept = _kept_lists(B, H, d)
    _check_kept(kept, st, N, keep, units)
    # out: the oracle probabilities of the final logits over the kernel's kept rows, V = qv * vscale
    msb, lsb, scale, qv, vscale = ph
    V = qv.astype(np.float32) * vscale
    probs = orc.softmax_probs(logits)
    o = host(out).reshape(B, H, d)
    for b, h in units:
        idx = np.sort(kept[b, h, :keep])
        ref = probs[b, h, idx] @ V[b, h, idx]
        np.testing.assert_allclose(o[b, h], orc.round_dt(ref, dt), err_msg=f"{(b, h)}", **OUT_TOL[dt])
        if keep == N:
            np.testing.assert_allclose(o[b, h], orc.round_dt(want_full[b, h], dt), **OUT_TOL[dt])
    if use_heads:     # pruned heads: nothing written
        pruned = [h for h in range(H) if h not in heads]
        assert not o[:, pruned].any() and not st[:, pruned].any() and (got_need[:, pruned] == -1).all()


@pytest.mark.parametrize("prof,dt,d", [((8, 8), "bf16", 128), ((4, 8), "f16", 64), ((6, 6), "f32", 128)])
def test_pq_local_v_matches_pqv(prof, dt, d):
    """Same inputs, splits and layout as attn_decode_pqv: stash and need_lsb bit-identical; at keep = n the output agrees."""
    from spatten_amd import ops
    kb, vb = prof
    B, H, P = 1, 16, 4500
    planes, ph, qr, qd, krd, vd, cos, sin, N = _build(B, H, H, d, P, dt, 71, kb, vb, extra=100)
    thr = _split_threshold(ph, qr, d)
    res = []
    for composed in (False, True):
        need_dev = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
        scores = torch.zeros(B, H, N + 100, dtype=TORCH_DT[dt], device="cuda")
        lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
        if composed:
            out = ops.attn_decode_pq_local_v(qd, planes, N, cos, sin, N - 1, thr, N, scores, lse, need_lsb=need_dev,
                                             layout=N + 100)
        else:
            out = ops.attn_decode_pqv(qd, planes, N, cos, sin, N - 1, thr, need_lsb=need_dev, scores=scores, lse=lse,
                                      layout=N + 100)
        torch.cuda.synchronize()
        res.append((out.clone(), scores.clone(), need_dev.clone(), lse.clone()))
    (o0, s0, n0, l0), (o1, s1, n1, l1) = res
    assert torch.equal(s0, s1) and torch.equal(n0, n1) and torch.equal(l0, l1)
    assert 0 < int(n0.sum()) < B * H
    np.testing.assert_allclose(host(o1), host(o0), **OUT_TOL[dt])


def test_pq_local_v_ties_go_to_the_lowest_index():
    """A zero query: every logit ties, across every split boundary — the kept rows are 0 .. k-1."""
    from spatten_amd import ops
    dt, d, B, H, P = "bf16", 128, 1, 4, 3000
    planes, ph, qr, qd, krd, vd, cos, sin, N = _build(B, H, H, d, P, dt, 5, 8, 8)
    qz = torch.zeros_like(qd)
    scores = torch.zeros(B, H, N, dtype=TORCH_DT[dt], device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    keep = 777
    out = ops.attn_decode_pq_local_v(qz, planes, N, cos, sin, N - 1, 0.5, keep, scores, lse)
    torch.cuda.synchronize()
    kept = _kept_lists(B, H, d)
    for h in range(H):
        assert np.array_equal(kept[0, h, :keep], np.arange(keep))
    V = ph[3].astype(np.float32) * ph[4]
    ref = V[0, :, :keep].sum(1) / N
    np.testing.assert_allclose(host(out).reshape(H, d), orc.round_dt(ref, dt), **OUT_TOL[dt])


@pytest.mark.parametrize("thr", [0.0, 2.0])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_pq_local_v_cascade_accumulation(thr, dt):
    """T = 5 consecutive steps (one row more each) with the fused, deferred accumulation, then the flush: acc equals the sum of
    the oracle's softmax probabilities of the T final logit rows."""
    from spatten_amd import ops
    B, H, d, P, T = 2, 6, 64, 600, 5
    planes, ph, qr, qd, krd, vd, cos, sin, N = _build(B, H, H, d, P + T, dt, 81, 8, 8)
    c, s = orc.rope_table(N, d, dt)
    q_host = host(qd)[:, :, None]
    acc = torch.zeros(H, N + 9, dtype=torch.float32, device="cuda")
    acc_ref = np.zeros((H, N + 9), dtype=np.float64)
    scores = torch.zeros(B, H, N + 9, dtype=TORCH_DT[dt], device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    prev_lse = torch.zeros_like(lse)
    msb, lsb, scale, qv, vscale = ph
    for t in range(T):
        n = N - T + 1 + t
        qr_t = orc.apply_rotary_pos_emb_single(q_host, c, s, np.full((B, 1), n - 1), dt)[:, :, 0]
        _, _, logits = orc.pq_decode_attention_profile(qr_t, msb[:, :, :n], lsb[:, :, :n], scale[:, :, :n], qv[:, :, :n],
                                                       vscale[:, :, :n], thr)
        acc_ref[:, :n] += orc.softmax_probs(logits).sum(0)
        ops.attn_decode_pq_local_v(qd, planes, n, cos, sin, n - 1, thr, max(1, n // 3), scores, lse,
                                   cascade=(acc, prev_lse, 0 if t == 0 else n - 1))
    n = N
    ops.importance_accumulate(acc, planes.msb_logit[:, :, None, :n], lse[:, :, None, :])      # the flush
    torch.cuda.synchronize()
    np.testing.assert_allclose(acc.cpu().numpy(), acc_ref, atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize("use_heads", [False, True])
def test_pq_local_v_graph_replay_bit_identical(use_heads):
    """The device-length form captured once and replayed for 16 tokens across a capacity-laid-out slab (append inside the MSB
    pass, kept count ceil(f * length) on the device, fused accumulation by state word 3) equals the eager host-length loop bit for
    bit: stash, out, acc, need_lsb."""
    from spatten_amd import ops
    dt, d, B, H, P, T, kb, vb = "bf16", 128, 1, 8, 1200, 16, 8, 8
    cap = P + 64
    rs = np.random.default_rng(3)
    tdt = TORCH_DT[dt]
    K = torch.from_numpy(rs.standard_normal((B, H, cap, d)).astype(np.float32)).to(tdt).cuda()
    Vv = torch.from_numpy(rs.standard_normal((B, H, cap, d)).astype(np.float32)).to(tdt).cuda()
    qs = torch.from_numpy(rs.standard_normal((T, B, H, d)).astype(np.float32) * 2).to(tdt).cuda()
    c, s = orc.rope_table(cap, d, dt)
    cos = torch.from_numpy(c[:, : d // 2]).to(tdt).cuda()
    sin = torch.from_numpy(s[:, : d // 2]).to(tdt).cuda()
    hid = torch.tensor([0, 2, 3, 6], dtype=torch.int32, device="cuda") if use_heads else None
    frac, thr = 0.3, 0.02

    def fresh():
        k, v = torch.zeros_like(K), torch.zeros_like(Vv)
        k[:, :, :P], v[:, :, :P] = K[:, :, :P], Vv[:, :, :P]
        kr = torch.zeros_like(K)
        ops.build_shadow(k, kr, 0, P, cos, sin)
        pl = ops.PQProfilePlanes(B, H, H, cap, d, "cuda", key_bits=kb, value_bits=vb)
        ops.pq_pack_planes(kr, v, pl, 0, P)
        bufs = dict(scores=torch.zeros(B, H, cap, dtype=tdt, device="cuda"), lse=torch.zeros(B, H, 2, device="cuda"),
                    prev=torch.zeros(B, H, 2, device="cuda"), acc=torch.zeros(H, cap, device="cuda"),
                    out=torch.zeros(B, H * d, dtype=tdt, device="cuda"),
                    need=torch.zeros(B * H, dtype=torch.int32, device="cuda"))
        return k, v, kr, pl, bufs

    def record(bf, rows):
        return (bf["scores"].clone(), bf["out"].clone(), bf["acc"].clone(), bf["need"].clone(), rows)

    # eager, host lengths
    k, v, kr, pl, bf = fresh()
    eager = []
    for t in range(T):
        n = P + 1 + t
        if hid is not None:
            ops.kv_append_planes(K[:, :, n - 1], Vv[:, :, n - 1], k, kr, v, pl, n - 1, cos, sin)
            app = None
        else:
            app = (K[:, :, n - 1], Vv[:, :, n - 1], k, kr, v)
        ops.attn_decode_pq_local_v(qs[t], pl, n, cos, sin, n - 1, thr, max(1, min(n, math.ceil(frac * n))), bf["scores"],
                                   bf["lse"], out=bf["out"], need_lsb=bf["need"], head_ids=hid, layout=cap, keep_fraction=frac,
                                   cascade=(bf["acc"], bf["prev"], 0 if t == 0 else n - 1), append=app)
        eager.append(record(bf, n))
    # device length, one captured step replayed
    k, v, kr, pl, bf = fresh()
    q_in = torch.zeros_like(qs[0])
    kn, vn = torch.zeros_like(K[:, :, 0]), torch.zeros_like(Vv[:, :, 0])
    st = ops.StepState(cos, sin)
    st.set(P, P - 1)

    def step():
        st.advance()
        if hid is not None:
            ops.kv_append_planes(kn, vn, k, kr, v, pl, 0, cos, sin, step=st)
            app = None
        else:
            app = (kn, vn, k, kr, v)
        ops.attn_decode_pq_local_v(q_in, pl, cap, cos, sin, 0, thr, 1, bf["scores"], bf["lse"], out=bf["out"],
                                   need_lsb=bf["need"], keep_fraction=frac, head_ids=hid,
                                   cascade=(bf["acc"], bf["prev"], 0), step=st, append=app)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        step()                      # warm-up outside the capture (the side stream's workspaces), then back to the start
        side.synchronize()
        for x in (k, v, kr):
            x[:, :, P:] = 0
        ops.pq_pack_planes(kr, v, pl, 0, P)
        for x in bf.values():
            x.zero_()
        st.set(P, P - 1)
        side.synchronize()
        pins = ops.set_ws_pins([])
        try:
            with torch.cuda.graph(g, stream=side):
                step()
        finally:
            ops.set_ws_pins(pins)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in range(T):
        n = P + 1 + t
        q_in.copy_(qs[t])
        kn.copy_(K[:, :, n - 1])
        vn.copy_(Vv[:, :, n - 1])
        g.replay()
        got = record(bf, n)
        want = eager[t]
        assert torch.equal(got[0][:, :, :n], want[0][:, :, :n]), t
        assert torch.equal(got[1], want[1]), t
        assert torch.equal(got[2], want[2]), t
        assert torch.equal(got[3], want[3]), t
    ops.check_workspaces()


@pytest.mark.parametrize("mode", ["schedule", "trace"])
def test_trace_runner_full_cascade(mode):
    """run_spatten_synthetic.py --full-cascade on the fixture, as a child process under a time limit: the plugin's multi-turn
    protocol with prune events (--schedule) and the per-layer composed step (--trace --pq) both run and print every layer."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fx = os.path.join(root, "tests", "golden", "trace_full_cascade.csv")
    if mode == "schedule":
        cmd = ["--schedule", fx, "--full-cascade", "--pq-threshold", "0.05", "--layers", "4", "--heads", "8", "--turns", "3",
               "--max-gen-len", "24", "--prompt-len", "120", "--important_size", "64", "--recent_size", "64", "--start_size", "4"]
    else:
        cmd = ["--trace", fx, "--pq", "--full-cascade", "--pq-threshold", "0.05", "--kv-len", "2048", "--heads", "8"]
    r = subprocess.run([sys.executable, os.path.join(root, "run_spatten_synthetic.py")] + cmd, capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    table = [ln for ln in lines if len(ln) >= 5 and ln[0].isdigit()]
    assert len(table) == 4, r.stdout
    if mode == "trace":
        assert all(int(ln[2]) < int(ln[1]) for ln in table)          # values fetched < keys kept: the composed step ran
    else:
        assert "pruned token this round" in r.stdout and "(8, 8)" in r.stdout
