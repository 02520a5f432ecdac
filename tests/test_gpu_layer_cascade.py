"""The layer-cascade prune event (spatten_prune_layer_cascade; ops.prune_layer_cascade / ops.LayerCascadePlan;
SpAttenKVCache._prune_layer_cascade) against the oracle on every path of its dispatch.  Needs an MI355X.

Every comparison is equality of bits: tests/layer_cascade_cases.py holds the cases, the oracle-side reference and the checker;
tests/test_layer_cascade_cpu.py shows that the checker is sharp and that no case passes vacuously.  Paths are reached by
geometry, the way a user reaches them; every case prints what the host's rule selects for it (lc.dispatch, computed from the
same constants as prune_layer_cascade_impl), and the first test asserts it for the cases that stand for a path:

  select kernel   layer_cascade_select_blocked_kernel: every window <= 4096 and a map exists
                  layer_cascade_select_kernel (chain_body): keys in LDS for windows <= 15360, in the global scratch beyond
  membership      stamp map for ids in [map_base, map_base + map_ids), binary search of the previous id row for the others
                  (the spread / clusters families; ids below a later leg's map_base), search only when there is no map
                  (255 layers or more)
  legs            min(max(4, ceil(layers / 48)), layers) at the default setting
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import layer_cascade_cases as lc
from tests.util import dev, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAT = lc.catalogue()


def test_the_geometries_select_every_path():
    """(restated on the GPU side so that a run of this file alone shows which kernels its cases reach)"""
    d = {n: lc.dispatch(CAT[n]()) for n in ("llama7b", "win4096", "chain_lds_4097", "chain_lds_15360", "chain_scratch_15361",
                                            "chain_scratch_20000", "layers254", "layers255", "layers97")}
    for n, v in d.items():
        print(f"{n}: {v['select']}, keys in {v['keys']}, map of {v['map_ids']} ids, {v['legs']} legs over {v['bounds'][0]} ...")
    assert d["llama7b"]["select"] == d["win4096"]["select"] == d["layers254"]["select"] == "layer_cascade_select_blocked_kernel"
    assert d["chain_lds_4097"]["keys"] == d["chain_lds_15360"]["keys"] == ["lds"]
    assert d["chain_scratch_15361"]["keys"] == d["chain_scratch_20000"]["keys"] == ["lds", "scratch"]
    assert d["layers255"]["map_ids"] == 0 and d["layers255"]["select"] == "layer_cascade_select_kernel" and d["layers255"]["legs"] == 6


@pytest.mark.parametrize("name", list(CAT))
def test_event_equals_the_oracle(name):
    """positions, ids, K / V rows, the rotated shadow and the accumulators of one event, bit for bit; events of up to eight
    layers go through ops.LayerCascadePlan with caller-supplied, sentinel-filled destinations (rows beyond new_len untouched)"""
    case = CAT[name]()
    dsp = lc.dispatch(case)
    print(f"{name}: {dsp['select']}, keys {dsp['keys']}, map_ids {dsp['map_ids']}, legs {dsp['legs']}, max window {dsp['max_w']}")
    lc.run_and_check(case, use_dst=case.rows == "numpy" and case.nl <= 8)


@pytest.mark.parametrize("sdt", ["bf16", "f16", "f32"])
def test_three_successive_events_of_one_conversation(sdt):
    """the protocol: each event is fed the DEVICE's new ids of the event before as known ids, plus appended rows under a risen
    id_base, accumulators and rows carried along — the case where a token kept by layer l-2, dropped by layer l-1 and still
    held by layer l meets the never-cleared stamp map"""
    lc.run_protocol_on_device(lc.protocol_cases(sdt=sdt))


def test_protocol_at_windows_beyond_the_blocked_select():
    lc.run_protocol_on_device(lc.build_protocol("protocol_chain", 33, 3, 2, 9000, 24, [3000, 2600, 2200], 2500, d=16, sdt="bf16"))


# ---- the forms chosen by environment: read once per process by the library, so each runs in a fresh child process
@pytest.mark.parametrize("env", [{"SPATTEN_LC_LEGS": "1"}, {"SPATTEN_LC_LEGS": "2"}, {"SPATTEN_LC_BLOCKED": "0"}],
                         ids=["serial", "two_legs", "chain_body_at_small_windows"])
def test_forms_chosen_by_environment(env):
    r = subprocess.run([sys.executable, "-m", "tests.layer_cascade_cases", "--run", "blocked_small"], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True, text=True, timeout=600)
    if r.returncode < 0 or r.returncode in (134, 139):        # the child died of a signal: nothing more is started on this GPU
        pytest.exit(f"layer-cascade child process died ({r.returncode}) under {env}:\n" + r.stdout[-2000:] + r.stderr[-3000:], returncode=3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"all {len(lc.RUNNER_FAMILIES['blocked_small'])} cases pass" in r.stdout, r.stdout[-2000:]


# ---- refusals: each raises before anything is written
def _refusal_setup():
    from spatten_amd import ops
    case = CAT["ragged_bf16_bf16"]()
    tdt = torch.bfloat16
    K, V = case.kv()
    Ks, Vs = [dev(x, "bf16") for x in K], [dev(x, "bf16") for x in V]
    scores = [dev(s, "bf16") for s in case.scores]
    known = [torch.from_numpy(k).cuda() for k in case.known]
    caps = [max(case.new_lens) + 8] * case.nl
    mk = lambda: [torch.full((case.B, case.H, caps[l], case.d), 0x7B7B, dtype=torch.int16, device="cuda").view(tdt) for l in range(case.nl)]
    dst = (mk(), mk(), mk())
    c, s = orc.rope_table(max(caps), case.d, "bf16")
    rope = (dev(c[:, :case.d // 2], "bf16"), dev(s[:, :case.d // 2], "bf16"))
    return ops, case, scores, known, Ks, Vs, caps, rope, dst


def _untouched(dst):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.int16) == 0x7B7B).all()) for plane in dst for t in plane)


def test_refusals_leave_the_destinations_untouched():
    ops, case, scores, known, Ks, Vs, caps, rope, dst = _refusal_setup()
    args = lambda **kw: dict(dict(scores=scores, known_ids=known, id_base=case.id_base, Ks=Ks, Vs=Vs, lens=case.lens, his=case.his,
                                  keeps=case.keeps, start=case.start, capacities=caps, rope=rope, dst=dst), **kw)
    # a window smaller than its k
    with pytest.raises(ValueError):
        ops.prune_layer_cascade(**args(his=[case.start + 10] * case.nl, lens=[case.start + 10 + case.tail] * case.nl,
                                       known_ids=[None] * case.nl))
    assert _untouched(dst)
    # keeps that grow from one layer to the next
    grow = list(case.keeps)
    grow[2] = grow[1] + 1
    with pytest.raises((ValueError, RuntimeError)):
        ops.prune_layer_cascade(**args(keeps=grow))           # (the planes have room for the grown layer: the C side refuses)
    assert _untouched(dst)
    # destination planes too small
    short = tuple([t[:, :, :case.new_lens[l] - 1] for l, t in enumerate(p)] for p in dst)
    with pytest.raises(ValueError):
        ops.prune_layer_cascade(**args(dst=short))
    assert _untouched(dst)
    # rope tables shorter than a new length
    with pytest.raises((ValueError, RuntimeError)):
        ops.prune_layer_cascade(**args(rope=(rope[0][:max(case.new_lens) - 1], rope[1][:max(case.new_lens) - 1])))
    assert _untouched(dst)
    # ... and the valid call on the same tensors still passes
    out = ops.prune_layer_cascade(**args())
    torch.cuda.synchronize()
    ref = lc.reference(case)
    for l in range(case.nl):
        assert np.array_equal(out[3][l].cpu().numpy(), ref["idx"][l]) and np.array_equal(host(out[0][l]), ref["K"][l])


# ---- the per-layer helpers the composition test is built from
@pytest.mark.parametrize("sdt", ["bf16", "f16", "f32"])
def test_cascade_rank_equals_isin(sdt):
    """ops.cascade_rank against np.isin + -inf: random rows, every / no slot a member, previous rows of 1 and 100,000 ids"""
    from spatten_amd import ops
    rng = np.random.default_rng(3)
    H = 3

    def one(ids, prev, family="special"):
        L = ids.shape[1]
        sc = lc.make_scores(rng, family, H, L, sdt)
        got = ops.cascade_rank(dev(sc, sdt), torch.from_numpy(ids).cuda(), torch.from_numpy(prev).cuda())
        torch.cuda.synchronize()
        want = np.stack([np.where(np.isin(ids[h], prev[h]), sc[h], np.float32(-np.inf)) for h in range(H)]).astype(np.float32)
        assert got.dtype == torch.float32
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert np.array_equal(np.where(np.isnan(g), 0, g).view(np.uint32), np.where(np.isnan(want), 0, want).view(np.uint32))

    def draw(pool, n):             # H ascending duplicate-free rows of n ids below ``pool``
        rows = []
        for _ in range(H):
            u = np.unique(rng.integers(0, pool, 2 * n + 16))
            rows.append(np.sort(rng.choice(u, n, replace=False)))
        return np.stack(rows).astype(np.int32)

    one(draw(5000, 1500), draw(5000, 700))
    one(draw(5000, 1), draw(5000, 700))
    ids = draw(3000, 1000)
    one(ids, ids.copy())                                              # every slot a member
    one(ids, (draw(3000, 400) + 10000).astype(np.int32))              # no slot a member
    one(draw(400000, 3000), draw(400000, 1))                          # a previous row of one id
    one(draw(400000, 257), draw(400000, 100000), "normal")            # ... and of 100,000
    one((draw(1 << 30, 2000) - (1 << 29)).astype(np.int32), (draw(1 << 30, 3000) - (1 << 29)).astype(np.int32))     # negative ids, wide spread


def test_cascade_rank_with_an_empty_previous_row_ranks_nothing():
    from spatten_amd import ops
    rng = np.random.default_rng(4)
    sc = lc.make_scores(rng, "normal", 2, 300, "bf16")
    ids = np.tile(np.arange(300, dtype=np.int32)[None], (2, 1))
    prev = torch.zeros(2, 0, dtype=torch.int32, device="cuda")
    try:
        got = ops.cascade_rank(dev(sc, "bf16"), torch.from_numpy(ids).cuda(), prev)
    except (ValueError, RuntimeError):
        return                                                        # refused: also a defined answer
    torch.cuda.synchronize()
    assert bool(torch.isneginf(got).all())


def test_gather_rows_i32_and_importance_compact_equal_numpy_indexing():
    from spatten_amd import ops
    rng = np.random.default_rng(5)
    H, L, start, hi, k = 5, 1300, 4, 1200, 500
    idx = np.stack([np.sort(rng.choice(np.arange(start, hi), k, replace=False)) for _ in range(H)]).astype(np.int32)
    ids = rng.integers(-2 ** 31, 2 ** 31 - 1, (H, L + 7)).astype(np.int32)
    acc = rng.random((H, L + 7), dtype=np.float32)
    acc[0, :40] = np.array([np.nan, np.inf, -np.inf, -0.0] * 10, dtype=np.float32)
    want = lambda a: np.stack([np.concatenate([a[h, :start], a[h, idx[h]], a[h, hi:L]]) for h in range(H)])
    di = torch.from_numpy(idx).cuda()
    got = ops.gather_rows_i32(torch.from_numpy(ids).cuda()[:, :L], di, start, hi, L)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want(ids))
    n = start + k + L - hi
    for cap in (None, n, n + 300, 4 * L):                             # destinations as wide as the result, and wider than the source
        got = ops.importance_compact(torch.from_numpy(acc).cuda(), di, start, hi, L, cap)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        assert g.shape[1] == max(cap or n, n)
        assert np.array_equal(g[:, :n].view(np.uint32), want(acc).view(np.uint32)) and not g[:, n:].view(np.uint32).any()
    # no tail, start = 0
    idx0 = np.stack([np.sort(rng.choice(L, 100, replace=False)) for _ in range(H)]).astype(np.int32)
    got = ops.gather_rows_i32(torch.from_numpy(ids).cuda()[:, :L], torch.from_numpy(idx0).cuda(), 0, L, L)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), np.stack([ids[h, idx0[h]] for h in range(H)]))


# ---- through the plugin
@pytest.mark.parametrize("mode,H,Hkv", [("reference", 4, 4), ("cascade", 4, 4), ("reference", 4, 2)],
                         ids=["reference", "cascade_accumulators", "grouped_query"])
def test_plugin_layer_cascade_at_windows_that_reach_chain_body(mode, H, Hkv, capsys):
    """SpAttenKVCache with layer_keep on eight layers of bf16 K / V, windows near 5,000 (beyond the blocked select), two prune
    events with rows and scores written directly between them: keep_indices, ext.tok_ids, new K / V and the slab's rotated
    shadow against the oracle — in reference importance mode, with importance_mode="cascade" accumulators, and on a
    grouped-query cache (a key's importance = its group's summed score)."""
    from spatten_amd import kv_slab
    from spatten_amd.extensions import SpattenExtensions
    from spatten_amd.kv_cache_token_pruning import SpAttenKVCache
    B, d, layers, start, recent, coming, appended = 1, 64, 8, 4, 128, 16, 3000
    keeps = [2000 - 100 * l for l in range(layers)]
    G = H // Hkv
    cache = SpAttenKVCache(start_size=start, recent_size=recent, important_size=keeps[0], importance_mode=mode)
    cache.ext = SpattenExtensions(cache, layers, cascade=(mode == "cascade"), layer_keep=keeps)
    rng = np.random.default_rng(41)
    rnd = lambda *shape: orc.round_dt(rng.standard_normal(shape, dtype=np.float32), "bf16")
    Kr = [rnd(B, Hkv, 5200, d) for _ in range(layers)]
    Vr = [rnd(B, Hkv, 5200, d) for _ in range(layers)]
    ids_r, next_id, accs = None, 0, None
    if mode == "cascade":
        accs = [rng.random((H, 5200 + 16), dtype=np.float32) for _ in range(layers)]
    for event in range(2):
        lens = [k.shape[2] for k in Kr]
        assert all(L - recent + coming - start > lc.BLOCKED_MAX for L in lens)          # chain_body, keys in LDS
        past = [[dev(Kr[l], "bf16"), dev(Vr[l], "bf16")] for l in range(layers)]
        if mode == "cascade":
            for l in range(layers):
                cache.ext.layers[l].acc = torch.from_numpy(accs[l]).cuda()
            imp = [a[:, :L] for a, L in zip(accs, lens)]
            stashes = [None] * layers
        else:
            raw = [orc.round_dt(rng.random((H, L), dtype=np.float32), "bf16") for L in lens]
            stashes = [dev(s, "bf16")[None, :, None, :] for s in raw]
            imp = [orc.round_dt(s.reshape(Hkv, G, -1).sum(1), "bf16") for s in raw]       # (G <= 2: the fp32 sum is exact)
        new = cache.apply_token_pruning(past, coming, stashes)
        torch.cuda.synchronize()
        n_new = lens[0] - (0 if ids_r is None else ids_r[0].shape[1])
        fresh = np.tile(np.arange(next_id, next_id + n_new, dtype=np.int32)[None], (Hkv, 1))
        ids_now = [fresh if ids_r is None else np.concatenate([ids_r[l], fresh], 1) for l in range(layers)]
        next_id += n_new
        past_r, ids_r, idxs = orc.layer_cascade_prune([(Kr[l], Vr[l]) for l in range(layers)], ids_now, imp, coming, start, recent, keeps)
        for l in range(layers):
            n = start + keeps[l] + recent - coming
            assert np.array_equal(cache.keep_indices[l].cpu().numpy(), idxs[l]), (event, l)
            assert np.array_equal(cache.ext.tok_ids[l].cpu().numpy(), ids_r[l]), (event, l)
            assert new[l][0].shape[2] == n
            assert np.array_equal(host(new[l][0]), past_r[l][0]) and np.array_equal(host(new[l][1]), past_r[l][1]), (event, l)
            slab = kv_slab.slab_of(new[l][0])
            cos, sin = slab.tables(n)
            full = lambda t: np.concatenate([host(t[:n]), host(t[:n])], 1)
            want = orc.apply_rotary_pos_emb_single(past_r[l][0], full(cos), full(sin), np.arange(n)[None], "bf16")
            assert np.array_equal(host(slab.kr[:, :, :n]).view(np.uint32), want.view(np.uint32)), (event, l)
            if mode == "cascade":
                a = accs[l]
                want_acc = np.stack([np.concatenate([a[h, :start], a[h, idxs[l][h]], a[h, lens[l] - recent + coming:lens[l]]]) for h in range(H)])
                got_acc = cache.ext.layers[l].acc.cpu().numpy()
                assert np.array_equal(got_acc[:, :n].view(np.uint32), want_acc.view(np.uint32)) and not got_acc[:, n:].any(), (event, l)
                accs[l] = np.concatenate([want_acc, rng.random((H, appended + 16), dtype=np.float32)], 1)
        # rows appended since, written directly
        Kr = [np.concatenate([past_r[l][0], rnd(B, Hkv, appended, d)], 2) for l in range(layers)]
        Vr = [np.concatenate([past_r[l][1], rnd(B, Hkv, appended, d)], 2) for l in range(layers)]
