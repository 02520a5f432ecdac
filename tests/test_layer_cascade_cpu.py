"""The layer-cascade checker is sharp (no GPU needed): on every case of tests/layer_cascade_cases.py the oracle and a second,
deliberately dumb statement of the selection rule agree; a numpy emulation of the event as the kernels structure it passes
the checker; eleven seeded faults each fail it on a named case; and the conditions that keep the GPU cases from passing
vacuously hold (fill rule on both sides of k, ties at the threshold in every head, ids no map can hold, previous-leg ids
below a leg's map_base, a token kept by layer l-2, dropped by layer l-1 and still held by layer l)."""
import functools

import numpy as np
import pytest

from oracle import spatten_oracle as orc
from tests import layer_cascade_cases as lc

CAT = lc.catalogue()
# the dumb reference is a Python sort per (layer, head): the big geometries are compared with it on a few layers' worth only
DUMB_SKIP = {"llama7b"}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CAT[name]()


@functools.lru_cache(maxsize=None)
def _protocol():
    return tuple(lc.protocol_cases())


@pytest.mark.parametrize("name", list(CAT) + ["protocol"])
def test_the_oracle_and_the_dumb_statement_of_the_rule_agree(name):
    """H1 (lowest position at ties) and the fill rule (lowest-position non-candidates) are pinned by two statements that share
    no selection code: orc.layer_cascade_prune (-inf + orc.topk_window) and lc.select_dumb (a plain sort)."""
    cases = _protocol() if name == "protocol" else [_case(name)]
    for c in cases:
        ref = lc.reference(c, rows=False)
        if name in DUMB_SKIP:          # 32 x 32 x 4096: the first three layers of four heads
            c = lc.Case(c.name, 1, 4, c.d, c.start, c.sdt, c.kdt, c.lens[:3], c.tail, c.keeps[:3], c.id_base,
                        [k[:4] for k in c.known[:3]], [s[:4] for s in c.scores[:3]], None, c.kv_seed, "device")
            ref = dict(idx=[x[:4] for x in ref["idx"][:3]], new_ids=[x[:4] for x in ref["new_ids"][:3]])
        idxs, nids = lc.reference_dumb(c)
        for l in range(c.nl):
            assert np.array_equal(idxs[l], ref["idx"][l]), (c.name, l)
            assert np.array_equal(nids[l], ref["new_ids"][l]), (c.name, l)


@pytest.mark.parametrize("name", list(CAT) + ["protocol"])
def test_the_emulation_of_the_event_passes_the_checker(name):
    """stamp map + fallback search, legs, masked keys, threshold + first-need_eq compaction, head / kept / tail rows, the
    gathers and the shadow at the NEW position, written into sentinel-filled planes: equal to the oracle on every case."""
    for c in (_protocol() if name == "protocol" else [_case(name)]):
        outputs, planes, _ = lc.emulate(c)
        lc.check_event(c, outputs, lc.reference(c), planes)
        if c.nl >= 3 and c.nl <= 8:    # the forms chosen by environment give the same results
            for legs, blk in ((1, 1), (2, 1), (4, 0)):
                o2, p2, _ = lc.emulate(c, legs_env=legs, blocked_env=blk)
                lc.check_event(c, o2, lc.reference(c), p2)


# fault -> (what it is, cases on which the checker must fail, whether the per-layer composition check of
# tests/test_gpu_cascade.py could see it: it cannot see a fault in a rule BOTH of its sides share — cascade_rank's reading of
# "member" over the whole previous id row, the numbering of fresh ids, "every non-member ranks as -inf")
FAULTS = {
    1: ("membership ignores the previous layer's head and tail rows", ["ragged_bf16_bf16", "heads40"], False),
    2: ("membership means kept by ANY earlier layer (stale stamps)", ["protocol"], True),
    3: ("fresh slot ids off by one", ["known_none", "ragged_bf16_bf16"], False),
    4: ("ties at the threshold keep the highest positions", ["few_bf16", "equal_f32", "lowbits_f16"], True),
    5: ("non-members ranked by their own score (fill rule)", ["ragged_f32_f32", "special_bf16", "layers255"], False),
    6: ("f16 keys cut to two radix digits, fp32 keys to three", ["lowbits_f16", "lowbits_f32", "chain_lds_15360"], True),
    7: ("NaN ranked lowest", ["special_bf16", "special_f16", "special_f32"], True),
    8: ("tail starts at hi + 1", ["ragged_bf16_bf16", "long_tail"], True),
    9: ("shadow rotated with the row's old position", ["ragged_bf16_bf16", "d80_bf16"], True),
    10: ("accumulator gathered with a window-relative position", ["ragged_bf16_bf16", "known_none"], True),
    11: ("batch row 1 gathered from batch row 0's source plane", ["ragged_bf16_bf16", "batch3"], True),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_seeded_fault_fails_the_checker(fault):
    what, names, composition_sees = FAULTS[fault]
    for name in names:
        cases = _protocol() if name == "protocol" else [_case(name)]
        caught = []
        for c in cases:
            outputs, planes, _ = lc.emulate(c, faults=(fault,))
            try:
                lc.check_event(c, outputs, lc.reference(c), planes)
            except AssertionError as e:
                caught.append(str(e)[:120])
        assert caught, f"fault {fault} ({what}) passes the checker on {name}"
    print(f"fault {fault}: {what}: caught on {names}; visible to the per-layer composition check: {'yes' if composition_sees else 'no (shared rule)'}")


def test_faults_invisible_to_the_composition_check_are_the_shared_rule_ones():
    assert sorted(f for f, v in FAULTS.items() if not v[2]) == [1, 3, 5]


# ---- conditions on the cases: no GPU case passes vacuously
@functools.lru_cache(maxsize=None)
def _stats(name):
    return lc.emulate(_case(name))[2]


@pytest.mark.parametrize("name", [n for n in CAT if "fill" in _case(n).claims])
def test_fill_families_have_windows_with_fewer_and_with_more_candidates_than_k(name):
    c, st = _case(name), _stats(name)
    pairs = [(st["members"][l][h], c.keeps[l]) for l in range(1, c.nl) for h in range(c.H)]
    assert any(m < k for m, k in pairs), f"{name}: no (layer, head) behind the first with fewer candidates than k"
    assert any(m > k for m, k in pairs), f"{name}: no (layer, head) behind the first with more candidates than k"


@pytest.mark.parametrize("name", [n for n in CAT if "ties" in _case(n).claims])
def test_tie_families_tie_at_the_threshold_in_every_head(name):
    c, st = _case(name), _stats(name)
    for h in range(c.H):
        n_eq, need = st["eq"][0][h]
        assert 0 < need < n_eq, f"{name}: head {h}: {n_eq} entries at the threshold key, {need} of them kept"


@pytest.mark.parametrize("name", [n for n in CAT if "outside" in _case(n).claims])
def test_outside_the_map_families_hold_ids_no_map_can_reach(name):
    c, st = _case(name), _stats(name)
    for l in range(c.nl):
        ids = c.ids(l).astype(np.int64)
        assert np.all(ids[:, c.his[l] - 1] - ids[:, c.start] >= 1 << 20), f"{name}: layer {l}: window ids less than 2^20 apart"
    assert (1 << 20) > lc.DYN_LDS           # a byte per id: no map fits the dynamic LDS
    assert st["search"] > 0 and st["map"] > 0, f"{name}: membership never answered by " + ("search" if st["search"] == 0 else "the map")


@pytest.mark.parametrize("name", [n for n in CAT if "below_base" in _case(n).claims])
def test_multi_leg_families_ask_for_ids_below_a_legs_map_base(name):
    c, st = _case(name), _stats(name)
    assert lc.dispatch(c)["legs"] >= 4 and st["search_below"] > 0, name


def test_protocol_family_holds_a_token_kept_two_layers_up_dropped_one_layer_up_and_still_present():
    found = 0
    for c in _protocol()[1:]:
        ref = lc.reference(c, rows=False)
        for l in range(2, c.nl):
            for h in range(c.H):
                w = c.ids(l)[h, c.start:c.his[l]]
                found += int(np.sum(np.isin(w, ref["new_ids"][l - 2][h]) & ~np.isin(w, ref["new_ids"][l - 1][h])))
        assert found > 0, c.name
    # ... and the stale-stamp fault gets exactly those wrong (fault 2 above fails on this family)


def test_dispatch_covers_every_path_of_the_event():
    """select kernel, key home, map / no map, leg counts: what the geometry of the catalogue selects, by the host's rule"""
    d = {n: lc.dispatch(_case(n)) for n in CAT}
    assert d["llama7b"]["select"] == d["win4096"]["select"] == "layer_cascade_select_blocked_kernel"
    for n in ("chain_lds_4097", "chain_lds_8192", "chain_lds_15360", "clusters_chain"):
        assert d[n]["select"] == "layer_cascade_select_kernel" and d[n]["keys"] == ["lds"], n
    for n in ("chain_scratch_15361", "chain_scratch_20000"):
        assert d[n]["select"] == "layer_cascade_select_kernel" and d[n]["keys"] == ["lds", "scratch"], n
    assert d["layers254"]["map_ids"] > 0 and d["layers255"]["map_ids"] == 0
    assert d["layers255"]["select"] == "layer_cascade_select_kernel"      # no map: the blocked select is not taken
    assert d["layers254"]["legs"] == d["layers255"]["legs"] == 6
    assert [d[f"layers{n}"]["legs"] for n in (1, 2, 3, 5, 49, 97)] == [1, 2, 3, 4, 4, 4]
    assert lc.dispatch(_case("layers97"), legs_env=1)["legs"] == 3
    assert lc.dispatch(_case("win4096"), blocked_env=0)["select"] == "layer_cascade_select_kernel"


def test_score_families_need_the_last_radix_pass():
    """lowbits: the keys are equal under the mask one pass shorter, distinct under the dtype's own"""
    rng = np.random.default_rng(0)
    for sdt, short in (("f32", 0xFFFFFF00), ("f16", 0xFFFF0000), ("bf16", 0xFF000000)):
        key = orc.ordered_key(lc.make_scores(rng, "lowbits", 1, 500, sdt)[0])
        assert len(np.unique(key & np.uint32(short))) == 1 and len(np.unique(key & np.uint32(lc.KEY_MASK[sdt]))) > 2
        assert np.array_equal(key & np.uint32(lc.KEY_MASK[sdt]), key)        # the mask drops nothing a score of this dtype sets
    for sdt in ("bf16", "f16", "f32"):
        x = lc.make_scores(rng, "special", 2, 4000, sdt)
        assert np.array_equal(orc.round_dt(x, sdt).view(np.uint32), x.view(np.uint32))      # representable, NaN and -0 included
        assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and np.signbit(x[x == 0]).any()
