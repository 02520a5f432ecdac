"""Cases, references and the checker for the layer-cascade prune event (spatten_prune_layer_cascade; ops.LayerCascadePlan).

Everything the event produces is exact by construction — kept positions, slot ids, moved rows, the shadow's three
reproducible roundings, moved accumulator entries — so every comparison in this module is EQUALITY of bits.

  * ``Case`` + the builders: seeded inputs of one event (numpy only), in the fill / score families of ``catalogue`` below;
  * ``reference``: oracle.spatten_oracle.layer_cascade_prune for positions, ids and rows, the oracle's rotary for the
    shadow, numpy indexing for the accumulators; ``select_dumb``: a second statement of the selection rule that does not
    call the oracle's top-k;
  * ``emulate``: the event as the kernels structure it (stamp map + fallback search, legs, masked keys, threshold +
    first-need_eq compaction, head / kept / tail rows), with the seeded faults of tests/test_layer_cascade_cpu.py, and the
    host's dispatch rule (which select kernel, where the keys live, map size, legs) as ``dispatch``;
  * ``check_event``: the one checker, used on the emulation (CPU) and on the device's outputs (GPU);
  * ``run_on_device`` and ``python -m tests.layer_cascade_cases --run NAME ...``: the event on the GPU through
    ops.prune_layer_cascade / ops.LayerCascadePlan, for the GPU tests and for the fresh child processes that run the
    forms chosen by environment variables (the library reads those once per process).
"""
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from oracle import spatten_oracle as orc

KEY_MASK = {"bf16": 0xFFFF0000, "f16": 0xFFFFFF00, "f32": 0xFFFFFFFF}      # significant key bits = radix passes x 8
ES = {"bf16": 2, "f16": 2, "f32": 4}
# the host's dispatch constants (prune_layer_cascade_impl)
BLOCKED_MAX, LDS_KEYS_MAX, MAP_MAX, DYN_LDS, MAP_LAYERS, LEG_LAYERS, DEFAULT_LEGS = 4096, 15360, 96 * 1024, 140 * 1024, 254, 48, 4


@dataclass
class Case:
    name: str
    B: int
    H: int
    d: int
    start: int
    sdt: str
    kdt: str
    lens: List[int]
    tail: int                                   # rows behind the window, the same for every layer (hi = len - tail)
    keeps: List[int]
    id_base: int
    known: List[Optional[np.ndarray]]           # per layer int32 [H, n_known] ascending, or None
    scores: List[np.ndarray]                    # per layer float32 [H, len], values representable in sdt
    accs: Optional[List[np.ndarray]] = None     # per layer float32 [H, len + pad]
    kv_seed: int = 0
    rows: str = "numpy"                         # "numpy": K / V in numpy, rows checked against the oracle; "device": see run_on_device
    claims: tuple = ()                          # conditions tests/test_layer_cascade_cpu.py asserts: fill, ties, outside, below_base, protocol
    _kv: Optional[tuple] = field(default=None, repr=False)

    @property
    def nl(self):
        return len(self.lens)

    @property
    def his(self):
        return [L - self.tail for L in self.lens]

    @property
    def new_lens(self):
        return [self.start + k + self.tail for k in self.keeps]

    def ids(self, l, off_by_one=False):
        """int32 [H, len_l]: the known ids, then id_base + (j - n_known) for the rows appended since."""
        kn = self.known[l]
        nk = 0 if kn is None else kn.shape[1]
        fresh = (self.id_base + np.arange(self.lens[l] - nk, dtype=np.int64) + (1 if off_by_one else 0)).astype(np.int32)
        fresh = np.tile(fresh[None], (self.H, 1))
        return fresh if kn is None else np.concatenate([kn, fresh], 1)

    def kv(self):
        """(K list, V list) float32 [B, H, len_l, d], values representable in kdt."""
        if self._kv is None:
            rng = np.random.default_rng(1000 + self.kv_seed)
            shape = lambda L: (self.B, self.H, L, self.d)
            self._kv = ([orc.round_dt(rng.standard_normal(shape(L), dtype=np.float32), self.kdt) for L in self.lens],
                        [orc.round_dt(rng.standard_normal(shape(L), dtype=np.float32), self.kdt) for L in self.lens])
        return self._kv


# ------------------------------------------------------------------------------------------------
# score families
# ------------------------------------------------------------------------------------------------
def _bits_to_f32(bits, sdt):
    bits = np.asarray(bits)
    if sdt == "bf16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if sdt == "f16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    return bits.astype(np.uint32).view(np.float32)


def make_scores(rng, family, H, n, sdt):
    if family == "normal":
        return orc.round_dt(rng.standard_normal((H, n), dtype=np.float32), sdt)
    if family == "few":                 # a handful of distinct values: the threshold ties in every head
        vals = orc.round_dt(np.array([-1.5, -0.25, 0.125, 0.75, 2.0], dtype=np.float32), sdt)
        return vals[rng.integers(0, 5, (H, n))]
    if family == "equal":
        return np.full((H, n), 0.5, dtype=np.float32)
    if family == "special":
        x = orc.round_dt(rng.standard_normal((H, n), dtype=np.float32), sdt)
        sub = {"bf16": _bits_to_f32([0x0001, 0x0040, 0x8001], "bf16"), "f16": _bits_to_f32([0x0001, 0x03FF, 0x8001], "f16"),
               "f32": _bits_to_f32([0x00000001, 0x007FFFFF, 0x80000001], "f32")}[sdt]
        specials = np.concatenate([np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32), sub])
        hit = rng.random((H, n)) < 0.25
        return np.where(hit, specials[rng.integers(0, len(specials), (H, n))], x).astype(np.float32)
    if family in ("mono_up", "mono_down"):          # strictly monotone: consecutive bit patterns of positive values
        base = {"bf16": 0x1000, "f16": 0x0400, "f32": 0x3F000000}[sdt]
        assert sdt == "f32" or base + n < {"bf16": 0x7F80, "f16": 0x7C00}[sdt]
        row = _bits_to_f32(base + np.arange(n), sdt)
        row = row if family == "mono_up" else row[::-1]
        assert np.all(np.diff(row) != 0)
        return np.tile(row[None], (H, 1)).astype(np.float32)
    if family == "lowbits":             # differ only in the digits the LAST radix pass reads
        if sdt == "f32":                # accumulator-like, in [0.5, 0.5 + 2^-16): only the fourth digit differs
            return _bits_to_f32(0x3F000000 + rng.integers(0, 16, (H, n)) * 16, "f32")
        if sdt == "f16":                # last two mantissa bits -> fp32 bits 13, 14: the third digit
            return _bits_to_f32(0x3800 + rng.integers(0, 4, (H, n)), "f16")
        return _bits_to_f32(0x3F00 + rng.integers(0, 4, (H, n)), "bf16")       # bf16: the second (last) digit
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
def _draw(rng, pool, n):
    return np.sort(rng.choice(pool, size=n, replace=False)).astype(np.int32)


def build(name, seed, nl, H, lens, tail, keeps, *, start=4, sdt="bf16", kdt="bf16", B=1, d=64, fill="subset", none_layers=(),
          score="normal", appended=None, pool=None, id_base=None, acc=False, rows="numpy", claims=(), boost_prev_head=False):
    """One event.  ``fill``: how the known ids of layer l are drawn —
    "none": no known ids at all (every slot is a row appended since: ids = id_base + j);
    "subset": a subset of layer l-1's known ids (what an earlier cascade leaves);
    "independent": every layer draws from one common pool (many non-members: the fill rule);
    "spread": independent draws from a pool whose ids lie 2^20 or more apart (no map can hold them);
    "clusters": dense low ids, with id_base 3 * 2^20 above them (the appended rows of the window are outside the map).
    ``none_layers``: layers whose known ids are None although others have some.  ``boost_prev_head``: a window slot whose
    token sits in the previous layer's HEAD rows gets a top score (with uniform start and tail this only happens under the
    independent fill: the case that tells "member of the whole previous id row" from "member of what was kept")."""
    rng = np.random.default_rng(seed)
    lens = [lens] * nl if isinstance(lens, int) else list(lens)
    keeps = [keeps] * nl if isinstance(keeps, int) else list(keeps)
    assert len(lens) == len(keeps) == nl and all(b <= a for a, b in zip(keeps, keeps[1:]))
    appended = min(lens) // 10 if appended is None else appended
    known = [None] * nl
    if fill != "none":
        nks = [L - appended for L in lens]
        if fill == "spread":
            pool_ids = np.cumsum(rng.integers(1 << 20, (1 << 20) + 4096, size=pool or int(max(nks) * 1.5)))
            assert pool_ids[-1] < (1 << 31) - (1 << 22)
            id_base = int(pool_ids[-1]) + (1 << 21) if id_base is None else id_base
        elif fill == "clusters":
            pool_ids = np.arange(pool or int(max(nks) * 1.5))
            id_base = 3 << 20 if id_base is None else id_base
        else:
            pool_ids = np.arange(pool or int(max(nks) * 1.6))
        prev = None
        for l in range(nl):
            rows_ = []
            for h in range(H):
                src = pool_ids if (prev is None or fill != "subset") else prev[h]
                rows_.append(_draw(rng, src, nks[l]))
            known[l] = np.stack(rows_)
            prev = known[l]
        for l in none_layers:
            known[l] = None
        id_base = int(pool_ids[-1]) + 1000 if id_base is None else id_base
    else:
        id_base = 0 if id_base is None else id_base
    scores = [make_scores(rng, score, H, L, sdt) for L in lens]
    if boost_prev_head:
        for l in range(1, nl):
            for h in range(H):
                hit = np.isin(known[l][h], known[l - 1][h, :start])
                hit[:start] = False
                scores[l][h, :len(hit)][hit] = 4.0
    accs = [rng.random((H, L + 16), dtype=np.float32) for L in lens] if acc else None
    return Case(name, B, H, d, start, sdt, kdt, lens, tail, keeps, int(id_base), known, scores, accs, seed, rows, tuple(claims))


def build_protocol(name, seed, nl, H, len0, tail, keeps, appended, events=3, **kw):
    """``events`` successive events of one conversation: event e + 1 holds, per layer, what event e left (its new ids as the
    known ids, its rows and accumulators) plus ``appended`` new rows, under a risen id_base; scores are drawn anew.  This is
    where a token kept by layer l-2, dropped by layer l-1 and still held by layer l occurs."""
    score = kw.pop("score", "normal")
    acc = kw.pop("acc", True)
    first = build(f"{name}/0", seed, nl, H, len0, tail, keeps, fill="none", id_base=0, score=score, acc=acc, claims=("protocol",), **kw)
    out = [first]
    rng = np.random.default_rng(seed + 77)
    for e in range(1, events):
        c = out[-1]
        ref = reference(c)
        K, V = c.kv()
        n_app = c.lens[0] - (0 if c.known[0] is None else c.known[0].shape[1])
        lens = [n + appended for n in c.new_lens]
        newK = [np.concatenate([ref["K"][l], orc.round_dt(rng.standard_normal((c.B, c.H, appended, c.d), dtype=np.float32), c.kdt)], 2)
                for l in range(nl)]
        newV = [np.concatenate([ref["V"][l], orc.round_dt(rng.standard_normal((c.B, c.H, appended, c.d), dtype=np.float32), c.kdt)], 2)
                for l in range(nl)]
        accs = None
        if acc:
            accs = [np.concatenate([ref["accs"][l], rng.random((c.H, appended + 16), dtype=np.float32)], 1) for l in range(nl)]
        scores = [make_scores(rng, score, H, L, c.sdt) for L in lens]
        nxt = Case(f"{name}/{e}", c.B, c.H, c.d, c.start, c.sdt, c.kdt, lens, tail, list(keeps), c.id_base + n_app,
                   [x.copy() for x in ref["new_ids"]], scores, accs, seed + e, "numpy", ("protocol",))
        nxt._kv = (newK, newV)
        out.append(nxt)
    return out


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def select_dumb(ids, score, prev_ids, start, hi, k):
    """The selection rule of one (layer, head), stated without the oracle's top-k: order the window by (candidates first, key
    descending, position ascending), take k, sort by position.  A candidate is a slot whose token the previous layer kept;
    the fill rule — a window with fewer than k candidates is filled with the LOWEST-POSITION other slots — and the oracle's
    reading of it (a candidate scored -inf ranks with the non-candidates: both carry the key of -inf) are stated as: the
    others all compare equal."""
    w = np.arange(start, hi)
    kept_before = None if prev_ids is None else set(prev_ids.tolist())
    member = np.ones(len(w), bool) if prev_ids is None else np.array([int(t) in kept_before for t in ids[start:hi]], dtype=bool)
    key = orc.ordered_key(score[start:hi]).astype(np.int64)
    floor = int(orc.ordered_key(np.array([-np.inf], dtype=np.float32))[0])
    eff = np.where(member & (key > floor), key, floor)
    order = sorted(range(len(w)), key=lambda i: (-int(eff[i]), i))[:k]
    return np.sort(w[np.array(order)]).astype(np.int32)


def reference(case: Case, rows=True):
    """dict(idx, new_ids, K, V, Kr, accs): the oracle's event.  K / V / Kr are None for a case whose rows live on the device."""
    rows = rows and case.rows == "numpy"
    nl, H = case.nl, case.H
    ids = [case.ids(l) for l in range(nl)]
    if rows:
        K, V = case.kv()
        past = [(K[l], V[l]) for l in range(nl)]
    else:
        past = [(np.zeros((1, H, L, 1), np.float32),) * 2 for L in case.lens]
    new_past, new_ids, idxs = orc.layer_cascade_prune(past, ids, case.scores, 0, case.start, case.tail, case.keeps)
    out = dict(idx=idxs, new_ids=[x.astype(np.int32) for x in new_ids], K=None, V=None, Kr=None, accs=None)
    if rows:
        out["K"], out["V"] = [p[0] for p in new_past], [p[1] for p in new_past]
        out["Kr"] = [shadow_of(out["K"][l], case.d, case.kdt) for l in range(nl)]
    if case.accs is not None:
        out["accs"] = [np.stack([np.concatenate([a[h, :case.start], a[h, idxs[l][h]], a[h, case.his[l]:case.lens[l]]]) for h in range(H)])
                       for l, a in enumerate(case.accs)]
    return out


def shadow_of(K_new, d, kdt):
    n = K_new.shape[2]
    cos, sin = orc.rope_table(n, d, kdt)
    return orc.apply_rotary_pos_emb_single(K_new, cos, sin, np.arange(n)[None], kdt)


def reference_dumb(case: Case):
    """(idx, new_ids) per layer from select_dumb alone."""
    idxs, nids, prev = [], [], None
    for l in range(case.nl):
        ids, hi = case.ids(l), case.his[l]
        idx = np.stack([select_dumb(ids[h], case.scores[l][h], None if prev is None else prev[h], case.start, hi, case.keeps[l])
                        for h in range(case.H)])
        nid = np.stack([np.concatenate([ids[h, :case.start], ids[h, idx[h]], ids[h, hi:]]) for h in range(case.H)])
        idxs.append(idx)
        nids.append(nid)
        prev = nid
    return idxs, nids


# ------------------------------------------------------------------------------------------------
# the host's dispatch, and the event as the kernels structure it
# ------------------------------------------------------------------------------------------------
def dispatch(case: Case, legs_env=DEFAULT_LEGS, blocked_env=1):
    """What prune_layer_cascade_impl chooses for this geometry: select kernel, where each layer's keys live, map size, legs."""
    nl, start = case.nl, case.start
    max_w = max(case.his) - start
    lds_keys = min(max_w, LDS_KEYS_MAX)
    map_ids = (min(MAP_MAX, DYN_LDS - lds_keys * 4) & ~3) if nl <= MAP_LAYERS else 0
    legs = min(max(legs_env, -(-nl // LEG_LAYERS)), nl)
    bounds = [(nl * g // legs, nl * (g + 1) // legs) for g in range(legs)]
    assert all(b - a <= LEG_LAYERS for a, b in bounds)
    blocked = bool(blocked_env) and max_w <= BLOCKED_MAX and map_ids > 0
    keys = sorted({"registers" if blocked else ("lds" if hi - start <= lds_keys else "scratch") for hi in case.his})
    return dict(select="layer_cascade_select_blocked_kernel" if blocked else "layer_cascade_select_kernel", keys=keys,
                map_ids=map_ids, legs=legs, bounds=bounds, max_w=max_w)


def _sentinel_planes(case, caps):
    """raw-bit destination planes filled with a sentinel pattern, as float32-free integer arrays"""
    dt = np.uint32 if ES[case.kdt] == 4 else np.uint16
    val = 0x7B7B7B7B if ES[case.kdt] == 4 else 0x7B7B
    return [np.full((case.B, case.H, caps[l], case.d), val, dtype=dt) for l in range(case.nl)]


def raw_bits(x, kdt):
    """float32 array of kdt-representable values -> the dtype's bit patterns"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if kdt == "f32":
        return x.view(np.uint32)
    if kdt == "bf16":
        return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return x.astype(np.float16).view(np.uint16)


def emulate(case: Case, faults=(), legs_env=DEFAULT_LEGS, blocked_env=1, caps=None):
    """The event in numpy, structured like the kernels.  Returns (outputs, planes, stats): outputs = the event's six results
    (K', V', Kr', idx, new_ids, new accs — lists per layer; rows None for a device-rows case), planes = the full raw-bit
    destination planes (sentinel beyond new_len), stats = how membership was answered (map hits, searches, searches of ids
    below the leg's map_base) and per (layer, head) the candidates in the window.  ``faults``: the seeded faults 1..11 of
    tests/test_layer_cascade_cpu.py."""
    F = set(faults)
    nl, H, start = case.nl, case.H, case.start
    dsp = dispatch(case, legs_env, blocked_env)
    R = dsp["map_ids"]
    mask = KEY_MASK[case.sdt]
    if 6 in F:
        mask = {"f16": 0xFFFF0000, "f32": 0xFFFFFF00, "bf16": 0xFF000000}[case.sdt]
    ids_all = [case.ids(l, off_by_one=3 in F) for l in range(nl)]
    idxs = [np.zeros((H, case.keeps[l]), np.int32) for l in range(nl)]
    nids = [np.zeros((H, case.new_lens[l]), np.int32) for l in range(nl)]
    stats = dict(map=0, search=0, search_below=0, members=[[0] * H for _ in range(nl)], eq=[[(0, 0)] * H for _ in range(nl)])
    neg_inf_key = int(orc.ordered_key(np.array([-np.inf], np.float32))[0])
    for h in range(H):
        ever = np.zeros(0, np.int32)
        member_rows = [None] * nl          # what layer l "kept" as the next layer's membership sees it
        for l0, l1 in dsp["bounds"]:
            smap = np.zeros(max(R, 1), np.uint8)
            map_base = int(ids_all[l0][h, start])

            def stamp(row, l):
                off = (row.astype(np.int64) - map_base) & 0xFFFFFFFF
                ok = off < R
                smap[off[ok]] = (l + 1) & 0xFF

            prev = None
            if l0 > 0:
                prev = member_rows[l0 - 1]
                stamp(prev, l0 - 1)
            for l in range(l0, l1):
                tid, hi, k, L = ids_all[l][h], case.his[l], case.keeps[l], case.lens[l]
                w = tid[start:hi]
                sc = case.scores[l][h, start:hi]
                member = np.ones(len(w), bool)
                if prev is not None:
                    off = (w.astype(np.int64) - map_base) & 0xFFFFFFFF
                    inmap = off < R
                    member = np.zeros(len(w), bool)
                    member[inmap] = smap[off[inmap]] == (l & 0xFF)
                    out = ~inmap
                    pos = np.searchsorted(prev, w[out])
                    member[out] = (pos < len(prev)) & (prev[np.minimum(pos, len(prev) - 1)] == w[out])
                    stats["map"] += int(inmap.sum())
                    stats["search"] += int(out.sum())
                    stats["search_below"] += int((w[out].astype(np.int64) < map_base).sum())
                    if 2 in F:
                        member = np.isin(w, ever)
                stats["members"][l][h] = int(member.sum())
                key = orc.ordered_key(np.where(member, sc, np.float32(-np.inf)).astype(np.float32)).astype(np.int64)
                if 7 in F:
                    key = np.where(np.isnan(sc) & member, 0, key)
                if 5 in F and prev is not None:      # non-members keep an order of their own below every member
                    own = orc.ordered_key(sc).astype(np.int64)
                    key = np.where(member & (key > neg_inf_key), key + (1 << 33), own)
                key = key & mask if 5 not in F else key
                thr = np.sort(key)[::-1][k - 1]
                gt, eq = key > thr, key == thr
                need = k - int(gt.sum())
                stats["eq"][l][h] = (int(eq.sum()), need)
                eq_pos = np.flatnonzero(eq)
                take = eq_pos[-need:] if 4 in F else eq_pos[:need]
                keep = gt.copy()
                keep[take] = True
                idx = (np.flatnonzero(keep) + start).astype(np.int32)
                assert len(idx) == k
                idxs[l][h] = idx
                t0 = min(hi + 1, L) if 8 in F else hi
                tail_rows = np.minimum(np.arange(t0, t0 + (L - hi)), L - 1)
                nid = np.concatenate([tid[:start], tid[idx], tid[tail_rows]])
                nids[l][h] = nid
                seen = tid[idx] if 1 in F else nid
                seen = np.sort(seen)
                stamp(seen, l)
                member_rows[l] = seen
                ever = np.union1d(ever, seen)
                prev = seen
    # ---- the ragged gathers
    caps = caps or [n + 5 for n in case.new_lens]
    Kd = Vd = Krd = None
    outs = [None, None, None]
    if case.rows == "numpy":
        K, V = case.kv()
        Kd, Vd, Krd = _sentinel_planes(case, caps), _sentinel_planes(case, caps), _sentinel_planes(case, caps)
        outs = [[], [], []]
        for l in range(nl):
            hi, L, n = case.his[l], case.lens[l], case.new_lens[l]
            t0 = min(hi + 1, L) if 8 in F else hi
            tail_rows = np.minimum(np.arange(t0, t0 + (L - hi)), L - 1)
            src = np.stack([np.concatenate([np.arange(start), idxs[l][h], tail_rows]) for h in range(H)])      # [H, n]
            kn = np.stack([np.stack([K[l][0 if (11 in F and b == 1) else b, h, src[h]] for h in range(H)]) for b in range(case.B)])
            vn = np.stack([np.stack([V[l][0 if (11 in F and b == 1) else b, h, src[h]] for h in range(H)]) for b in range(case.B)])
            cos, sin = orc.rope_table(max(n, L), case.d, case.kdt)
            if 9 in F:
                kr = np.stack([orc.apply_rotary_pos_emb_single(kn[:, h:h + 1], cos, sin, src[h][None], case.kdt)[:, 0] for h in range(H)], 1)
            else:
                kr = orc.apply_rotary_pos_emb_single(kn, cos, sin, np.arange(n)[None], case.kdt)
            for plane, x, o in ((Kd, kn, outs[0]), (Vd, vn, outs[1]), (Krd, kr, outs[2])):
                plane[l][:, :, :n] = raw_bits(x, case.kdt)
                o.append(x)
    new_accs = None
    if case.accs is not None:
        new_accs = []
        for l, a in enumerate(case.accs):
            hi, L, n = case.his[l], case.lens[l], case.new_lens[l]
            t0 = min(hi + 1, L) if 8 in F else hi
            tail_rows = np.minimum(np.arange(t0, t0 + (L - hi)), L - 1)
            wide = np.zeros((H, max(caps[l], a.shape[1])), np.float32)
            for h in range(H):
                mid = idxs[l][h] - (start if 10 in F else 0)
                wide[h, :n] = np.concatenate([a[h, :start], a[h, mid], a[h, tail_rows]])
            new_accs.append(wide)
    planes = None if Kd is None else dict(K=Kd, V=Vd, Kr=Krd, sentinel=0x7B7B7B7B if ES[case.kdt] == 4 else 0x7B7B)
    return (outs[0], outs[1], outs[2], idxs, nids, new_accs), planes, stats


# ------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------
def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def check_event(case: Case, outputs, ref, planes=None):
    """The event's six outputs (K', V', Kr', idx, new_ids, new accs: lists per layer of numpy arrays; new accs at their full
    width) against ``reference(case)``.  Everything is equality of bits.  ``planes`` = dict(K, V, Kr: the full caller-supplied
    destination planes as raw bit patterns, sentinel: the pattern they were filled with): rows beyond new_len untouched.
    Raises AssertionError naming the first difference."""
    Kn, Vn, Krn, idxs, nids, accs = outputs
    start = case.start
    for l in range(case.nl):
        hi, k, n = case.his[l], case.keeps[l], case.new_lens[l]
        idx, nid = np.asarray(idxs[l]), np.asarray(nids[l])
        assert idx.shape == (case.H, k) and nid.shape == (case.H, n), (case.name, l, idx.shape, nid.shape)
        assert np.all(np.diff(idx.astype(np.int64), axis=1) > 0), f"{case.name}: layer {l}: kept positions not strictly ascending"
        assert idx.min() >= start and idx.max() < hi, f"{case.name}: layer {l}: kept positions outside [{start}, {hi})"
        assert np.all(np.diff(nid.astype(np.int64), axis=1) > 0), f"{case.name}: layer {l}: new ids not strictly ascending"
        assert np.array_equal(idx, ref["idx"][l]), f"{case.name}: layer {l}: kept positions differ from the oracle " \
            f"(heads {np.flatnonzero((idx != ref['idx'][l]).any(1))[:8].tolist()})"
        assert np.array_equal(nid, ref["new_ids"][l]), f"{case.name}: layer {l}: new ids differ from the oracle"
        if ref["K"] is not None:
            assert Kn is not None and Kn[l].shape == ref["K"][l].shape, (case.name, l)
            assert np.array_equal(_bits(Kn[l]), _bits(ref["K"][l])), f"{case.name}: layer {l}: K rows differ"
            assert np.array_equal(_bits(Vn[l]), _bits(ref["V"][l])), f"{case.name}: layer {l}: V rows differ"
            assert np.array_equal(_bits(Krn[l]), _bits(ref["Kr"][l])), f"{case.name}: layer {l}: rotated shadow differs"
        if ref["accs"] is not None:
            a = np.asarray(accs[l])
            assert a.shape[1] >= n and np.array_equal(_bits(a[:, :n]), _bits(ref["accs"][l])), f"{case.name}: layer {l}: accumulators differ"
            assert not _bits(a[:, n:]).any(), f"{case.name}: layer {l}: new accumulator tail not zero"
        if planes is not None and planes.get("sentinel") is not None:
            for name in ("K", "V", "Kr"):
                assert np.all(planes[name][l][:, :, n:] == planes["sentinel"]), f"{case.name}: layer {l}: {name} rows beyond new_len written"


# ------------------------------------------------------------------------------------------------
# the catalogue
# ------------------------------------------------------------------------------------------------
def _shrink(k0, nl, by):
    return [max(k0 - by * l, 1) for l in range(nl)]


def _stairs(k0, nl, every=2, factor=0.4):
    """keeps that stay for ``every`` layers, then drop by ``factor``: under the independent fill a layer whose k equals the
    previous layer's finds FEWER candidates than k in its window (not every kept token is held by the next layer), a layer
    behind a drop finds MORE"""
    return [max(int(k0 * factor ** (l // every)), 2) for l in range(nl)]


def _window_case(W, k, **kw):
    """3 layers, 2 heads, window of exactly W entries, independent fill"""
    start, tail = kw.pop("start", 4), kw.pop("tail", 9)
    L = start + W + tail
    name = kw.pop("name", f"win{W}_k{k}")
    return build(name, 11 + W + k, 3, 2, L, tail, k, start=start, fill=kw.pop("fill", "independent"),
                 appended=kw.pop("appended", min(L // 10, max(tail - 1, 0)) + 1), **kw)


def catalogue():
    """name -> zero-argument builder.  Every case is a valid call."""
    C = {}

    def add(name, fn):
        assert name not in C
        C[name] = fn
    # ---- blocked select (every window <= 4096)
    for sdt in ("bf16", "f16", "f32"):
        for kdt in ("bf16", "f16", "f32"):
            add(f"ragged_{sdt}_{kdt}", lambda sdt=sdt, kdt=kdt: build(
                f"ragged_{sdt}_{kdt}", 3, 4, 3, [700, 650, 650, 500], 40, _stairs(300, 4), sdt=sdt, kdt=kdt, B=2, d=64,
                fill="independent", pool=1000, acc=True, claims=("fill",), boost_prev_head=True))
    for W in (1, 1023, 1024, 1025, 4095, 4096):
        add(f"win{W}", lambda W=W: _window_case(W, max(W // 3, 1), name=f"win{W}"))
    add("win_k", lambda: _window_case(300, 300, name="win_k"))                      # k = window: keep everything
    add("win_k_plus_1", lambda: _window_case(301, 300, name="win_k_plus_1"))
    add("keep_one", lambda: _window_case(500, 1, name="keep_one"))
    add("start0", lambda: _window_case(600, 200, start=0, name="start0", acc=True))
    add("no_tail", lambda: _window_case(600, 200, tail=0, appended=30, name="no_tail", acc=True))
    add("start0_no_tail", lambda: _window_case(600, 200, start=0, tail=0, appended=30, name="start0_no_tail", acc=True))
    add("long_tail", lambda: build("long_tail", 5, 3, 2, 3200, 2500, [300, 200, 100], fill="subset", appended=2700, acc=True))
    for B in (1, 3):
        add(f"batch{B}", lambda B=B: build(f"batch{B}", 6, 3, 2, 400, 30, [150, 140, 100], B=B, d=128, fill="subset"))
    for d, kdt in ((80, "bf16"), (256, "f16"), (64, "f32"), (8, "f32"), (16, "bf16")):
        add(f"d{d}_{kdt}", lambda d=d, kdt=kdt: build(f"d{d}_{kdt}", 7, 3, 2, 300, 20, [100, 90, 90], d=d, kdt=kdt, B=2, fill="subset"))
    add("heads1", lambda: build("heads1", 8, 3, 1, 500, 20, [200, 150, 100], fill="independent"))
    add("heads40", lambda: build("heads40", 9, 3, 40, 500, 20, [200, 200, 80], d=16, fill="independent", claims=("fill",),
                                 boost_prev_head=True))
    add("known_none", lambda: build("known_none", 10, 4, 4, [900, 880, 860, 860], 64, _shrink(400, 4, 30), fill="none", id_base=700, acc=True))
    add("known_some_none", lambda: build("known_some_none", 12, 5, 3, 600, 30, _shrink(250, 5, 20), fill="subset", none_layers=(1, 3)))
    add("short_then_long", lambda: build("short_then_long", 13, 4, 2, [3000, 600, 2800, 500], 16, [200, 150, 150, 100], fill="independent",
                                         pool=4000))                                # the prefetch clamps: W < 1024 next to W > 1024
    for sdt in ("bf16", "f16", "f32"):
        add(f"special_{sdt}", lambda sdt=sdt: build(f"special_{sdt}", 14, 4, 4, 700, 30, _stairs(300, 4), sdt=sdt, fill="independent",
                                                    pool=1000, score="special", claims=("fill",)))
        add(f"few_{sdt}", lambda sdt=sdt: build(f"few_{sdt}", 15, 3, 4, 2000, 30, _shrink(700, 3, 100), sdt=sdt, fill="subset", score="few",
                                                claims=("ties",)))
        add(f"equal_{sdt}", lambda sdt=sdt: build(f"equal_{sdt}", 16, 3, 3, 800, 30, _shrink(300, 3, 50), sdt=sdt, fill="subset",
                                                  score="equal", claims=("ties",)))
        add(f"lowbits_{sdt}", lambda sdt=sdt: build(f"lowbits_{sdt}", 17, 3, 3, 3000, 30, _shrink(1000, 3, 100), sdt=sdt, fill="subset",
                                                    score="lowbits", claims=("ties",)))
        add(f"mono_up_{sdt}", lambda sdt=sdt: build(f"mono_up_{sdt}", 18, 3, 2, 1500, 30, _shrink(500, 3, 100), sdt=sdt, fill="none",
                                                    score="mono_up"))
        add(f"mono_down_{sdt}", lambda sdt=sdt: build(f"mono_down_{sdt}", 19, 3, 2, 1500, 30, _shrink(500, 3, 100), sdt=sdt, fill="subset",
                                                      score="mono_down"))
    add("llama7b", lambda: build("llama7b", 20, 32, 32, 4096, 128, [2048 - 40 * l for l in range(32)], d=128, fill="subset", appended=96,
                                 acc=False, rows="device"))
    # ---- chain_body, keys in LDS (some window in 4097 .. 15360); one small layer inside the same launch
    for W, sdt, score in ((4097, "bf16", "normal"), (8192, "f16", "few"), (15360, "f32", "lowbits")):
        L = 4 + W + 33
        add(f"chain_lds_{W}", lambda W=W, sdt=sdt, score=score, L=L: build(
            f"chain_lds_{W}", 21, 4, 3, [900, L, L - 100, 800], 33, _stairs(600, 4), sdt=sdt, d=16, fill="independent",
            pool=int(L * 1.4), score=score, acc=True, claims=("fill",) + (("ties",) if score != "normal" else ())))
    add("chain_lds_special", lambda: build("chain_lds_special", 22, 3, 2, 5000, 40, [2000, 1500, 1000], sdt="bf16", d=16, fill="subset",
                                           score="special"))
    # ---- chain_body, keys in the global scratch (some window > 15360)
    for W, sdt in ((15361, "bf16"), (20000, "f32")):
        L = 4 + W + 20
        add(f"chain_scratch_{W}", lambda W=W, sdt=sdt, L=L: build(
            f"chain_scratch_{W}", 23, 4, 4, [L, L - 3000, L - 3000, 2000], 20, [6000, 6000, 2400, 700], sdt=sdt, d=16, fill="independent", pool=int(L * 1.4),
            acc=True, claims=("fill",)))
    # ---- membership by binary search: ids no map can hold
    add("spread_blocked", lambda: build("spread_blocked", 24, 4, 3, 1200, 30, _stairs(500, 4), fill="spread", pool=1900, d=16,
                                        claims=("outside", "fill")))
    add("clusters_blocked", lambda: build("clusters_blocked", 25, 4, 3, 3000, 30, _shrink(1200, 4, 100), fill="clusters", appended=1400, d=16,
                                          claims=("outside",)))
    add("clusters_chain", lambda: build("clusters_chain", 26, 4, 3, [6000, 6000, 5500, 5000], 30, _shrink(2500, 4, 200), fill="clusters",
                                        appended=2500, d=16, claims=("outside",)))
    add("spread_legs", lambda: build("spread_legs", 27, 8, 2, 1000, 30, _shrink(400, 8, 20), fill="spread", pool=1700, d=16,
                                     claims=("outside", "below_base")))
    # ---- map / no map, more than four legs, legs re-stamping the previous leg's row
    for nl in (254, 255):
        add(f"layers{nl}", lambda nl=nl: build(f"layers{nl}", 28, nl, 2, 340, 16, _stairs(150, nl, 42, 0.7), d=16,
                                               fill="independent", pool=320, acc=True, claims=("fill", "below_base")))
    for nl in (1, 2, 3, 5, 49, 97):
        add(f"layers{nl}", lambda nl=nl: build(f"layers{nl}", 29, nl, 2, 400, 16, _stairs(180, nl, max(2, nl // 6), 0.7), d=16,
                                               fill="independent", pool=380, claims=("fill",) if nl > 2 else ()))
    return C


def protocol_cases(seed=31, sdt="bf16", len0=700, nl=4):
    return build_protocol("protocol", seed, nl, 3, len0, 24, _shrink(260, nl, 30), 90, sdt=sdt, d=16, B=2)


# the forms chosen by environment (read once per process by the library): small families for the child runner
RUNNER_FAMILIES = {
    "blocked_small": ["ragged_bf16_bf16", "ragged_f32_f16", "few_f16", "special_f32", "win1", "win1025", "win4096", "start0_no_tail",
                      "spread_blocked", "layers5", "layers49", "layers97", "layers254", "layers255", "protocol"],
}


# ------------------------------------------------------------------------------------------------
# the event on the device
# ------------------------------------------------------------------------------------------------
def run_on_device(case: Case, use_dst=False, known_override=None):
    """The event through ops.prune_layer_cascade (``use_dst``: through ops.LayerCascadePlan with caller-supplied, sentinel-filled
    destination planes).  Returns (outputs, planes) for check_event.  A device-rows case returns rows None and checks them here,
    against plain torch indexing driven by the ORACLE's positions (and the shadow of the first and last layer against the
    numpy oracle)."""
    import torch
    from spatten_amd import ops
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    nl, H, B, d, start = case.nl, case.H, case.B, case.d, case.start
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(tdt[dt]).cuda()
    scores = [up(s, case.sdt) for s in case.scores]
    known = [None if k is None else torch.from_numpy(np.ascontiguousarray(k)).cuda() for k in (known_override or case.known)]
    accs = None if case.accs is None else [torch.from_numpy(a).cuda() for a in case.accs]
    new_lens = case.new_lens
    n_tab = max(max(new_lens), 8)
    c, s = orc.rope_table(n_tab, d, case.kdt)
    rope = (up(c[:, :d // 2], case.kdt), up(s[:, :d // 2], case.kdt))
    if case.rows == "numpy":
        K, V = case.kv()
        Ks, Vs = [up(x, case.kdt) for x in K], [up(x, case.kdt) for x in V]
    else:
        g = torch.Generator(device="cuda").manual_seed(case.kv_seed)
        Ks = [torch.randn(B, H, L, d, device="cuda", generator=g).to(tdt[case.kdt]) for L in case.lens]
        Vs = [torch.randn(B, H, L, d, device="cuda", generator=g).to(tdt[case.kdt]) for L in case.lens]
    caps = [n + 5 for n in new_lens]
    planes = None
    if use_dst:
        idt = torch.int32 if ES[case.kdt] == 4 else torch.int16
        sent = 0x7B7B7B7B if ES[case.kdt] == 4 else 0x7B7B
        mk = lambda: [torch.full((B, H, caps[l], d), sent, dtype=idt, device="cuda").view(tdt[case.kdt]) for l in range(nl)]
        dst = (mk(), mk(), mk())
        plan = ops.LayerCascadePlan(scores, known, case.id_base, Ks, Vs, case.lens, case.his, case.keeps, start, caps, rope, accs, dst=dst)
        out = plan.run()
    else:
        out = ops.prune_layer_cascade(scores, known, case.id_base, Ks, Vs, case.lens, case.his, case.keeps, start, caps, rope, accs)
    torch.cuda.synchronize()
    Kn, Vn, Krn, idxs, nids, naccs = out
    f32 = lambda t: t.float().cpu().numpy()
    if use_dst:
        udt = np.uint32 if ES[case.kdt] == 4 else np.uint16
        raw = lambda ts: [t.view(idt).cpu().numpy().view(udt) for t in ts]
        planes = dict(K=raw(dst[0]), V=raw(dst[1]), Kr=raw(dst[2]), sentinel=sent)
    res_idx, res_ids = [t.cpu().numpy() for t in idxs], [t.cpu().numpy() for t in nids]
    res_acc = None if naccs is None else [t.cpu().numpy() for t in naccs]
    if case.rows == "numpy":
        return ([f32(t) for t in Kn], [f32(t) for t in Vn], [f32(t) for t in Krn], res_idx, res_ids, res_acc), planes
    # ---- rows on the device: torch indexing with the oracle's positions; no project kernel on this side
    ref = reference(case, rows=False)
    for l in range(nl):
        io = torch.from_numpy(ref["idx"][l].astype(np.int64)).cuda()[None, :, :, None].expand(B, H, case.keeps[l], d)
        for got, src, what in ((Kn[l], Ks[l], "K"), (Vn[l], Vs[l], "V")):
            want = torch.cat([src[:, :, :start], src.gather(2, io), src[:, :, case.his[l]:case.lens[l]]], 2)
            assert torch.equal(got, want), f"{case.name}: layer {l}: {what} rows differ from torch indexing with the oracle's positions"
    for l in (0, nl - 1):
        want = shadow_of(f32(Kn[l]), d, case.kdt)
        assert np.array_equal(_bits(f32(Krn[l])), _bits(want)), f"{case.name}: layer {l}: rotated shadow differs"
    return (None, None, None, res_idx, res_ids, res_acc), planes


def run_and_check(case: Case, use_dst=False):
    outputs, planes = run_on_device(case, use_dst)
    check_event(case, outputs, reference(case), planes)


def run_protocol_on_device(cases):
    """Successive events: each is fed the DEVICE's new ids of the event before as its known ids."""
    import torch  # noqa: F401
    fed = None
    for c in cases:
        outputs, _ = run_on_device(c, known_override=fed)
        check_event(c, outputs, reference(c))
        fed = outputs[4]


def main(argv):
    """--run NAME [NAME ...]: the named catalogue cases (or families of RUNNER_FAMILIES; "protocol") on the device, in this
    process, against the same checker.  Prints one line per case; exit status 0 only when all pass."""
    if len(argv) < 2 or argv[0] != "--run":
        print(main.__doc__)
        return 2
    names = []
    for a in argv[1:]:
        names += RUNNER_FAMILIES.get(a, [a])
    C = catalogue()
    for n in names:
        if n == "protocol":
            run_protocol_on_device(protocol_cases())
        else:
            case = C[n]()
            run_and_check(case, use_dst=case.rows == "numpy" and case.nl <= 8)
        print(f"ok {n}", flush=True)
    print(f"all {len(names)} cases pass")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
