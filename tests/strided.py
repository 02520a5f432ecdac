"""Padded views with guard bands: the infrastructure of the strided-argument tests (tests/test_gpu_strided_views.py on the
GPU, tests/test_strided_views_cpu.py everywhere).  Test infrastructure only: no fixture, no pytest setting.

The criterion: a call whose tensor arguments are views into larger parents must give, bit for bit, what the
same call on freshly allocated contiguous tensors gives, must not change a byte of a parent outside its view, and — because the
guards of inputs hold NaN / 0x7fffffff / 0xFF — must not have read one either.

``padded`` builds one view, ``Guards`` watches the parents of one call, ``Case`` runs a call twice (contiguous, strided) and
asserts the three properties.  ``COVERED`` / ``NOT_COVERED`` are the ledger of every stride ``include/spatten.h`` declares.
"""
import os
import re
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spatten.h")

I32_GUARD = 0x7FFFFFFF
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's values as integers of the same width (NaN patterns compare equal under torch.equal)."""
    t = t.contiguous()
    return t if not t.dtype.is_floating_point else t.view(_BITS[t.element_size()])


def guard_value(dtype: torch.dtype):
    """Default guard fill: NaN for floating tensors, 0x7fffffff for int32 / int64 (an index or a position far outside every
    table), 0xFF for bytes, -1 otherwise."""
    if dtype.is_floating_point:
        return float("nan")
    if dtype in (torch.int32, torch.int64):
        return I32_GUARD
    if dtype == torch.uint8:
        return 0xFF
    return -1


def padded(t: torch.Tensor, pads, guard=None):
    """(view, parent, mask): ``view`` has t's shape and values and lies inside the freshly allocated ``parent``, which is larger
    than t by ``pads[dim]`` elements in front and behind in every dimension (0 = no pad: the innermost dimension of a row the ABI
    wants contiguous, the row pitch of a cache); ``mask`` is a boolean tensor of the parent's shape, True on the view's elements.
    A pad of dimension i + 1 is what moves the stride of dimension i away from its contiguous value; a pad of dimension i is the
    guard a kernel lands in when it is off by one in that dimension.  ``pads="flat"``: t stays dense inside a 1-D parent with 64
    guard elements on either side (arguments the ABI takes without strides).  Everything outside the view holds ``guard``."""
    g = guard_value(t.dtype) if guard is None else guard
    if isinstance(pads, str):
        assert pads == "flat"
        n = t.numel()
        parent = torch.full((n + 128,), g, dtype=t.dtype, device=t.device)
        mask = torch.zeros(n + 128, dtype=torch.bool, device=t.device)
        mask[64:64 + n] = True
        view = parent[64:64 + n].view(t.shape)
        view.copy_(t)
        return view, parent, mask
    assert len(pads) == t.dim(), (pads, t.shape)
    shape = [n + 2 * p for n, p in zip(t.shape, pads)]
    parent = torch.full(shape, g, dtype=t.dtype, device=t.device)
    sl = tuple(slice(p, p + n) for n, p in zip(t.shape, pads))
    view = parent[sl]
    view.copy_(t)
    mask = torch.zeros(shape, dtype=torch.bool, device=t.device)
    mask[sl] = True
    return view, parent, mask


def contiguous_strides(shape):
    out, acc = [], 1
    for n in reversed(shape):
        out.append(acc)
        acc *= n
    return tuple(reversed(out))


def padded_strides(shape, pads):
    """The element strides ``padded`` gives a tensor of ``shape`` (pure arithmetic: the pad tables are judged without tensors)."""
    if isinstance(pads, str):
        return contiguous_strides(shape)
    return contiguous_strides([n + 2 * p for n, p in zip(shape, pads)])


class GuardTouched(AssertionError):
    pass


class Guards:
    """The parents of one call.  ``snapshot()`` keeps every parent's bytes; ``check()`` raises GuardTouched with the argument's
    name and the first byte offset that differs outside the view."""

    def __init__(self):
        self.items = []          # (name, parent, byte mask of the view)
        self.before = None

    def add(self, name, parent, mask):
        bm = mask.reshape(-1, 1).expand(-1, parent.element_size()).reshape(-1)
        self.items.append((name, parent, bm))

    @staticmethod
    def _bytes(parent):
        return parent.reshape(-1).view(torch.uint8)

    def snapshot(self):
        self.before = [self._bytes(p).clone() for _, p, _ in self.items]

    def check(self):
        assert self.before is not None, "snapshot() first"
        for (name, parent, bm), was in zip(self.items, self.before):
            touched = (self._bytes(parent) != was) & ~bm
            if bool(touched.any()):
                off = int(touched.nonzero()[0, 0])
                raise GuardTouched(f"{name}: byte {off} of the parent (element {off // parent.element_size()}, parent shape "
                                   f"{tuple(parent.shape)}) lies outside the view and changed")


class BitMismatch(AssertionError):
    pass


def assert_same_bits(got, want, name):
    if got.shape != want.shape or got.dtype != want.dtype:
        raise BitMismatch(f"{name}: {tuple(got.shape)} {got.dtype} from the strided call, {tuple(want.shape)} {want.dtype} from the contiguous one")
    a, b = bits(got), bits(want)
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1).nonzero()
        raise BitMismatch(f"{name}: {bad.numel()} of {a.numel()} elements differ between the strided and the contiguous call, "
                          f"first at flat index {int(bad[0, 0])}")


def _flatten(x, prefix, out):
    if x is None:
        return
    if isinstance(x, torch.Tensor):
        out.append((prefix, x))
    elif isinstance(x, (list, tuple)):
        for i, y in enumerate(x):
            _flatten(y, f"{prefix}[{i}]", out)
    else:
        raise TypeError(f"{prefix}: a call returns tensors (or lists of them), got {type(x)}")


class Case:
    """One call, run twice.  ``arg(name, t, pads)`` registers a tensor argument with its initial contents (inputs: the values;
    outputs: what the buffer holds before the call — the same in both runs); ``run(fn)`` calls ``fn(a)`` with a namespace of fresh
    contiguous clones, then with the padded views, and asserts bit identity of every argument after the call and of whatever fn
    returns, and untouched guards.  ``pads``: see ``padded``; None = a plain clone in both runs (no parent)."""

    def __init__(self):
        self.specs = []
        self.exposed = {}

    def arg(self, name, t, pads, guard=None):
        """``pads``: an entry of a PADS table — (pads per dimension, exposed dimensions) —, bare pads, "flat" or None."""
        dims = ()
        if isinstance(pads, tuple) and len(pads) == 2 and isinstance(pads[0], tuple):
            pads, dims = pads
        self.specs.append((name, t, pads, guard))
        self.exposed[name] = dims
        return self

    def stride_problems(self):
        """What ``distinct_strides`` finds in this call's own shapes (empty = every exposed stride is distinct and moved)."""
        return distinct_strides({n: (tuple(t.shape), p, self.exposed[n]) for n, t, p, _ in self.specs
                                 if p is not None and not isinstance(p, str)})

    def run(self, fn, sync=None):
        sync = sync or (torch.cuda.synchronize if any(t.is_cuda for _, t, _, _ in self.specs) else (lambda: None))
        problems = self.stride_problems()
        assert not problems, problems
        a_c = types.SimpleNamespace(strided=False, **{n: t.clone() for n, t, _, _ in self.specs})
        r_c = fn(a_c)
        sync()
        guards, views = Guards(), {}
        for n, t, p, g in self.specs:
            if p is None:
                views[n] = t.clone()
                continue
            v, parent, mask = padded(t, p, g)
            guards.add(n, parent, mask)
            views[n] = v
        sync()
        guards.snapshot()
        a_s = types.SimpleNamespace(strided=True, **views)
        r_s = fn(a_s)
        sync()
        guards.check()
        for n, _, _, _ in self.specs:
            assert_same_bits(getattr(a_s, n), getattr(a_c, n), n)
        fc, fs = [], []
        _flatten(r_c, "returned", fc)
        _flatten(r_s, "returned", fs)
        assert len(fc) == len(fs)
        for (n, x), (_, y) in zip(fc, fs):
            assert_same_bits(y, x, n)
        return a_c, r_c


def distinct_strides(table):
    """Problems of a pad table {arg: (shape, pads, exposed dims)} as a list of strings: an exposed stride that equals its contiguous
    value, or two exposed strides of one call that coincide.  Empty = the table does what the issue asks of it."""
    seen, bad = {}, []
    for name, (shape, pads, dims) in table.items():
        got, dense = padded_strides(shape, pads), contiguous_strides(shape)
        for dim in dims:
            if got[dim] == dense[dim]:
                bad.append(f"{name}: stride of dim {dim} is its contiguous value {dense[dim]}")
            if got[dim] in seen:
                bad.append(f"{name} dim {dim} and {seen[got[dim]]} share the stride {got[dim]}")
            seen[got[dim]] = f"{name} dim {dim}"
        for dim in dims:  
            if dim + 1 < len(pads) and all(q == 0 for q in pads[dim + 1:]):
                bad.append(f"{name}: no pad behind dim {dim}")
        for p in pads[1:]:
            if p > 2 and p % 8:
                bad.append(f"{name}: pad {p} is no multiple of 8 elements (16 bytes at 16 bits)")
    return bad


# ------------------------------------------------------------------------------------------------
# include/spatten.h: every stride it declares, keyed by entry point or struct
# ------------------------------------------------------------------------------------------------
_STRIDE_NAME = re.compile(r"^(?:[a-z0-9_]+_)?s[a-z]$")


def header_strides(path: str = HEADER):
    """{(entry point or struct, name)} of every int64_t parameter / field whose name ends in ``_s<letter>`` (q_sb, w_sn, idx_sr,
    key_scratch_sh ...) or IS ``s<letter>`` (spatten_importance's sb / sh / sq)."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    found = set()
    for m in re.finditer(r"typedef\s+struct\s+(spatten_\w+)\s*\{(.*?)\}", src, flags=re.S):
        for stmt in m.group(2).split(";"):
            d = re.match(r"\s*int64_t\s+([^*]+)$", stmt, flags=re.S)
            if d:
                for name in d.group(1).split(","):
                    if _STRIDE_NAME.match(name.strip()):
                        found.add((m.group(1), name.strip()))
    for m in re.finditer(r"\b(?:int|size_t)\s+(spatten_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        for par in m.group(2).split(","):
            d = re.match(r"\s*int64_t\s+(\w+)\s*$", par, flags=re.S)
            if d and _STRIDE_NAME.match(d.group(1)):
                found.add((m.group(1), d.group(1)))
    return found


# ------------------------------------------------------------------------------------------------
# Pad tables: {argument: (pads per dimension, dimensions whose stride the ABI exposes)}.  Every pad is a multiple of 8 elements
# (16 bytes at 16 bits) where it moves a stride, 1 or 2 where it is only the guard of an outer dimension; within a family the
# exposed strides come out pairwise distinct and away from their contiguous values (asserted on NOMINAL below, and again by
# Case.run on the shapes of the call).  Plane pads are in bytes (uint8 tensors).
# ------------------------------------------------------------------------------------------------
PADS = {
    "decode": {
        "q": ((1, 1, 8), (0, 1)), "k_new": ((1, 1, 16), (0, 1)), "v_new": ((1, 1, 16), ()),
        "K": ((1, 1, 64, 0), (0, 1)), "Kr": ((1, 1, 64, 0), ()), "V": ((1, 1, 64, 0), ()),
        "mask": ((1, 24), (0,)), "pos": ((1, 1), (0,)), "out": ((1, 32), (0,)),
        "scores": ((1, 2, 40), (0, 1)), "prev": ((1, 1, 24), (0, 1)), "acc": ((1, 16), (0,)),
        "W": ((1, 8), (0,)), "y": ((1, 40), (0,)),
    },
    "planes": {
        "q": ((1, 1, 8), (0, 1)), "k_new": ((1, 1, 16), (0, 1)), "v_new": ((1, 1, 16), ()),
        "K": ((1, 1, 64, 0), (0, 1)), "Kr": ((1, 1, 64, 0), ()), "V": ((1, 1, 64, 0), ()),
        "out": ((1, 32), (0,)), "scores": ((1, 2, 40), (0, 1)), "acc": ((1, 8), (0,)),
        "msb": ((1, 1, 16, 0), (0, 1)), "lsb": ((1, 1, 32, 0), (0, 1)), "vq": ((1, 1, 48, 0), (0, 1)),
        "scale": ((1, 1, 16), (0, 1)), "vscale": ((1, 1, 16), ()), "lg": ((1, 2, 24), (0, 1)),
        "q_int": ((1, 1, 24), (0, 1)),
    },
    "legacy_planes": {
        "q": ((1, 1, 8), (0, 1)), "k_new": ((1, 1, 16), (0, 1)), "v_new": ((1, 1, 16), ()),
        "K": ((1, 1, 64, 0), (0, 1)), "Kr": ((1, 1, 64, 0), ()), "V": ((1, 1, 64, 0), ()),
        "out": ((1, 32), (0,)), "scores": ((1, 2, 40), (0, 1)),
        "msb": ((1, 1, 16, 0), (0, 1)), "lsb": ((1, 1, 16, 0), ()), "scale": ((1, 1, 16), (0, 1)),
    },
    "append": {
        "k_new4": ((1, 1, 1, 8), (0, 1, 2)), "v_new4": ((1, 1, 1, 8), ()),
        "K": ((1, 1, 64, 0), (0, 1)), "Kr": ((1, 1, 64, 0), ()), "V": ((1, 1, 64, 0), ()),
    },
    "rope": {"x": ((1, 1, 2, 8), (0, 1, 2)), "y": ((1, 2, 2, 16), (0, 1, 2)), "pos": ((1, 8), (0,))},
    "prefill": {
        "qp": ((1, 1, 1, 8), (0, 1, 2)), "K": ((1, 1, 64, 0), (0, 1)), "Kr": ((1, 1, 64, 0), ()), "V": ((1, 1, 64, 0), ()),
        "mask": ((1, 1, 8), (0, 1)), "out": ((1, 1, 16), (0, 1)), "stash": ((1, 1, 1, 24), (0, 1, 2)), "pos": ((1, 8), (0,)),
        "acc": ((1, 16), (0,)), "msb": ((1, 1, 16, 0), (0, 1)), "lsb": ((1, 1, 16, 0), ()), "scale": ((1, 1, 16), (0, 1)),
    },
    "importance": {
        "stash": ((1, 1, 1, 8), (0, 1, 2)), "mask": ((1, 1, 16), (0, 1)), "acc": ((1, 32), (0,)), "imp": ((1, 24), (0,)),
        "stash3": ((1, 2, 40), (0, 1)), "mask2": ((1, 40), (0,)), "V": ((1, 1, 64, 0), (0, 1)), "idx": ((1, 32), (0,)),
        "out": ((1, 32), (0,)), "out3": ((1, 1, 16), (0, 1)),
    },
    "prune": {
        "score": ((1, 8), (0,)), "idx": ((1, 8), (0,)), "Ks": ((1, 1, 16, 0), (0, 1)), "Vs": ((1, 1, 16, 0), ()),
        "Kd": ((1, 1, 24, 0), (0, 1)), "Vd": ((1, 1, 24, 0), ()), "Krd": ((1, 1, 24, 0), ()),
        "acc": ((1, 16), (0,)), "acc_dst": ((1, 40), (0,)), "ids": ((1, 48), (0,)), "prev_ids": ((1, 32), (0,)),
        "rank": ((1, 56), (0,)),
    },
    "gemv": {"x": ((1, 8), (0,)), "W": ((1, 16), (0,)), "y": ((1, 24), (0,))},
}

# the shapes the GPU file uses (B 2, H 4, Hkv 2, d 128 ...), for the table check that needs no GPU
_B, _H, _G, _D, _CAP = 2, 4, 2, 128, 512
NOMINAL = {
    "decode": {"q": (_B, _H, _D), "k_new": (_B, _G, _D), "v_new": (_B, _G, _D), "K": (_B, _G, _CAP, _D), "Kr": (_B, _G, _CAP, _D),
               "V": (_B, _G, _CAP, _D), "mask": (_B, 333), "pos": (_B, 1), "out": (_B, _H * _D), "scores": (_B, _H, _CAP),
               "prev": (_B, _H, _CAP), "acc": (_H, _CAP), "W": (_H * _D + 24, _H * _D), "y": (_B, _H * _D + 24)},
    "planes": {"q": (_B, _H, _D), "k_new": (_B, _G, _D), "v_new": (_B, _G, _D), "K": (_B, _G, _CAP, _D), "Kr": (_B, _G, _CAP, _D),
               "V": (_B, _G, _CAP, _D), "out": (_B, _H * _D), "scores": (_B, _H, _CAP), "acc": (_H, _CAP),
               "msb": (_B, _G, _CAP, _D), "lsb": (_B, _G, _CAP, _D // 2), "vq": (_B, _G, _CAP, _D), "scale": (_B, _G, _CAP),
               "vscale": (_B, _G, _CAP), "lg": (_B, _H, _CAP), "q_int": (_B, _H, _D)},
    "legacy_planes": {"q": (_B, _H, _D), "k_new": (_B, _G, _D), "v_new": (_B, _G, _D), "K": (_B, _G, _CAP, _D),
                      "Kr": (_B, _G, _CAP, _D), "V": (_B, _G, _CAP, _D), "out": (_B, _H * _D), "scores": (_B, _H, _CAP),
                      "msb": (_B, _G, _CAP, _D // 2), "lsb": (_B, _G, _CAP, _D // 2), "scale": (_B, _G, _CAP)},
    "append": {"k_new4": (_B, 5, _G, _D), "v_new4": (_B, 5, _G, _D), "K": (_B, _G, _CAP, _D), "Kr": (_B, _G, _CAP, _D),
               "V": (_B, _G, _CAP, _D)},
    "rope": {"x": (_B, _H, 7, _D), "y": (_B, _H, 7, _D), "pos": (_B, 7)},
    "prefill": {"qp": (_B, 130, _H, _D), "K": (_B, _G, 256, _D), "Kr": (_B, _G, 256, _D), "V": (_B, _G, 256, _D),
                "mask": (_B, 130, 207), "out": (_B, 130, _H * _D), "stash": (_B, _H, 130, 207), "pos": (_B, 130), "acc": (_H, 207),
                "msb": (_B, _G, 256, _D // 2), "lsb": (_B, _G, 256, _D // 2), "scale": (_B, _G, 256)},
    "importance": {"stash": (_B, _H, 9, 300), "mask": (_B, 9, 300), "acc": (_H, 300), "imp": (_H, 300), "stash3": (_B, _H, 384),
                   "mask2": (_B, 300), "V": (_B, _G, 384, _D), "idx": (_B * _H, 90), "out": (_B, _H * _D), "out3": (_B, 9, _H * _D)},
    "prune": {"score": (_H, 96), "idx": (_H, 16), "Ks": (_B, _H, 96, 64), "Vs": (_B, _H, 96, 64), "Kd": (_B, _H, 64, 64),
              "Vd": (_B, _H, 64, 64), "Krd": (_B, _H, 64, 64), "acc": (_H, 96), "acc_dst": (_H, 64), "ids": (_H, 96),
              "prev_ids": (_H, 24), "rank": (_H, 96)},
    "gemv": {"x": (2, 520), "W": (37, 520), "y": (2, 37)},
}


def pad_table(family):
    """{arg: (nominal shape, pads, exposed dims)} — the input of ``distinct_strides``."""
    return {n: (NOMINAL[family][n], p, dims) for n, (p, dims) in PADS[family].items()}


# ------------------------------------------------------------------------------------------------
# The ledger: every (entry point or struct, stride) of the header is either exercised by a test of
# tests/test_gpu_strided_views.py or listed with the reason why not.  tests/test_strided_views_cpu.py asserts the partition.
# ------------------------------------------------------------------------------------------------
def _rows(entry, names, value):
    return {(entry, n): value for n in names.split()}


COVERED = {
    **_rows("spatten_decode_args", "q_sb q_sh kv_sb kv_sh new_sb new_sh pos_sb mask_sb out_sb sc_sb sc_sh prev_sb prev_sh acc_sh "
                                   "proj_w_sn proj_out_sb", "test_plain_decode_step"),
    **_rows("spatten_decode_args", "pq_pl_sb pq_pl_sh pq_sc_sb pq_sc_sh", "test_legacy_planes"),
    **_rows("spatten_chain_args", "kv_sb kv_sh new_sb new_sh out_sb sc_sb sc_sh", "test_chained_decode"),
    **_rows("spatten_attn_decode_local_v", "q_sb q_sh kv_sb kv_sh out_sb sc_sb sc_sh", "test_local_v"),
    **_rows("spatten_attn_decode_local_v_append", "q_sb q_sh new_sb new_sh kv_sb kv_sh out_sb sc_sb sc_sh", "test_local_v"),
    **_rows("spatten_pq_planes", "km_sb km_sh kl_sb kl_sh vq_sb vq_sh sc_sb sc_sh lg_sb lg_sh", "test_profiled_planes"),
    **_rows("spatten_pq_pack_planes", "kv_sb kv_sh", "test_profiled_planes"),
    **_rows("spatten_kv_append_planes", "new_sb new_sh kv_sb kv_sh", "test_profiled_planes"),
    **_rows("spatten_pq_decode_args", "q_sb q_sh out_sb sc_sb sc_sh new_sb new_sh kv_sb kv_sh", "test_profiled_planes"),
    **_rows("spatten_pq_cascade_args", "acc_sh", "test_profiled_planes"),
    **_rows("spatten_pq_qint_args", "qi_sb qi_sh", "test_profiled_planes"),
    **_rows("spatten_pq_pack", "kv_sb kv_sh pl_sb pl_sh sc_sb sc_sh", "test_legacy_planes"),
    **_rows("spatten_kv_append_step", "pl_sb pl_sh sc_sb sc_sh", "test_legacy_planes"),
    **_rows("spatten_kv_append_step", "new_sb new_sh kv_sb kv_sh", "test_append_and_rotation"),
    **_rows("spatten_kv_append", "new_sb new_sh new_sn kv_sb kv_sh", "test_append_and_rotation"),
    **_rows("spatten_rope_single", "x_sb x_sh x_sn y_sb y_sh y_sn pos_sb", "test_append_and_rotation"),
    **_rows("spatten_attn_prefill", "q_sb q_sh q_sq kv_sb kv_sh pos_sb mask_sb mask_sq out_sb out_sq sc_sb sc_sh sc_sq", "test_prefill"),
    **_rows("spatten_attn_prefill_pq", "q_sb q_sh q_sq pl_sb pl_sh sc_sb sc_sh kv_sb kv_sh pos_sb mask_sb mask_sq out_sb out_sq",
            "test_prefill"),
    **_rows("spatten_importance_accumulate_prefill", "q_sb q_sh q_sq kv_sb kv_sh pos_sb acc_sh", "test_prefill"),
    **_rows("spatten_importance", "sb sh sq out_sh", "test_importance_and_gather"),
    **_rows("spatten_row_lse", "sb sh sq mask_sb mask_sq", "test_importance_and_gather"),
    **_rows("spatten_importance_accumulate", "sb sh sq mask_sb mask_sq acc_sh", "test_importance_and_gather"),
    **_rows("spatten_head_scores", "out_sb out_sq", "test_importance_and_gather"),
    **_rows("spatten_pv_gather", "sc_sb sc_sh mask_sb kv_sb kv_sh idx_sr out_sb", "test_importance_and_gather"),
    **_rows("spatten_topk_select", "score_sh idx_sh", "test_prune"),
    **_rows("spatten_kv_compact", "src_sb src_sh dst_sb dst_sh idx_sh", "test_prune"),
    **_rows("spatten_importance_compact", "src_sh dst_sh idx_sh", "test_prune"),
    **_rows("spatten_cascade_rank", "score_sh ids_sh prev_sh rank_sh", "test_prune"),
    **_rows("spatten_prune_layers_scored", "score_sh src_sb src_sh dst_sb dst_sh acc_src_sh acc_dst_sh", "test_prune"),
    **_rows("spatten_gemv", "x_sm w_sn y_sm", "test_gemv"),
}

NOT_COVERED = {
    **_rows("spatten_attn_decode", "q_sb q_sh kv_sb kv_sh new_sb new_sh pos_sb mask_sb out_sb sc_sb sc_sh",
            "the positional form copies its arguments into the block spatten_attn_decode_args takes; no ops front end calls it"),
    **_rows("spatten_decode_args", "qkv_w_sn", "the fused q/k/v projection step is out of this issue's scope"),
    **_rows("spatten_prune_layers", "score_sh src_sb src_sh dst_sb dst_sh",
            "forwards to spatten_prune_layers_scored, which ops.prune_layers calls and test_prune covers"),
    **_rows("spatten_pq_local_v_args", "acc_sh", "the composed PQ + local-V step is not on this issue's list of entry points; its "
                                                 "step block is spatten_pq_decode_args, covered through attn_decode_pqv"),
    **_rows("spatten_prune_layer_cascade", "key_scratch_sh", "the layer-cascade event is out of this issue's scope (its per-layer strides "
                                                             "travel in a table the header documents in prose)"),
}
