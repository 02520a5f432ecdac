"""The ledger and the harness of the strided-argument tests, without a GPU (tests/strided.py).

Ledger: COVERED and NOT_COVERED partition the strides include/spatten.h declares, and every COVERED row names a test that exists.
Harness: pure-torch stand-in ops that take explicit strides and address flat storage show that Guards.check() and the bit
comparison catch what they are for — and that the correct stand-in passes both."""
import ast
import os

import pytest
import torch

from tests import strided
from tests.strided import BitMismatch, Case, GuardTouched, Guards, padded

GPU_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_strided_views.py")


def test_ledger_partitions_the_header():
    declared = strided.header_strides()
    assert len(declared) > 150 and ("spatten_decode_args", "q_sb") in declared and ("spatten_importance", "sq") in declared \
        and ("spatten_gemv", "w_sn") in declared and ("spatten_pv_gather", "idx_sr") in declared \
        and ("spatten_prune_layer_cascade", "key_scratch_sh") in declared and ("spatten_pq_planes", "km_sb") in declared
    cov, ncov = set(strided.COVERED), set(strided.NOT_COVERED)
    assert not cov & ncov, sorted(cov & ncov)
    assert not declared - cov - ncov, f"strides the header declares and the ledger does not place: {sorted(declared - cov - ncov)}"
    assert not (cov | ncov) - declared, f"stale ledger rows: {sorted((cov | ncov) - declared)}"
    assert all(isinstance(r, str) and len(r) > 20 for r in strided.NOT_COVERED.values())


def test_every_covered_row_names_a_gpu_test():
    tree = ast.parse(open(GPU_FILE).read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    missing = {t for t in strided.COVERED.values() if t not in tests}
    assert not missing, missing
    assert tests == set(strided.COVERED.values()), "a family of the GPU file covers no ledger row"


@pytest.mark.parametrize("family", sorted(strided.PADS))
def test_pad_tables_give_distinct_strides(family):
    table = strided.pad_table(family)
    assert set(strided.NOMINAL[family]) == set(strided.PADS[family])
    assert strided.distinct_strides(table) == []
    for name, (shape, pads, dims) in table.items():
        assert pads[0] >= 1, f"{name}: no guard in front of and behind the outermost dimension"
        if len(shape) == 4 and pads[3] == 0 and name not in ("qp", "k_new4", "v_new4", "x", "y", "stash"):
            assert pads[2] > 0 and pads[1] >= 1            # a cache: pitch fixed, capacity and head padded


def test_distinct_strides_reports_what_it_should():
    assert strided.distinct_strides({"a": ((2, 4, 8), (1, 1, 0), (0, 1))})                        # head stride = its dense value
    assert strided.distinct_strides({"a": ((2, 4, 8), (1, 1, 8), (0, 1)), "b": ((2, 4, 8), (1, 1, 8), (0, 1))})   # shared
    assert strided.distinct_strides({"a": ((2, 4, 8), (1, 1, 5), (0, 1))})                        # 10 bytes of pad
    assert strided.distinct_strides({"a": ((2, 4, 8), (1, 1, 8), (0, 1)), "b": ((2, 4, 8), (1, 1, 16), (0, 1))}) == []


def test_padded_view_parent_and_mask():
    t = torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8).to(torch.bfloat16)
    v, parent, mask = padded(t, (1, 2, 8))
    assert v.shape == t.shape and torch.equal(v, t) and parent.shape == (4, 7, 24) and v.stride() == strided.padded_strides(t.shape, (1, 2, 8))
    assert v.stride() != t.stride() and v.data_ptr() % 16 == parent.data_ptr() % 16
    assert int(mask.sum()) == t.numel() and torch.isnan(parent[~mask].float()).all() and torch.equal(parent[mask].reshape(t.shape), t)
    one = torch.ones(1, 3, 8)
    v1, p1, _ = padded(one, (1, 1, 8))
    assert v1.stride() == (5 * 24, 24, 1) and p1.shape == (3, 5, 24)          # a dimension of size 1 keeps its real stride
    i = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    vi, pi, mi = padded(i, (1, 8))
    assert (pi[~mi] == 0x7FFFFFFF).all()
    u = torch.zeros(2, 4, dtype=torch.uint8)
    _, pu, mu = padded(u, (1, 16))
    assert (pu[~mu] == 0xFF).all()
    vf, pf, mf = padded(t, "flat")
    assert vf.is_contiguous() and pf.dim() == 1 and int(mf.sum()) == t.numel() and torch.equal(vf, t)


# ------------------------------------------------------------------------------------------------
# stand-in ops: out[b, h, j] = 2 x[b, h, j] + bias[h, j] (+ x[b, h, j + 1] in the form that reads a row too far), addressed
# through explicit strides on the flat storage, the way a kernel addresses device memory
# ------------------------------------------------------------------------------------------------
def _flat(t):
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def _standin(a, fault=None):
    x, o, w = a.x, a.out, a.bias
    B, H, n = x.shape
    fx, fo, fw = _flat(x), _flat(o), _flat(w)
    x_sb, x_sh = x.stride(0), x.stride(1)
    o_sb, o_sh = o.stride(0), o.stride(1)
    w_sh = w.stride(0)
    if fault == "swapped strides":
        x_sh, w_sh = w_sh, x_sh                    # x's head stride taken for the bias's and the other way round
    if fault == "head offset from the shape":
        x_sh = n                                   # h * n instead of h * x_sh
    b, h, j = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(n), indexing="ij")
    xi = x.storage_offset() + b * x_sb + h * x_sh + j
    val = 2 * fx[xi.clamp(max=fx.numel() - 1)] + fw[(w.storage_offset() + h * w_sh + j).clamp(max=fw.numel() - 1)]
    if fault == "reads one row past":
        val = val + 0 * fx[(xi + n).clamp(max=fx.numel() - 1)]          # 0 * NaN is NaN: a guard value reaches the result
    oi = o.storage_offset() + b * o_sb + h * o_sh + j
    stray = {"writes past the row": (b[:, :, :1], h[:, :, :1], n), "writes into the head slack": (b[:, :1, :], H, j[:, :1, :]),
             "writes into the batch slack": (B, h[:1], j[:1])}.get(fault)
    if stray is not None:                           # first, so that the real stores of a dense tensor cover what they can
        si = (o.storage_offset() + stray[0] * o_sb + stray[1] * o_sh + stray[2]).reshape(-1)
        si = si[si < fo.numel()]
        fo[si] = 42.0
    fo[oi.reshape(-1)] = val.reshape(-1).to(o.dtype)


def _case():
    g = torch.Generator().manual_seed(5)
    B, H, n = 2, 3, 16
    c = Case().arg("x", torch.randn(B, H, n, generator=g), ((1, 1, 8), (0, 1)))
    c.arg("bias", torch.randn(H, n, generator=g), ((1, 16), (0,))).arg("out", torch.full((B, H, n), 0.5), ((1, 2, 24), (0, 1)))
    return c


def test_correct_standin_passes_both_checks():
    a, _ = _case().run(_standin)
    assert torch.isfinite(a.out).all() and not (a.out == 0.5).any()


@pytest.mark.parametrize("fault", ["writes past the row", "writes into the head slack", "writes into the batch slack"])
def test_guards_catch_stray_writes(fault):
    with pytest.raises(GuardTouched, match="out: byte"):
        _case().run(lambda a: _standin(a, fault))


@pytest.mark.parametrize("fault", ["swapped strides", "head offset from the shape", "reads one row past"])
def test_bit_identity_catches_wrong_addresses(fault):
    with pytest.raises(BitMismatch, match="out: "):
        _case().run(lambda a: _standin(a, fault))
    # ... each of which the contiguous call alone cannot see: dense tensors give the fault the strides it assumes
    dense = _case()
    a = type("A", (), {n: t.clone() for n, t, _, _ in dense.specs})
    b = type("B", (), {n: t.clone() for n, t, _, _ in dense.specs})
    _standin(a)
    _standin(b, fault)
    assert torch.equal(a.out, b.out)


def test_guards_report_name_and_first_offset():
    t = torch.zeros(2, 4)
    v, parent, mask = padded(t, (1, 8))
    g = Guards()
    g.add("stash", parent, mask)
    g.snapshot()
    v.fill_(3.0)                                   # inside the view: allowed
    g.check()
    parent[1, 8 + 4] = 1.0                         # one element past the first row of the view
    with pytest.raises(GuardTouched, match=r"stash: byte %d " % ((20 + 12) * 4 + 2)):
        g.check()
