"""SPATTEN_DECODE_GROUPED_HEADS (include/spatten.h): the opt-in flag with which a head-pruning step — head_ids / n_active_heads
and / or head_abs_acc — may take the matrix-core grouped-query form.  spatten_decode_gqa_form answers by the launch's own
eligibility routine (csrc/decode_gqa.hip decode_gqa_plan), host arithmetic only: the pointers below are never dereferenced, so
this runs on a machine without a GPU."""
import ctypes
import os
import re

import pytest

from tests.test_gqa_cascade_cpu import ROOT, _block, _dtype_codes, _lib

SCORES_ONLY, GROUPED_HEADS = 1, 2


def _heads(a, ids=True, abs_=True, flag=True, n_active=24):
    if ids:
        a.head_ids, a.n_active_heads = 0x100000, n_active
    if abs_:
        a.head_abs_acc = 0x140000
    if flag:
        a.flags |= GROUPED_HEADS
    return a


@pytest.fixture
def env():
    from spatten_amd import ops
    lib = _lib()
    codes = _dtype_codes()
    prev = ops.set_decode_gqa(1)
    yield ops, (lambda a: lib.spatten_decode_gqa_form(ctypes.byref(a))), codes["SPATTEN_BF16"], codes["SPATTEN_F16"], codes["SPATTEN_F32"]
    ops.set_decode_gqa(prev)


def test_the_header_defines_the_flag_and_the_abi_stays():
    text = open(os.path.join(ROOT, "include", "spatten.h")).read()
    assert re.search(r"^#define\s+SPATTEN_DECODE_GROUPED_HEADS\s+2\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+SPATTEN_DECODE_SCORES_ONLY\s+1\s*$", text, flags=re.M)
    lib = _lib()
    lib.spatten_abi_version.restype = ctypes.c_int
    assert lib.spatten_abi_version() == 5          # no new symbol, no struct change


def test_without_the_flag_a_head_pruning_block_stays_per_query_head(env):
    ops, form, bf16, f16, f32 = env
    for cascade in (False, True):
        for ids, abs_ in ((True, False), (False, True), (True, True)):
            assert form(_heads(_block(bf16, cascade=cascade), ids, abs_, flag=False)) == 0, (cascade, ids, abs_)


def test_scores_only_and_mask_keep_a_flagged_block_out(env):
    ops, form, bf16, f16, f32 = env
    a = _heads(_block(bf16))
    a.flags |= SCORES_ONLY
    a.k_new = a.v_new = None                      # (what a scores-only call requires)
    assert form(a) == 0
    a = _block(bf16)
    a.flags = SCORES_ONLY | GROUPED_HEADS
    a.k_new = a.v_new = None
    assert form(a) == 0
    a = _heads(_block(bf16))
    a.mask, a.mask_sb = 0x180000, 1024
    assert form(a) == 0


def test_with_the_flag_the_grouped_form_serves_head_pruning(env):
    ops, form, bf16, f16, f32 = env
    for dt in (bf16, f16):
        for cascade in (False, True):
            for ids, abs_ in ((True, False), (False, True), (True, True)):
                assert form(_heads(_block(dt, cascade=cascade), ids, abs_)) == 1, (dt, cascade, ids, abs_)
    # ... with the device-length state too (any non-NULL pointer: nothing is dereferenced)
    for cascade in (False, True):
        a = _heads(_block(bf16, cascade=cascade))
        a.step_state, a.kv_len, a.pos_q = 0x1C0000, 1024, 0
        assert form(a) == 1, cascade
    # one listed head, every listed head
    assert form(_heads(_block(bf16), n_active=1)) == 1
    assert form(_heads(_block(bf16), n_active=32)) == 1


def test_the_flag_widens_nothing_else(env):
    ops, form, bf16, f16, f32 = env
    for cascade in (False, True):
        assert form(_heads(_block(f32, cascade=cascade))) == 0, "fp32"
        assert form(_heads(_block(bf16, d=64, cascade=cascade))) == 0, "d = 64"
        assert form(_heads(_block(bf16, heads=8, kv_heads=8, cascade=cascade), n_active=6)) == 0, "heads == kv_heads"
    a = _heads(_block(bf16))
    a.pq_msb, a.pq_lsb, a.pq_scale, a.pq_need_lsb = 0x200000, 0x210000, 0x220000, 0x230000
    a.k_new = a.v_new = None
    assert form(a) == 0, "quantised keys"
    assert form(_heads(_block(bf16), n_active=33)) == 0, "a list longer than the heads: the call rejects it"


def test_the_flag_alone_changes_nothing(env):
    ops, form, bf16, f16, f32 = env
    for cascade in (False, True):
        plain = _block(bf16, cascade=cascade)
        flagged = _heads(_block(bf16, cascade=cascade), ids=False, abs_=False)
        assert form(plain) == form(flagged) == 1
    assert form(_heads(_block(f32), ids=False, abs_=False)) == 0
    ops.set_decode_gqa(0)
    assert form(_heads(_block(bf16), ids=False, abs_=False)) == 0
    ops.set_decode_gqa(-1)
    long = _heads(_block(bf16, kv_len=1000), ids=False, abs_=False)
    long.kv_len_layout = 16384
    assert form(long) == 1
    short = _heads(_block(bf16, kv_len=600), ids=False, abs_=False)
    plain_short = _block(bf16, kv_len=600)
    assert form(short) == form(plain_short)


def test_modes_0_and_default_keep_a_flagged_head_list_per_query_head(env):
    ops, form, bf16, f16, f32 = env
    ops.set_decode_gqa(0)
    assert form(_heads(_block(bf16))) == 0
    ops.set_decode_gqa(-1)
    plain = _block(bf16, kv_len=1000)
    plain.kv_len_layout = 16384
    assert form(plain) == 1                       # the plain step of this layout takes the form by the fitted rule ...
    for ids, abs_ in ((True, False), (False, True), (True, True)):
        a = _heads(_block(bf16, kv_len=1000), ids, abs_)
        a.kv_len_layout = 16384
        assert form(a) == 0, (ids, abs_)          # ... a head-pruning step was never timed in both forms: mode 1 only


def test_the_keywords_exist_and_default_to_off():
    import inspect

    from spatten_amd import ops
    from spatten_amd.enable_spatten_llm import enable_spatten_llm
    from spatten_amd.extensions import SpattenExtensions
    assert inspect.signature(ops.attn_decode).parameters["grouped_heads"].default is False
    assert inspect.signature(enable_spatten_llm).parameters["grouped_head_pruning"].default is False
    assert inspect.signature(SpattenExtensions.__init__).parameters["grouped_head_pruning"].default is False


def _host_step(H=8, Hkv=2, N=300, cap=320, d=128):
    """The tensors of one appending step in HOST memory: the predicate never dereferences them."""
    import torch
    dt = torch.bfloat16
    z = lambda *s: torch.zeros(*s, dtype=dt)
    return dict(q=z(1, H, d), kc=z(1, Hkv, cap, d), krc=z(1, Hkv, cap, d), vc=z(1, Hkv, cap, d), cos=z(cap, d // 2), sin=z(cap, d // 2),
                kn=z(1, Hkv, d), vn=z(1, Hkv, d), out=z(1, H * d), stash=z(1, H, cap), lse=torch.zeros(1, H, 2),
                ids=torch.tensor([0, 1, 2, 5, 6], dtype=torch.int32), habs=torch.zeros(H), N=N)


def test_ops_attn_decode_puts_the_bit_into_the_block(monkeypatch):
    """ops.attn_decode(grouped_heads=True) assembles the block with SPATTEN_DECODE_GROUPED_HEADS set: read from the block the C
    predicate is handed, and through the predicate's answer (mode 1).  Host tensors, device checks patched out; nothing is launched."""
    import types

    import torch
    from spatten_amd import _lib as lib_mod, ops
    t = _host_step()
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    ws = types.SimpleNamespace(buf=torch.zeros(1 << 20, dtype=torch.uint8), max_splits=64)
    real = lib_mod.load()
    flags = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def spatten_decode_gqa_form(self, ref):
            flags.append(int(ref._obj.flags))
            return real.spatten_decode_gqa_form(ref)

    monkeypatch.setattr(lib_mod, "load", lambda: Spy())
    args = (t["q"], t["kc"], t["krc"], t["vc"], t["N"], t["cos"], t["sin"], t["N"] - 1)
    kw = dict(k_new=t["kn"], v_new=t["vn"], out=t["out"], scores=t["stash"], lse=t["lse"], workspace=ws, head_abs=t["habs"])
    prev = ops.set_decode_gqa(1)
    try:
        assert ops.decode_gqa_form(*args, **kw) is False and flags[-1] == 0
        assert ops.decode_gqa_form(*args, grouped_heads=True, **kw) is True and flags[-1] == GROUPED_HEADS
        assert ops.decode_gqa_form(*args, **dict(kw, head_abs=None)) is True and flags[-1] == 0
    finally:
        ops.set_decode_gqa(prev)


def test_the_extension_forwards_its_option_on_the_plain_step(monkeypatch):
    """SpattenExtensions(grouped_head_pruning=...) passes grouped_heads on the plain decode call (host lengths), together with the
    head importance accumulator the step carries from the first token on."""
    import types

    import torch
    from spatten_amd import ops
    from spatten_amd.extensions import SpattenExtensions
    t = _host_step()
    calls = []
    monkeypatch.setattr(ops, "attn_decode", lambda *a, **kw: calls.append(kw))
    slab = types.SimpleNamespace(k=t["kc"], kr=t["krc"], v=t["vc"], capacity=t["kc"].shape[2])
    for flag in (True, False):
        ext = SpattenExtensions(types.SimpleNamespace(important_size=64), 2, head_keep=6, grouped_head_pruning=flag)
        ext.decode_step(1, t["q"], t["kn"], t["vn"], slab, t["N"], t["N"] - 1, t["cos"], t["sin"])
        assert calls[-1]["grouped_heads"] is flag and calls[-1]["head_abs"] is not None
