"""spatten_decode_gqa_form (include/spatten.h): would THIS argument block run in the matrix-core grouped-query form?  Host
arithmetic on the block — the eligibility routine the launch itself goes by (csrc/decode_gqa.hip decode_gqa_plan) — so it answers
on a machine without a GPU: the pointers below are never dereferenced."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from spatten_amd import _lib
    return _lib.load()


def _dtype_codes():
    text = open(os.path.join(ROOT, "include", "spatten.h")).read()
    return {n: int(v) for n, v in re.findall(r"\b(SPATTEN_(?:F32|F16|BF16))\s*=\s*(\d+)", text)}


def _block(dtype, heads=32, kv_heads=8, d=128, kv_len=600, batch=1, cascade=False):
    """A single-row appending step the way ops.attn_decode fills it; every pointer is a 16-byte aligned dummy."""
    from spatten_amd._lib import DecodeArgs
    a = DecodeArgs()
    a.struct_size = ctypes.sizeof(DecodeArgs)
    a.dtype = dtype
    cap = 1024
    a.q, a.q_sb, a.q_sh = 0x10000, heads * d, d
    a.k_cache, a.kr_cache, a.v_cache = 0x20000, 0x30000, 0x40000
    a.kv_sb, a.kv_sh = kv_heads * cap * d, cap * d
    a.k_new, a.v_new, a.new_sb, a.new_sh = 0x50000, 0x60000, kv_heads * d, d
    a.cos, a.sin, a.table_rows = 0x70000, 0x80000, cap
    a.out, a.out_sb = 0x90000, heads * d
    a.scores, a.sc_sb, a.sc_sh = 0xA0000, heads * cap, cap
    a.lse = 0xB0000
    a.workspace, a.workspace_splits = 0xC0000, 64
    a.batch, a.heads, a.kv_heads, a.head_dim, a.kv_len, a.pos_q, a.n_splits = batch, heads, kv_heads, d, kv_len, kv_len - 1, 0
    if cascade:
        a.importance_acc, a.acc_sh = 0xD0000, cap
        a.prev_scores, a.prev_sb, a.prev_sh = 0xE0000, heads * cap, cap
        a.prev_lse, a.prev_len = 0xF0000, kv_len - 1
    return a


def test_the_predicate_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spatten.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+spatten_decode_gqa_form\s*\(\s*const\s+spatten_decode_args_t\s*\*", text)
    lib = _lib()
    assert hasattr(lib, "spatten_decode_gqa_form")
    assert lib.spatten_decode_gqa_form.restype is ctypes.c_int and len(lib.spatten_decode_gqa_form.argtypes) == 1
    from spatten_amd import ops
    assert callable(ops.decode_gqa_form)
    lib.spatten_abi_version.restype = ctypes.c_int
    assert lib.spatten_abi_version() == 5          # a new symbol, no struct change


def test_the_predicate_follows_the_eligibility_of_the_launch():
    from spatten_amd import ops
    from spatten_amd._lib import DecodeArgs
    lib = _lib()
    codes = _dtype_codes()
    bf16, f16, f32 = codes["SPATTEN_BF16"], codes["SPATTEN_F16"], codes["SPATTEN_F32"]
    form = lambda a: lib.spatten_decode_gqa_form(ctypes.byref(a))
    prev = ops.set_decode_gqa(1)
    try:
        assert form(_block(bf16)) == 1                                   # 32 / 8 heads, d = 128, single row, no accumulation
        assert form(_block(bf16, cascade=True)) == 1                     # ... with importance_acc / prev_scores / prev_lse / prev_len
        assert form(_block(f16, cascade=True)) == 1
        for cascade in (False, True):
            a = _block(bf16, cascade=cascade); a.mask, a.mask_sb = 0x100000, 1024
            assert form(a) == 0, "mask"
            a = _block(bf16, cascade=cascade); a.head_ids, a.n_active_heads = 0x100000, 8
            assert form(a) == 0, "head_ids"
            a = _block(bf16, cascade=cascade); a.head_abs_acc = 0x100000
            assert form(a) == 0, "head_abs_acc"
            a = _block(bf16, cascade=cascade)
            a.pq_msb, a.pq_lsb, a.pq_scale, a.pq_need_lsb = 0x100000, 0x110000, 0x120000, 0x130000
            assert form(a) == 0, "pq_msb"
            assert form(_block(f32, cascade=cascade)) == 0, "fp32"
            assert form(_block(bf16, d=64, cascade=cascade)) == 0, "d = 64"
            assert form(_block(bf16, heads=8, kv_heads=8, cascade=cascade)) == 0, "heads == kv_heads"
            a = _block(bf16, cascade=cascade); a.struct_size = ctypes.sizeof(DecodeArgs) - 8
            assert form(a) == 0, "short struct_size"
        # previous stash rows the 16-byte LDS-DMA pieces cannot fetch: the step takes the per-query-head kernel
        a = _block(bf16, cascade=True); a.prev_scores = 0xE0008
        assert form(a) == 0
        a = _block(bf16, cascade=True); a.prev_sh = 1023
        assert form(a) == 0
        assert lib.spatten_decode_gqa_form(None) == 0
        ops.set_decode_gqa(0)
        assert form(_block(bf16)) == 0 and form(_block(bf16, cascade=True)) == 0
        # default mode: the plain step by the fitted rule (layout length), accumulation steps stay on the per-query-head kernel
        ops.set_decode_gqa(-1)
        long = _block(bf16, kv_len=1000)
        long.kv_len_layout = 16384
        assert form(long) == ops.decode_gqa_selected(__import__("torch").bfloat16, 1, 32, 8, 128, 16384) == 1
        longc = _block(bf16, kv_len=1000, cascade=True)
        longc.kv_len_layout = 16384
        assert form(longc) == 0
    finally:
        ops.set_decode_gqa(prev)
