"""One step state per sequence (spatten_decode_args_t::step_state_sb, include/spatten.h): the field's place in the argument block and
what spatten_decode_gqa_form — host arithmetic through decode_rows_check, the validation the launch itself goes by — answers for
strided blocks.  No GPU: the pointers below are never dereferenced."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dtype_codes():
    text = open(os.path.join(ROOT, "include", "spatten.h")).read()
    return {n: int(v) for n, v in re.findall(r"\b(SPATTEN_(?:F32|F16|BF16))\s*=\s*(\d+)", text)}


def test_step_state_sb_sits_directly_behind_kv_len_layout(tmp_path):
    """The renamed pad word: same offset in the header (gcc's offsetof) and in the ctypes mirror, the int32 right after
    kv_len_layout; the block keeps its size, the ABI version stays 5."""
    from spatten_amd import _lib
    from spatten_amd._lib import DecodeArgs
    fields = [f[0] for f in DecodeArgs._fields_]
    assert "step_state_sb" in fields and "pad3_" not in fields
    assert fields[fields.index("step_state_sb") - 1] == "kv_len_layout"
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu %zu %zu %zu %zu", '
            "sizeof(spatten_decode_args_t), offsetof(spatten_decode_args_t, kv_len_layout), offsetof(spatten_decode_args_t, step_state_sb), "
            "offsetof(spatten_decode_args_t, proj_weight), sizeof(((spatten_decode_args_t*)0)->step_state_sb));return 0;}")
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_lay, off_sb, off_proj, width = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert width == 4 and off_sb == off_lay + 4 and off_proj == off_sb + 4
    assert off_sb == DecodeArgs.step_state_sb.offset and DecodeArgs.step_state_sb.size == 4
    assert size == ctypes.sizeof(DecodeArgs)
    assert _lib.load().spatten_abi_version() == 5


def _block(dtype, stride, step=0x140000):
    """bf16, B = 2, 8 / 2 heads, d = 128, bound 704: an appending device-length step the way ops.attn_decode fills it."""
    from spatten_amd._lib import DecodeArgs
    B, heads, kv_heads, d, cap = 2, 8, 2, 128, 704
    a = DecodeArgs()
    a.struct_size = ctypes.sizeof(DecodeArgs)
    a.dtype = dtype
    a.q, a.q_sb, a.q_sh = 0x10000, heads * d, d
    a.k_cache, a.kr_cache, a.v_cache = 0x20000, 0x30000, 0x40000
    a.kv_sb, a.kv_sh = kv_heads * cap * d, cap * d
    a.k_new, a.v_new, a.new_sb, a.new_sh = 0x50000, 0x60000, kv_heads * d, d
    a.cos, a.sin, a.table_rows = 0x70000, 0x80000, 720
    a.out, a.out_sb = 0x90000, heads * d
    a.scores, a.sc_sb, a.sc_sh = 0xA0000, heads * cap, cap
    a.lse = 0xB0000
    a.workspace, a.workspace_splits = 0xC0000, 64
    a.batch, a.heads, a.kv_heads, a.head_dim, a.kv_len, a.pos_q, a.n_splits = B, heads, kv_heads, d, cap, 0, 0
    a.step_state = step
    a.step_state_sb = stride
    return a


def test_gqa_form_answers_for_strided_blocks():
    from spatten_amd import ops
    lib = ops._lib.load()
    bf16 = _dtype_codes()["SPATTEN_BF16"]
    lib.spatten_step_state_bytes.restype = ctypes.c_size_t
    state = lib.spatten_step_state_bytes(bf16, 128)
    assert state >= 64 + 4 * 64 * 2 and state % 256 == 0
    form = lambda a: lib.spatten_decode_gqa_form(ctypes.byref(a))
    prev = ops.set_decode_gqa(1)
    try:
        assert form(_block(bf16, state)) == 1                       # one state per sequence
        assert form(_block(bf16, 2 * state)) == 1                   # ... further apart
        assert form(_block(bf16, 0)) == 1                           # one state for the batch, as before
        assert form(_block(bf16, 100)) == 0                         # no multiple of 256
        assert form(_block(bf16, state - 256)) == 0                 # states would overlap
        assert form(_block(bf16, 256)) == 0
        assert form(_block(bf16, -int(state))) == 0
        assert form(_block(bf16, state, step=None)) == 0            # a stride without a state
        a = _block(bf16, state)
        a.importance_acc, a.acc_sh = 0xD0000, 704
        a.prev_scores, a.prev_sb, a.prev_sh, a.prev_lse = 0xE0000, 8 * 704, 704, 0xF0000
        assert form(a) == 0                                         # the accumulator [H, L] has no batch axis
        a.step_state_sb = 0
        assert form(a) == 1                                         # (the shared state admits it)
        a = _block(bf16, state)
        a.pq_msb, a.pq_lsb, a.pq_scale, a.pq_need_lsb = 0x100000, 0x110000, 0x120000, 0x130000
        assert form(a) == 0
    finally:
        ops.set_decode_gqa(prev)
