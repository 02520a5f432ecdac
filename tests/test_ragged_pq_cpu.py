"""One step state per sequence over the profiled planes (spatten_pq_decode_args_t::step_state_sb, include/spatten.h): the field's
place in the argument block and what the entry points answer for strided blocks — host arithmetic in pq_validate, before the first
HIP call.  No GPU: only refused blocks are submitted, the pointers below are never dereferenced."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


def _codes():
    text = open(os.path.join(ROOT, "include", "spatten.h")).read()
    dts = {n: int(v) for n, v in re.findall(r"\b(SPATTEN_(?:F32|F16|BF16))\s*=\s*(\d+)", text)}
    errs = {n: int(v) for n, v in re.findall(r"\b(SPATTEN_ERR_(?:INVALID|UNSUPPORTED))\s*=\s*(-?\d+)", text)}
    return dts, errs


def test_status_codes_are_the_headers():
    _, errs = _codes()
    assert errs == {"SPATTEN_ERR_INVALID": INVALID, "SPATTEN_ERR_UNSUPPORTED": UNSUPPORTED}


def test_step_state_sb_sits_where_the_pad_word_sat(tmp_path):
    """The renamed pad word: same offset in the header (gcc's offsetof) and in the ctypes mirror, the int32 right behind
    n_active_heads and in front of head_abs_acc; the block keeps its size, the ABI version stays 5."""
    from spatten_amd import _lib
    from spatten_amd._lib import PQDecodeArgs
    fields = [f[0] for f in PQDecodeArgs._fields_]
    assert "step_state_sb" in fields and "pad0_" not in fields
    assert fields[fields.index("step_state_sb") - 1] == "n_active_heads"
    assert fields[fields.index("step_state_sb") + 1] == "head_abs_acc"
    t = "spatten_pq_decode_args_t"
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu", '
            f"sizeof({t}), offsetof({t}, n_active_heads), offsetof({t}, step_state_sb), offsetof({t}, head_abs_acc), "
            f"sizeof((({t}*)0)->step_state_sb), offsetof({t}, head_ids));return 0;}}")
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_na, off_sb, off_habs, width, off_ids = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert width == 4 and off_sb == off_na + 4 and off_habs == off_sb + 4
    # where pad0_ sat: the second int32 behind the 8-byte head_ids pointer
    assert off_sb == off_ids + 12
    assert off_sb == PQDecodeArgs.step_state_sb.offset and PQDecodeArgs.step_state_sb.size == 4
    assert off_na == PQDecodeArgs.n_active_heads.offset and off_habs == PQDecodeArgs.head_abs_acc.offset
    assert size == ctypes.sizeof(PQDecodeArgs)
    assert _lib.load().spatten_abi_version() == 5


B, HEADS, KV_HEADS, D, CAP = 2, 8, 2, 128, 704


def _planes(kb=8, vb=8):
    from spatten_amd._lib import PQPlanesDesc
    p = PQPlanesDesc()
    p.struct_size = ctypes.sizeof(PQPlanesDesc)
    p.key_msb_bits, p.value_bits = kb, vb
    p.key_msb, p.key_lsb, p.key_scale, p.val_q, p.val_scale, p.msb_logit = 0x200000, 0x210000, 0x220000, 0x230000, 0x240000, 0x250000
    p.km_sb, p.km_sh = KV_HEADS * CAP * D * kb // 8, CAP * D * kb // 8
    p.kl_sb, p.kl_sh = KV_HEADS * CAP * D // 2, CAP * D // 2
    p.vq_sb, p.vq_sh = KV_HEADS * CAP * D * vb // 8, CAP * D * vb // 8
    p.sc_sb, p.sc_sh = KV_HEADS * CAP, CAP
    p.lg_sb, p.lg_sh = HEADS * CAP, CAP
    return p


def _fill(a, planes, dtype, stride, step=0x140000):
    """bf16, B = 2, 8 / 2 heads, d = 128, bound 704: a device-length step the way ops.attn_decode_pqv fills it."""
    from spatten_amd._lib import PQDecodeArgs
    a.struct_size = ctypes.sizeof(PQDecodeArgs)
    a.dtype = dtype
    a.q, a.q_sb, a.q_sh = 0x10000, HEADS * D, D
    a.planes = ctypes.pointer(planes)
    a.cos, a.sin, a.table_rows, a.pos_q = 0x70000, 0x80000, 720, 0
    a.out, a.out_sb = 0x90000, HEADS * D
    a.scores, a.sc_sb, a.sc_sh = 0xA0000, HEADS * CAP, CAP
    a.lse = 0xB0000
    a.need_lsb, a.threshold = 0x150000, 0.5
    a.workspace, a.workspace_splits = 0xC0000, 64
    a.batch, a.heads, a.kv_heads, a.head_dim, a.kv_len = B, HEADS, KV_HEADS, D, CAP
    a.step_state = step
    a.step_state_sb = stride
    return a


def _state_bytes(lib, dtype):
    lib.spatten_step_state_bytes.restype = ctypes.c_size_t
    state = lib.spatten_step_state_bytes(dtype, D)
    assert state >= 64 + 4 * 64 * 2 and state % 256 == 0
    return int(state)


def _bad_strides(state):
    return [(100, 0x140000), (256, 0x140000), (state - 256, 0x140000), (-state, 0x140000), (state, None)]


def test_decode_pq_refuses_invalid_strides():
    from spatten_amd import _lib
    lib = _lib.load()
    bf16 = _codes()[0]["SPATTEN_BF16"]
    state = _state_bytes(lib, bf16)
    planes = _planes()
    for stride, step in _bad_strides(state):
        a = _fill(_lib.PQDecodeArgs(), planes, bf16, stride, step)
        assert lib.spatten_attn_decode_pq(ctypes.byref(a), None) == INVALID, (stride, step)
    # ... at every batch size
    a = _fill(_lib.PQDecodeArgs(), planes, bf16, 100)
    a.batch = 1
    assert lib.spatten_attn_decode_pq(ctypes.byref(a), None) == INVALID
    # the quantised-query entry point goes by the same rule
    for stride, step in _bad_strides(state):
        qa = _lib.PQQintArgs()
        qa.struct_size, qa.query_bits = ctypes.sizeof(_lib.PQQintArgs), 8
        _fill(qa.step, planes, bf16, stride, step)
        qa.q_int, qa.qi_sb, qa.qi_sh, qa.q_scale = 0x160000, HEADS * D, D, 0x170000
        assert lib.spatten_attn_decode_pq_qint(ctypes.byref(qa), None) == INVALID, (stride, step)


def _append_ragged(lib, planes, dtype, step, stride, batch=B):
    return lib.spatten_kv_append_planes_ragged(dtype, 0x50000, 0x60000, KV_HEADS * D, D, 0x20000, 0x30000, 0x40000,
                                               KV_HEADS * CAP * D, CAP * D, ctypes.byref(planes), 0x70000, 0x80000, 720, batch,
                                               KV_HEADS, D, 0, CAP, step, stride, None)


def test_append_planes_ragged_refuses_invalid_strides_and_a_missing_state():
    from spatten_amd import _lib
    lib = _lib.load()
    bf16 = _codes()[0]["SPATTEN_BF16"]
    state = _state_bytes(lib, bf16)
    planes = _planes()
    for stride, step in _bad_strides(state):
        assert _append_ragged(lib, planes, bf16, step, stride) == INVALID, (stride, step)
    assert _append_ragged(lib, planes, bf16, None, 0) == INVALID           # the ragged entry requires the state
    assert _append_ragged(lib, planes, bf16, 0x140000, 100, batch=1) == INVALID
    assert _append_ragged(lib, planes, bf16, 0x140000, (1 << 31) + 256) == INVALID   # beyond the decode block's int32 field


def test_cascade_local_v_and_grouped_forms_refuse_a_valid_stride():
    """SPATTEN_ERR_UNSUPPORTED before the first HIP call: these forms keep the one shared state (include/spatten.h)."""
    from spatten_amd import _lib
    lib = _lib.load()
    bf16 = _codes()[0]["SPATTEN_BF16"]
    state = _state_bytes(lib, bf16)
    planes = _planes()
    for stride in (state, 2 * state):
        ca = _lib.PQCascadeArgs()
        ca.struct_size, ca.prev_len = ctypes.sizeof(_lib.PQCascadeArgs), 0
        _fill(ca.step, planes, bf16, stride)
        ca.importance_acc, ca.acc_sh, ca.prev_lse = 0xD0000, CAP, 0xF0000
        assert lib.spatten_attn_decode_pq_cascade(ctypes.byref(ca), None) == UNSUPPORTED

        la = _lib.PQLocalVArgs()
        la.struct_size, la.keep, la.keep_fraction = ctypes.sizeof(_lib.PQLocalVArgs), 0, 0.5
        _fill(la.step, planes, bf16, stride)
        la.workspace, la.workspace_rows = 0x180000, CAP
        assert lib.spatten_attn_decode_pq_local_v(ctypes.byref(la), None) == UNSUPPORTED

        qa = _lib.PQQintArgs()
        qa.struct_size, qa.query_bits = ctypes.sizeof(_lib.PQQintArgs), 8
        _fill(qa.step, planes, bf16, stride)
        qa.q_int, qa.qi_sb, qa.qi_sh, qa.q_scale = 0x160000, HEADS * D, D, 0x170000
        assert lib.spatten_attn_decode_pq_qint_gqa(ctypes.byref(qa), None) == UNSUPPORTED
    # an invalid stride is invalid there too
    ca = _lib.PQCascadeArgs()
    ca.struct_size = ctypes.sizeof(_lib.PQCascadeArgs)
    _fill(ca.step, planes, bf16, 100)
    ca.importance_acc, ca.acc_sh, ca.prev_lse = 0xD0000, CAP, 0xF0000
    assert lib.spatten_attn_decode_pq_cascade(ctypes.byref(ca), None) == INVALID


def test_ops_refuses_batched_states_where_the_library_does():
    """The ops-level refusals that need no device: raised before any tensor is looked at."""
    import pytest
    from spatten_amd import ops

    class Batched:                       # what ops asks of a StepState(batch=B)
        batch, stride = 3, 768

    with pytest.raises(NotImplementedError, match="shared state"):
        ops.pq_pack_planes(None, None, None, 0, 1, step=Batched())
    with pytest.raises(NotImplementedError, match="kept count"):
        ops.attn_decode_pq_local_v(None, None, 8, None, None, 0, 0.5, 4, None, None, step=Batched())

    class Q:
        shape = (2, 8, 128)

    with pytest.raises(NotImplementedError, match="batch axis"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(None, None, 0), lse=0)
    with pytest.raises(NotImplementedError, match="grouped"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), query_bits=8, grouped=True)
    with pytest.raises(ValueError, match="3 sequences"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched())
