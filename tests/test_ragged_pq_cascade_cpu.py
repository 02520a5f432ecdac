"""The cascade step of a ragged batch over the profiled planes (spatten_attn_decode_pq_cascade_ragged, include/spatten.h): the
symbol, the argument block it shares with spatten_attn_decode_pq_cascade, and what the entry points and ops answer for refused
calls — host arithmetic, before the first HIP call.  No GPU: only refused blocks are submitted, the pointers below are never
dereferenced."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.test_ragged_pq_cpu import CAP, HEADS, INVALID, UNSUPPORTED, _bad_strides, _codes, _fill, _planes, _state_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "spatten_attn_decode_pq_cascade_ragged"
ACC_SB = HEADS * CAP


def _block(planes, dtype, stride, step=0x140000):
    from spatten_amd import _lib
    ca = _lib.PQCascadeArgs()
    ca.struct_size, ca.prev_len = ctypes.sizeof(_lib.PQCascadeArgs), 0
    _fill(ca.step, planes, dtype, stride, step)
    ca.importance_acc, ca.acc_sh, ca.prev_lse = 0xD0000, CAP, 0xF0000
    return ca


def test_symbol_is_declared_exported_and_typed():
    from spatten_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spatten.h")).read(), flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)", text)
    assert decl is not None, "not declared in include/spatten.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert params == ["const spatten_pq_cascade_args_t* args", "int64_t acc_batch_stride", "void* stream"]
    raw = ctypes.CDLL(os.path.join(ROOT, "spatten_amd", "lib", "libspatten_hip.so"))
    assert hasattr(raw, NAME), "not exported by the library"
    lib = _lib.load()
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.POINTER(_lib.PQCascadeArgs), ctypes.c_int64, ctypes.c_void_p]
    assert lib.spatten_abi_version() == 5


def test_cascade_block_keeps_its_layout(tmp_path):
    """The new entry point takes spatten_pq_cascade_args_t unchanged: the fields, the C compiler's size and offsets and the
    ctypes mirror agree, and the block is what the last ABI-5 header laid down (no field added behind prev_lse)."""
    from spatten_amd._lib import PQCascadeArgs, PQDecodeArgs
    fields = [f[0] for f in PQCascadeArgs._fields_]
    assert fields == ["struct_size", "prev_len", "step", "importance_acc", "acc_sh", "prev_lse"]
    t = "spatten_pq_cascade_args_t"
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu", sizeof(' + t + '));' + \
        "".join(f'printf(" %zu", offsetof({t}, {f}));' for f in fields) + "return 0;}"
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == ctypes.sizeof(PQCascadeArgs) == 8 + ctypes.sizeof(PQDecodeArgs) + 24
    assert nums[1:] == [getattr(PQCascadeArgs, f).offset for f in fields]
    assert nums[1:4] == [0, 4, 8] and nums[4:] == [nums[0] - 24, nums[0] - 16, nums[0] - 8]


def test_every_documented_refusal_returns_its_code():
    from spatten_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    bf16 = _codes()[0]["SPATTEN_BF16"]
    state = _state_bytes(lib, bf16)
    planes = _planes()
    call = lambda ca, sb=ACC_SB: fn(ctypes.byref(ca), sb, None)

    # the state: required, strided, and by step_stride_ok's rule at every batch size
    assert call(_block(planes, bf16, state, None)) == INVALID
    assert call(_block(planes, bf16, 0)) == INVALID                  # the shared state stays with the old call
    for stride, step in _bad_strides(state):
        assert call(_block(planes, bf16, stride, step)) == INVALID, (stride, step)
        ca = _block(planes, bf16, stride, step)
        ca.step.batch = 1
        assert call(ca) == INVALID, (stride, step, "batch 1")
    # whatever spatten_attn_decode_pq_cascade refuses as invalid
    for edit in (dict(importance_acc=None), dict(prev_lse=None), dict(struct_size=ctypes.sizeof(_lib.PQCascadeArgs) - 8)):
        ca = _block(planes, bf16, state)
        for k, v in edit.items():
            setattr(ca, k, v)
        assert call(ca) == INVALID, edit
    for edit in (dict(lse=None), dict(q=None), dict(need_lsb=None), dict(kv_len=0), dict(heads=7), dict(n_active_heads=9, head_ids=0x190000),
                 dict(struct_size=8), dict(dtype=17), dict(kv_len_layout=-1), dict(k_new=0x50000)):      # (k_new without v_new)
        ca = _block(planes, bf16, state)
        for k, v in edit.items():
            setattr(ca.step, k, v)
        assert call(ca) == INVALID, edit
    no_lg = _planes()
    no_lg.msb_logit = None
    assert call(_block(no_lg, bf16, state)) == INVALID
    # the accumulator's batch stride
    assert call(_block(planes, bf16, state), -ACC_SB) == INVALID
    assert call(_block(planes, bf16, state), -1) == INVALID
    for stride in (state, 2 * state):
        assert call(_block(planes, bf16, stride), 0) == UNSUPPORTED  # a valid block: one [H, L] accumulator, many lengths
    ca = _block(planes, bf16, state)
    ca.step.batch = 1
    assert call(ca, 0) == UNSUPPORTED
    assert call(_block(planes, bf16, state), 1 << 31) == UNSUPPORTED   # beyond the 32 bits spatten_decode_args_t's acc_sb has too
    # the append stays outside the launch
    ca = _block(planes, bf16, state)
    ca.step.k_new, ca.step.v_new, ca.step.kr_cache, ca.step.v_cache = 0x50000, 0x60000, 0x30000, 0x40000
    assert call(ca) == UNSUPPORTED
    # geometry the profiled step does not have
    ca = _block(planes, bf16, state)
    ca.step.head_dim = 96
    assert call(ca) == UNSUPPORTED
    # prev_len is ignored (every state's word 3 takes its place): a value the old call refuses changes nothing here
    ca = _block(planes, bf16, state)
    ca.prev_len = -1
    ca.step.k_new, ca.step.v_new, ca.step.kr_cache, ca.step.v_cache = 0x50000, 0x60000, 0x30000, 0x40000
    assert call(ca) == UNSUPPORTED


def test_old_entry_point_still_refuses_a_valid_stride():
    from spatten_amd import _lib
    lib = _lib.load()
    bf16 = _codes()[0]["SPATTEN_BF16"]
    state = _state_bytes(lib, bf16)
    planes = _planes()
    for stride in (state, 2 * state):
        assert lib.spatten_attn_decode_pq_cascade(ctypes.byref(_block(planes, bf16, stride)), None) == UNSUPPORTED
    assert lib.spatten_attn_decode_pq_cascade(ctypes.byref(_block(planes, bf16, 100)), None) == INVALID


class Batched:                           # what ops asks of a StepState(batch=B)
    batch, stride = 3, 768


class Q:
    shape = (3, 8, 128)


def test_ops_keeps_refusing_an_accumulator_without_a_batch_axis():
    import torch
    from spatten_amd import ops
    with pytest.raises(NotImplementedError, match="batch axis"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(None, None, 0), lse=0)
    with pytest.raises(NotImplementedError, match="batch axis"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(torch.zeros(8, 16), None, 0), lse=0)
    # the other forms a cascade step never had
    with pytest.raises(NotImplementedError, match="quantised-query"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(torch.zeros(3, 8, 16), None, 0), lse=0,
                            query_bits=8)
    with pytest.raises(NotImplementedError, match="append"):
        ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(torch.zeros(3, 8, 16), None, 0), lse=0,
                            append=(None,) * 5)


def test_ops_refuses_a_batched_accumulator_of_the_wrong_batch():
    import torch
    from spatten_amd import ops
    for rows in (2, 4):
        with pytest.raises(ValueError, match="sequences"):
            ops.attn_decode_pqv(Q(), None, 8, None, None, 0, 0.5, step=Batched(), cascade=(torch.zeros(rows, 8, 16), None, 0), lse=0)
