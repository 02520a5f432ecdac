"""The ragged prune event and the per-sequence cascade accumulator, as far as host arithmetic goes (include/spatten.h: "Ragged prune
event", spatten_decode_args_t::acc_sb, spatten_importance_accumulate_step): the argument blocks' layout, what spatten_decode_gqa_form
answers for acc_sb, every host refusal of the two new entry points, and the numpy restatement of the event
(tests/ragged_prune_case.py) against oracle.apply_token_pruning at a uniform length.  No GPU: the pointers below are never
dereferenced — every call returns its code before the first launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import spatten_oracle as orc
from tests import ragged_prune_case as rpc
from tests.strided import header_strides
from tests.test_ragged_step_cpu import _block, _dtype_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _offsets(tmp_path, cname, fields):
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu", sizeof(' + cname + "));" +
            "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + "return 0;}")
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_prune_ragged_block_matches_the_header(tmp_path):
    from spatten_amd._lib import PruneRaggedArgs
    fields = [f[0] for f in PruneRaggedArgs._fields_]
    nums = _offsets(tmp_path, "spatten_prune_ragged_args_t", fields)
    assert nums[0] == ctypes.sizeof(PruneRaggedArgs)
    assert nums[1:] == [getattr(PruneRaggedArgs, f).offset for f in fields]


def test_acc_sb_takes_the_place_of_the_pad_word(tmp_path):
    """The renamed pad word: the int32 right behind prev_len, in front of importance_acc; the block keeps its size (the parent's:
    the offsets of its neighbours are those gcc gives), the ABI version stays 5."""
    from spatten_amd import _lib
    from spatten_amd._lib import DecodeArgs
    fields = [f[0] for f in DecodeArgs._fields_]
    assert "acc_sb" in fields and "pad1_" not in fields
    assert fields[fields.index("acc_sb") - 1] == "prev_len" and fields[fields.index("acc_sb") + 1] == "importance_acc"
    size, off_prev, off_sb, off_acc = _offsets(tmp_path, "spatten_decode_args_t", ["prev_len", "acc_sb", "importance_acc"])
    assert off_sb == off_prev + 4 and off_acc == off_sb + 4
    assert off_sb == DecodeArgs.acc_sb.offset and DecodeArgs.acc_sb.size == 4
    assert size == ctypes.sizeof(DecodeArgs) == 512              # the parent's size
    assert _lib.load().spatten_abi_version() == 5


def test_the_stride_ledger_does_not_name_the_new_entry_points():
    names = {entry for entry, _ in header_strides()}
    assert not names & {"spatten_prune_ragged", "spatten_prune_ragged_args", "spatten_importance_accumulate_step"}
    assert ("spatten_decode_args", "acc_sh") in header_strides() and ("spatten_decode_args", "acc_sb") not in header_strides()


def test_gqa_form_answers_for_acc_sb():
    from spatten_amd import ops
    lib = ops._lib.load()
    bf16 = _dtype_codes()["SPATTEN_BF16"]
    lib.spatten_step_state_bytes.restype = ctypes.c_size_t
    state = lib.spatten_step_state_bytes(bf16, 128)
    form = lambda a: lib.spatten_decode_gqa_form(ctypes.byref(a))

    def casc(stride, acc_sb):
        a = _block(bf16, stride)
        a.importance_acc, a.acc_sh, a.acc_sb = 0xD0000, 704, acc_sb
        a.prev_scores, a.prev_sb, a.prev_sh, a.prev_lse = 0xE0000, 8 * 704, 704, 0xF0000
        return a

    prev = ops.set_decode_gqa(1)
    try:
        assert form(casc(state, 8 * 704)) == 1                      # one state AND one accumulator per sequence
        assert form(casc(state, 0)) == 0                            # ... one accumulator for the batch: refused, as before
        assert form(casc(state, -8 * 704)) == 0
        assert form(casc(0, 8 * 704)) == 1                          # the shared state admits both
        assert form(casc(0, 0)) == 1
        assert form(casc(0, -1)) == 0
        a = _block(bf16, state)
        a.acc_sb = 8 * 704                                          # a stride without an accumulator
        assert form(a) == 0
        lib.spatten_attn_decode_args.restype = ctypes.c_int
        assert lib.spatten_attn_decode_args(ctypes.byref(a), None) == INVALID
        assert lib.spatten_attn_decode_args(ctypes.byref(casc(state, -1)), None) == INVALID
        assert lib.spatten_attn_decode_args(ctypes.byref(casc(state, 0)), None) == UNSUPPORTED
        a = casc(state, 8 * 704)
        a.k_new, a.v_new = None, None
        a.pq_msb, a.pq_lsb, a.pq_scale, a.pq_need_lsb = 0x100000, 0x110000, 0x120000, 0x130000
        assert lib.spatten_attn_decode_args(ctypes.byref(a), None) == UNSUPPORTED
    finally:
        ops.set_decode_gqa(prev)


def _ragged_block(**over):
    """layers 2, B = 3, 2 heads, d = 128 bf16, fp32 scores, start 4 / recent 8 / k 16 / 1 coming: keep_rows 27."""
    from spatten_amd._lib import PruneRaggedArgs
    codes = _dtype_codes()
    a = PruneRaggedArgs()
    a.struct_size = ctypes.sizeof(PruneRaggedArgs)
    a.score_dtype, a.kv_dtype = codes["SPATTEN_F32"], codes["SPATTEN_BF16"]
    a.layers, a.batch, a.heads, a.head_dim = 2, 3, 2, 128
    a.lens, a.lens_step = 0x1000, 1
    a.bound, a.start, a.recent, a.k, a.num_coming, a.out_rows, a.table_rows = 320, 4, 8, 16, 1, 40, 64
    a.score_ptrs, a.score_batch_stride, a.score_head_stride = 0x2000, 2 * 320, 320
    a.k_src_ptrs, a.v_src_ptrs, a.src_batch_stride, a.src_head_stride = 0x3000, 0x4000, 2 * 320 * 128, 320 * 128
    a.k_dst_ptrs, a.v_dst_ptrs, a.kr_dst_ptrs, a.dst_batch_stride, a.dst_head_stride = 0x5000, 0x6000, 0x7000, 2 * 40 * 128, 40 * 128
    a.cos, a.sin, a.idx, a.new_lens = 0x8000, 0x9000, 0xA000, 0xB000
    a.acc_src_ptrs, a.acc_dst_ptrs, a.acc_heads, a.acc_cols = 0xC000, 0xD000, 4, 48
    a.acc_src_batch_stride, a.acc_src_head_stride, a.acc_dst_batch_stride, a.acc_dst_head_stride = 4 * 320, 320, 4 * 48, 48
    for name, v in over.items():
        setattr(a, name, v)
    return a


REFUSALS = [
    (dict(num_coming=9), INVALID), (dict(num_coming=-1), INVALID), (dict(start=-1), INVALID), (dict(k=0), INVALID),
    (dict(recent=-1, num_coming=0), INVALID),
    (dict(out_rows=26), INVALID), (dict(acc_cols=26), INVALID),
    (dict(acc_src_ptrs=None), INVALID), (dict(acc_dst_ptrs=None), INVALID),
    (dict(acc_heads=3), INVALID), (dict(acc_heads=0), INVALID),
    (dict(struct_size=8), INVALID), (dict(struct_size=ctypes.sizeof(ctypes.c_void_p) * 1000), INVALID),
    (dict(lens=None), INVALID), (dict(score_ptrs=None), INVALID), (dict(k_src_ptrs=None), INVALID), (dict(v_src_ptrs=None), INVALID),
    (dict(k_dst_ptrs=None), INVALID), (dict(v_dst_ptrs=None), INVALID), (dict(idx=None), INVALID), (dict(new_lens=None), INVALID),
    (dict(cos=None), INVALID), (dict(sin=None), INVALID), (dict(table_rows=39), INVALID),
    (dict(lens_step=0), INVALID), (dict(bound=0), INVALID), (dict(layers=0), INVALID), (dict(batch=0), INVALID), (dict(heads=0), INVALID),
    (dict(score_dtype=7), INVALID), (dict(kv_dtype=7), INVALID), (dict(src_head_stride=-1), INVALID),
    (dict(head_dim=8), UNSUPPORTED),                               # 16-byte rows: no pair of 16-byte pieces
    (dict(head_dim=24), UNSUPPORTED),
    (dict(batch=40000), UNSUPPORTED), (dict(layers=40000), UNSUPPORTED),           # grid limits
]


@pytest.mark.parametrize("over,want", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_prune_ragged_refuses_before_the_first_launch(over, want):
    from spatten_amd import _lib
    lib = _lib.load()
    assert lib.spatten_prune_ragged(ctypes.byref(_ragged_block(**over)), None) == want
    assert lib.spatten_prune_ragged(None, None) == INVALID


def test_importance_accumulate_step_refuses_before_the_launch():
    from spatten_amd import _lib
    lib = _lib.load()
    bf16 = _dtype_codes()["SPATTEN_BF16"]
    good = dict(dtype=bf16, stash0=0x1000, lse0=0x2000, stash1=0x3000, lse1=0x4000, sb=8 * 704, sh=704, acc=0x5000, acc_b=8 * 704,
                acc_h=704, batch=2, heads=8, bound=704, state=0x6000, state_sb=512)
    call = lambda **o: lib.spatten_importance_accumulate_step(*{**good, **o}.values(), None)
    for o in (dict(stash0=None), dict(lse0=None), dict(stash1=None), dict(lse1=None), dict(acc=None), dict(state=None), dict(dtype=9),
              dict(batch=0), dict(heads=0), dict(bound=0), dict(acc_b=0), dict(acc_b=-1), dict(acc_h=-1), dict(state_sb=-256),
              dict(state_sb=6)):
        assert call(**o) == INVALID, o


@pytest.mark.parametrize("dt,d", [("bf16", 128), ("f32", 64)])
def test_the_restatement_is_the_oracle_at_a_uniform_length(dt, d):
    """Every sequence at one length: the helper is oracle.apply_token_pruning of the batch, with per-sequence scores.  (The oracle
    ranks ONE score row per head for the whole batch; the helper ranks each sequence's own — compared sequence by sequence.)"""
    start, recent, k, nc, layers, H, L = 4, 8, 16, 1, 2, 2, 50
    B = 2
    Ks = [orc.synth_normal(31, 2 * l, (B, H, L, d), dt) for l in range(layers)]
    Vs = [orc.synth_normal(31, 2 * l + 1, (B, H, L, d), dt) for l in range(layers)]
    scores = rpc.make_scores(5, layers, B, H, L, [L] * B, start, recent, k, nc)
    accs = [orc.synth_normal(32, l, (B, 2 * H, L), "f32") for l in range(layers)]
    keep = rpc.keep_rows(start, recent, k, nc)
    got = rpc.reference(scores, Ks, Vs, [L] * B, start, recent, k, nc, keep + 5, dt, accs=accs, acc_cols=keep + 2)
    assert list(got["new_lens"]) == [keep] * B
    cos, sin = orc.rope_table(keep, d, dt)
    for b in range(B):
        past = [(Ks[l][b:b + 1], Vs[l][b:b + 1]) for l in range(layers)]
        stash = [scores[l][b:b + 1, :, None, :] for l in range(layers)]
        want, idxs = orc.apply_token_pruning(past, nc, stash, start, recent, k, "f32")       # fp32 scores: importance() is the identity
        for l in range(layers):
            assert np.array_equal(got["idx"][(l, b)], idxs[l])
            assert np.array_equal(got["K"][l][b, :, :keep], want[l][0][0]) and np.array_equal(got["V"][l][b, :, :keep], want[l][1][0])
            kr = orc.apply_rotary_pos_emb_single(want[l][0], cos, sin, np.arange(keep)[None], dt)[0]
            assert np.array_equal(got["Kr"][l][b, :, :keep], kr)
            for t in ("K", "V", "Kr"):
                assert not got[t][l][b, :, keep:].any()
            hi = L - recent + nc
            for a in range(2 * H):
                rows = np.concatenate([np.arange(start), idxs[l][a // 2], np.arange(hi, L)])
                assert np.array_equal(got["acc"][l][b, a, :keep], accs[l][b, a, rows])
            assert not got["acc"][l][b, :, keep:].any()
    # the planted ties: head 0 keeps the two LOWEST indices of the plateau; head 1 keeps the NaN
    s0 = scores[0][0]
    plateau = np.flatnonzero(s0[0, start:L - recent + nc] == 5.0) + start
    kept = set(got["idx"][(0, 0)][0].tolist())
    assert len(plateau) > 2 and [p in kept for p in plateau] == [True, True] + [False] * (len(plateau) - 2)
    assert int(np.flatnonzero(np.isnan(s0[1]))[0]) in set(got["idx"][(0, 0)][1].tolist())
    # an unpruned length passes through with the zero fill
    short = rpc.reference(scores, Ks, Vs, [27, 0], start, recent, k, nc, keep + 5, dt)
    assert list(short["new_lens"]) == [27, 0] and not short["idx"]
    assert np.array_equal(short["K"][1][0, :, :27], Ks[1][0, :, :27]) and not short["K"][1][0, :, 27:].any() and not short["V"][0][1].any()
