"""The profiled decode step with the folded cascade importance (spatten_attn_decode_pq_cascade; ``pq_cascade=True``) without a
GPU: the keyword rules of the plugin, the export and its ctypes binding, the C compiler's layout of the argument block, and the
evidence that the criterion of tests/test_gpu_pq_cascade.py tells a wrong kernel from a right one on that test's own inputs."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from spatten_amd import enable_spatten_llm
from tests import pq_cascade_case as pcc
from tests import pq_exact as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hf_llama():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=3,
                                   num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=64)
    return transformers.LlamaForCausalLM(cfg)


def test_pq_cascade_is_accepted_and_graph_capable(hf_llama):
    c = enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_profile=(8, 8), importance_mode="cascade", pq_cascade=True)
    assert c.ext.pq_cascade and c.ext.cascade and not c.ext.pq_local_v and c.ext.graph_capable()
    c = enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_profile=(6, 6), importance_mode="cascade", pq_cascade=True,
                           head_keep=[4, 3, 2])
    assert c.ext.pq_cascade and c.ext.graph_capable()


@pytest.mark.parametrize("kw", [
    dict(pq_profile=(8, 8), importance_mode="cascade", local_v_keep=1.0),            # the composed step already accumulates
    dict(pq_profile=(8, 8), importance_mode="cascade", pq_query_bits=8),
    dict(pq_profile=(8, 8), importance_mode="cascade", pq_query_bits=8, pq_grouped=True),
    dict(pq_profile=(8, 8)),                                                          # no cascade mode
    dict(importance_mode="cascade")])                                                 # no profile
def test_pq_cascade_invalid_combinations(hf_llama, kw):
    with pytest.raises(ValueError, match="pq_cascade"):
        enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_cascade=True, **kw)


def test_invalid_combinations_at_the_extension_class():
    from spatten_amd.extensions import SpattenExtensions
    base = dict(cascade=True, pq_threshold=0.05, pq_profile=(8, 8), pq_cascade=True)
    for kw in (dict(local_v_keep=0.5), dict(pq_query_bits=8), dict(pq_query_bits=8, pq_grouped=True), dict(cascade=False),
               dict(pq_profile=None)):
        with pytest.raises(ValueError, match="pq_cascade"):
            SpattenExtensions(None, 2, **{**base, **kw})
    assert SpattenExtensions(None, 2, **base).pq_logit_fold


def test_without_the_keyword_the_refusal_stays_and_names_it(hf_llama):
    with pytest.raises(ValueError, match="does not carry the fused.*pq_cascade=True"):
        enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.1, pq_profile=(8, 8), importance_mode="cascade")


def test_entry_point_is_exported_and_bound():
    from spatten_amd import _lib
    lib = _lib.load()
    fn = lib.spatten_attn_decode_pq_cascade
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.POINTER(_lib.PQCascadeArgs), ctypes.c_void_p]
    assert lib.spatten_abi_version() == 5
    # NULL / a wrong struct_size are refused on the host, before anything touches a device
    assert fn(None, None) == -1                 # SPATTEN_ERR_INVALID
    bad = _lib.PQCascadeArgs()
    bad.struct_size = ctypes.sizeof(_lib.PQCascadeArgs) - 8
    assert fn(ctypes.byref(bad), None) == -1


def test_pq_cascade_args_struct_matches_the_header():
    from spatten_amd._lib import PQCascadeArgs
    fields = [f[0] for f in PQCascadeArgs._fields_]
    cname = "spatten_pq_cascade_args_t"
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu", sizeof(' + cname + '));' + \
        "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        nums = [int(x) for x in subprocess.check_output([exe]).split()]
    assert nums[0] == ctypes.sizeof(PQCascadeArgs)
    assert nums[1:] == [getattr(PQCascadeArgs, f).offset for f in fields]


def test_ops_refuses_the_forms_out_of_scope_before_touching_a_device():
    import torch
    from spatten_amd import ops
    q = torch.zeros(1, 4, 128)
    for kw in (dict(query_bits=8), dict(query_bits=8, grouped=True), dict(append=(None,) * 5)):
        with pytest.raises(NotImplementedError, match="cascade"):
            ops.attn_decode_pqv(q, None, 8, None, None, 7, 0.1, lse=torch.zeros(1, 4, 2), cascade=(None, None, 0), **kw)
    with pytest.raises(ValueError, match="lse"):
        ops.attn_decode_pqv(q, None, 8, None, None, 7, 0.1, cascade=(None, None, 0))


# ---- the criterion on the GPU test's inputs --------------------------------------------------------------------------------
_CPU_CASES = [c for c in pcc.GPU_CASES if c[4] <= 600] + [("bf16", (8, 8), 128, 4, 1031, 4)]


@pytest.mark.parametrize("dt,prof,d,Hkv,N,ns", _CPU_CASES)
def test_criterion_accepts_the_emulated_kernel_and_rejects_every_fault(dt, prof, d, Hkv, N, ns):
    """pq_exact.emulate_cascade over the steps of the case: fault-free passes check_cascade (with the slack and constants the
    GPU test uses), each of CASCADE_FAULTS fails it.  (n_splits does not enter the emulation: a fold is one add per row.)"""
    pc = pcc.case(dt, prof[0], prof[1], d, 4, Hkv, N)
    thr = pcc.threshold(pc)
    em = pcc.emulated_steps(pc, thr)
    assert em.needs[-1].any() and not em.needs[-1].all()
    ex_sum, or_sum, slack = pcc.references(pc, thr, em.needs)
    T = len(em.rows)
    px.check_cascade(px.emulate_cascade(em.rows), or_sum, ex_sum, T, slack=slack, name="fault-free")
    for fault in px.CASCADE_FAULTS:
        with pytest.raises(AssertionError, match="importance"):
            px.check_cascade(px.emulate_cascade(em.rows, fault=fault), or_sum, ex_sum, T, slack=slack, name=fault)


def test_criterion_at_batch_two():
    pc = pcc.case("bf16", 8, 8, 128, 4, 4, 600, B=2)
    thr = pcc.threshold(pc)
    em = pcc.emulated_steps(pc, thr)
    ex_sum, or_sum, slack = pcc.references(pc, thr, em.needs)
    px.check_cascade(px.emulate_cascade(em.rows), or_sum, ex_sum, len(em.rows), slack=slack)
    for fault in px.CASCADE_FAULTS:
        with pytest.raises(AssertionError, match="importance"):
            px.check_cascade(px.emulate_cascade(em.rows, fault=fault), or_sum, ex_sum, len(em.rows), slack=slack)
