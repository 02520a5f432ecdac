"""The composed step over the quantised planes without a GPU: the plugin accepts the combination the RTL's fullest trace runs
(profile + local V + cascade importance + head pruning) and captures it, and the C ABI block of spatten_attn_decode_pq_local_v
has the C compiler's layout."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from spatten_amd import enable_spatten_llm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hf_llama():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=3,
                                   num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=64)
    return transformers.LlamaForCausalLM(cfg)


def test_profile_local_v_cascade_heads_is_accepted_and_graph_capable(hf_llama):
    c = enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_profile=(8, 8), local_v_keep=0.3,
                           importance_mode="cascade", head_keep=[4, 3, 2])
    assert c.ext.pq_local_v and c.ext.cascade and c.ext.graph_capable()
    c = enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_profile=(6, 6), local_v_keep=1.0, importance_mode="cascade")
    assert c.ext.pq_local_v and c.ext.graph_capable()
    c = enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.05, pq_profile=(4, 8), local_v_keep=0.5)
    assert c.ext.pq_local_v and not c.ext.cascade and c.ext.graph_capable()


def test_refusals_without_the_profile_stay(hf_llama):
    with pytest.raises(ValueError, match="cannot be combined"):
        enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.1, local_v_keep=0.5)
    with pytest.raises(ValueError, match="cascade"):
        enable_spatten_llm(hf_llama, 4, 8, 8, pq_threshold=0.1, pq_profile=(8, 8), importance_mode="cascade")
    with pytest.raises(ValueError, match="auto_graph"):
        enable_spatten_llm(hf_llama, 4, 8, 8, local_v_keep=0.5, importance_mode="cascade", auto_graph=True)


def test_pq_local_v_args_struct_matches_the_header():
    from spatten_amd._lib import PQLocalVArgs
    fields = [f[0] for f in PQLocalVArgs._fields_]
    cname = "spatten_pq_local_v_args_t"
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu", sizeof(' + cname + '));' + \
        "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        nums = [int(x) for x in subprocess.check_output([exe]).split()]
    assert nums[0] == ctypes.sizeof(PQLocalVArgs)
    assert nums[1:] == [getattr(PQLocalVArgs, f).offset for f in fields]


def _sched_args(**kw):
    from types import SimpleNamespace
    a = dict(schedule=os.path.join(ROOT, "tests", "golden", "trace_full_cascade.csv"), layers=4, heads=8, important_size=150,
             pq_threshold=0.05, local_v_keep=None, cascade=False, full_cascade=True)
    a.update(kw)
    return SimpleNamespace(**a)


def test_full_cascade_schedule_mapping():
    """--schedule --full-cascade on the fixture (keys 1024 -> 640 of 1024, values ~0.31 of the keys, heads 8 -> 4, 12-bit keys
    and 8-bit values without a threshold, cumulative importance on)."""
    import run_spatten_synthetic as rs
    ext = rs.schedule_options(_sched_args())
    assert ext["pq_profile"] == (8, 8) and ext["pq_threshold"] == 0.05
    assert ext["local_v_keep"] == round(1034 / 3328, 4)
    assert ext["importance_mode"] == "cascade"
    assert ext["layer_keep"] == [150, 131, 112, 94]
    assert ext["head_keep"] == [8, 8, 6, 4]
    assert ext["token_scope"] == "global"
    # the trace carries no threshold (auto_requant_thres -1): --pq-threshold is then required, by name
    with pytest.raises(SystemExit, match="--pq-threshold"):
        rs.schedule_options(_sched_args(pq_threshold=None))
    # without --full-cascade the schedule keeps its old mapping (no local V, no profile without a threshold)
    old = rs.schedule_options(_sched_args(full_cascade=False, pq_threshold=None))
    assert "local_v_keep" not in old and "pq_profile" not in old
