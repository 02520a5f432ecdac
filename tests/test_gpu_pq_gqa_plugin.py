"""enable_spatten_llm(..., pq_profile=(8, 8), pq_query_bits=8, pq_grouped=True) on a grouped-query HF-4.33-style stack (H = 8,
Hkv = 2, D = 128: the stack of test_decode_graph_on_a_grouped_query_stack under a whole LM): the eager loop and auto_graph give
bit-identical logits, the captured graph really replays, and every layer's first decode step is judged against exact math with
the query that layer exported (tests/pq_qint_exact.check_step).  Needs an MI355X."""
import contextlib
import io

import pytest
import torch
from torch import nn

from tests.test_gpu_graph_decode import D, H, HID, _HFStyleLM, _TinyLM
from tests.test_gpu_pq_qint_plugin import BITS, GEN, THR, _check_first_step

pytestmark = pytest.mark.gpu

HKV = 2


def _gqa_lm(dt):
    m = _HFStyleLM(dt)
    for layer in m.layers:
        a = layer.self_attn
        a.num_key_value_heads, a.num_key_value_groups = HKV, H // HKV
        a.k_proj = nn.Linear(HID, HKV * D, bias=False, dtype=dt, device="cuda")
        a.v_proj = nn.Linear(HID, HKV * D, bias=False, dtype=dt, device="cuda")
    return m


def test_plugin_grouped_eager_and_auto_graph_agree_and_first_step_is_exact():
    from spatten_amd import enable_spatten_llm
    dt = torch.bfloat16
    torch.manual_seed(5)
    a, b = _gqa_lm(dt), _gqa_lm(dt)
    b.load_state_dict(a.state_dict())
    caches = []
    for m, auto in ((a, False), (b, True)):
        with contextlib.redirect_stdout(io.StringIO()):
            caches.append(enable_spatten_llm(m, 4, 40, 40, auto_graph=auto, pq_threshold=THR, pq_profile=(8, 8),
                                             pq_query_bits=BITS, pq_grouped=True))
    assert all(c.ext.pq_grouped for c in caches)
    g = torch.Generator(device="cuda").manual_seed(21)
    ids = torch.randint(0, _TinyLM.VOCAB, (1, 90), device="cuda", generator=g)
    logits = [[], []]
    flagged = 0
    with torch.no_grad():
        for k, (model, cache) in enumerate(zip((a, b), caches)):
            out = model(input_ids=ids, past_key_values=None, use_cache=True)
            past = out.past_key_values
            assert past[0][0].shape[1] == HKV
            pred = out.logits[:, -1, :].argmax(dim=-1).unsqueeze(1)
            logits[k].append(out.logits[:, -1].clone())
            for t in range(GEN):
                out = model(input_ids=pred, past_key_values=past, use_cache=True)
                past = out.past_key_values
                torch.cuda.synchronize()
                if t == 0:
                    _check_first_step(model, cache, past, "auto_graph" if k else "eager")
                flagged += int(sum(int(st.need_lsb.sum()) for st in cache.ext.layers))
                pred = out.logits[:, -1, :].argmax(dim=-1).unsqueeze(1)
                logits[k].append(out.logits[:, -1].clone())
    for x, y in zip(*logits):
        assert torch.equal(x, y)
    graph = b._spatten_auto_graph["graph"]
    assert graph is not None and graph.n_replays == GEN - 1          # a real capture (a failed one falls back with no replays)


def test_plugin_grouped_keyword_is_refused_where_it_cannot_run():
    from spatten_amd import enable_spatten_llm
    ok = dict(pq_threshold=0.1, pq_profile=(8, 8), pq_query_bits=8)
    for kw in (dict(ok, pq_query_bits=None), dict(ok, pq_profile=(4, 8)), dict(ok, head_keep=6), dict(ok, local_v_keep=0.5)):
        with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
            enable_spatten_llm(_gqa_lm(torch.bfloat16), 4, 40, 40, pq_grouped=True, **kw)
    # a model that is not grouped-query raises at its first decode step
    m = _HFStyleLM(torch.bfloat16)
    with contextlib.redirect_stdout(io.StringIO()):
        enable_spatten_llm(m, 4, 40, 40, pq_grouped=True, **ok)
    ids = torch.randint(0, _TinyLM.VOCAB, (1, 30), device="cuda")
    with torch.no_grad():
        out = m(input_ids=ids, past_key_values=None, use_cache=True)
        with pytest.raises(NotImplementedError, match="grouped"):
            m(input_ids=ids[:, :1], past_key_values=out.past_key_values, use_cache=True)
