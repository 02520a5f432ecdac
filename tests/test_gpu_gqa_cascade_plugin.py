"""enable_spatten_llm(importance_mode="cascade") on a small grouped-query Llama-style stack (4 query heads on 2 KV heads, d = 128)
with the matrix-core grouped-query step forced: the decode step carries the fused accumulation in the grouped form (the predicate
says so for the very block the plugin assembles), and the eager token loop and DecodeGraph replay agree bit for bit in the hidden
states, the kept indices of a prune event and the accumulator.  Needs an MI355X."""
import contextlib
import io

import pytest
import torch
from torch import nn

from tests.test_gpu_graph_decode import D, Stack

pytestmark = pytest.mark.gpu

HQ, HKV = 4, 2
HID = HQ * D


def _gqa_stack(dt):
    st = Stack(dt)
    for m in st.layers:
        m.num_heads, m.num_key_value_heads, m.num_key_value_groups, m.hidden_size = HQ, HKV, HQ // HKV, HID
        m.q_proj = nn.Linear(HID, HQ * D, bias=False, dtype=dt, device="cuda")
        m.k_proj = nn.Linear(HID, HKV * D, bias=False, dtype=dt, device="cuda")
        m.v_proj = nn.Linear(HID, HKV * D, bias=False, dtype=dt, device="cuda")
        m.o_proj = nn.Linear(HQ * D, HID, bias=False, dtype=dt, device="cuda")
    return st


def test_plugin_cascade_step_runs_grouped_eager_and_captured(monkeypatch):
    from spatten_amd import enable_spatten_llm, ops
    from spatten_amd.graph import DecodeGraph
    dt = torch.bfloat16
    torch.manual_seed(7)
    a = _gqa_stack(dt)
    for p in a.parameters():
        p.data.mul_(0.5)
    b = _gqa_stack(dt)
    b.load_state_dict(a.state_dict())
    forms = []
    launch = ops.attn_decode

    def spy(*args, **kw):
        if kw.get("cascade") is not None and not kw.get("gqa_form"):
            forms.append(ops.decode_gqa_form(*args, **kw))
        return launch(*args, **kw)

    prev = ops.set_decode_gqa(1)
    monkeypatch.setattr(ops, "attn_decode", spy)
    try:
        caches = []
        for m in (a, b):
            with contextlib.redirect_stdout(io.StringIO()):
                caches.append(enable_spatten_llm(m, 4, 60, 64, importance_mode="cascade"))
        g = torch.Generator(device="cuda").manual_seed(3)
        x0 = torch.randn(1, 170, HID, device="cuda", generator=g).to(dt)
        _, past_a = a(x0, None)
        _, past_b = b(x0, None)
        assert past_a[0][0].shape[1] == HKV
        for turn in range(2):
            graph = DecodeGraph(lambda past, x: tuple(reversed(b(x, past))), past_b, horizon=8)
            for t in range(8):
                x = torch.randn(1, 1, HID, device="cuda", generator=g).to(dt)
                ya, past_a = a(x, past_a)
                yb = graph.step(x)
                assert torch.equal(ya, yb), (turn, t)
            past_b = graph.past_key_values
            torch.cuda.synchronize()
            new_a = caches[0].apply_token_pruning(past_a, 14, [m.attn_scores for m in a.layers])
            new_b = caches[1].apply_token_pruning(past_b, 14, [m.attn_scores for m in b.layers])
            assert new_a is not past_a
            assert torch.equal(caches[0].keep_indices, caches[1].keep_indices)
            for sa, sb in zip(caches[0].ext.layers, caches[1].ext.layers):
                assert torch.equal(sa.acc, sb.acc) and float(sa.acc.sum()) > 0.0
            for (ka, va), (kb, vb) in zip(new_a, new_b):
                assert ka.shape[1] == HKV and torch.equal(ka, kb) and torch.equal(va, vb)
            xp = torch.randn(1, 6, HID, device="cuda", generator=g).to(dt)
            ya, past_a = a(xp, new_a)
            yb, past_b = b(xp, new_b)
            assert torch.equal(ya, yb)
        assert forms and all(forms), "the plugin's cascade step did not take the grouped form"
        ops.check_workspaces()
    finally:
        ops.set_decode_gqa(prev)
