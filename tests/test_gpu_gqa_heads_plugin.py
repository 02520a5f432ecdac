"""enable_spatten_llm(head_keep=..., grouped_head_pruning=True) under the restated transformers 4.33 decoder stack
(tests/llama433.py) at a tiny grouped-query geometry — 8 query heads on 2 KV heads, d = 128, 2 layers — with the matrix-core form
allowed (set_decode_gqa(1)): the very blocks the plugin assembles for its head-pruning steps take the grouped form (head importance
alone before the first prune event, head list + head importance after it), the same stack without the keyword keeps them on the
per-query-head kernel, and both prune the same heads and produce the same logits.  Eager loop and auto_graph.  Needs an MI355X.

Tolerance: tests/test_gpu_gqa_cascade_plugin.py compares two runs of ONE kernel form and can ask for equal bits.  Here the two runs
take different forms, whose attention outputs differ in summation order (tests/util.py OUT_TOL), so the logits are held to the bound
this suite states for bf16 logits of this stack (tests/test_gpu_hf_decoder.py: atol 0.15, rtol 0.1); the kept-head lists must be equal."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import llama433

pytestmark = pytest.mark.gpu

HQ, HKV, LAYERS, HID = 8, 2, 2, 1024
LOGIT_TOL = dict(atol=0.15, rtol=0.1)


@pytest.mark.parametrize("auto_graph", [False, True])
def test_head_keep_turn_takes_the_grouped_form_and_prunes_the_same_heads(monkeypatch, auto_graph):
    from spatten_amd import enable_spatten_llm, ops
    dt = torch.bfloat16
    torch.manual_seed(3)
    cfg = llama433.tiny_config(hidden=HID, heads=HQ, kv_heads=HKV, layers=LAYERS, inter=512)
    models = [llama433.LlamaForCausalLM(cfg).cuda().to(dt) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    seen = [[], []]                    # per model: (the block carries a head list, the form the predicate reports)
    current = [0]
    launch = ops.attn_decode

    def spy(*args, **kw):
        if not kw.get("gqa_form") and (kw.get("head_ids") is not None or kw.get("head_abs") is not None):
            seen[current[0]].append((kw.get("head_ids") is not None, ops.decode_gqa_form(*args, **kw)))
        return launch(*args, **kw)

    g = torch.Generator(device="cuda").manual_seed(9)
    prompt = torch.randint(0, cfg.vocab_size, (1, 170), device="cuda", generator=g)
    turns = [torch.randint(0, cfg.vocab_size, (8,), device="cuda", generator=g) for _ in range(2)]
    prev = ops.set_decode_gqa(1)
    monkeypatch.setattr(ops, "attn_decode", spy)
    try:
        logits, kept = [[], []], []
        for k, (model, flag) in enumerate(zip(models, (True, False))):
            current[0] = k
            with contextlib.redirect_stdout(io.StringIO()):
                cache = enable_spatten_llm(model, 4, 60, 64, head_keep=[7, 6], grouped_head_pruning=flag, auto_graph=auto_graph)
            assert cache.ext.grouped_head_pruning is flag
            mods = [m for m in model.modules() if type(m).__name__ == "LlamaAttention"]
            past = model(input_ids=prompt, past_key_values=None, use_cache=True).past_key_values
            assert past[0][0].shape[1] == HKV
            for turn, toks in enumerate(turns):
                for t in range(toks.numel()):
                    out = model(input_ids=toks[t].view(1, 1), past_key_values=past, use_cache=True)
                    past = out.past_key_values
                    logits[k].append(out.logits[:, -1].float().cpu().numpy())
                torch.cuda.synchronize()
                if turn == 0:          # the prune event: tokens, and the heads ranked by the importance the decode steps added
                    new = cache.apply_token_pruning(past, 14, [m.attn_scores for m in mods])
                    assert new is not past
                    past = new
            kept.append(cache.ext.stats()["kept_heads"])
            ops.check_workspaces()
    finally:
        ops.set_decode_gqa(prev)
    # a head died in every layer, and both runs kept the same heads
    assert kept[0] == kept[1]
    assert [len(x) for x in kept[0]] == [7, 6]
    # the flagged run's steps took the grouped form — before the prune event (head importance alone) and after it (with the list)
    assert seen[0] and all(form for _, form in seen[0])
    assert any(has_list for has_list, _ in seen[0]) and any(not has_list for has_list, _ in seen[0])
    # ... the same stack without the keyword kept them on the per-query-head kernel
    assert seen[1] and not any(form for _, form in seen[1])
    worst = max(float(np.abs(a - b).max()) for a, b in zip(*logits))
    print(f"[gqa-heads-plugin] auto_graph={auto_graph}: {len(logits[0])} steps, max |logit difference| {worst:.4f}")
    for a, b in zip(*logits):
        np.testing.assert_allclose(a, b, **LOGIT_TOL)
