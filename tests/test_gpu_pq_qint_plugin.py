"""enable_spatten_llm(..., pq_profile=(8, 8), pq_query_bits=8) on the HF-4.33-style stack: the eager loop and auto_graph give
bit-identical logits, the captured graph really replays, and every layer's first decode step is judged against exact math
with the query that layer exported (tests/pq_qint_exact.py, as tests/test_gpu_pq_qint.py does).  Needs an MI355X."""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pq_qint_exact as qx
from tests.test_gpu_graph_decode import _HFStyleLM, _TinyLM
from tests.util import host

pytestmark = pytest.mark.gpu

THR, BITS, GEN = 0.05, 8, 12


def _check_first_step(model, cache, past, name):
    """Each layer's step against qint_exact: planes, exported query, fp32 MSB logits, stash, flags and output as the launch left
    them.  (The model-dtype rotated query is not observable here: the exported query stands in for it, so the quantisation
    itself is tests/test_gpu_pq_qint.py's to judge.)"""
    from spatten_amd import kv_slab
    for i, layer in enumerate(model.layers):
        slab = kv_slab.slab_of(past[i][0])
        N = past[i][0].shape[2]
        st = cache.ext.layers[i]
        planes = slab.pq.unpack(N)
        B, H = st.q_quant[1].shape
        d = st.q_quant[0].shape[2]
        q_int, q_scale = st.q_quant[0].cpu().numpy().astype(np.int64), st.q_quant[1].cpu().numpy()
        res = SimpleNamespace(q_int=q_int, q_scale=q_scale, msb_logit=slab.pq.msb_logit[:, :, :N].cpu().numpy(),
                              stash=host(layer.self_attn.attn_scores)[:, :, 0, :N], need=st.need_lsb.cpu().numpy().reshape(B, H),
                              out=host(st.out).reshape(B, H, d))
        assert np.abs(q_int).max() == qx.qmax(BITS) and (q_scale > 0).all(), f"{name} layer {i}: no query exported"
        qx.check_step(qx.query64(q_int, q_scale), planes, "bf16", BITS, THR, res, only=("msb_logit", "stash", "flags", "out"),
                      name=f"{name} layer {i}")


def test_plugin_qint_eager_and_auto_graph_agree_and_first_step_is_exact():
    from spatten_amd import enable_spatten_llm
    dt = torch.bfloat16
    torch.manual_seed(5)
    a, b = _HFStyleLM(dt), _HFStyleLM(dt)
    b.load_state_dict(a.state_dict())
    caches = []
    for m, auto in ((a, False), (b, True)):
        with contextlib.redirect_stdout(io.StringIO()):
            caches.append(enable_spatten_llm(m, 4, 40, 40, auto_graph=auto, pq_threshold=THR, pq_profile=(8, 8),
                                             pq_query_bits=BITS))
    assert all(c.ext.pq_query_bits == BITS for c in caches)
    g = torch.Generator(device="cuda").manual_seed(21)
    ids = torch.randint(0, _TinyLM.VOCAB, (1, 90), device="cuda", generator=g)
    logits = [[], []]
    flagged = 0
    with torch.no_grad():
        for k, (model, cache) in enumerate(zip((a, b), caches)):
            out = model(input_ids=ids, past_key_values=None, use_cache=True)
            past = out.past_key_values
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
    assert flagged > 0


def test_plugin_qint_keyword_is_refused_where_it_cannot_run():
    from spatten_amd import enable_spatten_llm
    m = _HFStyleLM(torch.bfloat16)
    for kw in (dict(pq_threshold=0.1, pq_profile=(6, 6)), dict(pq_threshold=0.1),
               dict(pq_threshold=0.1, pq_profile=(8, 8), local_v_keep=0.5)):
        with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
            enable_spatten_llm(m, 4, 40, 40, pq_query_bits=8, **kw)
