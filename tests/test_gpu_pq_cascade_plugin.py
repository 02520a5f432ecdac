"""The profiled decode step with the folded cascade importance (pq_profile + importance_mode="cascade" + pq_cascade=True, with
and without head pruning) through the plugin: captured by DecodeGraph and by auto_graph bit for bit against the eager loop, and
the reference's multi-turn caller protocol against the oracle replica (PARITY UNPINNED: oracle/spatten_oracle.py's
pq_decode_attention_profile -> every V row -> cascade_importance_accumulate of the final fp32 logits)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import test_gpu_e2e_protocol as e2e
from tests.test_gpu_graph_decode import HID, _HFStyleLM, _models, _TinyLM

pytestmark = pytest.mark.gpu

MODES = [dict(pq_threshold=0.05, pq_profile=(8, 8), importance_mode="cascade", pq_cascade=True),
         dict(pq_threshold=0.05, pq_profile=(6, 6), importance_mode="cascade", pq_cascade=True, head_keep=6)]


def _launched(ext):
    return [slice(None) if st.head_ids is None else st.head_ids.long() for st in ext.layers]


@pytest.mark.parametrize("kw", MODES)
def test_decode_graph_of_the_fused_step_equals_the_eager_loop(kw):
    """DecodeGraph over 17 tokens per turn, two turns with a prune event between them: every token's hidden state, stash
    (attn_scores), attention output, accumulator and refetch flags equal the eager loop's bit for bit; then the prune event
    (kept positions, kept heads, compacted caches, carried accumulators)."""
    from spatten_amd.graph import DecodeGraph
    dt = torch.bfloat16
    a, b, (cache_a, cache_b) = _models(dt, **kw)
    assert cache_b.ext.pq_cascade and not cache_b.ext.pq_local_v and cache_b.ext.graph_capable()
    g = torch.Generator(device="cuda").manual_seed(17)
    P, T = 180, 17
    x0 = torch.randn(1, P, HID, device="cuda", generator=g).to(dt)
    _, past_a = a(x0, None)
    _, past_b = b(x0, None)
    flagged = 0
    for turn in range(2):
        graph = DecodeGraph(lambda past, x: tuple(reversed(b(x, past))), past_b, horizon=T)
        for t in range(T):
            x = torch.randn(1, 1, HID, device="cuda", generator=g).to(dt)
            ya, past_a = a(x, past_a)
            yb = graph.step(x)
            graph.sync_scores()
            torch.cuda.synchronize()
            assert torch.equal(ya, yb), (turn, t, (ya.float() - yb.float()).abs().max().item())
            for ma, mb, la, lb, hk in zip(a.layers, b.layers, cache_a.ext.layers, cache_b.ext.layers, _launched(cache_a.ext)):
                assert ma.attn_scores.shape == mb.attn_scores.shape, (turn, t)
                assert torch.equal(ma.attn_scores[:, hk], mb.attn_scores[:, hk]), (turn, t)
                assert torch.equal(la.out, lb.out), (turn, t)
                assert torch.equal(la.need_lsb, lb.need_lsb), (turn, t)
                flagged += int(la.need_lsb.view(-1, la.need_lsb.numel())[:, hk].sum())
                if cache_a.ext.cascade:
                    assert torch.equal(la.acc[hk], lb.acc[hk]), (turn, t)
        assert graph.n_replays == T - 1
        past_b = graph.past_key_values
        coming = 6 + T
        hks = _launched(cache_a.ext)
        new_a = cache_a.apply_token_pruning(past_a, coming, [m.attn_scores for m in a.layers])
        new_b = cache_b.apply_token_pruning(past_b, coming, [m.attn_scores for m in b.layers])
        assert new_a is not past_a and new_b is not past_b
        for la, lb, hk in zip(cache_a.ext.layers, cache_b.ext.layers, hks):
            if cache_a.ext.cascade:
                assert torch.equal(la.acc[hk, :new_a[0][0].shape[2]], lb.acc[hk, :new_a[0][0].shape[2]])
            assert torch.equal(la.head_abs, lb.head_abs)
            assert (la.head_ids is None and lb.head_ids is None) or torch.equal(la.head_ids, lb.head_ids)
        for (ka, va), (kb, vb), la in zip(new_a, new_b, cache_a.ext.layers):
            kept = slice(None) if la.head_ids is None else la.head_ids.long()
            assert torch.equal(ka[:, kept], kb[:, kept]) and torch.equal(va[:, kept], vb[:, kept])
        if "head_keep" in kw:
            assert any(st.head_ids is not None for st in cache_b.ext.layers)
        xp = torch.randn(1, 6, HID, device="cuda", generator=g).to(dt)
        _, past_a = a(xp, new_a)
        _, past_b = b(xp, new_b)
    assert flagged > 0          # both the confident and the refetch branch ran


@pytest.mark.parametrize("kw", MODES)
def test_auto_graph_of_the_fused_step_equals_the_eager_loop(kw):
    """enable_spatten_llm(..., auto_graph=True) with pq_cascade: the reference's unchanged loop (three turns, prune events
    from m.attn_scores) replays one graph per token — and really captures it: tokens, logits, stashes and pruned caches equal the
    loop without auto_graph, bit for bit, and every single-token call after the first two of a turn is a replay."""
    from spatten_amd import enable_spatten_llm
    dt = torch.bfloat16
    torch.manual_seed(5)
    a, b = _HFStyleLM(dt), _HFStyleLM(dt)
    b.load_state_dict(a.state_dict())
    caches = []
    for m, auto in ((a, False), (b, True)):
        with contextlib.redirect_stdout(io.StringIO()):
            caches.append(enable_spatten_llm(m, 4, 40, 40, auto_graph=auto, **kw))

    def greedy_generate(model, input_ids, past_key_values, max_gen_len):          # run_spatten_llama.py:18-57
        outputs = model(input_ids=input_ids, past_key_values=past_key_values, use_cache=True)
        past_key_values = outputs.past_key_values
        pred = outputs.logits[:, -1, :].argmax(dim=-1).unsqueeze(1)
        generated, logits = [pred.item()], [outputs.logits[:, -1].clone()]
        for _ in range(max_gen_len - 1):
            outputs = model(input_ids=pred, past_key_values=past_key_values, use_cache=True)
            past_key_values = outputs.past_key_values
            pred = outputs.logits[:, -1, :].argmax(dim=-1).unsqueeze(1)
            generated.append(pred.item())
            logits.append(outputs.logits[:, -1].clone())
        return past_key_values, generated, logits

    def inference(model, kv_cache, prompts, max_gen_len):                         # run_spatten_llama.py:60-87
        past, trace = None, []
        for idx, ids in enumerate(prompts):
            if idx > 0:
                scores = [m.self_attn.attn_scores for m in model.layers]
                trace.append([s[:, hk].clone() for s, hk in zip(scores, _launched(kv_cache.ext))])
                n_prev = past[0][0].size(2)
                past = kv_cache.apply_token_pruning(past, ids.shape[1] + max_gen_len, scores)
                trace.append((n_prev, past[0][0].size(2)))
            past, gen, logits = greedy_generate(model, ids, past, max_gen_len)
            trace.append((gen, logits))
        return past, trace

    g = torch.Generator(device="cuda").manual_seed(21)
    prompts = [torch.randint(0, _TinyLM.VOCAB, (1, n), device="cuda", generator=g) for n in (90, 17, 23)]
    with torch.no_grad():
        past_a, tr_a = inference(a, caches[0], prompts, 18)
        past_b, tr_b = inference(b, caches[1], prompts, 18)
    for ea, eb in zip(tr_a, tr_b):
        if isinstance(ea, list):                             # the stashes the prune event ranks by
            assert all(torch.equal(x, y) for x, y in zip(ea, eb))
        elif isinstance(ea[0], int):
            assert ea == eb                                  # cache lengths before / after each prune
        else:
            assert ea[0] == eb[0]                            # the generated tokens
            assert all(torch.equal(x, y) for x, y in zip(ea[1], eb[1]))
    for (ka, va), (kb, vb), hk in zip(past_a, past_b, _launched(caches[0].ext)):
        assert torch.equal(ka[:, hk], kb[:, hk]) and torch.equal(va[:, hk], vb[:, hk])
    n = past_a[0][0].shape[2]
    for la, lb, hk in zip(caches[0].ext.layers, caches[1].ext.layers, _launched(caches[0].ext)):
        # (the buffers' capacities differ — the eager loop grows them with the cache, the graph sizes them for its slab: the live
        #  rows are compared)
        assert torch.equal(la.acc[hk, :n], lb.acc[hk, :n]), (la.acc.shape, lb.acc.shape)
        assert torch.equal(la.out, lb.out) and torch.equal(la.need_lsb, lb.need_lsb)
    graph = b._spatten_auto_graph["graph"]
    assert graph is not None and graph.n_replays == 18 - 1 - 1       # a real capture (a failed one falls back with no replays)
    assert caches[1].ext.pq_cascade and flagged_any(caches[0].ext)


def flagged_any(ext):
    return any(int(st.need_lsb.sum()) > 0 for st in ext.layers)


class PqCascadeReplica(e2e.ExtReplica):
    """ExtReplica + the profiled step at single-token calls: orc.pq_decode_attention_profile for logits, flags and the output
    over EVERY row of the quantised values; the stash (and the cascade accumulation) are the final fp32 logits."""

    def forward(self, ids, past):
        L, H, D = e2e.L, e2e.H, e2e.D
        B, q = ids.shape
        if q > 1:
            return super().forward(ids, past)
        P = past[0][0].shape[2]
        N = P + 1
        pos = np.tile(np.arange(P, N)[None], (B, 1))
        mask = orc.causal_mask(B, 1, N, "f32")
        x = self.emb[ids]
        new_past = []
        sp = lambda t: np.swapaxes(t.reshape(B, 1, H, D), 1, 2)
        kb, vb = self.pq_profile
        for i, w in enumerate(self.w):
            qh, kh, vh = sp(x @ w["q_proj"].T), sp(x @ w["k_proj"].T), sp(x @ w["v_proj"].T)
            kc, vc = np.concatenate([past[i][0], kh], 2), np.concatenate([past[i][1], vh], 2)
            cos, sin = orc.rope_table(N, D, "f32")
            qr = orc.apply_rotary_pos_emb_single(qh, cos, sin, pos, "f32")[:, :, 0]
            kr = orc.apply_rotary_pos_emb_single(kc, cos, sin, np.arange(N)[None], "f32")
            msb, lsb, scale = orc.pq_quantize(kr, bits=kb + 4)
            qv, vscale = orc.pq_quantize_values(vc, bits=vb)
            o, self.need[i], logits = orc.pq_decode_attention_profile(qr, msb, lsb, scale, qv, vscale, self.pq_threshold)
            o = np.asarray(o, np.float32).reshape(B, 1, H * D)
            if self.kept[i] is not None:
                o = o.reshape(B, 1, H, D).copy()
                o[:, :, np.setdiff1d(np.arange(H), self.kept[i])] = 0
                o = o.reshape(B, 1, H * D)
            self.head_abs[i] = self.head_abs[i] + orc.head_scores(o, H)
            stash = logits[:, :, None, :]
            self.stash[i] = stash
            if self.cascade:
                self.accumulate(i, stash, mask)
            x = x + o @ w["o_proj"].T
            new_past.append((kc, vc))
        return x @ self.lm.T, new_past


@pytest.mark.parametrize("mode", ["pq88+cascade", "head+pq66+cascade"])
def test_multi_turn_protocol_of_the_fused_step(mode):
    """The reference's caller protocol (three turns, prune events) through enable_spatten_llm with pq_cascade, fp32, GPU vs
    the oracle replica: generated tokens, logits, refetch flags, kept heads, kept token positions and the accumulators."""
    from spatten_amd import enable_spatten_llm
    L, H = e2e.L, e2e.H
    START, IMPORTANT, RECENT, MAX_GEN = e2e.START, e2e.IMPORTANT, e2e.RECENT, e2e.MAX_GEN
    torch.manual_seed(3)
    model = e2e.TinyLlama().cuda().float()
    for p in model.parameters():
        p.data.mul_(0.6)
    kw = dict(pq_threshold=0.06, pq_profile=(8, 8) if "pq88" in mode else (6, 6))
    if "head" in mode:
        kw["head_keep"] = 3
    ref = PqCascadeReplica(model, cascade=True, **kw)
    kv_cache = enable_spatten_llm(model, START, IMPORTANT, RECENT, importance_mode="cascade", pq_cascade=True, **kw)
    assert kv_cache.ext.pq_cascade
    flagged = 0
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, e2e.VOCAB, size=n)[None] for n in (38, 26, 31)]
    past_g = past_r = None
    for turn, prompt in enumerate(prompts):
        if turn > 0:
            space_needed = prompt.shape[1] + MAX_GEN
            Lc = past_r[0][0].shape[2]
            for i in range(L):        # accumulators of the launched heads agree before the prune (the last step folded first)
                live = np.arange(H) if ref.kept[i] is None else ref.kept[i]
                np.testing.assert_allclose(e2e.acc_of(kv_cache, i, Lc)[live], ref.acc[i][live, :Lc], rtol=2e-3, atol=2e-5)
            past_g = kv_cache.apply_token_pruning(past_g, space_needed, None)
            ref.select_heads()
            if "head" in mode:
                for i in range(L):
                    got = kv_cache.ext.layers[i].head_ids
                    got = np.arange(H) if got is None else got.cpu().numpy()
                    assert np.array_equal(got, ref.kept[i]), f"turn {turn} layer {i}: kept heads"
            assert Lc + space_needed > START + IMPORTANT + RECENT
            lo, hi = START, min(Lc - RECENT + space_needed, Lc)
            new_r = []
            for i in range(L):
                idx = orc.topk_window(ref.acc[i][:, :Lc], lo, hi, IMPORTANT)
                live = np.arange(H) if ref.kept[i] is None else ref.kept[i]
                assert np.array_equal(kv_cache.keep_indices[i].cpu().numpy()[live], idx[live]), f"turn {turn} layer {i}"
                idx_g = kv_cache.keep_indices[i].cpu().numpy()                     # follow the GPU for dead heads
                Kn, Vn = orc.kv_compact(past_r[i][0], past_r[i][1], idx_g, START, hi)
                a = ref.acc[i][:, :Lc]
                ref.acc[i] = np.concatenate([a[:, :START], np.take_along_axis(a, idx_g, 1), a[:, hi:]], 1)
                new_r.append((Kn, Vn))
            past_r = new_r
        tg, past_g, lg_ = e2e.greedy(lambda i, p: model(i, p), torch.from_numpy(prompt).cuda(), past_g,
                                     lambda a: torch.tensor(a, device="cuda"))
        tr, past_r, lr_ = e2e.greedy(ref.forward, prompt, past_r, lambda a: np.asarray(a))
        assert tg == tr, f"turn {turn}: generated tokens differ {tg} vs {tr}"
        np.testing.assert_allclose(lg_.cpu().numpy(), lr_, atol=5e-4, rtol=5e-4)
        for i in range(L):
            need_g = kv_cache.ext.layers[i].need_lsb.cpu().numpy().reshape(1, H).astype(bool)
            live = np.arange(H) if ref.kept[i] is None else ref.kept[i]
            assert np.array_equal(need_g[:, live], ref.need[i][:, live]), f"turn {turn} layer {i}: refetch flags"
            flagged += int(need_g[:, live].sum())
    assert kv_cache.n_pruned_total > 0 and flagged > 0
    if "head" in mode:
        assert all(k is not None and len(k) == 3 for k in ref.kept)
