"""The ragged prune event (spatten_prune_ragged, include/spatten.h) restated in numpy: the reference's rule
(kv_cache_token_pruning.py:46,59,80-82) applied SEQUENCE BY SEQUENCE at each sequence's own length, from the oracle's pieces —
orc.topk_window, orc.kv_compact, orc.rope_table / orc.apply_rotary_pos_emb_single — plus what the event adds: the zero fill of the
defined region and the accumulator row map with ``acc_heads``.  Test infrastructure (no GPU)."""
import numpy as np

from oracle import spatten_oracle as orc


def keep_rows(start, recent, k, num_coming):
    return start + k + recent - num_coming


def needs_pruning(n, start, recent, k, num_coming):
    return n + num_coming > start + k + recent


def reference(scores, Ks, Vs, lens, start, recent, k, num_coming, out_rows, dt, accs=None, acc_cols=0):
    """scores[l] [B, H, >=bound] fp32; Ks[l] / Vs[l] [B, H, >=bound, d] fp32 values of dtype ``dt``; accs[l] [B, A, >=bound] fp32.
    Returns dict(K, V, Kr [layers][B, H, out_rows, d], idx {(l, b): [H, k]} for pruned sequences, new_lens [B],
    acc [layers][B, A, acc_cols] or None)."""
    nl, (B, H, _, d) = len(Ks), Ks[0].shape
    keep = keep_rows(start, recent, k, num_coming)
    assert out_rows >= keep
    cos, sin = orc.rope_table(out_rows, d, dt)
    pos = np.arange(out_rows)[None, :]
    Kn = [np.zeros((B, H, out_rows, d), np.float32) for _ in range(nl)]
    Vn = [np.zeros((B, H, out_rows, d), np.float32) for _ in range(nl)]
    Krn = [np.zeros((B, H, out_rows, d), np.float32) for _ in range(nl)]
    An = None
    if accs is not None:
        A = accs[0].shape[1]
        assert A % H == 0 and acc_cols >= keep
        An = [np.zeros((B, A, acc_cols), np.float32) for _ in range(nl)]
    idxs, new_lens = {}, np.zeros(B, np.int32)
    for b, n in enumerate(lens):
        pruned = needs_pruning(n, start, recent, k, num_coming)
        new_lens[b] = keep if pruned else n
        for l in range(nl):
            Kb, Vb = Ks[l][b:b + 1, :, :n], Vs[l][b:b + 1, :, :n]
            if pruned:
                hi = n - recent + num_coming
                idx = orc.topk_window(scores[l][b, :, :n], start, hi, k)            # [H, k]
                idxs[(l, b)] = idx
                kk, vv = orc.kv_compact(Kb, Vb, idx, start, hi)
                rows = [np.concatenate([np.arange(start), idx[h], np.arange(hi, n)]) for h in range(H)]
            else:
                kk, vv = Kb, Vb
                rows = [np.arange(n)] * H
            m = kk.shape[2]
            assert m == new_lens[b] and m <= keep
            Kn[l][b, :, :m], Vn[l][b, :, :m] = kk[0], vv[0]
            if m:
                Krn[l][b, :, :m] = orc.apply_rotary_pos_emb_single(kk, cos, sin, pos[:, :m], dt)[0]
            if An is not None:
                g = An[l].shape[1] // H
                for a in range(An[l].shape[1]):
                    An[l][b, a, :m] = accs[l][b, a, rows[a // g]]
    return dict(K=Kn, V=Vn, Kr=Krn, idx=idxs, new_lens=new_lens, acc=An)


def make_scores(seed, layers, B, H, bound, lens, start, recent, k, num_coming):
    """fp32 scores with a planted TIE at the k-th value in head 0 (a run of equal values wider than what is left of k, so the lowest
    indices must win) and one NaN in head 1 (ranks largest), inside every pruned sequence's window."""
    out = []
    for l in range(layers):
        s = np.abs(orc.synth_normal(seed, 40 + l, (B, H, bound), "f32")).astype(np.float32)
        for b, n in enumerate(lens):
            if not needs_pruning(n, start, recent, k, num_coming):
                continue
            hi = n - recent + num_coming
            W = hi - start
            # head 0: the k - 2 largest are distinct and large, then a plateau of min(W - (k - 2), 6) equal values of which 2 are kept
            w = np.full(W, 0.25, np.float32) * np.linspace(0.1, 0.9, W, dtype=np.float32)
            order = (np.arange(W) * 7919) % W
            big = order[:max(k - 2, 0)]
            w[big] = 10.0 + np.arange(len(big), dtype=np.float32)
            rest = np.setdiff1d(np.arange(W), big)
            plateau = rest[::max(len(rest) // 6, 1)][:6]
            w[plateau] = 5.0
            s[b, 0, start:hi] = w
            if H > 1:
                s[b, 1, start + (W // 2)] = np.nan
        out.append(s)
    return out
