"""The final fold of the decode step — the row groups of a wave reduced with a reduce-scatter over the permlane swaps, the
waves folded through one LDS hop — at the shapes where it can go wrong: WHO holds WHICH element (every head dim / lane
layout, both teams) and EMPTY rows or waves (caches of 1 .. 641 rows cut into 1, 2 or 8 splits; a single dominant row).

Every case is checked twice: against the exact-math oracle at the decode tests' tolerances, and BIT FOR BIT against what the
commit before the fold was rewritten produced (tests/golden/decode_fold_parent.npz, written by
tools/make_decode_fold_golden.py from the case list below: a missing entry fails the test).  Needs an MI355X."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.util import OUT_TOL, TORCH_DT, attn_inputs, check_stash, dev, host

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_fold_parent.npz")
B, H = 1, 2
KV_LENS = (1, 7, 9, 63, 65, 300, 641)
SPLITS = (1, 2, 8)
# (dtype, head dim, team): d = 128 in 16 bits runs on 512 or 256 threads; the others have one team (LPR = 4, fp32, LPR = 16)
GROUPS = [("bf16", 128, 512), ("bf16", 128, 256), ("f16", 128, 512), ("f16", 128, 256),
          ("bf16", 64, 0), ("f32", 128, 0), ("bf16", 256, 0)]
DOMINANT = [("bf16", 128, team, 300, 137, ns) for team in (512, 256) for ns in (1, 2)]   # (.., kv_len, dominant row, splits)
CHAIN_LENS = (9, 300)
CHAIN_LAYERS = 3


def group_cases(dt, d, team):
    return [(f"{dt}_d{d}_t{team}_n{n}_s{ns}", n, ns) for n in KV_LENS for ns in SPLITS]


def dominant_key(dt, d, team, n, row, ns):
    return f"dom_{dt}_d{d}_t{team}_n{n}_r{row}_s{ns}"


def chain_key(n, layer):
    return f"chain_bf16_d128_n{n}_l{layer}"


def all_keys():
    """Every golden entry the tests read (the generator writes exactly these)."""
    keys = []
    for g in GROUPS:
        keys += [f"{k}__{part}" for k, _, _ in group_cases(*g) for part in ("out", "stash", "lse")]
    keys += [f"{dominant_key(*c)}__{part}" for c in DOMINANT for part in ("out", "stash", "lse")]
    keys += [f"{chain_key(n, l)}__{part}" for n in CHAIN_LENS for l in range(CHAIN_LAYERS) for part in ("out", "stash")]
    return keys


def bits(t):
    """The tensor's bit pattern as a numpy integer array (what the golden file stores: -0 / NaN payloads included)."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def oracle_table(n, d, dt):
    cos, sin = orc.rope_table(n, d, dt)
    return dev(cos[:, : d // 2], dt), dev(sin[:, : d // 2], dt)


@functools.lru_cache(maxsize=None)
def inputs(dt, d, n, seed=None):
    return attn_inputs(B, H, H, d, n - 1, 1, dt, seed=900 + n if seed is None else seed)      # shared: never written to


@functools.lru_cache(maxsize=None)
def oracle(dt, d, n):
    q, k, v, past = inputs(dt, d, n)
    o, stash, _ = orc.attention_core(q, k, v, None if past is None else past[0], None if past is None else past[1],
                                     np.full((B, 1), n - 1), None, dt)
    return o, stash


def run_step(q, k, v, past, dt, n_splits, pos_q=None):
    """One fused decode step with append, stash and (max, sum): device tensors out [B,H*d], stash [B,H,N], lse [B,H,2]."""
    from spatten_amd import ops
    d = q.shape[-1]
    P = 0 if past is None else past[0].shape[2]
    N, cap = P + 1, P + 4
    tdt = TORCH_DT[dt]
    kc, krc, vc = (torch.full((B, H, cap, d), float("nan"), dtype=tdt, device="cuda") for _ in range(3))
    if P:
        kc[:, :, :P], vc[:, :, :P] = dev(past[0], dt), dev(past[1], dt)
    cos, sin = oracle_table(N + 5, d, dt)
    ops.build_shadow(kc, krc, 0, P, cos, sin)
    scores = torch.full((B, H, N + 2), float("nan"), dtype=tdt, device="cuda")
    lse = torch.zeros(B, H, 2, dtype=torch.float32, device="cuda")
    out = ops.attn_decode(dev(q[:, :, 0], dt), kc, krc, vc, N, cos, sin, P if pos_q is None else pos_q,
                          k_new=dev(k[:, :, 0], dt), v_new=dev(v[:, :, 0], dt), scores=scores, lse=lse, n_splits=n_splits)
    torch.cuda.synchronize()
    assert torch.isnan(scores[:, :, N:].float()).all(), "stash written past kv_len"
    for t in (kc, krc, vc):
        assert torch.isnan(t[:, :, N:].float()).all(), "cache written past kv_len"
    return out, scores[:, :, :N].contiguous(), lse


def with_team(team, fn):
    from spatten_amd import ops
    if not team:
        return fn()
    prev = ops.set_decode_team(team)
    try:
        return fn()
    finally:
        ops.set_decode_team(prev)


def run_group(dt, d, team):
    """{key: (out, stash, lse)} of one group's cases."""
    def go():
        return {key: run_step(*inputs(dt, d, n), dt, ns) for key, n, ns in group_cases(dt, d, team)}
    return with_team(team, go)


def dominant_inputs(dt, d, n, row):
    """The query is 8 x the key of `row` and sits at that row's position: that logit is 8 |k|^2 / sqrt(d) ~ 90, the others
    8 k.k' / sqrt(d) ~ N(0, 8^2)."""
    q, k, v, past = inputs(dt, d, n, seed=77)
    q = np.ascontiguousarray(8.0 * past[0][:, :, row:row + 1])
    return q, k, v, past


def run_dominant(dt, d, team, n, row, ns):
    return with_team(team, lambda: run_step(*dominant_inputs(dt, d, n, row), dt, ns, pos_q=row))


def run_chain(n):
    """Three layers of one token, chained and per layer, on two copies of the planes: ([chain (out, stash)], [per-layer])."""
    from spatten_amd import ops
    dt, d, L = "bf16", 128, CHAIN_LAYERS
    tdt, P, cap = TORCH_DT[dt], n - 1, n + 7
    cos, sin = oracle_table(cap + 8, d, dt)
    ins = [inputs(dt, d, n, seed=500 + 10 * l) for l in range(L)]
    sets = []
    for _ in range(2):
        planes = []
        for q, k, v, past in ins:
            kc = torch.zeros(B, H, cap, d, dtype=tdt, device="cuda")
            vc, krc = torch.zeros_like(kc), torch.zeros_like(kc)
            kc[:, :, :P], vc[:, :, :P] = dev(past[0], dt), dev(past[1], dt)
            ops.build_shadow(kc, krc, 0, P, cos, sin)
            planes.append((kc, krc, vc))
        sets.append(planes)
    qs = [dev(i[0][:, :, 0], dt) for i in ins]
    ks = [dev(i[1][:, :, 0], dt) for i in ins]
    vs = [dev(i[2][:, :, 0], dt) for i in ins]
    outs = [[torch.zeros(B, H * d, dtype=tdt, device="cuda") for _ in range(L)] for _ in range(2)]
    stash = [[torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(L)] for _ in range(2)]
    chain = ops.DecodeChain(qs, [p[0] for p in sets[0]], [p[1] for p in sets[0]], [p[2] for p in sets[0]], outs[0],
                            k_new=ks, v_new=vs, scores=stash[0])
    chain(n, cos, sin, P)
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    for l in range(L):
        kc, krc, vc = sets[1][l]
        ops.attn_decode(qs[l], kc, krc, vc, n, cos, sin, P, k_new=ks[l], v_new=vs[l], scores=stash[1][l], out=outs[1][l],
                        workspace=ws)
    torch.cuda.synchronize()
    chain.check()
    for l in range(L):
        for a, b_ in zip(sets[0][l], sets[1][l]):
            assert torch.equal(a, b_), (l, "planes")
    return [[(outs[s][l], stash[s][l][:, :, :n].contiguous()) for l in range(L)] for s in range(2)], ins


@functools.lru_cache(maxsize=None)
def parent():
    return np.load(GOLDEN, allow_pickle=False)


def assert_parent_bits(key, **parts):
    g = parent()
    for part, t in parts.items():
        want = g[f"{key}__{part}"]                    # KeyError = a case without a golden entry: a failure, never a skip
        got = bits(t)
        assert got.shape == want.shape and got.dtype == want.dtype, (key, part, got.shape, want.shape)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), \
            (key, part, f"{int((got != want).sum())} of {got.size} words differ from the parent commit")


def test_golden_file_holds_exactly_the_case_list():
    assert sorted(parent().files) == sorted(all_keys())


@pytest.mark.parametrize("dt,d,team", GROUPS)
def test_fold_vs_oracle_and_parent_bits(dt, d, team):
    res = run_group(dt, d, team)
    assert len(res) == len(KV_LENS) * len(SPLITS)
    for key, n, ns in group_cases(dt, d, team):
        out, stash, lse = res[key]
        o, st = oracle(dt, d, n)
        np.testing.assert_allclose(host(out)[:, None, :], o, err_msg=key, **OUT_TOL[dt])
        check_stash(host(stash)[:, :, None, :], st, dt, key)
        p = orc.softmax_probs(st)
        np.testing.assert_allclose(1.0 / host(lse)[:, :, 1], p[:, :, 0].max(-1), rtol=2e-2, err_msg=key)
        assert_parent_bits(key, out=out, stash=stash, lse=lse)


@pytest.mark.parametrize("case", DOMINANT, ids=lambda c: dominant_key(*c))
def test_fold_with_one_dominant_row(case):
    dt, d, team, n, row, ns = case
    q, k, v, past = dominant_inputs(dt, d, n, row)
    o, st, _ = orc.attention_core(q, k, v, past[0], past[1], np.full((B, 1), row), None, dt)
    # the premise: the row's logit stands so far above every other (> 30: 300 x exp(-30) ~ 3e-11) that the others vanish
    # from the fp32 sum and the rescale of every wave without that row is ~ 0
    top = np.sort(st[:, :, 0], axis=-1)
    assert np.all(st[:, :, 0].argmax(-1) == row) and np.all(top[..., -1] - top[..., -2] > 30.0)
    out, stash, lse = run_dominant(*case)
    key = dominant_key(*case)
    np.testing.assert_allclose(host(out)[:, None, :], o, err_msg=key, **OUT_TOL[dt])
    check_stash(host(stash)[:, :, None, :], st, dt, key)
    np.testing.assert_allclose(host(lse)[:, :, 1], 1.0, rtol=1e-6, err_msg=key)        # the sum is the dominant row's exp(0)
    assert_parent_bits(key, out=out, stash=stash, lse=lse)


@pytest.mark.parametrize("n", CHAIN_LENS)
def test_three_layer_chain_equals_per_layer_launches_on_short_caches(n):
    (chained, per_layer), ins = run_chain(n)
    for l in range(CHAIN_LAYERS):
        assert torch.equal(chained[l][0], per_layer[l][0]), (l, "out")
        assert torch.equal(chained[l][1], per_layer[l][1]), (l, "stash")
        q, k, v, past = ins[l]
        o, st, _ = orc.attention_core(q, k, v, past[0], past[1], np.full((B, 1), n - 1), None, "bf16")
        np.testing.assert_allclose(host(chained[l][0])[:, None, :], o, err_msg=f"layer {l}", **OUT_TOL["bf16"])
        check_stash(host(chained[l][1])[:, :, None, :], st, "bf16", f"layer {l}")
        assert_parent_bits(chain_key(n, l), out=chained[l][0], stash=chained[l][1])
