"""The attention kernels against EXACT softmax attention in the logit regimes real Llama attention has (tests/regimes.py):
attention sinks, logit spreads of std 4 and 12, a maximum that moves in every tile, a maximum inside one split with every
other split underflowing, the appended row as the maximum or far below, masked key ranges and fully masked rows.

Criterion: per (batch, query row, head) err(kernel, exact) <= C * err(oracle, exact) + 1 ulp, C = 2; the fp32-logit
prefill forms in addition no further from exact than the reference-numerics kernel + 1 ulp.  Stash rule (tests/util.py
check_stash) everywhere a stash is written.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import regimes as rg
from tests.test_gpu_decode import oracle_table
from tests.test_gpu_prefill import run_prefill
from tests.util import OUT_TOL, TORCH_DT, check_stash, dev, host

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(B, H, Hkv, d, P, ql, dt, regime, mask_kinds=None, seed=17):
    mask = None
    if mask_kinds is not None:
        mask = rg.decode_mask(B, P + 1, dt, mask_kinds)
    elif ql > 1:
        mask = orc.causal_mask(B, ql, P + ql, dt)
    return rg.make_case(B, H, Hkv, d, P, ql, dt, regime if isinstance(regime, str) else list(regime), seed, mask=mask)


def _decode(cs, n_splits=0, stash=True):
    """One ops.attn_decode step of the case (appending its new row); returns (out [B,1,H*d], stash [B,H,1,N] or None)."""
    from spatten_amd import ops
    B, H, Hkv, d, P, N, dt = cs.B, cs.H, cs.Hkv, cs.d, cs.P, cs.N, cs.dt
    tdt = TORCH_DT[dt]
    cap = N + 3
    kc = torch.zeros(B, Hkv, cap, d, dtype=tdt, device="cuda")
    vc, krc = torch.zeros_like(kc), torch.zeros_like(kc)
    if P:
        kc[:, :, :P], vc[:, :, :P] = dev(cs.past[0], dt), dev(cs.past[1], dt)
    cos, sin = oracle_table(N + 5, d, dt)
    ops.build_shadow(kc, krc, 0, P, cos, sin)
    scores = torch.full((B, H, N), float("nan"), dtype=tdt, device="cuda") if stash else None
    mask = None if cs.mask is None else dev(np.ascontiguousarray(cs.mask[:, 0, 0]), dt)
    out = ops.attn_decode(dev(cs.q[:, :, 0], dt), kc, krc, vc, N, cos, sin, P, k_new=dev(cs.k[:, :, 0], dt),
                          v_new=dev(cs.v[:, :, 0], dt), mask=mask, scores=scores, n_splits=n_splits)
    torch.cuda.synchronize()
    return host(out)[:, None], (None if scores is None else host(scores)[:, :, None])


def _check(cs, out, st=None, name=""):
    rg.check_out_exact(out, cs.out, cs.exact, cs.dt, cs.d, name=name)
    if st is not None:
        check_stash(st, cs.stash, cs.dt, name)
    if cs.regimes is not None and all(r == "flat" for r in cs.regimes):     # the control: today's tolerance still holds
        np.testing.assert_allclose(out, cs.out, err_msg=name, **OUT_TOL[cs.dt])


# ---- per-layer decode (decode_body.h: the appended row's own path, the split merge) ---------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("regime", rg.REGIMES)
def test_decode_regimes_c2_length(dt, regime):
    """2081 rows (C2), 8 heads, d 128: auto / 1 / 3 / 7 splits with a stash, auto without one, both attention teams."""
    from spatten_amd import ops
    cs = _case(1, 8, 8, 128, 2080, 1, dt, regime)
    for ns in (0, 1, 3, 7):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"{regime} ns={ns}")
    out, _ = _decode(cs, 0, stash=False)
    _check(cs, out, None, f"{regime} no stash")
    prev = ops.set_decode_team(256)
    try:
        for ns in (0, 1):
            out, st = _decode(cs, ns)
            _check(cs, out, st, f"{regime} team 256 ns={ns}")
    finally:
        ops.set_decode_team(prev)


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("regime", ["sink24", "new_max", "rising", "split_winner", "large12"])
def test_decode_regimes_head_dims(d, regime):
    cs = _case(1, 4, 2, d, 2080, 1, "bf16", regime)
    for ns in (0, 3, 7):
        out, st = _decode(cs, ns, stash=ns != 7)
        _check(cs, out, st, f"d={d} {regime} ns={ns}")


@pytest.mark.parametrize("regime", rg.REGIMES)
def test_decode_regimes_short_rows(regime):
    cs = _case(2, 4, 4, 128, 128, 1, "bf16", regime)
    for ns in (0, 1, 3, 7):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"129 rows {regime} ns={ns}")


@pytest.mark.parametrize("dt,regime", [("bf16", "rising"), ("bf16", "split_winner"), ("f16", "large12"), ("bf16", "sink24")])
def test_decode_regimes_c5_length(dt, regime):
    """8190 rows (C5): pipelined tiles, long chunks, the maximum in the last split / one split winning."""
    cs = _case(1, 2, 2, 128, 8189, 1, dt, regime)
    for ns in (0, 7):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"8190 rows {regime} ns={ns}")


@pytest.mark.parametrize("pair", [("sink24", "rising"), ("new_max", "large12"), ("split_winner", "flat"), ("new_min", "sink8")])
def test_decode_regimes_differ_per_batch_row(pair):
    cs = _case(2, 8, 8, 128, 2080, 1, "bf16", pair)
    for ns in (0, 3):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"{pair} ns={ns}")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_decode_masked_ranges_and_fully_masked_rows(dt):
    """Batch row 0: keys [N/4, 3N/4) masked (whole splits at 3 / 7 splits); row 1: every key masked (left padding): the
    reference's uniform average over the keys, not NaN or zeros; row 2 unmasked, over sink logits."""
    cs = _case(3, 4, 4, 128, 2080, 1, dt, "sink8", ("range", "full", "none"))
    want_full = cs.vc[1].astype(np.float64).mean(1).reshape(1, -1)
    np.testing.assert_allclose(cs.exact[1], want_full, rtol=1e-12, atol=1e-12)
    for ns in (0, 1, 3, 7):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"masked ns={ns}")


# ---- the chained launch against exact math (static and device-length forms) ----------------------------------------
@pytest.mark.parametrize("dt,regime", [("bf16", "sink24"), ("bf16", "rising"), ("f16", "split_winner"), ("bf16", "large12"),
                                       ("bf16", "new_max")])
def test_chain_regimes_against_exact(dt, regime):
    from spatten_amd import ops
    cs = _case(1, 8, 8, 128, 2080, 1, dt, regime)
    B, H, d, P, N = cs.B, cs.H, cs.d, cs.P, cs.N
    tdt = TORCH_DT[dt]
    cap = N + 63
    cos, sin = oracle_table(cap + 8, d, dt)
    for dyn in (False, True):
        L = 2
        planes = []
        for _ in range(L):
            kc = torch.zeros(B, H, cap, d, dtype=tdt, device="cuda")
            vc, krc = torch.zeros_like(kc), torch.zeros_like(kc)
            kc[:, :, :P], vc[:, :, :P] = dev(cs.past[0], dt), dev(cs.past[1], dt)
            ops.build_shadow(kc, krc, 0, P, cos, sin)
            planes.append((kc, krc, vc))
        qs = [dev(cs.q[:, :, 0], dt) for _ in range(L)]
        ks = [dev(cs.k[:, :, 0], dt) for _ in range(L)]
        vs = [dev(cs.v[:, :, 0], dt) for _ in range(L)]
        outs = [torch.zeros(B, H * d, dtype=tdt, device="cuda") for _ in range(L)]
        stash = [torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(L)]
        chain = ops.DecodeChain(qs, [p[0] for p in planes], [p[1] for p in planes], [p[2] for p in planes], outs, k_new=ks,
                                v_new=vs, scores=stash)
        if dyn:
            step = ops.StepState(cos, sin)
            step.set(P, P - 1)
            step.advance()
            chain(cap, cos, sin, 0, step=step)
        else:
            chain(N, cos, sin, P)
        torch.cuda.synchronize()
        chain.check()
        for l in range(L):
            _check(cs, host(outs[l])[:, None], host(stash[l][:, :, :N])[:, :, None], f"chain dyn={dyn} layer {l} {regime}")


# ---- the grouped-query step on the matrix cores ---------------------------------------------------------------------
@pytest.fixture
def gqa_forced():
    from spatten_amd import ops
    prev = ops.set_decode_gqa(1)
    yield
    ops.set_decode_gqa(prev)


@pytest.mark.parametrize("shape", [(1, 32, 8), (2, 12, 4), (1, 64, 2)])
@pytest.mark.parametrize("P", [332, 2099])
@pytest.mark.parametrize("regime", ["sink24", "new_max", "rising", "split_winner", "large12"])
def test_gqa_regimes(gqa_forced, shape, P, regime):
    B, H, Hkv = shape
    cs = _case(B, H, Hkv, 128, P, 1, "bf16", regime)
    for ns in (0, 1, 3, 7):
        out, st = _decode(cs, ns)
        _check(cs, out, st, f"gqa {shape} {regime} ns={ns}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gqa_regimes_16384_rows(gqa_forced, dt):
    cs = _case(1, 32, 8, 128, 16383, 1, dt, "large12" if dt == "bf16" else "rising")
    out, st = _decode(cs, 0)
    _check(cs, out, st, "gqa 16384 rows")


# ---- prefill: rows leg, flash kernel, transposing-read form, Vt pre-pass form, key-split turn prefill -----------------
PREFILL_FORMS = {
    "rows_f32": ("f32", 128, 1, 2, 2, 300, 40),
    "rows_q8": ("bf16", 128, 1, 4, 2, 700, 5),
    "rows_d256": ("bf16", 256, 1, 2, 2, 200, 64),
    "flash": ("bf16", 128, 2, 4, 2, 300, 200),
    "flash_d64": ("f16", 64, 1, 4, 4, 77, 512),
    "transposing": ("bf16", 128, 1, 4, 4, 700, 300),
    "transposing_prompt": ("bf16", 128, 1, 2, 2, 0, 2304),
    "vt_prepass": ("bf16", 128, 1, 2, 2, 300, 700),
    "key_split": ("bf16", 128, 1, 8, 8, 2000, 40),
    "key_split_gqa": ("bf16", 128, 1, 8, 2, 1500, 300),
}


def _prefill_all(cs, name):
    """numerics reference / fast / auto, each with and without a stash (causal flag, no mask read)."""
    args = (cs.q, cs.k, cs.v, cs.past, cs.dt)
    ref, _, _ = run_prefill(*args, causal=True, stash=False, numerics="reference")
    _check(cs, ref, None, f"{name} reference")
    _, st, _ = run_prefill(*args, causal=True, stash=True, numerics="reference")
    check_stash(st, cs.stash, cs.dt, f"{name} reference stash")
    fast, _, _ = run_prefill(*args, causal=True, stash=False, numerics="fast")
    _check(cs, fast, None, f"{name} fast")
    if cs.dt != "f32":
        rg.check_fast_vs_reference(fast, ref, cs.exact, cs.dt, cs.d, name=f"{name} fast vs reference")
    auto, _, _ = run_prefill(*args, causal=True, stash=False, numerics="auto")
    assert np.array_equal(auto, fast), name
    for num in ("fast", "auto"):
        o, st, _ = run_prefill(*args, causal=True, stash=True, numerics=num)
        _check(cs, o, st, f"{name} {num} with a stash")


@pytest.mark.parametrize("form", ["flash", "key_split", "transposing"])
@pytest.mark.parametrize("regime", [r for r in rg.REGIMES if r not in rg.DECODE_ONLY])
def test_prefill_regimes_main_forms(form, regime):
    dt, d, B, H, Hkv, P, ql = PREFILL_FORMS[form]
    _prefill_all(_case(B, H, Hkv, d, P, ql, dt, regime), f"{form} {regime}")


@pytest.mark.parametrize("form", ["rows_f32", "rows_q8", "rows_d256", "flash_d64", "transposing_prompt", "vt_prepass",
                                  "key_split_gqa"])
@pytest.mark.parametrize("regime", ["sink24", "rising", "large12"])
def test_prefill_regimes_other_forms(form, regime):
    dt, d, B, H, Hkv, P, ql = PREFILL_FORMS[form]
    _prefill_all(_case(B, H, Hkv, d, P, ql, dt, regime), f"{form} {regime}")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_prefill_masked_key_range_and_left_padding(dt):
    """Explicit mask: causal + keys [100, 228) masked for every query + left padding of 13 tokens in batch row 1 (its first 13
    query rows see no key: the uniform average)."""
    B, H, Hkv, d, P, ql = 2, 4, 2, 128, 300, 200
    N = P + ql
    mask = rg.prefill_mask(B, ql, N, dt, [0, 13], 100, 228)
    cs = rg.make_case(B, H, Hkv, d, P, ql, dt, "sink8", 23, mask=mask)
    got = {}
    for num in ("reference", "fast"):
        for stash in (False, True):
            o, st, _ = run_prefill(cs.q, cs.k, cs.v, cs.past, dt, mask=mask[:, 0], stash=stash, numerics=num)
            _check(cs, o, st, f"masked {num} stash={stash}")
            got[num, stash] = o
    if dt != "f32":
        rg.check_fast_vs_reference(got["fast", False], got["reference", False], cs.exact, dt, d, name="masked")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_prefill_deferred_rescale_spikes_fp32_logits(dt):
    """test_prefill_deferred_rescale_spikes' construction (keys whose logits jump by more and by less than the deferral
    threshold at different tiles) through the fp32-logit forms (numerics fast / auto, the default without a stash)."""
    from tests.util import attn_inputs
    B, H, Hkv, d, P, ql = 1, 2, 2, 128, 768, 256
    q, k, v, past = attn_inputs(B, H, Hkv, d, P, ql, dt, seed=4242)
    N = P + ql
    rng = np.random.default_rng(7)
    a = orc.round_dt((6.0 * (0.5 + rng.random((B, H, ql)))).astype(np.float32), dt)
    q[..., 63] = a
    q[..., 127] = a
    kc = np.concatenate([past[0], k], 2)
    kc[..., 63] = 0
    kc[..., 127] = 0
    for pos, b in ((40, 4.0), (300, 9.0), (430, 11.0), (700, 22.0), (850, 23.5)):
        kc[:, :, pos, 63] = b
        kc[:, :, pos, 127] = b
    kc = orc.round_dt(kc, dt)
    past = (kc[:, :, :P], past[1])
    k = kc[:, :, P:]
    cs = rg.case_from_inputs(q, k, v, past, orc.causal_mask(B, ql, N, dt), dt)
    assert np.diff(np.sort(cs.stash[0, 0, 0, [40, 300, 430, 700]])).max() > 8.0
    ref, _, _ = run_prefill(q, k, v, past, dt, causal=True, stash=False, numerics="reference")
    _check(cs, ref, None, "spikes reference")
    for num in ("fast", "auto"):
        o, _, _ = run_prefill(q, k, v, past, dt, causal=True, stash=False, numerics=num)
        _check(cs, o, None, f"spikes {num}")
        rg.check_fast_vs_reference(o, ref, cs.exact, dt, d, name=f"spikes {num}")
