"""CPU side of the logit-regime tests (tests/regimes.py): the exact reference agrees with the oracle and with torch's softmax,
every regime generator produces its regime, the numpy emulation of the kernels' arithmetic passes the exact criterion in
every regime while each seeded fault fails it, and the chained decode's host validation refuses bad layer sets."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import regimes as rg
from tests.util import OUT_TOL

D = 128


@pytest.mark.parametrize("ql,P,Hkv", [(1, 700, 4), (40, 90, 2)])
def test_attention_exact_agrees_with_the_f32_oracle_and_torch_softmax(ql, P, Hkv):
    B, H = 2, 4
    mask = orc.causal_mask(B, ql, P + ql, "f32") if ql > 1 else None
    cs = rg.make_case(B, H, Hkv, D, P, ql, "f32", "flat", 31, mask=mask)
    np.testing.assert_allclose(cs.exact, cs.out, atol=1e-6, rtol=0)
    # torch in float64 over the same rotated inputs
    qr, kr, v = (torch.from_numpy(x.astype(np.float64)) for x in (cs.qr, cs.kr, cs.vc))
    kr, v = kr.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    s = qr @ kr.transpose(2, 3) / D ** 0.5
    np.testing.assert_allclose(cs.logits, s.numpy(), rtol=1e-12, atol=1e-12)
    if mask is not None:
        s = s.masked_fill(torch.from_numpy(mask <= orc.finfo_min("f32") / 2), float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, ql, H * D).numpy()
    np.testing.assert_allclose(cs.exact, o, rtol=1e-12, atol=1e-13)


def test_attention_exact_fully_masked_row_is_the_uniform_average():
    B, H, N = 1, 2, 300
    cs = rg.make_case(B, H, H, D, N - 1, 1, "bf16", "sink24", 3, mask=rg.decode_mask(B, N, "bf16", ["full"]))
    want = cs.vc.astype(np.float64).mean(2).reshape(B, 1, H * D)
    np.testing.assert_allclose(cs.exact, want, rtol=1e-12, atol=1e-12)
    # the reference's own answer is that average too (all logits round to finfo_min)
    np.testing.assert_allclose(cs.out, want, atol=2e-2)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("regime", rg.REGIMES)
def test_decode_regime_generators_produce_their_regime(dt, regime):
    # make_case asserts the regime from the oracle's stash; 8190 rows: the rotated-space construction holds at long positions
    rg.make_case(1, 2, 2, D, 2080, 1, dt, regime, 7)
    if dt == "bf16":
        rg.make_case(1, 2, 1, 64, 8189, 1, dt, regime, 8)


@pytest.mark.parametrize("regime", [r for r in rg.REGIMES if r not in rg.DECODE_ONLY])
def test_prefill_regime_generators_produce_their_regime(regime):
    B, ql, P = 1, 96, 200
    rg.make_case(B, 4, 2, D, P, ql, "bf16", regime, 9, mask=orc.causal_mask(B, ql, P + ql, "bf16"))


def test_a_regime_generator_refuses_a_missing_regime():
    st = np.zeros((2, 1, 500), np.float32)
    with pytest.raises(AssertionError):
        rg.assert_regime(st, "sink8", 500)
    with pytest.raises(AssertionError):
        rg.assert_regime(st, "split_winner", 500)


# ---- the emulated kernels: the criterion holds for the documented arithmetic and catches seeded faults --------------
_CASES = {}


def _case(dt, regime, mask_kinds=None):
    key = (dt, regime, mask_kinds)
    if key not in _CASES:
        B = 1 if mask_kinds is None else len(mask_kinds)
        mask = None if mask_kinds is None else rg.decode_mask(B, 2081, dt, mask_kinds)
        _CASES[key] = rg.make_case(B, 8, 8, D, 2080, 1, dt, regime, 11, mask=mask)   # C2 decode geometry, 8 heads
    return _CASES[key]


def _ok(got, cs):
    return not (rg.exact_excess(got, cs.out, cs.exact, cs.dt, D) > 0).any()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_emulated_kernel_arithmetic_passes_the_exact_criterion_in_every_regime(dt):
    """Reference-numerics logits and fp32 logits, 1 / 3 / 7 splits, deferred or immediate rescale: all within
    C * err(oracle) + 1 ulp; the fp32-logit form within the reference-numerics form's error + 1 ulp."""
    for regime in rg.REGIMES:
        cs = _case(dt, regime)
        for S in (1, 3, 7):
            ref = rg.emulate_kernel(cs, "reference", S)
            rg.check_out_exact(ref, cs.out, cs.exact, dt, D, name=f"{regime} reference S={S}")
            for defer in (False, True):
                fast = rg.emulate_kernel(cs, "fast", S, defer=defer)
                rg.check_out_exact(fast, cs.out, cs.exact, dt, D, name=f"{regime} fast S={S}")
                if dt != "f32":           # (f32 logits ARE fp32: the two forms differ by summation order only)
                    rg.check_fast_vs_reference(fast, ref, cs.exact, dt, D, name=f"{regime} S={S}")
    cs = _case(dt if dt != "f16" else "bf16", "flat", ("range", "full"))
    rg.check_out_exact(rg.emulate_kernel(cs, "reference", 3), cs.out, cs.exact, cs.dt, D, name="masked")


def test_the_calibration_of_c():
    """C = 2 against the largest ratio the emulated arithmetic reaches (<= 1.4 reference numerics, fp32 logits
    below the oracle's own error): the ratio err(emulated) / err(oracle) with the one-ulp allowance taken off."""
    worst = {"reference": 0.0, "fast": 0.0}
    for dt in ("bf16", "f16"):
        for regime in rg.REGIMES:
            cs = _case(dt, regime)
            amax = np.abs(cs.exact).reshape(1, 1, 8, D).max(-1)
            eo = rg.row_err(cs.out, cs.exact, D)
            for num in worst:
                for S in (1, 3, 7):
                    r = (rg.row_err(rg.emulate_kernel(cs, num, S), cs.exact, D) - rg.ulp(amax, dt)) / np.maximum(eo, 1e-30)
                    worst[num] = max(worst[num], float(r.max()))
    assert worst["reference"] <= 1.4 and worst["fast"] <= 0.8, worst
    assert rg.C_EXACT >= 1.4 * worst["reference"]


def test_each_seeded_fault_fails_the_exact_criterion_somewhere():
    """Every fault fails check_out_exact in at least one regime; the table of where OUT_TOL alone would have passed the
    faulty output is recorded, and the appended row left out of P.V (flat logits) is in it."""
    caught, out_tol_escapes = {}, {}
    for f in rg.FAULTS:
        caught[f], out_tol_escapes[f] = [], []
        if f == "masked_row_zeros":
            cases = [("masked", _case("bf16", "flat", ("range", "full")))]
        else:
            cases = [(r, _case("bf16", r)) for r in rg.REGIMES]
        for name, cs in cases:
            got = rg.emulate_kernel(cs, "reference", 3, fault=f)
            if not _ok(got, cs):
                caught[f].append(name)
                if np.allclose(got, cs.out, **OUT_TOL["bf16"]):
                    out_tol_escapes[f].append(name)
    print("caught:", caught)
    print("passed OUT_TOL although wrong:", out_tol_escapes)
    assert all(caught[f] for f in rg.FAULTS), caught
    assert "flat" in out_tol_escapes["drop_new_row"], out_tol_escapes
    assert "flat" in caught["drop_new_row"] and "new_max" in caught["drop_new_row"]
    assert "flat" in caught["merge_weight_0p8"] and "large12" in caught["merge_stale_max"]
    assert "rising" in caught["defer_without_correction"]


# ---- DecodeChain host validation (shape / dtype logic; the device tests build real chains) ---------------------------
def _layers(L=2, B=1, H=4, cap=256, d=D, dt=torch.bfloat16, stash=256):
    mk = lambda *s: torch.zeros(*s, dtype=dt)
    return dict(q=[mk(B, H, d) for _ in range(L)], k_cache=[mk(B, H, cap, d) for _ in range(L)],
                kr_cache=[mk(B, H, cap, d) for _ in range(L)], v_cache=[mk(B, H, cap, d) for _ in range(L)],
                out=[mk(B, H * d) for _ in range(L)], k_new=[mk(B, H, d) for _ in range(L)], v_new=[mk(B, H, d) for _ in range(L)],
                scores=[mk(B, H, stash) for _ in range(L)])


def test_chain_validation_accepts_a_consistent_layer_set_and_reports_the_shortest_stash():
    from spatten_amd import ops
    t = _layers()
    t["scores"][1] = torch.zeros(1, 4, 200, dtype=torch.bfloat16)
    assert ops.chain_check_layers(**t) == 200
    t["scores"] = None
    assert ops.chain_check_layers(**t) is None
    ops.chain_check_stash(None, 10 ** 6, False)


def test_chain_validation_refuses_a_short_stash():
    from spatten_amd import ops
    t = _layers(stash=256)
    t["scores"][1] = torch.zeros(1, 4, 100, dtype=torch.bfloat16)
    rows = ops.chain_check_layers(**t)
    ops.chain_check_stash(rows, 100, False)
    with pytest.raises(ValueError):
        ops.chain_check_stash(rows, 101, False)
    with pytest.raises(ValueError):
        ops.chain_check_stash(rows, 100, True, layout=128)        # the device-length form: the layout bound too
    ops.chain_check_stash(rows, 90, False, layout=128)             # a static layout beyond the length writes no further


@pytest.mark.parametrize("bad", ["out_shape", "out_dtype", "mixed_plane_dtype", "plane_shape", "q_shape", "k_new_dtype",
                                 "v_new_shape", "scores_heads", "scores_dtype", "layer_count"])
def test_chain_validation_refuses_inconsistent_layers(bad):
    from spatten_amd import ops
    t = _layers()
    bf = torch.bfloat16
    if bad == "out_shape":
        t["out"][1] = torch.zeros(1, 4 * D + 8, dtype=bf)
    elif bad == "out_dtype":
        t["out"][0] = torch.zeros(1, 4 * D, dtype=torch.float16)
    elif bad == "mixed_plane_dtype":
        t["v_cache"][1] = t["v_cache"][1].to(torch.float16)
    elif bad == "plane_shape":
        t["kr_cache"][1] = torch.zeros(1, 4, 128, D, dtype=bf)
    elif bad == "q_shape":
        t["q"][1] = torch.zeros(1, 3, D, dtype=bf)
    elif bad == "k_new_dtype":
        t["k_new"][1] = t["k_new"][1].float()
    elif bad == "v_new_shape":
        t["v_new"][0] = torch.zeros(1, 4, D // 2, dtype=bf)
    elif bad == "scores_heads":
        t["scores"][1] = torch.zeros(1, 2, 256, dtype=bf)
    elif bad == "scores_dtype":
        t["scores"][1] = torch.zeros(1, 4, 256, dtype=torch.float32)
    elif bad == "layer_count":
        t["out"] = t["out"][:1]
    with pytest.raises(ValueError):
        ops.chain_check_layers(**t)
    with pytest.raises(ValueError):            # the constructor validates before it touches a device
        ops.DecodeChain(**t)
