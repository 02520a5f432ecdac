"""CPU side of the quantised-query decode (spatten_attn_decode_pq_qint): the criteria of tests/pq_qint_exact.py applied to a
numpy emulation of the documented arithmetic, the evidence that they see seeded faults, the calibration of ``logit_bound``,
the derived method bound, the threshold condition the GPU test starts from, the trace mapping and the ABI.  No GPU."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import pq_exact as px
from tests import pq_qint_exact as qx
from tests import regimes as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The case grid (shared with tests/test_gpu_pq_qint.py): every decode regime pq_case offers at both profiles; dtype, head_dim,
# Hkv and query_bits rotate through the regimes so that every value meets both profiles (a covering design: the full product
# is 288 cases of float64 reference work each)
_DT_D_HKV_BITS = [("bf16", 128, 4, 8), ("f16", 64, 2, 5), ("bf16", 64, 4, 5), ("f16", 128, 2, 8),
                  ("bf16", 128, 2, 5), ("f16", 64, 4, 8), ("bf16", 64, 2, 8), ("f16", 128, 4, 5)]
GRID = [(r, kb, 8) + _DT_D_HKV_BITS[(i + (kb == 4)) % len(_DT_D_HKV_BITS)]
        for kb in (8, 4) for i, r in enumerate(rg.REGIMES)]
GRID_IDS = [f"{r}-{kb}-{dt}-d{d}-hkv{hkv}-q{bits}" for r, kb, _, dt, d, hkv, bits in GRID]


@functools.lru_cache(maxsize=None)
def case(regime, kb, vb, dt, d, Hkv, N=600, B=2, H=4):
    return px.pq_case(B, H, Hkv, d, N, dt, regime, kb, vb)


def case_thresholds(pc, bits):
    """Thresholds of a case: from the exact p1max of the documented quantisation of its query, alone."""
    ex0 = qx.qint_exact(*qx.quantise_query(pc.qr, bits), pc.planes, 0.0)
    return qx.thresholds(ex0), ex0


def run_emulation(pc, bits, thr, fault=None, **kw):
    return qx.emulate_qint(pc.qr, pc.planes, thr, pc.dt, bits, kb=pc.kb, fault=fault, q_unrotated=pc.cs.q[:, :, 0], **kw)


def passes(pc, bits, thr, fault=None, stats=None):
    try:
        qx.check_step(pc.qr, pc.planes, pc.dt, bits, thr, run_emulation(pc, bits, thr, fault), stats=stats)
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("regime,kb,vb,dt,d,Hkv,bits", GRID, ids=GRID_IDS)
def test_emulation_passes_every_criterion_and_thresholds_are_decided(regime, kb, vb, dt, d, Hkv, bits):
    pc = case(regime, kb, vb, dt, d, Hkv)
    ths, ex0 = case_thresholds(pc, bits)
    for thr in ths:
        # the threshold condition: picked from the exact p1max alone, at most BAND_CAP of the heads inside the band
        assert qx.band_share(ex0, thr) <= px.BAND_CAP, (regime, thr)
        qx.check_step(pc.qr, pc.planes, pc.dt, bits, thr, run_emulation(pc, bits, thr), name=f"{regime} thr={thr!r}")
    res = run_emulation(pc, bits, 0.0, msb_only=True)
    qx.check_step(pc.qr, pc.planes, pc.dt, bits, 0.0, res, msb_only=True, name="msb only")


def test_calibration_emulation_uses_at_most_half_of_logit_bound(capsys):
    worst = 0.0
    for regime, kb, vb, dt, d, Hkv, bits in GRID:
        pc = case(regime, kb, vb, dt, d, Hkv)
        em = run_emulation(pc, bits, 2.0)                               # every head refetched: z = s2
        ex = qx.qint_exact(em.q_int, em.q_scale, pc.planes, 2.0)
        for got, s in ((em.msb_logit, ex.s1), (em.z, ex.s2)):
            lb = qx.logit_bound(ex.s1, s)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nan_to_num(np.abs(got - s) / lb).max()))
    with capsys.disabled():
        print(f"\nworst |s_emul - s_exact| / logit_bound = {worst:.3f}")
    assert worst <= 0.5


# the case each fault is caught on (regime, kb, vb, dt, d, Hkv, bits) and the threshold index into qx.thresholds
FAULT_CASES = {
    "bias_not_removed": (("flat", 8, 8, "bf16", 128, 4, 8), 0),
    "lsb_odd_even_swapped": (("flat", 8, 8, "bf16", 128, 4, 8), 1),             # threshold 1.5: every head refetches
    "q_scale_of_neighbour_head": (("sink24", 8, 8, "bf16", 64, 4, 5), 0),
    "msb_term_not_x16": (("flat", 4, 8, "f16", 64, 2, 5), 0),
    "q_not_rotated": (("rising", 4, 8, "bf16", 64, 2, 8), 0),
    "refetch_rereads_unscaled_lsb": (("flat", 8, 8, "bf16", 128, 4, 8), 1),
    "q_int_piece_order_exported": (("flat", 4, 8, "f16", 64, 2, 5), 0),
}


@pytest.mark.parametrize("fault", qx.FAULTS)
def test_seeded_fault_fails_a_criterion(fault):
    args, ti = FAULT_CASES[fault]
    assert args in [g for g in GRID], "the named case is one of the grid's"
    pc = case(*args[:6])
    bits = args[6]
    thr = case_thresholds(pc, bits)[0][ti]
    assert passes(pc, bits, thr), "the emulation without the fault passes on the named case"
    assert not passes(pc, bits, thr, fault), f"{fault}: passes every criterion on {args}, threshold {thr!r}"


@pytest.mark.parametrize("regime,kb,vb,dt,d,Hkv,bits", GRID[::3], ids=GRID_IDS[::3])
def test_method_bound_against_the_unquantised_query(regime, kb, vb, dt, d, Hkv, bits):
    """|s_q - s| <= (q_scale / 2) sum_i |k_i| / sqrt(d) for every key (derived from |q_i - q_int_i q_scale| <= q_scale / 2)."""
    pc = case(regime, kb, vb, dt, d, Hkv)
    q_int, q_scale = qx.quantise_query(pc.qr, bits)
    exq = qx.qint_exact(q_int, q_scale, pc.planes, 0.0)
    ex = px.pq_exact(pc.qr, *pc.planes, 0.0)
    b1, b2 = qx.method_bound(q_scale, pc.planes, pc.H, pc.d)
    assert (np.abs(exq.s1 - ex.s1) <= b1 * (1 + 1e-9)).all() and (np.abs(exq.s2 - ex.s2) <= b2 * (1 + 1e-9)).all()


def observed_effect():
    """Worst relative output movement against pq_exact with the 16-bit query (max |out_q - out| / max |out| per head), at
    query_bits 8 / 6 / 4 on the flat, rising and sink regimes, (8, 8), bf16, d 128 — a property of the method: recorded in
    DESIGN.md 3.7, no pass bar."""
    rows = {}
    for regime in ("flat", "rising", "sink24"):
        pc = case(regime, 8, 8, "bf16", 128, 4)
        ex = px.pq_exact(pc.qr, *pc.planes, 2.0)
        for bits in (8, 6, 4):
            exq = qx.qint_exact(*qx.quantise_query(pc.qr, bits), pc.planes, 2.0)
            rows[(regime, bits)] = float((np.abs(exq.out - ex.out).max(-1) / np.abs(ex.out).max(-1)).max())
    return rows


def test_observed_effect_is_recorded(capsys):
    rows = observed_effect()
    with capsys.disabled():
        print("\nrelative output movement (regime, query_bits):", {k: f"{v:.3g}" for k, v in rows.items()})
    assert all(np.isfinite(v) for v in rows.values())


def test_trace_query_bits(tmp_path):
    from spatten_amd import traces
    for name in ("trace_full_cascade.csv", "trace_synthetic.csv"):
        sch = traces.read_trace(os.path.join(ROOT, "tests", "golden", name))
        assert all(s.query_bits == 16 for s in sch.layers()), name         # as written in the trace
        assert sch.query_bits() is None, name                                # 16-bit query: today's path
    row = "0,0,{h},64,128,128,8,{qb},0.1,True,4,128,8,True,False,True,64\n"
    for qb, want in ((8, 8), (5, 5), (-1, None), (12, None)):
        p = tmp_path / f"t{qb}.csv"
        p.write_text(",".join(traces.COLUMNS) + "\n" + "".join(row.format(h=h, qb=qb) for h in range(2)))
        sch = traces.read_trace(str(p))
        assert sch.layers()[0].query_bits == qb and sch.query_bits() == want, qb


def test_abi_declares_the_entry_points_and_the_struct_matches(tmp_path):
    from tests.test_abi_exports import declared_functions
    from spatten_amd import _lib
    names = declared_functions()
    assert "spatten_attn_decode_pq_qint" in names and "spatten_pq_qint_supported" in names
    cls, cname = _lib.PQQintArgs, "spatten_pq_qint_args_t"
    fields = [f[0] for f in cls._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "spatten.h"\nint main(){printf("%zu", sizeof(' + cname + '));' + \
        "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + \
        'printf(" %zu", sizeof(spatten_pq_decode_args_t)); return 0;}'
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == ctypes.sizeof(cls)
    assert nums[1:-1] == [getattr(cls, f).offset for f in fields]
    assert nums[-1] == ctypes.sizeof(_lib.PQDecodeArgs)                      # the wrapped step keeps its size


def test_supported_rule_and_validation_without_a_gpu():
    from spatten_amd import _lib
    lib = _lib.load()
    F32, F16, BF16 = 0, 1, 2
    for dt in (F32, F16, BF16):
        for d in (32, 64, 128, 256):
            for kb, vb in ((8, 8), (4, 8), (6, 6), (8, 6)):
                for qb in range(2, 11):
                    want = dt in (F16, BF16) and d in (64, 128) and (kb, vb) in ((8, 8), (4, 8)) and 4 <= qb <= 8
                    assert lib.spatten_pq_qint_supported(dt, d, kb, vb, qb) == int(want), (dt, d, kb, vb, qb)
    # argument validation happens before anything touches a device
    a = _lib.PQQintArgs()
    assert lib.spatten_attn_decode_pq_qint(None, None) == -1
    assert lib.spatten_attn_decode_pq_qint(ctypes.byref(a), None) == -1      # struct_size 0
    a.struct_size, a.query_bits = ctypes.sizeof(_lib.PQQintArgs), 8
    assert lib.spatten_attn_decode_pq_qint(ctypes.byref(a), None) == -1      # NULL outputs
    buf = (ctypes.c_char * 64)()
    a.q_int = a.q_scale = ctypes.addressof(buf)
    a.query_bits = 9
    assert lib.spatten_attn_decode_pq_qint(ctypes.byref(a), None) == -1      # query_bits outside [4, 8]


def test_plugin_keyword_is_validated():
    from spatten_amd.extensions import SpattenExtensions
    cache = type("C", (), {"important_size": 8})()
    with pytest.raises(ValueError):
        SpattenExtensions(cache, 2, pq_threshold=0.1, pq_profile=(6, 6), pq_query_bits=8)
    with pytest.raises(ValueError):
        SpattenExtensions(cache, 2, pq_threshold=0.1, pq_query_bits=8)
    with pytest.raises(ValueError):
        SpattenExtensions(cache, 2, pq_threshold=0.1, pq_profile=(8, 8), local_v_keep=0.5, pq_query_bits=8)
    with pytest.raises(ValueError):
        SpattenExtensions(cache, 2, pq_threshold=0.1, pq_profile=(8, 8), pq_query_bits=9)
    assert SpattenExtensions(cache, 2, pq_threshold=0.1, pq_profile=(4, 8), pq_query_bits=5).pq_query_bits == 5
