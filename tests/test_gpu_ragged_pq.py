"""The decode step over the profiled planes with ONE STATE PER SEQUENCE (spatten_pq_decode_args_t::step_state_sb,
ops.attn_decode_pqv(step=StepState(batch=B))): a ragged batch — every sequence its own cache length, query position and append
slot — through both passes of spatten_attn_decode_pq, the quantised-query form, and spatten_kv_append_planes_ragged.

Three yardsticks per case.  Bit exact: for each sequence b today's static launch of the same batch (kv_len = length_b, pos_q =
pos_b, laid out for the bound, same splits and heads) on clones of the buffers, whose row b the ragged launch must reproduce bit
for bit.  Untouched: sentinels past a sequence's length, in pruned heads' rows and in every plane / cache row but length_b - 1.
Independent: oracle.spatten_oracle.pq_decode_attention_profile on each sequence alone, with the tolerances of
tests/test_gpu_pq_profiles.py.

Shapes: bound 704, lengths after the append (704, 353, 352, 236, 1): 352 | 353 is the chunk edge of two splits, 236 lies beside
that of three; every length but 704 ends inside a 128-row (d 128) / 256-row (d 64) tile; length 1 is the appended row alone; the
refetch pass has its own layout (3 splits of ~256 rows) at one and two splits.  Thresholds 0.0 (nothing flagged), 2.0 (everything
flagged) and one in between, picked on the CPU from the oracle's max MSB probabilities so that one sequence has more than half of
its launched heads flagged (the compact pass's coarse layout), one has some but at most half (the fine layout), the length-1
sequence none — and every |p1max - thr| > 1e-3, ten times the flag band of 1e-4: no flag is left undecided.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests import pq_qint_exact as qx
from tests.test_gpu_decode import oracle_table
from tests.util import OUT_TOL, TORCH_DT, dev, host

pytestmark = pytest.mark.gpu

CAP = 704
LENS = (704, 353, 352, 236, 1)            # cache lengths AFTER the step's append
POS_OFF = (0, 3, 0, 9, 5)                 # query position = length - 1 + offset
TABLE_ROWS = 724
PLANE_FILL, STASH_FILL, OUT_FILL, LOGIT_FILL, BYTE_FILL = 7.0, 5.0, 3.0, 9.0, 0x5A
BAND = 1e-3                               # every |p1max - thr| must exceed it (the project's flag band is 1e-4)

# (name, key bits, value bits, dtype, d, H, Hkv, head list, head_abs, query_bits, seed)
ROUTES = [
    ("p88-bf16", 8, 8, "bf16", 128, 4, 4, None, False, None, 0),
    ("p48-f16-d64", 4, 8, "f16", 64, 8, 4, None, False, None, 0),
    ("p66-bf16-gqa", 6, 6, "bf16", 128, 8, 2, None, False, None, 0),
    ("p88-f32", 8, 8, "f32", 128, 4, 2, None, False, None, 0),
    ("p88-head-list", 8, 8, "bf16", 128, 4, 4, (0, 2, 3), True, None, 0),
    ("p88-qint8", 8, 8, "bf16", 128, 4, 4, None, False, 8, 0),
    ("p48-f16-d64-qint8", 4, 8, "f16", 64, 8, 4, None, False, 8, 0),
]
ROUTE_IDS = [r[0] for r in ROUTES]


def rotated(x, pos, d, dt):
    """x [Hx, n, d] rotated at positions pos [n] by the oracle's own rotary embedding."""
    c, s = orc.rope_table(TABLE_ROWS, d, dt)
    return orc.apply_rotary_pos_emb_single(x[None], c, s, np.asarray(pos)[None], dt)[0]


def oracle_sequence(q_b, K, V, pos_q, kb, vb, G, dt, bits):
    """One sequence alone: K / V [Hkv, n, d] un-rotated (the appended row included), q_b [H, d].  Returns the planes repeated to the
    query heads, the (rotated, for the quantised-query form quantised and dequantised) query and the max MSB probability per head."""
    d = K.shape[-1]
    kr = rotated(K, np.arange(K.shape[1]), d, dt)
    msb, lsb, scale = orc.pq_quantize(kr[None], bits=kb + 4)
    qv, vscale = orc.pq_quantize_values(V[None], bits=vb)
    rep = lambda a: orc.repeat_kv(a, G)
    planes = tuple(rep(np.asarray(a)) for a in (msb.astype(np.int64), lsb.astype(np.int64), scale, qv.astype(np.int64), vscale))
    qr = rotated(q_b[:, None], [pos_q], d, dt)[:, 0][None]                  # [1, H, d]
    if bits is not None:
        q_int, q_scale = qx.quantise_query(qr, bits)
        qr = (q_int.astype(np.float32) * q_scale[..., None]).astype(np.float32)
    s1 = np.einsum("bhd,bhld->bhl", qr.astype(np.float32), orc.pq_dequant(planes[0], None, planes[2])) / np.float32(np.sqrt(d))
    return planes, qr, orc.softmax_probs(s1).max(-1)[0]


def pick_mid_threshold(p1max, live, last):
    """A threshold between two neighbouring max probabilities that meets the docstring's conditions, or None."""
    p = p1max[:, live]
    vals = np.unique(p)
    for thr in (vals[:-1] + vals[1:]) / 2:
        cnt = (p < thr).sum(1)
        if np.abs(p - thr).min() > BAND and (2 * cnt > len(live)).any() and ((cnt > 0) & (2 * cnt <= len(live))).any() and cnt[last] == 0:
            return float(thr)
    return None


_CASES = {}


def case(route, seed=None):
    """Host inputs of a route and its oracle at the three thresholds, computed once and shared (never modified)."""
    name, kb, vb, dt, d, H, Hkv, hlist, _, bits, seed0 = route
    seed = seed0 if seed is None else seed
    key = (name, seed)
    if key in _CASES:
        return _CASES[key]
    B, G = len(LENS), H // Hkv
    s = 9300 + 7 * H + Hkv + d + kb + 1000 * seed
    q = orc.synth_normal(s, 0, (B, H, d), dt)
    kn = orc.synth_normal(s, 1, (B, Hkv, d), dt)
    vn = orc.synth_normal(s, 2, (B, Hkv, d), dt)
    pasts = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n - 1, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n - 1, d), dt))
             for b, n in enumerate(LENS)]
    pos = [n - 1 + o for n, o in zip(LENS, POS_OFF)]
    live = list(range(H)) if hlist is None else list(hlist)
    seqs = []
    for b in range(B):
        K = np.concatenate([pasts[b][0], kn[b][:, None]], axis=1)
        V = np.concatenate([pasts[b][1], vn[b][:, None]], axis=1)
        seqs.append(oracle_sequence(q[b], K, V, pos[b], kb, vb, G, dt, bits))
    p1max = np.stack([sq[2] for sq in seqs])
    mid = pick_mid_threshold(p1max, live, LENS.index(1))
    c = dict(q=q, kn=kn, vn=vn, pasts=pasts, pos=pos, live=live, p1max=p1max, mid=mid, want={})
    if mid is not None:
        for thr in (0.0, 2.0, mid):
            c["want"][thr] = [orc.pq_decode_attention_profile(sq[1], *sq[0], thr) for sq in seqs]
    _CASES[key] = c
    return c


class Buffers:
    """Device tensors of one launch: cache planes [B, Hkv, CAP, d], the quantised planes, and every output, all pre-filled with finite
    sentinels; each sequence's past rows [0, length_b - 1) written and packed (with_new_row: row length_b - 1 too)."""
    NAMES = ("kc", "krc", "vc", "msb", "lsb", "scale", "vq", "vscale", "lg", "out", "st", "lse", "need", "habs", "qi", "qs")
    STORE = ("kc", "krc", "vc", "msb", "lsb", "scale", "vq", "vscale")        # what an append writes

    def __init__(self, kb, vb, dt, d, H, Hkv, B):
        tdt = TORCH_DT[dt]
        self.geom = (kb, vb, d, H, Hkv, B)
        self.kc = torch.full((B, Hkv, CAP, d), PLANE_FILL, dtype=tdt, device="cuda")
        self.krc, self.vc = self.kc.clone(), self.kc.clone()
        u8 = dict(dtype=torch.uint8, device="cuda")
        self.msb = torch.full((B, Hkv, CAP, d * kb // 8), BYTE_FILL, **u8)
        self.lsb = torch.full((B, Hkv, CAP, d // 2), BYTE_FILL, **u8)
        self.vq = torch.full((B, Hkv, CAP, d * vb // 8), BYTE_FILL, **u8)
        self.scale = torch.full((B, Hkv, CAP), PLANE_FILL, dtype=torch.float32, device="cuda")
        self.vscale = self.scale.clone()
        self.lg = torch.full((B, H, CAP), LOGIT_FILL, dtype=torch.float32, device="cuda")
        self.out = torch.full((B, H * d), OUT_FILL, dtype=tdt, device="cuda")
        self.st = torch.full((B, H, CAP), STASH_FILL, dtype=tdt, device="cuda")
        self.lse = torch.full((B, H, 2), -1.0, dtype=torch.float32, device="cuda")
        self.need = torch.full((B * H,), -1, dtype=torch.int32, device="cuda")
        self.habs = torch.zeros(B * H, dtype=torch.float32, device="cuda")
        self.qi = torch.full((B, H, d), -128, dtype=torch.int8, device="cuda")
        self.qs = torch.full((B, H), -1.0, dtype=torch.float32, device="cuda")

    def clone(self):
        c = object.__new__(Buffers)
        c.geom = self.geom
        for k in self.NAMES:
            setattr(c, k, getattr(self, k).clone())
        return c

    def copy_from(self, other):
        for k in self.NAMES:
            getattr(self, k).copy_(getattr(other, k))

    def planes(self, b=None):
        """The planes of the batch, or of sequence b alone (views)."""
        from spatten_amd import ops
        kb, vb, d, H, Hkv, B = self.geom
        ts = (self.msb, self.lsb, self.scale, self.vq, self.vscale, self.lg)
        if b is not None:
            ts, B = tuple(t[b:b + 1] for t in ts), 1
        return ops.PQProfilePlanes(B, Hkv, H, CAP, d, "cuda", key_bits=kb, value_bits=vb, tensors=ts)

    def fill_past(self, pasts, lens, dt, cos, sin):
        """pasts[b] = (K, V) [Hkv, >= lens[b] - 1, d]: rows [0, lens[b] - 1) of sequence b, rotated and packed."""
        from spatten_amd import ops
        for b, n in enumerate(lens):
            if n > 1:
                self.kc[b, :, :n - 1] = dev(pasts[b][0][:, :n - 1], dt)
                self.vc[b, :, :n - 1] = dev(pasts[b][1][:, :n - 1], dt)
                ops.build_shadow(self.kc[b:b + 1], self.krc[b:b + 1], 0, n - 1, cos, sin)
                ops.pq_pack_planes(self.krc[b:b + 1], self.vc[b:b + 1], self.planes(b), 0, n - 1)

    def append_host_rows(self, kn, vn, lens, cos, sin):
        """Row lens[b] - 1 of sequence b by the host-row call, one sequence at a time."""
        from spatten_amd import ops
        for b, n in enumerate(lens):
            ops.kv_append_planes(kn[b:b + 1], vn[b:b + 1], self.kc[b:b + 1], self.krc[b:b + 1], self.vc[b:b + 1], self.planes(b),
                                 n - 1, cos, sin)


def launch(buf, route, q, kn, vn, cos, sin, ws, n_splits, thr, ids, kv_len, pos_q=0, step=None, layout=0, append=False):
    from spatten_amd import ops
    use_habs, bits = route[8], route[9]
    kw = dict(out=buf.out, need_lsb=buf.need, scores=buf.st, lse=buf.lse, head_ids=ids, head_abs=buf.habs if use_habs else None,
              step=step, layout=layout, n_splits=n_splits, workspace=ws)
    if append:
        kw["append"] = (kn, vn, buf.kc, buf.krc, buf.vc)
    if bits is not None:
        kw.update(query_bits=bits, q_quant=(buf.qi, buf.qs))
    ops.attn_decode_pqv(q, buf.planes(), kv_len, cos, sin, pos_q, thr, **kw)


def ragged_state(cos, sin, lens, pos):
    from spatten_amd import ops
    step = ops.StepState(cos, sin, batch=len(lens))
    step.set([n - 1 for n in lens], [p - 1 for p in pos])
    step.advance()
    assert step.read() == list(zip(lens, pos))
    return step


def check_oracle(buf, b, n, want, live, dt, d, H, msg):
    """Row b of a launch against the oracle on that sequence alone: flags equal on every launched head (none is undecided), output
    within the model dtype's output tolerance, stash within 2^-7 (bf16) / 2^-10 relative."""
    o_ref, need_ref, logits = want
    B = buf.out.shape[0]
    got_need = buf.need.view(B, H)[b].cpu().numpy()
    assert np.array_equal(got_need[live].astype(bool), need_ref[0][live]), (msg, got_need, need_ref)
    np.testing.assert_allclose(host(buf.out).reshape(B, H, d)[b, live], orc.round_dt(o_ref[0], dt)[live], err_msg=msg, **OUT_TOL[dt])
    st = host(buf.st)[b, live, :n]
    tol = 2.0 ** (-7 if dt == "bf16" else -10)
    lg = logits[0][live]
    assert np.all(np.abs(st - lg) <= tol * np.maximum(np.abs(lg), 1.0) + 1e-6), msg


def check_untouched(rag, base, b, n, dead, dead_kv, appended, H, d, msg):
    B = rag.out.shape[0]
    assert (rag.st[b, :, n:] == STASH_FILL).all() and (rag.lg[b, :, n:] == LOGIT_FILL).all(), msg
    if dead:
        assert (rag.st[b, dead] == STASH_FILL).all() and (rag.lg[b, dead] == LOGIT_FILL).all(), msg
        assert (rag.out.view(B, H, d)[b, dead] == OUT_FILL).all() and (rag.lse[b, dead] == -1.0).all(), msg
        assert (rag.need.view(B, H)[b, dead] == -1).all() and (rag.habs.view(B, H)[b, dead] == 0).all(), msg
        assert (rag.qi[b, dead] == -128).all() and (rag.qs[b, dead] == -1.0).all(), msg
    for k in Buffers.STORE:
        x, y = getattr(rag, k), getattr(base, k)
        assert torch.equal(x[b, :, :n - 1], y[b, :, :n - 1]) and torch.equal(x[b, :, n:], y[b, :, n:]), (msg, k)
        if not appended:
            assert torch.equal(x[b, :, n - 1], y[b, :, n - 1]), (msg, k)
        elif dead_kv:
            assert torch.equal(x[b, dead_kv, n - 1], y[b, dead_kv, n - 1]), (msg, k)


def check_same_row(rag, sta, b, n, msg):
    """Row b of the ragged launch against the static launch at this sequence's length and position: bit for bit."""
    for k in ("out", "lse", "qi", "qs") + Buffers.STORE:
        assert torch.equal(getattr(rag, k)[b], getattr(sta, k)[b]), (msg, k)
    B = rag.out.shape[0]
    for k in ("need", "habs"):
        assert torch.equal(getattr(rag, k).view(B, -1)[b], getattr(sta, k).view(B, -1)[b]), (msg, k)
    for k in ("st", "lg"):
        assert torch.equal(getattr(rag, k)[b, :, :n], getattr(sta, k)[b, :, :n]), (msg, k)


@pytest.mark.parametrize("n_splits", [1, 2, 3])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_ragged_pq_step_vs_static_launches_sentinels_and_oracle(route, n_splits):
    from spatten_amd import ops
    name, kb, vb, dt, d, H, Hkv, hlist, use_habs, bits, _ = route
    c = case(route)
    B, G = len(LENS), H // Hkv
    live = c["live"]
    # ---- the condition on the inputs, on CPU values, before anything is launched
    assert c["mid"] is not None, f"{name}: no threshold meets the conditions — pick another seed"
    for thr in (0.0, 2.0, c["mid"]):
        assert np.abs(c["p1max"][:, live] - thr).min() > BAND, (name, thr)
    cnt = (c["p1max"][:, live] < c["mid"]).sum(1)
    assert (2 * cnt > len(live)).any() and ((cnt > 0) & (2 * cnt <= len(live))).any() and cnt[LENS.index(1)] == 0, (name, cnt)

    dead = [h for h in range(H) if h not in live]
    dead_kv = [g for g in range(Hkv) if g not in {h // G for h in live}]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    q, kn, vn = dev(c["q"], dt), dev(c["kn"], dt), dev(c["vn"], dt)
    ids = None if hlist is None else torch.tensor(hlist, dtype=torch.int32, device="cuda")
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    base_app = Buffers(kb, vb, dt, d, H, Hkv, B)
    base_app.fill_past(c["pasts"], LENS, dt, cos, sin)
    base_packed = base_app.clone()
    base_packed.append_host_rows(kn, vn, LENS, cos, sin)
    step = ragged_state(cos, sin, LENS, c["pos"])
    modes = [("packed", base_packed, False)]
    if bits is None:                                           # (the quantised-query form refuses the append inside the launch)
        modes.append(("append", base_app, True))
    for mode, base, app in modes:
        for thr in (0.0, 2.0, c["mid"]):
            rag = base.clone()
            launch(rag, route, q, kn, vn, cos, sin, ws, n_splits, thr, ids, CAP, step=step, append=app)
            torch.cuda.synchronize()
            ws.check()
            for b, n in enumerate(LENS):
                msg = f"{name} {mode} S={n_splits} thr={thr} b={b} len={n}"
                check_untouched(rag, base, b, n, dead, dead_kv, app, H, d, msg)
                sta = base.clone()
                launch(sta, route, q, kn, vn, cos, sin, ws, n_splits, thr, ids, n, pos_q=c["pos"][b], layout=CAP, append=app)
                torch.cuda.synchronize()
                check_same_row(rag, sta, b, n, msg)
                check_oracle(rag, b, n, c["want"][thr][b], live, dt, d, H, msg)
            ws.check()


APPEND_LENS = LENS + (CAP + 1,)           # the last sequence's state says capacity + 1: its row is not written


@pytest.mark.parametrize("kb,vb,dt,d", [(8, 8, "bf16", 128), (4, 8, "f16", 64), (6, 6, "f32", 128)])
def test_ragged_append_equals_the_host_row_call_per_sequence(kb, vb, dt, d):
    """ops.kv_append_planes(step=StepState(batch=B)) -> spatten_kv_append_planes_ragged: sequence b's row length_b - 1 of the caches
    and of every plane bit for bit what the host-row call leaves for that sequence alone, every other row untouched; a sequence
    whose state length is capacity + 1 writes nothing."""
    from spatten_amd import ops
    H, Hkv, B = 4, 2, len(APPEND_LENS)
    s = 9500 + kb + d
    lens = APPEND_LENS[:-1]
    pasts = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n - 1, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n - 1, d), dt))
             for b, n in enumerate(lens)]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    kn, vn = dev(orc.synth_normal(s, 1, (B, Hkv, d), dt), dt), dev(orc.synth_normal(s, 2, (B, Hkv, d), dt), dt)
    base = Buffers(kb, vb, dt, d, H, Hkv, B)
    base.fill_past(pasts, lens, dt, cos, sin)
    ref = base.clone()
    ref.append_host_rows(kn, vn, lens, cos, sin)               # (nothing for the last sequence)
    rag = base.clone()
    step = ops.StepState(cos, sin, batch=B)
    step.set([n - 1 for n in APPEND_LENS], [n - 1 for n in APPEND_LENS])
    step.advance()
    assert [r[0] for r in step.read()] == list(APPEND_LENS)
    ops.kv_append_planes(kn, vn, rag.kc, rag.krc, rag.vc, rag.planes(), 0, cos, sin, step=step)
    torch.cuda.synchronize()
    for k in Buffers.STORE:
        assert torch.equal(getattr(rag, k), getattr(ref, k)), k
        assert torch.equal(getattr(rag, k)[B - 1], getattr(base, k)[B - 1]), k
    for b, n in enumerate(lens):                               # the row was written at all
        assert torch.equal(rag.kc[b, :, n - 1], kn[b]) and torch.equal(rag.vc[b, :, n - 1], vn[b]), b
    with pytest.raises(ValueError):
        ops.kv_append_planes(kn[:2], vn[:2], rag.kc[:2], rag.krc[:2], rag.vc[:2], rag.planes(), 0, cos, sin, step=step)


def test_ragged_append_on_padded_views_with_guard_bands():
    """The strides spatten_kv_append_planes_ragged takes (k_new / v_new batch and head, cache batch and head): the call on views
    into larger NaN-filled parents leaves, bit for bit, what the call on contiguous tensors leaves, and changes no byte of a parent
    outside its view (tests/strided.py's criterion; the planes' own strides travel in spatten_pq_planes_t)."""
    from spatten_amd import ops
    from tests.strided import Guards, padded
    kb, vb, dt, d, H, Hkv, B = 8, 8, "bf16", 128, 4, 2, len(LENS)
    s = 9600
    pasts = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n - 1, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n - 1, d), dt))
             for b, n in enumerate(LENS)]
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    kn, vn = dev(orc.synth_normal(s, 1, (B, Hkv, d), dt), dt), dev(orc.synth_normal(s, 2, (B, Hkv, d), dt), dt)
    base = Buffers(kb, vb, dt, d, H, Hkv, B)
    base.fill_past(pasts, LENS, dt, cos, sin)
    step = ragged_state(cos, sin, LENS, [n - 1 + o for n, o in zip(LENS, POS_OFF)])
    dense = base.clone()
    ops.kv_append_planes(kn, vn, dense.kc, dense.krc, dense.vc, dense.planes(), 0, cos, sin, step=step)
    strided = base.clone()
    guards, views = Guards(), {}
    for name, t, pads in (("k_new", kn, (1, 1, 16)), ("v_new", vn, (1, 1, 16)), ("kc", base.kc, (1, 1, 64, 0)),
                          ("krc", base.krc, (1, 1, 64, 0)), ("vc", base.vc, (1, 1, 64, 0))):
        views[name], parent, mask = padded(t, pads)
        guards.add(name, parent, mask)
    assert views["k_new"].stride() != kn.stride() and views["kc"].stride()[:2] != base.kc.stride()[:2]
    guards.snapshot()
    ops.kv_append_planes(views["k_new"], views["v_new"], views["kc"], views["krc"], views["vc"], strided.planes(), 0, cos, sin, step=step)
    torch.cuda.synchronize()
    guards.check()
    for name in ("kc", "krc", "vc"):
        assert torch.equal(views[name], getattr(dense, name)), name
    for name in ("msb", "lsb", "scale", "vq", "vscale"):
        assert torch.equal(getattr(strided, name), getattr(dense, name)), name
    for b, n in enumerate(LENS):
        assert torch.equal(views["kc"][b, :, n - 1], kn[b]), b


GRAPH_START = (699, 351, 350, 234, 0)     # cache lengths BEFORE the first token: sequence 1 crosses 352 | 353 while the steps run


def test_three_tokens_of_a_ragged_pq_batch_as_one_captured_graph():
    """[advance, attn_decode_pqv(step, append)] captured ONCE, replayed for three tokens with fresh q / k_new / v_new: equal to the
    same calls issued eagerly on clones bit for bit — out, stash, flags, caches and planes — and to the oracle at every step."""
    from spatten_amd import ops
    route = ("graph-p88-bf16", 8, 8, "bf16", 128, 4, 4, None, False, None, 0)
    name, kb, vb, dt, d, H, Hkv, _, _, bits, _ = route
    B, T, n_splits, G = len(GRAPH_START), 3, 2, 1
    final = tuple(n + T for n in GRAPH_START)
    s = 9700
    full = [(orc.synth_normal(s, 10 + 2 * b, (Hkv, n, d), dt), orc.synth_normal(s, 11 + 2 * b, (Hkv, n, d), dt))
            for b, n in enumerate(final)]
    toks, wants, p1 = [], [], []
    for t in range(T):
        qt = orc.synth_normal(s, 200 + t, (B, H, d), dt)
        tk = np.stack([full[b][0][:, GRAPH_START[b] + t] for b in range(B)])
        tv = np.stack([full[b][1][:, GRAPH_START[b] + t] for b in range(B)])
        toks.append((qt, tk, tv))
        seqs = [oracle_sequence(qt[b], full[b][0][:, :GRAPH_START[b] + t + 1], full[b][1][:, :GRAPH_START[b] + t + 1],
                                GRAPH_START[b] + t + POS_OFF[b], kb, vb, G, dt, bits) for b in range(B)]
        wants.append(seqs)
        p1.append(np.stack([sq[2] for sq in seqs]))
    # ---- one threshold for the turn, decided at every step (a condition on the inputs, asserted before anything is launched)
    p1 = np.stack(p1)
    vals = np.unique(p1)
    thr = next((float(v) for v in (vals[:-1] + vals[1:]) / 2
                if np.abs(p1 - v).min() > BAND and 0.25 < (p1 < v).mean() < 0.75), None)
    assert thr is not None, "no threshold is decided at every step — pick another seed"
    wants = [[orc.pq_decode_attention_profile(sq[1], *sq[0], thr) for sq in seqs] for seqs in wants]

    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    base = Buffers(kb, vb, dt, d, H, Hkv, B)
    base.fill_past(full, tuple(n0 + 1 for n0 in GRAPH_START), dt, cos, sin)      # rows [0, n0) are the past
    ws = ops.DecodeWorkspace(B, H, d, "cuda")
    tdt = TORCH_DT[dt]
    q, kn, vn = (torch.zeros(B, H, d, dtype=tdt, device="cuda"), torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"),
                 torch.zeros(B, Hkv, d, dtype=tdt, device="cuda"))
    sets = {kind: (base.clone(), ops.StepState(cos, sin, batch=B)) for kind in ("graph", "eager")}

    def token(kind):
        buf, step = sets[kind]
        step.advance()
        launch(buf, route, q, kn, vn, cos, sin, ws, n_splits, thr, None, CAP, step=step, append=True)

    def reset(kind):
        buf, step = sets[kind]
        buf.copy_from(base)
        step.set(list(GRAPH_START), [n0 - 1 + o for n0, o in zip(GRAPH_START, POS_OFF)])

    reset("graph")
    token("graph")                                         # warm-up outside the capture
    torch.cuda.synchronize()
    reset("graph"); reset("eager")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        token("graph")
    reset("graph")                                         # (nothing ran during the capture; states as set)
    for t in range(T):
        q.copy_(dev(toks[t][0], dt)); kn.copy_(dev(toks[t][1], dt)); vn.copy_(dev(toks[t][2], dt))
        gr.replay()
        token("eager")
        torch.cuda.synchronize()
        ws.check()
        g_, e_ = sets["graph"][0], sets["eager"][0]
        lens = [n0 + t + 1 for n0 in GRAPH_START]
        assert sets["graph"][1].read() == sets["eager"][1].read() == [(n, n - 1 + o) for n, o in zip(lens, POS_OFF)], t
        for k in Buffers.NAMES:
            assert torch.equal(getattr(g_, k), getattr(e_, k)), (t, k)
        for b, n in enumerate(lens):
            msg = f"{name} t={t} b={b} len={n}"
            assert (g_.st[b, :, n:] == STASH_FILL).all() and (g_.vc[b, :, n:] == PLANE_FILL).all(), msg
            assert (g_.vq[b, :, n:] == BYTE_FILL).all() and (g_.scale[b, :, n:] == PLANE_FILL).all(), msg
            check_oracle(g_, b, n, wants[t][b], list(range(H)), dt, d, H, msg)


def test_ops_refuses_what_the_library_refuses_for_a_batched_state():
    from spatten_amd import ops
    dt, d, H, Hkv, B = "bf16", 128, 4, 2, 2
    cos, sin = oracle_table(TABLE_ROWS, d, dt)
    buf = Buffers(8, 8, dt, d, H, Hkv, B)
    q = torch.zeros(B, H, d, dtype=TORCH_DT[dt], device="cuda")
    step = ops.StepState(cos, sin, batch=B)
    step.set([9, 4], [9, 4])
    step.advance()
    args = (q, buf.planes(), CAP, cos, sin, 0, 0.5)
    acc, prev = torch.zeros(H, CAP, device="cuda"), torch.zeros(B, H, 2, device="cuda")
    with pytest.raises(NotImplementedError, match="batch axis"):
        ops.attn_decode_pqv(*args, step=step, lse=buf.lse, cascade=(acc, prev, 0))
    with pytest.raises(NotImplementedError, match="grouped"):
        ops.attn_decode_pqv(*args, step=step, query_bits=8, grouped=True)
    with pytest.raises(ValueError, match="sequences"):
        ops.attn_decode_pqv(*args, step=ops.StepState(cos, sin, batch=B + 1))
    with pytest.raises(NotImplementedError, match="kept count"):
        ops.attn_decode_pq_local_v(*args, 4, buf.st, buf.lse, keep_fraction=0.5, step=step)
    with pytest.raises(NotImplementedError, match="shared state"):
        ops.pq_pack_planes(buf.krc, buf.vc, buf.planes(), 0, CAP, step=step)
