"""Head pruning inside the matrix-core grouped-query decode step (csrc/decode_gqa.hip, HL; opt-in: grouped_heads=True =
SPATTEN_DECODE_GROUPED_HEADS, mode 1): the grid stays one workgroup column per KV head, every workgroup derives its group's live
mask from the device list.  Live heads carry the plain grouped step's bits, pruned heads' rows are untouched, a group without a
survivor appends nothing, and the head importance is a fixed-order fp32 sum.  Every grouped call is preceded by
ops.decode_gqa_form(...) is True.  Needs an MI355X.

Shapes: 32-row tiles round-robin over four waves, a split holds at least 128 rows — N = 5 (inside one tile), 130 (just over one
split's minimum), 600 (several tiles per wave), 1031 (ragged end); G = 3, 4 and 32."""
import numpy as np
import pytest
import torch

from oracle import spatten_oracle as orc
from tests.test_gpu_gqa import check_stash
from tests.test_gpu_gqa_cascade import Step
from tests.util import OUT_TOL, TORCH_DT, host

pytestmark = pytest.mark.gpu
D = 128
OUT_S, STASH_S, LSE_S, ACC_S = 7.0, -3.0, 5.0, 3.0          # sentinels


class HStep(Step):
    def go(self, mode, ids=None, flag=False, acc=None, head_abs=None, n_splits=0, q=None, prev=None, form=None):
        """One appending step on private copies of the caches, outputs pre-filled with sentinels."""
        from spatten_amd import ops
        N = self.N
        kc, krc, vc = self.kc.clone(), self.krc.clone(), self.vc.clone()
        stash = torch.full((self.B, self.H, self.cap), STASH_S, dtype=self.tdt, device="cuda")
        lse = torch.full((self.B, self.H, 2), LSE_S, dtype=torch.float32, device="cuda")
        out = torch.full((self.B, self.H * self.d), OUT_S, dtype=self.tdt, device="cuda")
        kw = dict(k_new=self.kn, v_new=self.vn, out=out, scores=stash, lse=lse, n_splits=n_splits, head_ids=ids, head_abs=head_abs,
                  cascade=None if acc is None else (acc, self.prev if prev is None else prev, self.plse, N - 1))
        if flag:
            kw["grouped_heads"] = True
        args = (self.q if q is None else q, kc, krc, vc, N, self.cos, self.sin, N - 1)
        old = ops.set_decode_gqa(mode)
        try:
            if form is not None:
                assert ops.decode_gqa_form(*args, **kw) is form
            ops.attn_decode(*args, **kw)
        finally:
            ops.set_decode_gqa(old)
        torch.cuda.synchronize()
        return dict(out=out.view(self.B, self.H, self.d), stash=stash, lse=lse, k=kc, kr=krc, v=vc)


def head_lists(H, Hkv):
    G = H // Hkv
    return {"all": list(range(H)), "one": [H // 2],
            "first dropped": [h for h in range(H) if h % G != 0], "last dropped": [h for h in range(H) if h % G != G - 1],
            "group dropped": [h for h in range(H) if h // G != 1]}


def split_heads(ids, H, Hkv):
    G = H // Hkv
    live = torch.zeros(H, dtype=torch.bool, device="cuda")
    live[ids] = True
    groups = live.view(Hkv, G).any(1)               # KV heads with a survivor
    return live, groups


def abs_bound_check(got, a0, out, live_units, name):
    """|got - (a0 + sum_e |out_e|)| <= 130 * 2^-24 * (a0 + sum_e |out_e|): 128 fp32 additions of exact 16-bit terms and the add into
    the accumulator, each at most half an ulp of a partial sum that never exceeds the total (all terms >= 0) — derived."""
    want = a0.double().cpu().numpy() + np.abs(out.double().cpu().numpy()).sum(-1).reshape(-1)
    g = got.double().cpu().numpy()
    lv = live_units.cpu().numpy()
    err = np.abs(g - want)[lv]
    assert (err <= 130 * 2.0 ** -24 * want[lv]).all(), (name, float(err.max()), float(want[lv].max()))
    assert torch.equal(got[~live_units], a0[~live_units]), f"{name}: pruned units moved"


CASES = [("bf16", 1, 12, 4), ("bf16", 2, 8, 2), ("bf16", 1, 64, 2), ("f16", 1, 12, 4)]


@pytest.mark.parametrize("n_splits", [1, 4])
@pytest.mark.parametrize("N", [5, 130, 600, 1031])
@pytest.mark.parametrize("dt,B,H,Hkv", CASES)
def test_flagged_head_list_step(dt, B, H, Hkv, N, n_splits):
    from spatten_amd import ops
    s = HStep(B, H, Hkv, N, dt)
    G = H // Hkv
    a0 = (1.5 + 0.25 * torch.arange(B * H, device="cuda", dtype=torch.float32))
    plain = s.go(1, n_splits=n_splits, form=True)
    for name, lst in head_lists(H, Hkv).items():
        ids = torch.tensor(lst, dtype=torch.int32, device="cuda")
        live, groups = split_heads(lst, H, Hkv)
        dead = ~live
        live_units = live.repeat(B)
        for casc in (False, True):
            tag = f"{name} casc={casc}"
            acc = torch.zeros(H, s.cap, dtype=torch.float32, device="cuda") if casc else None
            ha = a0.clone()
            got = s.go(1, ids=ids, flag=True, acc=acc, head_abs=ha, n_splits=n_splits, form=True)
            # 1. live heads carry the plain grouped step's bits; pruned rows keep the sentinel
            for key in ("out", "stash", "lse"):
                assert torch.equal(got[key][:, live], plain[key][:, live]), (tag, key)
            assert bool((got["out"][:, dead] == OUT_S).all()) and bool((got["stash"][:, dead] == STASH_S).all()) \
                and bool((got["lse"][:, dead] == LSE_S).all()), tag
            # 2. the append follows the group
            for key, src in (("k", s.kc), ("kr", s.krc), ("v", s.vc)):
                assert torch.equal(got[key][:, groups], plain[key][:, groups]), (tag, key)
                assert torch.equal(got[key][:, ~groups], src[:, ~groups]), (tag, key, "emptied group appended")
            # 3. against the per-query-head kernel with the same list
            acc0 = torch.zeros_like(acc) if casc else None
            ha0 = a0.clone()
            ref = s.go(0, ids=ids, acc=acc0, head_abs=ha0, n_splits=n_splits, form=False)
            for key in ("k", "kr", "v"):
                assert torch.equal(got[key], ref[key]), (tag, key)
            np.testing.assert_allclose(host(got["out"][:, live]), host(ref["out"][:, live]), err_msg=tag, **OUT_TOL[dt])
            check_stash(host(got["stash"][:, live, :N]), host(ref["stash"][:, live, :N]), dt, tag)
            assert bool((ref["out"][:, dead] == OUT_S).all())
            # 5. head importance: the derived bound against the `out` the call left, pruned units bit-unchanged, run-to-run identical
            abs_bound_check(ha, a0, got["out"], live_units, tag)
            ha2 = a0.clone()
            acc2 = torch.zeros_like(acc) if casc else None
            again = s.go(1, ids=ids, flag=True, acc=acc2, head_abs=ha2, n_splits=n_splits, form=True)
            assert torch.equal(ha2, ha) and torch.equal(again["out"], got["out"]), tag
            # 6. cascade importance: the per-query-head kernel's bits on live rows; pruned rows and columns >= prev_len untouched
            if casc:
                assert torch.equal(acc[live], acc0[live]) and torch.equal(acc2, acc), tag
                assert float(acc[live, :N - 1].min()) > 0.0
                guard = torch.full_like(acc, ACC_S)
                s.go(1, ids=ids, flag=True, acc=guard, n_splits=n_splits, form=True)
                assert bool((guard[dead] == ACC_S).all()) and bool((guard[:, N - 1:] == ACC_S).all()), tag
                assert bool((guard[live, :N - 1] != ACC_S).any()), tag
            # 4. what the pruned heads' inputs hold reaches nothing
            if dead.any():
                qn = s.q.clone()
                qn[:, dead] = float("nan")
                pn = s.prev.clone()
                pn[:, dead] = float("nan")
                ha3 = a0.clone()
                acc3 = torch.zeros_like(acc) if casc else None
                nan = s.go(1, ids=ids, flag=True, acc=acc3, head_abs=ha3, n_splits=n_splits, q=qn, prev=pn, form=True)
                for key in ("out", "stash", "lse", "k", "kr", "v"):
                    assert torch.equal(nan[key], got[key]), (tag, key, "NaN leaked")
                assert torch.equal(ha3, ha), tag
                if casc:
                    assert torch.equal(acc3, acc), tag
    # head importance without a list
    ha = a0.clone()
    got = s.go(1, flag=True, head_abs=ha, n_splits=n_splits, form=True)
    assert torch.equal(got["out"], plain["out"]) and torch.equal(got["stash"], plain["stash"])
    abs_bound_check(ha, a0, got["out"], torch.ones(B * H, dtype=torch.bool, device="cuda"), "no list")
    # ... and without the flag the block stays on the per-query-head kernel
    ids = torch.tensor(head_lists(H, Hkv)["one"], dtype=torch.int32, device="cuda")
    s.go(1, ids=ids, n_splits=n_splits, form=False)
    ops.check_workspaces()


def test_live_heads_against_the_oracle():
    dt, B, H, Hkv, N = "bf16", 1, 12, 4, 600
    s = HStep(B, H, Hkv, N, dt, seed=4)
    lst = head_lists(H, Hkv)["first dropped"]
    ids = torch.tensor(lst, dtype=torch.int32, device="cuda")
    got = s.go(1, ids=ids, flag=True, n_splits=4, form=True)
    f = lambda t: host(t)
    o, stash, _ = orc.attention_core(f(s.q)[:, :, None], f(s.kn)[:, :, None], f(s.vn)[:, :, None], f(s.kc[:, :, :N - 1]),
                                     f(s.vc[:, :, :N - 1]), np.full((B, 1), N - 1), None, dt)
    o = np.asarray(o).reshape(B, H, D)
    np.testing.assert_allclose(host(got["out"])[:, lst], o[:, lst], **OUT_TOL[dt])
    check_stash(host(got["stash"])[:, lst, :N], np.asarray(stash)[:, lst, 0, :N], dt, "oracle")


def test_device_length_form_with_a_shrinking_list():
    """Three steps after a step_set, a head dies between steps (the last list empties a group): the device-length form equals the
    static flagged step laid out for the same bound, bit for bit — out, both stash / (max, sum) buffers, both accumulators, caches."""
    from spatten_amd import ops
    B, H, Hkv, P, T, bound, cap, tdt = 1, 8, 2, 250, 3, 300, 304, torch.bfloat16
    lists = [[0, 1, 2, 4, 5, 6, 7], [0, 1, 2, 4, 5, 7], [0, 1, 2]]
    g = torch.Generator(device="cuda").manual_seed(23)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32, generator=g).to(tdt)
    cos, sin = ops.rope_table(cap + 8, D, tdt, "cuda")
    k0, v0 = rnd(B, Hkv, P, D), rnd(B, Hkv, P, D)
    toks = [(rnd(B, H, D), rnd(B, Hkv, D), rnd(B, Hkv, D)) for _ in range(T)]
    ids = [torch.tensor(l, dtype=torch.int32, device="cuda") for l in lists]

    def bufs():
        kc = torch.zeros(B, Hkv, cap, D, dtype=tdt, device="cuda")
        krc, vc = torch.zeros_like(kc), torch.zeros_like(kc)
        kc[:, :, :P], vc[:, :, :P] = k0, v0
        ops.build_shadow(kc, krc, 0, P, cos, sin)
        return dict(kc=kc, krc=krc, vc=vc, out=torch.full((B, H * D), OUT_S, dtype=tdt, device="cuda"),
                    stash=[torch.zeros(B, H, cap, dtype=tdt, device="cuda") for _ in range(2)],
                    lse=[torch.zeros(B, H, 2, dtype=torch.float32, device="cuda") for _ in range(2)],
                    acc=torch.zeros(H, cap, dtype=torch.float32, device="cuda"),
                    ha=torch.full((B * H,), 0.5, dtype=torch.float32, device="cuda"))

    rec = lambda b: [x.clone() for x in (b["out"], *b["stash"], *b["lse"], b["acc"], b["ha"], b["kc"], b["krc"], b["vc"])]
    old = ops.set_decode_gqa(1)
    try:
        a, want = bufs(), []
        for t in range(T):
            n, cur, prv = P + 1 + t, t & 1, (t & 1) ^ 1
            q, kn, vn = toks[t]
            args = (q, a["kc"], a["krc"], a["vc"], n, cos, sin, n - 1)
            kw = dict(k_new=kn, v_new=vn, out=a["out"], scores=a["stash"][cur], lse=a["lse"][cur], head_ids=ids[t], head_abs=a["ha"],
                      cascade=(a["acc"], a["stash"][prv], a["lse"][prv], 0 if t == 0 else n - 1), layout=bound, grouped_heads=True)
            assert ops.decode_gqa_form(*args, **kw) is True
            ops.attn_decode(*args, **kw)
            torch.cuda.synchronize()
            want.append(rec(a))
        b = bufs()
        st = ops.StepState(cos, sin)
        st.set(P, P - 1)
        for t in range(T):
            q, kn, vn = toks[t]
            st.advance()
            args = (q, b["kc"], b["krc"], b["vc"], bound, cos, sin, 0)
            kw = dict(k_new=kn, v_new=vn, out=b["out"], scores=b["stash"][0], lse=b["lse"][0], head_ids=ids[t], head_abs=b["ha"],
                      cascade=(b["acc"], b["stash"][1], b["lse"][1], 0), step=st, grouped_heads=True)
            assert ops.decode_gqa_form(*args, **kw) is True
            ops.attn_decode(*args, **kw)
            torch.cuda.synchronize()
            for i, (x, w) in enumerate(zip(rec(b), want[t])):
                assert torch.equal(x, w), f"step {t}, buffer {i}"
    finally:
        ops.set_decode_gqa(old)
    assert float(want[-1][5][:3].min()) >= 0.0 and float(want[-1][6].min()) >= 0.5
    assert bool((want[-1][7][:, 1, P + T - 1] == 0).all()), "the emptied group appended"       # kv head 1 at the last step
    ops.check_workspaces()


def test_alternation_on_one_workspace():
    """A flagged list step, a plain grouped step and a per-query-head list step interleaved on one workspace (four splits: tagged
    partials, generation words) give what each gives alone; the workspace reports no error."""
    from spatten_amd import ops
    B, H, Hkv, N = 1, 12, 4, 600
    s = HStep(B, H, Hkv, N, "bf16", seed=6)
    ids = torch.tensor(head_lists(H, Hkv)["group dropped"][1:], dtype=torch.int32, device="cuda")
    runs = {"flagged": lambda: s.go(1, ids=ids, flag=True, n_splits=4, form=True),
            "plain": lambda: s.go(1, n_splits=4, form=True),
            "per head": lambda: s.go(0, ids=ids, n_splits=4, form=False)}
    alone = {k: f() for k, f in runs.items()}
    for k in ("flagged", "plain", "per head", "flagged", "per head", "plain", "flagged", "flagged", "plain"):
        got = runs[k]()
        for key in got:
            assert torch.equal(got[key], alone[k][key]), (k, key)
    ops.check_workspaces()
