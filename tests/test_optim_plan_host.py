"""CPU: (1) every case table of tests/test_hip_optim_branches.py reaches the route it names, through pcg_launch_plan_describe alone, and
PCG_ADAM_TICK_BLOCKS=0 (a fresh child: the knob is read once per process) still plans at least one block; (2) the float64 references of
tests/optim_ref.py agree with torch.optim.Adam / AdamW and with torch autograd in float64; (3) the new bounds, evaluated at the inputs
of test_hip_ops.py::test_adam / test_bce_losses, are nowhere looser than those tests' tolerances; (4) optim.Adam._plan / _dense_span on
CPU tensors carved from one buffer: which parameters share a launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402
import test_hip_optim_branches as T  # noqa: E402


# ---- (1) routes --------------------------------------------------------------------------------------------------------------------
def test_adam_cases_reach_their_routes():
    assert os.environ.get("PCG_ADAM_TICK_BLOCKS") is None
    T.check_all_routes()
    assert {n for n, *_ in T.ADAM_ROUTE_CASES} >= {1, 3, 4, 7, 1003, 262144, 262151, 65537, 8388613}


def test_launch_plan_describe_refuses_bad_adam_arguments():
    import pcgan_amd
    from pcgan_amd import _lib, ops
    for args in ((_lib.PLAN_ADAM, 0, 1, 1), (_lib.PLAN_ADAM, -4, 1, 0), (_lib.PLAN_ADAM, 8, 1), (_lib.PLAN_ADAM, 8, 1, 1, 1), (_lib.PLAN_ADAM + 1, 8, 1, 1)):
        with pytest.raises(pcgan_amd.PcgError, match="pcg_launch_plan_describe"):
            ops.launch_plan(*args)
    # below four elements there is no 16-byte lane whatever the pointers; the eager scalar grid is not capped at 256
    assert ops.launch_plan(_lib.PLAN_ADAM, 3, 1, 1) == ops.launch_plan(_lib.PLAN_ADAM, 3, 0, 1) == "scalar lanes: 1 block of 256: 1 pass"
    assert ops.launch_plan(_lib.PLAN_ADAM, 65537, 0, 0) == "scalar lanes: 257 blocks of 256: 1 pass"


@pytest.mark.parametrize("value,want", T.KNOB_SETTINGS + [("nonsense", T.KNOB_SETTINGS[0][1]), ("-3", T.KNOB_SETTINGS[0][1])])
def test_tick_blocks_knob_plans_at_least_one_block(value, want):
    """The describe text of the knob size in a child started with the knob: "0", a non-number and a negative number are clamped to one
    block (they used to ask for an empty grid, or for none at all)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adam_knob_child.py")
    r = subprocess.run([sys.executable, child, "--plan"], env={**os.environ, "PCG_ADAM_TICK_BLOCKS": value}, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want
    assert not want.startswith("float4 lanes: 0 ")


# ---- (2) references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", sorted(T.DECAYS))
@pytest.mark.parametrize("beta1", T.BETA1S, ids=repr)
def test_reference_adam_matches_torch(decay, beta1):
    """Four chained R.adam_step calls against torch.optim.Adam / AdamW in float64 (foreach=False): parameters and both moments."""
    p, g0, _, _ = (x.double() for x in T.adam_state(1003))
    hp = T.hyper(decay, beta1)
    q = torch.nn.Parameter(p.clone())
    cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
    opt = cls([q], lr=hp["lr"], betas=(beta1, hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    gen = torch.Generator().manual_seed(5)
    for t in range(1, 5):
        g = g0 if t == 1 else torch.randn(1003, generator=gen).double()
        q.grad = g.clone()
        opt.step()
        r = R.adam_step(p, g, m, v, t, hp["lr"], beta1, hp["beta2"], hp["eps"], hp["wd"], hp["decoupled"])
        p, m, v = r["p"], r["m"], r["v"]
        torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(m, opt.state[q]["exp_avg"], rtol=1e-13, atol=1e-16)
        torch.testing.assert_close(v, opt.state[q]["exp_avg_sq"], rtol=1e-13, atol=1e-18)
        for k in ("p_bound", "m_bound", "v_bound"):
            assert bool(torch.isfinite(r[k]).all()) and bool((r[k] >= 0).all())
        assert bool((r["p_bound"] > 0).all())


def test_reference_adam_compounding_grows():
    """err_in only ever adds to a bound, and by at least the incoming error scaled by its first-order factor."""
    p, g, m, v = (x.double() for x in T.adam_state(1003))
    hp = T.hyper("l2", 0.9)
    a = R.adam_step(p, g, m, v, 2, hp["lr"], 0.9, hp["beta2"], hp["eps"], hp["wd"], False)
    e = (torch.full_like(p, 1e-6), torch.full_like(p, 1e-7), torch.full_like(p, 1e-8))
    b = R.adam_step(p, g, m, v, 2, hp["lr"], 0.9, hp["beta2"], hp["eps"], hp["wd"], False, e)
    assert bool((b["p_bound"] >= a["p_bound"] + 1e-6).all())
    assert bool((b["m_bound"] >= a["m_bound"] + 0.9 * 1e-7).all()) and bool((b["v_bound"] >= a["v_bound"] + hp["beta2"] * 1e-8).all())


def test_lerp_threshold_values():
    b = R.beta1_just_above_half()
    assert 0.5 < b < 0.5 + 2.0 ** -25 and np.float32(1.0 - b) == np.float32(0.5) - np.float32(2.0 ** -25)
    assert [R.lerp_takes_first_form(x) for x in T.BETA1S] == [False, False, True, True]
    assert 1.0 - T.BETA2 ** T.T_LARGE != 1.0 and np.float32(1.0 - T.BETA2 ** T.T_LARGE) == np.float32(1.0)
    assert np.float32(np.sqrt(1.0 - T.BETA2 ** T.T_LARGE)) == np.float32(1.0)


@pytest.mark.parametrize("n", [7, 257])
def test_reference_bce_matches_autograd(n):
    p, soft, z = (x.double() for x in T.bce_inputs(n))
    for t in (torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64), torch.full((n,), 0.9, dtype=torch.float64), soft):
        pr = p.clone().requires_grad_(True)
        loss = F.binary_cross_entropy(pr, t)
        (1.9 * loss).backward()
        r = R.bce(p, t, 1.9)
        torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(r["dp"], pr.grad, rtol=1e-12, atol=1e-18)
        assert bool((r["dp_bound"][r["dp"] != 0] > 0).all()) and float(r["loss_bound"]) > 0
    for t in (0.0, 1.0, 0.9):
        zr = z.clone().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(zr, torch.full((n,), t, dtype=torch.float64))
        (-0.85 * loss).backward()
        r = R.bce_with_logits(z, t, -0.85)
        torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(r["dz"], zr.grad, rtol=1e-12, atol=1e-300)
        assert bool((r["dz_bound"] > 0).all()) and bool(torch.isfinite(r["dz_bound"]).all())


def test_reference_bce_pair_matches_autograd():
    n = 257
    p = T.bce_inputs(2 * n, seed=5)[0].double()
    g0, g1, g2 = T.PAIR_COTANGENTS
    for mask in range(8):
        cot = [c if mask >> i & 1 else None for i, c in enumerate((g0, g1, g2))]
        pr = p.clone().requires_grad_(True)
        l0 = F.binary_cross_entropy(pr[:n], torch.full((n,), 0.9, dtype=torch.float64))
        l1 = F.binary_cross_entropy(pr[n:], torch.zeros(n, dtype=torch.float64))
        outs = torch.stack([l0, l1, l0 + l1])
        w = torch.ones(3, dtype=torch.float64) if mask == 0 else torch.tensor([0.0 if c is None else c for c in cot], dtype=torch.float64)
        if mask == 0:
            (l0 + l1).backward()                 # all three missing counts as 1 per half: the gradient of the sum
        else:
            outs.backward(w)
        r = R.bce_pair(p, n, 0.9, 0.0, *cot)
        torch.testing.assert_close(r["loss"], outs.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(r["dp"], pr.grad, rtol=1e-12, atol=1e-18)
    assert R.pair_scales(None, None, None) == (1.0, 1.0) and R.pair_scales(0.7, None, None) == (0.7, 0.0) and R.pair_scales(None, None, 2.0) == (2.0, 2.0)


# ---- (3) no looser than the older tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 1000, 7])
def test_bce_bounds_inside_the_tolerances_of_test_bce_losses(n):
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(np.float32)
    p[0] = 0.0; p[-1] = 1.0
    z = (rng.standard_normal(n) * 5).astype(np.float32)
    p, z = torch.from_numpy(p).double(), torch.from_numpy(z).double()
    tt = torch.from_numpy((rng.random(n) > 0.5).astype(np.float32)).double()
    for t in (0.0, 1.0, tt):
        r = R.bce(p, t)
        assert float(r["loss_bound"]) <= 2e-6 * abs(float(r["loss"]))
        assert bool((r["dp_bound"] <= 2e-5 * r["dp"].abs() + 1e-9).all())
    for t in (0.0, 1.0):
        r = R.bce_with_logits(z, t)
        assert float(r["loss_bound"]) <= 2e-6 * abs(float(r["loss"]))
        assert bool((r["dz_bound"] <= 2e-5 * r["dz"].abs() + 1.2e-7 / n).all())


@pytest.mark.parametrize("betas,wd,decoupled", [((0.5, 0.999), 0.0, False), ((0.9, 0.999), 0.0, False), ((0.0, 0.9), 0.01, True)])
@pytest.mark.parametrize("n", [4096, 1003])
def test_adam_bounds_inside_the_tolerances_of_test_adam(betas, wd, decoupled, n):
    """The one-step bound along test_adam's float64 trajectory against that test's tolerances (rtol 1e-6 / 1e-5 / 1e-5 with atol 1e-7 /
    1e-7 / 1e-9), which it applies after four accumulated steps."""
    rng = np.random.default_rng(n)
    p = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 5):
        g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).double()
        r = R.adam_step(p, g, m, v, step, 2e-4, betas[0], betas[1], 1e-8, wd, decoupled)
        p, m, v = r["p"], r["m"], r["v"]
        assert bool((r["p_bound"] <= 1e-6 * p.abs() + 1e-7).all())
        assert bool((r["m_bound"] <= 1e-5 * m.abs() + 1e-7).all())
        assert bool((r["v_bound"] <= 1e-5 * v.abs() + 1e-9).all())


# ---- (4) optim.Adam._plan ------------------------------------------------------------------------------------------------------------
def _carve(buf, gbuf, spans, goffs=None):
    """Parameters over buf[a:b] with gradients over gbuf[a + goff : b + goff]."""
    out = []
    for i, (a, b) in enumerate(spans):
        p = torch.nn.Parameter(buf[a:b])
        off = goffs[i] if goffs else 0
        p.grad = gbuf[a + off:b + off]
        assert p.data_ptr() == buf.data_ptr() + 4 * a
        out.append(p)
    return out


def _runs(opt):
    return [[[id(p) for p in s["params"]] for s in segs] for segs in opt._plan(on_gpu=False)]


def test_plan_merges_by_gap():
    """Gaps of 0 and 3 floats merge (FlatModule pads every parameter to a multiple of four floats), a gap of 4 splits."""
    from pcgan_amd import optim
    buf, gbuf = torch.zeros(64), torch.zeros(64)
    ps = _carve(buf, gbuf, [(0, 8), (8, 16), (19, 27), (31, 39)])
    opt = optim.Adam(ps)
    assert _runs(opt) == [[[id(ps[0]), id(ps[1]), id(ps[2])], [id(ps[3])]]]
    seg = opt._plan(on_gpu=False)[0][0]
    assert seg["pptr"] == buf.data_ptr() and seg["pend"] == buf.data_ptr() + 4 * 27 and seg["gptr"] == gbuf.data_ptr()


def test_plan_splits_on_a_differing_gradient_offset_and_sorts():
    from pcgan_amd import optim
    buf, gbuf = torch.zeros(64), torch.zeros(64)
    ps = _carve(buf, gbuf, [(0, 8), (8, 16), (16, 24)], goffs=[0, 4, 4])
    assert _runs(optim.Adam(ps)) == [[[id(ps[0])], [id(ps[1]), id(ps[2])]]]      # the gradient of the second lies 4 floats further on
    ps = _carve(buf, gbuf, [(0, 8), (8, 16), (16, 24)])
    assert _runs(optim.Adam([ps[2], ps[0], ps[1]])) == [[[id(ps[0]), id(ps[1]), id(ps[2])]]]      # given out of memory order


def test_plan_dense_views_groups_and_frozen_parameters():
    import pcgan_amd
    from pcgan_amd import optim
    buf, gbuf = torch.zeros(64), torch.zeros(64)
    perm = torch.nn.Parameter(buf[0:24].view(2, 3, 4).permute(0, 2, 1))          # dense under a permutation: accepted
    perm.grad = gbuf[0:24].view(2, 3, 4).permute(0, 2, 1)
    nxt = _carve(buf, gbuf, [(24, 32)])[0]
    assert optim.Adam._dense_span(perm.data) == (buf.data_ptr(), 24)
    assert _runs(optim.Adam([perm, nxt])) == [[[id(perm), id(nxt)]]]
    strided = torch.nn.Parameter(buf[32:48:2])                                     # every other float: refused
    strided.grad = gbuf[32:48:2]
    assert optim.Adam._dense_span(strided.data) is None
    with pytest.raises(pcgan_amd.PcgError, match="dense"):
        optim.Adam([strided])._plan(on_gpu=False)
    mixed = torch.nn.Parameter(buf[0:24].view(2, 3, 4).permute(0, 2, 1))          # dense, but the gradient in another layout
    mixed.grad = gbuf[0:24].view(2, 4, 3)
    with pytest.raises(pcgan_amd.PcgError, match="identical layout"):
        optim.Adam([mixed])._plan(on_gpu=False)
    a, b = _carve(buf, gbuf, [(0, 8), (8, 16)])                                    # adjacent, but in two groups: never one launch
    assert _runs(optim.Adam([dict(params=[a]), dict(params=[b], lr=1e-2)])) == [[[id(a)]], [[id(b)]]]
    a, frozen, c = _carve(buf, gbuf, [(0, 8), (8, 12), (12, 20)])                  # a frozen parameter without a gradient is skipped,
    frozen.requires_grad_(False)                                                   # and its four floats keep its neighbours apart
    frozen.grad = None
    assert _runs(optim.Adam([a, frozen, c])) == [[[id(a)], [id(c)]]]
    missing = _carve(buf, gbuf, [(0, 8)])[0]
    missing.grad = None
    with pytest.raises(pcgan_amd.PcgError, match="no gradient yet"):
        optim.Adam([missing])._plan(on_gpu=False)
    assert optim.Adam._dense_span(torch.zeros(0)) is None
    with pytest.raises(pcgan_amd.PcgError, match="float32 tensors on the GPU"):
        optim.Adam([a])._plan()                                                    # the default refuses what is not on the GPU
