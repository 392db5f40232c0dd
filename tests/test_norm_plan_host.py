"""CPU: (1) every case table of tests/test_hip_norm_branches.py reaches the route it names, through pcg_launch_plan_describe alone, and
every route that file is there to cover is reached; (2) the hand-written float64 references of tests/norm_ref.py agree with
torch.float64 autograd; (3) the mask-gap condition holds for every seed of the tables: no non-zero pre-activation of the reference
lies within 8 of its own bounds of zero; (4) the new bounds, evaluated at the inputs of the three older tests of the same kernels
(test_batchnorm_fwd_bwd, test_instance_norm_forward_backward_and_backward_of_backward, test_spectral_norm_matches_torch), are nowhere
looser than those tests' tolerances."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402
import test_hip_norm_branches as T  # noqa: E402

U = R.U


def test_norm_cases_reach_their_routes():
    T.check_all_routes()


def test_launch_plan_describe_refuses_bad_norm_arguments():
    import pcgan_amd
    from pcgan_amd import _lib, ops
    bad = [(_lib.PLAN_BN_COLREDUCE, 0, 8, 1), (_lib.PLAN_BN_COLREDUCE, 5, 8), (_lib.PLAN_BN_APPLY, 3, 5, 8, 1), (_lib.PLAN_BN_APPLY, 0, 5, 0, 1),
           (_lib.PLAN_BN_APPLY, 0, 5, 8), (_lib.PLAN_BN_FINALIZE, 0), (_lib.PLAN_BN_FINALIZE, 4, 4), (_lib.PLAN_INSTNORM, 3, 2, 4, 4, 1),
           (_lib.PLAN_INSTNORM, 0, 2, 0, 4, 1), (_lib.PLAN_INSTNORM, 0, 2, 4, 4), (_lib.PLAN_SPECTRAL_NORM, 2, 8, 8), (_lib.PLAN_SPECTRAL_NORM, 0, 257, 8),
           (_lib.PLAN_SPECTRAL_NORM, 1, 8, 257), (_lib.PLAN_SPECTRAL_NORM, 0, 8), (_lib.PLAN_ADAM + 1, 1)]
    for args in bad:
        with pytest.raises(pcgan_amd.PcgError, match="pcg_launch_plan_describe"):
            ops.launch_plan(*args)
    # a channel count that is no multiple of 4 streams scalar lanes whatever the pointers
    assert ops.launch_plan(_lib.PLAN_INSTNORM, 0, 2, 15, 6, 1) == ops.launch_plan(_lib.PLAN_INSTNORM, 0, 2, 15, 6, 0)


# ---- (2) references against autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,slope,dy_scale", [(R.ACT_NONE, 0.0, 1.0), (R.ACT_RELU, 0.0, 0.5), (R.ACT_LRELU, 0.2, 0.5)])
def test_reference_batchnorm_matches_autograd(act, slope, dy_scale):
    d = T.bn_inputs(37, 10)
    st = d["stats"]
    x, gamma, beta = d["x"][:, 2:], d["gamma"][2:], d["beta"][2:]            # the hard channels have their own test below
    mean, invstd = st["mean"][2:], st["invstd"][2:]
    torch.testing.assert_close(st["var"][2:], d["x"].var(0, unbiased=False)[2:], rtol=1e-9, atol=1e-14)
    ap = R.bn_apply(x, mean, invstd, gamma, beta, act, slope)
    n = F.batch_norm(x, None, None, gamma, beta, training=True, eps=R.f32_scalar(T.EPS))
    torch.testing.assert_close(ap["out"], n if act == R.ACT_NONE else F.leaky_relu(n, R.neg_of(act, slope)), rtol=1e-12, atol=1e-13)
    res = d["res"][:, 2:]
    torch.testing.assert_close(R.bn_apply(x, mean, invstd, gamma, beta, act, slope, res, 0.7)["out"], res + R.f32_scalar(0.7) * ap["out"], rtol=1e-13, atol=1e-14)
    ev = R.bn_apply(x, mean, st["var"][2:], gamma, beta, act, slope, var_eps=T.EPS)
    torch.testing.assert_close(ev["out"], ap["out"], rtol=1e-12, atol=1e-13)
    dy = d["dy"][:, 2:]
    ref = R.bn_bwd(dy, x, mean, invstd, gamma, ap["pre"], act, slope, dy_scale)
    dx, dg, db = R.bn_autograd(dy, x, gamma, beta, act, slope, T.EPS, dy_scale)
    torch.testing.assert_close(ref["dx"], dx, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(ref["dgamma"], dg, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(ref["dbeta"], db, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(ref["dcol"], dx.sum(0), rtol=0, atol=1e-11)
    rm = F.batch_norm(x, d["rm0"][2:].clone(), d["rv0"][2:].clone(), gamma, beta, training=True, momentum=R.f32_scalar(T.MOM), eps=1e-5)
    del rm
    rmean, rvar = d["rm0"].clone(), d["rv0"].clone()
    F.batch_norm(d["x"], rmean, rvar, None, None, training=True, momentum=R.f32_scalar(T.MOM), eps=1e-5)
    torch.testing.assert_close(st["rm"], rmean, rtol=1e-7, atol=1e-9)          # (1 - m) is the float32 difference in the reference
    torch.testing.assert_close(st["rv"][2:], rvar[2:], rtol=1e-7, atol=1e-9)


def test_reference_hard_channels():
    """Channel 0 is constant: variance exactly 0, invstd = 1 / sqrt(eps), output exactly beta.  Channel 1 has mean 100 and standard
    deviation about 0.01: a float32 accumulation of sum x^2 cannot resolve its variance (the 1-ulp bound on save_invstd can)."""
    for rows, C in [(c[0], c[1]) for c in T.BN_CASES]:
        d = T.bn_inputs(rows, C)
        st = d["stats"]
        assert float(st["var"][0]) == 0.0 and float(st["invstd"][0]) == 1.0 / np.sqrt(float(np.float32(1e-5)))
        ap = R.bn_apply(d["x"], d["mean32"], d["invstd32"], d["gamma"], d["beta"], R.ACT_NONE, 0.0)
        assert bool((ap["out"][:, 0] == d["beta"][0]).all()) and abs(float(d["beta"][0])) == 0.5
        assert abs(float(st["mean"][1]) - 100) < 0.02 and 0.003 < float(st["var"][1]) ** 0.5 < 0.03
        x1 = d["x"][:, 1].float()
        var_f32 = float((x1 * x1).sum() / rows - (x1.sum() / rows) ** 2)       # what a float accumulation makes of it
        assert abs(var_f32 - float(st["var"][1])) > 1e-2 * float(st["var"][1]) or rows < 5


@pytest.mark.parametrize("case", T.IN_CASES[:-1], ids=T._in_id)
def test_reference_instance_norm_matches_autograd(case):
    C, HW, _, fwd, bb = case
    rf = T.in_refs(C, HW, fwd, bb)
    d, f = rf["d"], rf["f"]
    kw = dict(rtol=1e-8, atol=1e-10)
    auto = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], T.EPS, T.SLOPE, d["dy"], d["r"])
    torch.testing.assert_close(f["n"], auto["n"], **kw)
    torch.testing.assert_close(R.act_out(f["n"], f["n_bound"], T.SLOPE)[0], auto["y"], **kw)
    assert float(f["invstd"][0, 0]) == 1.0 / np.sqrt(float(np.float32(1e-5)))          # the constant map
    torch.testing.assert_close(rf["bwd"]["dx"], auto["dx"], **kw)
    torch.testing.assert_close(rf["bwd"]["dgamma_part"].sum(0), auto["dgamma"], **kw)
    torch.testing.assert_close(rf["bwd"]["dbeta_part"].sum(0), auto["dbeta"], **kw)
    torch.testing.assert_close(rf["bb"]["ddy"], auto["ddy"], **kw)
    torch.testing.assert_close(rf["bb"]["ez"], auto["ez"], rtol=1e-7, atol=1e-9)
    torch.testing.assert_close(rf["bb"]["dgamma_part"].sum(0), auto["dgamma2"], rtol=1e-7, atol=1e-9)
    dn = R.f32_exact(d["cot"] * rf["mask"])
    auto_f = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], T.EPS, T.SLOPE, dn)
    torch.testing.assert_close(rf["fused"]["dx"], auto_f["dx"] + d["add"], **kw)
    torch.testing.assert_close(rf["fused"]["dxsum"], (auto_f["dx"] + d["add"]).sum(1), **kw)
    for k in ("dx", "dgamma_part", "dbeta_part", "dxsum"):
        assert bool((rf["fused"][k + "_bound"] >= 0).all()) and bool(torch.isfinite(rf["fused"][k + "_bound"]).all())


@pytest.mark.parametrize("case", T.SN_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_reference_spectral_norm_matches_autograd(case):
    O, I = case[0], case[1]
    d, calls, ev = T.sn_reference(O, I)
    u, v = d["u"], d["v"]
    for k, ref in enumerate(calls):
        w_bar, sigma, u, v = R.sn_fwd_by_hand(d["W"], u, v, 1e-12, True)
        for name, val in (("w_bar", w_bar), ("u", u), ("v", v)):
            torch.testing.assert_close(val, ref[name], rtol=1e-11, atol=1e-13)
        torch.testing.assert_close(R.sn_bwd_by_hand(d["dwbar"][k], w_bar, u, v, sigma), ref["dW"], rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(R.sn_fwd_by_hand(d["W"], u, v, 1e-12, False)[0], ev["w_bar"], rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ev["u"], calls[1]["u"], rtol=0, atol=0)


# ---- (3) the mask-gap condition ---------------------------------------------------------------------------------------------------
def test_mask_gap_condition_holds_for_every_table_seed():
    shapes = [(c[0], c[1]) for c in T.BN_CASES] + [T.BN_COLSUM_ONLY[:2]] + T.BN_KNOB_SHAPES
    for rows, C in dict.fromkeys(shapes):
        for what, ok, n_bad in T.bn_mask_gaps(rows, C):
            assert ok, f"{what}: {n_bad} pre-activations within 8 bounds of zero"
    for C, HW, _, fwd, _ in T.IN_CASES:
        ok, n_bad = T.in_mask_gap(C, HW, fwd)
        assert ok, f"instance norm C={C} HW={HW}: {n_bad} pre-activations within 8 bounds of zero"


# ---- (4) the new bounds are no looser than the older tests' tolerances, at those tests' inputs ----------------------------------------
def _leq(bound, tol, what):
    worst = float((bound / (tol * (1 + 1e-12))).max())
    assert worst <= 1.0, f"{what}: the new bound is {worst:.2f} x the older tolerance somewhere"


@pytest.mark.parametrize("rows,C", [(4 * 16 * 16, 128), (4 * 8 * 8, 256), (6 * 28 * 28, 64), (37, 10), (1000, 512), (5, 8)])
@pytest.mark.parametrize("act,slope", [(R.ACT_RELU, 0.0), (R.ACT_LRELU, 0.2)])
def test_batchnorm_bounds_against_test_batchnorm_fwd_bwd(rows, C, act, slope):
    rng = np.random.default_rng(rows + C)
    x = (rng.standard_normal((rows, C)) * 1.5 + 0.3).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C)).astype(np.float32)
    dy = rng.standard_normal((rows, C)).astype(np.float32)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), (1 + rng.random(C)).astype(np.float32)
    x, gamma, beta, dy, rm0, rv0 = (torch.from_numpy(a).double() for a in (x, gamma, beta, dy, rm0, rv0))
    st = R.bn_stats(x, 1e-5, 0.1, rm0, rv0)
    for k in ("mean", "invstd"):
        _leq(R.ulp32(R.f32_exact(st[k])) + U * st[k].abs(), 1e-5 * st[k].abs() + 1e-6, k)
    _leq(st["rm_bound"], 1e-5 * st["rm"].abs() + 1e-6, "running_mean")
    _leq(st["rv_bound"], 1e-5 * st["rv"].abs() + 1e-6, "running_var")
    m32, i32 = R.f32_exact(st["mean"]), R.f32_exact(st["invstd"])
    ap = R.bn_apply(x, m32, i32, gamma, beta, act, slope)
    _leq(ap["bound"], 2e-5 * ap["out"].abs() + 2e-6, "y")
    ev = R.bn_apply(x, R.f32_exact(st["rm"]), R.f32_exact(st["rv"]), gamma, beta, act, slope, var_eps=1e-5)
    _leq(ev["bound"], 2e-5 * ev["out"].abs() + 2e-6, "y (evaluation form)")
    bw = R.bn_bwd(dy, x, m32, i32, gamma, ap["pre"], act, slope)
    scale = rows ** 0.5
    _leq(R.accumulated(bw["dgamma"], bw["dgamma_bound"], 1.0)[1], 1e-4 * bw["dgamma"].abs() + 2e-5 * scale, "dgamma")
    _leq(R.accumulated(bw["dbeta"], bw["dbeta_bound"], -1.0)[1], 1e-4 * bw["dbeta"].abs() + 2e-5 * scale, "dbeta")
    _leq(bw["dx_bound"], 1e-4 * bw["dx"].abs() + 2e-5, "dx")


@pytest.mark.parametrize("B,C,H,W", [(3, 4, 13, 13), (2, 8, 6, 6), (5, 16, 2, 2), (2, 256, 13, 13), (3, 1024, 2, 2), (2, 100, 3, 5),
                                     (2, 1024, 2, 2), (2, 512, 6, 6), (2, 256, 13, 13)])
def test_instance_norm_bounds_against_the_older_test(B, C, H, W):
    """The last three shapes are that test's bench shapes with its B = 256 / 256 / 64 cut to 2: every bound here is per sample."""
    from pcgan_amd import _lib, ops
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1.7 + 0.3
    gamma = torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    r = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    HW = H * W
    nhwc = lambda t: R.f32_exact(t.reshape(B, C, HW).permute(0, 2, 1))
    x, dy, r, gamma, beta = nhwc(x), nhwc(dy), nhwc(r), R.f32_exact(gamma), R.f32_exact(beta)
    fwd, bb = (ops.launch_plan(_lib.PLAN_INSTNORM, p, B, HW, C, 1) for p in (0, 2))
    f = R.instnorm_fwd(x, gamma, beta, 1e-5, *T.in_plan_numbers(fwd, HW), T.RSQRT_U)
    y, y_bound = R.act_out(f["n"], f["n_bound"], 0.2)
    _leq(R.in_bound("y", y_bound, y), 2e-5 * y.abs() + 2e-5, "y")
    b = R.instnorm_bwd(f, dy, gamma)
    _leq(R.in_bound("dx", b["dx_bound"], b["dx"]), 1e-4 * b["dx"].abs() + 2e-5 * float(b["dx"].abs().max()), "dx")
    for k in ("dgamma", "dbeta"):
        s = b[k + "_part"].sum(0)
        _leq(R.in_bound(k, b[k + "_part_bound"].sum(0), s), 1e-4 * s.abs() + 2e-5 * float(s.abs().max()) + 1e-5, k)
    f2 = dict(f, K=R.instnorm_fwd(x, gamma, beta, 1e-5, *T.in_plan_numbers(bb, HW), T.RSQRT_U)["K"])
    q = R.instnorm_bwd_bwd(f2, r, dy, gamma)
    _leq(R.in_bound("ddy", q["ddy_bound"], q["ddy"]), 1e-4 * q["ddy"].abs() + 2e-5 * float(q["ddy"].abs().max()), "ddy")
    _leq(R.in_bound("ez", q["ez_bound"], q["ez"], q["ez_floor"]), 2e-4 * q["ez"].abs() + 5e-5 * float(q["ez"].abs().max()), "ez")
    s = q["dgamma_part"].sum(0)
    _leq(R.in_bound("dgamma2", q["dgamma_part_bound"].sum(0), s), 2e-4 * s.abs() + 5e-5 * float(s.abs().max()) + 1e-5, "dgamma (second order)")


def test_spectral_norm_bounds_are_the_older_tests():
    assert R.SN_TOL == dict(u=(1e-5, 1e-6), v=(1e-5, 1e-6), w_bar=(1e-5, 1e-6), dW=(2e-4, 1e-5))
    ref = torch.tensor([[0.5, -2.0], [0.0, 1e-3]], dtype=torch.float64)
    torch.testing.assert_close(R.sn_bound("dW", ref), 2e-4 * ref.abs() + 1e-5 * 2.0, rtol=0, atol=0)
    torch.testing.assert_close(R.sn_bound("w_bar", ref), 1e-5 * ref.abs() + 1e-6, rtol=0, atol=0)
