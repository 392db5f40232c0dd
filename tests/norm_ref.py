"""Float64 references of the normalisation kernels (csrc/batchnorm.hip, instnorm.hip, spectral_norm_body.h) and the error bounds
tests/test_hip_norm_branches.py holds them to.  Plain torch on the CPU.  The hand-written backwards (BatchNorm with dy_scale,
InstanceNorm first and second order, spectral norm) are pinned to torch.float64 autograd by tests/test_norm_plan_host.py, so a wrong
reference fails there and not on the GPU.  Every function takes float64 tensors whose values are exact in float32 (the test rounds
first: the reference sees the kernel's operands) and returns, beside the value, the bound derived from the kernel's arithmetic.

u = 2^-24.  "K" below is the reduction constant (chain + lanes + 2) u of an fp32 sum: the longest per-thread chain, the number of
partial sums added in order behind it, and two roundings of the terms themselves."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def f32_exact(t):
    return t.float().double()


def f32_scalar(v):
    """The float32 a C float argument becomes, as a Python float."""
    return float(np.float32(v))


def neg_of(act, slope):
    return 1.0 if act == ACT_NONE else (0.0 if act == ACT_RELU else f32_scalar(slope))


def ulp32(t):
    """Spacing of float32 at |t| (t: float64 tensor of float32 values)."""
    return torch.from_numpy(np.spacing(np.abs(t.numpy()).astype(np.float32)).astype(np.float64))


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------
def bn_stats(x, eps, momentum, rm0=None, rv0=None):
    """Training statistics of x [rows][C]: dict(mean, invstd, var) in float64 (two-pass variance: no cancellation) and, with running
    statistics, their update and its bound 3u (|(1 - m) r| + |m s|)."""
    rows = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    eps, m = f32_scalar(eps), f32_scalar(momentum)
    out = dict(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps))
    if rm0 is not None:
        unb = var * (rows / (rows - 1.0) if rows > 1 else 1.0)
        one_m = float(np.float32(1.0) - np.float32(momentum))
        out.update(rm=one_m * rm0 + m * mean, rm_bound=3 * U * ((one_m * rm0).abs() + (m * mean).abs()),
                   rv=one_m * rv0 + m * unb, rv_bound=3 * U * ((one_m * rv0).abs() + (m * unb).abs()))
    return out


def bn_apply(x, mean, stat, gamma, beta, act, slope, residual=None, alpha=1.0, var_eps=-1.0):
    """alpha * act((x - mean) * gamma * invstd + beta) + residual, as csrc/batchnorm.hip folds it: sc = gamma * invstd [1 rounding],
    sh = fma(-mean, sc, beta) [1], pre = fma(x, sc, sh) [1]: 3 u (|x sc| + |mean sc| + |beta|) before the activation (c = 3); the
    evaluation form computes invstd = 1 / sqrtf(var + eps) itself [add, sqrt, divide, each correctly rounded: 2.5 u relative on sc],
    c = 6.  The activation is 1- or slope-Lipschitz on the side the reference is on (the mask-gap condition keeps the device on the
    same side) and multiplies by the slope [1]; alpha * a + residual is one fma [1].
    Returns dict(out, bound, pre, pre_bound)."""
    C = x.shape[1]
    g = gamma if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = beta if beta is not None else torch.zeros(C, dtype=torch.float64)
    invstd = stat if var_eps < 0 else 1.0 / torch.sqrt(stat + f32_scalar(var_eps))
    sc = g * invstd
    pre = (x - mean) * sc + b
    mag = (x * sc).abs() + (mean * sc).abs() + b.abs()
    c = 3 if var_eps < 0 else 6
    pre_bound = c * U * mag
    neg = neg_of(act, slope)
    lip = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, neg))
    a = pre * lip
    al = f32_scalar(alpha)
    out = al * a + (residual if residual is not None else 0.0)
    bound = abs(al) * (lip * pre_bound + (U * a.abs() if act == ACT_LRELU else 0.0))
    if residual is not None or al != 1.0:
        bound = bound + U * ((al * a).abs() + (residual.abs() if residual is not None else 0.0))
    return dict(out=out, bound=bound, pre=pre, pre_bound=pre_bound)


def bn_bwd(dy, x, mean, invstd, gamma, pre, act, slope, dy_scale=1.0):
    """BatchNorm(train) + activation backward by hand.  dz = dy_scale * dy * act'(pre) [2 roundings], xh = (x - mean) * invstd [2];
    dbeta = sum dz, dgamma = sum dz xh are fp64 sums of exact products of those fp32 terms: 2 u sum|dz| and 4 u sum|dz xh|, plus
    one output rounding (the caller adds the rounding of an accumulating add).  dx = k0 (dz - k1 - xh k2) with k0 = gamma invstd [1],
    k1 = mean(dz) and k2 = mean(dz xh) [the sums' error over rows, + 1 each], three roundings inside the bracket and one outside:
      u |k0| (6 |dz| + 5 |k1| + 2 mean|dz| + 7 |xh k2| + 4 |xh| mean|dz xh|).
    dcol, the column sums of the dx the kernel wrote (fp64), carries the sum of those bounds plus one output rounding."""
    rows, C = x.shape
    neg = neg_of(act, slope)
    grad = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, neg)) if act != ACT_NONE else torch.ones_like(x)
    dz = f32_scalar(dy_scale) * dy * grad
    xh = (x - mean) * invstd
    sdz, sdzx, mdz, mdzx = dz.sum(0), (dz * xh).sum(0), dz.abs().sum(0), (dz * xh).abs().sum(0)
    k0 = (gamma if gamma is not None else torch.ones(C, dtype=torch.float64)) * invstd
    k1, k2 = sdz / rows, sdzx / rows
    dx = k0 * (dz - k1 - xh * k2)
    dx_bound = U * k0.abs() * (6 * dz.abs() + 5 * k1.abs() + 2 * mdz / rows + 7 * (xh * k2).abs() + 4 * xh.abs() * mdzx / rows)
    return dict(dx=dx, dx_bound=dx_bound, dbeta=sdz, dbeta_bound=2 * U * mdz + U * sdz.abs(), dgamma=sdzx,
                dgamma_bound=4 * U * mdzx + U * sdzx.abs(), dcol=dx.sum(0), dcol_bound=dx_bound.sum(0) + U * dx.sum(0).abs(), dz=dz, xh=xh)


def accumulated(value, bound, old):
    """(old + value, bound + u |old + value|): a float32 `+=` into a non-zero buffer."""
    return old + value, bound + U * (old + value).abs()


def bn_autograd(dy, x, gamma, beta, act, slope, eps, dy_scale=1.0):
    """(dx, dgamma, dbeta) of dy_scale * <dy, act(batch_norm(x))> by torch.float64 autograd (host check of bn_bwd)."""
    xr, g, b = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    n = F.batch_norm(xr, None, None, g, b, training=True, eps=f32_scalar(eps))
    y = n if act == ACT_NONE else F.leaky_relu(n, neg_of(act, slope))
    return torch.autograd.grad(y, [xr, g, b], f32_scalar(dy_scale) * dy)


# ---- InstanceNorm (NHWC: [B][HW][C]) ---------------------------------------------------------------------------------------------
def _to_nchw(t):
    return t.permute(0, 2, 1).unsqueeze(-1)          # [B][C][HW][1]


def _to_nhwc(t):
    return t.squeeze(-1).permute(0, 2, 1)


def instnorm_autograd(x, gamma, beta, eps, slope, d, r=None, add=None):
    """float64 autograd of z -> InstanceNorm -> LeakyReLU: dict(n, y; dx, dgamma, dbeta for the cotangent `d` on n; with a second
    cotangent r on dx (create_graph=True): ddy, ez, dgamma2).  Everything [B][HW][C] / [C]."""
    xr = _to_nchw(x).clone().requires_grad_(True)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dr = _to_nchw(d).clone().requires_grad_(True)
    n = F.instance_norm(xr, weight=g, bias=b, eps=f32_scalar(eps))
    dx, dg, db = torch.autograd.grad(n, [xr, g, b], dr, create_graph=True)
    out = dict(n=_to_nhwc(n.detach()), y=_to_nhwc(F.leaky_relu(n.detach(), f32_scalar(slope))), dx=_to_nhwc(dx.detach()), dgamma=dg.detach(),
               dbeta=db.detach())
    if r is not None:
        ddy, ez, dg2 = torch.autograd.grad(dx, [dr, xr, g], _to_nchw(r))
        out.update(ddy=_to_nhwc(ddy), ez=_to_nhwc(ez), dgamma2=dg2)
    return out


def instnorm_fwd(x, gamma, beta, eps, np_, lanes, rsqrt_u):
    """Forward by hand with its bounds.  K = (np + lanes + 2) u.  mean = sum x / HW: K mean|x| + u |mean|.  var = sum (x - mean)^2 / HW
    + eps: K var + 2 mean|d| e_mean + e_mean^2 + 2 u var + 2 u (var + eps).  invstd = rsqrtf(var + eps): half the relative error of its
    argument plus rsqrt_u u (the measured allowance for rsqrtf).  n = fma(x - mean, gamma invstd, beta): the errors of its operands
    plus three roundings."""
    HW = x.shape[1]
    K = (np_ + lanes + 2) * U
    eps = f32_scalar(eps)
    mean = x.mean(1, keepdim=True)
    e_mean = K * x.abs().mean(1, keepdim=True) + U * mean.abs()
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    e_var = K * var + 2 * d.abs().mean(1, keepdim=True) * e_mean + e_mean ** 2 + 2 * U * var + 2 * U * (var + eps)
    invstd = 1.0 / torch.sqrt(var + eps)
    rho = 0.5 * e_var / (var + eps) + rsqrt_u * U          # relative error of invstd
    xh = d * invstd
    e_xh = (e_mean + U * d.abs()) * invstd + xh.abs() * (rho + U)
    n = gamma * xh + beta
    e_n = gamma.abs() * e_xh + U * (gamma * xh).abs() + U * ((gamma * xh).abs() + beta.abs())
    return dict(mean=mean.squeeze(1), mean_bound=e_mean.squeeze(1), invstd=invstd.squeeze(1), invstd_bound=(rho * invstd).squeeze(1),
                n=n, n_bound=e_n, xh=xh, e_xh=e_xh, rho=rho, K=K, is_=invstd, e_mean=e_mean)


def act_out(n, n_bound, slope, act=ACT_LRELU):
    neg = neg_of(act, slope)
    lip = torch.where(n > 0, torch.ones_like(n), torch.full_like(n, neg))
    return n * lip, lip * n_bound + (U * (n * lip).abs() if act == ACT_LRELU else 0.0)


def instnorm_bwd(f, d, gamma, d_rounded=False, add=None):
    """Backward by hand from the forward record f: s0 = sum d, s1 = sum d xh (K sum|terms| + the terms' own error); dbeta_part = s0,
    dgamma_part = s1; dx = gamma invstd (d - s0/HW - xh s1/HW) (+ add); dxsum = sum dx over the map (K sum|dx| + the sum of dx's bounds).
    d_rounded: d is the product of the cotangent with the LeakyReLU slope [1 rounding]."""
    HW = d.shape[1]
    K, xh, e_xh, rho, is_ = f["K"], f["xh"], f["e_xh"], f["rho"], f["is_"]
    e_d = U * d.abs() if d_rounded else torch.zeros_like(d)
    s0, s1 = d.sum(1, keepdim=True), (d * xh).sum(1, keepdim=True)
    e0 = K * d.abs().sum(1, keepdim=True) + e_d.sum(1, keepdim=True)
    e1 = K * (d * xh).abs().sum(1, keepdim=True) + (d.abs() * e_xh + e_d * xh.abs()).sum(1, keepdim=True)
    m1, m2 = s0 / HW, s1 / HW
    e_m1, e_m2 = e0 / HW + 2 * U * m1.abs(), e1 / HW + 2 * U * m2.abs()
    g = gamma * is_
    t = d - m1 - xh * m2
    e_t = e_d + e_m1 + e_xh * m2.abs() + xh.abs() * e_m2 + 3 * U * (d.abs() + m1.abs() + (xh * m2).abs())
    dx = g * t
    e_dx = g.abs() * e_t + dx.abs() * (rho + 2 * U)
    if add is not None:
        dx = dx + add
        e_dx = e_dx + U * dx.abs()
    dxsum = dx.sum(1)
    return dict(dx=dx, dx_bound=e_dx, dgamma_part=s1.squeeze(1), dgamma_part_bound=e1.squeeze(1), dbeta_part=s0.squeeze(1),
                dbeta_part_bound=e0.squeeze(1), dxsum=dxsum, dxsum_bound=K * dx.abs().sum(1) + e_dx.sum(1))


def instnorm_bwd_bwd(f, r, dy, gamma, dy_rounded=False):
    """Backward of the backward by hand (the formulas at the top of csrc/instnorm.hip), each bound first-order in the errors of the
    sums (K sum|terms| + the terms' own error), of xh and of invstd, plus the roundings of the expression itself."""
    HW = r.shape[1]
    K, xh, e_xh, rho, is_ = f["K"], f["xh"], f["e_xh"], f["rho"], f["is_"]
    e_dy = U * dy.abs() if dy_rounded else torch.zeros_like(dy)
    sm = lambda t: t.sum(1, keepdim=True)
    mr, q, md, m = sm(r) / HW, sm(r * xh) / HW, sm(dy) / HW, sm(dy * xh) / HW
    e_mr = K * sm(r.abs()) / HW + 2 * U * mr.abs()
    e_q = (K * sm((r * xh).abs()) + sm(r.abs() * e_xh)) / HW + 2 * U * q.abs()
    e_md = (K * sm(dy.abs()) + sm(e_dy)) / HW + 2 * U * md.abs()
    e_m = (K * sm((dy * xh).abs()) + sm(dy.abs() * e_xh + e_dy * xh.abs())) / HW + 2 * U * m.abs()
    rt, a = r - mr, dy - md
    e_rt, e_a = e_mr + U * rt.abs(), e_md + e_dy + U * a.abs()
    pp = sm(rt * a) / HW
    e_pp = (K * sm((rt * a).abs()) + sm(e_rt * a.abs() + rt.abs() * e_a)) / HW + 2 * U * pp.abs()
    dg = is_ * HW * (pp - m * q)
    e_dg = dg.abs() * (rho + 3 * U) + is_ * HW * (e_pp + e_m * q.abs() + m.abs() * e_q + 2 * U * (pp.abs() + (m * q).abs()))
    g1, g2 = gamma * is_, -gamma * is_ * is_
    k3 = pp - 3 * m * q
    e_k3 = e_pp + 3 * (e_m * q.abs() + m.abs() * e_q) + 3 * U * (pp.abs() + 3 * (m * q).abs())
    o1 = g1 * (rt - xh * q)
    e_o1 = g1.abs() * (e_rt + e_xh * q.abs() + xh.abs() * e_q + 2 * U * (rt.abs() + (xh * q).abs())) + o1.abs() * (rho + 2 * U)
    o2 = g2 * (q * a + m * rt + k3 * xh)
    e_o2 = g2.abs() * (e_q * a.abs() + q.abs() * e_a + e_m * rt.abs() + m.abs() * e_rt + e_k3 * xh.abs() + k3.abs() * e_xh
                       + 3 * U * ((q * a).abs() + (m * rt).abs() + (k3 * xh).abs())) + o2.abs() * (2 * rho + 3 * U)
    ez_floor = g2.abs() * 3 * U * ((q * a).abs() + (m * rt).abs() + (k3 * xh).abs()) + 3 * U * o2.abs()      # the expression's own roundings
    return dict(ddy=o1, ddy_bound=e_o1, ez=o2, ez_bound=e_o2, ez_floor=ez_floor, dgamma_part=dg.squeeze(1), dgamma_part_bound=e_dg.squeeze(1))


# (rtol, atol as a multiple of max|ref|, absolute atol) of test_instance_norm_forward_backward_and_backward_of_backward
IN_OLDER_TOL = dict(y=(2e-5, 0.0, 2e-5), dx=(1e-4, 2e-5, 0.0), dgamma=(1e-4, 2e-5, 1e-5), dbeta=(1e-4, 2e-5, 1e-5), ddy=(1e-4, 2e-5, 0.0),
                    ez=(2e-4, 5e-5, 0.0), dgamma2=(2e-4, 5e-5, 1e-5))


def in_bound(name, derived, ref, floor=None):
    """The bound an InstanceNorm output is held to: the derived worst-case bound, or the older test's tolerance at the same reference
    where that is smaller (a 256-lane reduction's worst case exceeds it), so that no bound here is looser than that test's.
    floor: the roundings of the output's own expression, which no fp32 evaluation avoids -- the older tolerance is relative to
    max|ref|, and where a whole output is cancellation residue (ez of a 2-position map: the terms are O(1), their sum 1e-6) it falls
    below that; the cap never goes under the floor."""
    rtol, arel, aabs = IN_OLDER_TOL[name]
    cap = rtol * ref.abs() + arel * float(ref.abs().max()) + aabs
    return torch.minimum(derived, cap if floor is None else torch.maximum(cap, floor))


# ---- spectral norm ---------------------------------------------------------------------------------------------------------------
SN_TOL = dict(u=(1e-5, 1e-6), v=(1e-5, 1e-6), w_bar=(1e-5, 1e-6), dW=(2e-4, 1e-5))     # (rtol, atol [dW: x max|dW|]) of test_spectral_norm_matches_torch


def sn_bound(name, ref):
    rtol, atol = SN_TOL[name]
    return rtol * ref.abs() + atol * (float(ref.abs().max()) if name == "dW" else 1.0)


def sn_module(W, u, v):
    """torch.nn.utils.spectral_norm(Linear) in float64 holding exactly these weight_orig, u, v."""
    O, I = W.shape
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(I, O, bias=False).double(), eps=1e-12)
    with torch.no_grad():
        lin.weight_orig.copy_(W); lin.weight_u.copy_(u); lin.weight_v.copy_(v)
    return lin


def sn_forward(lin, dwbar=None):
    """One forward of the module in its current mode: dict(w_bar, u, v[, dW for the cotangent dwbar on w_bar])."""
    lin.zero_grad()
    lin(torch.zeros(1, lin.in_features, dtype=torch.float64))
    out = dict(w_bar=lin.weight.detach().clone(), u=lin.weight_u.detach().clone(), v=lin.weight_v.detach().clone())
    if dwbar is not None:
        (lin.weight * dwbar).sum().backward()
        out["dW"] = lin.weight_orig.grad.detach().clone()
    return out


def sn_fwd_by_hand(W, u, v, eps, power_iteration):
    """(w_bar, sigma, u, v) of one call: v <- normalize(W^T u), u <- normalize(W v), sigma = u . W v."""
    if power_iteration:
        t = W.T @ u
        v = t / max(float(t.norm()), eps)
        w = W @ v
        u = w / max(float(w.norm()), eps)
    sigma = u @ (W @ v)
    return W / sigma, sigma, u, v


def sn_bwd_by_hand(dwbar, w_bar, u, v, sigma):
    """dW = (dWbar - <dWbar, Wbar> u v^T) / sigma"""
    return (dwbar - (dwbar * w_bar).sum() * torch.outer(u, v)) / sigma


def mask_gap_ok(pre, pre_bound):
    """The mask-gap condition: no non-zero pre-activation of the reference within 8x its own bound of zero."""
    bad = (pre != 0) & (pre.abs() <= 8 * pre_bound)
    return not bool(bad.any()), int(bad.sum())


def chain_len(n, threads):
    return int(math.ceil(n / threads))
