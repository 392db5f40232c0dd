"""Float64 references and derived error bounds of the front half of csrc/pointwise.hip -- the fused Adam step (adam_kernel<4> /
adam_kernel<1>: adam_one, and adam_upd of csrc/epoch_wg.h) and the three BCE kernels -- what tests/test_hip_optim_branches.py compares
the HIP kernels with.  tests/test_optim_plan_host.py pins these references to torch.optim.Adam / AdamW and to torch autograd in
float64, so a wrong reference fails there and not on the GPU.

u = 2^-24 is the unit roundoff of float32: one fp32 operation returns its exact result times (1 + d), |d| <= u.  Every bound below is
first order in u and per element, in float64; the factor SLACK = 1 + 2^-10 covers the second-order terms (u^2, some 6e-8 of a bound)
and the float64 reference's own roundings (2^-53 against 2^-24: 2e-9 of a bound).  Division and square root are taken as correctly
rounded (one u each): that is the compiler's default for HIP device code and the build passes no fast-math flag -- a kernel built
with the approximate forms is meant to fail here.

Adam, one step
--------------
The reference takes the device's own fp32 state before the step (p, m, v) and the fp32 gradient, promotes them to float64 and applies
torch's formulas with the hyper-parameters as the Python doubles the caller passes.  Each step is checked on its own ("teacher
forced"), so nothing compounds.  The kernel works with fp32 roundings of the constants, each within u of the double:
lr, wd, w1 = 1 - beta1, 1 - w1, beta2, 1 - beta2, eps, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) (the last two are
formed in double on the host or on the device and rounded once).  E_x is the bound on |x_device - x_float64|:

  decay     decoupled: p' = p * (1 - lr * wd), c = 1 - lr wd: the product lr * wd carries 3 u (two constants, one rounding), the
            difference one, the product with p one:            E_p' = u (2 |p c| + 3 |p| lr wd)
            L2: g' = fmaf(wd, p, g): the constant and one rounding:
                                                                 E_g' = u (2 |wd p| + |g|)            (no decay: both 0)
  m         with d = g' - m (one rounding, u |d|), rho(c) <= u the actual relative error of the fp32 constant c (computed here, not
            bounded: test_adam's tolerance on a cancelled m leaves no room for a rounding that does not happen), and the final
            rounding scaled by the result it rounds:
            w1 <  0.5f:  m' = fmaf(w1, d, m):        E_m = w1 E_g' + (u + rho(w1)) w1 |d| + u |m'|
            w1 >= 0.5f:  m' = g' - d * (1 - w1):     the product carries E_d, its constant and its own rounding -- none when 1 - w1 is a
                         power of two or zero (beta1 = 0.5, 0: the product is exact) --, the difference one more (none if the compiler
                         contracts it into an fma).  g' enters twice with the same error, net factor w1:
                                                                 E_m = w1 E_g' + (u + rho(1 - w1) + u [product]) (1 - w1) |d| + u |m'|
  v         v' = fmaf(v, beta2, (1 - beta2) g' g'), T = (1 - beta2) g'^2: T carries its constant and two roundings (3 u T) and twice the
            relative error of g'; the fma its constant and one rounding:
                                                                 E_v = u (4 T + 2 |v beta2|) + 2 (1 - beta2) |g'| E_g'
  denom     S = sqrtf(v') / bc2_sqrt: half the relative error of v', the square root, the constant, the division:
                                                                 E_S = S (E_v / (2 v') + 3 u)
            denom = S + eps:                                     E_den = E_S + u eps + u denom
  p         r = m' / denom:                                      E_r = E_m / denom + |r| (E_den / denom + u)
            q = step_size * r: its constant and its rounding:    E_q = step_size E_r + 2 u |q|
            p - q: one rounding.  Whether the compiler contracts p - step_size * r into one fma is not assumed: that only removes
            the rounding of q, and the bound holds either way:   E_p = E_p' + E_q + u (|p'| + |q|)

Every term scales with the magnitude sum of what it rounds, never with a cancelled result.  The two instantiations and the tail
lanes run the same adam_one, so one bound serves all of them.

Compounding (three steps against torch.optim.Adam in float64, the segments test).  The float64 run starts from the same fp32
parameters and sees the same fp32 gradients; after step k the device's state is off by at most (E_p, E_m, E_v)_k.  Step k + 1 applies
the same map to the perturbed state, so its bound is the one-step bound evaluated on the float64 trajectory plus the incoming errors
carried through the same first-order expressions: E_p enters p' with |c| (and g' with wd for L2), E_m enters d, hence m' with
1 - w1, E_v enters v' with beta2.  adam_step takes the incoming errors as `err_in`; chaining three calls is the compounded bound.

BCE
---
Each kernel is one block of 256 threads: thread j adds its terms j, j + 256, ... in fp32 (a chain of L = ceil(n / 256) additions), then
block_sum_256 adds the 256 partial sums in a tree of depth T = 9 (six butterfly steps inside a wave, three additions over the four
waves), and the sum is multiplied by 1 / n (two more roundings):
  loss      ((L + T + 2) u sum|terms| + sum of the per-term errors) / n
Device logf / log1pf / expf: FN_ULP = 2 ulp each, a relative error of 2 * 2^-23 = 4 u -- the figure tests/test_hip_rng_exact.py takes
from HIP's math API documentation for single precision without fast-math and holds logf to; it is applied to the other two
unchanged.  tests/test_optim_plan_host.py checks that with it every bound stays inside the tolerances of test_bce_losses.
  bce       term = (t - 1) lq - t lp, lp = max(logf(p), -100), lq = max(log1pf(-p), -100) (max is 1-Lipschitz, -p is exact): each part
            carries its function value (4 u), t - 1 (one, exact for t in [0.5, 2]), its product and the difference:
                                                                 7 u (|t lp| + |(1 - t) lq|)
            gradient gs / n * (p - t) / max((1 - p) p, 1e-12f), gs = grad_scale * grad_out: eight roundings (gs, 1 / n, their product,
            p - t, that product, 1 - p, the product with p, the division), all relative; the clamp is the float constant 1e-12f in
            torch as well (also when it computes in float64), so the reference clamps at that very number:
                                                                 8 u |dp|
            plus gradual underflow, ETA = 2^-150 (half the smallest fp32 subnormal) per result that can fall below the normal range:
            the product gs / n * (p - t) (p a denormal, t = 0) is formed before the division, which scales its ETA by 1 / den; so
            are the errors of den's own product and of gs / n; the quotient adds one more:
                                                                 ETA ((1 + |p - t| + |dp|) / den + 1)
  pair      the two halves as above; gs of half h = g_h + g2 (missing: 0; all three missing: 1), one rounding like the product with
            grad_out; loss[2] is the fp32 sum of the device's loss[0] and loss[1] (compared exactly).
  logits    term = (1 - t) x + mx + logf(expf(-mx) + expf(-x - mx)), mx = max(-x, 0); -x - mx is exact.  With a = (1 - t) x, b = mx,
            s the sum of the two exponentials (1 <= s <= 2), c = log s: 1 - t and the product 2 u |a|, the first sum u |a + b| (the
            sum it rounds: for x < 0 the two cancel to -t x), the exponentials 4 u s and their sum u s, through the logarithm
            (d log s = ds / s) 5 u, logf itself 4 u c, the last sum u |a + b + c|:
                                                                 u (2 |a| + |a + b| + |a + b + c| + 4 c + 5)
            The terms the chain adds are the finished a + b + c >= 0.
            gradient gs / n * (sig - t), sig = 1 / (1 + expf(-x)): expf's 4 u e reaches sig as 4 u sig (1 - sig); the sum and the
            division one u sig each -- together at most 2 u = 2^-23, one fp32 ulp of 1.0: the absolute floor test_bce_losses argues for
            (sig - t cancels in fp32 when |x| is large; it also covers expf overflowing to inf, where sig is 0 for a float64 value
            below 1e-38).  sig - t, 1 / n, gs and the two products: five relative roundings:
                                                                 |gs| / n (2^-23 + 4 u sig (1 - sig)) + 5 u |dz|
"""
import math

import numpy as np
import torch

U = 2.0 ** -24        # unit roundoff of float32
SLACK = 1.0 + 2.0 ** -10
ETA = 2.0 ** -150      # half the smallest fp32 subnormal: the absolute error of a result that underflows gradually
FN_ULP = 2            # device logf / log1pf / expf, in fp32 ulps (tests/test_hip_rng_exact.py)
FN_U = 2 * FN_ULP     # the same in units of u
TREE_DEPTH = 9        # block_sum_256: six __shfl_xor steps, then red[0] + red[1] + red[2] + red[3]
BCE_THREADS = 256
BCE_DENOM_CLAMP = float(np.float32(1e-12))      # torch's `constexpr float EPSILON = 1e-12`, the kernel's 1e-12f


def f32_exact(t):
    """float64 values that are exactly representable in float32."""
    return t.float().double()


def f32_scalar(x):
    """The float64 value of the float32 rounding of a Python float (what a `float` argument of the C ABI becomes)."""
    return float(np.float32(x))


def beta1_just_above_half():
    """The smallest double above 0.5 whose 1 - beta1 rounds below 0.5f.  The fp32 neighbour below 0.5 is 0.5 - 2^-25; the midpoint
    0.5 - 2^-26 is a tie that rounds to the even 0.5, so 1 - beta1 (exact in double for beta1 in [0.5, 1]) must lie below the
    midpoint: beta1 is the double after 0.5 + 2^-26."""
    b = float(np.nextafter(0.5 + 2.0 ** -26, 1.0))
    assert np.float32(1.0 - b) < np.float32(0.5) and np.float32(1.0 - (0.5 + 2.0 ** -26)) == np.float32(0.5)
    return b


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
def lerp_takes_first_form(beta1):
    """adam_upd's switch: the fp32 weight 1 - beta1 below 0.5f."""
    return bool(np.float32(1.0 - beta1) < np.float32(0.5))


def _rho(c):
    """The relative error of the fp32 rounding of the constant c (at most u)."""
    return abs(float(np.float32(c)) - c) / abs(c) if c != 0.0 else 0.0


def _product_exact(c):
    """A product with the fp32 constant c is exact: c is zero or a power of two (no overflow or underflow at these magnitudes)."""
    c = float(np.float32(c))
    return c == 0.0 or math.frexp(c)[0] == 0.5


def adam_step(p, g, m, v, t, lr, beta1, beta2, eps, wd=0.0, decoupled=False, err_in=None):
    """One torch.optim.Adam (decoupled: AdamW) step number t on float64 tensors.  Returns {"p", "m", "v", "p_bound", "m_bound",
    "v_bound"}: the new state and the per-element bounds of the module docstring.  err_in = (E_p, E_m, E_v) are bounds on the error
    the incoming state already carries (compounding); None: the state is the device's own."""
    z = torch.zeros_like(p)
    Ep, Em, Ev = (z, z, z) if err_in is None else err_in
    w1 = 1.0 - beta1
    if wd != 0.0 and decoupled:
        c = 1.0 - lr * wd
        p1 = p * c
        E_p1 = U * (2 * p1.abs() + 3 * p.abs() * lr * wd) + abs(c) * Ep
        g1, E_g = g, z
    elif wd != 0.0:
        g1 = g + wd * p
        E_g = U * (2 * (wd * p).abs() + g.abs()) + abs(wd) * Ep
        p1, E_p1 = p, Ep
    else:
        p1, E_p1, g1, E_g = p, Ep, g, z
    d = g1 - m
    m1 = m + w1 * d                                        # exp_avg.lerp_(grad, 1 - beta1)
    if lerp_takes_first_form(beta1):
        E_m = w1 * E_g + (U + _rho(w1)) * w1 * d.abs() + U * m1.abs()
    else:
        om = 1.0 - w1                                      # the kernel's constant is the fp32 rounding of this double
        E_m = w1 * E_g + (U + _rho(om) + (0.0 if _product_exact(om) else U)) * om * d.abs() + U * m1.abs()
    E_m = E_m + (1 - w1) * Em
    T = (1.0 - beta2) * g1 * g1
    v1 = v * beta2 + T                                     # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    E_v = U * (4 * T + 2 * (v * beta2).abs()) + 2 * (1.0 - beta2) * g1.abs() * E_g + beta2 * Ev
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    step_size = lr / bc1
    S = v1.sqrt() / math.sqrt(bc2)
    denom = S + eps
    E_S = S * (torch.where(v1 > 0, E_v / (2 * v1.clamp_min(1e-300)), z) + 3 * U)
    E_den = E_S + U * eps + U * denom
    r = m1 / denom
    E_r = E_m / denom + r.abs() * (E_den / denom + U)
    q = step_size * r
    E_q = step_size * E_r + 2 * U * q.abs()
    p2 = p1 - q
    E_p = E_p1 + E_q + U * (p1.abs() + q.abs())
    return {"p": p2, "m": m1, "v": v1, "p_bound": SLACK * E_p, "m_bound": SLACK * E_m, "v_bound": SLACK * E_v}


# ---- BCE ---------------------------------------------------------------------------------------------------------------------------
def _chain(n):
    return -(-n // BCE_THREADS)


def _loss_bound(mag, term_err, n):
    return SLACK * ((_chain(n) + TREE_DEPTH + 2) * U * mag.sum() + term_err.sum()) / n


def bce(p, t, gs=1.0):
    """nn.BCELoss(mean) on float64 p, t (t a tensor or a number): {"loss", "loss_bound", "dp", "dp_bound"}; dp = gs * d loss / d p with
    torch's clamps (log terms at -100, the denominator at 1e-12f)."""
    n = p.numel()
    t = torch.as_tensor(t, dtype=torch.float64).expand_as(p)
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)
    a, b = -(t * lp), -((1.0 - t) * lq)
    den = ((1.0 - p) * p).clamp_min(BCE_DENOM_CLAMP)
    dp = (gs / n) * (p - t) / den
    dp_bound = SLACK * (8 * U * dp.abs() + ETA * ((1 + (p - t).abs() + dp.abs()) / den + 1))
    return {"loss": (a + b).sum() / n, "loss_bound": _loss_bound(a.abs() + b.abs(), (FN_U + 3) * U * (a.abs() + b.abs()), n),
            "dp": dp, "dp_bound": dp_bound}


def bce_with_logits(x, t, gs=1.0):
    """nn.BCEWithLogitsLoss(mean) on float64 logits against the constant t: {"loss", "loss_bound", "dz", "dz_bound"}."""
    n = x.numel()
    mx = (-x).clamp_min(0.0)
    s = torch.exp(-mx) + torch.exp(-x - mx)
    A, B, C = (1.0 - t) * x, mx, torch.log(s)
    sig = torch.sigmoid(x)
    dz = (gs / n) * (sig - t)
    term = A + B + C
    return {"loss": term.sum() / n,
            "loss_bound": _loss_bound(term.abs(), U * (2 * A.abs() + (A + B).abs() + term.abs() + FN_U * C + FN_U + 1), n),
            "dz": dz, "dz_bound": SLACK * (abs(gs) / n * (2.0 ** -23 + FN_U * U * sig * (1 - sig)) + 5 * U * dz.abs())}


def pair_scales(g0, g1, g2):
    """bce_pair's cotangent rule on numbers or None: (gs of half 0, gs of half 1).  All three missing counts as 1, otherwise a missing
    one counts as 0."""
    if g0 is None and g1 is None and g2 is None:
        return 1.0, 1.0
    z = lambda g: 0.0 if g is None else g          # noqa: E731
    return z(g0) + z(g2), z(g1) + z(g2)


def bce_pair(p, n_half, t0, t1, g0=None, g1=None, g2=None):
    """pcg_bce_pair on float64 p of 2 * n_half elements: {"loss" [3], "loss_bound" [3], "dp", "dp_bound"}.  loss[2]'s bound is for the
    float64 sum; the test compares the device's loss[2] with the fp32 sum of the device's own loss[0] and loss[1] exactly."""
    s0, s1 = pair_scales(g0, g1, g2)
    h0, h1 = bce(p[:n_half], t0, s0), bce(p[n_half:], t1, s1)
    loss = torch.stack([h0["loss"], h1["loss"], h0["loss"] + h1["loss"]])
    lb = torch.stack([h0["loss_bound"], h1["loss_bound"], h0["loss_bound"] + h1["loss_bound"] + U * (h0["loss"].abs() + h1["loss"].abs())])
    return {"loss": loss, "loss_bound": lb, "dp": torch.cat([h0["dp"], h1["dp"]]), "dp_bound": torch.cat([h0["dp_bound"], h1["dp_bound"]])}
