"""GPU parity of the thin-channel convolutions (csrc/thin_conv.hip, thin_rows.inc, thin_fast.inc) against float64, branch by branch.

launch_expand / launch_reduce / thin_conv_wgrad choose among ~30 kernel instantiations by the thin channel count Cs, the wide channel
count C, the kernel shape, the stride, the tap map (direct / transposed), whether the row-block plan fits (rows_plan) and the
PCG_EXPAND_MFMA switch.  Every case below is picked from those predicates to reach one branch (its id names it; the suffix -C<n> is the
wide channel count), and between the shapes of a branch there are B = 1, odd B, non-square images, padding 0 and 1 and a last row-block
unit shorter than the others.  Inputs are randn everywhere (borders included) and rounded to float32 before the float64 reference
sees them, biases are nonzero: a padding, tap-flip or tail error shows up as an O(1) difference.

Tolerance: the bound of test_hip_ops.py, |err| <= 2e-6 * sqrt(K) * scale + 1e-6, K the true length of the dot product (taps x Cin for
the forward, taps x Cout for the grad-input, B*OH*OW for the weight gradient), scale 4 for the forward / grad-input and 8 for the weight
gradient.
"""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd


def dev():
    return torch.device("cuda:0")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _tol(K, scale):
    return 2e-6 * math.sqrt(K) * scale + 1e-6


def _k2(k):
    return k if isinstance(k, tuple) else (k, k)


def _wide(shape):
    return shape[2] if shape[1] <= 3 else shape[1]


def _params(cases):
    return [pytest.param(s, id=f"{name}-C{_wide(s)}") for name, s in cases]


def _act64(v, act, slope):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def _randn(*shape, g, scale=1.0):
    """float64 values that are exactly representable in float32 (the kernels' inputs are then the reference's inputs)."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def _ref(shape, seed):
    """float64 forward + autograd backward of F.conv2d on the CPU: x, w, b, bias_x, y, dy (x.grad / w.grad filled)."""
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = _k2(k)
    g = torch.Generator().manual_seed(seed)
    x = _randn(B, Cin, H, W, g=g).requires_grad_(True)
    w = _randn(Cout, Cin, kh, kw, g=g, scale=1.0 / math.sqrt(Cin * kh * kw)).requires_grad_(True)
    b = _randn(Cout, g=g)
    bx = _randn(Cin, g=g)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    dy = _randn(*y.shape, g=g)
    y.backward(dy)
    return x, w, b, bx, y, dy


def _geom(ops, shape):
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = _k2(k)
    return ops.conv_geom(B, H, W, Cin, Cout, kh, kw, s, p)


def _on_dev(t):
    return t.detach().float().contiguous().to(dev())


def _err(got, want):
    return (got.cpu().double() - want).abs().max().item()


# (B, Cin, Cout, H, W, k, s, p); k may be (KH, KW).  Row-block plan (expand): R = ceil(max(16 * 256 / C, 256) / OW) rows per unit,
# patch ((R-1)*s + KH) x ((OW-1)*s + KW) x Cs <= 2048 floats, >= 64 iteration pixels.  Comments: the other two ops' branches.
CASES = [
    # -- forward, Cin-thin, row-block expand on the matrix cores (C = 64)
    ("fwd-rows-mfma-k44-cs1-tail", (3, 1, 64, 46, 46, 4, 2, 1)),       # OH 23: R 12, last unit 11 rows; dgrad col2im (W 46)
    ("fwd-rows-mfma-k44-cs1-b1", (1, 1, 64, 20, 35, 4, 2, 0)),
    ("fwd-rows-mfma-k33-cs1-tail", (2, 1, 64, 27, 19, 3, 1, 0)),       # OH 25: R 16, last unit 9 rows
    ("fwd-rows-mfma-k33-cs1-s2", (1, 1, 64, 30, 33, 3, 2, 1)),
    ("fwd-rows-mfma-k33-cs2-s2", (1, 2, 64, 29, 17, 3, 2, 0)),         # dgrad tapdot64 mfma <2> + col2im32
    ("fwd-rows-mfma-k33-cs2-s1", (3, 2, 64, 13, 21, 3, 1, 1)),
    ("fwd-rows-mfma-k33-cs3-tail", (5, 3, 64, 28, 28, 3, 1, 1)),       # R 10: units of 10, 10, 8 rows
    ("fwd-rows-mfma-k33-cs3-s2", (1, 3, 64, 25, 14, 3, 2, 0)),
    ("fwd-rows-mfma-units1152", (384, 1, 64, 28, 28, 3, 1, 1)),        # 1152 units > 1024 blocks (grid-stride); wgrad 2688 units, 6 per slab
    # -- forward, Cin-thin, row-block expand on the vector ALU (C != 64)
    ("fwd-rows-k44-cs1", (3, 1, 16, 30, 30, 4, 2, 1)),
    ("fwd-rows-k44-cs1-b1", (1, 1, 128, 20, 35, 4, 2, 0)),
    ("fwd-rows-k33-cs1-tail", (2, 1, 256, 27, 19, 3, 1, 0)),
    ("fwd-rows-k33-cs1-s2", (1, 1, 16, 30, 33, 3, 2, 1)),
    ("fwd-rows-k33-cs2-s2", (1, 2, 128, 29, 17, 3, 2, 0)),             # dgrad tapdot32<18> + col2im32
    ("fwd-rows-k33-cs2-s1", (3, 2, 16, 13, 21, 3, 1, 1)),
    ("fwd-rows-k33-cs3-tail", (5, 3, 128, 28, 28, 3, 1, 1)),           # dgrad tapdot32<27> + col2im32
    ("fwd-rows-k33-cs3-s2", (1, 3, 16, 25, 14, 3, 2, 0)),
    # -- forward, Cin-thin, 16 channels per thread (rows_plan refuses)
    ("fwd-expand16-k33-c48", (3, 1, 48, 17, 23, 3, 1, 1)),             # C not a power of two; wgrad: the fallback
    ("fwd-expand16-k44-c48", (1, 1, 48, 30, 30, 4, 2, 1)),
    ("fwd-expand16-k44-oh63", (3, 1, 64, 14, 18, 4, 2, 1)),            # 7 x 9 = 63 output pixels
    ("fwd-expand16-k33-oh63", (1, 1, 128, 9, 11, 3, 1, 0)),
    ("fwd-expand16-k11", (3, 1, 64, 9, 13, 1, 1, 0)),                  # wgrad thin_wgrad_kernel<1,1,1>
    ("fwd-expand16-k11-s2", (1, 1, 32, 15, 16, 1, 2, 1)),              # dgrad tapdot<1>
    ("fwd-expand16-k44-patch2056", (1, 1, 64, 8, 512, 4, 2, 1)),       # patch 10 x 514 floats > 2048; dgrad col2im_s2k4
    ("fwd-expand16-k33-patch", (1, 1, 64, 5, 1000, 3, 1, 1)),
    # -- forward, Cin-thin, the generic expand
    ("fwd-expand-cs2-c48", (3, 2, 48, 11, 13, 3, 1, 1)),
    ("fwd-expand-c20", (1, 1, 20, 12, 9, 3, 1, 1)),                    # dgrad generic reduce
    ("fwd-expand-k5p2", (3, 1, 64, 14, 11, 5, 1, 2)),
    ("fwd-expand-k2s2", (1, 1, 64, 16, 13, 2, 2, 0)),
    ("fwd-expand-k3x1", (3, 3, 32, 10, 12, (3, 1), 1, 0)),
    ("fwd-expand-s3", (1, 1, 64, 22, 17, 3, 3, 1)),
    ("fwd-expand-k44-cs2", (3, 2, 64, 18, 14, 4, 2, 1)),
    # -- forward, Cout-thin: tap-dot on the matrix cores (2..3 thin channels) + col2im32; grad-input row-block / generic expand
    ("fwd-tapdot64-mfma2-cs2-s1", (3, 64, 2, 15, 17, 3, 1, 1)),
    ("fwd-tapdot64-mfma2-cs3-s2", (1, 64, 3, 21, 14, 3, 2, 0)),
    # -- forward, Cout-thin: vector tap-dot over 18 / 27 outputs + col2im32
    ("fwd-tapdot32-18-s1", (2, 32, 2, 13, 11, 3, 1, 1)),
    ("fwd-tapdot32-18-s2", (3, 128, 2, 9, 10, 3, 2, 0)),
    ("fwd-tapdot32-27-s2", (1, 128, 3, 12, 17, 3, 2, 1)),
    ("fwd-tapdot32-27-s1", (1, 32, 3, 16, 15, 3, 1, 0)),
    # -- forward, Cout-thin, one channel: tap-dot on the matrix cores (C = 64 / multiples of 64 up to 512) + col2im
    ("fwd-tapdot64-mfma1-k33", (2, 64, 1, 17, 13, 3, 1, 1)),
    ("fwd-tapdot64-mfma1-k44", (1, 64, 1, 20, 22, 4, 2, 1)),
    ("fwd-tapdot64-mfma1multi-k33", (3, 128, 1, 11, 9, 3, 1, 0)),
    ("fwd-tapdot64-mfma1multi-k44", (1, 512, 1, 10, 12, 4, 2, 1)),
    # -- forward, Cout-thin, one channel: vector tap-dot over 16 / 9 / 1 taps + col2im
    ("fwd-tapdot16-s2", (2, 16, 1, 12, 13, 4, 2, 1)),
    ("fwd-tapdot16-s1", (1, 48, 1, 14, 16, 4, 1, 2)),
    ("fwd-tapdot9-s1", (1, 48, 1, 11, 10, 3, 1, 1)),
    ("fwd-tapdot9-s2", (3, 1024, 1, 6, 5, 3, 2, 1)),
    ("fwd-tapdot1-b3", (3, 1024, 1, 5, 6, 1, 1, 0)),
    ("fwd-tapdot1-b1", (1, 16, 1, 9, 7, 1, 1, 0)),
    # -- forward, Cout-thin, the generic reduce
    ("fwd-reduce-c20", (1, 20, 1, 9, 11, 3, 1, 1)),
    ("fwd-reduce-s3", (2, 64, 1, 16, 14, 3, 3, 1)),                    # wgrad: transposed map at stride 3 (the fallback)
    ("fwd-reduce-k5", (1, 64, 1, 12, 13, 5, 1, 2)),
    ("fwd-reduce-k44-cs2", (3, 64, 2, 12, 10, 4, 2, 1)),
    # -- grad-input, Cin-thin: the sub-pixel col2im (k4 s2, input width % 4 == 0) and the plain one
    ("dgrad-col2im-s2k4", (2, 1, 64, 28, 20, 4, 2, 1)),
    ("dgrad-col2im-s2k4-multi", (1, 1, 128, 16, 12, 4, 2, 1)),
    ("dgrad-col2im-k4s2-w30", (1, 1, 64, 30, 30, 4, 2, 1)),
    # -- grad-input, Cout-thin: row-block expand on the transposed map (stride 1), matrix cores / vector
    ("dgrad-rows-mfma-k33-cs1-tail", (3, 64, 1, 15, 22, 3, 1, 1)),
    ("dgrad-rows-mfma-k44-cs1", (1, 64, 1, 17, 13, 4, 1, 1)),
    ("dgrad-rows-mfma-k33-cs3-tail", (1, 64, 3, 18, 21, 3, 1, 1)),
    ("dgrad-rows-k33-cs2", (1, 128, 2, 14, 11, 3, 1, 1)),
    ("dgrad-rows-k33-cs3", (3, 128, 3, 9, 12, 3, 1, 0)),
    # -- grad-input, Cout-thin at stride 2: expand16 (one channel) / generic expand
    ("dgrad-expand16-s2-k33", (2, 64, 1, 15, 18, 3, 2, 1)),
    ("dgrad-expand16-s2-k44", (1, 128, 1, 16, 14, 4, 2, 1)),
    ("dgrad-expand-s2-cs3", (1, 64, 3, 13, 16, 3, 2, 1)),
    ("dgrad-expand-s2-cs2", (3, 128, 2, 12, 11, 3, 2, 0)),
    # -- weight gradient, thin_wgrad_kernel (no row-block plan)
    ("wgrad-thin-cout-s2-k44", (3, 64, 1, 12, 14, 4, 2, 1)),
    ("wgrad-thin-cout-s2-k33-cs2", (1, 128, 2, 15, 14, 3, 2, 1)),
    ("wgrad-thin-k11-cs3", (3, 3, 64, 9, 10, 1, 1, 0)),
    ("wgrad-thin-k11-cout2", (1, 64, 2, 11, 7, 1, 1, 0)),
    ("wgrad-thin-ow300", (1, 1, 64, 6, 300, 3, 1, 1)),                  # OW > 128 at C = 64: no row-block wgrad plan
    ("wgrad-thin-ow200-k44", (2, 1, 64, 8, 402, 4, 2, 1)),
    # -- weight gradient, the fallback for geometries without an instantiation (forward and grad-input accept them)
    ("wgrad-any-c48-k33", (2, 1, 48, 12, 10, 3, 1, 1)),                # Conv2d(1, 48, 3, padding=1)
    ("wgrad-any-k55", (2, 1, 64, 12, 10, 5, 1, 2)),                     # Conv2d(1, 64, 5, padding=2)
    ("wgrad-any-k22-cout", (3, 64, 1, 9, 12, 2, 1, 0)),
    ("wgrad-any-k3x1-cout3", (1, 32, 3, 11, 8, (3, 1), 1, 1)),
    ("wgrad-any-c1040", (1, 1040, 1, 6, 5, 3, 1, 1)),                   # C % 4 == 0, above 1024
]


@pytest.mark.parametrize("shape", _params(CASES))
def test_thin_conv_against_float64(pcg, shape):
    ops = pcg.ops
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = _k2(k)
    x, w, b, bx, y, dy = _ref(shape, seed=B * 1009 + Cin * 31 + Cout * 7 + H)
    g = _geom(ops, shape)
    assert (g.OH, g.OW) == tuple(y.shape[2:])
    xd, wd, bd, bxd, dyd = _on_dev(nhwc(x)), _on_dev(nhwc(w)), _on_dev(b), _on_dev(bx), _on_dev(nhwc(dy))

    err = _err(ops.conv2d_fwd(g, xd, wd, bd), nhwc(y.detach()))
    assert err <= _tol(Cin * kh * kw, 4.0), f"fwd max err {err}"

    err = _err(ops.conv2d_dgrad(g, dyd, wd, bxd), nhwc(x.grad) + bx)
    assert err <= _tol(Cout * kh * kw, 4.0), f"dgrad max err {err}"

    ref, K = nhwc(w.grad), B * g.OH * g.OW
    assert pcg.load().pcg_conv2d_wgrad_workspace_bytes(ctypes.byref(g)) >= Cout * kh * kw * Cin * 4     # at least one slab
    dwd = torch.full((Cout, kh, kw, Cin), 0.5, dtype=torch.float32, device=dev())
    ops.conv2d_wgrad(g, xd, dyd, dwd, accumulate=False)           # overwrites the 0.5 fill
    err = _err(dwd, ref)
    assert err <= _tol(K, 8.0), f"wgrad max err {err}"
    ops.conv2d_wgrad(g, xd, dyd, dwd, accumulate=True)
    err = _err(dwd, 2 * ref)
    assert err <= 2 * _tol(K, 8.0), f"wgrad accumulate max err {err}"


ACTS = [pytest.param(ACT_RELU, 0.0, id="relu"), pytest.param(ACT_LRELU, 0.2, id="lrelu"), pytest.param(ACT_TANH, 0.0, id="tanh"),
        pytest.param(ACT_SIGMOID, 0.0, id="sigmoid")]

ACT_CASES = [     # one shape per family; the forward and the grad-input both take the activation
    ("act-rows-mfma-cs3", (3, 3, 64, 13, 11, 3, 1, 1)),
    ("act-rows-cs1", (1, 1, 128, 20, 35, 4, 2, 0)),
    ("act-expand16", (3, 1, 48, 17, 23, 3, 1, 1)),
    ("act-expand", (1, 1, 20, 12, 9, 3, 1, 1)),
    ("act-tapdot64-mfma2", (3, 64, 2, 15, 17, 3, 1, 1)),
    ("act-tapdot32", (1, 128, 3, 12, 17, 3, 2, 1)),
    ("act-tapdot64-mfma1", (1, 64, 1, 20, 22, 4, 2, 1)),
    ("act-tapdot9", (1, 48, 1, 11, 10, 3, 1, 1)),
    ("act-reduce", (2, 64, 1, 16, 14, 3, 3, 1)),
]


@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("shape", _params(ACT_CASES))
def test_thin_conv_activation_against_float64(pcg, shape, act, slope):
    """ReLU / LeakyReLU are fused into the wide-output writes, Tanh / Sigmoid run as a second pass there; the thin-output kernels apply
    all four in their write."""
    ops = pcg.ops
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = _k2(k)
    x, w, b, bx, y, dy = _ref(shape, seed=B * 17 + Cin + act)
    g = _geom(ops, shape)
    xd, wd, bd, bxd, dyd = _on_dev(nhwc(x)), _on_dev(nhwc(w)), _on_dev(b), _on_dev(bx), _on_dev(nhwc(dy))
    err = _err(ops.conv2d_fwd(g, xd, wd, bd, act=act, slope=slope), _act64(nhwc(y.detach()), act, slope))
    assert err <= _tol(Cin * kh * kw, 4.0), f"fwd max err {err}"
    err = _err(ops.conv2d_dgrad(g, dyd, wd, bxd, act=act, slope=slope), _act64(nhwc(x.grad) + bx, act, slope))
    assert err <= _tol(Cout * kh * kw, 4.0), f"dgrad max err {err}"


MASK_CASES = [    # Cout-thin grad-input times act'(a_below) in the row-block expand (transposed map, stride 1)
    ("mask-rows-mfma-k33-cs1-tail", (2, 64, 1, 15, 22, 3, 1, 1)),
    ("mask-rows-mfma-k33-cs2", (1, 64, 2, 13, 19, 3, 1, 0)),
    ("mask-rows-mfma-k33-cs3", (3, 64, 3, 12, 9, 3, 1, 1)),
    ("mask-rows-mfma-k44-cs1", (1, 64, 1, 17, 13, 4, 1, 1)),
    ("mask-rows-k33-cs1", (1, 128, 1, 14, 21, 3, 1, 1)),
    ("mask-rows-k33-cs2", (3, 128, 2, 11, 12, 3, 1, 1)),
    ("mask-rows-k33-cs3", (1, 128, 3, 16, 9, 3, 1, 0)),
    ("mask-rows-k44-cs1", (2, 128, 1, 12, 15, 4, 1, 2)),
]


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("shape", _params(MASK_CASES))
def test_thin_grad_input_with_mask_against_float64(pcg, shape, act, slope):
    ops, lib = pcg.ops, pcg.load()
    B, Cin, Cout, H, W, k, s, p = shape
    x, w, b, bx, y, dy = _ref(shape, seed=B * 13 + Cout + act)
    g = _geom(ops, shape)
    assert lib.pcg_conv2d_dgrad_mask_thin_ok(ctypes.byref(g)) == 1
    gen = torch.Generator().manual_seed(5)
    a_below = torch.randn(B, H, W, Cin, generator=gen)
    res = ops.conv_bwd_data_fused(g, _on_dev(nhwc(dy)), _on_dev(nhwc(w)), False, act, slope, a_below=a_below.to(dev()))
    assert res is not None
    want = nhwc(x.grad) * torch.where(a_below.double() > 0, 1.0, slope)
    err = _err(res[0], want)
    assert err <= _tol(Cout * k * k, 4.0), f"masked dgrad max err {err}"


BNBWD_CASES = [   # pcg_conv2d_fwd_bnbwd_thin: the sums pass on the matrix cores (C = 64) or the vector ALU
    ("bnbwd-sums-mfma-b3", (3, 1, 64, 22, 30, 4, 2, 1)),
    ("bnbwd-sums-mfma-b1", (1, 1, 64, 16, 40, 4, 2, 1)),
    ("bnbwd-sums-b5", (5, 1, 128, 18, 26, 4, 2, 1)),
    ("bnbwd-sums-b3", (3, 1, 128, 20, 16, 4, 2, 1)),
]


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("shape", _params(BNBWD_CASES))
def test_thin_forward_through_batchnorm_backward_against_float64(pcg, shape, act, slope):
    """d = conv(x, w) taken as the gradient w.r.t. act(BatchNorm_train(z)), pushed through that backward: dz, dgamma, dbeta in float64."""
    ops = pcg.ops
    B, Cin, C, H, W, k, s, p = shape
    g = _geom(ops, shape)
    assert ops.thin_fwd_bn_bwd_ok(g)
    gen = torch.Generator().manual_seed(B * 3 + C)
    x = _randn(B, H, W, 1, g=gen)
    w = _randn(C, k, k, 1, g=gen, scale=0.25)
    z = _randn(B, g.OH, g.OW, C, g=gen, scale=1.3) + 0.25
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = _randn(C, g=gen, scale=0.1)
    zr = z.reshape(-1, C)
    mean = zr.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(zr.var(0, unbiased=False) + 1e-5)).float().double()
    # float64 chain
    d = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1).reshape(-1, C)
    sc = gamma * invstd
    pre = zr * sc + (beta - mean * sc)
    neg = slope if act == ACT_LRELU else 0.0
    dm = d * torch.where(pre > 0, 1.0, neg)
    xh = (zr - mean) * invstd
    n = zr.shape[0]
    db_ref, dg_ref = dm.sum(0), (dm * xh).sum(0)
    dz_ref = sc * (dm - db_ref / n - xh * dg_ref / n)
    # elements whose pre-activation sits at the float32 rounding of 0 may take either side of the mask
    amb = pre.abs() < 1e-5
    slack_b = (d.abs() * amb).sum(0) * (1 - neg)
    slack_g = (d.abs() * xh.abs() * amb).sum(0) * (1 - neg)
    e_d = _tol(k * k, 4.0)                                  # bound on one element of d (16 taps)
    tol_b = e_d * n ** 0.5 + _tol(n, 8.0) * float(dm.abs().max()) + slack_b
    tol_g = e_d * float(xh.abs().max()) * n ** 0.5 + _tol(n, 8.0) * float((dm * xh).abs().max()) + slack_g
    tol_z = sc * (e_d * (2 + xh.abs().max()) + (slack_b + xh.abs().max() * slack_g) / n)

    for accumulate in (False, True):
        dg0, db0 = _randn(C, g=gen), _randn(C, g=gen)
        dgd, dbd = _on_dev(dg0), _on_dev(db0)
        dz = ops.thin_fwd_bn_bwd(g, _on_dev(x), _on_dev(w), _on_dev(z), _on_dev(mean), _on_dev(invstd), _on_dev(gamma), _on_dev(beta),
                                 act, slope, dgd, dbd, accumulate)
        base_g, base_b = (dg0, db0) if accumulate else (torch.zeros(C, dtype=torch.float64),) * 2
        diff_b = (dbd.cpu().double() - (base_b + db_ref)).abs()
        diff_g = (dgd.cpu().double() - (base_g + dg_ref)).abs()
        assert bool((diff_b <= tol_b + 1e-6).all()), f"dbeta max err {float(diff_b.max())} (accumulate={accumulate})"
        assert bool((diff_g <= tol_g + 1e-6).all()), f"dgamma max err {float(diff_g.max())} (accumulate={accumulate})"
        diff_z = (dz.cpu().double().reshape(-1, C) - dz_ref).abs()
        bad = ~amb & (diff_z > tol_z + 1e-6)
        assert not bool(bad.any()), f"dz max err {float((diff_z * ~amb).max())} (accumulate={accumulate})"


def test_vector_forms_at_64_channels_in_a_child_process():
    """The non-matrix-core forms at C = 64 are what a caller with tensors that are not 16-byte aligned runs.  A fresh process with
    PCG_EXPAND_MFMA=0 (read once, at the first launch) runs every C = 64 case of this file against float64 on those forms."""
    env = dict(os.environ, PCG_EXPAND_MFMA="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "C64 and not child_process"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out after {e.timeout} s\n{e.stdout or ''}\n{e.stderr or ''}")
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"child exit {r.returncode}\n{out[-8000:]}"
    assert " passed" in r.stdout and "skipped" not in r.stdout, out[-4000:]
