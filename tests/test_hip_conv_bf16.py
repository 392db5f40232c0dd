"""GPU: the bf16-operand mode of the implicit-GEMM convolutions (ops.conv_precision("bf16")), layer by layer.

Semantics under test: the two GEMM operands are rounded once to bf16 (round-to-nearest-even, after an input transform), the
products are summed in fp32, every epilogue is the fp32 one.  So:
  * against a float64 evaluation of the BF16-ROUNDED operands (t.to(torch.bfloat16) on the CPU is RNE) the result is as close as an
    fp32 accumulation is: the bound of test_hip_benchshape.py (16 x u*K*s/sqrt(6) + 1e-6), and
  * against the float64 evaluation of the UNROUNDED operands it is at least 10x further than that bound — a path that quietly ran
    fp32 fails here;
  * fp32 mode is bit-identical before and after bf16 was switched on and off again; the thin edge layers ignore the mode;
  * the fused forms run the same main loop as the plain call, so in bf16 mode they reproduce the plain bf16 result bit for bit
    (the input transform: bit for bit against the transformed tensor the BatchNorm-apply pass writes, one shared definition).
Geometries: every MFMA layer of the DCGAN and CounteRGAN nets (the DCGAN / CounteRGAN rows of test_hip_benchshape.LAYERS) at
test-sized batches.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# name, B, Cin, Cout, H(=W), k, s, p
LAYERS = [
    ("dcgan D2 / G4 adjoint", 8, 64, 128, 32, 4, 2, 1),
    ("dcgan D3 / G3 adjoint", 8, 128, 256, 16, 4, 2, 1),
    ("dcgan D4 / G2 adjoint", 8, 256, 512, 8, 4, 2, 1),
    ("dcgan G1 as 1x1 GEMM", 64, 8192, 100, 1, 1, 1, 0),
    ("countergan resblock 3x3", 4, 64, 64, 28, 3, 1, 1),
    ("countergan D 14->7", 8, 64, 128, 14, 3, 2, 1),
]


def _bound(K, s_term):
    return 16.0 * U * K * s_term / math.sqrt(6.0) + 1e-6


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    from pcgan_amd import ops
    assert pcgan_amd.load().pcg_conv_precision_get() == 0
    yield ops
    pcgan_amd.load().pcg_conv_precision_set(0)


def _inputs(B, Cin, Cout, H, k, s, p, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    OH = (H + 2 * p - k) // s + 1
    x = torch.randn(B, H, H, Cin, generator=g, device=DEV)
    w = torch.randn(Cout, k, k, Cin, generator=g, device=DEV) / math.sqrt(Cin * k * k)
    dy = torch.randn(B, OH, OH, Cout, generator=g, device=DEV)
    return x, w, dy


def _r(t, rounded):
    """NHWC / OHWI device tensor -> NCHW / OIHW float64 on the CPU, optionally through bf16 (RNE) first."""
    t = t.detach().cpu()
    if rounded:
        t = t.to(torch.bfloat16)
    return t.double().permute(0, 3, 1, 2)


def _refs(x, w, dy, s, p, rounded):
    xr, wr, dyr = _r(x, rounded), _r(w, rounded), _r(dy, rounded)
    y = F.conv2d(xr, wr, stride=s, padding=p).permute(0, 2, 3, 1)
    dx = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, stride=s, padding=p).permute(0, 2, 3, 1)
    dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, stride=s, padding=p).permute(0, 2, 3, 1)
    return y, dx, dw


def _run(ops, geom, x, w, dy):
    y = ops.conv2d_fwd(geom, x, w)
    dx = ops.conv2d_dgrad(geom, dy, w)
    dw = torch.empty_like(w)
    ops.conv2d_wgrad(geom, x, dy, dw, False)
    torch.cuda.synchronize()
    return y, dx, dw


@pytest.mark.parametrize("name,B,Cin,Cout,H,k,s,p", LAYERS, ids=[l[0] for l in LAYERS])
def test_layer_bf16_vs_rounded_float64(ops, name, B, Cin, Cout, H, k, s, p):
    x, w, dy = _inputs(B, Cin, Cout, H, k, s, p, seed=11 + len(name))
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    f32_before = _run(ops, geom, x, w, dy)
    with ops.conv_precision("bf16"):
        got = _run(ops, geom, x, w, dy)
    f32_after = _run(ops, geom, x, w, dy)
    for a, b in zip(f32_before, f32_after):
        assert torch.equal(a, b), f"{name}: fp32 results changed after a bf16 section"
    rounded, exact = _refs(x, w, dy, s, p, True), _refs(x, w, dy, s, p, False)
    K = k * k * Cin
    bounds = {"fwd": _bound(K, 1 / math.sqrt(K)), "dgrad": _bound(Cout * ((k + s - 1) // s) ** 2, 1 / math.sqrt(K)),
              "wgrad": _bound(B * geom.OH * geom.OW, 1.0)}
    for what, t, rr, re_, f32 in zip(("fwd", "dgrad", "wgrad"), got, rounded, exact, f32_before):
        t64 = t.cpu().double()
        err = (t64 - rr).abs().max().item()
        far = (t64 - re_).abs().max().item()
        assert err <= bounds[what], f"{name} {what}: max |err| vs bf16-rounded float64 {err:.3e} > bound {bounds[what]:.3e}"
        assert far >= 10 * bounds[what], f"{name} {what}: only {far:.3e} from the unrounded float64 — did it run fp32?"
        assert not torch.equal(t, f32)


def test_thin_layers_ignore_the_mode(ops):
    """DCGAN D1 (Cin = 1) and G5 (its adjoint, Cout = 1 forward): the thin kernels are fp32 in both modes, bit for bit."""
    for B, Cin, Cout, H, k, s, p in ((8, 1, 64, 64, 4, 2, 1), (8, 64, 1, 64, 4, 2, 1)):
        x, w, dy = _inputs(B, Cin, Cout, H, k, s, p, seed=5)
        geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
        a = _run(ops, geom, x, w, dy)
        with ops.conv_precision("bf16"):
            b = _run(ops, geom, x, w, dy)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_nan_operand_stays_nan(ops):
    B, Cin, Cout, H, k, s, p = 4, 64, 128, 16, 4, 2, 1
    x, w, dy = _inputs(B, Cin, Cout, H, k, s, p, seed=9)
    x[1, 7, 9, 13] = float("nan")
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    y32 = ops.conv2d_fwd(geom, x, w)
    with ops.conv_precision("bf16"):
        y16 = ops.conv2d_fwd(geom, x, w)
        dw16 = torch.empty_like(w)
        ops.conv2d_wgrad(geom, x, dy, dw16, False)
    dw32 = torch.empty_like(w)
    ops.conv2d_wgrad(geom, x, dy, dw32, False)
    torch.cuda.synchronize()
    assert int(torch.isnan(y32).sum()) > 0 and torch.equal(torch.isnan(y16), torch.isnan(y32))
    assert not torch.isnan(y16[0]).any() and torch.isnan(y16[1]).any()
    assert int(torch.isnan(dw32).sum()) > 0 and torch.equal(torch.isnan(dw16), torch.isnan(dw32))


def _bn_input(ops, B, H, C, seed, act=2, slope=0.2):
    """A pre-BatchNorm tensor z, its batch statistics / folded coefficients, and the activated tensor the apply pass writes."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(B, H, H, C, generator=g, device=DEV) * 1.7 + 0.3
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.1
    mean, invstd, coef = ops.bn_train_stats(z, C, 1e-5, 0.1, gamma=gamma, beta=beta)
    a = ops.bn_apply_act(z, C, mean, invstd, gamma, beta, act, slope)
    return z, a, mean, invstd, gamma, beta, ops.InputXform(coef, act, slope)


def test_fused_forms_run_bf16(ops):
    """_bn, _bn_g (grouped), _xf / _bn_xf, _bnbwd on DCGAN D3 at its bench batch, where the plain calls take no K-slices either (the
    fused forms cannot; test_hip_benchshape.py::test_fused_forms_at_bench_batch is the fp32 twin); _add_mask / _add_bnsum and the
    grad-input transform on the CounteRGAN 3x3 (stride 1: the plain grad-input is the phase kernel as well)."""
    B, Cin, Cout, H, k, s, p = 512, 128, 256, 16, 4, 2, 1
    x, w, dy = _inputs(B, Cin, Cout, H, k, s, p, seed=21)
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    z_x, a_x, *_, xf_x = _bn_input(ops, B, H, Cin, 31)
    z_dy, a_dy, *_, xf_dy = _bn_input(ops, B, geom.OH, Cout, 32, act=1, slope=0.0)
    z_b, _, mean_b, invstd_b, gamma_b, beta_b, _ = _bn_input(ops, B, H, Cin, 33)
    with ops.conv_precision("bf16"):
        plain_f = ops.conv2d_fwd(geom, x, w)
        plain_d = ops.conv2d_dgrad(geom, dy, w)
        z, _, _ = ops.conv_bn_train(geom, x, w, None, False, 1e-5, 0.1, None, None, None)
        assert torch.equal(z, plain_f)                                               # _bn (Conv2d)
        z, _, _ = ops.conv_bn_train(geom, dy, w, None, True, 1e-5, 0.1, None, None, None)
        assert torch.equal(z, plain_d)                                               # _bn (ConvTranspose2d: grad-input kernel)
        z, _, _ = ops.conv_bn_train_g(geom, x, w, None, 1e-5, 0.1, None, None, None, 2)
        assert torch.equal(z, plain_f)                                               # _bn_g
        assert torch.equal(ops.conv2d_fwd(geom, z_x, w, xf=xf_x), ops.conv2d_fwd(geom, a_x, w))          # _xf
        z, _, _ = ops.conv_bn_train(geom, z_x, w, None, False, 1e-5, 0.1, None, None, None, xf=xf_x)
        assert torch.equal(z, ops.conv2d_fwd(geom, a_x, w))                          # _bn_xf
        dw_xf, dw_a = torch.empty_like(w), torch.empty_like(w)
        ops.conv2d_wgrad(geom, z_x, dy, dw_xf, False, xf_x=xf_x)
        ops.conv2d_wgrad(geom, a_x, dy, dw_a, False)
        assert torch.equal(dw_xf, dw_a)                                              # wgrad, x transformed
        ops.conv2d_wgrad(geom, x, z_dy, dw_xf, False, xf_dy=xf_dy)
        ops.conv2d_wgrad(geom, x, a_dy, dw_a, False)
        assert torch.equal(dw_xf, dw_a)                                              # wgrad, dy transformed
        dm, _, _ = ops.conv_bwd_data_fused(geom, dy, w, False, 2, 0.2, z_below=z_b, bn=(mean_b, invstd_b, gamma_b, beta_b))
    pre = z_b * (gamma_b * invstd_b) + (beta_b - mean_b * gamma_b * invstd_b)
    want = torch.where(pre > 0, plain_d, plain_d * 0.2)
    flips = dm != want                                                               # _bnbwd: its mask is one fma, see benchshape
    assert int(flips.sum()) <= 1e-5 * dm.numel() and bool(((pre.abs() < 1e-5) | ~flips).all())
    assert not torch.equal(plain_f, ops.conv2d_fwd(geom, x, w))                     # (and all of the above was not fp32)

    B, C, H = 4, 64, 28
    x, w, dy = _inputs(B, C, C, H, 3, 1, 1, seed=41)
    geom = ops.conv_geom(B, H, H, C, C, 3, 3, 1, 1)
    g = torch.Generator(device=DEV).manual_seed(42)
    addend = torch.randn(B, H, H, C, generator=g, device=DEV)
    a_below = torch.randn(B, H, H, C, generator=g, device=DEV)
    z_next, _, mean_n, invstd_n, *_ = _bn_input(ops, B, H, C, 43)
    with ops.conv_precision("bf16"):
        plain_d = ops.conv2d_dgrad(geom, dy, w)
        plain_f = ops.conv2d_fwd(geom, dy, w)
        got = ops.conv2d_dgrad_add_mask(geom, dy, w, addend, a_below, 2, 0.2)
        assert torch.equal(got, torch.where(a_below > 0, plain_d + addend, (plain_d + addend) * 0.2))   # _add_mask
        got = ops.conv2d_dgrad_add_mask(geom, dy, w, addend, a_below, 2, 0.2, transposed=True)
        assert torch.equal(got, torch.where(a_below > 0, plain_f + addend, (plain_f + addend) * 0.2))   # fwd _add_mask
        got, _, _ = ops.conv2d_dgrad_add(geom, dy, w, addend, bnsum=(z_next, mean_n, invstd_n, 0.1))
        assert torch.equal(got, plain_d + addend)                                                      # _add_bnsum
        got, _, _ = ops.conv2d_dgrad_add(geom, dy, w, addend, bnsum=(z_next, mean_n, invstd_n, 0.1), transposed=True)
        assert torch.equal(got, plain_f + addend)                                                      # fwd _add_bnsum
        z_dy, a_dy, *_, xf_dy = _bn_input(ops, B, H, C, 44)
        assert torch.equal(ops.conv2d_dgrad(geom, z_dy, w, xf=xf_dy), ops.conv2d_dgrad(geom, a_dy, w))   # dgrad _xf
    assert not torch.equal(plain_d, ops.conv2d_dgrad(geom, dy, w))
