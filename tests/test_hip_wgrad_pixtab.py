"""GPU: the weight gradient reading its pixels from the geometry's descriptor table (pcg_conv_pixtab_register, conv_loaders.h PixDesc8)
against the loaders that derive them per k-tile — bit for bit, pcg_tune_set("wgrad_pixtab", 0 | 1) in one process — and against a
float64 weight gradient on the CPU at the tolerance of tests/test_hip_benchshape.py (_bound: 16 standard deviations of a K-term
fp32 fma chain).  Shapes: the smallest at which the table loader can go wrong (see CASES)."""
import ctypes

import pytest
import torch

from test_hip_benchshape import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name, B, Cin, Cout, H(=W), k, s, p
CASES = [
    # K = 48 pixels: the second k-tile spans images 1 and 2 and ends in a 16-pixel tail; M = 32 is a partial tile; every border tap
    ("k4s2p1 8->4 B3 32->32", 3, 32, 32, 8, 4, 2, 1),
    # OH*OW = 49: no power of two, a wave's 8 pixels cross images at odd places (the table's tail entries); N = 576: the 64x192 tile
    ("k3s1p1 7x7 B2 64->64 (64x192)", 2, 64, 64, 7, 3, 1, 1),
    # Cin = 16 < 32: eight taps inside one 128-column tile; N = 144 leaves a column tail
    ("k3s2p1 7->4 B2 16->32", 2, 16, 32, 7, 3, 2, 1),
    # K = 2048: several K-slices, kt_begin != 0
    ("k4s2p1 32->16 B8 32->64", 8, 32, 64, 32, 4, 2, 1),
    # OH*OW = 1: every pixel is its own image (the tail entries carry up to 7 image strides)
    ("k4s1p0 4->1 B40 32->32", 40, 32, 32, 4, 4, 1, 0),
]
# M > 64 and 128 tiles of 128x128: the stream-K kernel (stream_k = 2 cuts the 8 k-tiles of every tile into two ranges)
SK_CASE = ("k4s2p1 8->4 B16 512->256 (stream-K)", 16, 512, 256, 8, 4, 2, 1)


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import dcgan  # noqa: F401
    return pcgan_amd


def _inputs(B, Cin, Cout, H, k, s, p, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    OH = (H + 2 * p - k) // s + 1
    x = torch.randn(B, H, H, Cin, generator=g, device=DEV)
    dy = torch.randn(B, OH, OH, Cout, generator=g, device=DEV)
    g0 = torch.randn(Cout, k, k, Cin, generator=g, device=DEV)
    return x, dy, g0, OH


def _ref64(x, dy, k, s, p):
    """float64 weight gradient on the CPU, OHWI."""
    x64 = x.cpu().double().permute(0, 3, 1, 2)
    dy64 = dy.cpu().double().permute(0, 3, 1, 2)
    w = torch.zeros(dy64.shape[1], x64.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x64, w, None, s, p).backward(dy64)
    return w.grad.permute(0, 2, 3, 1).contiguous()


def _both(ops, fn):
    """fn() with the switch at 0 and at 1 -> (result of 0, result of 1)."""
    out = []
    try:
        for v in (0, 1):
            ops.tune("wgrad_pixtab", v)
            out.append(fn())
        torch.cuda.synchronize()
    finally:
        ops.tune("wgrad_pixtab", -1)
    return out


def _registered(ops, geom):
    return ops._pixtabs.get(ops._pixtab_key(geom, torch.device(DEV).index)) is not None


@pytest.mark.parametrize("name,B,Cin,Cout,H,k,s,p", CASES, ids=[c[0] for c in CASES])
def test_table_loader_is_bit_identical_and_right(pcg, name, B, Cin, Cout, H, k, s, p):
    ops = pcg.ops
    x, dy, g0, OH = _inputs(B, Cin, Cout, H, k, s, p, seed=len(name))
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    ref = _ref64(x, dy, k, s, p)
    K = B * OH * OH

    a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
    assert _registered(ops, geom)
    assert torch.equal(a, b), f"{name}: table loader differs from the per-k-tile loader"
    err = (b.cpu().double() - ref).abs().max().item()
    print(f"{name}: max |err| vs float64 {err:.3e} (bound {_bound(K, 1.0):.3e})")
    assert err <= _bound(K, 1.0)
    assert ref.abs().max().item() > 1.0

    # accumulate into a non-zero .grad: one more O(1) term in every sum
    a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, g0.clone(), True))
    assert torch.equal(a, b), f"{name}: accumulate"
    err = (b.cpu().double() - (ref + g0.cpu().double())).abs().max().item()
    assert err <= _bound(K + 1, 1.0), f"{name} accumulate: {err:.3e}"

    # two groups: the halves of the batch as separate launches accumulating into one gradient (nn.SequentialConvNet's paired pass);
    # the second launch's geometry has another B but the same table
    if B % 2 == 0:
        h = B // 2
        gh = ops.conv_geom(h, H, H, Cin, Cout, k, k, s, p)

        def halves():
            dw = torch.empty_like(g0)
            ops.conv2d_wgrad(gh, x[:h], dy[:h], dw, False)
            return ops.conv2d_wgrad(gh, x[h:], dy[h:], dw, True)
        a, b = _both(ops, halves)
        assert torch.equal(a, b), f"{name}: two groups"
        err = (b.cpu().double() - ref).abs().max().item()
        assert err <= _bound(K + 1, 1.0), f"{name} two groups: {err:.3e}"


def test_stream_k_and_bf16_forms(pcg):
    ops = pcg.ops
    name, B, Cin, Cout, H, k, s, p = SK_CASE
    x, dy, g0, OH = _inputs(B, Cin, Cout, H, k, s, p, seed=5)
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    ref = _ref64(x, dy, k, s, p)
    K = B * OH * OH
    lib = pcg.load()
    desc = ctypes.create_string_buffer(256)
    try:
        ops.tune("stream_k", 2)
        # the launch is stream-K only if this stream has its scratch: register it as every conv call does, then ask for the plan of
        # the stream as it IS (assume_scratch = 0)
        ops._conv_scratch()
        st = torch.cuda.current_stream()
        assert ops._sk_streams.get((st.device_index, st.cuda_stream)) is not None
        assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
        assert desc.value.decode().startswith("stream-K"), desc.value
        a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
        assert torch.equal(a, b), "stream-K"
        err = (b.cpu().double() - ref).abs().max().item()
        assert err <= _bound(K, 1.0), f"stream-K: {err:.3e}"
        a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, g0.clone(), True))
        assert torch.equal(a, b), "stream-K accumulate"
    finally:
        ops.tune("stream_k", -1)
    # the bf16-operand twin and the transformed-x variant share the loader: bit-identical under the switch as well
    with ops.conv_precision("bf16"):
        a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
    assert torch.equal(a, b), "bf16 twin"
    xf = ops.InputXform(torch.cat([torch.rand(Cin, device=DEV) + 0.5, torch.randn(Cin, device=DEV) * 0.1]).contiguous(), ops.ACT_LRELU, 0.2)
    a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False, xf_x=xf))
    assert torch.equal(a, b), "input transform on x"
    assert _registered(ops, geom)


def test_geometry_without_a_table_runs_the_old_loader(pcg):
    ops = pcg.ops
    name, B, Cin, Cout, H, k, s, p = CASES[0]
    H = 10                                   # a geometry no other test registers: 10 -> 5
    x, dy, g0, OH = _inputs(B, Cin, Cout, H, k, s, p, seed=11)
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    key = ops._pixtab_key(geom, torch.device(DEV).index)
    ops.drop_conv_pixtab(geom, torch.device(DEV))
    try:
        a, b = _both(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
        assert not _registered(ops, geom)
        assert torch.equal(a, b)
        err = (b.cpu().double() - _ref64(x, dy, k, s, p)).abs().max().item()
        assert err <= _bound(B * OH * OH, 1.0)
    finally:
        ops._pixtabs.pop(key, None)
    c = ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False)          # now with its table
    torch.cuda.synchronize()
    assert _registered(ops, geom) and torch.equal(a, c)


def test_captured_backward_replays_bit_equal_to_eager(pcg):
    """A DCGAN step (three MFMA weight gradients per backward sweep) captured with the tables registered by its warm-up steps."""
    from pcgan_amd.nn import GraphedStep
    D, ops = pcg.dcgan, pcg.ops
    cfg = {"g_hidden": 32, "d_hidden": 32, "z_dim": 32}
    B = 8
    g = torch.Generator().manual_seed(5)
    reals = [(torch.rand(B, 1, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    noises = [torch.randn(B, 32, 1, 1, generator=g).to(DEV) for _ in range(2)]

    def fresh():
        torch.manual_seed(0)
        netG, netD = D.Generator(cfg).to(DEV), D.Discriminator(cfg).to(DEV)
        netG.apply(D.weights_init); netD.apply(D.weights_init)
        return (netG, netD) + tuple(D.make_optimizers(netG, netD, cfg))

    netG, netD, crit, optD, optG = fresh()
    for i in range(2):
        D.train_step(netG, netD, crit, optD, optG, reals[i], noises[i], cfg)
    want = (netG.flat_params.clone(), netD.flat_params.clone())
    assert _registered(ops, ops.conv_geom(B, 16, 16, 64, 128, 4, 4, 2, 1))          # D3 of this width
    netG, netD, crit, optD, optG = fresh()
    s_real, s_noise = reals[0].clone(), noises[0].clone()
    gs = GraphedStep(lambda: D.train_step(netG, netD, crit, optD, optG, s_real, s_noise, cfg), {"real": s_real, "noise": s_noise},
                     [netG, netD], [optD, optG])
    for i in range(2):
        gs.load(real=reals[i], noise=noises[i])
        gs.replay()
    torch.cuda.synchronize()
    assert torch.equal(netG.flat_params, want[0]) and torch.equal(netD.flat_params, want[1])
