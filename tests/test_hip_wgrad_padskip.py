"""GPU: the fp32 weight gradients whose consumer waves leave out the MFMAs that multiply only padding (csrc/igemm_core.h PadSkip,
pcg_tune_set("wgrad_padskip", 0 .. 3)) against today's kernels — bit for bit in one process: the default (1), every eligible launch in
the paired block order (2) and in today's order (3) — and against a float64 weight gradient on the CPU at the tolerance
tests/test_hip_wgrad_pixtab.py uses (test_hip_benchshape._bound: 16 standard deviations of a K-term fp32 fma chain).

Shapes are the smallest at which each rule can go wrong.  IH = 8: OW = 4, MFMA t of every k-group is padding for kw = 0 / 3 (fixed
per wave); IH = 16: a k-group is one output row, padding for kh = 0 / 3 at the first / last row; IH = 32: half a row.  Cin = 64 puts
two taps into a 128-column tile (one per wave tile), Cin = 128 one; Cout = 64 takes the 64x128 tile, Cout = 96 the 128x128 one with a
ragged M tile; B = 12 gives K-slices that begin inside the batch at other positions than B = 8 does.  Every result is computed
with and without the pixel table, with `accumulate`, and as two BatchNorm groups.  The stream-K kernel needs more than 96 tiles
(Cin = 448, not a power of two: the tap of a wave tile is a real division) and the paired order at least 512 workgroups."""
import ctypes

import pytest
import torch

from test_hip_benchshape import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K4 = (4, 2, 1)          # kernel, stride, pad of every case


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import dcgan  # noqa: F401
    return pcgan_amd


def _inputs(B, Cin, Cout, H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, H, H, Cin, generator=g, device=DEV)
    dy = torch.randn(B, H // 2, H // 2, Cout, generator=g, device=DEV)
    g0 = torch.randn(Cout, 4, 4, Cin, generator=g, device=DEV)
    return x, dy, g0


def _ref64(x, dy):
    """float64 weight gradient on the CPU, OHWI: dy^T (K x Cout) times the im2col rows of x (K x Cin*16), one GEMM."""
    B, H, _, Cin = x.shape
    cols = torch.nn.functional.unfold(x.cpu().double().permute(0, 3, 1, 2), 4, padding=1, stride=2)      # [B][Cin*16][OH*OW]
    cols = cols.permute(0, 2, 1).reshape(-1, Cin, 4, 4)
    d = dy.cpu().double().reshape(-1, dy.shape[-1])
    return torch.einsum("ko,kchw->ohwc", d, cols).contiguous()


def _modes(ops, fn, modes=(0, 2, 3, 1)):
    """fn() under every value of the switch."""
    out = []
    try:
        for v in modes:
            ops.tune("wgrad_padskip", v)
            out.append(fn())
        torch.cuda.synchronize()
    finally:
        ops.tune("wgrad_padskip", -1)
    return out


def _same(r):
    return all(torch.equal(r[0], v) for v in r[1:])


def _check_all_forms(ops, x, dy, g0, name):
    """Switch 0 .. 3 bit-equal, right against float64: plain, accumulate, two groups; with and without the pixel table."""
    B, H, _, Cin = x.shape
    Cout = dy.shape[-1]
    k, s, p = K4
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    assert ops.conv_wgrad_padskip_query(geom)[0], name
    ref = _ref64(x, dy)
    assert ref.abs().max().item() > 1.0
    K = B * (H // 2) ** 2
    try:
        for tab in (1, 0):
            ops.tune("wgrad_pixtab", tab)
            what = f"{name} pixtab {tab}"
            r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
            assert _same(r), what
            err = (r[1].cpu().double() - ref).abs().max().item()
            print(f"{what}: max |err| vs float64 {err:.3e} (bound {_bound(K, 1.0):.3e})")
            assert err <= _bound(K, 1.0), what

            r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, g0.clone(), True))
            assert _same(r), what + " accumulate"
            err = (r[1].cpu().double() - (ref + g0.cpu().double())).abs().max().item()
            assert err <= _bound(K + 1, 1.0), f"{what} accumulate: {err:.3e}"

            # two BatchNorm groups: the halves of the batch as two launches into one gradient (another B, the same geometry otherwise)
            h = B // 2
            gh = ops.conv_geom(h, H, H, Cin, Cout, k, k, s, p)

            def halves():
                dw = torch.empty_like(g0)
                ops.conv2d_wgrad(gh, x[:h], dy[:h], dw, False)
                return ops.conv2d_wgrad(gh, x[h:], dy[h:], dw, True)
            r = _modes(ops, halves)
            assert _same(r), what + " two groups"
            err = (r[1].cpu().double() - ref).abs().max().item()
            assert err <= _bound(K + 1, 1.0), f"{what} two groups: {err:.3e}"
    finally:
        ops.tune("wgrad_pixtab", -1)


@pytest.mark.parametrize("H", [8, 16, 32])
@pytest.mark.parametrize("Cin,Cout,B", [(64, 64, 8), (64, 96, 12), (128, 64, 12), (128, 96, 8)])
def test_data_parallel_kernels(pcg, H, Cin, Cout, B):
    ops = pcg.ops
    x, dy, g0 = _inputs(B, Cin, Cout, H, seed=H + Cin + Cout + B)
    for sk in (0, 2):           # at most 16 tiles: the slab form under either setting
        try:
            ops.tune("stream_k", sk)
            _check_all_forms(ops, x, dy, g0, f"{H}->{H // 2} B{B} {Cin}->{Cout} stream_k {sk}")
        finally:
            ops.tune("stream_k", -1)


# 2 x 56 tiles of 128x128 (M = 160: a ragged second M tile), K = 512 positions = 16 k-tiles: stream_k 2 cuts them into 512 ranges of
# 3 or 4 k-tiles, so segments begin at k-tiles 3, 4, 7, ... — inside an image at IH = 8 and 16, inside an output row's neighbours at 32
@pytest.mark.parametrize("H,B", [(8, 32), (16, 8), (32, 2)])
def test_stream_k_kernel(pcg, H, B):
    ops = pcg.ops
    Cin, Cout = 448, 160
    x, dy, g0 = _inputs(B, Cin, Cout, H, seed=H)
    k, s, p = K4
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    desc = ctypes.create_string_buffer(256)
    lib = pcg.load()
    try:
        ops.tune("stream_k", 2)
        ops.tune("sk_blocks", 512)              # (the planner's model rates 256 ranges of 7 k-tiles a hair better at this K)
        ops._conv_scratch()
        assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
        assert desc.value.decode().startswith("stream-K") and "over 512 ranges" in desc.value.decode(), desc.value
        _check_all_forms(ops, x, dy, g0, f"stream-K {H}->{H // 2} B{B}")
        ops.tune("stream_k", 0)                 # the same gradient as 112 tiles x K-slices (slabs)
        assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
        assert desc.value.decode().startswith("128x128 tiles"), desc.value
        r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
        assert _same(r)
    finally:
        ops.tune("stream_k", -1)
        ops.tune("sk_blocks", -1)


# 512 workgroups, so that the paired order (1, 2) really permutes a round: 32 tiles x 16 K-slices tile-major (the D3 form) and 8 tiles x 64
# K-slices slice-major (the D2 form)
@pytest.mark.parametrize("H,B,Cin,Cout", [(16, 64, 128, 256), (32, 128, 64, 128)])
def test_paired_block_order_at_512_workgroups(pcg, H, B, Cin, Cout):
    ops = pcg.ops
    x, dy, g0 = _inputs(B, Cin, Cout, H, seed=3)
    k, s, p = K4
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    desc = ctypes.create_string_buffer(256)
    assert pcg.load().pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
    tiles = (Cout // 128) * (16 * Cin // 128)
    assert desc.value.decode().startswith(f"128x128 tiles: {tiles} x {512 // tiles} K-slices"), desc.value
    r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
    assert _same(r)
    K = B * (H // 2) ** 2
    err = (r[2].cpu().double() - _ref64(x, dy)).abs().max().item()
    assert err <= _bound(K, 1.0), f"{err:.3e}"


def test_ineligible_and_bf16_launches_do_not_move(pcg):
    """Cin = 32 (a wave tile spans two taps) and the bf16 twin launch the kernels they launch today under every value of the switch."""
    ops = pcg.ops
    x, dy, g0 = _inputs(8, 32, 64, 16, seed=9)
    k, s, p = K4
    geom = ops.conv_geom(8, 16, 16, 32, 64, k, k, s, p)
    assert not ops.conv_wgrad_padskip_query(geom)[0]
    r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
    assert _same(r)
    assert (r[1].cpu().double() - _ref64(x, dy)).abs().max().item() <= _bound(8 * 64, 1.0)
    x, dy, g0 = _inputs(8, 64, 64, 16, seed=10)
    geom = ops.conv_geom(8, 16, 16, 64, 64, k, k, s, p)
    with ops.conv_precision("bf16"):
        assert not ops.conv_wgrad_padskip_query(geom)[0]
        r = _modes(ops, lambda: ops.conv2d_wgrad(geom, x, dy, torch.empty_like(g0), False))
    assert _same(r)


def test_captured_backward_replays_bit_equal_to_eager(pcg):
    """A DCGAN step at width 64 (D2 .. D4 and G2 .. G4 are eligible layers) with the skip on: eager against captured and replayed."""
    from pcgan_amd.nn import GraphedStep
    D, ops = pcg.dcgan, pcg.ops
    cfg = {"g_hidden": 64, "d_hidden": 64, "z_dim": 32}
    B = 8
    g = torch.Generator().manual_seed(5)
    reals = [(torch.rand(B, 1, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    noises = [torch.randn(B, 32, 1, 1, generator=g).to(DEV) for _ in range(2)]
    assert ops.conv_wgrad_padskip_query(ops.conv_geom(B, 32, 32, 64, 128, 4, 4, 2, 1))[0]          # D2 of this width

    def fresh():
        torch.manual_seed(0)
        netG, netD = D.Generator(cfg).to(DEV), D.Discriminator(cfg).to(DEV)
        netG.apply(D.weights_init); netD.apply(D.weights_init)
        return (netG, netD) + tuple(D.make_optimizers(netG, netD, cfg))

    def eager(mode):            # 2: D2 / G4 (OW = 16) skip as well
        ops.tune("wgrad_padskip", mode)
        netG, netD, crit, optD, optG = fresh()
        for i in range(2):
            D.train_step(netG, netD, crit, optD, optG, reals[i], noises[i], cfg)
        return netG.flat_params.clone(), netD.flat_params.clone()

    try:
        want = eager(2)
        base = eager(0)
        assert torch.equal(want[0], base[0]) and torch.equal(want[1], base[1]), "the skip changed a training step"
        ops.tune("wgrad_padskip", 2)
        netG, netD, crit, optD, optG = fresh()
        s_real, s_noise = reals[0].clone(), noises[0].clone()
        gs = GraphedStep(lambda: D.train_step(netG, netD, crit, optD, optG, s_real, s_noise, cfg), {"real": s_real, "noise": s_noise},
                         [netG, netD], [optD, optG])
        for i in range(2):
            gs.load(real=reals[i], noise=noises[i])
            gs.replay()
        torch.cuda.synchronize()
        assert torch.equal(netG.flat_params, want[0]) and torch.equal(netD.flat_params, want[1])
    finally:
        ops.tune("wgrad_padskip", -1)
