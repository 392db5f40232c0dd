"""GPU: the position-major forward / grad-input launches that skip their all-padding taps (csrc/conv_cliptab.h, CLIP kernels in
conv_igemm.hip) against today's kernels in one process — pcg_tune_set("pad_clip", 0) against the clipped path — and against float64
at the tolerance of tests/test_hip_igemm_branches.py.

The shapes are the smallest that hold every tile class (corner, edge, interior positions): 8x8 <-> 4x4 and 16x16 <-> 8x8, batch 128
(one 128-row tile per position) and batch 64 on the 64-row tile.  At these sizes a launch is a fraction of one round of workgroups, so
the schedule model (switch 1) predicts no gain and leaves it alone; the tests therefore force the path with the measurement values of
the switch, 2 / 3 / 4 (tiles long first / short first / in pairs) and 5 (64-row tiles), and assert through pcg_conv_pad_clip_query
that every case really ran clipped.  stream_k is 0 and fwd_splits is 1 in these tests: launches of 16 to 64 tiles would otherwise go
stream-K or split-K, which the clipped path leaves alone.

Conv outputs must be bit-equal (same products in the same order per output element, only zeros left out).  Fused BatchNorm sums reach
the finalize kernels as the same fp64 partial rows in another order: regrouping sums of <= 1e5 fp32 values in fp64 perturbs them far
below 2^-24 relative, so the finalized fp32 statistics may differ by at most 1 ulp; the number of entries that differ is printed."""
import contextlib

import pytest
import torch

from test_hip_igemm_branches import _dgrad64, _err, _fwd64, _nhwc, _on_dev, _operands, _tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, DGRAD = 0, 1
ORDERS = (2, 3, 4)
LRELU = 2


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import dcgan  # noqa: F401
    assert pcgan_amd.ops.ACT_LRELU == LRELU
    return pcgan_amd


@contextlib.contextmanager
def _switch(ops, mode):
    try:
        ops.tune("stream_k", 0)
        ops.tune("fwd_splits", 1)
        ops.tune("pad_clip", mode)
        yield
        torch.cuda.synchronize()
    finally:
        ops.tune("pad_clip", -1)
        ops.tune("fwd_splits", -1)
        ops.tune("stream_k", -1)


def _taken(ops, g, op, mode, groups=1):
    with _switch(ops, mode):
        return ops.conv_pad_clip_query(g, op, groups)[0]


def _ulp_close(a, b):
    """(all within 1 fp32 ulp, number of entries that differ at all)"""
    a, b = a.flatten(), b.flatten()
    ok = (a == b) | (torch.nextafter(a, b) == b)
    return bool(ok.all()), int((a != b).sum())


# form, IH, Cin, Cout, B, modes
CASES = [
    (FWD, 8, 64, 64, 128, ORDERS), (FWD, 16, 64, 64, 128, ORDERS), (FWD, 8, 64, 96, 128, ORDERS), (FWD, 8, 64, 96, 64, (5,)),
    (FWD, 16, 64, 96, 64, (5,)), (DGRAD, 8, 64, 64, 128, ORDERS), (DGRAD, 16, 64, 64, 128, ORDERS), (DGRAD, 8, 96, 64, 128, ORDERS),
]
IDS = [f"{'dgrad' if c[0] else 'fwd'}-{c[1]}to{c[1] // 2}-{c[2]}x{c[3]}-B{c[4]}" for c in CASES]


@pytest.mark.parametrize("form,IH,Cin,Cout,B,modes", CASES, ids=IDS)
def test_plain_epilogue_bit_equal_and_against_float64(pcg, form, IH, Cin, Cout, B, modes):
    ops = pcg.ops
    shape = (B, Cin, Cout, IH, IH, 4, 4, 2, 1)
    g = ops.conv_geom(B, IH, IH, Cin, Cout, 4, 4, 2, 1)
    x, w, dy, b, bx = _operands(shape, 1000 * IH + Cout + B + form)
    xd, wd, dyd, bd, bxd = _on_dev(_nhwc(x)), _on_dev(_nhwc(w)), _on_dev(_nhwc(dy)), _on_dev(b), _on_dev(bx)
    run = (lambda: ops.conv2d_fwd(g, xd, wd, bd)) if form == FWD else (lambda: ops.conv2d_dgrad(g, dyd, wd, bxd))
    with _switch(ops, 0):
        base = run()
    assert not _taken(ops, g, form, 0)
    want = _fwd64(x, w, 2, 1, b) if form == FWD else _dgrad64(x.shape, w, dy, 2, 1, bx)
    bound = _tol(16 * (Cin if form == FWD else Cout), 4.0)
    for mode in modes:
        assert _taken(ops, g, form, mode), f"mode {mode}: the launch did not take the clipped path"
        with _switch(ops, mode):
            got = run()
        assert torch.equal(got, base), f"mode {mode}: clipped output differs from today's kernel"
        err = _err(got, want)
        print(f"mode {mode}: max |err| vs float64 {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    # activation fused into the epilogue
    act = (lambda: ops.conv2d_fwd(g, xd, wd, bd, act=LRELU, slope=0.2)) if form == FWD else (lambda: ops.conv2d_dgrad(g, dyd, wd, bxd, act=LRELU, slope=0.2))
    with _switch(ops, 0):
        base = act()
    with _switch(ops, modes[0]):
        assert torch.equal(act(), base)


@pytest.mark.parametrize("form", [FWD, DGRAD], ids=["fwd", "dgrad"])
def test_batch_that_is_no_multiple_of_a_tile_stays_on_todays_kernels(pcg, form):
    ops = pcg.ops
    B, IH, C = 96, 8, 64
    g = ops.conv_geom(B, IH, IH, C, C, 4, 4, 2, 1)
    x, w, dy, b, bx = _operands((B, C, C, IH, IH, 4, 4, 2, 1), 96 + form)
    xd, wd, dyd = _on_dev(_nhwc(x)), _on_dev(_nhwc(w)), _on_dev(_nhwc(dy))
    run = (lambda: ops.conv2d_fwd(g, xd, wd)) if form == FWD else (lambda: ops.conv2d_dgrad(g, dyd, wd))
    with _switch(ops, 0):
        base = run()
    for mode in (1, 2, 3, 4, 5):
        assert not _taken(ops, g, form, mode)
        with _switch(ops, mode):
            assert torch.equal(run(), base)


STAT_CASES = [(f, ih) for f in (FWD, DGRAD) for ih in (8, 16)]


@pytest.mark.parametrize("form,IH", STAT_CASES, ids=[f"{'dgrad' if f else 'fwd'}-{ih}to{ih // 2}" for f, ih in STAT_CASES])
def test_fused_statistics_and_bnbwd_epilogues(pcg, form, IH):
    ops = pcg.ops
    B, C = 128, 64
    g = ops.conv_geom(B, IH, IH, C, C, 4, 4, 2, 1)
    x, w, dy, _, _ = _operands((B, C, C, IH, IH, 4, 4, 2, 1), 7 * IH + form)
    a = _on_dev(_nhwc(x)) if form == FWD else _on_dev(_nhwc(dy))       # the kernel's activation operand
    wd = _on_dev(_nhwc(w))
    gen = torch.Generator(device=DEV).manual_seed(IH + form)
    out_shape = (B, g.OH, g.OW, C) if form == FWD else (B, IH, IH, C)
    z_below = torch.randn(out_shape, generator=gen, device=DEV)
    mean, invstd = torch.randn(C, generator=gen, device=DEV) * 0.1, torch.rand(C, generator=gen, device=DEV) + 0.5
    gamma, beta = torch.rand(C, generator=gen, device=DEV) + 0.5, torch.randn(C, generator=gen, device=DEV) * 0.1

    def stats():
        rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        z, m, i = ops.conv_bn_train(g, a, wd, None, form == DGRAD, 1e-5, 0.1, rm, rv, nbt)
        return z, (m, i, rm, rv)

    def bnbwd():
        dm, partial, nparts = ops.conv_bwd_data_fused(g, a, wd, form == FWD, LRELU, 0.2, z_below=z_below, bn=(mean, invstd, gamma, beta))
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ops.bn_bwd_partial(dm.clone(), z_below, C, mean, invstd, gamma, partial, nparts, dg, db, False)
        return dm, (dg, db)

    for name, fn in (("statistics", stats), ("bnbwd", bnbwd)):
        with _switch(ops, 0):
            base, base_fin = fn()
        for mode in ORDERS:
            assert _taken(ops, g, form, mode)
            with _switch(ops, mode):
                got, fin = fn()
            assert torch.equal(got, base), f"{name} mode {mode}: conv output differs"
            for k, (p, q) in enumerate(zip(fin, base_fin)):
                ok, n = _ulp_close(p, q)
                print(f"{name} mode {mode} output {k}: {n} of {p.numel()} entries differ")
                assert ok, f"{name} mode {mode} output {k}: more than 1 ulp"


def test_grouped_epilogues_two_groups_of_128(pcg):
    ops = pcg.ops
    B, C, IH, G = 256, 64, 8, 2
    g = ops.conv_geom(B, IH, IH, C, C, 4, 4, 2, 1)
    x, w, dy, _, _ = _operands((B, C, C, IH, IH, 4, 4, 2, 1), 256)
    xd, wd, dyd = _on_dev(_nhwc(x)), _on_dev(_nhwc(w)), _on_dev(_nhwc(dy))
    gen = torch.Generator(device=DEV).manual_seed(2)
    z_below = torch.randn(B, IH, IH, C, generator=gen, device=DEV)
    mean, invstd = torch.randn(G, C, generator=gen, device=DEV) * 0.1, torch.rand(G, C, generator=gen, device=DEV) + 0.5
    gamma, beta = torch.rand(C, generator=gen, device=DEV) + 0.5, torch.randn(C, generator=gen, device=DEV) * 0.1

    def fwd_g():
        rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        z, m, i = ops.conv_bn_train_g(g, xd, wd, None, 1e-5, 0.1, rm, rv, nbt, G)
        return z, (m, i, rm, rv)

    def dgrad_g():
        dm, partial, nparts, nph = ops.conv_bwd_data_fused_g(g, dyd, wd, LRELU, 0.2, z_below, (mean, invstd, gamma, beta), G)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ops.bn_bwd_partial_g(dm.clone(), z_below, C, mean, invstd, gamma, partial, nparts, nph, dg, db, False, G)
        return dm, (dg, db)

    for form, fn in ((FWD, fwd_g), (DGRAD, dgrad_g)):
        with _switch(ops, 0):
            base, base_fin = fn()
        # the two groups' statistics really differ (a mixed-up group row would show)
        if form == FWD:
            assert not torch.equal(base_fin[0][0], base_fin[0][1])
        for mode in ORDERS:
            assert _taken(ops, g, form, mode, G)
            with _switch(ops, mode):
                got, fin = fn()
            assert torch.equal(got, base), f"form {form} mode {mode}: conv output differs"
            for k, (p, q) in enumerate(zip(fin, base_fin)):
                ok, n = _ulp_close(p, q)
                print(f"grouped form {form} mode {mode} output {k}: {n} of {p.numel()} entries differ")
                assert ok


def test_small_dcgan_step_eager_against_graph_replay(pcg):
    """One DCGAN step (width 16, batch 128) with the clipped path on: eager against graph replay, bit for bit (the check of
    tests/test_hip_graph.py)."""
    from pcgan_amd.nn import GraphedStep
    from test_hip_graph import _fresh
    D, ops = pcg.dcgan, pcg.ops
    cfg = {"g_hidden": 16, "d_hidden": 16, "z_dim": 32}
    B = 128
    gen = torch.Generator().manual_seed(11)
    real = (torch.rand(B, 1, 64, 64, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(B, 32, 1, 1, generator=gen).to(DEV)
    with _switch(ops, 2):
        netG, netD, crit, optD, optG = _fresh(D, cfg)
        o = D.train_step(netG, netD, crit, optD, optG, real, noise, cfg)
        want = ([o[k].item() for k in ("errD_real", "errD_fake", "errG")], netG.flat_params.clone(), netD.flat_params.clone())
        netG, netD, crit, optD, optG = _fresh(D, cfg)
        s_real, s_noise = real.clone(), noise.clone()
        gs = GraphedStep(lambda: D.train_step(netG, netD, crit, optD, optG, s_real, s_noise, cfg), {"real": s_real, "noise": s_noise},
                         [netG, netD], [optD, optG])
        gs.load(real=real, noise=noise)
        o = gs.replay()
        torch.cuda.synchronize()
        got = ([o[k].item() for k in ("errD_real", "errD_fake", "errG")], netG.flat_params, netD.flat_params)
        assert got[0] == want[0]
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
        # the step's 16 <-> 8 layer (32 -> 64 channels) at this batch is eligible and ran clipped
        assert ops.conv_pad_clip_query(ops.conv_geom(B, 16, 16, 32, 64, 4, 4, 2, 1), 0)[0]
