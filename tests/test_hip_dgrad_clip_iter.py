"""GPU: the tap walk of the clipped grad-input kernel (DgradTapIterT<true>::advance, csrc/conv_loaders.h) in both k-tile orders and with
a ragged last channel chunk, and the pad_clip_dgrad switch.

advance() computes on locals and stores every field once, after the branch on the k-tile order, so that the loaders stay in registers
(DESIGN.md section 3.1.3).  A wrong rewrite visits the
(tap, channel chunk) k-tiles in another order, twice, or not at all: the sums of an output element then come out in another order or
short of a tap, which bit-equality with today's kernel (pad_clip 0, the unclipped walk) catches; the float64 bound of
tests/test_hip_pad_clip.py is asserted beside it.  K = Cout: 64 and 96 are whole 32-channel chunks, 48 leaves a last chunk of 16.

The launches here are a fraction of one round of workgroups, so the schedule model leaves them alone; the walk tests force the clipped
path with the switch's measurement values 2 / 3 / 4 and assert through pcg_conv_pad_clip_query that it ran."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_hip_igemm_branches import _dgrad64, _err, _nhwc, _on_dev, _operands, _tol
from test_hip_pad_clip import DGRAD, FWD, ORDERS, _switch, _taken, pcg  # noqa: F401  (pcg: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, CIN = 128, 64


@functools.lru_cache(maxsize=None)
def _case(IH, Cout):
    """operands on the device and the float64 grad-input, once per shape (shared by the two k-tile orders)"""
    x, w, dy, _, bx = _operands((B, CIN, Cout, IH, IH, 4, 4, 2, 1), 31 * IH + Cout)
    want = _dgrad64(x.shape, w, dy, 2, 1, bx)
    return _on_dev(_nhwc(w)), _on_dev(_nhwc(dy)), _on_dev(bx), want


@pytest.mark.parametrize("korder", [0, 1])
@pytest.mark.parametrize("Cout", [48, 64, 96])
@pytest.mark.parametrize("IH", [8, 16], ids=["8to4", "16to8"])
def test_tap_walk_both_orders_and_k_tail(pcg, IH, Cout, korder):
    ops = pcg.ops
    g = ops.conv_geom(B, IH, IH, CIN, Cout, 4, 4, 2, 1)
    wd, dyd, bxd, want = _case(IH, Cout)
    bound = _tol(16 * Cout, 4.0)
    try:
        ops.tune("korder", korder)
        ops.tune("pad_clip_dgrad", 1)
        with _switch(ops, 0):
            base = ops.conv2d_dgrad(g, dyd, wd, bxd)
        assert not _taken(ops, g, DGRAD, 0)
        for mode in ORDERS:
            assert _taken(ops, g, DGRAD, mode), f"mode {mode}: the launch did not take the clipped path"
            with _switch(ops, mode):
                got = ops.conv2d_dgrad(g, dyd, wd, bxd)
            assert torch.equal(got, base), f"korder {korder} mode {mode}: clipped output differs from today's kernel"
            err = _err(got, want)
            print(f"korder {korder} mode {mode}: max |err| vs float64 {err:.3e} (bound {bound:.3e})")
            assert err <= bound
    finally:
        ops.tune("pad_clip_dgrad", -1)
        ops.tune("korder", -1)


def _model(lib, lens):
    a = np.asarray(lens, dtype=np.int32)
    return lib.pcg_conv_sched_model(ctypes.c_void_p(a.ctypes.data), len(a))


def _best_ratio(lib, P, tiles):
    """best of long first / short first over today's launch for `tiles` 128-row tiles of four P x P phase grids, by the schedule model:
    per phase (P-1)^2 positions keep 4 taps, 2(P-1) keep 2 and one keeps 1 (tests/test_conv_pad_clip_host.py)"""
    per = tiles // (P * P)
    c = [4] * ((P - 1) ** 2 * per) + [2] * (2 * (P - 1) * per) + [1] * per
    base = _model(lib, [4] * tiles)
    return min(_model(lib, sorted(c, reverse=True)), _model(lib, sorted(c))) / base


def test_pad_clip_dgrad_0_keeps_the_grad_input_on_todays_kernel(pcg):
    """Switch 1 of pad_clip: among the 256 -> 512 8 <-> 4 and 128 -> 256 16 <-> 8 grad-inputs at batches 512 .. 4096 the one the schedule
    model gives most to is taken with pad_clip_dgrad 1 (the default) and left alone with 0; the forward answer does not move."""
    ops, lib = pcg.ops, pcg.load()
    cands = []
    for IH, Cin, Cout in ((8, 256, 512), (16, 128, 256)):
        for batch in (512, 1024, 2048, 4096):
            P = IH // 2
            tiles = 4 * P * P * (batch // 128) * ((Cin + 127) // 128)
            cands.append((_best_ratio(lib, P, tiles), IH, Cin, Cout, batch))
    ratio, IH, Cin, Cout, batch = min(cands)
    print(f"schedule model: best candidate {Cin}->{Cout} {IH}x{IH} batch {batch}, clipped / today's {ratio:.3f}")
    assert ratio < 0.95
    g = ops.conv_geom(batch, IH, IH, Cin, Cout, 4, 4, 2, 1)
    try:
        ops.tune("pad_clip", 1)
        answers = {}
        for v in (1, 0, -1):
            ops.tune("pad_clip_dgrad", v)
            answers[v] = (ops.conv_pad_clip_query(g, DGRAD), ops.conv_pad_clip_query(g, FWD))
        assert answers[1][0][0] == 1, f"the model does not take the launch it predicts {ratio:.3f} for: {answers[1][0]}"
        assert answers[-1] == answers[1]                          # on by default
        assert answers[0][0][0] == 0
        assert answers[0][1] == answers[1][1]                     # the forward kernel's answer is not touched
        # the forced modes are measurements of the kernel itself: not gated
        ops.tune("pad_clip", 3)
        assert ops.conv_pad_clip_query(g, DGRAD)[0] == 1
    finally:
        ops.tune("pad_clip_dgrad", -1)
        ops.tune("pad_clip", -1)


def _eager_and_replay(pcg, seed):
    """one DCGAN step (width 16, batch 128) eagerly and as a graph replay from the same start: (losses, G params, D params) of each"""
    from pcgan_amd.nn import GraphedStep
    from test_hip_graph import _fresh
    D = pcg.dcgan
    cfg = {"g_hidden": 16, "d_hidden": 16, "z_dim": 32}
    gen = torch.Generator().manual_seed(seed)
    real = (torch.rand(B, 1, 64, 64, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(B, 32, 1, 1, generator=gen).to(DEV)
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
    got = ([o[k].item() for k in ("errD_real", "errD_fake", "errG")], netG.flat_params.clone(), netD.flat_params.clone())
    return want, got


def _same(want, got):
    assert got[0] == want[0]
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_small_dcgan_step_eager_against_graph_replay_default_switches(pcg):
    """One DCGAN step (width 16, batch 128) as shipped — no switch set: eager against graph replay, bit for bit.  (At this size no
    grad-input launch reaches one round of workgroups, so the planner leaves them all; the next test clips them.)"""
    _same(*_eager_and_replay(pcg, 12))


def test_small_dcgan_step_with_clipped_grad_inputs_eager_against_graph_replay(pcg):
    """The same step with pad_clip 1 and pad_clip_dgrad 2 — every eligible grad-input launch on the clipped kernel, in the planner's
    order (stream_k 0: launches this small would otherwise go stream-K, which the clipped path leaves alone): the clipped grad-input
    under capture and replay against eager, bit for bit."""
    ops = pcg.ops
    try:
        ops.tune("pad_clip_dgrad", 2)
        with _switch(ops, 1):
            # a 16 <-> 8 layer of the step (32 -> 64 channels) at this batch: its grad-input runs clipped
            assert ops.conv_pad_clip_query(ops.conv_geom(B, 16, 16, 32, 64, 4, 4, 2, 1), DGRAD)[0] == 1
            want, got = _eager_and_replay(pcg, 13)
        _same(want, got)
        ops.tune("pad_clip_dgrad", 1)
        with _switch(ops, 1):       # as shipped, the same launch is below one round of workgroups and stays on today's kernel
            assert ops.conv_pad_clip_query(ops.conv_geom(B, 16, 16, 32, 64, 4, 4, 2, 1), DGRAD)[0] == 0
    finally:
        ops.tune("pad_clip_dgrad", -1)
