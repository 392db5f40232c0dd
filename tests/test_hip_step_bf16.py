"""GPU: whole training steps with the nets' convolutions in bf16-operand mode (FlatModule.conv_precision = "bf16").

  * against the float64 oracle (the sizes of test_hip_dcgan.py::test_full_width_step_vs_oracle and test_hip_countergan.py::
    test_step_vs_oracle_float64): losses within relative 1e-2, every G and D gradient within relative L2 5e-2 — and every gradient
    FURTHER from float64 than the fp32 HIP step's: the backward, which autograd runs on its own thread, ran in bf16 too;
  * the mode is per net: an fp32 generator is bit-identical whatever the calling thread or the discriminator use;
  * a captured GraphedStep replays the eager bf16 step bit for bit;
  * ten DCGAN steps stay finite and close to the fp32 trajectory (closer than that trajectory is to its start).
"""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import countergan_ref as CR
from oracle import dcgan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import countergan, dcgan  # noqa: F401
    yield pcgan_amd
    assert pcgan_amd.load().pcg_conv_precision_get() == 0       # no net leaves its mode on the calling thread


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _smooth(net, slope=0.99):
    """Every ReLU / LeakyReLU -> LeakyReLU(0.99), as in test_hip_benchshape.py (c): the same kernels and mask paths, but an activation
    whose sign the operand rounding flips changes its gradient by 1 % instead of 80-100 %."""
    for i, m in enumerate(net.main):
        if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
            net.main[i] = torch.nn.LeakyReLU(slope, inplace=False)
    return net


def _check_grads(tag, bf_net, f32_net, r64_net, loose=None, bound=5e-2):
    bad, worst = {}, 0.0
    for (n, p), (_, q), (_, t) in zip(bf_net.named_parameters(), f32_net.named_parameters(), r64_net.named_parameters()):
        t64 = t.grad.detach().cpu().double().numpy()
        e16, e32 = _rel_l2(p.grad.cpu().numpy(), t64), _rel_l2(q.grad.cpu().numpy(), t64)
        if e32 > 0.5:                    # a gradient that is zero up to rounding (a conv bias in front of a BatchNorm): no signal to test
            continue
        if not (e32 < e16 <= (loose or {}).get(n, bound)):   # within the bound, and further from float64 than the fp32 step (it ran bf16)
            bad[f"{tag}.{n}"] = (f"bf16 {e16:.2e}", f"fp32 {e32:.2e}")
        worst = max(worst, e16)
    print(f"{tag}: worst bf16 gradient rel-L2 {worst:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("smooth", [True, False], ids=["slope0.99", "reference-activations"])
@pytest.mark.parametrize("batch,pair", [(8, True), (6, False)], ids=["paired-D", "statement-order-D"])
def test_dcgan_step_vs_oracle(pcg, batch, pair, smooth):
    """As test_hip_benchshape.py (c) runs the stated-tolerance step: lr = 0 in both implementations (every kernel still runs, Adam
    included; Adam's sign-like first update would turn the D gradients' rounding into 2*lr weight changes before the G step), and every
    ReLU / LeakyReLU as LeakyReLU(0.99).  With the reference's own activations the operand rounding moves ~1e-3 of the
    pre-activations across the ReLU kinks of G at batch 8, each flip worth 80-100 % of an element's gradient: measured 12-16 %
    rel-L2 on every G gradient, 10-11 % on the worst D one (fp32: 1e-6 .. 2e-3) — a property of bf16 operands on this net, not of the kernels.
    The reference-activations variant holds the reference nets themselves to that measured level: every gradient within 0.25 and
    further from float64 than the fp32 step's."""
    D = pcg.dcgan
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = {"lr": 0.0}
    refG, refD = R.build(None, seed=1)
    sd_G, sd_D = refG.state_dict(), refD.state_dict()
    sm = _smooth if smooth else (lambda n: n)
    r64G, r64D = sm(copy.deepcopy(refG).double()), sm(copy.deepcopy(refD).double())
    real, noise = R.synthetic_batch(batch, seed=10)
    tru = R.dcgan_step(r64G, r64D, *R.make_optimizers(r64G, r64D, cfg), real.double(), noise.double())
    nets, outs = {}, {}
    for prec in ("fp32", "bf16"):
        netG, netD = sm(D.Generator()), sm(D.Discriminator())
        netG.load_state_dict(sd_G); netD.load_state_dict(sd_D)
        netG.to(DEV); netD.to(DEV)
        netG.conv_precision = netD.conv_precision = prec
        outs[prec] = D.train_step(netG, netD, *D.make_optimizers(netG, netD, cfg), real.to(DEV), noise.to(DEV), skip_dead_d_wgrad=False,
                                  pair=pair)
        nets[prec] = (netG, netD)
    torch.cuda.synchronize()
    for name in ("errD_real", "errD_fake", "errG"):
        got = outs["bf16"][name].item()
        assert abs(got - tru[name]) <= 1e-2 * abs(tru[name]), f"{name}: {got} vs {tru[name]}"
    bound = 5e-2 if smooth else 0.25
    _check_grads("G", nets["bf16"][0], nets["fp32"][0], r64G, bound=bound)
    _check_grads("D", nets["bf16"][1], nets["fp32"][1], r64D, bound=bound)


def _cg_build(pcg, seed):
    K = pcg.countergan
    refG, refD, refC = CR.build(seed=seed)
    G, D, C = K.ResidualGenerator(), K.Discriminator(), K.CNNClassifier()
    G.load_state_dict(refG.state_dict()); D.load_state_dict(refD.state_dict()); C.load_state_dict(refC.state_dict())
    C.eval()
    for p in C.parameters():
        p.requires_grad = False
    return (G.to(DEV), D.to(DEV), C.to(DEV)), (refG, refD, refC)


def test_countergan_step_vs_oracle(pcg):
    K = pcg.countergan
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x, y, t, m = CR.synthetic_batch(16, seed=5)
    runs = {}
    for prec in ("fp32", "bf16"):
        (G, D, C), refs = _cg_build(pcg, seed=3)
        G.conv_precision = D.conv_precision = prec
        opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
        out = K.train_step(G, D, C, opt_g, opt_d, bce, ce, x.to(DEV), y.to(DEV), t.to(DEV), m.to(DEV), skip_dead_d_wgrad=False)
        runs[prec] = (G, D, out)
    r64 = [copy.deepcopy(n).double() for n in refs]
    tru = CR.countergan_step(*r64, *CR.make_optimizers(r64[0], r64[1]), x.double(), y, t, m.double())
    torch.cuda.synchronize()
    for name in ("d_loss", "g_adv", "g_cls", "reg_l1", "mask_pen", "g_loss"):
        got = runs["bf16"][2][name].item()
        assert abs(got - tru[name]) <= 1e-2 * abs(tru[name]) + 1e-6, f"{name}: {got} vs {tru[name]}"
    # the label embedding's gradient is a sum over the label-map plane of a grad-input that mostly cancels: already the worst-
    # conditioned tensor in fp32 (2e-5 where the others are ~1e-6); in bf16 8e-2 (measured)
    _check_grads("G", runs["bf16"][0], runs["fp32"][0], r64[0], loose={"embed.weight": 0.15})
    # D's LeakyReLU(0.2) kinks: the operand rounding moves pre-activations across them (each flip 80 % of an element's gradient),
    # and the layers nearest the input collect the flips of every layer above — measured 5.4e-2 .. 7.8e-2 on cond_embed / main.0 /
    # main.2 (fp32: 1e-6), the rest below 5e-2.  The DCGAN test above removes the kinks and holds every gradient to 5e-2.
    _check_grads("D", runs["bf16"][1], runs["fp32"][1], r64[1], bound=1e-1)


def test_precision_is_per_net(pcg):
    D, ops = pcg.dcgan, pcg.ops
    cfg = {"g_hidden": 32, "d_hidden": 32, "z_dim": 64}
    torch.manual_seed(2)
    netG, netD = D.Generator(cfg).to(DEV), D.Discriminator(cfg).to(DEV)
    netG.apply(D.weights_init); netD.apply(D.weights_init)
    noise = torch.randn(16, 64, 1, 1, device=DEV)
    with torch.no_grad():
        g32 = netG(noise)
        d32 = netD(g32)
        netD.conv_precision = "bf16"
        with ops.conv_precision("bf16"):             # the calling thread's mode does not reach an fp32 net
            g_mixed = netG(noise)
        d16 = netD(g_mixed)
    assert torch.equal(g32, g_mixed)
    assert not torch.equal(d16, d32)
    # the autograd path: G's output with D in bf16 inside one training step equals the all-fp32 one
    crit, optD, optG = D.make_optimizers(netG, netD, cfg)
    fake = netG(noise)
    loss = crit(netD(fake), torch.ones(16, device=DEV))
    loss.backward()
    assert torch.equal(fake.detach(), g32)


def test_nets_without_the_mode_pin_fp32(pcg):
    """WGAN-GP and the house nets refuse "bf16"; their sweeps also stay fp32 inside a caller's bf16 scope (their large linears run on
    the implicit-GEMM kernels as 1x1 convolutions, nn._lin_mfma)."""
    from pcgan_amd import house as H
    from pcgan_amd import wgan as W
    ops = pcg.ops
    torch.manual_seed(3)
    critic, gen = W.Critic().to(DEV), W.Generator().to(DEV)
    clf = H.NNClassifier(17, 4).to(DEV).eval()
    img, cond = torch.randn(64, 1, 28, 28, device=DEV), torch.eye(10, device=DEV)[torch.arange(64, device=DEV) % 10]
    lat = torch.randn(64, 32, device=DEV)
    rows = torch.randn(4096, 17, device=DEV)
    with torch.no_grad():
        want = (critic(img, cond), gen(lat, cond), clf(rows))
        with ops.conv_precision("bf16"):
            got = (critic(img, cond), gen(lat, cond), clf(rows))
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def _fresh(D, cfg, prec, seed=5):
    torch.manual_seed(seed)
    netG, netD = D.Generator(cfg).to(DEV), D.Discriminator(cfg).to(DEV)
    netG.apply(D.weights_init); netD.apply(D.weights_init)
    netG.conv_precision = netD.conv_precision = prec
    return (netG, netD) + tuple(D.make_optimizers(netG, netD, cfg))


def test_graph_replay_matches_eager_bf16(pcg):
    from pcgan_amd.nn import GraphedStep
    D = pcg.dcgan
    cfg = {"g_hidden": 32, "d_hidden": 32, "z_dim": 64}
    real, noise = R.synthetic_batch(32, seed=4, config=cfg)
    real, noise = real.to(DEV), noise.to(DEV)
    netG, netD, crit, optD, optG = _fresh(D, cfg, "bf16")
    eager = D.train_step(netG, netD, crit, optD, optG, real, noise, cfg)
    gG, gD, gcrit, goptD, goptG = _fresh(D, cfg, "bf16")
    s_real, s_noise = real.clone(), noise.clone()
    gs = GraphedStep(lambda: D.train_step(gG, gD, gcrit, goptD, goptG, s_real, s_noise, cfg), {"real": s_real, "noise": s_noise},
                     [gG, gD], [goptD, goptG])
    out = gs.replay()
    torch.cuda.synchronize()
    for k in ("errD_real", "errD_fake", "errG"):
        assert torch.equal(out[k], eager[k]), k
    assert torch.equal(gG.flat_params, netG.flat_params) and torch.equal(gD.flat_params, netD.flat_params)
    f32G, f32D, *opt = _fresh(D, cfg, "fp32")
    D.train_step(f32G, f32D, *opt, real, noise, cfg)
    assert not torch.equal(f32D.flat_params, netD.flat_params)


def test_ten_step_trajectory(pcg):
    D = pcg.dcgan
    cfg = {"g_hidden": 32, "d_hidden": 32, "z_dim": 64}
    batches = [tuple(t.to(DEV) for t in R.synthetic_batch(32, seed=100 + i, config=cfg)) for i in range(10)]
    runs = {}
    for prec in ("fp32", "bf16"):
        netG, netD, crit, optD, optG = _fresh(D, cfg, prec)
        w0 = [netG.flat_params.clone(), netD.flat_params.clone()]
        for real, noise in batches:
            out = D.train_step(netG, netD, crit, optD, optG, real, noise, cfg)
            assert all(torch.isfinite(out[k]).item() for k in ("errD_real", "errD_fake", "errG")), prec
        runs[prec] = (w0, [netG.flat_params.clone(), netD.flat_params.clone()])
    for i, tag in enumerate(("G", "D")):
        assert torch.equal(runs["fp32"][0][i], runs["bf16"][0][i])
        moved = float((runs["fp32"][1][i] - runs["fp32"][0][i]).norm())
        apart = float((runs["bf16"][1][i] - runs["fp32"][1][i]).norm())
        assert 0 < apart < moved, f"{tag}: bf16 trajectory {apart:.3e} from fp32, which moved {moved:.3e}"
