"""Restatement of the additive-delta MNIST CounteRGAN (conditional_counteRGAN/mnist/modules/generator.py:4-22,
modules/discriminator.py:4-23) and of one iteration of its training loop (gan_train.py:117-144) in plain torch on the CPU, in whatever
dtype it is given: float64 is the truth, float32 the yardstick of what fp32 arithmetic in another order gives.  The reference of
tests/test_hip_delta_gan*.py; tests/test_delta_gan_host.py pins it to the reference's own recorded runs
(tests/golden/delta_gan_ref.npz).  The frozen classifier is tests/pool_clf_restate.py's; with `pins` (idx1, live1, idx2, live2,
liveh: the max-pool routing and the ReLU masks of the run under test, NCHW) its forward is pool_clf_restate.pinned_forward."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_clf_restate as PR  # noqa: E402

SEED_GAN, SEED_BATCHES, TARGET_CLASS = 7, 0, 5
LAMBDA_CLS, LAMBDA_REG, LR = 3.0, 0.05, 1e-3           # gan_train.py:21-25
G_KEYS = ("label_embed.weight", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.6.weight",
          "net.6.bias")
G_SHAPES = ((10, 784), (64, 2, 3, 3), (64,), (64, 64, 3, 3), (64,), (32, 64, 3, 3), (32,), (1, 32, 3, 3), (1,))
D_KEYS = ("label_embed.weight", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.7.weight",
          "net.7.bias")
D_SHAPES = ((10, 784), (64, 2, 3, 3), (64,), (128, 64, 3, 3), (128,), (256, 128, 3, 3), (256,), (1, 12544), (1,))
LOSSES = ("loss_D", "loss_G", "loss_adv", "loss_cls", "loss_reg")


class TorchGenerator(nn.Module):
    """The layer list of modules/generator.py:7-16 under the same attribute names: same state_dict keys, same default initialisation
    draws in the same order."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, 28 * 28)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(64, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 1, 3, padding=1))

    def forward(self, x, c):
        delta = self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))
        return x + delta, delta


class TorchDiscriminator(nn.Module):
    """modules/discriminator.py:7-18, likewise."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, 28 * 28)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, stride=2, padding=1), nn.LeakyReLU(0.2), nn.Conv2d(64, 128, 3, stride=2, padding=1),
                                 nn.LeakyReLU(0.2), nn.Conv2d(128, 256, 3, stride=1, padding=1), nn.LeakyReLU(0.2), nn.Flatten(),
                                 nn.Linear(256 * 7 * 7, 1))

    def forward(self, x, c):
        return self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))


def seeded_nets(dtype=torch.float32):
    """(G, D) as the golden script builds them: torch.manual_seed(7), then Generator(), Discriminator()."""
    torch.manual_seed(SEED_GAN)
    G, D = TorchGenerator(), TorchDiscriminator()
    return G.to(dtype), D.to(dtype)


def classifier_state(dtype=torch.float32):
    return PR.cast(PR.seeded_state(PR.SEED), dtype)


def batches(B, steps=3):
    """[(x [B,1,28,28] in [-1, 1), y [B])] * steps from torch.Generator().manual_seed(0): x, then y, step after step."""
    gen = torch.Generator().manual_seed(SEED_BATCHES)
    out = []
    for _ in range(steps):
        x = 2.0 * torch.rand(B, 1, 28, 28, generator=gen) - 1.0
        out.append((x, torch.randint(0, 10, (B,), generator=gen)))
    return out


def make_optimizers(G, D, lr=LR):
    return torch.optim.Adam(G.parameters(), lr=lr), torch.optim.Adam(D.parameters(), lr=lr)


def grads_of(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def iteration(G, D, Csd, opt_g, opt_d, x, y, target, lambda_cls=LAMBDA_CLS, lambda_reg=LAMBDA_REG, pins=None, step=True):
    """gan_train.py:117-144 in the dtype of the nets.  Returns the five losses (floats), the forward tensors delta, x_cf, d_real, d_fake
    (the D step's, :124), d_fake_g (the G step's, :134), cls_logits, and the gradients "grad_D" (after :129) and "grad_G" (after
    :143) per parameter name.  step=False leaves the parameters alone (no optimizer step)."""
    bce = nn.BCEWithLogitsLoss()
    x_cf, _ = G(x, target)
    d_real = D(x, y)
    d_fake = D(x_cf.detach(), target)
    loss_D = bce(d_real, torch.ones_like(d_real)) + bce(d_fake, torch.zeros_like(d_fake))
    opt_d.zero_grad()
    loss_D.backward()
    grad_D = grads_of(D)
    if step:
        opt_d.step()
    x_cf, delta = G(x, target)
    d_fake_g = D(x_cf, target)
    if pins is None:
        cls_pred = PR.forward(Csd, x_cf)["logits"]
    else:
        cls_pred = PR.pinned_forward(Csd, x_cf, *pins)
    loss_adv = bce(d_fake_g, torch.ones_like(d_fake_g))
    loss_cls = F.cross_entropy(cls_pred, target)
    loss_reg = torch.mean(torch.abs(delta))
    loss_G = loss_adv + lambda_cls * loss_cls + lambda_reg * loss_reg
    opt_g.zero_grad()
    loss_G.backward()
    grad_G = grads_of(G)
    if step:
        opt_g.step()
    return {"loss_D": float(loss_D.detach()), "loss_G": float(loss_G.detach()), "loss_adv": float(loss_adv.detach()),
            "loss_cls": float(loss_cls.detach()), "loss_reg": float(loss_reg.detach()), "delta": delta.detach(), "x_cf": x_cf.detach(), "d_real": d_real.detach(), "d_fake": d_fake.detach(),
            "d_fake_g": d_fake_g.detach(), "cls_logits": cls_pred.detach(), "grad_D": grad_D, "grad_G": grad_G}


def run(B, dtype, steps=3):
    """The recorded run: seeded nets and classifier, `steps` iterations on batches(B).  -> (per-step results, G, D)."""
    G, D = seeded_nets(dtype)
    Csd = classifier_state(dtype)
    opt_g, opt_d = make_optimizers(G, D)
    res = []
    for x, y in batches(B, steps):
        res.append(iteration(G, D, Csd, opt_g, opt_d, x.to(dtype), y, torch.full_like(y, TARGET_CLASS)))
    return res, G, D


def digest(t, stride=97):
    """(sum, absolute sum, strided samples) of a tensor in float64: what the golden file keeps of a large tensor."""
    v = np.asarray(t.detach().double().reshape(-1).numpy())
    return np.concatenate([[v.sum(), np.abs(v).sum()], v[::stride]])


def adam_f64(p, g, m, v, t, lr=LR, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update number t (1-based) in float64 on numpy arrays: (p', m', v')."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v
