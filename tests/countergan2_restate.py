"""Restatement of the full-resolution MNIST CounteRGAN (conditional_counteRGAN/mnist/countergan2.py:57-93) and of one iteration of its
training loop (:180-205) in plain torch on the CPU, in whatever dtype it is given: float64 is the truth, float32 the yardstick of what
fp32 arithmetic in another order gives.  The reference of tests/test_hip_countergan2.py; tests/test_countergan2_host.py pins it to the
reference's own recorded runs (tests/golden/countergan2_ref.npz).  Seeds, batches, the classifier, the digest and the float64 Adam are
tests/delta_gan_restate.py's; with `pins` (the max-pool routing and the ReLU masks of the run under test) the classifier's forward is
pool_clf_restate.pinned_forward."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_clf_restate as PR  # noqa: E402
from delta_gan_restate import (LAMBDA_CLS, LAMBDA_REG, LOSSES, LR, SEED_BATCHES, SEED_GAN, TARGET_CLASS, adam_f64, batches,  # noqa: E402,F401
                               classifier_state, digest, grads_of, make_optimizers)

EPS = 1e-6                                             # countergan2.py:188,198
G_KEYS = ("label_embed.weight", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
G_SHAPES = ((10, 784), (64, 2, 3, 3), (64,), (64, 64, 3, 3), (64,), (1, 64, 3, 3), (1,))
D_KEYS = ("label_embed.weight", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.5.weight", "net.5.bias")
D_SHAPES = ((10, 784), (64, 2, 3, 3), (64,), (64, 64, 3, 3), (64,), (1, 50176), (1,))
FORWARD = ("delta", "x_cf", "d_real", "d_fake", "d_fake_g", "cls_logits")


def _label_map(embed, c):
    return embed(c).view(-1, 1, 28, 28)


class TorchGenerator(nn.Module):
    """The layer list of countergan2.py:60-67 under the same attribute names: same state_dict keys, same default initialisation draws
    in the same order."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(64, 1, 3, padding=1))

    def forward(self, x, c):
        delta = self.net(torch.cat([x, _label_map(self.label_embed, c)], dim=1))
        return x + delta, delta


class TorchDiscriminator(nn.Module):
    """countergan2.py:79-88, likewise; returns probabilities."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.LeakyReLU(0.2), nn.Conv2d(64, 64, 3, padding=1), nn.LeakyReLU(0.2),
                                 nn.Flatten(), nn.Linear(64 * 784, 1), nn.Sigmoid())

    def forward(self, x, c):
        return self.net(torch.cat([x, _label_map(self.label_embed, c)], dim=1))


def seeded_nets(dtype=torch.float32):
    """(G, D) as the golden script builds them: torch.manual_seed(7), then Generator(), Discriminator()."""
    torch.manual_seed(SEED_GAN)
    G, D = TorchGenerator(), TorchDiscriminator()
    return G.to(dtype), D.to(dtype)


def iteration(G, D, Csd, opt_g, opt_d, x, y, target, lambda_cls=LAMBDA_CLS, lambda_reg=LAMBDA_REG, pins=None, step=True):
    """countergan2.py:180-205 in the dtype of the nets.  Returns the five losses (floats), the forward tensors delta, x_cf, d_real,
    d_fake (the D step's, :187), d_fake_g (the G step's, :195), cls_logits, and the gradients "grad_D" (after :190) and "grad_G" (after
    :204) per parameter name.  step=False leaves the parameters alone."""
    x_cf, _ = G(x, target)
    d_real = D(x, y)
    d_fake = D(x_cf.detach(), target)
    loss_D = -(torch.log(d_real + EPS) + torch.log(1 - d_fake + EPS)).mean()
    opt_d.zero_grad()
    loss_D.backward()
    grad_D = grads_of(D)
    if step:
        opt_d.step()
    x_cf, delta = G(x, target)
    d_fake_g = D(x_cf, target)
    cls_pred = PR.forward(Csd, x_cf)["logits"] if pins is None else PR.pinned_forward(Csd, x_cf, *pins)
    loss_adv = -torch.log(d_fake_g + EPS).mean()
    loss_cls = F.cross_entropy(cls_pred, target)
    loss_reg = delta.abs().mean()
    loss_G = loss_adv + lambda_cls * loss_cls + lambda_reg * loss_reg
    opt_g.zero_grad()
    loss_G.backward()
    grad_G = grads_of(G)
    if step:
        opt_g.step()
    res = {k: float(v.detach()) for k, v in (("loss_D", loss_D), ("loss_G", loss_G), ("loss_adv", loss_adv), ("loss_cls", loss_cls),
                                             ("loss_reg", loss_reg))}
    res.update(delta=delta.detach(), x_cf=x_cf.detach(), d_real=d_real.detach(), d_fake=d_fake.detach(), d_fake_g=d_fake_g.detach(),
               cls_logits=cls_pred.detach(), grad_D=grad_D, grad_G=grad_G)
    return res


def run(B, dtype, steps=3):
    """The recorded run: seeded nets and classifier, `steps` iterations on batches(B).  -> (per-step results, G, D)."""
    G, D = seeded_nets(dtype)
    Csd = classifier_state(dtype)
    opt_g, opt_d = make_optimizers(G, D)
    res = []
    for x, y in batches(B, steps):
        res.append(iteration(G, D, Csd, opt_g, opt_d, x.to(dtype), y, torch.full_like(y, TARGET_CLASS)))
    return res, G, D
