"""Test-side restatement of the moons CounteRGAN's classifier fit — conditional_counteRGAN/moons/trainer.py:13-29 — in any dtype:
the float64 oracle of tests/test_hip_moons_clf_fit.py.  A plain nn.Sequential plus torch.optim.Adam, nothing else.  Pinned to the
reference's own code by tests/test_moons_clf_fit_host.py: run in fp32 from the fixture's initial state it reproduces the losses and
the step-100 weights that tests/golden/make_golden_moons_clf.py recorded from the reference's unmodified train_classifier.

    Linear(2, 32) ReLU Linear(32, 32) ReLU Linear(32, 3);  loss = CrossEntropyLoss()(net(X), y) over all rows;  Adam(lr 1e-2)
"""
import os

import numpy as np
import torch
import torch.nn as nn

KEYS = tuple(f"net.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))
SHAPES = {"net.0.weight": (32, 2), "net.0.bias": (32,), "net.2.weight": (32, 32), "net.2.bias": (32,), "net.4.weight": (3, 32), "net.4.bias": (3,)}
LR = 1e-2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    """(the recorded fit, the moons data it ran on) as dicts of arrays."""
    return dict(np.load(os.path.join(GOLD, "moons_clf_ref.npz"))), dict(np.load(os.path.join(GOLD, "moons_cf_ref.npz")))


def gold_state(gold, k, tag="C"):
    """{key: array} of the parameters after step k (k = 0: the initial state)."""
    pre = "init.C." if k == 0 else f"it{k}.{tag}."
    return {key: gold[pre + key] for key in KEYS}


def gold_moments(gold, k):
    """({key: exp_avg}, {key: exp_avg_sq}, step) after step k of the recorded fp32 run (k = 0: a fresh optimizer)."""
    if k == 0:
        return {key: np.zeros(SHAPES[key], np.float32) for key in KEYS}, {key: np.zeros(SHAPES[key], np.float32) for key in KEYS}, 0
    return ({key: gold[f"it{k}.opt.{key}.exp_avg"] for key in KEYS}, {key: gold[f"it{k}.opt.{key}.exp_avg_sq"] for key in KEYS},
            int(gold[f"it{k}.opt.step"]))


class Fit:
    """The net, its Adam and the data in one dtype; state (parameters, moments, step counter) can be loaded before the first step."""

    def __init__(self, params, X, y, dtype=torch.float64, lr=LR, moments=None):
        torch.set_num_threads(1)
        self.dtype = dtype
        self.net = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3)).to(dtype)
        self.net.load_state_dict({k[4:]: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()})
        self.named = {"net." + k: p for k, p in self.net.named_parameters()}
        self.opt = torch.optim.Adam(self.net.parameters(), lr=lr)
        self.loss_fn = nn.CrossEntropyLoss()
        self.X, self.y = torch.tensor(np.asarray(X), dtype=dtype), torch.tensor(np.asarray(y), dtype=torch.long)
        if moments is not None:
            m, v, t = moments
            for k, p in self.named.items():
                self.opt.state[p] = {"step": torch.tensor(float(t)), "exp_avg": torch.tensor(np.asarray(m[k]), dtype=dtype).clone(),
                                     "exp_avg_sq": torch.tensor(np.asarray(v[k]), dtype=dtype).clone()}

    def step(self):
        """One iteration of trainer.py:23-25; returns the loss before the update."""
        loss = self.loss_fn(self.net(self.X), self.y)
        self.opt.zero_grad(); loss.backward(); self.opt.step()
        return float(loss.detach())

    def run(self, n):
        return np.array([self.step() for _ in range(n)])

    def eager_step(self, grads):
        """opt.step() with the given gradients {key: array}."""
        for k, p in self.named.items():
            p.grad = torch.tensor(np.asarray(grads[k]), dtype=self.dtype)
        self.opt.step()

    def grads(self):
        return {k: p.grad.detach().numpy().copy() for k, p in self.named.items()}

    def params(self):
        return {k: p.detach().numpy().copy() for k, p in self.named.items()}

    def moments(self):
        return ({k: self.opt.state[p]["exp_avg"].numpy().copy() for k, p in self.named.items()},
                {k: self.opt.state[p]["exp_avg_sq"].numpy().copy() for k, p in self.named.items()},
                int(self.opt.state[self.named[KEYS[0]]]["step"]))

    def logits(self, X):
        with torch.no_grad():
            return self.net(torch.tensor(np.asarray(X), dtype=self.dtype)).numpy()


def state_tol(ref):
    """The project's state tolerance (tests/test_hip_moons_cf.py): rtol 1e-4, atol 1e-6 + 1e-5 max|ref|."""
    return 1e-4, 1e-6 + 1e-5 * float(np.abs(ref).max())
