"""Test-side restatement of the moons GAN family — simple_gan/moons/make_moons_gan.py (label_dim 0) and
conditional_gan/moons/make_moons_cgan.py (label_dim 2) — for any label_dim and in any dtype: the float64 oracle of
tests/test_hip_moons_gan.py.  Pinned to the reference's own code by tests/test_moons_gan_host.py: run in fp32 it reproduces
tests/golden/moons_cgan_ref.npz (recorded from the script's lifted code by tests/golden/make_golden_moons_cgan.py) and, with
label_dim 0, tests/golden/moons_ref.npz.  oracle.moons_ref stays the definition for label_dim 0; this file only generalises it.

    G: Linear(z_dim + L, H) ReLU Linear(H, 2) on cat[z, onehot];  D: Linear(2 + L, H) ReLU Linear(H, 1) Sigmoid on cat[x, onehot]
    D step: loss_D = -mean(log D(real) + log(1 - D(G(z_d)))), Adam on D;  G step: loss_G = -mean(log D(G(z_g))), Adam on G
"""
import math

import numpy as np
import torch

SEED = 3                     # the recorded cGAN fixture (chosen for the kink precondition, see test_moons_gan_host.py)
ITERS, BATCH, Z_DIM, HIDDEN, LABEL_DIM, LR = 4, 50, 32, 128, 2, 1e-3
G_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias")
KINK_BAND = 4e-6             # |pre-activation| >= KINK_BAND * rms of its tensor (tests/test_hip_mnist_gan.py uses the same band)


def moons_data(n, seed, noise=0.05):
    """Two interleaving half circles with both labels present (the shape of sklearn's make_moons): X [n][2] float32, Y [n] int64."""
    rs = np.random.RandomState(seed)
    y = (np.arange(n) % 2).astype(np.int64)
    rs.shuffle(y)
    t = rs.uniform(0.0, math.pi, n)
    x = np.where(y == 0, np.cos(t), 1.0 - np.cos(t))
    v = np.where(y == 0, np.sin(t), 0.5 - np.sin(t))
    X = np.stack([x, v], 1) + rs.normal(scale=noise, size=(n, 2))
    return X.astype(np.float32), y


def init_params(z_dim, label_dim, hidden, seed):
    """nn.Linear's default initialisation (uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias), as float64 arrays keyed
    like the reference's state_dict without its prefix: {"G": {"0.weight": ...}, "D": {...}}."""
    rs = np.random.RandomState(seed)

    def lin(o, i):
        k = 1.0 / math.sqrt(i)
        return rs.uniform(-k, k, (o, i)), rs.uniform(-k, k, (o,))
    out = {}
    for tag, (i1, o2) in (("G", (z_dim + label_dim, 2)), ("D", (2 + label_dim, 1))):
        w1, b1 = lin(hidden, i1)
        w2, b2 = lin(o2, hidden)
        out[tag] = {"0.weight": w1, "0.bias": b1, "2.weight": w2, "2.bias": b2}
    return out


class Model:
    """Both nets and both Adam states in one dtype."""

    def __init__(self, params, dtype=torch.float64, lr=LR, betas=(0.9, 0.999), eps=1e-8):
        self.dtype, self.lr, self.betas, self.eps = dtype, lr, betas, eps
        self.p = {t: {k: torch.tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for k, v in params[t].items()} for t in ("G", "D")}
        self.m = {t: {k: torch.zeros_like(v) for k, v in self.p[t].items()} for t in ("G", "D")}
        self.v = {t: {k: torch.zeros_like(v) for k, v in self.p[t].items()} for t in ("G", "D")}
        self.t = {"G": 0, "D": 0}
        self.label_dim = self.p["D"]["0.weight"].shape[1] - 2

    def onehot(self, labels):
        if self.label_dim == 0:
            return None
        return torch.nn.functional.one_hot(torch.as_tensor(labels, dtype=torch.int64), self.label_dim).to(self.dtype)

    def hidden(self, tag, x, oh):
        p = self.p[tag]
        if oh is not None:
            x = torch.cat([x, oh], 1)
        return torch.nn.functional.linear(x, p["0.weight"], p["0.bias"])

    def G(self, z, oh, pre=None):
        a = self.hidden("G", z, oh)
        if pre is not None:
            pre.append(a.detach())
        return torch.nn.functional.linear(torch.relu(a), self.p["G"]["2.weight"], self.p["G"]["2.bias"])

    def D(self, x, oh, pre=None):
        a = self.hidden("D", x, oh)
        if pre is not None:
            pre.append(a.detach())
        return torch.sigmoid(torch.nn.functional.linear(torch.relu(a), self.p["D"]["2.weight"], self.p["D"]["2.bias"]))

    def adam(self, tag, grads):
        """torch.optim.Adam, defaults: exp_avg.lerp_(g, 1 - b1); exp_avg_sq = b2 v + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)."""
        b1, b2 = self.betas
        self.t[tag] += 1
        t = self.t[tag]
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        with torch.no_grad():
            for k, p in self.p[tag].items():
                g = grads[k]
                self.m[tag][k].lerp_(g, 1.0 - b1)
                self.v[tag][k].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                denom = (self.v[tag][k].sqrt() / math.sqrt(bc2)).add_(self.eps)
                p.addcdiv_(self.m[tag][k], denom, value=-(self.lr / bc1))

    def step(self, real, real_labels, z_d, labels_d, z_g, labels_g):
        """One iteration.  Returns {"loss_D", "loss_G" (floats), "grad_D", "grad_G" (what each optimizer consumed), "pre" (the five
        hidden pre-activation tensors: G(z_d), D(real), D(fake) of the D step; G(z_g), D(fake) of the G step)}."""
        dt = self.dtype
        real, z_d, z_g = (torch.as_tensor(a).to(dt) for a in (real, z_d, z_g))
        pre = []
        oh_d = self.onehot(labels_d)
        fake = self.G(z_d, oh_d, pre)
        D_real = self.D(real, self.onehot(real_labels), pre)
        D_fake = self.D(fake.detach(), oh_d, pre)
        loss_D = -torch.mean(torch.log(D_real) + torch.log(1 - D_fake))
        gD = dict(zip(self.p["D"], torch.autograd.grad(loss_D, list(self.p["D"].values()))))
        self.adam("D", gD)
        oh_g = self.onehot(labels_g)
        fake = self.G(z_g, oh_g, pre)
        D_fake = self.D(fake, oh_g, pre)
        loss_G = -torch.mean(torch.log(D_fake))
        gG = dict(zip(self.p["G"], torch.autograd.grad(loss_G, list(self.p["G"].values()))))
        self.adam("G", gG)
        return {"loss_D": loss_D.item(), "loss_G": loss_G.item(), "grad_D": gD, "grad_G": gG, "pre": pre}

    def state(self, tag):
        return {k: v.detach().numpy().copy() for k, v in self.p[tag].items()}


def kink_margin(pre):
    """min over the tensors of min|a| / rms(a): the kink precondition asks for >= KINK_BAND."""
    return min(float(a.abs().min() / a.pow(2).mean().sqrt()) for a in pre)


def random_case(B, H, Z, L, seed, n_rows=None, iters=1):
    """Inputs of `iters` iterations from one seed: parameters, a moons-shaped set, row indices, noise and labels."""
    n_rows = n_rows or 4 * B
    X, Y = moons_data(n_rows + (n_rows % 2), 1000 + seed)
    rs = np.random.RandomState(2000 + seed)
    return {"params": init_params(Z, L, H, 3000 + seed), "X": X, "Y": Y,
            "rows": rs.randint(0, X.shape[0], (iters, B)).astype(np.int64),
            "z": rs.normal(size=(iters, 2, B, Z)).astype(np.float32),
            "labels": rs.randint(0, max(L, 1), (iters, 2, B)).astype(np.int64)}


def run_case(case, dtype=torch.float64, lr=LR):
    """The iterations of random_case through Model: (model, [step results])."""
    m = Model(case["params"], dtype=dtype, lr=lr)
    L = m.label_dim
    outs = []
    for it in range(case["rows"].shape[0]):
        r = case["rows"][it]
        outs.append(m.step(case["X"][r], case["Y"][r] if L else None, case["z"][it, 0], case["labels"][it, 0] if L else None,
                           case["z"][it, 1], case["labels"][it, 1] if L else None))
    return m, outs


# ---- the cases of tests/test_hip_moons_gan.py; tests/test_moons_gan_host.py asserts the kink precondition for every one of them ------
# (B, H, Z, L, seed): single steps from a recorded state.  (256, 128, 32) and (50, 128, 64) need the global activation scratch.
STEP_CASES = [(50, 128, 32, 0, 1), (50, 128, 32, 2, 1), (256, 128, 32, 0, 1), (256, 128, 32, 2, 2), (7, 32, 8, 0, 1), (7, 32, 8, 2, 1),
              (50, 128, 64, 0, 1), (50, 128, 64, 2, 1)]
# (B, H, Z, L, seed, iterations): several iterations in one launch against the same in single launches, bit for bit
MULTI_CASES = [(50, 128, 32, 2, 9, 5), (50, 128, 32, 0, 12, 5), (256, 128, 32, 2, 15, 3)]
LOOP_EPOCHS, LOOP_ROWS, LOOP_BATCH = 3, 150, 50          # train_gan / moons_cgan.train with hooks: 3 epochs of 3 iterations
LOOP_SEEDS = {0: 4, 2: 7}                                # label_dim -> seed (scanned for the kink precondition, with margin)


def loop_case(L, seed=None, H=HIDDEN, Z=Z_DIM):
    """Inputs of a hooked training run: parameters, the set, one permutation per epoch and the draws of every iteration."""
    seed = LOOP_SEEDS[L] if seed is None else seed
    X, Y = moons_data(LOOP_ROWS, 4000 + seed)
    rs = np.random.RandomState(5000 + seed)
    steps = LOOP_ROWS // LOOP_BATCH
    return {"params": init_params(Z, L, H, 6000 + seed), "X": X, "Y": Y,
            "perms": [rs.permutation(LOOP_ROWS) for _ in range(LOOP_EPOCHS)],
            "z": rs.normal(size=(LOOP_EPOCHS, steps, 2, LOOP_BATCH, Z)).astype(np.float32),
            "labels": rs.randint(0, max(L, 1), (LOOP_EPOCHS, steps, 2, LOOP_BATCH)).astype(np.int64)}


def run_loop(case, dtype=torch.float64, lr=LR):
    """The epoch loop of both scripts on loop_case: cumulative re-indexing by the epoch's permutation, batches in order.
    Returns (model, loss_D_values, loss_G_values, [step results])."""
    m = Model(case["params"], dtype=dtype, lr=lr)
    L = m.label_dim
    X, Y = case["X"], case["Y"]
    lD, lG, outs = [], [], []
    for e, p in enumerate(case["perms"]):
        X, Y = X[p], Y[p]
        tD = tG = 0
        for b in range(LOOP_ROWS // LOOP_BATCH):
            sl = slice(b * LOOP_BATCH, (b + 1) * LOOP_BATCH)
            z, lab = case["z"][e, b], case["labels"][e, b]
            o = m.step(X[sl], Y[sl] if L else None, z[0], lab[0] if L else None, z[1], lab[1] if L else None)
            tD += o["loss_D"]; tG += o["loss_G"]
            outs.append(o)
        lD.append(tD); lG.append(tG)
    return m, lD, lG, outs
