"""Test-side restatement of simple_gan/mnist/mnist_gan.py on the CPU, in torch.float64 (the yardstick) or torch.float32 (what the
reference itself computes): the two nets (:41-83), the loop body (:116-134) and the data the fixture run used.  The package never
imports this module.  Shared by tests/test_mnist_gan_host.py, tests/test_hip_dense_rows.py and tests/test_hip_mnist_gan.py."""
import numpy as np
import torch
import torch.nn as nn

LATENT, IMG = 100, 784
SEED = 1234
SIZES = (64, 64, 64, 64, 64, 32)          # five full batches and the 60000 % 64 tail
# Linear layers in front of a BatchNorm1d: their bias gradient is exactly 0 in exact arithmetic (BatchNorm subtracts the mean), so
# in fp32 it is rounding noise that Adam normalises into steps of order lr.  The running means contain those biases.
GRADIENT_FREE = ("model.2.bias", "model.5.bias", "model.8.bias")
INHERITS_GRADIENT_FREE = ("model.3.running_mean", "model.6.running_mean", "model.9.running_mean")
LR, BETAS = 0.0002, (0.5, 0.999)


KINK = 4e-6      # a pre-activation within KINK x rms of its tensor may land on either side of the kink in fp32 (see KinkLeaky)


class KinkLeaky(nn.Module):
    """LeakyReLU(0.2) that can be told which side of the kink a pre-activation within fp32 rounding of zero took.

    In fp32 a GEMM output carries up to 3.1e-6 of its column's scale in rounding error at K = 1024 (the FLOOR argument of
    tests/test_hip_dense_rows.py), so for |x| < KINK * rms(x) the sign, and with it the unit's derivative (1 or 0.2), depends on the
    summation order: both sides are correct fp32 results.  `queue` holds, per coming call, a boolean tensor "this run's output
    was positive"; for the near-kink elements ONLY the mask follows it, every other element keeps its own sign.  Without a queued
    entry this is nn.LeakyReLU(0.2) bit for bit.  `near` / `changed` count the elements that were near and those that were moved."""

    def __init__(self):
        super().__init__()
        self.queue, self.near, self.changed = [], 0, 0

    def forward(self, x):
        if not self.queue:
            return nn.functional.leaky_relu(x, 0.2)
        side = self.queue.pop(0)
        pos = x > 0
        near = x.detach().abs() < KINK * x.detach().pow(2).mean().sqrt()
        self.near += int(near.sum())
        self.changed += int((near & (pos != side)).sum())
        pos = torch.where(near, side, pos)
        return torch.where(pos, x, 0.2 * x)


class Net(nn.Module):
    def __init__(self, seq):
        super().__init__()
        self.model = seq

    def forward(self, x):
        return self.model(x.reshape(x.shape[0], -1))


def build(dtype=torch.float64, seed=SEED):
    """Generator and Discriminator with the reference's layer order and default initialisation: constructed in fp32 under
    torch.manual_seed(seed), generator first (as the script does, :85-86), then cast."""
    torch.manual_seed(seed)

    def block(i, o, normalize=True):
        return [nn.Linear(i, o)] + ([nn.BatchNorm1d(o, 0.8)] if normalize else []) + [KinkLeaky()]

    G = Net(nn.Sequential(*block(LATENT, 128, False), *block(128, 256), *block(256, 512), *block(512, 1024), nn.Linear(1024, IMG), nn.Tanh()))
    D = Net(nn.Sequential(nn.Linear(IMG, 512), KinkLeaky(), nn.Linear(512, 256), KinkLeaky(),
                          nn.Linear(256, 1), nn.Sigmoid()))
    return G.to(dtype), D.to(dtype)


def optimizers(G, D):
    return torch.optim.Adam(G.parameters(), lr=LR, betas=BETAS), torch.optim.Adam(D.parameters(), lr=LR, betas=BETAS)


def normalize_u8(u8):
    """ToTensor() + Normalize((0.5,), (0.5,)) (:98-101) with torchvision's two fp32 roundings."""
    return ((u8.astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)


def inputs(seed=SEED, sizes=SIZES):
    """Synthetic 8-bit images (normalised to [-1, 1] like MNIST is) and latent rows, fp32, one pair per iteration."""
    rs = np.random.RandomState(seed)
    return [(normalize_u8(rs.randint(0, 256, (n, IMG)).astype(np.uint8)), rs.normal(0.0, 1.0, (n, LATENT)).astype(np.float32)) for n in sizes]


def leakies(net):
    return [m for m in net.model if isinstance(m, KinkLeaky)]


def step(G, D, opt_g, opt_d, real, z, keep_grads=False, sides=None):
    """Loop body :116-134.  Returns dict(g_loss, d_loss, d_fake_g (D's output inside the G step), d_real, d_fake, fake[, g_grads,
    d_grads: the gradients each optimizer consumed]).
    sides: dict(g=[..], d_fake_g=[..], d_real=[..], d_fake=[..]) of boolean "output was positive" tensors per LeakyReLU of the four
    forward passes, from the run under test: its kink decisions for near-zero pre-activations (KinkLeaky)."""
    if sides is not None:
        for m, t in zip(leakies(G), sides["g"]):
            m.queue = [t]
        for j, m in enumerate(leakies(D)):
            m.queue = [sides["d_fake_g"][j], sides["d_real"][j], sides["d_fake"][j]]
    n = real.shape[0]
    ones = torch.full((n, 1), 1.0, dtype=real.dtype)
    zeros = torch.full((n, 1), 0.0, dtype=real.dtype)
    bce = nn.BCELoss()
    opt_g.zero_grad()
    fake = G(z)
    d_fake_g = D(fake)
    g_loss = bce(d_fake_g, ones)
    g_loss.backward()
    out = {}
    if keep_grads:
        out["g_grads"] = {k: p.grad.detach().clone() for k, p in G.named_parameters()}
    opt_g.step()
    opt_d.zero_grad()
    d_real = D(real)
    d_fake = D(fake.detach())
    d_loss = (bce(d_real, ones) + bce(d_fake, zeros)) / 2
    d_loss.backward()
    if keep_grads:
        out["d_grads"] = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
    opt_d.step()
    out.update(g_loss=g_loss.item(), d_loss=d_loss.item(), d_fake_g=d_fake_g.detach(), d_real=d_real.detach(), d_fake=d_fake.detach(),
               fake=fake.detach())
    return out


def digest(t):
    """fp64 sum, L2 norm and a fixed strided sample of a large tensor."""
    a = np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64).ravel()
    return np.concatenate([[a.sum(), np.sqrt((a * a).sum())], a[::max(1, a.size // 64)][:64]])


LARGE = 4096      # tensors with more elements are recorded as digests


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def np64(t):
    return t.detach().cpu().double().numpy()
