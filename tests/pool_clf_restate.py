"""Restatement of the max-pool MNIST classifier (conditional_counteRGAN/mnist/modules/classifier.py:4-21) and of its fit
(countergan2.py:120-136) in plain torch on the CPU, in whatever dtype its inputs have: float64 is the truth, float32 the yardstick of
what fp32 arithmetic in another order gives.  The reference of tests/test_hip_pool_classifier.py; tests/test_pool_classifier_host.py
pins it to the reference's own recorded results (tests/golden/mnist_pool_clf_ref.npz).

Layout: everything here is NCHW, as torch has it; a pooled tensor [B, C, Hp, Wp] and its window positions (0..3 = dh * 2 + dw).  The
kernels hold NHWC: `nhwc(t)` / `nchw(t)` convert.

Routing-pinned backward.  Max-pooling is piecewise linear: where two cells of a window are within rounding of each other, an fp32 run
may route the gradient through another cell than the float64 run -- a discontinuity of the derivative, not an error of either.
`pinned_forward` therefore takes the window positions and the ReLU masks from OUTSIDE (the run under test) and computes, in its own
dtype, the forward whose derivative is exactly what such a run must produce: gather the window cell, multiply by the mask."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

KEYS = ("net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias", "net.7.weight", "net.7.bias", "net.9.weight", "net.9.bias")
SHAPES = ((32, 1, 3, 3), (32,), (64, 32, 3, 3), (64,), (128, 3136), (128,), (10, 128), (10,))
SEED = 5                                             # torch.manual_seed before the module is built: the golden file's weights


class TorchClassifier(nn.Module):
    """The layer list of modules/classifier.py:7-18 under the same attribute name: same state_dict keys, same default initialisation
    draws in the same order."""

    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(),
                                 nn.MaxPool2d(2), nn.Flatten(), nn.Linear(64 * 7 * 7, 128), nn.ReLU(), nn.Linear(128, 10))

    def forward(self, x):
        return self.net(x)


def seeded_state(seed=SEED):
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in TorchClassifier().state_dict().items()}


def cast(sd, dtype):
    return {k: v.detach().to(dtype) for k, v in sd.items()}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def windows(z):
    """[B, C, H, W] -> [B, C, H//2, W//2, 4]: the cells of every 2x2 window in row-major order (floor mode)."""
    B, C, H, W = z.shape
    Hp, Wp = H // 2, W // 2
    return z[:, :, :2 * Hp, :2 * Wp].reshape(B, C, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Hp, Wp, 4)


def relu_pool(z):
    """(p, idx) of torch's own max_pool2d(relu(z), 2, return_indices=True), its flat indices turned into 0..3 = dh * 2 + dw."""
    W = z.shape[3]
    p, flat = F.max_pool2d(torch.relu(z), 2, return_indices=True)
    h, w = flat // W, flat % W
    return p, ((h % 2) * 2 + (w % 2)).to(torch.uint8)


def top2_gap(z):
    """Top-two gap of relu(z) per window, [B, C, Hp, Wp]."""
    top = torch.sort(windows(torch.relu(z)), dim=-1).values
    return top[..., 3] - top[..., 2]


def forward(sd, x):
    """Logits and every intermediate of the eval forward: dict z1, p1, idx1, z2, p2, idx2, h, logits."""
    z1 = F.conv2d(x, sd["net.0.weight"], sd["net.0.bias"], padding=1)
    p1, idx1 = relu_pool(z1)
    z2 = F.conv2d(p1, sd["net.3.weight"], sd["net.3.bias"], padding=1)
    p2, idx2 = relu_pool(z2)
    h = torch.relu(p2.flatten(1) @ sd["net.7.weight"].T + sd["net.7.bias"])
    return dict(z1=z1, p1=p1, idx1=idx1, z2=z2, p2=p2, idx2=idx2, h=h, logits=h @ sd["net.9.weight"].T + sd["net.9.bias"])


def pinned_forward(sd, x, idx1, live1, idx2, live2, liveh):
    """Logits of the forward whose routing is given: idx* [B, C, Hp, Wp] window positions, live* the ReLU masks of the pooled cells
    (p > 0) and of fc1's output (h > 0), all taken from the run under test.  Differentiable in x and in sd's tensors."""
    dt = x.dtype
    z1 = F.conv2d(x, sd["net.0.weight"], sd["net.0.bias"], padding=1)
    p1 = windows(z1).gather(-1, idx1.long()[..., None])[..., 0] * live1.to(dt)
    z2 = F.conv2d(p1, sd["net.3.weight"], sd["net.3.bias"], padding=1)
    p2 = windows(z2).gather(-1, idx2.long()[..., None])[..., 0] * live2.to(dt)
    h = (p2.flatten(1) @ sd["net.7.weight"].T + sd["net.7.bias"]) * liveh.to(dt)
    return h @ sd["net.9.weight"].T + sd["net.9.bias"]


def input_grad(sd, x, target):
    """d/dx of CrossEntropyLoss(reduction="sum")(logits, target)."""
    x = x.detach().clone().requires_grad_(True)
    F.cross_entropy(forward(sd, x)["logits"], target, reduction="sum").backward()
    return x.grad


def adam_steps(sd, batches, lr=1e-3):
    """countergan2.py:121-136 on the batches [(x, y), ...] from state `sd`, in sd's dtype: torch.optim.Adam, mean cross-entropy.
    -> (losses, state after the last step)."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses = []
    for x, y in batches:
        loss = F.cross_entropy(forward(params, x)["logits"], y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.asarray(losses, np.float64), {k: v.detach() for k, v in params.items()}
