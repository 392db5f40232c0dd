"""torchvision's make_grid and the pixels of save_image restated in torch on the CPU, fp32, for the calls the reference makes
(torchvision is not a dependency).  Every step is one fp32 rounding:

  1. C == 1: the channel three times
  2. normalize: lo, hi = value_range or the global min and max; (clamp(x, lo, hi) - lo) / d with d = float32(max(double(hi) -
     double(lo), 1e-5)), a true fp32 division
  3. N == 1: the image itself
  4. else xmaps = min(nrow, N), ymaps = ceil(N / xmaps), cells of (H + padding) x (W + padding) behind a border of `padding`,
     filled with pad_value, image k at cell (k // xmaps, k % xmaps)
  5. save_image: uint8(clamp(g * 255 + 0.5, 0, 255)) by truncation, HWC

`pre = (a, b)`: every element is a * x + b first (two roundings), what the reference's `deltas * 0.5 + 0.5` computes."""
import math

import numpy as np
import torch


def pre_apply(t, pre=(1.0, 0.0)):
    a, b = np.float32(pre[0]), np.float32(pre[1])
    t = t.detach().to(torch.float32).cpu()
    if a == 1.0 and b == 0.0:
        return t.clone()
    return t * float(a) + float(b)                         # two fp32 tensor operations: two roundings


def image_range(t, pre=(1.0, 0.0)):
    t = pre_apply(t, pre)
    return torch.stack([t.min(), t.max()])


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, pre=(1.0, 0.0)):
    t = pre_apply(tensor, pre)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.shape[1] == 1:
        t = torch.cat((t, t, t), 1)
    if normalize:
        if value_range is not None:
            lo, hi = float(value_range[0]), float(value_range[1])
        else:
            lo, hi = float(t.min()), float(t.max())
        d = torch.tensor(max(hi - lo, 1e-5), dtype=torch.float64).to(torch.float32)
        lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
        # a full tensor of divisors: an elementwise fp32 division, never a product with a reciprocal
        t = torch.true_divide(torch.minimum(torch.maximum(t, lo32), hi32) - lo32, torch.full_like(t, float(d)))
    N, C, H, W = t.shape
    if N == 1:
        return t[0]
    xmaps = min(nrow, N)
    ymaps = int(math.ceil(N / xmaps))
    ch, cw = H + padding, W + padding
    grid = torch.full((C, ymaps * ch + padding, xmaps * cw + padding), float(pad_value), dtype=torch.float32)
    for k in range(N):
        y, x = divmod(k, xmaps)
        grid[:, y * ch + padding:y * ch + padding + H, x * cw + padding:x * cw + padding + W] = t[k]
    return grid


def to_u8(grid):
    """[C, Hg, Wg] float -> [Hg, Wg, C] uint8."""
    q = (grid * 255.0 + 0.5).clamp(0.0, 255.0)             # a product, a sum: two roundings
    return q.permute(1, 2, 0).to(torch.uint8).contiguous()


def sheet_u8(tensor, **kw):
    return to_u8(make_grid(tensor, **kw))


def cells(u8, n, nrow, H, W, padding=2):
    """The n image cells [n, H, W] of a recorded sheet [Hg, Wg, 3] (first channel)."""
    a = np.asarray(u8)
    out = np.empty((n, H, W), a.dtype)
    for k in range(n):
        y, x = divmod(k, nrow)
        out[k] = a[y * (H + padding) + padding:y * (H + padding) + padding + H, x * (W + padding) + padding:x * (W + padding) + padding + W, 0]
    return out


def padding_mask(n, nrow, H, W, padding=2):
    """True where a sheet of n cells holds padding (the unused cells of the last row too)."""
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    m = np.ones((ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), bool)
    for k in range(n):
        y, x = divmod(k, xmaps)
        m[y * (H + padding) + padding:y * (H + padding) + padding + H, x * (W + padding) + padding:x * (W + padding) + padding + W] = False
    return m
