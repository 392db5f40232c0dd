"""The normalised image sheets of the trainers on the device (csrc/image_sheet.hip): torchvision's `make_grid` and
`save_image` as the reference calls them (mnist_dcgan.py:190, :222; mnist_gan.py:141; gan_train.py:161-163; countergan2.py:222-224;
mnist_wgan_conditional.py:123-125, :181-182), without torchvision and without a trip of the float batch through the host.

    make_grid(t, nrow, padding, normalize, value_range, pad_value)   -> the float grid [3, Hg, Wg] on the device
    sheet_u8(t, ..., gray=False)                                     -> the uint8 image [Hg, Wg, 3] (or [Hg, Wg]) on the device
    image_range(t)                                                   -> [2] = (min, max) on the device
    save_image(t, path, ...)                                         -> one download of the uint8 image, an RGB PNG

With normalize=True and no value_range the sheet is two launches, the range pass and the sheet pass; the second reads the range from
device memory, so there is no host read between them and both can be captured in one HIP graph.  `scale_each` is not implemented
(the reference never uses it).  `pre=(a, b)` makes every element a * x + b first (two fp32 roundings): the reference's
`deltas * 0.5 + 0.5` without a pass of its own.  Pixels of a NaN input are unspecified.  There is no CPU path: a tensor that is not a
contiguous fp32 tensor on the GPU raises PcgError."""
import ctypes

import numpy as np
import torch

from . import _cfeval, _lib
from ._lib import PcgError, check
from .ops import _p, _stream

_ws_pool, _ws_of_stream = {}, {}


def _range_workspace(device):
    """The range pass's workspace for the current stream: its ticket must be zero before the FIRST launch only (every launch leaves it
    zero).  New ones come from a small pool zeroed outside any graph capture, like ops._ticket_buffer's."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_of_stream.get(key)
    if ws is None:
        n = _lib.load().pcg_image_range_workspace_bytes()
        pool = _ws_pool.setdefault(device.index, [])
        if not pool and not torch.cuda.is_current_stream_capturing():
            pool.extend(torch.zeros((8, n), dtype=torch.uint8, device=device).unbind(0))
        ws = pool.pop() if pool else torch.zeros(n, dtype=torch.uint8, device=device)
        _ws_of_stream[key] = ws
    return ws


def _images(t, who):
    if not torch.is_tensor(t):
        raise PcgError(f"{who}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise PcgError(f"{who}: the images are on {t.device}; libpcgan_hip has no CPU path")
    if t.dtype != torch.float32:
        raise PcgError(f"{who}: expected torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise PcgError(f"{who}: expected a contiguous tensor, got strides {t.stride()} for shape {tuple(t.shape)}")
    t = t.detach()
    if t.dim() == 2:                                       # make_grid: a single H x W image
        t = t.unsqueeze(0)
    if t.dim() == 3:                                       # a single C x H x W image
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] not in (1, 3) or min(t.shape) < 1:
        raise PcgError(f"{who}: expected [N, C, H, W] with C 1 or 3 and no empty dimension, got {tuple(t.shape)}")
    return t


def _pre(pre):
    a, b = (float(np.float32(v)) for v in pre)
    return a, b


def image_range(tensor, pre=(1.0, 0.0)):
    """[2] on the device: the minimum and the maximum of pre[0] * tensor + pre[1] over all elements (any shape)."""
    if not (torch.is_tensor(tensor) and tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous() and tensor.numel() >= 1):
        raise PcgError("image_range: expected a non-empty contiguous float32 tensor on the GPU (libpcgan_hip has no CPU path), got "
                       f"{getattr(tensor, 'dtype', type(tensor).__name__)} on {getattr(tensor, 'device', None)}")
    t = tensor.detach()
    a, b = _pre(pre)
    out = torch.empty(2, dtype=torch.float32, device=t.device)
    ws = _range_workspace(t.device)
    check(_lib.load().pcg_image_range(_p(t), t.numel(), a, b, _p(out), _p(ws), ws.numel(), _stream()), "pcg_image_range")
    return out


def grid_shape(N, H, W, nrow=8, padding=2):
    """(Hg, Wg) of make_grid's result for N images of H x W."""
    if N == 1:
        return H, W
    xmaps = min(int(nrow), N)
    ymaps = -(-N // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def _sheet(who, tensor, nrow, padding, normalize, value_range, pad_value, pre, want_grid, want_u8, gray):
    t = _images(tensor, who)
    N, C, H, W = t.shape
    nrow, padding = int(nrow), int(padding)
    if nrow < 1 or padding < 0:
        raise PcgError(f"{who}: nrow {nrow} must be >= 1 and padding {padding} >= 0")
    if gray and C != 1:
        raise PcgError(f"{who}: gray=True takes one-channel images, got C = {C}")
    a, b = _pre(pre)
    args = _lib.ImageSheetArgs()
    args.x, args.pad_value, args.pre_scale, args.pre_shift = t.data_ptr(), float(pad_value), a, b
    args.N, args.C, args.H, args.W, args.nrow, args.padding = N, C, H, W, nrow, padding
    args.normalize, args.gray = int(bool(normalize)), int(bool(gray))
    rng = None
    if normalize:
        if value_range is not None:
            lo, hi = (float(v) for v in value_range)
            if not lo <= hi:
                raise PcgError(f"{who}: value_range {value_range!r} is not (min, max)")
            args.lo, args.hi, args.d = lo, hi, max(hi - lo, 1e-5)          # the divisor from the two doubles, rounded once
        else:
            rng = image_range(t, pre=(a, b))
            args.range = rng.data_ptr()
    Hg, Wg = grid_shape(N, H, W, nrow, padding)
    grid = torch.empty((3, Hg, Wg), dtype=torch.float32, device=t.device) if want_grid else None
    u8 = torch.empty((Hg, Wg) if gray else (Hg, Wg, 3), dtype=torch.uint8, device=t.device) if want_u8 else None
    args.grid, args.u8 = (grid.data_ptr() if want_grid else None), (u8.data_ptr() if want_u8 else None)
    check(_lib.load().pcg_image_sheet(ctypes.byref(args), _stream()), "pcg_image_sheet")
    return grid, u8, rng


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, pre=(1.0, 0.0)):
    """torchvision.utils.make_grid of a [N, C, H, W] batch (C 1 or 3; [C, H, W] and [H, W] are one image): the float grid
    [3, Hg, Wg] on the device.  N == 1: the image itself, without padding."""
    return _sheet("make_grid", tensor, nrow, padding, normalize, value_range, pad_value, pre, True, False, False)[0]


def sheet_u8(tensor, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, pre=(1.0, 0.0), gray=False, with_grid=False,
             with_range=False):
    """The pixels save_image writes: uint8 [Hg, Wg, 3] on the device ([Hg, Wg] with gray=True and one-channel images).  with_grid:
    returns (u8, float grid) from the same launch.  with_range: the device [2] range the normalisation used is appended (None when
    it ran no range pass)."""
    grid, u8, rng = _sheet("sheet_u8", tensor, nrow, padding, normalize, value_range, pad_value, pre, bool(with_grid), True, gray)
    out = (u8,) + ((grid,) if with_grid else ()) + ((rng,) if with_range else ())
    return out if len(out) > 1 else u8


def save_image(tensor, path, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, pre=(1.0, 0.0)):
    """torchvision.utils.save_image to an 8-bit RGB PNG: the uint8 image is made on the device, downloaded (the only copy to the
    host) and written by _cfeval.write_png_rgb.  Returns the [Hg, Wg, 3] uint8 array."""
    u8 = _sheet("save_image", tensor, nrow, padding, normalize, value_range, pad_value, pre, False, True, False)[1].cpu().numpy()
    _cfeval.write_png_rgb(path, u8)
    return u8
