"""Tensor-level wrappers over the C ABI: PyTorch-ROCm tensors in, raw pointers across the boundary.

Activations are *physically* NHWC: tensors of shape [B, H, W, C], contiguous.  Conv weights are physically
OHWI [Cout, KH, KW, Cin] (ConvTranspose2d: [Cin, KH, KW, Cout]); `ohwi(p)` gives that view of a PyTorch
parameter of logical shape [Cout, Cin, KH, KW] kept in channels_last memory format.  Nothing here computes
on the CPU and nothing falls back to ATen kernels: every function launches kernels of libpcgan_hip.so on
torch's current HIP stream.
"""
import ctypes
import threading

import torch

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ConvGeom, check  # noqa: F401

_ws_cache = {}

# Optional per-launch timing hook (bench.py): when set, every MFMA-family conv call is bracketed by two
# torch.cuda.Event records on the current stream and reported as hook(label, flops, start_event, end_event).
_conv_hook = None


def set_conv_hook(hook):
    global _conv_hook
    _conv_hook = hook


def _conv_label(g, op):
    """Kernel the C dispatcher picks for this geometry (mirrors conv_igemm.hip / thin_conv.hip)."""
    if g.Cin <= 3 or g.Cout <= 3:
        return f"thin_{op}"
    if op == "wgrad":
        n = g.KH * g.KW * g.Cin
        if g.Cout <= 64:
            return "conv_wgrad192_kernel<64x192>" if (n % 192 == 0 and n % 128 != 0) else "conv_wgrad_kernel<64x128>"
        return "conv_wgrad_kernel<128x128>"
    n = g.Cout if op == "fwd" else g.Cin
    if n > 64:
        return f"conv_{op}_kernel<128x128>"
    swz = op == "fwd" or g.stride == 1          # three-per-CU swizzled config: forward and single-phase grad-input
    return f"conv_{op}_kernel<128x64{'/swz3' if swz else ''}>"


def _conv_flops(g):
    return 2.0 * g.B * g.OH * g.OW * g.Cout * g.KH * g.KW * g.Cin


class _Timed:
    def __init__(self, g, op):
        _conv_scratch()                      # every conv entry point passes here: the stream-K launches get their scratch
        _conv_cliptab(g)                     # ... and a k4 s2 p1 geometry its tile table (the clipped forward / grad-input launches)
        self.on = _conv_hook is not None
        if self.on:
            self.g, self.op = g, op
            self.t0 = torch.cuda.Event(enable_timing=True)
            self.t1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.on:
            self.t0.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.t1.record()
            _conv_hook(_conv_label(self.g, self.op), _conv_flops(self.g), self.t0, self.t1)
        return False


_sk_streams = {}      # (device index, stream handle) -> (parts, arrivals): scratch of the stream-K conv launches, alive for the process
_sk_pool = {}         # device index -> [(parts, arrivals), ...] spare scratch sets, allocated and zeroed OUTSIDE any capture
_sk_arrival_pool = _sk_pool      # (name kept for the tests)
_SK_SPARES = 2
_sk_last = None       # the stream key seen by the previous conv call (eager launches: skips the dictionary work)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def prepare_conv_scratch(device_index=None):
    """Keep `_SK_SPARES` spare stream-K scratch sets (64 MiB of partial tiles + zeroed arrival counters each) for the device:
    the library holds these pointers for the life of the process, so they must never come out of a graph's private pool, and
    the counters' zero-fill must never become a captured fill node.  Called when the library loads (current device) and by every
    conv call outside a capture; a conv call INSIDE a capture on a stream that has no scratch yet is served from the spares."""
    if device_index is None:
        device_index = torch.cuda.current_device()
    if torch.cuda.is_current_stream_capturing():
        return
    lib = _lib.load()
    dev = torch.device("cuda", device_index)
    nparts, narr = lib.pcg_conv_scratch_parts_bytes(), lib.pcg_conv_scratch_arrivals_bytes()
    pool = _sk_pool.setdefault(device_index, [])
    while len(pool) < _SK_SPARES:
        pool.append((torch.empty(nparts, dtype=torch.uint8, device=dev), torch.zeros(narr, dtype=torch.uint8, device=dev)))


def _conv_scratch():
    """First conv call on a stream: give the hybrid stream-K launches their scratch for it (include/pcgan_hip.h,
    pcg_conv_set_scratch).  The scratch comes from the spares of prepare_conv_scratch — never from an allocation made while a stream
    captures (r03 allocated the counters inside the capture when the pool was empty: memory of the graph's private pool handed to
    the library for the life of the process).  An empty pool under capture raises.  A stream the library has no slot left for (it
    keeps 64) simply runs the plain launches — same results up to the order of the K sum."""
    global _sk_last
    s = torch.cuda.current_stream()
    key = (s.device_index, s.cuda_stream)
    if key == _sk_last:
        return
    if key not in _sk_streams:
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            prepare_conv_scratch(s.device_index)
        pool = _sk_pool.setdefault(s.device_index, [])
        if not pool:
            raise _lib.PcgError("conv call on a new stream inside a HIP-graph capture with no spare stream-K scratch left: call "
                                "pcgan_amd.ops.prepare_conv_scratch() on this device before capturing (the scratch must not come "
                                "from the graph's private memory pool)")
        parts, arrivals = pool.pop()
        lib = _lib.load()
        if lib.pcg_conv_set_scratch(ctypes.c_void_p(s.cuda_stream), _p(parts), parts.numel(), _p(arrivals), arrivals.numel()) == 0:
            _sk_streams[key] = (parts, arrivals)
        else:
            pool.append((parts, arrivals))
            _sk_streams[key] = None
        if not capturing:
            prepare_conv_scratch(s.device_index)      # refill: the next capture stream finds a spare
    _sk_last = key


_pixtabs = {}         # (device index, IH, IW, OH, OW, stride, pad, KH, KW, Cin) -> the registered table (alive for the process), or None


def _pixtab_key(g, device_index):
    return (device_index, g.IH, g.IW, g.OH, g.OW, g.stride, g.pad, g.KH, g.KW, g.Cin)


def prepare_conv_pixtab(g, device=None):
    """Build, upload and register the pixel descriptor table of `g`'s geometry (include/pcgan_hip.h, pcg_conv_pixtab_register): the
    weight-gradient launches of that geometry then read their pixel offsets and tap masks from it.  Done by the first conv2d_wgrad
    of a geometry outside a capture — the eager warm-up step of every trainer — since the table is memory the library keeps
    pointing at: it must not come out of a graph's private pool.  Under capture an unseen geometry runs the per-k-tile loaders."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    key = _pixtab_key(g, device.index)
    if key in _pixtabs or torch.cuda.is_current_stream_capturing():
        return _pixtabs.get(key)
    lib = _lib.load()
    n = lib.pcg_conv_pixtab_bytes(ctypes.byref(g))
    host = torch.empty(n, dtype=torch.uint8)
    check(lib.pcg_conv_pixtab_register(ctypes.byref(g), _p(host), n, None), "pcg_conv_pixtab_register")
    with torch.cuda.device(device):
        tab = host.to(device)                  # a blocking copy: the table is on the device before the library hears of it
        check(lib.pcg_conv_pixtab_register(ctypes.byref(g), None, 0, _p(tab)), "pcg_conv_pixtab_register")
    _pixtabs[key] = tab
    return tab


def drop_conv_pixtab(g, device=None):
    """Forget the table of `g`'s geometry and do not build it again: its weight gradients run the per-k-tile loaders (tests)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    with torch.cuda.device(device):
        check(_lib.load().pcg_conv_pixtab_register(ctypes.byref(g), None, 0, None), "pcg_conv_pixtab_register")
    _pixtabs[_pixtab_key(g, device.index)] = None


_cliptabs = {}        # (device index, OH, OW) -> the registered tile table (alive for the process), or None: no table for the geometry


def _conv_cliptab(g):
    """Build, upload and register the tile descriptor table of `g`'s geometry (include/pcgan_hip.h, pcg_conv_cliptab_register) on its
    first use outside a capture — like the pixel table, it is memory the library keeps pointing at.  Under capture an unseen geometry
    runs the unclipped kernels."""
    if g.KH != 4 or g.stride != 2 or g.pad != 1:
        return
    key = (torch.cuda.current_device(), g.OH, g.OW)
    if key in _cliptabs or torch.cuda.is_current_stream_capturing():
        return
    lib = _lib.load()
    n = lib.pcg_conv_cliptab_bytes(ctypes.byref(g))
    tab = None
    if n:
        host = torch.empty(n, dtype=torch.uint8)
        check(lib.pcg_conv_cliptab_register(ctypes.byref(g), _p(host), n, None), "pcg_conv_cliptab_register")
        tab = host.cuda()                      # a blocking copy: the table is on the device before the library hears of it
        check(lib.pcg_conv_cliptab_register(ctypes.byref(g), None, 0, _p(tab)), "pcg_conv_cliptab_register")
    _cliptabs[key] = tab


def conv_pad_clip_query(g, op, groups=1, assume_scratch=True):
    """(taken, order, tile_rows, predicted) of pcg_conv_pad_clip_query: op 0 forward kernel, 1 grad-input kernel."""
    taken, order, rows, pred = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(1.0)
    check(_lib.load().pcg_conv_pad_clip_query(ctypes.byref(g), int(op), int(groups), int(bool(assume_scratch)), ctypes.byref(taken),
                                              ctypes.byref(order), ctypes.byref(rows), ctypes.byref(pred)), "pcg_conv_pad_clip_query")
    return bool(taken.value), order.value, rows.value, pred.value


def conv_wgrad_padskip_query(g, op=2):
    """(applies, fraction) of pcg_conv_wgrad_padskip_query: does the launch of `g` for op (2: grad-weight) have the consumers that skip
    all-padding MFMAs, and which share of the launch's MFMAs do they leave out."""
    applies, frac = ctypes.c_int32(0), ctypes.c_double(0.0)
    check(_lib.load().pcg_conv_wgrad_padskip_query(ctypes.byref(g), int(op), ctypes.byref(applies), ctypes.byref(frac)),
          "pcg_conv_wgrad_padskip_query")
    return bool(applies.value), frac.value


def conv_wgrad_padskip_plan(g, assume_scratch=True):
    """(mode, pair_bit) of pcg_conv_wgrad_padskip_plan: 0 today's kernel, 1 skipping consumers in today's block order, 2 in the paired
    order, and that order's bit."""
    mode, bit = ctypes.c_int32(-1), ctypes.c_int32(-1)
    check(_lib.load().pcg_conv_wgrad_padskip_plan(ctypes.byref(g), int(bool(assume_scratch)), ctypes.byref(mode), ctypes.byref(bit)),
          "pcg_conv_wgrad_padskip_plan")
    return mode.value, bit.value


def launch_plan(op, *args):
    """The route a non-convolution launch takes, as text (pcg_launch_plan_describe: host logic, no device).  op: one of _lib.PLAN_*;
    args: that op's integers, e.g. launch_plan(_lib.PLAN_GEMM_ACT, transA, transB, M, N, K) -> 'skinny: 33 blocks, ...'."""
    buf = ctypes.create_string_buffer(256)
    arr = (ctypes.c_int64 * max(len(args), 1))(*[int(a) for a in args])
    check(_lib.load().pcg_launch_plan_describe(int(op), arr, len(args), buf, 256), "pcg_launch_plan_describe")
    return buf.value.decode()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _chk(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.PcgError(f"{name}: expected a tensor on the GPU (libpcgan_hip has no CPU path), got {t.device}")
    if t.dtype != dtype:
        raise _lib.PcgError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PcgError(f"{name}: expected a contiguous tensor, got strides {t.stride()} for shape {tuple(t.shape)}")
    return t


_ws_retired = []   # scratch buffers that were outgrown: kept alive for the life of the process (see workspace())


def _scratch(kind, nbytes, device):
    """A cached scratch buffer per (device, HIP stream, kind), grown on demand.

    Stream-ordered use: the buffer belongs to the stream that is current at the call, so work issued on a side stream
    (GradSync.sync_then callbacks, graph capture streams) never shares scratch with the main stream.  A buffer that is outgrown
    is RETIRED, never freed: a captured HIP graph (nn.GraphedStep, house.GraphedTrainStep) has its address baked into split-K
    slabs / BatchNorm partial rows / weight-gradient slabs, and returning it to the caching allocator would let a later replay
    write into memory that meanwhile belongs to another tensor (tests/test_hip_graph.py)."""
    stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    key = (device.type, device.index, stream, kind)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def workspace(nbytes, device):
    """Scratch for the current stream (split-K slabs, BatchNorm partial rows, reductions)."""
    return _scratch(0, nbytes, device)


def workspace2(nbytes, device):
    """A second scratch buffer (slab partials of linear_wgrad), separate from `workspace` so the two never alias."""
    return _scratch(2, nbytes, device)


_ticket_pool = {}


def _ticket_buffer(device):
    """Zero-initialised ticket counters of the linear weight-gradient kernels (they leave them zero), one set per stream.
    New sets come from a small pool zeroed OUTSIDE any graph capture: a `torch.zeros` issued while a stream is capturing would
    become a fill node that replays with every launch of the graph."""
    stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    key = (device.type, device.index, stream, "tickets")
    tk = _ws_cache.get(key)
    if tk is None:
        n = _lib.load().pcg_linear_wgrad_ticket_count()
        pool = _ticket_pool.setdefault((device.type, device.index), [])
        capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if not pool and not capturing:
            pool.extend(torch.zeros((8, n), dtype=torch.int32, device=device).unbind(0))                  # setup: zeroed once
        tk = pool.pop() if pool else torch.zeros(n, dtype=torch.int32, device=device)
        _ws_cache[key] = tk
    return tk


def ohwi(w):
    """Physical [O, KH, KW, I] view of a conv parameter of logical shape [O, I, KH, KW] (channels_last memory)."""
    v = w.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise _lib.PcgError("conv weight is not in channels_last (OHWI) memory layout; FlatModule keeps it that way")
    return v


def conv_geom(B, IH, IW, Cin, Cout, KH, KW, stride, pad):
    OH = (IH + 2 * pad - KH) // stride + 1
    OW = (IW + 2 * pad - KW) // stride + 1
    return ConvGeom(B, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad)


# ---- convolution family --------------------------------------------------------------------------
class InputXform:
    """An activation that exists only as (pre-BatchNorm tensor z, folded BatchNorm coef[2][C], activation): consumers read
    act(z * coef[0][c] + coef[1][c]) inside their gathers (pcg_in_xform, include/pcgan_hip.h)."""

    def __init__(self, coef, act, slope):
        C = coef.numel() // 2
        self.coef, self.act, self.slope, self.C = coef, int(act), float(slope), C
        self.c_struct = _lib.InXform(coef.data_ptr(), coef.data_ptr() + 4 * C, int(act), float(slope))

    def ref(self):
        return ctypes.byref(self.c_struct)


def xform_ok(g, operand):
    """Can the conv kernels of geometry g take an input transform?  (MFMA path only; operand: 'x' -> Cin channels, 'dy' -> Cout.)"""
    return g.Cin > 3 and g.Cout > 3 and g.Cin % 4 == 0 and g.Cout % 4 == 0 and g.stride <= 2


class BnInput:
    """An activation that exists only as (pre-BatchNorm tensor z, the producing layer's batch statistics mean / invstd [groups][C], its
    gamma / beta, activation): a full-window one-channel convolution reads act(bn(z)) in its own loads (pcg_conv2d_*_bnin_full).  Accepted
    where an InputXform is: conv2d_fwd(xf=), conv2d_wgrad(xf_x=)."""

    def __init__(self, mean, invstd, gamma, beta, act, slope, groups=1):
        self.mean, self.invstd, self.gamma, self.beta = mean, invstd, gamma, beta
        self.act, self.slope, self.groups = int(act), float(slope), int(groups)


def bnin_full_ok(g, groups=1):
    return bool(_lib.load().pcg_conv2d_bnin_full_ok(ctypes.byref(g), int(groups)))


def xform_thin_ok(g):
    """A Cin = 1 layer whose dy-side operand may carry an input transform (pcg_conv2d_xf_thin_ok): conv2d_dgrad(xf=) / conv2d_wgrad(xf_dy=)."""
    return bool(_lib.load().pcg_conv2d_xf_thin_ok(ctypes.byref(g)))


def _xref(xf):
    return xf.ref() if xf is not None else None


def _conv2d_call(g, op, **fields):
    """Fill a pcg_conv_args (_lib.ConvArgs) from `fields` and launch it: tensors go in as their pointers, `xf` as the InputXform's
    struct, `epi` by its name in _lib.CONV_EPIS; None leaves a member zero.  The label that PCG_TRACE_OPS logs names the entry, the op
    and whatever is not default — the plain convolution, with or without an output activation, is exactly 'pcg_conv2d fwd'."""
    a = _lib.ConvArgs(op=op)
    for k, v in fields.items():
        if v is None:
            continue
        if k == "epi":
            a.epi = _lib.CONV_EPIS.index(v)
        elif k == "xf":
            a.xf = ctypes.addressof(v.c_struct)
        else:
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    label = ["pcg_conv2d", "dgrad" if op else "fwd"] + [_lib.CONV_EPIS[a.epi]] * bool(a.epi) + ["stats"] * bool(a.stats) + ["xf"] * bool(a.xf)
    check(_lib.load().pcg_conv2d(ctypes.byref(g), ctypes.byref(a), _stream()), " ".join(label + [f"g{a.groups}"] * bool(a.groups)))


def _conv2d(g, op, **fields):
    with _Timed(g, "dgrad" if op else "fwd"):
        _conv2d_call(g, op, **fields)


def _ws_fields(ws):
    return dict(workspace=ws, workspace_bytes=ws.numel() if ws is not None else 0)


def conv2d_fwd(g, x, w, bias=None, out=None, act=0, slope=0.0, xf=None):
    """y[B,OH,OW,Cout] = act(conv(x[B,IH,IW,Cin], w OHWI) (+ bias)); xf: input transform on x (InputXform)."""
    _chk(x, "x"); _chk(w, "w")
    assert x.numel() == g.B * g.IH * g.IW * g.Cin and w.numel() == g.Cout * g.KH * g.KW * g.Cin
    y = out if out is not None else torch.empty((g.B, g.OH, g.OW, g.Cout), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    need = lib.pcg_conv2d_fwd_workspace_bytes(ctypes.byref(g))
    ws = workspace(need, x.device) if need else None
    if isinstance(xf, BnInput):
        with _Timed(g, "fwd"):
            check(lib.pcg_conv2d_fwd_bnin_full(ctypes.byref(g), _p(x), _p(xf.mean), _p(xf.invstd), _p(xf.gamma), _p(xf.beta), xf.act, xf.slope,
                                               xf.groups, _p(w), _p(bias), int(act), float(slope), _p(y), _stream()), "pcg_conv2d_fwd_bnin_full")
        return y
    assert xf is None or xf.C == g.Cin
    _conv2d(g, _lib.CONV_FWD, in_=x, w=w, bias=bias, out=y, act=int(act), slope=float(slope), xf=xf, **_ws_fields(ws))
    return y


def conv2d_dgrad(g, dy, w, bias_x=None, out=None, act=0, slope=0.0, xf=None):
    """dx[B,IH,IW,Cin] = act(conv_transpose(dy[B,OH,OW,Cout], w OHWI) (+ bias_x per Cin)); xf: input transform on dy (the forward
    input of a ConvTranspose2d layer)."""
    _chk(dy, "dy"); _chk(w, "w")
    assert dy.numel() == g.B * g.OH * g.OW * g.Cout and w.numel() == g.Cout * g.KH * g.KW * g.Cin
    dx = out if out is not None else torch.empty((g.B, g.IH, g.IW, g.Cin), dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    need = lib.pcg_conv2d_dgrad_workspace_bytes(ctypes.byref(g))
    ws = workspace(need, dy.device) if need else None
    assert xf is None or xf.C == g.Cout
    _conv2d(g, _lib.CONV_DGRAD, in_=dy, w=w, bias=bias_x, out=dx, act=int(act), slope=float(slope), xf=xf, **_ws_fields(ws))
    return dx


def conv_bn_train(g, a, w, bias, transposed, eps, momentum, running_mean, running_var, num_batches_tracked, xf=None, gamma=None,
                  beta=None):
    """Convolution (transposed=False: fwd; True: dgrad = ConvTranspose2d forward) + training-mode BatchNorm statistics of
    its output.  One fused call on MFMA layers (statistics come out of the conv epilogue), two calls otherwise.
    xf: input transform on the activation operand `a`.  gamma + beta given: also return the folded scale / shift [2][C] of this
    layer's BatchNorm (written by the statistics finalize — the next consumer's transform).
    Returns (z, save_mean, save_invstd) or (z, save_mean, save_invstd, coef)."""
    _chk(a, "a"); _chk(w, "w")
    lib = _lib.load()
    C = g.Cin if transposed else g.Cout
    shape = (g.B, g.IH, g.IW, g.Cin) if transposed else (g.B, g.OH, g.OW, g.Cout)
    need = (lib.pcg_conv2d_dgrad_bn_workspace_bytes if transposed else lib.pcg_conv2d_fwd_bn_workspace_bytes)(ctypes.byref(g))
    want_coef = gamma is not None
    if need == 0:
        z = conv2d_dgrad(g, a, w, bias, xf=xf) if transposed else conv2d_fwd(g, a, w, bias, xf=xf)
        return (z,) + tuple(bn_train_stats(z, C, eps, momentum, running_mean, running_var, num_batches_tracked, gamma=gamma, beta=beta))
    z = torch.empty(shape, dtype=torch.float32, device=a.device)
    mean = torch.empty(C, dtype=torch.float32, device=a.device)
    invstd = torch.empty(C, dtype=torch.float32, device=a.device)
    coef = torch.empty(2 * C, dtype=torch.float32, device=a.device) if want_coef else None
    ws = workspace(need, a.device)
    _conv2d(g, int(transposed), in_=a, w=w, bias=bias, out=z, xf=xf, stats=1, eps=eps, momentum=momentum, save_mean=mean, save_invstd=invstd,
            running_mean=running_mean, running_var=running_var, num_batches_tracked=num_batches_tracked, gamma=gamma, beta=beta,
            coef_out=coef, **_ws_fields(ws))
    return (z, mean, invstd, coef) if want_coef else (z, mean, invstd)


def conv_bwd_data_fused(g, d, w, transposed, below_act, below_slope, a_below=None, z_below=None, bn=None):
    """Gradient w.r.t. a layer's input with the activation derivative of the layer BELOW applied in the epilogue.
    transposed=False: Conv2d (grad-input kernel); True: ConvTranspose2d (its grad-input is a forward convolution).
    z_below + bn=(mean, invstd, gamma, beta): the layer below is Conv -> BatchNorm(train) -> act; returns (dm, partial, nparts)
    for bn_bwd_partial.  a_below: the layer below is Conv -> act without BatchNorm; returns (dx_masked, None, 0).
    Returns None when the layer is not eligible (thin layers, split-K): the caller then takes the unfused path."""
    lib = _lib.load()
    if (not transposed and bn is None and a_below is not None and g.Cout <= 3
            and lib.pcg_conv2d_dgrad_mask_thin_ok(ctypes.byref(g))):       # a one-channel layer's grad-input: mask in the thin expand kernel
        _chk(d, "d"); _chk(w, "w"); _chk(a_below, "a_below")
        out = torch.empty((g.B, g.IH, g.IW, g.Cin), dtype=torch.float32, device=d.device)
        assert a_below.numel() == out.numel()
        _conv2d_call(g, _lib.CONV_DGRAD, in_=d, w=w, out=out, epi="mask", a_below=a_below, epi_act=int(below_act), epi_slope=float(below_slope))
        return out, None, 0
    if g.Cin <= 3 or g.Cout <= 3 or g.Cin % 4 or g.Cout % 4 or g.stride > 2:
        return None
    shape = (g.B, g.OH, g.OW, g.Cout) if transposed else (g.B, g.IH, g.IW, g.Cin)
    if transposed and lib.pcg_conv2d_fwd_workspace_bytes(ctypes.byref(g)) != 0:   # split-K forward: sums are incomplete per slab
        return None
    _chk(d, "d"); _chk(w, "w")
    out = torch.empty(shape, dtype=torch.float32, device=d.device)
    if bn is None:
        _chk(a_below, "a_below")
        assert a_below.numel() == out.numel()
        _conv2d(g, int(not transposed), in_=d, w=w, out=out, epi="mask", a_below=a_below, epi_act=int(below_act), epi_slope=float(below_slope))
        return out, None, 0
    _chk(z_below, "z_below")
    assert z_below.numel() == out.numel()
    mean, invstd, gamma, beta = bn
    need = (lib.pcg_conv2d_fwd_bn_workspace_bytes if transposed else lib.pcg_conv2d_dgrad_bn_workspace_bytes)(ctypes.byref(g))
    if need == 0:
        return None
    nparts = (lib.pcg_conv2d_fwd_bn_partial_rows if transposed else lib.pcg_conv2d_dgrad_bn_partial_rows)(ctypes.byref(g))
    partial = torch.empty(need // 4, dtype=torch.float32, device=d.device)   # own tensor: lives until bn_bwd_partial has read it
    _conv2d(g, int(not transposed), in_=d, w=w, out=out, epi="bnbwd", z=z_below, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
            epi_act=int(below_act), epi_slope=float(below_slope), partial=partial, partial_bytes=need)
    return out, partial, nparts


def conv_weight_adjoint(w):
    """OHWI weight of the adjoint convolution of a stride-1 layer: w[co][kh][kw][ci] -> [ci][KH-1-kh][KW-1-kw][co]."""
    _chk(w, "w")
    Cout, KH, KW, Cin = w.shape
    wa = torch.empty((Cin, KH, KW, Cout), dtype=torch.float32, device=w.device)
    check(_lib.load().pcg_conv_weight_adjoint(_p(w), _p(wa), Cout, KH, KW, Cin, _stream()), "pcg_conv_weight_adjoint")
    return wa


def conv_weight_adjoint_many(ws):
    """conv_weight_adjoint of up to 16 OHWI weights of one shape in ONE launch; returns the list of adjoint weights (views of one buffer)."""
    n = len(ws)
    Cout, KH, KW, Cin = ws[0].shape
    for w in ws:
        _chk(w, "w")
        assert tuple(w.shape) == (Cout, KH, KW, Cin)
    buf = torch.empty((n, Cin, KH, KW, Cout), dtype=torch.float32, device=ws[0].device)
    src = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    dst = (ctypes.c_void_p * n)(*[buf[i].data_ptr() for i in range(n)])
    check(_lib.load().pcg_conv_weight_adjoint_many(src, dst, n, Cout, KH, KW, Cin, _stream()), "pcg_conv_weight_adjoint_many")
    return [buf[i] for i in range(n)]


def adjoint_geom(g):
    """Geometry of the grad-input of a stride-1 convolution seen as a forward convolution of dy (see conv_weight_adjoint)."""
    assert g.stride == 1
    return conv_geom(g.B, g.OH, g.OW, g.Cout, g.Cin, g.KH, g.KW, 1, g.KH - 1 - g.pad)


def conv2d_dgrad_add_mask(g, dy, w, addend, a_below, act, slope, out=None, transposed=False):
    """dx = (conv_dgrad(dy, w) + addend) * act'(a_below) in one epilogue (out may be `addend`); transposed: the forward-kernel form."""
    _chk(dy, "dy"); _chk(w, "w"); _chk(addend, "addend"); _chk(a_below, "a_below")
    shape = (g.B, g.OH, g.OW, g.Cout) if transposed else (g.B, g.IH, g.IW, g.Cin)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    assert addend.numel() == n and a_below.numel() == n
    dx = out if out is not None else torch.empty(shape, dtype=torch.float32, device=dy.device)
    _conv2d(g, int(not transposed), in_=dy, w=w, out=dx, epi="add_mask", addend=addend, a_below=a_below, epi_act=int(act), epi_slope=float(slope))
    return dx


def conv2d_dgrad_add(g, dy, w, addend, out=None, bnsum=None, transposed=False):
    """dx = conv_dgrad(dy, w) + addend (out may be `addend`: in place) — the add of a skip connection in the grad-input epilogue.
    bnsum = (z_next, mean, invstd, scale): also leave the BatchNorm-backward column sums of scale*dx for the BatchNorm whose
    pre-normalisation output is z_next (the next one down the skip chain); returns (dx, partial, nparts) for bn_bwd_partial(dm_scale=scale).
    transposed=True: the forward-kernel form (g, w describe a forward convolution whose input is `dy`: ConvTranspose2d layers, or a
    stride-1 layer through adjoint_geom / conv_weight_adjoint).  addend=None (with bnsum only): the plain grad-input and its sums."""
    _chk(dy, "dy"); _chk(w, "w")
    shape = (g.B, g.OH, g.OW, g.Cout) if transposed else (g.B, g.IH, g.IW, g.Cin)
    if addend is None:
        assert bnsum is not None, "conv2d_dgrad_add: addend=None only together with bnsum"
    else:
        _chk(addend, "addend")
        assert addend.numel() == shape[0] * shape[1] * shape[2] * shape[3]
    dx = out if out is not None else torch.empty(shape, dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    if bnsum is not None:
        z_next, mean, invstd, scale = bnsum
        _chk(z_next, "z_next")
        assert z_next.numel() == dx.numel()
        need = (lib.pcg_conv2d_fwd_bn_workspace_bytes if transposed else lib.pcg_conv2d_dgrad_bn_workspace_bytes)(ctypes.byref(g))
        if need == 0:
            raise _lib.PcgError("conv2d_dgrad_add(bnsum=...): layer not eligible for the fused column sums")
        nparts = (lib.pcg_conv2d_fwd_bn_partial_rows if transposed else lib.pcg_conv2d_dgrad_bn_partial_rows)(ctypes.byref(g))
        partial = torch.empty(need // 4, dtype=torch.float32, device=dy.device)
        _conv2d(g, int(not transposed), in_=dy, w=w, out=dx, epi="add_bnsum", addend=addend, z=z_next, mean=mean, invstd=invstd,
                sum_scale=float(scale), partial=partial, partial_bytes=need)
        return dx, partial, nparts
    _conv2d(g, int(not transposed), in_=dy, w=w, out=dx, epi="add", addend=addend)
    return dx


def bn_bwd_partial(dm, x, C, mean, invstd, gamma, partial, nparts, dgamma, dbeta, accumulate, out=None, dcol=None, accumulate_col=False,
                   dm_scale=1.0):
    """BatchNorm backward from the column sums a fused grad-input epilogue left in `partial` (dm is already masked).
    dcol: also accumulate the column sums of the returned dx there (the bias gradient of the conv in front of the BatchNorm).
    dm_scale: the sums include this factor and the apply pass multiplies dm by it (conv2d_dgrad_add(bnsum=...))."""
    _chk(dm, "dm"); _chk(x, "x")
    rows = x.numel() // C
    dx = out if out is not None else torch.empty_like(x)
    lib = _lib.load()
    if dcol is None and dm_scale == 1.0:
        ws = workspace(lib.pcg_bn_bwd_partial_workspace_bytes(C), x.device)
        check(lib.pcg_bn_bwd_partial(_p(dm), _p(x), rows, C, _p(mean), _p(invstd), _p(gamma), _p(partial), int(nparts), _p(dx), _p(dgamma),
                                     _p(dbeta), int(bool(accumulate)), _p(ws), ws.numel(), _stream()), "pcg_bn_bwd_partial")
    else:
        ws = workspace(lib.pcg_bn_bwd_partial_db_workspace_bytes(C), x.device)
        check(lib.pcg_bn_bwd_partial_db(_p(dm), _p(x), rows, C, _p(mean), _p(invstd), _p(gamma), _p(partial), int(nparts), float(dm_scale),
                                        _p(dx), _p(dgamma), _p(dbeta), int(bool(accumulate)), _p(dcol), int(bool(accumulate_col)), _p(ws),
                                        ws.numel(), _stream()), "pcg_bn_bwd_partial_db")
    return dx


# ---- operand precision of the matrix-core convolutions (pcg_conv_precision_*) -----------------------------------
CONV_PRECISIONS = {"fp32": 0, "bf16": 1}


class conv_precision:
    """with ops.conv_precision("bf16"): ... — the implicit-GEMM convolutions launched by THIS thread inside the block round their two
    GEMM operands to bf16 (RNE) and sum the products in fp32; tensors, workspaces and epilogues stay fp32, the thin edge layers and
    every other kernel are unaffected.  The library's setting is thread-local (autograd runs a backward on its own thread: a net
    enters its own precision there too, nn.FlatModule.conv_precision).  The exit restores the previous setting, also on an exception."""

    def __init__(self, precision):
        if precision not in CONV_PRECISIONS:
            raise ValueError(f"conv_precision: {precision!r} is not one of {sorted(CONV_PRECISIONS)}")
        self.value = CONV_PRECISIONS[precision]
        self._prev = []               # a stack: the same object may be entered again while it is active (nested / recursive use)

    def __enter__(self):
        lib = _lib.load()
        self._prev.append(lib.pcg_conv_precision_get())
        check(lib.pcg_conv_precision_set(self.value), "pcg_conv_precision_set")
        return self

    def __exit__(self, et, ev, tb):
        check(_lib.load().pcg_conv_precision_set(self._prev.pop()), "pcg_conv_precision_set")
        return False


def current_conv_precision():
    """The calling thread's setting: "fp32" or "bf16"."""
    return "bf16" if _lib.load().pcg_conv_precision_get() == 1 else "fp32"


# ---- deferred slab reductions (pcg_slab_defer_*): one reduction launch per backward sweep instead of one per weight gradient -------
_slab_defer = threading.local()      # per thread, like the library's record (autograd runs a net's backward on its own thread)
_SLAB_SLOT0 = 16                      # scratch kinds 16, 17, ...: one slab buffer per deferred weight gradient of the sweep


class slab_reductions_deferred:
    """with ops.slab_reductions_deferred(): ... conv2d_wgrad calls ... — the weight gradients (dw) are complete when the block exits.
    Inside, every split-K weight gradient keeps its slabs in its own scratch slot; the exit sums all of them in one launch,
    bit-identical to the per-call reductions.  Nothing inside the block may read a dw written inside it.  Not re-entrant; on the
    current stream of the entry."""

    def __init__(self, enabled=True):
        self.enabled = enabled and not getattr(_slab_defer, "on", False)

    def __enter__(self):
        if self.enabled:
            check(_lib.load().pcg_slab_defer_begin(_stream()), "pcg_slab_defer_begin")
            _slab_defer.on, _slab_defer.n = True, 0
        return self

    def __exit__(self, et, ev, tb):
        if self.enabled:
            _slab_defer.on = False
            rc = _lib.load().pcg_slab_defer_flush(_stream())
            if et is None:
                check(rc, "pcg_slab_defer_flush")
        return False


def conv2d_wgrad(g, x, dy, dw, accumulate, xf_x=None, xf_dy=None):
    """dw (OHWI, written in place) (+)= sum over pixels of dy (x) gathered x.  xf_x / xf_dy: input transform on the operand that
    is an activation (x for Conv2d; dy for ConvTranspose2d, whose forward input sits on the dy side of the adjoint geometry)."""
    _chk(x, "x"); _chk(dy, "dy"); _chk(dw, "dw")
    assert dw.numel() == g.Cout * g.KH * g.KW * g.Cin
    lib = _lib.load()
    need = lib.pcg_conv2d_wgrad_workspace_bytes(ctypes.byref(g))
    if getattr(_slab_defer, "on", False):
        ws = _scratch(_SLAB_SLOT0 + _slab_defer.n, need, x.device)       # its own slot: the slabs live until the sweep's flush
        _slab_defer.n += 1
    else:
        ws = workspace(need, x.device)
    if g.Cin > 3 and g.Cout > 3 and _pixtab_key(g, x.device.index) not in _pixtabs:
        prepare_conv_pixtab(g, x.device)
    with _Timed(g, "wgrad"):
        if isinstance(xf_x, BnInput):
            check(lib.pcg_conv2d_wgrad_bnin_full(ctypes.byref(g), _p(x), _p(xf_x.mean), _p(xf_x.invstd), _p(xf_x.gamma), _p(xf_x.beta), xf_x.act,
                                                 xf_x.slope, xf_x.groups, _p(dy), _p(dw), int(bool(accumulate)), _p(ws), ws.numel(), _stream()),
                  "pcg_conv2d_wgrad_bnin_full")
        elif xf_x is None and xf_dy is None:
            check(lib.pcg_conv2d_wgrad(ctypes.byref(g), _p(x), _p(dy), _p(dw), int(bool(accumulate)), _p(ws), ws.numel(), _stream()),
                  "pcg_conv2d_wgrad")
        else:
            check(lib.pcg_conv2d_wgrad_xf(ctypes.byref(g), _p(x), _xref(xf_x), _p(dy), _xref(xf_dy), _p(dw), int(bool(accumulate)), _p(ws),
                                          ws.numel(), _stream()), "pcg_conv2d_wgrad_xf")
    return dw


def colsum(dy2d_rows, C, dy, db, accumulate):
    lib = _lib.load()
    need = lib.pcg_colsum_workspace_bytes(dy2d_rows, C)
    ws = workspace(need, dy.device)
    check(lib.pcg_colsum(_p(dy), dy2d_rows, C, _p(db), int(bool(accumulate)), _p(ws), ws.numel(), _stream()), "pcg_colsum")
    return db


# ---- BatchNorm + activation -------------------------------------------------------------------------
def bn_train_stats(x, C, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None, gamma=None, beta=None):
    """(save_mean, save_invstd); with gamma + beta also the folded scale / shift [2][C] (see conv_bn_train)."""
    _chk(x, "x")
    rows = x.numel() // C
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    coef = torch.empty(2 * C, dtype=torch.float32, device=x.device) if gamma is not None else None
    lib = _lib.load()
    ws = workspace(lib.pcg_bn_workspace_bytes(rows, C), x.device)
    check(lib.pcg_bn_train_stats_coef(_p(x), rows, C, eps, momentum, _p(mean), _p(invstd), _p(running_mean), _p(running_var),
                                      _p(num_batches_tracked), _p(gamma), _p(beta), _p(coef), _p(ws), ws.numel(), _stream()),
          "pcg_bn_train_stats")
    return (mean, invstd, coef) if gamma is not None else (mean, invstd)


def bn_apply_act(x, C, mean, invstd_or_var, gamma, beta, act, slope=0.0, var_eps=-1.0, out=None, residual=None, alpha=1.0):
    """y = residual + alpha * act(bn(x))  (residual None, alpha 1: plain BatchNorm + activation)."""
    _chk(x, "x")
    y = out if out is not None else torch.empty_like(x)
    check(_lib.load().pcg_bn_apply_act(_p(x), x.numel() // C, C, _p(mean), _p(invstd_or_var), var_eps, _p(gamma), _p(beta),
                                       act, slope, _p(residual), alpha, _p(y), _stream()), "pcg_bn_apply_act")
    return y


def bn_act_bwd(dy, x, y, C, mean, invstd, gamma, act, slope, dgamma, dbeta, accumulate, out=None, dy_scale=1.0, beta=None, dcol=None,
               accumulate_col=False):
    """BatchNorm(train) + activation backward.  y=None with ReLU / LeakyReLU and `beta` given: the mask is recomputed from x
    (pcg_bn_act_bwd_premask) instead of read from the saved activation.  dcol: also accumulate the column sums of the returned dx
    there (the bias gradient of the conv in front of the BatchNorm) — taken in the apply pass, no separate reduction."""
    _chk(dy, "dy"); _chk(x, "x")
    if y is not None:
        _chk(y, "y")
    rows = x.numel() // C
    dx = out if out is not None else torch.empty_like(x)
    lib = _lib.load()
    if dcol is not None:
        premask = y is None and act in (ACT_RELU, ACT_LRELU)
        if premask and beta is None:
            raise _lib.PcgError("bn_act_bwd: pass y, or beta to recompute the activation mask")
        ws = workspace(lib.pcg_bn_db_workspace_bytes(rows, C), x.device)
        check(lib.pcg_bn_act_bwd_db(_p(dy), _p(x), _p(y), rows, C, _p(mean), _p(invstd), _p(gamma), _p(beta if premask else None), act, slope,
                                    dy_scale, _p(dx), _p(dgamma), _p(dbeta), int(bool(accumulate)), _p(dcol), int(bool(accumulate_col)),
                                    _p(ws), ws.numel(), _stream()), "pcg_bn_act_bwd_db")
        return dx
    ws = workspace(lib.pcg_bn_workspace_bytes(rows, C), x.device)
    if y is None and act in (ACT_RELU, ACT_LRELU):
        if beta is None:
            raise _lib.PcgError("bn_act_bwd: pass y, or beta to recompute the activation mask")
        check(lib.pcg_bn_act_bwd_premask(_p(dy), _p(x), rows, C, _p(mean), _p(invstd), _p(gamma), _p(beta), act, slope, dy_scale, _p(dx),
                                         _p(dgamma), _p(dbeta), int(bool(accumulate)), _p(ws), ws.numel(), _stream()), "pcg_bn_act_bwd_premask")
        return dx
    check(lib.pcg_bn_act_bwd(_p(dy), _p(x), _p(y), rows, C, _p(mean), _p(invstd), _p(gamma), act, slope, dy_scale, _p(dx), _p(dgamma),
                             _p(dbeta), int(bool(accumulate)), _p(ws), ws.numel(), _stream()), "pcg_bn_act_bwd")
    return dx


def act_fwd(x, act, slope=0.0, out=None):
    _chk(x, "x")
    y = out if out is not None else torch.empty_like(x)
    check(_lib.load().pcg_act_fwd(_p(x), x.numel(), act, slope, _p(y), _stream()), "pcg_act_fwd")
    return y


def act_bwd(dy, y, act, slope=0.0, out=None):
    _chk(dy, "dy"); _chk(y, "y")
    dx = out if out is not None else torch.empty_like(dy)
    check(_lib.load().pcg_act_bwd(_p(dy), _p(y), dy.numel(), act, slope, _p(dx), _stream()), "pcg_act_bwd")
    return dx


# ---- losses -------------------------------------------------------------------------------------------
def bce_fwd_bwd(p, target, target_const, grad_scale=1.0, need_loss=True, need_grad=True, grad_out=None):
    """nn.BCELoss(mean).  Returns (loss[1] or None, dp or None).  `target` tensor or None (=> constant);
    `grad_out`: optional one-element device tensor multiplied into dp (autograd's grad_output)."""
    _chk(p, "p")
    loss = torch.empty(1, dtype=torch.float32, device=p.device) if need_loss else None
    dp = torch.empty_like(p) if need_grad else None
    check(_lib.load().pcg_bce_fwd_bwd(_p(p), _p(target), float(target_const), p.numel(), grad_scale, _p(grad_out), _p(loss),
                                      _p(dp), _stream()), "pcg_bce_fwd_bwd")
    return loss, dp


def bce_logits_fwd_bwd(z, target_const, grad_scale=1.0, need_loss=True, need_grad=True, grad_out=None):
    _chk(z, "z")
    loss = torch.empty(1, dtype=torch.float32, device=z.device) if need_loss else None
    dz = torch.empty_like(z) if need_grad else None
    check(_lib.load().pcg_bce_logits_fwd_bwd(_p(z), float(target_const), z.numel(), grad_scale, _p(grad_out), _p(loss), _p(dz),
                                             _stream()), "pcg_bce_logits_fwd_bwd")
    return loss, dz


def bce_pair(p, n_half, target0, target1, need_loss=True, need_grad=False, cotangents=(None, None, None)):
    """Two nn.BCELoss(mean) over p[:n_half] / p[n_half:] in one launch (pcg_bce_pair).  Returns (loss3 or None, dp or None);
    loss3 = [BCE(first half, target0), BCE(second half, target1), their sum].  cotangents: one-element device tensors or None."""
    _chk(p, "p")
    assert p.numel() == 2 * n_half
    loss = torch.empty(3, dtype=torch.float32, device=p.device) if need_loss else None
    dp = torch.empty_like(p) if need_grad else None
    g0, g1, g2 = cotangents
    check(_lib.load().pcg_bce_pair(_p(p), int(n_half), float(target0), float(target1), _p(g0), _p(g1), _p(g2), _p(loss), _p(dp), _stream()),
          "pcg_bce_pair")
    return loss, dp


# ---- grouped batches: G independent batches side by side along the batch axis (include/pcgan_hip.h, "grouped batches") -------------
def _fast_channels(C):
    q = C // 4
    return C % 4 == 0 and 0 < q <= 256 and (q & (q - 1)) == 0


def group_fwd_ok(g, groups):
    """Can conv_bn_train_g run geometry g (B = all groups' images) with `groups` groups?"""
    lib = _lib.load()
    return (g.B % groups == 0 and ((g.B // groups) * g.OH * g.OW) % 128 == 0 and _fast_channels(g.Cout)
            and lib.pcg_conv2d_fwd_bn_workspace_bytes(ctypes.byref(g)) > 0)


def group_dgrad_ok(g, groups):
    """Can conv_bwd_data_fused_g run the grad-input of geometry g on `groups` groups (equal phases, whole tiles per group)?"""
    if g.B % groups or g.Cin <= 3 or g.Cout <= 3 or g.Cin % 4 or g.Cout % 4 or g.stride > 2 or not _fast_channels(g.Cin):
        return False
    if _lib.load().pcg_conv2d_dgrad_bn_workspace_bytes(ctypes.byref(g)) == 0:
        return False
    s = g.stride
    if g.IH % s or g.IW % s:
        return False
    return ((g.B // groups) * (g.IH // s) * (g.IW // s)) % 128 == 0


def conv_bn_train_g(g, a, w, bias, eps, momentum, running_mean, running_var, num_batches_tracked, groups):
    """Conv2d forward over `groups` side-by-side batches + per-group training-mode BatchNorm statistics (pcg_conv_args.groups).
    Returns (z, save_mean [groups, C], save_invstd [groups, C])."""
    _chk(a, "a"); _chk(w, "w")
    lib = _lib.load()
    C = g.Cout
    need = lib.pcg_conv2d_fwd_bn_workspace_bytes(ctypes.byref(g))
    z = torch.empty((g.B, g.OH, g.OW, C), dtype=torch.float32, device=a.device)
    mean = torch.empty((groups, C), dtype=torch.float32, device=a.device)
    invstd = torch.empty((groups, C), dtype=torch.float32, device=a.device)
    ws = workspace(need, a.device)
    _conv2d(g, _lib.CONV_FWD, in_=a, w=w, bias=bias, out=z, stats=1, eps=eps, momentum=momentum, save_mean=mean, save_invstd=invstd,
            running_mean=running_mean, running_var=running_var, num_batches_tracked=num_batches_tracked, groups=int(groups), **_ws_fields(ws))
    return z, mean, invstd


def bn_apply_act_g(x, C, mean, invstd, gamma, beta, act, slope, groups, out=None):
    _chk(x, "x")
    y = out if out is not None else torch.empty_like(x)
    check(_lib.load().pcg_bn_apply_act_g(_p(x), x.numel() // C, C, _p(mean), _p(invstd), _p(gamma), _p(beta), int(act), float(slope), _p(y),
                                         int(groups), _stream()), "pcg_bn_apply_act_g")
    return y


def conv_bwd_data_fused_g(g, d, w, below_act, below_slope, z_below, bn, groups):
    """The bnbwd grad-input on `groups` side-by-side batches: returns (dm, partial, nparts, nphases) for bn_bwd_partial_g."""
    lib = _lib.load()
    _chk(d, "d"); _chk(w, "w"); _chk(z_below, "z_below")
    out = torch.empty((g.B, g.IH, g.IW, g.Cin), dtype=torch.float32, device=d.device)
    assert z_below.numel() == out.numel()
    mean, invstd, gamma, beta = bn
    need = lib.pcg_conv2d_dgrad_bn_workspace_bytes(ctypes.byref(g))
    nparts = lib.pcg_conv2d_dgrad_bn_partial_rows(ctypes.byref(g))
    nphases = lib.pcg_conv2d_dgrad_bn_phases(ctypes.byref(g))
    partial = torch.empty(need // 4, dtype=torch.float32, device=d.device)
    _conv2d(g, _lib.CONV_DGRAD, in_=d, w=w, out=out, epi="bnbwd", z=z_below, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
            epi_act=int(below_act), epi_slope=float(below_slope), partial=partial, partial_bytes=need, groups=int(groups))
    return out, partial, nparts, nphases


def bn_bwd_partial_g(dm, x, C, mean, invstd, gamma, partial, nparts, nphases, dgamma, dbeta, accumulate, groups, out=None):
    _chk(dm, "dm"); _chk(x, "x")
    dx = out if out is not None else torch.empty_like(x)
    lib = _lib.load()
    ws = workspace(lib.pcg_bn_bwd_partial_g_workspace_bytes(C, int(groups)), x.device)
    check(lib.pcg_bn_bwd_partial_g(_p(dm), _p(x), x.numel() // C, C, _p(mean), _p(invstd), _p(gamma), _p(partial), int(nparts), int(nphases),
                                   _p(dx), _p(dgamma), _p(dbeta), int(bool(accumulate)), int(groups), _p(ws), ws.numel(), _stream()),
          "pcg_bn_bwd_partial_g")
    return dx


def bn_act_bwd_g(dy, x, C, mean, invstd, gamma, beta, act, slope, dgamma, dbeta, accumulate, groups, out=None):
    """BatchNorm(train) + ReLU / LeakyReLU backward of `groups` side-by-side batches (mask recomputed from x)."""
    _chk(dy, "dy"); _chk(x, "x")
    dx = out if out is not None else torch.empty_like(x)
    lib = _lib.load()
    rows = x.numel() // C
    ws = workspace(lib.pcg_bn_act_bwd_g_workspace_bytes(rows, C, int(groups)), x.device)
    check(lib.pcg_bn_act_bwd_premask_g(_p(dy), _p(x), rows, C, _p(mean), _p(invstd), _p(gamma), _p(beta), int(act), float(slope), _p(dx),
                                       _p(dgamma), _p(dbeta), int(bool(accumulate)), int(groups), _p(ws), ws.numel(), _stream()),
          "pcg_bn_act_bwd_premask_g")
    return dx


def full_dgrad_bn_bwd_ok(g, groups=1):
    return bool(_lib.load().pcg_conv2d_dgrad_bnbwd_full_ok(ctypes.byref(g), int(groups)))


def full_dgrad_bn_bwd(g, dy, w, z_below, mean, invstd, gamma, beta, act, slope, dgamma, dbeta, accumulate, groups=1):
    """conv2d_dgrad(g, dy, w) of a full-window Cout = 1 layer pushed through the BatchNorm + activation backward of the layer below
    without being written (pcg_conv2d_dgrad_bnbwd_full).  Returns dz [B, IH, IW, Cin]; mean / invstd [groups][C]."""
    _chk(dy, "dy"); _chk(w, "w"); _chk(z_below, "z_below")
    assert z_below.numel() == g.B * g.IH * g.IW * g.Cin and dy.numel() == g.B
    dz = torch.empty_like(z_below)
    lib = _lib.load()
    ws = workspace(lib.pcg_conv2d_dgrad_bnbwd_full_workspace_bytes(ctypes.byref(g), int(groups)), dy.device)
    check(lib.pcg_conv2d_dgrad_bnbwd_full(ctypes.byref(g), _p(dy), _p(w), _p(z_below), _p(mean), _p(invstd), _p(gamma), _p(beta), int(act),
                                          float(slope), _p(dz), _p(dgamma), _p(dbeta), int(bool(accumulate)), int(groups), _p(ws), ws.numel(),
                                          _stream()), "pcg_conv2d_dgrad_bnbwd_full")
    return dz


def thin_fwd_bn_bwd_ok(g):
    return bool(_lib.load().pcg_conv2d_fwd_bnbwd_thin_ok(ctypes.byref(g)))


def thin_fwd_bn_bwd(g, x, w, z_below, mean, invstd, gamma, beta, act, slope, dgamma, dbeta, accumulate):
    """conv2d_fwd(g, x, w) with Cin = 1 taken as the gradient w.r.t. act(bn(z_below)) and pushed through that BatchNorm + activation
    backward without being written (pcg_conv2d_fwd_bnbwd_thin).  Returns dz [B, OH, OW, Cout]."""
    _chk(x, "x"); _chk(w, "w"); _chk(z_below, "z_below")
    assert z_below.numel() == g.B * g.OH * g.OW * g.Cout
    dz = torch.empty_like(z_below)
    lib = _lib.load()
    ws = workspace(lib.pcg_conv2d_fwd_bnbwd_thin_workspace_bytes(ctypes.byref(g)), x.device)
    check(lib.pcg_conv2d_fwd_bnbwd_thin(ctypes.byref(g), _p(x), _p(w), _p(z_below), _p(mean), _p(invstd), _p(gamma), _p(beta), int(act),
                                        float(slope), _p(dz), _p(dgamma), _p(dbeta), int(bool(accumulate)), _p(ws), ws.numel(), _stream()),
          "pcg_conv2d_fwd_bnbwd_thin")
    return dz


# ---- optimizer / helpers ------------------------------------------------------------------------------
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, decoupled, step):
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, n)
    check(_lib.load().pcg_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
                                    weight_decay, int(bool(decoupled)), int(step), _stream()), "pcg_adam_step")


def adam_step_capturable(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, decoupled, step_dev, hyper_dev):
    check(_lib.load().pcg_adam_step_capturable(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1, beta2,
                                               eps, weight_decay, int(bool(decoupled)), _p(step_dev), _p(hyper_dev), _stream()),
          "pcg_adam_step_capturable")


def fill(t, value):
    _chk(t, "t")
    if t.numel():
        check(_lib.load().pcg_fill(_p(t), t.numel(), float(value), _stream()), "pcg_fill")
    return t


def add_bias_rows(x, C, bias):
    """x[..., c] += bias[c] in place."""
    _chk(x, "x"); _chk(bias, "bias")
    check(_lib.load().pcg_add_bias_rows(_p(x), x.numel() // C, C, _p(bias), _stream()), "pcg_add_bias_rows")
    return x


def sumsq(t, out, accumulate=False):
    _chk(t, "t")
    check(_lib.load().pcg_sumsq(_p(t), t.numel(), _p(out), int(bool(accumulate)), _stream()), "pcg_sumsq")
    return out


# ---- CounteRGAN pieces ---------------------------------------------------------------------------------------
def norm_sum(flat, seg, out=None):
    """out[0] = sum_s ||flat[seg[s,0] : seg[s,0] + seg[s,1]]||_2 (seg: int64 [n, 2] on the device) in one launch."""
    _chk(flat, "flat"); _chk(seg, "seg", torch.int64)
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=flat.device)
    check(_lib.load().pcg_norm_sum(_p(flat), _p(seg), seg.shape[0], _p(out), _stream()), "pcg_norm_sum")
    return out


def _chk_idx(idx, K, name="idx"):
    if idx.dtype != torch.int64 or not idx.is_cuda or not idx.is_contiguous():
        raise _lib.PcgError(f"{name}: expected a contiguous int64 tensor on the GPU")
    return idx


def embed_concat_fwd(x, idx, table, mask):
    """[B,H,W,C] with channels (x, table[idx], [mask]); x, mask: [B,1,H,W] or [B,H,W]; table: [K, H*W]."""
    _chk(x, "x"); _chk(table, "table"); _chk_idx(idx, table.shape[0])
    B, HW = idx.numel(), table.shape[1]
    C = 3 if mask is not None else 2
    out = torch.empty((B, HW, C), dtype=torch.float32, device=x.device)
    check(_lib.load().pcg_embed_concat_fwd(_p(x), _p(idx), _p(table), _p(mask), _p(out), B, HW, C, table.shape[0], _stream()),
          "pcg_embed_concat_fwd")
    return out


def embed_concat_bwd(dinp, idx, C, K, dtable=None, accumulate=False, need_dx=False):
    _chk(dinp, "dinp")
    B = idx.numel()
    HW = dinp.numel() // (B * C)
    dx = torch.empty((B, HW), dtype=torch.float32, device=dinp.device) if need_dx else None
    check(_lib.load().pcg_embed_concat_bwd(_p(dinp), _p(idx), _p(dtable), _p(dx), B, HW, C, K, int(bool(accumulate)), _stream()),
          "pcg_embed_concat_bwd")
    return dx


def embed_table_grad(dinp, idx, C, ch, K, dtable, accumulate=False):
    """dtable[k][p] (+)= sum over the rows b with idx[b] == k of dinp[b][p][ch] (dinp: [B, HW, C])."""
    _chk(dinp, "dinp"); _chk(dtable, "dtable")
    B = idx.numel()
    HW = dinp.numel() // (B * C)
    check(_lib.load().pcg_embed_table_grad(_p(dinp), _p(idx), _p(dtable), B, HW, C, int(ch), K, int(bool(accumulate)), _stream()),
          "pcg_embed_table_grad")


def gather_channel(t, ch):
    """[..., C] -> [..., 1]: channel `ch` of the last axis as a contiguous tensor (one tiny launch)."""
    _chk(t, "t")
    C = t.shape[-1]
    out = torch.empty(t.shape[:-1] + (1,), dtype=torch.float32, device=t.device)
    check(_lib.load().pcg_gather_channel(_p(t), _p(out), t.numel() // C, C, int(ch), _stream()), "pcg_gather_channel")
    return out


def axpby(a, x, b=0.0, y=None, out=None):
    _chk(x, "x")
    out = out if out is not None else torch.empty_like(x)
    check(_lib.load().pcg_axpby(_p(out), float(a), _p(x), float(b), _p(y), x.numel(), _stream()), "pcg_axpby")
    return out


def scale_mask_fwd(c, mask, scale):
    _chk(c, "c")
    raw, masked = torch.empty_like(c), torch.empty_like(c)
    check(_lib.load().pcg_scale_mask_fwd(_p(c), _p(mask), float(scale), _p(raw), _p(masked), c.numel(), _stream()), "pcg_scale_mask_fwd")
    return raw, masked


def scale_mask_bwd(d_raw, d_masked, mask, scale, like):
    dc = torch.empty_like(like)
    check(_lib.load().pcg_scale_mask_bwd(_p(d_raw), _p(d_masked), _p(mask), float(scale), _p(dc), like.numel(), _stream()),
          "pcg_scale_mask_bwd")
    return dc


def clamp_add_fwd(x, r, lo, hi):
    _chk(x, "x"); _chk(r, "r")
    y = torch.empty_like(x)
    check(_lib.load().pcg_clamp_add_fwd(_p(x), _p(r), float(lo), float(hi), _p(y), x.numel(), _stream()), "pcg_clamp_add_fwd")
    return y


def clamp_add_bwd(dy, x, r, lo, hi):
    _chk(dy, "dy")
    dr = torch.empty_like(x)
    check(_lib.load().pcg_clamp_add_bwd(_p(dy), _p(x), _p(r), float(lo), float(hi), _p(dr), x.numel(), _stream()), "pcg_clamp_add_bwd")
    return dr


def abs_mean_fwd(a, m=None, one_minus=False):
    _chk(a, "a")
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = workspace(lib.pcg_abs_mean_workspace_bytes(), a.device)
    check(lib.pcg_abs_mean_fwd(_p(a), _p(m), int(bool(one_minus)), a.numel(), _p(out), _p(ws), ws.numel(), _stream()), "pcg_abs_mean_fwd")
    return out


def abs_mean_bwd(a, m, one_minus, grad_out, scale=1.0, out=None, accumulate=False):
    da = out if out is not None else torch.empty_like(a)
    check(_lib.load().pcg_abs_mean_bwd(_p(a), _p(m), int(bool(one_minus)), a.numel(), _p(grad_out), float(scale), _p(da),
                                       int(bool(accumulate)), _stream()), "pcg_abs_mean_bwd")
    return da


def avgpool_fwd(x, B, HW, C):
    _chk(x, "x")
    y = torch.empty((B, C), dtype=torch.float32, device=x.device)
    check(_lib.load().pcg_avgpool_fwd(_p(x), _p(y), B, HW, C, _stream()), "pcg_avgpool_fwd")
    return y


def avgpool_bwd(dy, B, HW, C):
    _chk(dy, "dy")
    dx = torch.empty((B, HW, C), dtype=torch.float32, device=dy.device)
    check(_lib.load().pcg_avgpool_bwd(_p(dy), _p(dx), B, HW, C, _stream()), "pcg_avgpool_bwd")
    return dx


def cross_entropy_fwd_bwd(logits, target, need_loss=True, need_grad=True, grad_out=None, grad_scale=1.0, loss_out=None):
    _chk(logits, "logits"); _chk_idx(target, logits.shape[-1], "target")
    B, K = logits.shape
    loss = (loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logits.device)) if need_loss else None
    dz = torch.empty_like(logits) if need_grad else None
    check(_lib.load().pcg_cross_entropy_fwd_bwd(_p(logits), _p(target), B, K, float(grad_scale), _p(grad_out), _p(loss), _p(dz),
                                                _stream()), "pcg_cross_entropy_fwd_bwd")
    return loss, dz


# ---- tabular CounteRGAN building blocks (csrc/tabular.hip) ----------------------------------------------------------------
def gemm(A, B, M, N, K, transA=False, transB=False, lda=None, ldb=None, out=None, ldc=None, bias=None, accumulate=False, act=0, slope=0.0):
    """out[M][N] (+)= opA . opB (+ bias); A/B/out may be column slices of wider row-major buffers (ld* = row stride)."""
    for t, n in ((A, "A"), (B, "B")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.PcgError(f"gemm: {n} must be an fp32 tensor on the GPU")
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    ldc = ldc if ldc is not None else N
    check(_lib.load().pcg_gemm_act(int(transA), int(transB), M, N, K, _p(A), lda, _p(B), ldb, _p(out), ldc, _p(bias), int(bool(accumulate)),
                                   int(act), float(slope), _stream()), "pcg_gemm_act")
    return out


def linear_wgrad(dy, x, B, O, I, dW, db=None, ldy=None, ldx=None, accumulate_w=False, accumulate_b=False):
    """dW[O][I] (+)= dy^T x and db[O] (+)= colsum(dy) in one launch (deterministic slab split over the batch)."""
    lib = _lib.load()
    dev = x.device
    tk = _ticket_buffer(dev)
    nbytes = lib.pcg_linear_wgrad_workspace_bytes(B, O, I)
    ws = workspace2(nbytes, dev) if nbytes else None
    check(lib.pcg_linear_wgrad(_p(dy), ldy if ldy is not None else O, _p(x), ldx if ldx is not None else I, B, O, I, _p(dW), _p(db),
                               int(bool(accumulate_w)), int(bool(accumulate_b)), _p(ws), nbytes, _p(tk), _stream()), "pcg_linear_wgrad")


# ---- whole-batch dense layers, at most 128 rows (csrc/dense_rows.hip) ----------------------------------------------
class DenseBN:
    """The BatchNorm1d operands of dense_rows_fwd: parameters, buffers, and the tensors the launch leaves for the backward."""

    def __init__(self, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum=0.1, training=True, save_mean=None,
                 save_invstd=None, xhat=None):
        self.gamma, self.beta, self.running_mean, self.running_var, self.num_batches_tracked = gamma, beta, running_mean, running_var, num_batches_tracked
        self.eps, self.momentum, self.training = float(eps), float(momentum), bool(training)
        self.save_mean, self.save_invstd, self.xhat = save_mean, save_invstd, xhat


def dense_rows_fwd(x, w, bias=None, act=_lib.ACT_NONE, slope=0.0, bn=None, out=None):
    """y[R][O] = act(BN(x[R][I] w^T + bias)) in one launch, R <= 128 (pcg_dense_rows_fwd).  bn: a DenseBN; in training mode its
    save_mean / save_invstd / xhat are allocated here when absent and filled by the launch."""
    _chk(x, "x"); _chk(w, "w")
    R, I = x.shape
    O = w.shape[0]
    if w.shape[1] != I:
        raise _lib.PcgError(f"dense_rows_fwd: x has {I} features, the weight takes {w.shape[1]}")
    y = out if out is not None else torch.empty((R, O), dtype=torch.float32, device=x.device)
    _chk(y, "out")
    ref = None
    if bn is not None:
        if bn.training:
            if bn.save_mean is None:
                bn.save_mean = torch.empty(O, dtype=torch.float32, device=x.device)
            if bn.save_invstd is None:
                bn.save_invstd = torch.empty(O, dtype=torch.float32, device=x.device)
            if bn.xhat is None:
                bn.xhat = torch.empty((R, O), dtype=torch.float32, device=x.device)
        nbt = bn.num_batches_tracked if bn.training else None
        if nbt is not None and nbt.dtype != torch.int64:
            raise _lib.PcgError(f"dense_rows_fwd: num_batches_tracked must be int64, got {nbt.dtype}")
        tr = bn.training
        ref = ctypes.byref(_lib.DenseBn(_p(bn.gamma), _p(bn.beta), _p(bn.running_mean), _p(bn.running_var), _p(nbt), _p(bn.save_mean if tr else None),
                                        _p(bn.save_invstd if tr else None), _p(bn.xhat if tr else None), bn.eps, bn.momentum, int(tr)))
    check(_lib.load().pcg_dense_rows_fwd(_p(x), _p(w), _p(bias), R, I, O, ref, int(act), float(slope), _p(y), _stream()), "pcg_dense_rows_fwd")
    return y


def dense_rows_dgrad(dz, w, below_act=_lib.ACT_NONE, below_slope=0.0, y_below=None, bn=None, out=None):
    """dx = (dz[R][O] w[O][I]) * act'(y_below), then the BatchNorm1d backward of the layer below when bn = (xhat, gamma, invstd,
    dgamma, dbeta, accumulate) is given, in one launch (pcg_dense_rows_dgrad).  No activation and no bn: plain dx = dz w."""
    _chk(dz, "dz"); _chk(w, "w")
    R, O = dz.shape
    I = w.shape[1]
    if w.shape[0] != O:
        raise _lib.PcgError(f"dense_rows_dgrad: dz has {O} features, the weight has {w.shape[0]} rows")
    dx = out if out is not None else torch.empty((R, I), dtype=torch.float32, device=dz.device)
    _chk(dx, "out")
    if y_below is not None:
        _chk(y_below, "y_below")
    ref = None
    if bn is not None:
        xhat, gamma, invstd, dgamma, dbeta, acc = bn
        ref = ctypes.byref(_lib.DenseBnBwd(_p(_chk(xhat, "xhat")), _p(gamma), _p(invstd), _p(dgamma), _p(dbeta), int(bool(acc))))
    check(_lib.load().pcg_dense_rows_dgrad(_p(dz), _p(w), R, O, I, int(below_act), float(below_slope), _p(y_below), ref, _p(dx), _stream()),
          "pcg_dense_rows_dgrad")
    return dx


def dense_rows_wgrad(dz, x, dW, db=None, accumulate=False):
    """dW[O][I] (+)= dz^T x, db[O] (+)= column sums of dz over all R <= 128 rows in one launch (pcg_dense_rows_wgrad)."""
    _chk(dz, "dz"); _chk(x, "x"); _chk(dW, "dW")
    R, O = dz.shape
    I = x.shape[1]
    if x.shape[0] != R or tuple(dW.shape) != (O, I):
        raise _lib.PcgError(f"dense_rows_wgrad: dz {tuple(dz.shape)}, x {tuple(x.shape)}, dW {tuple(dW.shape)} do not agree")
    check(_lib.load().pcg_dense_rows_wgrad(_p(dz), _p(x), R, O, I, _p(dW), _p(db), int(bool(accumulate)), _stream()), "pcg_dense_rows_wgrad")
    return dW


def dense_rows_fwd_post(x, w, bias, bn, act=_lib.ACT_LRELU, slope=0.0, mask=None, p=0.0, a=None, out=None):
    """y = Dropout(BN_train(act(x[R][I] w^T + bias))) in one launch, 2 <= R <= 128 (pcg_dense_rows_fwd_post): the post-activation
    stage of the tabular classifier.  bn: a DenseBN in training mode; its save_mean / save_invstd are allocated here when absent.
    mask [R][O] of 0/1 (None: no Dropout), p the Dropout probability.  Returns (y, a): a = act(z) is all the backward needs."""
    _chk(x, "x"); _chk(w, "w")
    R, I = x.shape
    O = w.shape[0]
    if w.shape[1] != I:
        raise _lib.PcgError(f"dense_rows_fwd_post: x has {I} features, the weight takes {w.shape[1]}")
    if bn is None or not bn.training:
        raise _lib.PcgError("dense_rows_fwd_post: training-mode BatchNorm only (evaluation folds it into the next Linear)")
    dev = x.device
    y = out if out is not None else torch.empty((R, O), dtype=torch.float32, device=dev)
    a = a if a is not None else torch.empty((R, O), dtype=torch.float32, device=dev)
    _chk(y, "out"); _chk(a, "a")
    if tuple(y.shape) != (R, O) or tuple(a.shape) != (R, O) or (mask is not None and tuple(_chk(mask, "mask").shape) != (R, O)):
        raise _lib.PcgError(f"dense_rows_fwd_post: out, a and mask must be [{R}, {O}]")
    if bn.save_mean is None:
        bn.save_mean = torch.empty(O, dtype=torch.float32, device=dev)
    if bn.save_invstd is None:
        bn.save_invstd = torch.empty(O, dtype=torch.float32, device=dev)
    nbt = bn.num_batches_tracked
    if nbt is not None and nbt.dtype != torch.int64:
        raise _lib.PcgError(f"dense_rows_fwd_post: num_batches_tracked must be int64, got {nbt.dtype}")
    check(_lib.load().pcg_dense_rows_fwd_post(_p(x), _p(w), _p(bias), R, I, O, int(act), float(slope), _p(bn.gamma), _p(bn.beta),
                                              _p(bn.running_mean), _p(bn.running_var), _p(nbt), bn.eps, bn.momentum, _p(mask),
                                              1.0 / (1.0 - p), _p(a), _p(bn.save_mean), _p(bn.save_invstd), _p(y), _stream()),
          "pcg_dense_rows_fwd_post")
    return y, a


def dense_rows_dgrad_post(dz, w, a, mean, invstd, gamma, dgamma, dbeta, act=_lib.ACT_LRELU, slope=0.0, mask=None, p=0.0, accumulate=False,
                          out=None, db=None):
    """dx = the whole backward of the post-activation stage below (Dropout, BatchNorm1d, activation, in this order) applied to
    dz[R][O] w[O][I], in one launch (pcg_dense_rows_dgrad_post); a, mean, invstd as dense_rows_fwd_post left them; dgamma / dbeta are
    written (accumulate: added to); db ([I], optional): so is the column sum of dx, the bias gradient of the stage's Linear."""
    _chk(dz, "dz"); _chk(w, "w")
    R, O = dz.shape
    I = w.shape[1]
    if w.shape[0] != O:
        raise _lib.PcgError(f"dense_rows_dgrad_post: dz has {O} features, the weight has {w.shape[0]} rows")
    dx = out if out is not None else torch.empty((R, I), dtype=torch.float32, device=dz.device)
    _chk(dx, "out")
    if tuple(dx.shape) != (R, I) or (a is not None and tuple(_chk(a, "a").shape) != (R, I)) or \
            (mask is not None and tuple(_chk(mask, "mask").shape) != (R, I)):
        raise _lib.PcgError(f"dense_rows_dgrad_post: out, a and mask must be [{R}, {I}]")
    for t, name in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta"), (db, "db")):
        if t is not None and (_chk(t, name).numel() != I):
            raise _lib.PcgError(f"dense_rows_dgrad_post: {name} must have {I} entries")
    check(_lib.load().pcg_dense_rows_dgrad_post(_p(dz), _p(w), R, O, I, _p(mask), 1.0 / (1.0 - p), _p(a), _p(mean), _p(invstd), _p(gamma),
                                                int(act), float(slope), _p(dgamma), _p(dbeta), _p(db), int(bool(accumulate)), _p(dx), _stream()),
          "pcg_dense_rows_dgrad_post")
    return dx


def linear_wgrad_grouped(items, B, device):
    """items: list of (dy, x, O, I, dW, db or None, ldy, ldx, accumulate_w, accumulate_b) — layers that reduce over the same B rows,
    all in one launch (the library tiles them for the matrix cores)."""
    lib = _lib.load()
    n = len(items)
    arr = (_lib.WgradItem * n)()
    for k, (dy, x, O, I, dW, db, ldy, ldx, aw, ab) in enumerate(items):
        arr[k].dy, arr[k].x, arr[k].dW, arr[k].db = dy.data_ptr(), x.data_ptr(), dW.data_ptr(), (db.data_ptr() if db is not None else None)
        arr[k].ldy, arr[k].ldx, arr[k].O, arr[k].I = ldy, ldx, O, I
        arr[k].accumulate_w, arr[k].accumulate_b = int(bool(aw)), int(bool(ab))
        arr[k].tile_x, arr[k].tile_y = 0, 0
    tk = _ticket_buffer(device)
    nbytes = lib.pcg_linear_wgrad_grouped_workspace_bytes(B, arr, n)
    ws = workspace2(nbytes, device)
    check(lib.pcg_linear_wgrad_grouped(arr, n, B, _p(ws), nbytes, _p(tk), _stream()), "pcg_linear_wgrad_grouped")


def onehot(idx, K, out=None):
    _chk_idx(idx, K)
    if out is None:
        out = torch.empty((idx.numel(), K), dtype=torch.float32, device=idx.device)
    check(_lib.load().pcg_onehot(_p(idx), idx.numel(), K, _p(out), _stream()), "pcg_onehot")
    return out


def concat_cols(a, b):
    _chk(a, "a"); _chk(b, "b")
    rows = a.shape[0]
    out = torch.empty((rows, a.shape[1] + b.shape[1]), dtype=torch.float32, device=a.device)
    check(_lib.load().pcg_concat_cols(_p(a), a.shape[1], _p(b), b.shape[1], rows, _p(out), _stream()), "pcg_concat_cols")
    return out


def split_cols(d, ca, cb, need_a=True, need_b=True):
    _chk(d, "d")
    rows = d.shape[0]
    da = torch.empty((rows, ca), dtype=torch.float32, device=d.device) if need_a else None
    db = torch.empty((rows, cb), dtype=torch.float32, device=d.device) if need_b else None
    check(_lib.load().pcg_split_cols(_p(d), ca, cb, rows, _p(da), _p(db), _stream()), "pcg_split_cols")
    return da, db


def film_fwd(g, h, b):
    _chk(g, "gamma"); _chk(h, "h"); _chk(b, "beta")
    y = torch.empty_like(h)
    check(_lib.load().pcg_film_fwd(_p(g), _p(h), _p(b), _p(y), h.numel(), _stream()), "pcg_film_fwd")
    return y


def film_bwd(dy, g, h):
    _chk(dy, "dy")
    dg, dh = torch.empty_like(h), torch.empty_like(h)
    check(_lib.load().pcg_film_bwd(_p(dy), _p(g), _p(h), _p(dg), _p(dh), h.numel(), _stream()), "pcg_film_bwd")
    return dg, dh


def gumbel_softmax_fwd(logits, noise, seg_offsets, tau, hard=False):
    """(y_soft, y_hard or None)"""
    _chk(logits, "logits"); _chk(noise, "noise"); _chk(seg_offsets, "seg_offsets", torch.int32)
    B, T = logits.shape
    y = torch.empty_like(logits)
    yh = torch.empty_like(logits) if hard else None
    check(_lib.load().pcg_gumbel_softmax_fwd(_p(logits), _p(noise), _p(seg_offsets), seg_offsets.numel() - 1, T, B, float(tau), _p(y),
                                             _p(yh), _stream()), "pcg_gumbel_softmax_fwd")
    return y, yh


def gumbel_softmax_bwd(dy, y, seg_offsets, tau):
    _chk(dy, "dy")
    B, T = y.shape
    dl = torch.empty_like(y)
    check(_lib.load().pcg_gumbel_softmax_bwd(_p(dy), _p(y), _p(seg_offsets), seg_offsets.numel() - 1, T, B, float(tau), _p(dl),
                                             _stream()), "pcg_gumbel_softmax_bwd")
    return dl


def assemble_residual_fwd(cont, cont_idx, samples, seg_offsets, cat_idx, norm_vals, x):
    _chk(cont, "cont"); _chk(samples, "samples"); _chk(x, "x"); _chk(norm_vals, "norm_vals")
    B, D = x.shape
    res = torch.empty_like(x)
    check(_lib.load().pcg_assemble_residual_fwd(_p(cont), cont.shape[1], _p(cont_idx), _p(samples), _p(seg_offsets), cat_idx.numel(),
                                                samples.shape[1], _p(cat_idx), _p(norm_vals), _p(x), D, B, _p(res), _stream()),
          "pcg_assemble_residual_fwd")
    return res


def house_residual_fwd(cont, samples, seg_offsets, norm_vals, x, mask, col_src, sn=None):
    """(residual_full, masked_residual, x_cf, mask_penalty, am) of the tabular step in one launch: assemble_residual_fwd +
    scale_mask_fwd + axpby + 2 x abs_mean_fwd, bit for bit.  col_src: host list, per feature column the continuous index (>= 0) or
    -(head + 1).  sn: a training-mode batch of sn_fwd_batch — that spectral normalisation rides in the same launch (the two do not
    depend on each other); its outputs are appended to the returned tuple."""
    _chk(cont, "cont"); _chk(samples, "samples"); _chk(x, "x"); _chk(mask, "mask"); _chk(norm_vals, "norm_vals")
    B, D = x.shape
    res, masked, x_cf = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    scal = torch.empty(2, dtype=torch.float32, device=x.device)
    part = torch.empty(512, dtype=torch.float32, device=x.device)
    tk = _ticket_buffer(x.device)
    a = _lib.HouseResFwdArgs(cont=cont.data_ptr(), ncont=cont.shape[1], samples=samples.data_ptr(), seg_dev=seg_offsets.data_ptr(),
                             T=samples.shape[1], norm=norm_vals.data_ptr(), x=x.data_ptr(), mask=mask.data_ptr(),
                             col_src=(ctypes.c_int32 * D)(*[int(v) for v in col_src]), D=D, B=B, res=res.data_ptr(), masked=masked.data_ptr(),
                             x_cf=x_cf.data_ptr(), partial512=part.data_ptr(), ticket=tk.data_ptr() + 4 * 1024, pen_out=scal.data_ptr(),
                             am_out=scal.data_ptr() + 4)
    check(_lib.load().pcg_house_residual_fwd(a, sn, _stream()), "pcg_house_residual_fwd")
    return (res, masked, x_cf, scal[0], scal[1]) + (() if sn is None else (sn.outputs,))


def _diag_args(logits_cf, logits_orig, src_rows, target_y, masked, eps, out4, acc, who):
    _chk(logits_cf, "logits_cf"); _chk(logits_orig, "logits_orig"); _chk(masked, "masked"); _chk(target_y, "target_y", torch.int64)
    B, nc = logits_cf.shape
    if src_rows is not None:
        _chk(src_rows, "src_rows", torch.int64)
    elif logits_orig.shape[0] < B:
        raise _lib.PcgError(f"{who}: logits_orig has fewer rows than the batch and no src_rows were given")
    if acc is not None:
        _chk(acc, "acc", torch.float64)
        assert acc.numel() >= 8
    assert masked.shape[0] == B and logits_orig.shape[1] == nc and target_y.numel() == B
    return _lib.HouseDiagArgs(logits_cf=logits_cf.data_ptr(), logits_orig=logits_orig.data_ptr(), src_rows=_p(src_rows),
                              target_y=target_y.data_ptr(), masked=masked.data_ptr(), B=B, nc=nc, D=masked.shape[1], eps=float(eps),
                              out4=out4.data_ptr(), acc=_p(acc))


def house_residual_bwd(res, masked, mask, gx_a, gx_b, w_pen, w_am, ncont, cont_idx, seg_offsets, T, cat_idx, norm_vals, losses=None, diag=None):
    """(d_cont, d_samples): the tabular step's backward from dLoss/dx_cf = gx_a + gx_b and the two penalty weights down to the
    generator's outputs, in one launch (see pcg_house_residual_bwd).  losses = (d_real, d_fake, d_fake_g, g_cls, am, pen, lambda_cls,
    w_reg, lambda_mask, w_reg_log): pcg_house_losses rides in the same launch; its scalars (six floats: the five of pcg_house_losses
    and g_cls) are appended to the returned tuple.  g_cls: the cross-entropy value (a device scalar), or the [B] row terms the fused
    classifier forward left (then their mean is formed here, in the cross-entropy kernel's order).
    diag (with losses) = (logits_cf, logits_orig, src_rows or None, target_y, eps, acc or None): the trainer's four per-iteration
    diagnostics ride in the launch too (house_diag); their [4] tensor is appended after the scalars."""
    for t, nme in ((res, "res"), (masked, "masked"), (mask, "mask"), (gx_a, "gx_a"), (gx_b, "gx_b")):
        _chk(t, nme)
    B, D = res.shape
    dcont = torch.empty((B, ncont), dtype=torch.float32, device=res.device)
    dsamples = torch.empty((B, T), dtype=torch.float32, device=res.device)
    a = _lib.HouseResBwdArgs(res=res.data_ptr(), masked=masked.data_ptr(), mask=mask.data_ptr(), gx_a=gx_a.data_ptr(), gx_b=gx_b.data_ptr(),
                             w_pen=float(w_pen), w_am=float(w_am), ncont=ncont, cont_idx_dev=cont_idx.data_ptr(), seg_dev=seg_offsets.data_ptr(),
                             S=cat_idx.numel(), T=T, cat_idx_dev=cat_idx.data_ptr(), norm=norm_vals.data_ptr(), D=D, B=B,
                             dcont=dcont.data_ptr(), dsamples=dsamples.data_ptr())
    la = da = None
    outs = ()
    if losses is not None:
        d_real, d_fake, d_fake_g, g_cls, am, pen, l_cls, w_reg, l_mask, w_reg_log = losses
        out6 = torch.empty(6, dtype=torch.float32, device=res.device)
        rows = g_cls.numel() > 1
        la = _lib.HouseLossArgs(d_real=d_real.data_ptr(), d_fake=d_fake.data_ptr(), d_fake_g=d_fake_g.data_ptr(), n=d_real.numel(),
                                g_cls=None if rows else g_cls.data_ptr(), am=am.data_ptr(), pen=pen.data_ptr(), lambda_cls=float(l_cls),
                                w_reg=float(w_reg), lambda_mask=float(l_mask), w_reg_log=float(w_reg_log),
                                ce_row_loss=g_cls.data_ptr() if rows else None, n_ce=g_cls.numel() if rows else 0, out6=out6.data_ptr())
        outs = (out6,)
    if diag is not None:
        logits_cf, logits_orig, src_rows, target_y, eps, acc = diag
        out4 = torch.empty(4, dtype=torch.float32, device=res.device)
        da = _diag_args(logits_cf, logits_orig, src_rows, target_y, masked, eps, out4, acc, "house_residual_bwd(diag=...)")
        outs += (out4,)
    check(_lib.load().pcg_house_residual_bwd(a, la, da, _stream()), "pcg_house_residual_bwd")
    return (dcont, dsamples) + outs


def house_diag(logits_cf, logits_orig, target_y, masked, eps=1e-3, src_rows=None, acc=None):
    """[pred_gain, sparsity, reg_loss_l2, class_flip_rate] of house_sales_kc_usa/trainer.py:318-343 in one launch (pcg_house_diag).
    logits_orig: the frozen classifier on the original rows ([B, nc], or [N, nc] for the whole training set with src_rows [B]);
    acc: float64[8] epoch accumulators (acc[2..5] += the four values)."""
    out = torch.empty(4, dtype=torch.float32, device=logits_cf.device)
    check(_lib.load().pcg_house_diag(_diag_args(logits_cf, logits_orig, src_rows, target_y, masked, eps, out, acc, "house_diag"), _stream()),
          "pcg_house_diag")
    return out


def assemble_residual_bwd(dres, ncont, cont_idx, seg_offsets, T, cat_idx, norm_vals):
    _chk(dres, "dres")
    B, D = dres.shape
    dcont = torch.empty((B, ncont), dtype=torch.float32, device=dres.device)
    dsamples = torch.empty((B, T), dtype=torch.float32, device=dres.device)
    check(_lib.load().pcg_assemble_residual_bwd(_p(dres), ncont, _p(cont_idx), _p(seg_offsets), cat_idx.numel(), T, _p(cat_idx),
                                                _p(norm_vals), D, B, _p(dcont), _p(dsamples), _stream()), "pcg_assemble_residual_bwd")
    return dcont, dsamples


def mean_fwd(x):
    _chk(x, "x")
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = workspace(lib.pcg_mean_workspace_bytes(), x.device)
    check(lib.pcg_mean_fwd(_p(x), x.numel(), _p(out), _p(ws), ws.numel(), _stream()), "pcg_mean_fwd")
    return out


def mean_bwd(grad_out, scale, like):
    dx = torch.empty_like(like)
    check(_lib.load().pcg_mean_bwd(_p(grad_out), float(scale), like.numel(), _p(dx), _stream()), "pcg_mean_bwd")
    return dx


def spectral_norm_fwd(w_orig, u, v, eps, power_iteration):
    _chk(w_orig, "weight_orig"); _chk(u, "weight_u"); _chk(v, "weight_v")
    O, I = w_orig.shape
    w_bar = torch.empty_like(w_orig)
    sigma = torch.empty(1, dtype=torch.float32, device=w_orig.device)
    uu, vu = torch.empty_like(u), torch.empty_like(v)
    check(_lib.load().pcg_spectral_norm_fwd(_p(w_orig), O, I, _p(u), _p(v), float(eps), int(bool(power_iteration)), _p(w_bar), _p(sigma),
                                            _p(uu), _p(vu), _stream()), "pcg_spectral_norm_fwd")
    return w_bar, sigma, uu, vu


def _ptr_array(tensors):
    """A host array of the tensors' device pointers (None: a null entry)."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _i32_array(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def sn_fwd_batch(w_origs, us, vs, eps, reps=1, power_iteration=True):
    """(outputs, batch): the pcg_sn_fwd_batch of `reps` successive calls of these layers — for spectral_norm_fwd_batched, or as the
    rider of house_residual_fwd / house_classifier_bwd — and its freshly allocated outputs [[(w_bar, sigma, u_used, v_used)] per
    layer] per call (also `batch.outputs`).  The batch holds every tensor it points to."""
    outs = [[(torch.empty_like(w), torch.empty(1, dtype=torch.float32, device=w.device), torch.empty_like(u), torch.empty_like(v))
             for w, u, v in zip(w_origs, us, vs)] for _ in range(reps)]
    flat = [o for call in outs for o in call]
    b = _lib.SnFwdBatch(n=len(w_origs), reps=reps, power_iteration=int(bool(power_iteration)), eps=float(eps), w_orig=_ptr_array(w_origs),
                        out_features=_i32_array([w.shape[0] for w in w_origs]), in_features=_i32_array([w.shape[1] for w in w_origs]),
                        u=_ptr_array(us), v=_ptr_array(vs), w_bar=_ptr_array([o[0] for o in flat]), sigma=_ptr_array([o[1] for o in flat]),
                        u_used=_ptr_array([o[2] for o in flat]), v_used=_ptr_array([o[3] for o in flat]))
    b.outputs, b.tensors = outs, (list(w_origs), list(us), list(vs))
    return outs, b


def sn_bwd_batch(passes, dw_origs, accumulate, bias_adds=None):
    """The pcg_sn_bwd_batch of passes = [[(dw_bar, w_bar, u, v, sigma)] per layer] per call, applied in this order into dw_origs[l];
    bias_adds: per layer (dst, src) or None — dst += src afterwards.  For spectral_norm_bwd_batched, or as the rider of
    house_classifier_fwd.  The batch holds every tensor it points to."""
    flat = [e for call in passes for e in call]
    adds = [b if b is not None else (None, None) for b in (bias_adds or [None] * len(dw_origs))]
    b = _lib.SnBwdBatch(n=len(dw_origs), passes=len(passes), dw_bar=_ptr_array([e[0] for e in flat]), w_bar=_ptr_array([e[1] for e in flat]),
                        out_features=_i32_array([w.shape[0] for w in dw_origs]), in_features=_i32_array([w.shape[1] for w in dw_origs]),
                        u=_ptr_array([e[2] for e in flat]), v=_ptr_array([e[3] for e in flat]), sigma=_ptr_array([e[4] for e in flat]),
                        dw_orig=_ptr_array(dw_origs), accumulate=_i32_array([bool(a) for a in accumulate]),
                        db_dst=_ptr_array([d for d, _ in adds]), db_src=_ptr_array([s_ for _, s_ in adds]))
    b.tensors = (flat, list(dw_origs), adds)
    return b


def spectral_norm_fwd_batched(w_origs, us, vs, eps, power_iteration, reps=1):
    """All layers, `reps` successive calls, in one launch: [[(w_bar, sigma, u_used, v_used)] per layer] per call."""
    outs, b = sn_fwd_batch(w_origs, us, vs, eps, reps, power_iteration)
    check(_lib.load().pcg_spectral_norm_fwd_batched(b, _stream()), "pcg_spectral_norm_fwd_batched")
    return outs


def spectral_norm_bwd_batched(passes, dw_origs, accumulate, bias_adds=None):
    """All layers, all passes (see sn_bwd_batch; one call's backward: a list of one pass), in one launch."""
    check(_lib.load().pcg_spectral_norm_bwd_batched(sn_bwd_batch(passes, dw_origs, accumulate, bias_adds), _stream()),
          "pcg_spectral_norm_bwd_batched")


def house_g_fwd(desc, args):
    """The tabular generator's fused forward (csrc/house_fused.hip): a pcg_house_g_desc and pcg_house_g_fwd_args the module filled."""
    check(_lib.load().pcg_house_g_fwd(desc, args, _stream()), "pcg_house_g_fwd")


def house_g_bwd(desc, args):
    check(_lib.load().pcg_house_g_bwd(desc, args, _stream()), "pcg_house_g_bwd")


def house_critic_fwd(passes, w_bars, biases, slope=0.2):
    """The tabular critic's four layers for 1 or 2 passes in one launch (csrc/house_critic_fused.hip).  passes: [(x, onehot)];
    w_bars: the four normalised weights of every pass (pass-major).  Returns [([a0, a1, a2, a3], out)] per pass."""
    B = passes[0][0].shape[0]
    f32 = dict(dtype=torch.float32, device=passes[0][0].device)
    res = [([torch.empty((B, n), **f32) for n in (21, 32, 64, 128)], torch.empty((B, 1), **f32)) for _ in passes]
    a = _lib.HouseCriticFwdArgs(n_pass=len(passes), B=B, D=passes[0][0].shape[1], NC=passes[0][1].shape[1], slope=slope,
                                x=_ptr_array([_chk(x, "x") for x, _ in passes]), onehot=_ptr_array([_chk(o, "onehot") for _, o in passes]),
                                w_bar=_ptr_array(w_bars), bias=_ptr_array(biases), out=_ptr_array([o for _, o in res]),
                                **{f"a{i}": _ptr_array([acts[i] for acts, _ in res]) for i in range(4)})
    check(_lib.load().pcg_house_critic_fwd(a, _stream()), "pcg_house_critic_fwd")
    return res


def house_critic_bwd(douts, w_bars, acts, input_dim, need_dx, slope=0.2):
    """The backward of house_critic_fwd for the same passes (acts: their [a0..a3]) in one launch: [(d3, d2, d1, dx or None)] per pass."""
    B = douts[0].shape[0]
    f32 = dict(dtype=torch.float32, device=douts[0].device)
    res = [tuple(torch.empty((B, n), **f32) for n in (128, 64, 32)) + ((torch.empty((B, input_dim), **f32) if need_dx else None),) for _ in douts]
    a = _lib.HouseCriticBwdArgs(n_pass=len(douts), B=B, D=input_dim, slope=slope, dout=_ptr_array([_chk(d, "dout") for d in douts]),
                                w_bar=_ptr_array(w_bars), a1=_ptr_array([a_[1] for a_ in acts]), a2=_ptr_array([a_[2] for a_ in acts]),
                                a3=_ptr_array([a_[3] for a_ in acts]), d3=_ptr_array([r[0] for r in res]), d2=_ptr_array([r[1] for r in res]),
                                d1=_ptr_array([r[2] for r in res]), dx=_ptr_array([r[3] for r in res]))
    check(_lib.load().pcg_house_critic_bwd(a, _stream()), "pcg_house_critic_bwd")
    return res


def house_classifier_fwd(x, w_kmajor, biases, sn_bwd=None, ce=None):
    """The frozen tabular classifier's five layers in one launch (csrc/house_classifier_fused.hip): (logits, [a1, a2, a3, a4]).
    sn_bwd: a batch of sn_bwd_batch — that spectral-norm backward rides in the launch.  ce = (target, grad_scale), with a rider only:
    the launch also leaves the cross-entropy's gradient and row terms: (logits, acts, dlogits, row_loss)."""
    _chk(x, "x")
    B = x.shape[0]
    f32 = dict(dtype=torch.float32, device=x.device)
    acts = [torch.empty((B, n), **f32) for n in (256, 256, 128, 64)]
    logits = torch.empty((B, 4), **f32)
    a = _lib.HouseClsFwdArgs(x=x.data_ptr(), B=B, w_kmajor=_ptr_array(w_kmajor), bias=_ptr_array(biases), a1=acts[0].data_ptr(),
                             a2=acts[1].data_ptr(), a3=acts[2].data_ptr(), a4=acts[3].data_ptr(), logits=logits.data_ptr())
    tail = ()
    if ce is not None:
        tail = (torch.empty((B, 4), **f32), torch.empty((B,), **f32))
        a.ce_target, a.ce_grad_scale = _chk(ce[0], "ce target", torch.int64).data_ptr(), float(ce[1])
        a.ce_dlogits, a.ce_row_loss = tail[0].data_ptr(), tail[1].data_ptr()
    check(_lib.load().pcg_house_classifier_fwd(a, sn_bwd, _stream()), "pcg_house_classifier_fwd")
    return (logits, acts) + tail


def house_classifier_bwd(dlogits, w_stored, acts, sn_fwd=None):
    """dx [B, 17] of the frozen classifier in one launch.  sn_fwd: a training-mode batch of sn_fwd_batch — it rides in the launch;
    the return value is then (dx, its outputs)."""
    _chk(dlogits, "dlogits")
    B = dlogits.shape[0]
    dx = torch.empty((B, 17), dtype=torch.float32, device=dlogits.device)
    a = _lib.HouseClsBwdArgs(dlogits=dlogits.data_ptr(), B=B, w_stored=_ptr_array(w_stored), a1=acts[0].data_ptr(), a2=acts[1].data_ptr(),
                             a3=acts[2].data_ptr(), a4=acts[3].data_ptr(), dx=dx.data_ptr())
    check(_lib.load().pcg_house_classifier_bwd(a, sn_fwd, _stream()), "pcg_house_classifier_bwd")
    return dx if sn_fwd is None else (dx, sn_fwd.outputs)


def spectral_norm_bwd(dw_bar, w_bar, u, v, sigma, dw_orig, accumulate):
    O, I = w_bar.shape
    check(_lib.load().pcg_spectral_norm_bwd(_p(dw_bar), _p(w_bar), O, I, _p(u), _p(v), _p(sigma), _p(dw_orig), int(bool(accumulate)),
                                            _stream()), "pcg_spectral_norm_bwd")


def cross_entropy_weighted_fwd_bwd(logits, target, class_weight, need_loss=True, need_grad=True, grad_out=None, grad_scale=1.0):
    _chk(logits, "logits"); _chk_idx(target, logits.shape[-1], "target"); _chk(class_weight, "class_weight")
    B, K = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device) if need_loss else None
    dz = torch.empty_like(logits) if need_grad else None
    check(_lib.load().pcg_cross_entropy_weighted_fwd_bwd(_p(logits), _p(target), _p(class_weight), B, K, float(grad_scale), _p(grad_out),
                                                         _p(loss), _p(dz), _stream()), "pcg_cross_entropy_weighted_fwd_bwd")
    return loss, dz


def ce_weighted_tally(logits, target, class_weight, tally, seg=None, dlogits=None, seg_loss=None, dbias=None):
    """nn.CrossEntropyLoss(weight=class_weight) per run of `seg` rows (None: one run) with the epoch bookkeeping in one launch
    (pcg_ce_weighted_tally): tally (float64[3] on the device) += (sum of loss * rows, rows whose argmax is the target, rows).
    dlogits ([B, K], one run only): the gradient of the mean; dbias ([K], with dlogits): its column sums, the bias gradient of the
    logits layer; seg_loss (float32, one entry per run): the losses themselves."""
    _chk(logits, "logits"); _chk_idx(target, logits.shape[-1], "target"); _chk(class_weight, "class_weight")
    B, K = logits.shape
    seg = B if seg is None else int(seg)
    _chk(tally, "tally", torch.float64)
    if tally.numel() < 3 or target.numel() != B or class_weight.numel() != K:
        raise _lib.PcgError("ce_weighted_tally: tally must be float64[3], target [B], class_weight [K]")
    if dlogits is not None and tuple(_chk(dlogits, "dlogits").shape) != (B, K):
        raise _lib.PcgError(f"ce_weighted_tally: dlogits must be [{B}, {K}]")
    if dbias is not None and _chk(dbias, "dbias").numel() != K:
        raise _lib.PcgError(f"ce_weighted_tally: dbias must have {K} entries")
    if seg_loss is not None and (seg < 1 or _chk(seg_loss, "seg_loss").numel() < (B + min(seg, B) - 1) // min(seg, B)):
        raise _lib.PcgError("ce_weighted_tally: seg_loss needs one entry per segment")
    check(_lib.load().pcg_ce_weighted_tally(_p(logits), _p(target), _p(class_weight), B, K, seg, _p(tally), _p(dlogits), _p(dbias),
                                            _p(seg_loss), _stream()),
          "pcg_ce_weighted_tally")
    return tally


def dropout_apply(x, mask, p, inner=1, C=None, out=None):
    """y = x * mask / (1 - p); mask one entry per element (inner=1) or per (sample, channel) of an NHWC activation (inner=HW)."""
    _chk(x, "x"); _chk(mask, "mask")
    C = C if C is not None else x.shape[-1]
    y = out if out is not None else torch.empty_like(x)
    check(_lib.load().pcg_dropout_apply(_p(x), _p(mask), x.numel(), inner, C, 1.0 / (1.0 - p), _p(y), _stream()), "pcg_dropout_apply")
    return y


def weighted_sum_fwd(terms, weights, out=None):
    n = len(terms)
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=terms[0].device)
    check(_lib.load().pcg_weighted_sum_fwd(n, _ptr_array(terms), (ctypes.c_float * n)(*[float(w) for w in weights]), _p(out), _stream()),
          "pcg_weighted_sum_fwd")
    return out


def weighted_sum_bwd(weights, grad_out, needs):
    """[w_i * grad_out as a one-element tensor, or None where needs[i] is False]"""
    n = len(weights)
    dev = grad_out.device
    outs = [torch.empty(1, dtype=torch.float32, device=dev) if need else None for need in needs]
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() if o is not None else None for o in outs])
    check(_lib.load().pcg_weighted_sum_bwd(n, (ctypes.c_float * n)(*[float(w) for w in weights]), _p(grad_out), ptrs, _stream()),
          "pcg_weighted_sum_bwd")
    return outs


def cf_metrics(logits_cf, target, logits_ref=None, other=None):
    """[class-flip rate, prediction gain] as a 2-element device tensor (see pcg_cf_metrics)."""
    _chk(logits_cf, "logits_cf"); _chk_idx(target, logits_cf.shape[1], "target")
    B, K = logits_cf.shape
    out = torch.empty(2, dtype=torch.float32, device=logits_cf.device)
    check(_lib.load().pcg_cf_metrics(_p(logits_cf), _p(logits_ref), _p(target), _p(other), B, K, _p(out), _stream()), "pcg_cf_metrics")
    return out


# ---- WGAN-GP critic pieces (csrc/instnorm.hip) ----------------------------------------------------------------------------
def instnorm_fwd(x, B, HW, C, gamma, beta, eps, act=0, slope=0.0):
    _chk(x, "x")
    y = torch.empty_like(x)
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    check(_lib.load().pcg_instnorm_fwd(_p(x), B, HW, C, _p(gamma), _p(beta), float(eps), act, float(slope), _p(y), _p(mean), _p(invstd),
                                       _stream()), "pcg_instnorm_fwd")
    return y, mean, invstd


def instnorm_bwd(dy, x, B, HW, C, mean, invstd, gamma, need_dx=True, need_params=True):
    """(dx, dgamma_partial [B,C], dbeta_partial [B,C])"""
    _chk(dy, "dy"); _chk(x, "x")
    dx = torch.empty_like(x) if need_dx else None
    dgp = torch.empty((B, C), dtype=torch.float32, device=x.device) if need_params else None
    dbp = torch.empty((B, C), dtype=torch.float32, device=x.device) if need_params else None
    check(_lib.load().pcg_instnorm_bwd(_p(dy), _p(x), B, HW, C, _p(mean), _p(invstd), _p(gamma), _p(dx), _p(dgp), _p(dbp), _stream()),
          "pcg_instnorm_bwd")
    return dx, dgp, dbp


def instnorm_bwd_fused(dy, x, B, HW, C, mean, invstd, gamma, act_y=None, slope=0.0, keep_dn=False, addend=None, need_params=True,
                       need_dxsum=False):
    """LeakyReLU' -> InstanceNorm' (-> + addend) of a critic stage in one launch: (dx, dn or None, dgamma_partial, dbeta_partial,
    dxsum_partial), partials [B, C] (rowsum3 reduces them over B); see pcg_instnorm_bwd_fused in include/pcgan_hip.h."""
    _chk(dy, "dy"); _chk(x, "x")
    dx = torch.empty_like(x)
    dn = torch.empty_like(x) if (keep_dn and act_y is not None) else None
    mk = lambda on: torch.empty((B, C), dtype=torch.float32, device=x.device) if on else None
    dgp, dbp, dsp = mk(need_params), mk(need_params), mk(need_dxsum)
    check(_lib.load().pcg_instnorm_bwd_fused(_p(dy), _p(act_y), float(slope), _p(x), B, HW, C, _p(mean), _p(invstd), _p(gamma), _p(dn), _p(addend),
                                             _p(dx), _p(dgp), _p(dbp), _p(dsp), _stream()), "pcg_instnorm_bwd_fused")
    return dx, dn, dgp, dbp, dsp


def rowsum3(items, rows, C):
    """items: up to three (src [rows, C], dst [C], accumulate) — dst (+)= column sums of src, all in one launch."""
    assert 1 <= len(items) <= 3
    a = []
    for k in range(3):
        src, dst, acc = items[k] if k < len(items) else (None, None, False)
        a += [_p(src), _p(dst), int(bool(acc))]
    check(_lib.load().pcg_rowsum3(len(items), *a, int(rows), int(C), _stream()), "pcg_rowsum3")


def instnorm_bwd_bwd(r, dy, x, B, HW, C, mean, invstd, gamma, need_ddy=True, need_ez=True, need_gamma=True, act_y=None, slope=0.0):
    """(ddy, ez, dgamma_partial [B,C]); act_y: ddy continues through the stage's LeakyReLU (its output) in the same launch"""
    _chk(r, "r"); _chk(dy, "dy"); _chk(x, "x")
    ddy = torch.empty_like(x) if need_ddy else None
    ez = torch.empty_like(x) if need_ez else None
    dgp = torch.empty((B, C), dtype=torch.float32, device=x.device) if need_gamma else None
    check(_lib.load().pcg_instnorm_bwd_bwd_act(_p(r), _p(dy), _p(x), B, HW, C, _p(mean), _p(invstd), _p(gamma), _p(act_y), float(slope), _p(ddy),
                                               _p(ez), _p(dgp), _stream()), "pcg_instnorm_bwd_bwd_act")
    return ddy, ez, dgp


def nhwc_to_nchw_flat(src, B, HW, C, inverse=False):
    _chk(src, "src")
    dst = torch.empty_like(src)
    check(_lib.load().pcg_nhwc_to_nchw_flat(_p(src), _p(dst), B, HW, C, int(bool(inverse)), _stream()), "pcg_nhwc_to_nchw_flat")
    return dst


def _chk_pool(args):
    """args: (tensor, name, dtype, expected shape or None) per NHWC argument of a pooling call.  Shape, dtype and contiguity of EVERY
    argument first, the device last: the host-only checks can be exercised without a GPU."""
    for t, name, dtype, shape in args:
        if t.dim() != 4:
            raise _lib.PcgError(f"{name}: expected an NHWC tensor [B, H, W, C], got shape {tuple(t.shape)}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise _lib.PcgError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.shape[3] % 4 != 0:
            raise _lib.PcgError(f"{name}: C must be a multiple of 4 (one thread owns four channels), got {t.shape[3]}")
        if t.dtype != dtype:
            raise _lib.PcgError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.PcgError(f"{name}: expected a contiguous tensor, got strides {t.stride()} for shape {tuple(t.shape)}")
    for t, name, _, _ in args:
        if not t.is_cuda:
            raise _lib.PcgError(f"{name}: expected a tensor on the GPU (libpcgan_hip has no CPU path), got {t.device}")


def relu_maxpool2_fwd(z, out=None, idx=None):
    """nn.ReLU + nn.MaxPool2d(2) of the NHWC activation z [B, H, W, C] (C % 4 == 0) in one launch (pcg_relu_maxpool2_fwd):
    (p [B, H//2, W//2, C] fp32, idx uint8 of the same shape: the winning cell dh * 2 + dw, chosen as torch's max_pool2d chooses it).
    z may be raw or already through ReLU."""
    if z.dim() == 4 and min(z.shape[1], z.shape[2]) < 2:
        raise _lib.PcgError(f"relu_maxpool2_fwd: H and W must be at least 2, got {z.shape[1]}x{z.shape[2]}")
    ps = (z.shape[0], z.shape[1] // 2, z.shape[2] // 2, z.shape[3]) if z.dim() == 4 else None
    _chk_pool([(z, "z", torch.float32, None)] + ([(out, "out", torch.float32, ps)] if out is not None else [])
              + ([(idx, "idx", torch.uint8, ps)] if idx is not None else []))
    B, H, W, C = z.shape
    p = out if out is not None else torch.empty(ps, dtype=torch.float32, device=z.device)
    idx = idx if idx is not None else torch.empty(ps, dtype=torch.uint8, device=z.device)
    check(_lib.load().pcg_relu_maxpool2_fwd(_p(z), _p(p), _p(idx), B, H, W, C, _stream()), "pcg_relu_maxpool2_fwd")
    return p, idx


def relu_maxpool2_bwd(dp, p, idx, hw, out=None):
    """The backward of relu_maxpool2_fwd in one launch (pcg_relu_maxpool2_bwd): dz [B, H, W, C] for hw = (H, W), the gradient with
    respect to the convolution's raw output -- dp where p > 0 at each window's chosen cell, 0 everywhere else, every element
    written once.  Reads p (the forward's output), never z."""
    H, W = int(hw[0]), int(hw[1])
    if dp.dim() == 4 and (H // 2 != dp.shape[1] or W // 2 != dp.shape[2] or min(dp.shape[1], dp.shape[2]) < 1):
        raise _lib.PcgError(f"relu_maxpool2_bwd: hw = {H}x{W} does not pool to dp's {dp.shape[1]}x{dp.shape[2]}")
    zs = (dp.shape[0], H, W, dp.shape[3]) if dp.dim() == 4 else None
    _chk_pool([(dp, "dp", torch.float32, None), (p, "p", torch.float32, dp.shape), (idx, "idx", torch.uint8, dp.shape)]
              + ([(out, "out", torch.float32, zs)] if out is not None else []))
    B, C = dp.shape[0], dp.shape[3]
    dz = out if out is not None else torch.empty(zs, dtype=torch.float32, device=dp.device)
    check(_lib.load().pcg_relu_maxpool2_bwd(_p(dp), _p(p), _p(idx), _p(dz), B, H, W, C, _stream()), "pcg_relu_maxpool2_bwd")
    return dz


def drop2d_flatten_fwd(a, mask, p, R, HW, C, out=None):
    """nn.Dropout2d(p) + nn.Flatten of the NCHW tensor from the NHWC activation a [R, HW, C] in one launch
    (pcg_drop2d_flatten_fwd): out [R, C * HW], out[b, c * HW + q] = a[b, q, c] * mask[b, c] / (1 - p) -- the bits of
    dropout_apply(inner=HW) followed by nhwc_to_nchw_flat."""
    _chk(a, "a"); _chk(mask, "mask")
    if a.numel() != R * HW * C or mask.numel() != R * C:
        raise _lib.PcgError(f"drop2d_flatten_fwd: a must hold {R}x{HW}x{C} values and mask {R}x{C}")
    out = out if out is not None else torch.empty((R, C * HW), dtype=torch.float32, device=a.device)
    if _chk(out, "out").numel() != a.numel():
        raise _lib.PcgError(f"drop2d_flatten_fwd: out must be [{R}, {C * HW}]")
    check(_lib.load().pcg_drop2d_flatten_fwd(_p(a), _p(mask), 1.0 / (1.0 - p), R, HW, C, _p(out), _stream()), "pcg_drop2d_flatten_fwd")
    return out


def drop2d_flatten_bwd(dflat, mask, p, y, R, HW, C, act=_lib.ACT_RELU, slope=0.0, out=None):
    """The backward of drop2d_flatten_fwd and of the activation whose output y [R, HW, C] feeds it, in one launch
    (pcg_drop2d_flatten_bwd): out[b, q, c] = dflat[b, c * HW + q] * mask[b, c] / (1 - p) * act'(y[b, q, c]) -- the bits of
    nhwc_to_nchw_flat(inverse=True), dropout_apply(inner=HW), act_bwd."""
    _chk(dflat, "dflat"); _chk(mask, "mask"); _chk(y, "y")
    if dflat.numel() != R * HW * C or y.numel() != R * HW * C or mask.numel() != R * C:
        raise _lib.PcgError(f"drop2d_flatten_bwd: dflat and y must hold {R}x{HW}x{C} values and mask {R}x{C}")
    out = out if out is not None else torch.empty_like(y)
    if _chk(out, "out").numel() != y.numel():
        raise _lib.PcgError(f"drop2d_flatten_bwd: out must hold {R}x{HW}x{C} values")
    check(_lib.load().pcg_drop2d_flatten_bwd(_p(dflat), _p(mask), 1.0 / (1.0 - p), _p(y), int(act), float(slope), R, HW, C, _p(out), _stream()),
          "pcg_drop2d_flatten_bwd")
    return out


def mnist_clf_head(h, m1, p, W2, b2, y, tally, logits=None, loss=None, dW2=None, db2=None, dh=None, db1=None):
    """Everything above fc1's output of the MNIST classifier's training step in one launch of one workgroup (pcg_mnist_clf_head):
    Dropout(p) with the mask m1, Linear(W2, b2), mean cross-entropy against y, and the backward down to fc1's pre-activation.
    h [R, 256] is fc1's post-ReLU output, R <= 128, K = W2.shape[0] <= 16.  tally (float64[3]) += (loss * R, rows whose argmax is
    the label, R).  Returns (logits [R, K], loss [1], dW2 [K, 256], db2 [K], dh [R, 256], db1 [256]); buffers given are filled."""
    _chk(h, "h"); _chk(m1, "m1"); _chk(W2, "W2"); _chk(b2, "b2"); _chk_idx(y, W2.shape[0], "y"); _chk(tally, "tally", torch.float64)
    R, I = h.shape
    K = W2.shape[0]
    if tuple(m1.shape) != (R, I) or W2.shape[1] != I or b2.numel() != K or y.numel() != R or tally.numel() < 3:
        raise _lib.PcgError(f"mnist_clf_head: h [R, I] {tuple(h.shape)}, m1 {tuple(m1.shape)}, W2 [K, I] {tuple(W2.shape)}, b2 [K], y [R], "
                            "tally float64[3] do not agree")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=h.device)      # noqa: E731
    outs = []
    for t, name, shape in ((logits, "logits", (R, K)), (loss, "loss", (1,)), (dW2, "dW2", (K, I)), (db2, "db2", (K,)), (dh, "dh", (R, I)),
                           (db1, "db1", (I,))):
        t = t if t is not None else f32(*shape)
        if tuple(_chk(t, name).shape) != shape:
            raise _lib.PcgError(f"mnist_clf_head: {name} must be {list(shape)}, got {list(t.shape)}")
        outs.append(t)
    check(_lib.load().pcg_mnist_clf_head(_p(h), _p(m1), 1.0 / (1.0 - p), _p(W2), _p(b2), _p(y), R, I, K, *[_p(t) for t in outs[:2]], _p(tally),
                                         *[_p(t) for t in outs[2:]], _stream()), "pcg_mnist_clf_head")
    return tuple(outs)


# ---- the additive-delta MNIST CounteRGAN step (csrc/delta_gan.hip) -----------------------------------------------------
def delta_gan_workspace(B, HW, device):
    """A zeroed workspace for delta_gan_tail_fwd (arrival counter + one partial per 1024 elements) and, in its own tensor, the 16
    bytes of logit_head_fwd: (tail_ws, head_ws).  Allocate it outside any graph capture; the kernels leave the counters zero."""
    need = _lib.load().pcg_delta_gan_tail_workspace_bytes(int(B), int(HW))
    if need == 0:
        raise _lib.PcgError(f"delta_gan_workspace: {B} rows of {HW} pixels are outside the index range")
    return torch.zeros(need, dtype=torch.uint8, device=device), torch.zeros(16, dtype=torch.uint8, device=device)


def _delta_ws(B, HW, device):
    """The current stream's cached workspace pair, grown on demand (never while the stream captures: the zero fill would replay)."""
    stream = torch.cuda.current_stream(device).cuda_stream
    key = (device.type, device.index, stream, "delta_gan")
    ws = _ws_cache.get(key)
    need = _lib.load().pcg_delta_gan_tail_workspace_bytes(int(B), int(HW))
    if ws is None or ws[0].numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PcgError("delta_gan: pass a workspace from ops.delta_gan_workspace() made before the capture")
        if ws is not None:
            _ws_retired.append(ws)
        ws = delta_gan_workspace(B, HW, device)
        _ws_cache[key] = ws
    return ws


def _host_labels(t, name):
    if t is None:
        return None, ctypes.c_void_p(0)
    h = torch.as_tensor(t, dtype=torch.int64, device="cpu").contiguous()
    return h, ctypes.c_void_p(h.data_ptr())


def delta_gan_entry(x, y, target, table_g, table_d, g_in=None, d_in=None, labels_2b=None, head_w=None, head_w_packed=None, head_shape=None,
                    regather=False, y_host=None, target_host=None):
    """pcg_delta_gan_entry: g_in [B, HW, 2] = (x, table_g[target]); d_in [2B, HW, 2] rows 0..B = (x, table_d[y]), rows B..2B channel 1 =
    table_d[target]; labels_2b [2B] = (y, target); head_w_packed = the (h,w,c) image of head_w, head_shape = (C, P).  regather=True
    writes only channel 1 of d_in rows B..2B (and the packed head weight).  y_host / target_host: host copies, range-checked by the
    library before the launch.  Returns (g_in, d_in)."""
    _chk(table_d, "table_d"); _chk_idx(target, table_d.shape[0], "target")
    B, (K, HW) = target.numel(), table_d.shape
    dev = table_d.device
    if regather:
        if d_in is None:
            raise _lib.PcgError("delta_gan_entry: the regather needs the d_in it rewrites")
    else:
        _chk(x, "x"); _chk(table_g, "table_g"); _chk_idx(y, K, "y")
        if x.numel() != B * HW or y.numel() != B or tuple(table_g.shape) != (K, HW):
            raise _lib.PcgError(f"delta_gan_entry: x {tuple(x.shape)}, y {tuple(y.shape)}, tables {tuple(table_g.shape)} / {tuple(table_d.shape)} do not agree")
        g_in = g_in if g_in is not None else torch.empty((B, HW, 2), dtype=torch.float32, device=dev)
        d_in = d_in if d_in is not None else torch.empty((2 * B, HW, 2), dtype=torch.float32, device=dev)
        _chk(g_in, "g_in")
        if g_in.numel() != 2 * B * HW:
            raise _lib.PcgError(f"delta_gan_entry: g_in holds {g_in.numel()} floats, {2 * B * HW} needed")
    _chk(d_in, "d_in")
    if d_in.numel() != 4 * B * HW:
        raise _lib.PcgError(f"delta_gan_entry: d_in holds {d_in.numel()} floats, {4 * B * HW} needed")
    if labels_2b is not None and (_chk(labels_2b, "labels_2b", torch.int64).numel() != 2 * B):
        raise _lib.PcgError(f"delta_gan_entry: labels_2b holds {labels_2b.numel()} entries, {2 * B} needed")
    hc = hp = 0
    if head_w is not None:
        hc, hp = (int(v) for v in head_shape)
        _chk(head_w, "head_w"); _chk(head_w_packed, "head_w_packed")
        if head_w.numel() != hc * hp or head_w_packed.numel() != hc * hp:
            raise _lib.PcgError(f"delta_gan_entry: head weight of {head_w.numel()} columns is not {hc} x {hp}")
    yh, yhp = _host_labels(y_host, "y_host")
    th, thp = _host_labels(target_host, "target_host")
    a = _lib.DeltaGanEntryArgs(_p(None if regather else x), _p(None if regather else y), _p(target), yhp, thp, _p(None if regather else table_g),
                               _p(table_d), _p(None if regather else g_in), _p(d_in), _p(labels_2b), _p(head_w), _p(head_w_packed), B, HW, K,
                               _lib.DELTA_GAN_REGATHER if regather else _lib.DELTA_GAN_BUILD, hc, hp)
    check(_lib.load().pcg_delta_gan_entry(ctypes.byref(a), _stream()), "pcg_delta_gan_entry")
    return g_in, d_in


def delta_gan_tail_fwd(x, delta, d_in, x_cf=None, loss_reg=None, ws=None, grid=0):
    """pcg_delta_gan_tail_fwd: x_cf = x + delta to x_cf [B, HW] and to channel 0 of d_in rows B..2B; loss_reg [1] = mean|delta|.
    ws: the tail workspace of delta_gan_workspace (default: the stream's cached one).  Returns (x_cf, loss_reg)."""
    _chk(x, "x"); _chk(delta, "delta"); _chk(d_in, "d_in")
    B = x.shape[0]
    HW = x.numel() // B
    if delta.numel() != B * HW or d_in.numel() != 4 * B * HW:
        raise _lib.PcgError(f"delta_gan_tail_fwd: x {tuple(x.shape)}, delta {tuple(delta.shape)}, d_in {tuple(d_in.shape)} do not agree")
    x_cf = x_cf if x_cf is not None else torch.empty((B, HW), dtype=torch.float32, device=x.device)
    loss_reg = loss_reg if loss_reg is not None else torch.empty(1, dtype=torch.float32, device=x.device)
    _chk(x_cf, "x_cf"); _chk(loss_reg, "loss_reg")
    if x_cf.numel() != B * HW:
        raise _lib.PcgError(f"delta_gan_tail_fwd: x_cf holds {x_cf.numel()} floats, {B * HW} needed")
    ws = ws if ws is not None else _delta_ws(B, HW, x.device)[0]
    a = _lib.DeltaGanTailFwdArgs(_p(x), _p(delta), _p(x_cf), _p(d_in), _p(loss_reg), _p(ws), ws.numel(), B, HW, int(grid))
    check(_lib.load().pcg_delta_gan_tail_fwd(ctypes.byref(a), _stream()), "pcg_delta_gan_tail_fwd")
    return x_cf, loss_reg


def logit_head_fwd(a, w, bias, mode_g=False, logits=None, loss=None, dlogit=None, db=None, ws=None):
    """pcg_logit_head_fwd: logits [R] = a [R, F] . w [F] + bias; the BCE-with-logits loss of gan_train.py:127 (mode D: rows 0..R/2
    labelled 1, the rest 0, mean + mean) or :137 (mode_g: all rows labelled 1), its gradient dlogit [R] and db [1] = sum dlogit.
    Returns (logits, loss, dlogit, db)."""
    _chk(a, "a"); _chk(w, "w"); _chk(bias, "bias")
    R = a.shape[0]
    F = a.numel() // R
    if w.numel() != F or bias.numel() != 1:
        raise _lib.PcgError(f"logit_head_fwd: a [R, F] {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} do not agree")
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=a.device)      # noqa: E731
    outs = []
    for t, name, n in ((logits, "logits", R), (loss, "loss", 1), (dlogit, "dlogit", R), (db, "db", 1)):
        t = t if t is not None else f32(n)
        if _chk(t, name).numel() != n:
            raise _lib.PcgError(f"logit_head_fwd: {name} holds {t.numel()} floats, {n} needed")
        outs.append(t)
    ws = ws if ws is not None else _delta_ws(1, 4, a.device)[1]
    args = _lib.LogitHeadFwdArgs(_p(a), _p(w), _p(bias), *[_p(t) for t in outs], _p(ws), R, F, _lib.LOGIT_HEAD_G if mode_g else _lib.LOGIT_HEAD_D)
    check(_lib.load().pcg_logit_head_fwd(ctypes.byref(args), _stream()), "pcg_logit_head_fwd")
    return tuple(outs)


def logit_head_bwd(a, w, dlogit, slope, da=None, dw=None, dw_shape=None):
    """pcg_logit_head_bwd: da [R, F] = dlogit[r] * w[f] * (a > 0 ? 1 : slope); dw [F] (None: not formed) = sum_r dlogit[r] * a[r][f],
    stored in w's packed order, or with dw_shape = (C, P) at [c * P + p] for the packed column p * C + c.  Returns (da, dw)."""
    _chk(a, "a"); _chk(w, "w"); _chk(dlogit, "dlogit")
    R = a.shape[0]
    F = a.numel() // R
    if w.numel() != F or dlogit.numel() != R:
        raise _lib.PcgError(f"logit_head_bwd: a [R, F] {tuple(a.shape)}, w {tuple(w.shape)}, dlogit {tuple(dlogit.shape)} do not agree")
    da = da if da is not None else torch.empty_like(a)
    _chk(da, "da")
    if da.numel() != a.numel() or (dw is not None and _chk(dw, "dw").numel() != F):
        raise _lib.PcgError("logit_head_bwd: da must match a and dw must hold F floats")
    c, p = (int(v) for v in dw_shape) if dw_shape is not None else (0, 0)
    args = _lib.LogitHeadBwdArgs(_p(a), _p(w), _p(dlogit), _p(da), _p(dw), float(slope), R, F, c, p)
    check(_lib.load().pcg_logit_head_bwd(ctypes.byref(args), _stream()), "pcg_logit_head_bwd")
    return da, dw


def delta_gan_tail_bwd(dD, dC, delta, lambda_cls, lambda_reg, dD_stride=1, out=None):
    """pcg_delta_gan_tail_bwd: d_delta = dD[.. * dD_stride] + lambda_cls * dC + (lambda_reg / (B * HW)) * sign(delta), in that order."""
    _chk(dD, "dD"); _chk(dC, "dC"); _chk(delta, "delta")
    B = delta.shape[0]
    HW = delta.numel() // B
    if dC.numel() != B * HW or dD.numel() != B * HW * int(dD_stride):
        raise _lib.PcgError(f"delta_gan_tail_bwd: dD {tuple(dD.shape)}, dC {tuple(dC.shape)}, delta {tuple(delta.shape)} do not agree")
    out = out if out is not None else torch.empty((B, HW), dtype=torch.float32, device=delta.device)
    _chk(out, "d_delta")
    args = _lib.DeltaGanTailBwdArgs(_p(dD), _p(dC), _p(delta), _p(out), float(lambda_cls), float(lambda_reg) / (B * HW), B, HW, int(dD_stride))
    check(_lib.load().pcg_delta_gan_tail_bwd(ctypes.byref(args), _stream()), "pcg_delta_gan_tail_bwd")
    return out


# ---- the full-resolution MNIST CounteRGAN's head and losses (csrc/prob_head.hip) ---------------------------------------
LOG_EPS = 1e-6                                           # countergan2.py:188,198


def prob_head_workspace(R, device, slabs=0):
    """A zeroed workspace for prob_head_fwd on R rows (arrival counter + one partial per row and slab).  Allocate it outside any graph
    capture; the kernel leaves it zero."""
    need = _lib.load().pcg_prob_head_workspace_bytes(int(R), int(slabs))
    if need == 0:
        raise _lib.PcgError(f"prob_head_workspace: {R} rows in {slabs} slabs: 1..65535 rows, 0..{_lib.PROB_HEAD_MAX_SLABS} slabs")
    return torch.zeros(need, dtype=torch.uint8, device=device)


def _prob_head_ws(R, slabs, device):
    """The current stream's cached head workspace, grown on demand (never while the stream captures: the zero fill would replay)."""
    stream = torch.cuda.current_stream(device).cuda_stream
    key = (device.type, device.index, stream, "prob_head")
    ws = _ws_cache.get(key)
    need = _lib.load().pcg_prob_head_workspace_bytes(int(R), int(slabs))
    if need and (ws is None or ws.numel() < need):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PcgError("prob_head_fwd: pass a workspace from ops.prob_head_workspace() made before the capture")
        if ws is not None:
            _ws_retired.append(ws)
        ws = _ws_cache[key] = prob_head_workspace(R, device, slabs)
    return ws if ws is not None else torch.zeros(16, dtype=torch.uint8, device=device)     # an R / slabs the entry itself refuses


def prob_head_fwd(a, w, bias, mode_g=False, eps=LOG_EPS, slabs=0, logits=None, prob=None, loss=None, dlogit=None, db=None, ws=None):
    """pcg_prob_head_fwd: logits [R] = a [R, F] . w [F] + bias, prob = sigmoid(logits), the log-eps loss of countergan2.py:188 (mode D:
    rows 0..R/2 are D(real), the rest D(fake)) or :198 (mode_g: every row), its gradient dlogit [R] and db [1] = sum dlogit.  slabs: the
    column slabs a row is cut into (0: the library's choice).  Returns (logits, prob, loss, dlogit, db)."""
    _chk(a, "a"); _chk(w, "w"); _chk(bias, "bias")
    R = a.shape[0]
    F = a.numel() // R
    if w.numel() != F or bias.numel() != 1:
        raise _lib.PcgError(f"prob_head_fwd: a [R, F] {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} do not agree")
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=a.device)      # noqa: E731
    outs = []
    for t, name, n in ((logits, "logits", R), (prob, "prob", R), (loss, "loss", 1), (dlogit, "dlogit", R), (db, "db", 1)):
        t = t if t is not None else f32(n)
        if _chk(t, name).numel() != n:
            raise _lib.PcgError(f"prob_head_fwd: {name} holds {t.numel()} floats, {n} needed")
        outs.append(t)
    ws = ws if ws is not None else _prob_head_ws(R, slabs, a.device)
    args = _lib.ProbHeadFwdArgs(_p(a), _p(w), _p(bias), *[_p(t) for t in outs], _p(ws), ws.numel(), float(eps), R, F,
                                _lib.PROB_HEAD_G if mode_g else _lib.PROB_HEAD_D, int(slabs))
    check(_lib.load().pcg_prob_head_fwd(ctypes.byref(args), _stream()), "pcg_prob_head_fwd")
    return tuple(outs)


def log_eps_loss_fwd_bwd(p, mode_g=False, eps=LOG_EPS, need_loss=True, need_grad=True, grad_out=None, loss_out=None):
    """pcg_log_eps_loss_fwd_bwd on probabilities p [R]: the loss of countergan2.py:188 (rows 0..R/2 real, the rest fake) or :198
    (mode_g).  Returns (loss [1] or None, dp [R] or None); dp is the gradient with respect to p, times the one-element device tensor
    grad_out where given."""
    _chk(p, "p")
    loss = (loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=p.device)) if need_loss else None
    dp = torch.empty_like(p) if need_grad else None
    args = _lib.LogEpsLossArgs(_p(p), _p(grad_out), _p(loss), _p(dp), float(eps), p.numel(), _lib.PROB_HEAD_G if mode_g else _lib.PROB_HEAD_D)
    check(_lib.load().pcg_log_eps_loss_fwd_bwd(ctypes.byref(args), _stream()), "pcg_log_eps_loss_fwd_bwd")
    return loss, dp


# ---- the additive-delta CounteRGAN's prompted queries and random-target draw (csrc/delta_cf_eval.hip) ------------------
def delta_cf_entry(x, target, table, T=1, q0=0, nq=None, out=None, target_host=None):
    """pcg_delta_cf_entry: [nq, HW, 2] with channels (x[b], table[target(q)]) for the queries q = t * B + b of the window; x [B, HW];
    target None (the sweep over T classes) or [B] int64 on the GPU with T = 1.  target_host: a host copy of target, range-checked by
    the library before the launch (device labels are clamped into the table)."""
    _chk(x, "x"); _chk(table, "table")
    K, HW = table.shape
    B = x.numel() // HW
    if B < 1 or x.numel() != B * HW:
        raise _lib.PcgError(f"delta_cf_entry: x {tuple(x.shape)} is not rows of {HW} pixels")
    target = _targets(target, B, T, K)
    q0, nq = _window(B, T, q0, nq)
    out = out if out is not None else torch.empty((nq, HW, 2), dtype=torch.float32, device=x.device)
    if _chk(out, "out").numel() != nq * HW * 2:
        raise _lib.PcgError(f"delta_cf_entry: out holds {out.numel()} floats, {nq * HW * 2} needed")
    th, thp = _host_labels(target_host, "target_host")
    if th is not None and (target is None or th.numel() != B):
        raise _lib.PcgError(f"delta_cf_entry: target_host is the host copy of a target of {B} rows")
    a = _lib.DeltaCfEntryArgs(_p(x), _p(table), _p(target), thp, _p(out), B, int(T), HW, K, q0, nq)
    check(_lib.load().pcg_delta_cf_entry(ctypes.byref(a), _stream()), "pcg_delta_cf_entry")
    return out


def delta_cf_tail(delta, x, T=1, q0=0, nq=None, out=None):
    """pcg_delta_cf_tail: delta [nq, HW] of the window, x [B, HW] -> (x_cf [nq, HW] = clamp(x[b] + delta, -1, 1), sums [nq, 3] =
    sum |x_cf - x|, sum |delta|, sum (x_cf - x)^2); `out`: a dict of preallocated tensors under "x_cf" / "sums"."""
    _chk(delta, "delta"); _chk(x, "x")
    nq_d = delta.shape[0]
    HW = delta.numel() // nq_d
    B = x.numel() // HW
    if B < 1 or x.numel() != B * HW:
        raise _lib.PcgError(f"delta_cf_tail: x {tuple(x.shape)} is not rows of {HW} pixels")
    q0, nq = _window(B, T, q0, nq_d if nq is None else nq)
    if nq != nq_d:
        raise _lib.PcgError(f"delta holds {nq_d} queries, the window {nq}")
    out = out or {}
    res = []
    for name, shape in (("x_cf", (nq, HW)), ("sums", (nq, 3))):
        t = out.get(name)
        t = t if t is not None else torch.empty(shape, dtype=torch.float32, device=delta.device)
        if _chk(t, name).numel() != shape[0] * shape[1]:
            raise _lib.PcgError(f"out[{name!r}]: expected {shape[0] * shape[1]} values, got shape {tuple(t.shape)}")
        res.append(t)
    a = _lib.DeltaCfTailArgs(_p(delta), _p(x), _p(res[0]), _p(res[1]), B, int(T), HW, q0, nq)
    check(_lib.load().pcg_delta_cf_tail(ctypes.byref(a), _stream()), "pcg_delta_cf_tail")
    return res[0], res[1]


def delta_gan_target_draw(target, K, seed, offset=0, counter=None):
    """pcg_delta_gan_target_draw: ONE class in [0, K) -- out[0] of pcg_randint(out, 1, 0, K, NULL, seed, offset) -- written to every row
    of target [B] int64.  counter (int64[2] on the GPU, DeviceRNG.device_counter): the offset is counter[0] and the launch advances it
    by 1; `offset` is ignored then.  DeviceRNG.delta_gan_target keeps the host bookkeeping."""
    _chk_idx(target, K, "target")
    if counter is not None and (counter.dtype != torch.int64 or not counter.is_cuda or counter.numel() < 2 or not counter.is_contiguous()):
        raise _lib.PcgError("delta_gan_target_draw: counter must be int64[2] on the GPU (DeviceRNG.device_counter)")
    if target.numel() < 1 or int(K) < 1:
        raise _lib.PcgError(f"delta_gan_target_draw: {target.numel()} rows, {K} classes")
    a = _lib.DeltaGanTargetDrawArgs(_p(target), _p(counter), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, target.numel(), int(K))
    check(_lib.load().pcg_delta_gan_target_draw(ctypes.byref(a), _stream()), "pcg_delta_gan_target_draw")
    return target


def interpolate(alpha, real, fake):
    _chk(alpha, "alpha"); _chk(real, "real"); _chk(fake, "fake")
    B = alpha.numel()
    out = torch.empty_like(real)
    check(_lib.load().pcg_interpolate(_p(alpha), _p(real), _p(fake), _p(out), B, real.numel() // B, _stream()), "pcg_interpolate")
    return out


def interpolate_stack(alpha, real, fake):
    """[real | fake | alpha*real + (1-alpha)*fake] as one [3B, ...] tensor, one launch (the batched critic pass's input)."""
    _chk(alpha, "alpha"); _chk(real, "real"); _chk(fake, "fake")
    B = alpha.numel()
    assert real.shape == fake.shape and real.shape[0] == B
    x3 = torch.empty((3 * B,) + tuple(real.shape[1:]), dtype=torch.float32, device=real.device)
    check(_lib.load().pcg_interpolate_stack(_p(alpha), _p(real), _p(fake), _p(x3), B, real.numel() // B, _stream()), "pcg_interpolate_stack")
    return x3


def gradient_penalty_fwd(grads, B, lam):
    _chk(grads, "grads")
    norms = torch.empty(B, dtype=torch.float32, device=grads.device)
    pen = torch.empty(1, dtype=torch.float32, device=grads.device)
    check(_lib.load().pcg_gradient_penalty_fwd(_p(grads), B, grads.numel() // B, float(lam), _p(norms), _p(pen), _stream()),
          "pcg_gradient_penalty_fwd")
    return pen, norms


def gradient_penalty_bwd(grads, norms, grad_out, B, lam):
    dg = torch.empty_like(grads)
    check(_lib.load().pcg_gradient_penalty_bwd(_p(grads), _p(norms), _p(grad_out), B, grads.numel() // B, float(lam), _p(dg), _stream()),
          "pcg_gradient_penalty_bwd")
    return dg


# ---- device-side batch synthesis ---------------------------------------------------------------------------------
class DeviceRNG:
    """Counter-based stream: every draw advances `offset`, so a (seed, call sequence) pair is reproducible."""

    def __init__(self, seed=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.offset = 0

    def get_state(self):
        """{"seed", "offset"}: the whole stream position.  The graphed steppers advance device counters of their own and mirror them
        into `offset` after every replay, so this is the position at any point between two steps."""
        return {"seed": self.seed, "offset": self.offset}

    def set_state(self, state):
        """Continue the stream of get_state().  A device counter is made from `offset` when a stepper is built (device_counter), so
        restore the stream BEFORE building the stepper that draws from it."""
        seed, offset = int(state["seed"]), int(state["offset"])
        if offset < 0:
            raise _lib.PcgError(f"DeviceRNG.set_state: offset {offset}")
        self.seed, self.offset = seed & 0xFFFFFFFFFFFFFFFF, offset

    def _advance(self, n):
        # the Philox offset is a kernel ARGUMENT held on the host: a draw captured into a HIP graph would replay the same numbers
        # on every launch.  Draw outside the captured step and feed the result in as a static input (GraphedStep.load), or use the
        # device-counter form of the launch where there is one (house_draws(counter=...): the launch reads and advances the offset itself).
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.PcgError("DeviceRNG draw during HIP-graph capture: the captured kernel would replay identical random numbers; "
                                "draw before the step and pass the tensors in (GraphedStep inputs)")
        off = self.offset
        self.offset += int(n)
        return off

    def patch_mask(self, B, H, W, patch_size, num_selected, device):
        """build_mask (trainer.py:45-72) on the device: [B, 1, H, W] of {0, 1}."""
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
        check(_lib.load().pcg_patch_mask(_p(out), B, H, W, patch_size, num_selected, self.seed, self._advance(16 * B), _stream()),
              "pcg_patch_mask")
        return out

    def randint(self, low, high, n, device, exclude=None, out=None):
        out = out if out is not None else torch.empty((n,), dtype=torch.int64, device=device)
        check(_lib.load().pcg_randint(_p(out), n, low, high, _p(exclude), self.seed, self._advance((n + 3) // 4), _stream()),
              "pcg_randint")
        return out

    def delta_gan_target(self, target, K, counter=None):
        """The random-target iteration's ONE class (gan_train_copy.py:119-120) into every row of target [B]: the value
        randint(0, K, 1) gives at this offset.  counter None: the offset goes by value and the host offset advances by randint's span
        of one counter value.  counter (device_counter()): the launch reads and advances the device offset itself -- the form a HIP
        graph can capture; the host-side offset is not touched (see gan_train.GraphedTrainStep(rng=...))."""
        if counter is not None:
            return delta_gan_target_draw(target, K, self.seed, counter=counter)
        return delta_gan_target_draw(target, K, self.seed, offset=self._advance(1))

    def randn(self, shape, device, mean=0.0, std=1.0):
        out = torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        check(_lib.load().pcg_randn(_p(out), n, mean, std, self.seed, self._advance((n + 3) // 4), _stream()), "pcg_randn")
        return out

    def gumbel(self, shape, device, out=None):
        """Gumbel(0,1) noise, the draw F.gumbel_softmax makes (house_sales_kc_usa/models/generator.py:90)."""
        out = out if out is not None else torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        check(_lib.load().pcg_rand_gumbel(_p(out), n, self.seed, self._advance((n + 3) // 4), _stream()), "pcg_rand_gumbel")
        return out

    def house_draws(self, y, num_classes, D, T, zero_cols, out, onehots=None, counter=None):
        """target class != y, feature mask, Gumbel noise [B, T] in ONE launch, drawn into out = (target_y, mask, noise): the values
        randint(exclude=y), feature_mask, gumbel give when called in this order (same counter offsets).  onehots = (onehot(target_y),
        onehot(y)) float [B, num_classes] buffers: filled by the same launch.  counter: a device counter (device_counter()) that
        supplies the offsets and is advanced by the launch itself — the form a HIP graph can capture (every replay draws the next
        numbers of the stream); the host-side offset is not touched (see house.GraphedTrainStep(rng=...))."""
        o_t, o_m, o_n = out
        B = y.shape[0]
        nz = 0 if zero_cols is None else zero_cols.numel()
        oh_t, oh_y = onehots if onehots is not None else (None, None)
        if counter is not None:
            check(_lib.load().pcg_house_draws_counter(_p(o_t), B, num_classes, _p(y), _p(o_m), D, _p(zero_cols), nz, _p(o_n), T, self.seed,
                                                      _p(oh_t), _p(oh_y), _p(counter), _stream()), "pcg_house_draws_counter")
            return o_t, o_m, o_n
        off_t = self._advance((B + 3) // 4)
        off_m = self._advance((B * D + 3) // 4)
        off_n = self._advance((B * T + 3) // 4)
        check(_lib.load().pcg_house_draws(_p(o_t), B, num_classes, _p(y), off_t, _p(o_m), D, _p(zero_cols), nz, off_m, _p(o_n), T, off_n, self.seed,
                                          _p(oh_t), _p(oh_y), _stream()), "pcg_house_draws")
        return o_t, o_m, o_n

    def house_batch_draws(self, X, Y, perm, num_classes, T, zero_cols, out, onehots, counter, src_out=None):
        """house_draws(counter=...) that also takes the batch: rows perm[cursor .. cursor+B) of the resident training set (X [N, D]
        float32, Y [N] int64) are copied into out = (x, y, target_y, mask, noise), their source rows into src_out; the device counter
        (device_counter(device, cursor=True): int64[4] = [Philox offset, ticket, row cursor, 0]) is advanced by the launch."""
        o_x, o_y, o_t, o_m, o_n = out
        B, D = o_x.shape
        nz = 0 if zero_cols is None else zero_cols.numel()
        oh_t, oh_y = onehots if onehots is not None else (None, None)
        _chk(X, "X"); _chk(Y, "Y", torch.int64); _chk(perm, "perm", torch.int64)
        if counter.numel() < 4 or X.shape[1] != D or Y.numel() != X.shape[0] or perm.numel() < B:
            raise _lib.PcgError("house_batch_draws: counter must be int64[4] (device_counter(cursor=True)), X [N, D], Y [N], perm >= B entries")
        check(_lib.load().pcg_house_batch_draws_counter(_p(o_t), B, num_classes, _p(X), _p(Y), _p(perm), perm.numel(), X.shape[0], _p(o_x), _p(o_y),
                                                        _p(src_out), _p(o_m), D, _p(zero_cols), nz, _p(o_n), T, self.seed, _p(oh_t), _p(oh_y),
                                                        _p(counter), _stream()), "pcg_house_batch_draws_counter")
        return out

    def house_clf_batch(self, X, Y, perm, out, masks, keeps, counter=None, cursor=0):
        """The classifier fit's batch and its three Dropout masks in ONE launch: rows perm[cursor .. cursor+B) of the resident training
        set (X [N, D] float32, Y [N] int64) into out = (x [B, D], y [B]), and masks = (m0, m1, m2) ([B, width] each) with P(1) =
        keeps[i] -- the values three bernoulli() calls give in this order.  By value (counter None): `cursor` is the first row and the
        host offset advances.  counter (device_counter(device, cursor=True)): offset and cursor come from the device and the launch
        advances them itself -- the form a HIP graph can capture; the host-side offset is not touched."""
        o_x, o_y = out
        B, D = o_x.shape
        _chk(X, "X"); _chk(Y, "Y", torch.int64); _chk(perm, "perm", torch.int64); _chk(o_x, "x"); _chk(o_y, "y", torch.int64)
        if len(masks) != 3 or len(keeps) != 3 or any(_chk(m, "mask").dim() != 2 or m.shape[0] != B for m in masks):
            raise _lib.PcgError(f"house_clf_batch: three masks of {B} rows and three keep probabilities")
        if X.shape[1] != D or Y.numel() != X.shape[0] or o_y.numel() != B or perm.numel() < B:
            raise _lib.PcgError("house_clf_batch: X [N, D], Y [N], x [B, D], y [B], perm >= B entries")
        args = [a for m, k in zip(masks, keeps) for a in (_p(m), m.shape[1], float(k))]
        if counter is not None:
            if counter.numel() < 4 or counter.dtype != torch.int64 or not counter.is_cuda:
                raise _lib.PcgError("house_clf_batch: counter must be int64[4] on the device (device_counter(cursor=True))")
            check(_lib.load().pcg_house_clf_batch_counter(_p(X), _p(Y), _p(perm), perm.numel(), X.shape[0], _p(o_x), _p(o_y), B, D, *args, self.seed,
                                                          _p(counter), _stream()), "pcg_house_clf_batch_counter")
            return out, masks
        if cursor < 0 or cursor + B > perm.numel():
            raise _lib.PcgError(f"house_clf_batch: rows {cursor} .. +{B} of a permutation of {perm.numel()} entries")
        off = self._advance(self.house_clf_batch_span(B, [m.shape[1] for m in masks]))
        check(_lib.load().pcg_house_clf_batch(_p(X), _p(Y), _p(perm), perm.numel(), X.shape[0], _p(o_x), _p(o_y), B, D, *args, self.seed, off,
                                              int(cursor), _stream()), "pcg_house_clf_batch")
        return out, masks

    @staticmethod
    def house_clf_batch_span(B, widths):
        """Counter values one house_clf_batch call consumes."""
        return sum((B * w + 3) // 4 for w in widths)

    def mnist_clf_batch(self, X, Y, perm, out, masks, keeps, counter=None, cursor=0):
        """house_clf_batch with the MNIST classifier's TWO Dropout masks: rows perm[cursor .. cursor+B) of the resident set (X [N, D]
        float32, Y [N] int64) into out = (x [B, D], y [B]), and masks = (m0 [B, w0], m1 [B, w1]) with P(1) = keeps[i] -- the values
        two bernoulli() calls give in this order.  counter None: by value, the host offset advances; counter
        (device_counter(device, cursor=True)): offset and cursor live on the device and the launch advances them (capturable)."""
        o_x, o_y = out
        B, D = o_x.shape
        _chk(X, "X"); _chk(Y, "Y", torch.int64); _chk(perm, "perm", torch.int64); _chk(o_x, "x"); _chk(o_y, "y", torch.int64)
        if len(masks) != 2 or len(keeps) != 2 or any(_chk(m, "mask").dim() != 2 or m.shape[0] != B for m in masks):
            raise _lib.PcgError(f"mnist_clf_batch: two masks of {B} rows and two keep probabilities")
        if X.dim() != 2 or X.shape[1] != D or Y.numel() != X.shape[0] or o_y.numel() != B or perm.numel() < B:
            raise _lib.PcgError("mnist_clf_batch: X [N, D], Y [N], x [B, D], y [B], perm >= B entries")
        args = [a for m, k in zip(masks, keeps) for a in (_p(m), m.shape[1], float(k))]
        if counter is not None:
            if counter.numel() < 4 or counter.dtype != torch.int64 or not counter.is_cuda:
                raise _lib.PcgError("mnist_clf_batch: counter must be int64[4] on the device (device_counter(cursor=True))")
            check(_lib.load().pcg_mnist_clf_batch_counter(_p(X), _p(Y), _p(perm), perm.numel(), X.shape[0], _p(o_x), _p(o_y), B, D, *args, self.seed,
                                                          _p(counter), _stream()), "pcg_mnist_clf_batch_counter")
            return out, masks
        if cursor < 0 or cursor + B > perm.numel():
            raise _lib.PcgError(f"mnist_clf_batch: rows {cursor} .. +{B} of a permutation of {perm.numel()} entries")
        off = self._advance(self.mnist_clf_batch_span(B, [m.shape[1] for m in masks]))
        check(_lib.load().pcg_mnist_clf_batch(_p(X), _p(Y), _p(perm), perm.numel(), X.shape[0], _p(o_x), _p(o_y), B, D, *args, self.seed, off,
                                              int(cursor), _stream()), "pcg_mnist_clf_batch")
        return out, masks

    @staticmethod
    def mnist_clf_batch_span(B, widths):
        """Counter values one mnist_clf_batch call consumes."""
        return sum((B * w + 3) // 4 for w in widths)

    @staticmethod
    def house_draws_span(B, D, T):
        """Counter values one house_draws call consumes."""
        return (B + 3) // 4 + (B * D + 3) // 4 + (B * T + 3) // 4

    def device_counter(self, device, cursor=False):
        """int64[2] on the device: [this stream's current offset, ticket] — the counter argument of house_draws; cursor=True:
        int64[4] = [offset, ticket, row cursor, 0] for house_batch_draws."""
        return torch.tensor([self.offset, 0, 0, 0] if cursor else [self.offset, 0], dtype=torch.int64, device=device)

    def feature_mask(self, B, D, device, zero_cols=None, out=None):
        """Bernoulli(1/2) modifiable-feature mask with immutable columns zeroed (house_sales_kc_usa/trainer.py:253-255);
        zero_cols: int32 device tensor."""
        out = out if out is not None else torch.empty((B, D), dtype=torch.float32, device=device)
        nz = 0 if zero_cols is None else zero_cols.numel()
        check(_lib.load().pcg_feature_mask(_p(out), B, D, _p(zero_cols), nz, self.seed, self._advance((B * D + 3) // 4), _stream()),
              "pcg_feature_mask")
        return out

    def rand(self, shape, device):
        """torch.rand: uniform [0, 1) (WGAN-GP interpolation coefficients, mnist_wgan_conditional.py:146)."""
        out = torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        check(_lib.load().pcg_rand_uniform(_p(out), n, self.seed, self._advance((n + 3) // 4), _stream()), "pcg_rand_uniform")
        return out

    def bernoulli(self, shape, device, keep_prob):
        """0/1 mask with P(1) = keep_prob — the noise nn.Dropout / nn.Dropout2d draw."""
        out = torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        check(_lib.load().pcg_rand_bernoulli(_p(out), n, float(keep_prob), self.seed, self._advance((n + 3) // 4), _stream()),
              "pcg_rand_bernoulli")
        return out


def tune(name, value):
    """A/B switch of a launch-planning choice (pcg_tune_set): 'korder', 'wgrad_order', 'dgrad_interleave', 'wgrad_pixtab', ...; -1 = built-in."""
    check(_lib.load().pcg_tune_set(name.encode(), int(value)), "pcg_tune_set")


# ---- calibration (bench lines; not on the step's path) -------------------------------------------------------------------
def calibrate(device, mfma_ms=20.0, copy_mb=512, rounds=2, warm_ms=30.0):
    """What this box's fp32 matrix pipe and HBM sustain NOW: {"mfma_tflops", "mfma_clock_mhz", "hbm_gbs", ...}.

    A bare v_mfma_f32_32x32x2_f32 loop on every CU for ~mfma_ms (pcg_calib_mfma; the in-kernel shader clock comes from its
    s_memtime / s_memrealtime stamps) and a copy_mb-MiB device copy (pcg_calib_copy), each timed with events on the current
    stream.  bench.py runs it before and after the timed steps, outside the timed bracket, so that a step measured on a box
    with a slower clock can be told from a slower kernel (roofline.achieved / calib.mfma_tflops is box-independent)."""
    lib = _lib.load()
    nbytes = lib.pcg_calib_mfma_workspace_bytes(rounds)
    blocks = lib.pcg_calib_mfma_blocks(rounds)
    if blocks <= 0:
        raise _lib.PcgError("calibrate: no GPU visible to libpcgan_hip")
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    ws[:8192].view(torch.float32).copy_(torch.linspace(-1.0, 1.0, 2048))
    flop = ctypes.c_double(0.0)
    stamps = ctypes.c_uint64(0)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(iters):
        e[0].record()
        check(lib.pcg_calib_mfma(int(iters), rounds, _p(ws), nbytes, ctypes.byref(flop), ctypes.byref(stamps), _stream()), "pcg_calib_mfma")
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1])

    probe_iters = 2048
    run(probe_iters)                                   # code object load, clocks up
    ms = run(probe_iters)
    iters = max(probe_iters, int(probe_iters * mfma_ms / max(ms, 1e-3)))
    if warm_ms > 0:                                    # untimed: the reading that follows is not a cold-clock one (r03: "before" read
        run(int(iters * warm_ms / mfma_ms))            # 2273 MHz against 2365 after the timed steps)
    ms = run(iters)
    st = ws[8192 + blocks * 1024:].view(torch.int64).view(blocks, 2).cpu().double()
    mhz = (st[:, 0] / st[:, 1].clamp_min(1.0) * 100.0)
    out = {"mfma_tflops": round(flop.value / (ms * 1e-3) / 1e12, 2), "mfma_ms": round(ms, 3),
           "mfma_clock_mhz": round(float(mhz.median()), 0), "mfma_clock_mhz_min": round(float(mhz.min()), 0),
           "mfma_cycles_per_inst": round(float((st[:, 0] / (iters * 16.0)).median()), 2)}
    n = int(copy_mb) << 20
    src = torch.empty(n, dtype=torch.uint8, device=device)
    dst = torch.empty(n, dtype=torch.uint8, device=device)
    fill(src.view(torch.float32), 1.0)
    times = []
    for _ in range(4):
        e[0].record()
        check(lib.pcg_calib_copy(_p(src), _p(dst), n, _stream()), "pcg_calib_copy")
        e[1].record()
        e[1].synchronize()
        times.append(e[0].elapsed_time(e[1]))
    out["hbm_gbs"] = round(2.0 * n / (min(times[1:]) * 1e-3) / 1e9, 1)
    return out


# ---- MNIST CounteRGAN: prompted queries and per-target evaluation (csrc/mnist_cf_eval.hip) ------------------------
MASK_MODES = {"shared": _lib.MASK_SHARED, "row": _lib.MASK_PER_ROW, "query": _lib.MASK_PER_QUERY}


def _mask_mode(mask, mode, B, T, HW):
    """The PCG_MASK_* code of `mode`, after checking that `mask` holds what that mode reads."""
    if mode not in MASK_MODES:
        raise _lib.PcgError(f"mask_mode {mode!r} is not one of {sorted(MASK_MODES)}")
    want = {"shared": HW, "row": B * HW, "query": T * B * HW}[mode]
    _chk(mask, "mask")
    if mask.numel() != want:
        raise _lib.PcgError(f"mask: mask_mode {mode!r} reads {want} values ({B} rows x {T} targets of {HW} pixels), got shape {tuple(mask.shape)}")
    return MASK_MODES[mode]


def _window(B, T, q0, nq):
    nq = T * B - q0 if nq is None else nq
    if q0 < 0 or nq < 1 or q0 + nq > T * B:
        raise _lib.PcgError(f"query window [{q0}, {q0} + {nq}) is not inside the {T} x {B} queries")
    return int(q0), int(nq)


def _targets(target, B, T, K):
    if target is None:
        if not 1 <= T <= K:
            raise _lib.PcgError(f"the sweep form takes 1 <= T <= {K} target classes, got {T}")
        return None
    _chk_idx(target, K, "target")
    if T != 1 or target.numel() != B:
        raise _lib.PcgError(f"the per-row form takes T = 1 and one target per row ({B}), got T = {T} and {target.numel()} targets")
    return target


def patch_mask_bits(bits, H, W, ps):
    """bits [n] int64 on the GPU (bit p = patch p is modifiable) -> masks [n, 1, H, W] of whole ps x ps patches."""
    _chk(bits, "bits", torch.int64)
    n = bits.numel()
    if ps < 1 or H // ps < 1 or W // ps < 1:
        raise _lib.PcgError(f"patch size {ps} gives no patch on a {H} x {W} image")
    mask = torch.empty((n, 1, H, W), dtype=torch.float32, device=bits.device)
    a = _lib.PatchMaskBitsArgs(bits.data_ptr(), mask.data_ptr(), n, H, W, ps)
    check(_lib.load().pcg_patch_mask_bits(ctypes.byref(a), _stream()), "pcg_patch_mask_bits")
    return mask


def mnist_cf_entry(x, target, table, mask, mask_mode, T=1, q0=0, nq=None):
    """[nq, HW, 3] with channels (x[b], table[target(q)], mask[row(q)]) for the queries q = t * B + b of the window; x [B, HW]."""
    _chk(x, "x"); _chk(table, "table")
    K, HW = table.shape
    B = x.numel() // HW
    target = _targets(target, B, T, K)
    mode = _mask_mode(mask, mask_mode, B, T, HW)
    q0, nq = _window(B, T, q0, nq)
    out = torch.empty((nq, HW, 3), dtype=torch.float32, device=x.device)
    a = _lib.MnistCfEntryArgs(x.data_ptr(), table.data_ptr(), mask.data_ptr(), target.data_ptr() if target is not None else None,
                              out.data_ptr(), B, T, HW, K, mode, q0, nq)
    check(_lib.load().pcg_mnist_cf_entry(ctypes.byref(a), _stream()), "pcg_mnist_cf_entry")
    return out


def mnist_cf_tail(c, x, mask, mask_mode, scale, T=1, q0=0, nq=None, want_residuals=True, out=None):
    """conv_out's result c [nq, HW] -> (x_cf [nq, HW], raw, masked ([nq, HW] or None), sums [nq, 3]); `out`: a dict of preallocated
    tensors under those names (a given "raw" / "masked" is written whatever want_residuals says)."""
    _chk(c, "c"); _chk(x, "x")
    nq_c = c.shape[0]
    HW = c.numel() // nq_c
    B = x.numel() // HW
    mode = _mask_mode(mask, mask_mode, B, T, HW)
    q0, nq = _window(B, T, q0, nq_c if nq is None else nq)
    if nq != nq_c:
        raise _lib.PcgError(f"c holds {nq_c} queries, the window {nq}")
    out = dict(out or {})

    def buf(name, shape, need=True):
        t = out.get(name)
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=c.device) if need else None
        _chk(t, name)
        if t.numel() != shape[0] * shape[1]:
            raise _lib.PcgError(f"out[{name!r}]: expected {shape[0] * shape[1]} values, got shape {tuple(t.shape)}")
        return t
    x_cf, sums = buf("x_cf", (nq, HW)), buf("sums", (nq, 3))
    raw, masked = buf("raw", (nq, HW), want_residuals), buf("masked", (nq, HW), want_residuals)
    a = _lib.MnistCfTailArgs(c.data_ptr(), x.data_ptr(), mask.data_ptr(), x_cf.data_ptr(), raw.data_ptr() if raw is not None else None,
                             masked.data_ptr() if masked is not None else None, sums.data_ptr(), float(scale), B, T, HW, mode, q0, nq)
    check(_lib.load().pcg_mnist_cf_tail(ctypes.byref(a), _stream()), "pcg_mnist_cf_tail")
    return x_cf, raw, masked, sums


SCORE_FIELDS = ("pred", "conf", "p_target", "p_true", "p_orig_true", "flip")


def mnist_cf_score(logits_cf, K, B, T=1, target=None, y_true=None, logits_orig=None, tail_sums=None, group_rows=None, q0=0, nq=None,
                   outputs=SCORE_FIELDS, group_sums=True):
    """logits_cf [nq, ld] (ld >= K) -> {name: [nq] tensor for name in outputs} (+ "group_sums" [T, ceil(B / group_rows), 8])."""
    _chk(logits_cf, "logits_cf")
    nq_l, ld = logits_cf.shape
    target = _targets(target, B, T, K)
    q0, nq = _window(B, T, q0, nq_l if nq is None else nq)
    if nq != nq_l:
        raise _lib.PcgError(f"logits_cf holds {nq_l} queries, the window {nq}")
    if y_true is not None and (_chk_idx(y_true, K, "y_true").numel() != B):
        raise _lib.PcgError(f"y_true: expected {B} labels, got {y_true.numel()}")
    if logits_orig is not None and (tuple(_chk(logits_orig, "logits_orig").shape) != (B, ld) or y_true is None):
        raise _lib.PcgError(f"logits_orig: expected [{B}, {ld}] and y_true, got {tuple(logits_orig.shape)}")
    if tail_sums is not None and _chk(tail_sums, "tail_sums").numel() != nq * 3:
        raise _lib.PcgError(f"tail_sums: expected [{nq}, 3], got {tuple(tail_sums.shape)}")
    group_rows = B if group_rows is None else int(group_rows)
    if group_rows < 1:
        raise _lib.PcgError(f"group_rows {group_rows}")
    dev = logits_cf.device
    res = {n: torch.empty(nq, dtype=torch.int64 if n == "pred" else torch.float32, device=dev) for n in outputs}
    if group_sums:
        res["group_sums"] = torch.empty((T, (B + group_rows - 1) // group_rows, _lib.MNIST_CF_GROUP_SUMS), dtype=torch.float32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
    a = _lib.MnistCfScoreArgs(logits_cf.data_ptr(), ptr(logits_orig), ptr(target), ptr(y_true), ptr(tail_sums),
                              *(ptr(res.get(n)) for n in SCORE_FIELDS), ptr(res.get("group_sums")), B, T, K, ld, group_rows, q0, nq)
    check(_lib.load().pcg_mnist_cf_score(ctypes.byref(a), _stream()), "pcg_mnist_cf_score")
    return res


# ---- MNIST CounteRGAN: the report figures' numbers and pixels (csrc/cf_report.hip) --------------------------------
PICK_MODES = {"first": _lib.CLASS_PICK_FIRST, "best": _lib.CLASS_PICK_BEST}
PICK_MAX_ROW = (1 << 32) - 1          # rows must stay below this: a key holds 0xFFFFFFFF - row


def _pick_mode(mode, K):
    if mode not in PICK_MODES:
        raise _lib.PcgError(f"mode {mode!r} is not one of {sorted(PICK_MODES)}")
    if not 1 <= int(K) <= _lib.CLASS_PICK_KMAX:
        raise _lib.PcgError(f"K {K} is outside [1, {_lib.CLASS_PICK_KMAX}]")
    return PICK_MODES[mode]


def class_pick_state(K, device):
    """The zeroed uint64 [K] state of a pick, held as int64 (the same bits)."""
    _pick_mode("first", K)
    return torch.zeros(int(K), dtype=torch.int64, device=device)


def class_pick(state, labels, K, row0=0, logits=None, mode="first"):
    """Folds one chunk — labels [n] int64 and, in "best" mode, logits [n, kp] — whose first row is the data set's row `row0` into
    state (class_pick_state): per class the maximum of (confidence bits << 32) | (0xFFFFFFFF - row).  Returns state."""
    code = _pick_mode(mode, K)
    _chk(state, "state", torch.int64)
    if state.numel() != K:
        raise _lib.PcgError(f"state: expected {K} words, got shape {tuple(state.shape)}")
    _chk_idx(labels, K, "labels")
    n, kp = labels.numel(), 0
    if n < 1 or labels.dim() != 1:
        raise _lib.PcgError(f"labels: expected [n] with n >= 1, got shape {tuple(labels.shape)}")
    row0 = int(row0)
    if row0 < 0 or row0 + n > PICK_MAX_ROW:
        raise _lib.PcgError(f"rows [{row0}, {row0} + {n}) do not stay below 2^32 - 1")
    if mode == "best":
        if logits is None:
            raise _lib.PcgError("mode 'best' reads the classifier's logits")
        _chk(logits, "logits")
        kp = logits.shape[-1]
        if logits.dim() != 2 or logits.shape[0] != n or kp < K or kp % 4:
            raise _lib.PcgError(f"logits: expected [{n}, kp] with kp >= {K} a multiple of 4, got {tuple(logits.shape)}")
    check(_lib.load().pcg_class_pick(_p(logits) if mode == "best" else None, _p(labels), _p(state), n, kp, int(K), row0, code, _stream()),
          "pcg_class_pick")
    return state


def class_pick_gather(state, K, mode="first", X=None):
    """state -> (rows [K] int64, -1 for a class without a row; conf [K], 0 in "first" mode; sources [K, HW] = X[rows] for a data set
    X [N, HW] resident on the GPU, else None)."""
    code = _pick_mode(mode, K)
    _chk(state, "state", torch.int64)
    if state.numel() != K:
        raise _lib.PcgError(f"state: expected {K} words, got shape {tuple(state.shape)}")
    dev = state.device
    rows, conf = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.float32, device=dev)
    sources, N, HW = None, 0, 0
    if X is not None:
        _chk(X, "X")
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise _lib.PcgError(f"X: expected [N, HW], got {tuple(X.shape)}")
        N, HW = X.shape
        sources = torch.empty((K, HW), dtype=torch.float32, device=dev)
    check(_lib.load().pcg_class_pick_gather(_p(state), _p(X), _p(rows), _p(conf), _p(sources), int(K), int(N), int(HW), code, _stream()),
          "pcg_class_pick_gather")
    return rows, conf, sources


def cf_panels(x, x_cf, H, W, mask=None, mode="panels"):
    """mode "grid": x = sources [K, HW], x_cf [T, K, HW] -> (image [K*H, T*W] float in [0, 1], the same image as uint8).
    mode "panels": x, x_cf [n, HW], mask [HW] (shared) or [n, HW] -> (panels [n, 4, H, W] = (x + 1) / 2, (x_cf + 1) / 2, their
    |difference|, mask; vmax [1], the maximum of the third panel)."""
    _chk(x, "x"); _chk(x_cf, "x_cf")
    H, W = int(H), int(W)
    HW = H * W
    if H < 1 or W < 1 or x.dim() != 2 or x.shape[1] != HW:
        raise _lib.PcgError(f"x: expected [n, {H} * {W}], got {tuple(x.shape)}")
    n, dev = x.shape[0], x.device
    lib = _lib.load()
    if mode == "grid":
        if x_cf.dim() != 3 or x_cf.shape[1] != n or x_cf.shape[2] != HW:
            raise _lib.PcgError(f"x_cf: expected [T, {n}, {HW}] ([target][row]), got {tuple(x_cf.shape)}")
        T = x_cf.shape[0]
        image = torch.empty((n * H, T * W), dtype=torch.float32, device=dev)
        image_u8 = torch.empty((n * H, T * W), dtype=torch.uint8, device=dev)
        check(lib.pcg_cf_panels(_lib.CF_PANELS_GRID, _p(x), _p(x_cf), None, 0, _p(image), _p(image_u8), None, n, T, H, W, _stream()),
              "pcg_cf_panels")
        return image, image_u8
    if mode != "panels":
        raise _lib.PcgError(f"mode {mode!r} is not 'grid' or 'panels'")
    if tuple(x_cf.shape) != (n, HW):
        raise _lib.PcgError(f"x_cf: expected [{n}, {HW}], got {tuple(x_cf.shape)}")
    if mask is None:
        raise _lib.PcgError("mode 'panels' takes a mask")
    _chk(mask, "mask")
    if mask.numel() not in (HW, n * HW):
        raise _lib.PcgError(f"mask: expected {HW} (shared) or {n * HW} (per row) values, got shape {tuple(mask.shape)}")
    mm = _lib.MASK_SHARED if mask.numel() == HW else _lib.MASK_PER_ROW
    panels = torch.empty((n, 4, H, W), dtype=torch.float32, device=dev)
    vmax = torch.empty(1, dtype=torch.float32, device=dev)
    fill(vmax, 0.0)
    check(lib.pcg_cf_panels(_lib.CF_PANELS_PANELS, _p(x), _p(x_cf), _p(mask), mm, _p(panels), None, _p(vmax), n, 1, H, W, _stream()),
          "pcg_cf_panels")
    return panels, vmax
