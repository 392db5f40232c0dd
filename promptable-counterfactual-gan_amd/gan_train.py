"""Host-side mirror of `conditional_counteRGAN/mnist/gan_train.py` -- the additive-delta CounteRGAN of the shipped models/classifier.pt
and the outputs3/ pictures -- on the HIP kernels.

    reference                                              here
    ---------------------------------------------------    -----------------------------------------------------
    gan_train.py           params            :17-30         params (without the directories)
    modules/generator.py   Generator         :4-22          Generator (same ctor args, same state_dict keys)
    modules/discriminator.py Discriminator   :4-23          Discriminator
    gan_train.py           the classifier    :49-100        countergan.get_pool_classifier / load_classifier; frozen, eval
    gan_train.py           optimizers        :106-110       make_optimizers
    gan_train.py           loop body         :117-144       train_step (op chain) / GraphedTrainStep (fused, one graph replay)
    gan_train.py           loop              :115-148       train_gan
    gan_train.py           test pictures     :150-159       counterfactual_batch
    gan_train_copy.py      params            :17-29         params_random_target (no target_class: a random class per iteration)
    gan_train_copy.py      the class draw    :119-120       ops.DeviceRNG.delta_gan_target (train_gan / GraphedTrainStep(rng=...))
    gan_train_copy.py      prompted queries  :161-172       counterfactuals, counterfactual_sweep, evaluate_examples
    eval_utils.py          per-target means  :58-66,:97-102 evaluate_per_target

The torch layer objects are kept as parameter containers (`label_embed`, and `net`, the reference's nn.Sequential layer for layer), so
`state_dict()` keys and shapes are the reference's in both directions with strict=True.  Forward and backward are one autograd node per
network sequencing C-ABI calls on NHWC activations (csrc/delta_gan.hip holds the fused launches around the convolutions; DESIGN.md
§3.19; csrc/delta_cf_eval.hip the query windows and the class draw, §3.20)."""
import os

import torch
import torch.nn as nn

from . import checkpoint as _ckpt
from . import ops
from . import sheets
from ._graphed import Held, capture_steps
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, PcgError
from .countergan import (PER_CLASS_FIELDS, BCEWithLogitsLoss, Classifier, CrossEntropyLoss, _as_rows, _conv_fwd, _conv_wgrad, _dgrad_act, _geom,
                         _grid_report, _labels, _padded_logits, abs_mean, metrics_from_sums, pick_sources)
from .data import DeviceLoader
from .nn import FlatModule, in_conv_precision, linear_dgrad, linear_fwd, linear_wgrad, weighted_sum
from .optim import Adam

params = {                                             # gan_train.py:17-30
    "batch_size": 128,
    "epochs_clf": 10,
    "epochs_gan": 40,
    "lr_G": 1e-3,
    "lr_D": 1e-3,
    "lr_C": 1e-3,
    "lambda_cls": 3.0,
    "lambda_reg": 0.05,
    "target_class": 5,
    "device": "cuda",
}

params_random_target = {                               # gan_train_copy.py:17-29; no target_class: train_gan draws one per iteration (:119)
    "batch_size": 128,
    "epochs_clf": 10,
    "epochs_gan": 50,
    "lr_G": 5e-5,
    "lr_D": 1e-5,
    "lr_C": 1e-3,
    "lambda_cls": 2.0,
    "lambda_reg": 0.01,
    "device": "cuda",
}

H = W = 28
HW = H * W


def _need_gpu(t, who):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise PcgError(f"{who}: input is on {getattr(t, 'device', type(t))}; libpcgan_hip has no CPU path")


def _label_channel_grad(net, conv, g, d, idx, table):
    """The entry convolution's grad-input for the label-map channel alone (of its two input channels only that one has a consumer, the
    embedding table) and the table's gradient: 9 tap products per pixel instead of 18."""
    g1 = ops.conv_geom(g.B, g.IH, g.IW, 1, g.Cout, g.KH, g.KW, g.stride, g.pad)
    d1 = ops.conv2d_dgrad(g1, d, ops.gather_channel(ops.ohwi(conv.weight.data), 1))
    ge, acc = net._grad_view(table.weight)
    ops.embed_table_grad(d1, idx, 1, 0, table.num_embeddings, ge, accumulate=acc)


# ---- generator --------------------------------------------------------------------------------------------------------------------------
class _GFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, c, *weights):
        x_cf, delta, saved = net._run_forward(x, c)
        ctx.net, ctx.saved = net, saved
        return x_cf, delta

    @staticmethod
    def backward(ctx, d_xcf, d_delta):
        ctx.net._run_backward(ctx.saved, d_xcf, d_delta)
        return (None,) * len(ctx.needs_input_grad)


class Generator(FlatModule):
    """modules/generator.py:4-22 -- returns (x + delta, delta)."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, HW)
        self.net = nn.Sequential(
            nn.Conv2d(2, 64, kernel_size=3, padding=1), nn.ReLU(),
            nn.Conv2d(64, 64, kernel_size=3, padding=1), nn.ReLU(),
            nn.Conv2d(64, 32, kernel_size=3, padding=1), nn.ReLU(),
            nn.Conv2d(32, 1, kernel_size=3, padding=1),
        )

    def _convs(self):
        return [m for m in self.net if isinstance(m, nn.Conv2d)]

    def forward(self, x, c):
        _need_gpu(x, "Generator")
        self._ensure_flat()
        c = c.to(x.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _GFn.apply(self, x, c, *self.parameters())
        x_cf, delta, _ = self._run_forward(x, c, keep=False)
        return x_cf, delta

    @in_conv_precision
    def _run_forward(self, x, c, keep=True):
        B = x.shape[0]
        xr = _as_rows(x, B)
        a = ops.embed_concat_fwd(xr, c, self.label_embed.weight.data, None).view(B, H, W, 2)      # :19-20
        convs, layers = self._convs(), []
        for i, conv in enumerate(convs):
            g, z = _conv_fwd(conv, a, ACT_RELU if i + 1 < len(convs) else ACT_NONE)
            layers.append((g, a))
            a = z
        delta = a.view(B, HW)
        x_cf = ops.axpby(1.0, xr, 1.0, delta)                                                       # :22
        return x_cf.view(B, 1, H, W), delta.view(B, 1, H, W), ((layers, c) if keep else None)

    @in_conv_precision
    def forward_queries(self, x_rows, target, T=None, q0=0, nq=None, out=None):
        """The forward over the window [q0, q0 + nq) of the queries q = t * B + b, clamped as gan_train_copy.py:165-166 clamps it.
        x_rows [B, 784] (or [B,1,28,28]); target None: the sweep, query (t, b) asks for class t of T (default num_classes), or [B]
        int64 on the GPU with T = 1 -- x is never replicated.  One entry launch, the four convolutions on nq rows, one tail launch.
        Returns {"x_cf" [nq, 784], "delta" [nq, 784], "sums" [nq, 3]: sum |x_cf - x|, sum |delta|, sum (x_cf - x)^2}; `out`:
        preallocated tensors under those names."""
        _need_gpu(x_rows, "Generator.forward_queries")
        self._ensure_flat()
        B = x_rows.shape[0]
        xr = _as_rows(x_rows, B)
        if xr.shape[1] != HW:
            raise PcgError(f"Generator.forward_queries: expected {HW} pixels per row, got shape {tuple(x_rows.shape)}")
        T = (self.label_embed.num_embeddings if target is None else 1) if T is None else int(T)
        out = out or {}
        a = ops.delta_cf_entry(xr, target, self.label_embed.weight.data, T, q0, nq)                # generator.py:19-20
        n = a.shape[0]
        a = a.view(n, H, W, 2)
        convs = self._convs()
        for i, conv in enumerate(convs):
            last = i + 1 == len(convs)
            dst = out.get("delta") if last else None
            a = ops.conv2d_fwd(_geom(conv, n, H, W), a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_NONE if last else ACT_RELU,
                               out=dst.view(n, H, W, 1) if dst is not None else None)
        delta = a.view(n, HW)
        x_cf, sums = ops.delta_cf_tail(delta, xr, T, q0, n, out=out)                                # gan_train_copy.py:165-166
        return {"x_cf": x_cf, "delta": delta, "sums": sums}

    @in_conv_precision
    def _run_backward(self, saved, d_xcf, d_delta):
        layers, c = saved
        if d_xcf is None and d_delta is None:
            return
        if d_xcf is not None and d_delta is not None:
            d = ops.axpby(1.0, d_xcf.contiguous(), 1.0, d_delta.contiguous())
        else:
            d = (d_xcf if d_xcf is not None else d_delta).contiguous()
        convs = self._convs()
        for i in range(len(convs) - 1, -1, -1):
            g, a = layers[i]
            d = d.view(g.B, g.OH, g.OW, g.Cout)
            _conv_wgrad(self, convs[i], g, a, d, True)
            if i > 0:
                d = _dgrad_act(g, d, ops.ohwi(convs[i].weight.data), a, ACT_RELU, 0.0)
        _label_channel_grad(self, convs[0], layers[0][0], d, c, self.label_embed)


# ---- discriminator ----------------------------------------------------------------------------------------------------------------------
class _DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, c, *weights):
        out, saved = net._run_forward(x, c)
        ctx.net, ctx.saved = net, saved
        return out

    @staticmethod
    def backward(ctx, dlogits):
        dx = ctx.net._run_backward(ctx.saved, dlogits, ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:]))
        return (None, dx) + (None,) * (len(ctx.needs_input_grad) - 2)


class Discriminator(FlatModule):
    """modules/discriminator.py:4-23 -- logits [B, 1]; there is no sigmoid."""

    SLOPE = 0.2

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, HW)
        self.net = nn.Sequential(
            nn.Conv2d(2, 64, 3, stride=2, padding=1), nn.LeakyReLU(0.2),
            nn.Conv2d(64, 128, 3, stride=2, padding=1), nn.LeakyReLU(0.2),
            nn.Conv2d(128, 256, 3, stride=1, padding=1), nn.LeakyReLU(0.2),
            nn.Flatten(),
            nn.Linear(256 * 7 * 7, 1),
        )

    def _convs(self):
        return [m for m in self.net if isinstance(m, nn.Conv2d)]

    def forward(self, x, c):
        _need_gpu(x, "Discriminator")
        self._ensure_flat()
        c = c.to(x.device)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _DFn.apply(self, x, c, *self.parameters())
        return self._run_forward(x, c, keep=False)[0]

    @in_conv_precision
    def _run_forward(self, x, c, keep=True):
        B = x.shape[0]
        a = ops.embed_concat_fwd(_as_rows(x, B), c, self.label_embed.weight.data, None).view(B, H, W, 2)   # :21-22
        layers = []
        for conv in self._convs():
            g, z = _conv_fwd(conv, a, ACT_LRELU, self.SLOPE)
            layers.append((g, a, z))
            a = z
        hw, ch = a.shape[1] * a.shape[2], a.shape[3]
        flat = ops.nhwc_to_nchw_flat(a, B, hw, ch).view(B, hw * ch)                   # nn.Flatten of the NCHW tensor: net.7's own column order
        logits = linear_fwd(self.net[7], flat).view(B, 1)
        return logits, ((layers, flat, (hw, ch), c) if keep else None)

    @in_conv_precision
    def _run_backward(self, saved, dlogits, need_x, need_p):
        layers, flat, (hw, ch), c = saved
        B = flat.shape[0]
        lin = self.net[7]
        dl = dlogits.contiguous()
        if need_p:
            linear_wgrad(self, lin, flat, dl)
        d = linear_dgrad(lin.weight.data, dl, B)
        d = ops.nhwc_to_nchw_flat(d, B, hw, ch, inverse=True).view(layers[-1][2].shape)
        ops.act_bwd(d, layers[-1][2], ACT_LRELU, self.SLOPE, out=d)
        convs = self._convs()
        for i in range(len(convs) - 1, 0, -1):
            g, a, _ = layers[i]
            _conv_wgrad(self, convs[i], g, a, d, need_p)      # need_p False (the G step): D's weight gradients are dead, zero_grad clears them unread
            d = _dgrad_act(g, d, ops.ohwi(convs[i].weight.data), a, ACT_LRELU, self.SLOPE)
        g, a, _ = layers[0]
        _conv_wgrad(self, convs[0], g, a, d, need_p)
        w = ops.ohwi(convs[0].weight.data)
        if need_x and not need_p:
            # D(x_cf) in the G step: of the entry conv's two input channels only the image has a consumer
            g1 = ops.conv_geom(g.B, g.IH, g.IW, 1, g.Cout, g.KH, g.KW, g.stride, g.pad)
            return ops.conv2d_dgrad(g1, d, ops.gather_channel(w, 0)).view(B, 1, H, W)
        if not need_x:
            if need_p:                                          # D(real) / D(fake.detach()): only the label map has a consumer
                _label_channel_grad(self, convs[0], g, d, c, self.label_embed)
            return None
        ge, acc = self._grad_view(self.label_embed.weight)
        dx = ops.embed_concat_bwd(ops.conv2d_dgrad(g, d, w), c, 2, self.label_embed.num_embeddings, dtable=ge, accumulate=acc, need_dx=True)
        return dx.view(B, 1, H, W)


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
def make_optimizers(G, D, params=params):
    """gan_train.py:106-107 (the two losses of :109-110 are built where they are used)."""
    return Adam(G.parameters(), lr=params["lr_G"]), Adam(D.parameters(), lr=params["lr_D"])


def _check_classifier(C):
    if not isinstance(C, Classifier) or C.training:
        raise PcgError("the classifier must be a countergan.Classifier in eval mode (gan_train.py:49-100 leaves it loaded, frozen, eval)")


def train_step(G, D, C, opt_g, opt_d, x, y, target, params=params):
    """One iteration of gan_train.py:117-144 for a batch already on the GPU, as the op chain on the library's entries; `target` (:119)
    is passed in.  Returns the device scalars {loss_D, loss_G, loss_adv, loss_cls, loss_reg}; the reference's .item() calls are the
    caller's.  G(x, target) of :122 and of :133 is one forward (see GraphedTrainStep, restructuring 1); D's weight gradients in the G
    step are not formed (restructuring 3)."""
    _need_gpu(x, "train_step")
    _check_classifier(C)
    bce, ce = BCEWithLogitsLoss(), CrossEntropyLoss()                                  # :109-110
    x_cf, delta = G(x, target)                                                         # :122 == :133
    # Discriminator
    d_real = D(x, y)                                                                   # :123
    d_fake = D(x_cf.detach(), target)                                                  # :124
    loss_D = weighted_sum([bce(d_real, 1.0), bce(d_fake, 0.0)], [1.0, 1.0])            # :125-127
    opt_d.zero_grad()                                                                  # :128
    loss_D.backward()                                                                  # :129
    opt_d.step()                                                                       # :130
    # Generator
    for p in D.parameters():
        p.requires_grad_(False)
    try:
        d_fake = D(x_cf, target)                                                       # :134
        cls_pred = C(x_cf)                                                             # :135
        loss_adv = bce(d_fake, 1.0)                                                    # :137
        loss_cls = ce(cls_pred, target)                                                # :138
        loss_reg = abs_mean(delta)                                                     # :139
        loss_G = weighted_sum([loss_adv, loss_cls, loss_reg], [1.0, params["lambda_cls"], params["lambda_reg"]])   # :141
        opt_g.zero_grad()                                                              # :142
        loss_G.backward()                                                              # :143
    finally:
        for p in D.parameters():
            p.requires_grad_(True)
    opt_g.step()                                                                       # :144
    return {"loss_D": loss_D.detach(), "loss_G": loss_G.detach(), "loss_adv": loss_adv.detach(), "loss_cls": loss_cls.detach(),
            "loss_reg": loss_reg.detach()}


class GraphedTrainStep:
    """The iteration of gan_train.py:117-144 on the fused launches of csrc/delta_gan.hip around the library's convolutions, captured
    once per batch size as a single-stream, strictly linear HIP graph: a step is two small copies (the batch into the graph's input
    rows) and one replay.  One graph per batch size actually met (the full batch and the loader's tail; a tail of one row is valid:
    there is no BatchNorm).  Gradients are overwritten every step: there is no zero_grad.  graph=False calls the same entries
    eagerly, which is what the replays equal bit for bit.

    Three restructurings, none of which changes a number beyond the order of fp32 sums:
      1. G's forward runs once.  G(x, target) at :122 and at :133 read the same weights -- Adam(G), :144, comes after both -- so the
         two calls return the same bits; the one forward's saved activations serve the backward of :143.
      2. D(x, y) and D(x_cf.detach(), target) (:123-124) are one pass of 2B rows.  D has no BatchNorm, so a row's logit depends on that
         row alone; only the weight and bias gradients add the two halves' contributions in one sum instead of two.  D's pass of the G
         step (:134) is a fresh forward of the B fake rows after Adam(D) (:130), with its label channel regathered from the updated
         D.label_embed table.
      3. Dead work is skipped.  D's weight gradients of the G step (:143) are cleared by optimizer_D.zero_grad() (:128) before anyone
         reads them, so they are not formed.  At an entry convolution only one input channel has a consumer -- the label map in G and
         in D's own step (the embedding table), the image in D's pass of the G step (x_cf) -- so the grad-input is the one-channel
         convolution with that channel's weights: the other channel's gradient was never read."""

    F = 256 * 7 * 7

    @staticmethod
    def unsupported(G, D, C):
        """None, or why these nets cannot take the fused path."""
        if type(G) is not Generator or type(D) is not Discriminator:
            return f"the nets are {type(G).__name__} / {type(D).__name__}, not gan_train.Generator / Discriminator"
        if not isinstance(C, Classifier) or C.training:
            return "the classifier is not a countergan.Classifier in eval mode"
        if G.label_embed.num_embeddings != D.label_embed.num_embeddings:
            return "G and D embed different numbers of classes"
        for net in (G, D, C):
            prec = getattr(net, "conv_precision", "fp32")
            if prec != "fp32":
                return f"conv_precision {prec!r} on {type(net).__name__}: the fused step is fp32 only"
        return None

    def __init__(self, G, D, C, batch_size, params=params, graph=True, rng=None):
        """rng (ops.DeviceRNG): step(x, y) with no target then draws the iteration's one class (gan_train_copy.py:119-120) as the FIRST
        launch of the step -- 65 launches -- into the step's own target buffer, its Philox offset read from a device counter that the
        launch advances itself, so every replay draws the next class of the stream; rng.offset is kept in step on the host."""
        why = self.unsupported(G, D, C)
        if why is not None:
            raise PcgError(f"GraphedTrainStep: {why}")
        dev = next(G.parameters()).device
        if dev.type != "cuda" or next(D.parameters()).device != dev or next(C.parameters()).device != dev:
            raise PcgError(f"GraphedTrainStep: the nets are on {dev}; libpcgan_hip has no CPU path")
        if int(batch_size) < 1:
            raise PcgError(f"GraphedTrainStep: batch size {batch_size}")
        self.G, self.D, self.C, self.B, self.params, self.dev = G, D, C, int(batch_size), dict(params), dev
        self.K = G.label_embed.num_embeddings
        for net in (G, D):
            net._ensure_flat()
            net.zero_grad()                                   # attaches the .grad views; every step OVERWRITES them (no zero_grad)
        self.opt_g, self.opt_d = make_optimizers(G, D, self.params)
        self._graph = bool(graph)
        self._bufs, self._graphs, self._draw_graphs = {}, {}, {}
        self._rng = rng
        self._ctr = rng.device_counter(dev) if rng is not None else None

    # -- buffers of one batch size --------------------------------------------------------------------------------------------------------
    def _buffers(self, R):
        dev = self.dev
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)      # noqa: E731
        i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)                 # noqa: E731
        gg, hw = [], H
        for conv in self.G._convs():
            gg.append(_geom(conv, R, hw, hw))
        gd2, gd1, hw = [], [], H
        for conv in self.D._convs():
            gd2.append(_geom(conv, 2 * R, hw, hw))
            gd1.append(_geom(conv, R, hw, hw))
            hw = gd2[-1].OH
        tail_ws, head_ws = ops.delta_gan_workspace(R, HW, dev)
        losses = f32(5)
        return {"R": R, "x": f32(R, HW), "y": i64(R), "t": i64(R), "g_in": f32(R, H, W, 2), "d_in": f32(2 * R, H, W, 2), "yt": i64(2 * R),
                "w_hwc": f32(self.F), "gg": gg, "h": [f32(R, g.OH, g.OW, g.Cout) for g in gg], "x_cf": f32(R, HW),
                "gd2": gd2, "gd1": gd1, "a": [f32(2 * R, g.OH, g.OW, g.Cout) for g in gd2], "logits_d": f32(2 * R), "logits_g": f32(R),
                "dlogit": f32(2 * R), "db_dead": f32(1), "tail_ws": tail_ws, "head_ws": head_ws, "losses": losses,
                "out": {k: losses[i:i + 1] for i, k in enumerate(("loss_D", "loss_G", "loss_adv", "loss_cls", "loss_reg"))},
                "cls_logits": f32(R, self.C.num_classes)}

    # -- one step, Adam included, over the buffer set b -----------------------------------------------------------------------------------
    def _launches(self, b, draw=False):
        if draw:
            self._rng.delta_gan_target(b["t"], self.K, counter=self._ctr)                                                    # :119-120
        with ops.conv_precision("fp32"):
            self._step(b)

    def _step(self, b):
        G, D, C, R, out = self.G, self.D, self.C, b["R"], b["out"]
        gconv, dconv, lin = G._convs(), D._convs(), D.net[7]
        slope = D.SLOPE
        hw7 = self.F // 256
        # entry: both nets' inputs, the label index of D's table gradient, the (h,w,c) image of net.7's weight row
        ops.delta_gan_entry(b["x"], b["y"], b["t"], G.label_embed.weight.data, D.label_embed.weight.data, g_in=b["g_in"], d_in=b["d_in"],
                            labels_2b=b["yt"], head_w=lin.weight.data, head_w_packed=b["w_hwc"], head_shape=(256, hw7))
        # G forward, once (:122 == :133)
        a = b["g_in"]
        for i, (conv, g, o) in enumerate(zip(gconv, b["gg"], b["h"])):
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_RELU if i < 3 else ACT_NONE, out=o)
        delta = b["h"][3].view(R, HW)
        ops.delta_gan_tail_fwd(b["x"], delta, b["d_in"], x_cf=b["x_cf"], loss_reg=out["loss_reg"], ws=b["tail_ws"])       # :133, :139
        # D step: one pass of 2B rows (:123-124), the head with both loss terms (:125-127), backward (:129), Adam (:130)
        a = b["d_in"]
        for conv, g, o in zip(dconv, b["gd2"], b["a"]):
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_LRELU, slope=slope, out=o)
        a3 = b["a"][2].view(2 * R, self.F)
        ops.logit_head_fwd(a3, b["w_hwc"], lin.bias.data, mode_g=False, logits=b["logits_d"], loss=out["loss_D"], dlogit=b["dlogit"],
                           db=lin.bias.grad, ws=b["head_ws"])
        d, _ = ops.logit_head_bwd(a3, b["w_hwc"], b["dlogit"], slope, dw=lin.weight.grad.view(-1), dw_shape=(256, hw7))
        for i in (2, 1, 0):
            conv, g = dconv[i], b["gd2"][i]
            below = b["a"][i - 1] if i > 0 else b["d_in"]
            d = d.view(g.B, g.OH, g.OW, g.Cout)
            ops.conv2d_wgrad(g, below, d, ops.ohwi(conv.weight.grad), False)
            ops.colsum(d.numel() // conv.out_channels, conv.out_channels, d, conv.bias.grad, False)
            if i > 0:
                d = _dgrad_act(g, d, ops.ohwi(conv.weight.data), below, ACT_LRELU, slope)
        g0 = b["gd2"][0]
        g1 = ops.conv_geom(g0.B, g0.IH, g0.IW, 1, g0.Cout, g0.KH, g0.KW, g0.stride, g0.pad)
        w0 = ops.ohwi(dconv[0].weight.data)
        d1 = ops.conv2d_dgrad(g1, d, ops.gather_channel(w0, 1))
        ops.embed_table_grad(d1, b["yt"], 1, 0, self.K, D.label_embed.weight.grad, accumulate=False)
        self.opt_d.step()
        # G step: D's pass of the B fake rows on the updated weights (:134), its label map regathered from the updated table
        ops.delta_gan_entry(None, None, b["t"], None, D.label_embed.weight.data, d_in=b["d_in"], head_w=lin.weight.data,
                            head_w_packed=b["w_hwc"], head_shape=(256, hw7), regather=True)
        a = b["d_in"][R:]
        acts = []
        for conv, g, o in zip(dconv, b["gd1"], b["a"]):
            acts.append(a)
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_LRELU, slope=slope, out=o[R:])
        a3 = a.view(R, self.F)
        ops.logit_head_fwd(a3, b["w_hwc"], lin.bias.data, mode_g=True, logits=b["logits_g"], loss=out["loss_adv"], dlogit=b["dlogit"][:R],
                           db=b["db_dead"], ws=b["head_ws"])                                                                 # :137
        d, _ = ops.logit_head_bwd(a3, b["w_hwc"], b["dlogit"][:R], slope)                                                    # no dw: dead
        for i in (2, 1):
            g = b["gd1"][i]
            d = _dgrad_act(g, d.view(g.B, g.OH, g.OW, g.Cout), ops.ohwi(dconv[i].weight.data), acts[i], ACT_LRELU, slope)
        g0 = b["gd1"][0]
        g1 = ops.conv_geom(g0.B, g0.IH, g0.IW, 1, g0.Cout, g0.KH, g0.KW, g0.stride, g0.pad)
        dD = ops.conv2d_dgrad(g1, d.view(g0.B, g0.OH, g0.OW, g0.Cout), ops.gather_channel(ops.ohwi(dconv[0].weight.data), 0))
        # the classifier's guidance (:135, :138): forward, cross-entropy, input gradient
        cls_pred, saved = C._run_forward(b["x_cf"], keep=True)
        b["cls_logits"].copy_(cls_pred)                            # the 10 live columns of the padded logits (tiny strided copy)
        _, dl = ops.cross_entropy_fwd_bwd(b["cls_logits"], b["t"], loss_out=out["loss_cls"])
        dC = C._run_backward(saved, dl)
        d = ops.delta_gan_tail_bwd(dD, dC.view(R, HW), delta, self.params["lambda_cls"], self.params["lambda_reg"])         # :141-143
        # G backward (:143), Adam (:144)
        for i in (3, 2, 1, 0):
            conv, g = gconv[i], b["gg"][i]
            below = b["h"][i - 1] if i > 0 else b["g_in"]
            d = d.view(g.B, g.OH, g.OW, g.Cout)
            ops.conv2d_wgrad(g, below, d, ops.ohwi(conv.weight.grad), False)
            ops.colsum(d.numel() // conv.out_channels, conv.out_channels, d, conv.bias.grad, False)
            if i > 0:
                d = _dgrad_act(g, d, ops.ohwi(conv.weight.data), below, ACT_RELU, 0.0)
        g0 = b["gg"][0]
        g1 = ops.conv_geom(g0.B, g0.IH, g0.IW, 1, g0.Cout, g0.KH, g0.KW, g0.stride, g0.pad)
        d1 = ops.conv2d_dgrad(g1, d, ops.gather_channel(ops.ohwi(gconv[0].weight.data), 1))
        ops.embed_table_grad(d1, b["t"], 1, 0, self.K, G.label_embed.weight.grad, accumulate=False)
        self.opt_g.step()
        ops.weighted_sum_fwd([out["loss_adv"], out["loss_cls"], out["loss_reg"]], [1.0, self.params["lambda_cls"], self.params["lambda_reg"]],
                             out=out["loss_G"])                                                                              # :141

    def _capture(self, b, draw=False):
        """Capture needs one real execution of every launch first; the parameters, the Adam state and the draw's device counter are put
        back afterwards."""
        held = Held((self.G, self.D), (self.opt_g, self.opt_d), (self._ctr if draw else None,))
        return capture_steps([(lambda: self._launches(b, draw), 1)], held, self.dev)[0][0]

    def step(self, x, y, target=None):
        """One iteration on the batch (x [R,1,28,28] or [R,784], y [R], target [R]).  target None (a stepper built with rng): the
        step draws its one random class itself.  Returns the device scalars {loss_D, loss_G, loss_adv, loss_cls, loss_reg}: views of
        this batch size's loss buffer, overwritten by its next step."""
        R = int(x.shape[0])
        draw = target is None
        if draw and self._rng is None:
            raise PcgError("GraphedTrainStep.step: no target given and the stepper was built without rng: there is nothing to draw the class from")
        if R < 1 or y.numel() != R or (not draw and target.numel() != R) or x.numel() != R * HW:
            raise PcgError(f"GraphedTrainStep.step: x {tuple(x.shape)}, y {tuple(y.shape)}, target "
                           f"{'(drawn)' if draw else tuple(target.shape)} are not one batch of 28 x 28 images")
        for name, t in (("y", y),) if draw else (("y", y), ("target", target)):
            if not t.is_cuda and t.numel():                   # host-visible labels: refused here; device labels are clamped by the kernel
                v = t.numpy()
                if v.min() < 0 or v.max() >= self.K:
                    raise PcgError(f"GraphedTrainStep.step: a label of {name} is outside 0..{self.K - 1}")
        b = self._bufs.get(R)
        if b is None:
            b = self._bufs[R] = self._buffers(R)
        b["x"].copy_(x.reshape(R, HW)); b["y"].copy_(y)
        if not draw:
            b["t"].copy_(target)
        if self._graph:
            graphs = self._draw_graphs if draw else self._graphs
            if R not in graphs:
                graphs[R] = self._capture(b, draw)
            graphs[R].replay()
        else:
            self._launches(b, draw)
        if draw:
            self._rng.offset += 1                             # the host-side mirror of the device counter (DeviceRNG.randint(.., 1)'s span)
        return b["out"]


_fused_fallback_warned = False


def _warn_fused_fallback(why):
    global _fused_fallback_warned
    if not _fused_fallback_warned:
        import warnings
        warnings.warn(f"train_gan(fused=True): {why}; running the op chain instead", RuntimeWarning, stacklevel=3)
        _fused_fallback_warned = True


class _TargetSource:
    """Where an iteration's target class comes from (host logic; gan_train.py:119 / gan_train_copy.py:119-120).  params["target_class"]
    set: one fill per batch size, as before, and nothing is ever drawn.  Otherwise `targets` (an iterable of ints, one per iteration)
    or a draw: by the fused step itself (in_step: next() returns None) or by ops.DeviceRNG.delta_gan_target with the offset passed by
    value."""

    def __init__(self, params, K, dev, rng=None, targets=None, in_step=False):
        self.fixed, self.K, self.dev, self.rng, self.in_step = params.get("target_class"), int(K), dev, rng, bool(in_step)
        if self.fixed is not None and targets is not None:
            raise PcgError("train_gan: `targets` replaces the draws of random-target training, but params['target_class'] is set")
        self.given = iter(targets) if targets is not None else None
        if self.fixed is None and self.given is None and rng is None:
            raise PcgError("train_gan: params has no target_class, so every iteration draws its class: pass rng=ops.DeviceRNG(seed) "
                           "(or targets=, one class per iteration)")
        self._bufs, self.count = {}, 0

    def _buf(self, R):
        if R not in self._bufs:
            self._bufs[R] = torch.zeros(R, dtype=torch.int64, device=self.dev)
        return self._bufs[R]

    def next(self, R):
        """The [R] int64 target tensor of the next iteration, or None: the fused step draws the class itself."""
        self.count += 1
        if self.fixed is not None:
            if R not in self._bufs:                                                    # :119, one fill per batch size
                self._bufs[R] = torch.full((R,), int(self.fixed), dtype=torch.int64, device=self.dev)
            return self._bufs[R]
        if self.given is not None:
            try:
                cls = int(next(self.given))
            except StopIteration:
                raise PcgError(f"train_gan: `targets` ran out at iteration {self.count}") from None
            if not 0 <= cls < self.K:
                raise PcgError(f"train_gan: target class {cls} of iteration {self.count} is outside 0..{self.K - 1}")
            return self._buf(R).fill_(cls)
        if self.in_step:
            return None
        return self.rng.delta_gan_target(self._buf(R), self.K)                         # gan_train_copy.py:119-120


def train_gan(G, D, C, train_loader, params=params, fused=False, rng=None, targets=None, verbose=True):
    """gan_train.py:115-148 over any iterable of (x, y).  The reference prints and records the last iteration's loss_D / loss_G of each
    epoch, so an epoch makes ONE host read and none inside it.  fused=True: the iterations run through GraphedTrainStep (one replay
    each); nets or a conv_precision the fused step does not take warn once and run the op chain.  params without "target_class"
    (params_random_target) is gan_train_copy.py's loop: every iteration's class is drawn on the device from rng (ops.DeviceRNG; inside
    the replayed step when fused), or taken from `targets`, an iterable of ints, one per iteration.
    Three optional keys of `params` (this function's argument list is the reference-shaped one and stays as it is; the other trainers
    take the same three as keyword arguments): params["checkpoint"] (a path): the run's whole state (pcgan_amd.checkpoint, DESIGN.md
    §3.23: both nets, both optimizers, rng, a data.DeviceLoader's generator, torch's CPU generator, the histories) is written there
    after every params["checkpoint_every"]-th (default 1) epoch.  params["resume"] (a path or a loaded checkpoint): rng is restored
    first, so that the fused step's device counter starts at the stored offset; the optimizers (and the fused stepper) are built as
    always, the stored state is restored over them, and training continues with the next epoch.  params["epochs_gan"] may be larger than when the checkpoint was written; batch size, number of
    rows and rng's seed must be the same; `targets`, if given, holds the classes of the remaining iterations.  A resume at or past
    the last epoch returns the stored histories without a launch.
    Returns {"g_losses", "d_losses"}, after a resume the epochs before the interruption included."""
    checkpoint, checkpoint_every, resume = params.get("checkpoint"), params.get("checkpoint_every", 1), params.get("resume")
    _ckpt.check_args("train_gan", checkpoint, checkpoint_every, resume)
    _check_classifier(C)
    dev = next(G.parameters()).device
    if dev.type != "cuda":
        raise PcgError(f"train_gan: the nets are on {dev}; libpcgan_hip has no CPU path")
    for p in C.parameters():
        p.requires_grad_(False)                                                        # :99-100
    drawn = params.get("target_class") is None and targets is None
    run = {"batch_size": int(params["batch_size"]), "n_rows": _ckpt.loader_rows(train_loader), "seed": rng.seed if rng is not None else None}
    loader = {"loader": train_loader} if isinstance(train_loader, DeviceLoader) else {}
    state = None
    if resume is not None:
        state = _ckpt.open_resume(resume, "train_gan", **run)
        if _ckpt.value(state, "epoch") >= params["epochs_gan"]:                        # nothing left to run: no launch
            _ckpt.restore(state, G=G, D=D)
            return dict(_ckpt.value(state, "history"))
        if rng is not None:
            _ckpt.restore(state, rng=rng)                                              # before the stepper makes its device counter from it
    stepper = None
    if fused:
        why = GraphedTrainStep.unsupported(G, D, C)
        if why is None:
            if drawn and rng is None:
                raise PcgError("train_gan(fused=True): params has no target_class and no rng was given: the fused step draws the class "
                               "on the device and needs rng=ops.DeviceRNG(seed)")
            stepper = GraphedTrainStep(G, D, C, params["batch_size"], params, rng=rng if drawn else None)
        else:
            _warn_fused_fallback(why)
    opt_g, opt_d = (stepper.opt_g, stepper.opt_d) if stepper is not None else make_optimizers(G, D, params)
    source = _TargetSource(params, G.label_embed.num_embeddings, dev, rng=rng, targets=targets, in_step=stepper is not None)
    g_losses, d_losses = [], []
    first = 0
    if state is not None:
        vals = _ckpt.restore(state, G=G, D=D, opt_g=opt_g, opt_d=opt_d, **loader)
        first, g_losses, d_losses = vals["epoch"], vals["history"]["g_losses"], vals["history"]["d_losses"]
    for epoch in range(first, params["epochs_gan"]):
        out = None
        for x, y in train_loader:
            x, y = x.to(dev), y.to(dev)                                                # :117-118
            target = source.next(int(y.shape[0]))
            if stepper is not None:
                out = stepper.step(x, y, target)
            else:
                out = train_step(G, D, C, opt_g, opt_d, x, y, target, params)
        if out is None:
            raise PcgError("train_gan: the loader gave no batch")
        ld, lg = torch.cat([out["loss_D"].reshape(1), out["loss_G"].reshape(1)]).cpu().tolist()     # the epoch's one host read (:146-148)
        if verbose:
            print(f"[GAN] Epoch {epoch + 1}/{params['epochs_gan']} | D_loss: {ld:.4f} | G_loss: {lg:.4f}")
        d_losses.append(ld)
        g_losses.append(lg)
        if _ckpt.due(checkpoint, checkpoint_every, epoch):
            objs = dict(loader, rng=rng) if rng is not None else loader
            _ckpt.save(checkpoint, _ckpt.capture(G=G, D=D, opt_g=opt_g, opt_d=opt_d, epoch=epoch + 1,
                                                 history={"g_losses": g_losses, "d_losses": d_losses}, run=run, **objs))
    return {"g_losses": g_losses, "d_losses": d_losses}


def counterfactual_batch(G, imgs, target):
    """gan_train.py:150-159 -- (clamp(x + delta, -1, 1), delta) under no_grad."""
    _need_gpu(imgs, "counterfactual_batch")
    with torch.no_grad():
        _, delta = G(imgs, target)
        B = imgs.shape[0]
        cf = ops.clamp_add_fwd(_as_rows(imgs, B), delta.reshape(B, HW), -1.0, 1.0)
    return cf.view(B, 1, H, W), delta


def _example_sheets(imgs, cf, delta, output_dir):
    """The three sheets of gan_train.py:161-163 / countergan2.py:222-224 -- save_image(..., nrow=4, normalize=True) of the images, the
    counterfactuals and `deltas * 0.5 + 0.5` (the affine rides in the sheet's own launches: pre=(0.5, 0.5) on the raw delta) --
    made on the device (pcgan_amd.sheets), one uint8 download each.  Returns the three [Hg, Wg, 3] uint8 arrays."""
    B = imgs.shape[0]
    return tuple(sheets.save_image(t.detach().reshape(B, 1, H, W).contiguous(), os.path.join(output_dir, name + ".png"), nrow=4, normalize=True,
                                   pre=pre)
                 for name, t, pre in (("original", imgs, (1.0, 0.0)), ("counterfactual", cf, (1.0, 0.0)), ("delta", delta, (0.5, 0.5))))


def save_examples(G, imgs, target, output_dir):
    """gan_train.py:155-163 -- the counterfactuals of one batch towards `target` (a class for every row, or one class per row) and
    the files original.png, counterfactual.png, delta.png in output_dir.  Returns (original, counterfactual, delta) as uint8 arrays."""
    _need_gpu(imgs, "save_examples")
    if not torch.is_tensor(target):
        target = torch.full((imgs.shape[0],), int(target), dtype=torch.int64, device=imgs.device)      # :155
    cf, delta = counterfactual_batch(G, imgs, target)
    return _example_sheets(imgs, cf, delta, output_dir)


# ---- the promptable half: queries, the all-targets sweep, per-target evaluation (gan_train_copy.py:161-172) -------------
EVAL_FIELDS = PER_CLASS_FIELDS + ("mean_abs_delta", "l2")


def _check_query_nets(G, C, imgs, who, query_chunk=1):
    """The refusals of the query front ends, all on the host before any launch."""
    if int(query_chunk) < 1:
        raise PcgError(f"{who}: query_chunk {query_chunk}: a window holds at least one query")
    if not (torch.is_tensor(imgs) and imgs.is_cuda):
        raise PcgError(f"{who}: the images are on {getattr(imgs, 'device', type(imgs))}; libpcgan_hip has no CPU path")
    if imgs.dim() < 2 or imgs.shape[0] < 1 or imgs.numel() != imgs.shape[0] * HW:
        raise PcgError(f"{who}: expected [B,1,{H},{W}] images, got shape {tuple(imgs.shape)}")
    for name, net in (("generator", G), ("classifier", C)):
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise PcgError(f"{who}: the {name} is on {dev}; libpcgan_hip has no CPU path")
    if not isinstance(G, Generator):
        raise PcgError(f"{who}: the generator is a {type(G).__name__}, not gan_train.Generator")
    if C.training:
        raise PcgError(f"{who}: the classifier is in training mode: call .eval() first (gan_train_copy.py:164 runs it frozen)")
    if getattr(C, "num_classes", None) != G.label_embed.num_embeddings:
        raise PcgError(f"{who}: the generator embeds {G.label_embed.num_embeddings} classes, the classifier has {getattr(C, 'num_classes', None)}")


def _query_labels(v, B, K, dev, name):
    """An int, a list or a tensor of one class per row -> [B] int64 on the GPU.  Where the values are visible to the host a class
    outside 0..K-1 is refused; labels already on the device are clamped into the table by the kernels."""
    if v is None:
        return None
    host = None
    if not torch.is_tensor(v):
        host = torch.as_tensor(v, dtype=torch.int64).reshape(-1)
        if host.numel() == 1 and not isinstance(v, (list, tuple)):
            host = host.expand(B)
    elif not v.is_cuda:
        host = v.reshape(-1).to(torch.int64)
    if host is not None:
        if host.numel() != B:
            raise PcgError(f"{name}: expected {B} labels, got {host.numel()}")
        if int(host.min()) < 0 or int(host.max()) >= K:
            raise PcgError(f"{name}: a label is outside 0..{K - 1}")
        return host.contiguous().to(dev)
    return _labels(v, B, dev, name)


def _run_queries(G, C, x, target, T, y_true=None, group_rows=None, query_chunk=2048, keep=True, with_orig=True, outputs=ops.SCORE_FIELDS):
    """All T * B queries of a batch: generator + classifier over windows of `query_chunk` queries, then ONE score launch."""
    B = x.shape[0]
    xr = _as_rows(x, B)
    K, TB, dev = C.num_classes, T * B, x.device
    kp = (K + 3) // 4 * 4
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.no_grad():
        logits, sums = torch.empty((TB, kp), **f32), torch.empty((TB, 3), **f32)
        full = {k: torch.empty((TB, HW), **f32) for k in ("x_cf", "delta")} if keep else None
        for q0 in range(0, TB, int(query_chunk)):
            nq = min(int(query_chunk), TB - q0)
            out = {"sums": sums[q0:q0 + nq]}
            if keep:
                out.update({k: v[q0:q0 + nq] for k, v in full.items()})
            r = G.forward_queries(xr, target, T=T, q0=q0, nq=nq, out=out)
            _padded_logits(C, r["x_cf"], out=logits[q0:q0 + nq])
        logits_orig = _padded_logits(C, xr) if (with_orig and y_true is not None) else None
        res = ops.mnist_cf_score(logits, K, B, T, target=target, y_true=y_true, logits_orig=logits_orig, tail_sums=sums, group_rows=group_rows,
                                 outputs=outputs)
    res.update(sums=sums, logits=logits)
    if keep:
        res.update(full)
    return res


def counterfactuals(G, C, imgs, target, y_true=None, query_chunk=2048):
    """The prompted query of gan_train_copy.py:161-172: "turn these images into `target`" (an int, or one class per row).  C: any
    classifier countergan._padded_logits accepts, in eval mode.  Returns device tensors: x_cf (clamped, :166), delta [B,1,28,28]; pred
    (int64, the first maximum, :171), conf (:172), p_target, p_true / p_orig_true (with y_true), flip [B]; sums [B,3] = sum |x_cf - x|,
    sum |delta|, sum (x_cf - x)^2 over the pixels; group_sums [1,1,8] (countergan.SUM_FIELDS)."""
    _check_query_nets(G, C, imgs, "counterfactuals", query_chunk)
    B, K = imgs.shape[0], C.num_classes
    res = _run_queries(G, C, imgs, _query_labels(target, B, K, imgs.device, "target"), 1,
                       y_true=_query_labels(y_true, B, K, imgs.device, "y_true"), query_chunk=query_chunk)
    shp = (B, 1, H, W)
    out = {"x_cf": res["x_cf"].view(shp), "delta": res["delta"].view(shp), "sums": res["sums"], "group_sums": res["group_sums"]}
    out.update({k: res[k] for k in ops.SCORE_FIELDS})
    return out


def counterfactual_sweep(G, C, imgs, y_true=None, query_chunk=2048, group_rows=None):
    """counterfactuals() for ALL num_classes targets of every row: windows of `query_chunk` queries through G and C, then ONE score
    launch.  Results shaped [T,B,...] (x_cf, delta [T,B,1,28,28]; pred ... flip [T,B]; sums [T,B,3]) and group_sums
    [T, ceil(B / group_rows), 8] (countergan.SUM_FIELDS)."""
    _check_query_nets(G, C, imgs, "counterfactual_sweep", query_chunk)
    B, T = imgs.shape[0], G.label_embed.num_embeddings
    res = _run_queries(G, C, imgs, None, T, y_true=_query_labels(y_true, B, C.num_classes, imgs.device, "y_true"), group_rows=group_rows,
                       query_chunk=query_chunk)
    shp = (T, B, 1, H, W)
    out = {"x_cf": res["x_cf"].view(shp), "delta": res["delta"].view(shp), "sums": res["sums"].view(T, B, 3), "group_sums": res["group_sums"]}
    out.update({k: res[k].view(T, B) for k in ops.SCORE_FIELDS})
    return out


def counterfactual_grid(G, C, dataset, pick_best_source=False, chunk=2048, full_scan=False):
    """The source-by-target grid of eval_utils.py:113-201 for the additive-delta generator (and countergan2.Generator, which inherits
    it), each cell gan_train_copy.py:161-172: countergan.pick_sources, ONE counterfactual_sweep over the K sources, the grid image
    (ops.cf_panels).  Returns what countergan.counterfactual_grid returns."""
    sources, rows, conf = pick_sources(C, dataset, pick_best_source, chunk, full_scan)
    return _grid_report(sources, rows, conf, counterfactual_sweep(G, C, sources))


def evaluate_examples(G, C, imgs, targets=None, rng=None):
    """gan_train_copy.py:158-172 without the figure: one random target per image (:162), drawn on the device with rng.randint, or the
    `targets` supplied; the clamped counterfactuals and the classifier's prediction and confidence for each.  Returns
    (targets, x_cf, delta, pred, conf), all on the device."""
    _check_query_nets(G, C, imgs, "evaluate_examples")
    B, K = imgs.shape[0], C.num_classes
    if targets is None:
        if rng is None:
            raise PcgError("evaluate_examples: no targets given and no rng to draw them from: pass rng=ops.DeviceRNG(seed)")
        targets = rng.randint(0, K, B, imgs.device)                                                                       # :162
    else:
        targets = _query_labels(targets, B, K, imgs.device, "targets")
    res = _run_queries(G, C, imgs, targets, 1, outputs=("pred", "conf"), keep=True)
    shp = (B, 1, H, W)
    return targets, res["x_cf"].view(shp), res["delta"].view(shp), res["pred"], res["conf"]


def _fold_eval(group_sums):
    """Pure host.  [T][J][8] group sums (J loader batches) -> {target: {EVAL_FIELDS}} in float64: per target the mean over the batches
    of the per-batch means, the order of eval_utils.py:97-102 (a ragged last batch weighs as much as a full one).  class_flip_rate,
    prediction_gain and actionability as eval_utils.py:58-66 defines them; mean_abs_delta = mean |delta| (the un-clamped change); l2 =
    sqrt(mean over the batch's rows of sum_pixels (x_cf - x)^2), the root-mean-square L2 distance of a batch."""
    import numpy as np
    per = metrics_from_sums(group_sums, HW)
    if per["count"].ndim != 2:
        raise PcgError(f"_fold_eval: expected [T][J][8] sums, got {np.asarray(group_sums).shape}")
    live = per["count"] > 0
    if not live.any(axis=1).all():
        raise PcgError("_fold_eval: a target class has no batch")
    with np.errstate(invalid="ignore"):
        cols = {"class_flip_rate": per["class_flip_rate"], "prediction_gain": per["prediction_gain"], "actionability": per["actionability"],
                "mean_abs_delta": per["allowed_l1"], "l2": np.sqrt(per["mask_penalty_pre"] * float(HW))}
    folded = {k: np.where(live, v, 0.0).sum(axis=1) / live.sum(axis=1) for k, v in cols.items()}
    return {cls: {k: float(folded[k][cls]) for k in EVAL_FIELDS} for cls in range(live.shape[0])}


def evaluate_per_target(G, C, loader, one_pass=True, query_chunk=2048, verbose=True):
    """Per target class, over any iterable of (x, y): class_flip_rate, prediction_gain and actionability exactly as
    mnist/eval_utils.py:58-66 defines them for any generator, plus mean_abs_delta and l2 (_fold_eval), each the mean over the loader's
    batches of the per-batch means (:97-102).  one_pass: all num_classes targets of a loader batch in ONE sweep (windows of
    query_chunk queries), the group sums kept on the device and read ONCE for the whole loader; one_pass=False: one counterfactuals()
    call and one host read per (batch, target), the reference's own loop.  Host arithmetic in float64.  Returns
    {target class: {metric: value}}, which countergan.per_class_csv(result, fields=EVAL_FIELDS) prints."""
    import numpy as np
    from .countergan import per_class_csv
    T, dev = G.label_embed.num_embeddings, next(G.parameters()).device
    groups = []
    for x, y in loader:
        x = x.to(dev)
        _check_query_nets(G, C, x, "evaluate_per_target", query_chunk)
        B = x.shape[0]
        y = _query_labels(y, B, C.num_classes, dev, "y")
        if one_pass:
            groups.append(_run_queries(G, C, x, None, T, y_true=y, group_rows=B, query_chunk=query_chunk, keep=False, with_orig=False,
                                       outputs=())["group_sums"])
        else:
            groups.append(np.concatenate([counterfactuals(G, C, x, cls, y_true=y, query_chunk=query_chunk)["group_sums"].cpu().numpy()
                                          for cls in range(T)], axis=0))
    if not groups:
        raise PcgError("evaluate_per_target: the loader yielded no batch")
    sums = torch.cat(groups, dim=1).cpu().numpy() if one_pass else np.concatenate(groups, axis=1)      # [T][J][8]; one_pass: the one host read
    avg = _fold_eval(sums)
    if verbose:
        print(per_class_csv(avg, fields=EVAL_FIELDS), end="")
    return avg
