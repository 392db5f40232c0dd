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

The torch layer objects are kept as parameter containers (`label_embed`, and `net`, the reference's nn.Sequential layer for layer), so
`state_dict()` keys and shapes are the reference's in both directions with strict=True.  Forward and backward are one autograd node per
network sequencing C-ABI calls on NHWC activations (csrc/delta_gan.hip holds the fused launches around the convolutions; DESIGN.md
§3.19)."""
import torch
import torch.nn as nn

from . import ops
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, PcgError
from .countergan import BCEWithLogitsLoss, Classifier, CrossEntropyLoss, _as_rows, _conv_fwd, _conv_wgrad, _dgrad_act, _geom, abs_mean
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

    def __init__(self, G, D, C, batch_size, params=params, graph=True):
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
        self._bufs, self._graphs = {}, {}

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
    def _launches(self, b):
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

    def _capture(self, b):
        """Capture needs one real execution of every launch first; the parameters and the Adam state are put back afterwards."""
        G, D = self.G, self.D
        p0 = G.flat_params.clone(), D.flat_params.clone()
        snaps = self.opt_g.snapshot(), self.opt_d.snapshot()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._launches(b)
        torch.cuda.current_stream().wait_stream(side)
        if snaps[0] is None:                                  # the first execution built the Adam state: capture sees it at step 0 again
            self.opt_g.restore(None); self.opt_d.restore(None)
        # no finalizer may run while the stream captures (see nn._HipGraphCapture.begin): the cyclic collector is held off
        import gc
        gc_on = gc.isenabled()
        gc.disable()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._launches(b)
        finally:
            if gc_on:
                gc.enable()
        G.flat_params.copy_(p0[0]); D.flat_params.copy_(p0[1])
        self.opt_g.restore(snaps[0]); self.opt_d.restore(snaps[1])
        return graph

    def step(self, x, y, target):
        """One iteration on the batch (x [R,1,28,28] or [R,784], y [R], target [R]).  Returns the device scalars {loss_D, loss_G,
        loss_adv, loss_cls, loss_reg}: views of this batch size's loss buffer, overwritten by its next step."""
        R = int(x.shape[0])
        if R < 1 or y.numel() != R or target.numel() != R or x.numel() != R * HW:
            raise PcgError(f"GraphedTrainStep.step: x {tuple(x.shape)}, y {tuple(y.shape)}, target {tuple(target.shape)} are not one batch of 28 x 28 images")
        for name, t in (("y", y), ("target", target)):
            if not t.is_cuda and t.numel():                   # host-visible labels: refused here; device labels are clamped by the kernel
                v = t.numpy()
                if v.min() < 0 or v.max() >= self.K:
                    raise PcgError(f"GraphedTrainStep.step: a label of {name} is outside 0..{self.K - 1}")
        b = self._bufs.get(R)
        if b is None:
            b = self._bufs[R] = self._buffers(R)
        b["x"].copy_(x.reshape(R, HW)); b["y"].copy_(y); b["t"].copy_(target)
        if self._graph:
            if R not in self._graphs:
                self._graphs[R] = self._capture(b)
            self._graphs[R].replay()
        else:
            self._launches(b)
        return b["out"]


_fused_fallback_warned = False


def _warn_fused_fallback(why):
    global _fused_fallback_warned
    if not _fused_fallback_warned:
        import warnings
        warnings.warn(f"train_gan(fused=True): {why}; running the op chain instead", RuntimeWarning, stacklevel=3)
        _fused_fallback_warned = True


def train_gan(G, D, C, train_loader, params=params, fused=False, verbose=True):
    """gan_train.py:115-148 over any iterable of (x, y).  The reference prints and records the last iteration's loss_D / loss_G of each
    epoch, so an epoch makes ONE host read and none inside it.  fused=True: the iterations run through GraphedTrainStep (one replay
    each); nets or a conv_precision the fused step does not take warn once and run the op chain.  Returns {"g_losses", "d_losses"}."""
    _check_classifier(C)
    dev = next(G.parameters()).device
    if dev.type != "cuda":
        raise PcgError(f"train_gan: the nets are on {dev}; libpcgan_hip has no CPU path")
    for p in C.parameters():
        p.requires_grad_(False)                                                        # :99-100
    stepper = None
    if fused:
        why = GraphedTrainStep.unsupported(G, D, C)
        if why is None:
            stepper = GraphedTrainStep(G, D, C, params["batch_size"], params)
        else:
            _warn_fused_fallback(why)
    opt_g, opt_d = (stepper.opt_g, stepper.opt_d) if stepper is not None else make_optimizers(G, D, params)
    targets = {}
    g_losses, d_losses = [], []
    for epoch in range(params["epochs_gan"]):
        out = None
        for x, y in train_loader:
            x, y = x.to(dev), y.to(dev)                                                # :117-118
            R = int(y.shape[0])
            if R not in targets:                                                       # :119, one fill per batch size
                targets[R] = torch.full((R,), int(params["target_class"]), dtype=torch.int64, device=dev)
            if stepper is not None:
                out = stepper.step(x, y, targets[R])
            else:
                out = train_step(G, D, C, opt_g, opt_d, x, y, targets[R], params)
        if out is None:
            raise PcgError("train_gan: the loader gave no batch")
        ld, lg = torch.cat([out["loss_D"].reshape(1), out["loss_G"].reshape(1)]).cpu().tolist()     # the epoch's one host read (:146-148)
        if verbose:
            print(f"[GAN] Epoch {epoch + 1}/{params['epochs_gan']} | D_loss: {ld:.4f} | G_loss: {lg:.4f}")
        d_losses.append(ld)
        g_losses.append(lg)
    return {"g_losses": g_losses, "d_losses": d_losses}


def counterfactual_batch(G, imgs, target):
    """gan_train.py:150-159 -- (clamp(x + delta, -1, 1), delta) under no_grad."""
    _need_gpu(imgs, "counterfactual_batch")
    with torch.no_grad():
        _, delta = G(imgs, target)
        B = imgs.shape[0]
        cf = ops.clamp_add_fwd(_as_rows(imgs, B), delta.reshape(B, HW), -1.0, 1.0)
    return cf.view(B, 1, H, W), delta
