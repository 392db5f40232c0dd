"""Host-side mirror of `conditional_counteRGAN/mnist/countergan2.py` -- the CounteRGAN whose discriminator keeps the full 28 x 28
resolution, ends in a Sigmoid and is trained with log-eps losses on the probabilities, towards the one class of --target -- on the HIP
kernels.

    reference (countergan2.py)                             here
    ---------------------------------------------------    -----------------------------------------------------
    params, --target                  :16-34                params(target)
    Generator                         :57-73                Generator (same ctor args, same state_dict keys)
    Discriminator                     :76-93                Discriminator (probabilities [B, 1])
    Classifier and its pre-training   :96-167               countergan.Classifier / fit_pool_classifier; frozen, eval
    optimizers                        :170-171              make_optimizers
    loop body                         :180-205              train_step (op chain) / GraphedTrainStep (fused, one graph replay)
    loop                              :178-209              train_gan
    test pictures                     :213-224              counterfactual_batch, delta_image (no PNG writer)

The generator is gan_train's generator with another layer list: its sweeps are generic in the number of convolutions and are inherited.
The discriminator's head (Flatten + Linear(50176 -> 1) + Sigmoid) is the library's GEMM and pcg_act_fwd in the op chain and
pcg_prob_head_fwd (csrc/prob_head.hip) in the fused step; DESIGN.md §3.21."""
import torch
import torch.nn as nn

from . import gan_train as _gt
from . import ops
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, PcgError
from .countergan import Classifier, CrossEntropyLoss, _as_rows, _conv_fwd, _conv_wgrad, _dgrad_act, _geom, abs_mean  # noqa: F401
from .gan_train import HW, H, W, _check_classifier, _DFn, _label_channel_grad, _need_gpu, _TargetSource, make_optimizers  # noqa: F401
from .nn import FlatModule, in_conv_precision, linear_dgrad, linear_fwd, linear_wgrad, weighted_sum

EPS = ops.LOG_EPS                                      # :188, :198


def params(target):
    """The dict of countergan2.py:26-34 plus the class of --target (:17, :182)."""
    target = int(target)
    if not 0 <= target <= 9:
        raise PcgError(f"params: target class {target} is outside 0..9 (countergan2.py:17)")
    return {"batch_size": 128, "epochs": 50, "lr_G": 1e-3, "lr_D": 1e-3, "lambda_cls": 3.0, "lambda_reg": 0.05, "device": "cuda",
            "target": target}


# ---- the nets -----------------------------------------------------------------------------------------------------------------------------
class Generator(_gt.Generator):
    """countergan2.py:57-73 -- returns (x + delta, delta).  Forward, backward and the query windows are gan_train.Generator's: they
    walk whatever convolutions `net` holds."""

    def __init__(self, num_classes=10):
        FlatModule.__init__(self)                      # not gan_train.Generator's constructor: its layers would draw from the RNG first
        self.label_embed = nn.Embedding(num_classes, HW)
        self.net = nn.Sequential(
            nn.Conv2d(2, 64, kernel_size=3, padding=1), nn.ReLU(),
            nn.Conv2d(64, 64, kernel_size=3, padding=1), nn.ReLU(),
            nn.Conv2d(64, 1, kernel_size=3, padding=1),
        )


class Discriminator(FlatModule):
    """countergan2.py:76-93 -- probabilities [B, 1]: the Sigmoid is part of the net."""

    SLOPE = 0.2
    F = 64 * HW

    def __init__(self, num_classes=10):
        super().__init__()
        self.label_embed = nn.Embedding(num_classes, HW)
        self.net = nn.Sequential(
            nn.Conv2d(2, 64, 3, padding=1), nn.LeakyReLU(0.2),
            nn.Conv2d(64, 64, 3, padding=1), nn.LeakyReLU(0.2),
            nn.Flatten(),
            nn.Linear(64 * 28 * 28, 1),
            nn.Sigmoid(),
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
        a = ops.embed_concat_fwd(_as_rows(x, B), c, self.label_embed.weight.data, None).view(B, H, W, 2)   # :91-92
        layers = []
        for conv in self._convs():
            g, z = _conv_fwd(conv, a, ACT_LRELU, self.SLOPE)
            layers.append((g, a, z))
            a = z
        hw, ch = a.shape[1] * a.shape[2], a.shape[3]
        flat = ops.nhwc_to_nchw_flat(a, B, hw, ch).view(B, hw * ch)                   # nn.Flatten of the NCHW tensor: net.5's own column order
        prob = ops.act_fwd(linear_fwd(self.net[5], flat).view(B, 1), ACT_SIGMOID)    # :86-87
        return prob, ((layers, flat, (hw, ch), c, prob) if keep else None)

    @in_conv_precision
    def _run_backward(self, saved, dprob, need_x, need_p):
        layers, flat, (hw, ch), c, prob = saved
        B = flat.shape[0]
        lin = self.net[5]
        dl = ops.act_bwd(dprob.contiguous().view(B, 1), prob, ACT_SIGMOID)            # through the Sigmoid: dp * d (1 - d)
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


# ---- the losses of :188 and :198 as autograd nodes on pcg_log_eps_loss_fwd_bwd ----------------------------------------------------------------
class _LogEpsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode_g, *probs):
        p = probs[0].contiguous().view(-1) if len(probs) == 1 else torch.cat([q.reshape(-1) for q in probs])   # (real, fake): the halves
        ctx.mode_g, ctx.shapes = mode_g, [q.shape for q in probs]
        ctx.save_for_backward(p)
        loss, _ = ops.log_eps_loss_fwd_bwd(p, mode_g, EPS, need_grad=False)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        _, dp = ops.log_eps_loss_fwd_bwd(p, ctx.mode_g, EPS, need_loss=False, grad_out=g.contiguous().view(1))
        parts, off = [], 0
        for s in ctx.shapes:
            parts.append(dp[off:off + s.numel()].view(s))
            off += s.numel()
        return (None,) + tuple(parts)


def d_loss(d_real, d_fake):
    """-mean(log(d_real + 1e-6) + log(1 - d_fake + 1e-6)) (:188)."""
    if d_real.numel() != d_fake.numel():
        raise PcgError(f"d_loss: {d_real.numel()} real rows, {d_fake.numel()} fake rows")
    return _LogEpsFn.apply(False, d_real, d_fake)


def adv_loss(d_fake):
    """-mean(log(d_fake + 1e-6)) (:198)."""
    return _LogEpsFn.apply(True, d_fake)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------------
def train_step(G, D, C, opt_g, opt_d, x, y, target, params):
    """One iteration of countergan2.py:180-205 for a batch already on the GPU, as the op chain on the library's entries; `target`
    (:182) is passed in.  Returns the device scalars {loss_D, loss_G, loss_adv, loss_cls, loss_reg}; the reference's .item() calls are
    the caller's.  G(x, target) of :185 and of :194 is one forward (see GraphedTrainStep, restructuring 1); D's weight gradients in the
    G step are not formed (restructuring 3)."""
    _need_gpu(x, "train_step")
    _check_classifier(C)
    ce = CrossEntropyLoss()                                                            # :173
    x_cf, delta = G(x, target)                                                         # :185 == :194
    # Discriminator
    d_real = D(x, y)                                                                   # :186
    d_fake = D(x_cf.detach(), target)                                                  # :187
    loss_D = d_loss(d_real, d_fake)                                                    # :188
    opt_d.zero_grad()                                                                  # :189
    loss_D.backward()                                                                  # :190
    opt_d.step()                                                                       # :191
    # Generator
    for p in D.parameters():
        p.requires_grad_(False)
    try:
        d_fake = D(x_cf, target)                                                       # :195
        cls_pred = C(x_cf)                                                             # :196
        loss_adv = adv_loss(d_fake)                                                    # :198
        loss_cls = ce(cls_pred, target)                                                # :199
        loss_reg = abs_mean(delta)                                                     # :200
        loss_G = weighted_sum([loss_adv, loss_cls, loss_reg], [1.0, params["lambda_cls"], params["lambda_reg"]])   # :202
        opt_g.zero_grad()                                                              # :203
        loss_G.backward()                                                              # :204
    finally:
        for p in D.parameters():
            p.requires_grad_(True)
    opt_g.step()                                                                       # :205
    return {"loss_D": loss_D.detach(), "loss_G": loss_G.detach(), "loss_adv": loss_adv.detach(), "loss_cls": loss_cls.detach(),
            "loss_reg": loss_reg.detach()}


class GraphedTrainStep(_gt.GraphedTrainStep):
    """The iteration of countergan2.py:180-205 on the fused launches of csrc/delta_gan.hip and csrc/prob_head.hip around the library's
    convolutions, captured once per batch size met as a single-stream, strictly linear HIP graph with gan_train.GraphedTrainStep's
    mechanics (its constructor, step(), warm-up and capture are inherited; only the buffers and the launch sequence differ).
    graph=False calls the same entries eagerly, which is what the replays equal bit for bit.

    The three restructurings of gan_train.GraphedTrainStep hold here for the same reasons:
      1. G's forward runs once.  G(x, target) at :185 and at :194 read the same weights -- Adam(G), :205, comes after both.
      2. D(x, y) and D(x_cf.detach(), target) (:186-187) are one pass of 2B rows: D has no BatchNorm, so a row's probability depends on
         that row alone; only the weight and bias gradients add the two halves' contributions in one sum.  D's pass of the G step (:195)
         is a fresh forward of the B fake rows after Adam(D) (:191), its label channel regathered from the updated table.
      3. Dead work is skipped.  D's weight gradients of the G step (:204) are cleared by optimizer_D.zero_grad() (:189) before anyone
         reads them, so they are not formed; the entry convolutions' grad-inputs are the one-channel convolutions of the channel that
         has a consumer (the label map in G and in D's own step, the image in D's pass of the G step)."""

    F = Discriminator.F

    @staticmethod
    def unsupported(G, D, C):
        """None, or why these nets cannot take the fused path."""
        if type(G) is not Generator or type(D) is not Discriminator:
            return f"the nets are {type(G).__name__} / {type(D).__name__}, not countergan2.Generator / Discriminator"
        if not isinstance(C, Classifier) or C.training:
            return "the classifier is not a countergan.Classifier in eval mode"
        if G.label_embed.num_embeddings != D.label_embed.num_embeddings:
            return "G and D embed different numbers of classes"
        for net in (G, D, C):
            prec = getattr(net, "conv_precision", "fp32")
            if prec != "fp32":
                return f"conv_precision {prec!r} on {type(net).__name__}: the fused step is fp32 only"
        return None

    def __init__(self, G, D, C, batch_size, params, graph=True):
        super().__init__(G, D, C, batch_size, params, graph=graph)

    def _buffers(self, R):
        dev = self.dev
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)      # noqa: E731
        i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)                 # noqa: E731
        gg = [_geom(conv, R, H, W) for conv in self.G._convs()]
        gd2 = [_geom(conv, 2 * R, H, W) for conv in self.D._convs()]                  # every layer keeps 28 x 28
        gd1 = [_geom(conv, R, H, W) for conv in self.D._convs()]
        tail_ws, _ = ops.delta_gan_workspace(R, HW, dev)
        losses = f32(5)
        return {"R": R, "x": f32(R, HW), "y": i64(R), "t": i64(R), "g_in": f32(R, H, W, 2), "d_in": f32(2 * R, H, W, 2), "yt": i64(2 * R),
                "w_hwc": f32(self.F), "gg": gg, "h": [f32(R, g.OH, g.OW, g.Cout) for g in gg], "x_cf": f32(R, HW),
                "gd2": gd2, "gd1": gd1, "a": [f32(2 * R, g.OH, g.OW, g.Cout) for g in gd2], "logits_d": f32(2 * R), "logits_g": f32(R),
                "prob_d": f32(2 * R), "prob_g": f32(R), "dlogit": f32(2 * R), "db_dead": f32(1), "tail_ws": tail_ws,
                "head_ws": max((ops.prob_head_workspace(n, dev) for n in (2 * R, R)), key=lambda t: t.numel()), "losses": losses,
                "out": {k: losses[i:i + 1] for i, k in enumerate(("loss_D", "loss_G", "loss_adv", "loss_cls", "loss_reg"))},
                "cls_logits": f32(R, self.C.num_classes)}

    def _step(self, b):
        G, D, C, R, out = self.G, self.D, self.C, b["R"], b["out"]
        gconv, dconv, lin = G._convs(), D._convs(), D.net[5]
        nG, nD, slope = len(gconv), len(dconv), D.SLOPE
        head = (self.F // HW, HW)                                                     # net.5's columns are (c, h, w): 64 x 784
        # entry: both nets' inputs, the label index of D's table gradient, the (h,w,c) image of net.5's weight row
        ops.delta_gan_entry(b["x"], b["y"], b["t"], G.label_embed.weight.data, D.label_embed.weight.data, g_in=b["g_in"], d_in=b["d_in"],
                            labels_2b=b["yt"], head_w=lin.weight.data, head_w_packed=b["w_hwc"], head_shape=head)
        # G forward, once (:185 == :194)
        a = b["g_in"]
        for i, (conv, g, o) in enumerate(zip(gconv, b["gg"], b["h"])):
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_RELU if i + 1 < nG else ACT_NONE, out=o)
        delta = b["h"][nG - 1].view(R, HW)
        ops.delta_gan_tail_fwd(b["x"], delta, b["d_in"], x_cf=b["x_cf"], loss_reg=out["loss_reg"], ws=b["tail_ws"])       # :194, :200
        # D step: one pass of 2B rows (:186-187), the head with the loss (:188), backward (:190), Adam (:191)
        a = b["d_in"]
        for conv, g, o in zip(dconv, b["gd2"], b["a"]):
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_LRELU, slope=slope, out=o)
        top = b["a"][nD - 1].view(2 * R, self.F)
        ops.prob_head_fwd(top, b["w_hwc"], lin.bias.data, mode_g=False, eps=EPS, logits=b["logits_d"], prob=b["prob_d"], loss=out["loss_D"],
                          dlogit=b["dlogit"], db=lin.bias.grad, ws=b["head_ws"])
        d, _ = ops.logit_head_bwd(top, b["w_hwc"], b["dlogit"], slope, dw=lin.weight.grad.view(-1), dw_shape=head)
        for i in range(nD - 1, -1, -1):
            conv, g = dconv[i], b["gd2"][i]
            below = b["a"][i - 1] if i > 0 else b["d_in"]
            d = d.view(g.B, g.OH, g.OW, g.Cout)
            ops.conv2d_wgrad(g, below, d, ops.ohwi(conv.weight.grad), False)
            ops.colsum(d.numel() // conv.out_channels, conv.out_channels, d, conv.bias.grad, False)
            if i > 0:
                d = _dgrad_act(g, d, ops.ohwi(conv.weight.data), below, ACT_LRELU, slope)
        g0 = b["gd2"][0]
        g1 = ops.conv_geom(g0.B, g0.IH, g0.IW, 1, g0.Cout, g0.KH, g0.KW, g0.stride, g0.pad)
        d1 = ops.conv2d_dgrad(g1, d, ops.gather_channel(ops.ohwi(dconv[0].weight.data), 1))
        ops.embed_table_grad(d1, b["yt"], 1, 0, self.K, D.label_embed.weight.grad, accumulate=False)
        self.opt_d.step()
        # G step: D's pass of the B fake rows on the updated weights (:195), its label map regathered from the updated table
        ops.delta_gan_entry(None, None, b["t"], None, D.label_embed.weight.data, d_in=b["d_in"], head_w=lin.weight.data,
                            head_w_packed=b["w_hwc"], head_shape=head, regather=True)
        a = b["d_in"][R:]
        acts = []
        for conv, g, o in zip(dconv, b["gd1"], b["a"]):
            acts.append(a)
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_LRELU, slope=slope, out=o[R:])
        top = a.view(R, self.F)
        ops.prob_head_fwd(top, b["w_hwc"], lin.bias.data, mode_g=True, eps=EPS, logits=b["logits_g"], prob=b["prob_g"], loss=out["loss_adv"],
                          dlogit=b["dlogit"][:R], db=b["db_dead"], ws=b["head_ws"])                                          # :198
        d, _ = ops.logit_head_bwd(top, b["w_hwc"], b["dlogit"][:R], slope)                                                   # no dw: dead
        for i in range(nD - 1, 0, -1):
            g = b["gd1"][i]
            d = _dgrad_act(g, d.view(g.B, g.OH, g.OW, g.Cout), ops.ohwi(dconv[i].weight.data), acts[i], ACT_LRELU, slope)
        g0 = b["gd1"][0]
        g1 = ops.conv_geom(g0.B, g0.IH, g0.IW, 1, g0.Cout, g0.KH, g0.KW, g0.stride, g0.pad)
        dD = ops.conv2d_dgrad(g1, d.view(g0.B, g0.OH, g0.OW, g0.Cout), ops.gather_channel(ops.ohwi(dconv[0].weight.data), 0))
        # the classifier's guidance (:196, :199): forward, cross-entropy, input gradient
        cls_pred, saved = C._run_forward(b["x_cf"], keep=True)
        b["cls_logits"].copy_(cls_pred)                            # the 10 live columns of the padded logits (tiny strided copy)
        _, dl = ops.cross_entropy_fwd_bwd(b["cls_logits"], b["t"], loss_out=out["loss_cls"])
        dC = C._run_backward(saved, dl)
        d = ops.delta_gan_tail_bwd(dD, dC.view(R, HW), delta, self.params["lambda_cls"], self.params["lambda_reg"])         # :202-204
        # G backward (:204), Adam (:205)
        for i in range(nG - 1, -1, -1):
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
                             out=out["loss_G"])                                                                              # :202


_fused_fallback_warned = False


def _warn_fused_fallback(why):
    global _fused_fallback_warned
    if not _fused_fallback_warned:
        import warnings
        warnings.warn(f"train_gan(fused=True): {why}; running the op chain instead", RuntimeWarning, stacklevel=3)
        _fused_fallback_warned = True


def train_gan(G, D, C, train_loader, params, fused=False, verbose=True):
    """countergan2.py:178-209 over any iterable of (x, y).  The reference prints and records the last iteration's loss_D / loss_G of
    each epoch, so an epoch makes ONE host read and none inside it.  fused=True: the iterations run through GraphedTrainStep (one
    replay each); nets or a conv_precision the fused step does not take warn once and run the op chain.  Returns {"g_losses",
    "d_losses"}."""
    _check_classifier(C)
    dev = next(G.parameters()).device
    if dev.type != "cuda":
        raise PcgError(f"train_gan: the nets are on {dev}; libpcgan_hip has no CPU path")
    for p in C.parameters():
        p.requires_grad_(False)                                                        # :166-167
    stepper = None
    if fused:
        why = GraphedTrainStep.unsupported(G, D, C)
        if why is None:
            stepper = GraphedTrainStep(G, D, C, params["batch_size"], params)
        else:
            _warn_fused_fallback(why)
    opt_g, opt_d = (stepper.opt_g, stepper.opt_d) if stepper is not None else make_optimizers(G, D, params)
    source = _TargetSource({"target_class": params["target"]}, G.label_embed.num_embeddings, dev)   # :182, one fill per batch size
    g_losses, d_losses = [], []
    for epoch in range(params["epochs"]):
        out = None
        for x, y in train_loader:
            x, y = x.to(dev), y.to(dev)                                                # :180-181
            target = source.next(int(y.shape[0]))
            if stepper is not None:
                out = stepper.step(x, y, target)
            else:
                out = train_step(G, D, C, opt_g, opt_d, x, y, target, params)
        if out is None:
            raise PcgError("train_gan: the loader gave no batch")
        ld, lg = torch.cat([out["loss_D"].reshape(1), out["loss_G"].reshape(1)]).cpu().tolist()     # the epoch's one host read (:207-209)
        if verbose:
            print(f"Epoch {epoch + 1}/{params['epochs']} | D_loss: {ld:.4f} | G_loss: {lg:.4f}")
        d_losses.append(ld)
        g_losses.append(lg)
    return {"g_losses": g_losses, "d_losses": d_losses}


def counterfactual_batch(G, x, target):
    """countergan2.py:216-220 -- (clamp(x + delta, -1, 1), delta) under no_grad; target: the class of --target, or one class per row."""
    _need_gpu(x, "counterfactual_batch")
    if not torch.is_tensor(target):
        target = torch.full((x.shape[0],), int(target), dtype=torch.int64, device=x.device)       # :216
    return _gt.counterfactual_batch(G, x, target)


def save_examples(G, x, target, output_dir):
    """countergan2.py:213-224 -- the counterfactuals of one batch towards `target` and the files original.png, counterfactual.png,
    delta.png in output_dir (gan_train._example_sheets: the delta's `* 0.5 + 0.5` rides in the sheet's launches, from the raw delta).
    Returns (original, counterfactual, delta) as uint8 arrays."""
    cf, delta = counterfactual_batch(G, x, target)
    return _gt._example_sheets(x, cf, delta, output_dir)


def delta_image(delta):
    """countergan2.py:224 -- delta * 0.5 + 0.5, the picture of the change."""
    _need_gpu(delta, "delta_image")
    d = delta.detach().contiguous()
    out = ops.axpby(0.5, d)
    return ops.add_bias_rows(out, 1, torch.full((1,), 0.5, dtype=torch.float32, device=d.device))
