"""Host-side mirror of `conditional_counteRGAN/mnist/` on the HIP kernels.

    reference                                              here
    ---------------------------------------------------    -----------------------------------------------------
    config.py            Config            :3-28            Config (the fields the step reads)
    models/generator.py  ResidualGenerator :25-86           ResidualGenerator (same ctor args, same state_dict keys)
    models/discriminator.py Discriminator  :5-38            Discriminator
    models/classifier.py CNNClassifier     :4-28            CNNClassifier (frozen / eval use: forward + grad-input)
    modules/classifier.py Classifier       :4-30            Classifier, save_classifier, load_classifier (the max-pool net of countergan2.py /
                                                            gan_train.py; fit_pool_classifier: countergan2.py:120-151; get_pool_classifier:
                                                            gan_train.py:49-88)
    trainer.py           train_classifier  :8-39            train_classifier (fused=True: ClassifierFit, one graph replay per step)
    trainer.py           build_mask        :45-72           build_mask (same draws from torch's RNG)
    trainer.py           train_countergan  :76-123          make_optimizers + train_step (+ train_countergan loop)
    eval_utils.py        visualize_counterfactual_grid :113-201   pick_sources, counterfactual_grid (the data, not the figure)
    gr.py                make_and_save_heatmaps :346-441, save_user_modification_example :498-568
                                                            heatmap_batch, user_modification_example (likewise)

The torch layer objects are kept as parameter containers (identical `state_dict()` keys: `embed.weight`,
`conv_in.*`, `resblocks.{0..5}.{conv1,bn1,conv2,bn2}.*`, `conv_mid.*`, `conv_out.*`; `cond_embed.weight`, `main.{0,2,4,6}.weight`,
`adv_head.*`; `conv.{0,2,4}.*`, `fc.{1,4}.*`), forward/backward are one autograd node per network sequencing C-ABI
calls on NHWC activations.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._cfeval import confusion_csv, write_png_gray
from ._graphed import BatchWalkFit
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, PcgError
from .nn import weighted_sum, FlatModule, FrozenClassifier, in_conv_precision
from .optim import Adam


class Config:
    """config.py:3-28."""
    batch_size = 128
    num_epochs_gan = 20
    d_lr = 1e-5
    g_lr = 5e-5
    cls_lr = 1e-3
    num_epochs_clf = 10
    lambda_adv = 1.0
    lambda_cls = 1.0
    lambda_reg = 2.5
    lambda_mask = 2.0
    patch_size = 7
    num_modifiable_patches = 10
    img_shape = (1, 28, 28)
    num_classes = 10
    min_modifiable_patches = 6                       # config.py:18-20: the evaluation's patch prompts
    max_modifiable_patches = 15
    user_input_patches = [1, 5, 10, 12, 13, 14]
    device = "cuda"
    save_dir = "./results"


# ---- conv helpers on NHWC activations ------------------------------------------------------------------------------
def _geom(conv, B, H, W):
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    return ops.conv_geom(B, H, W, conv.in_channels, conv.out_channels, k[0], k[1], s[0], p[0])


def _conv_fwd(conv, a, act=ACT_NONE, slope=0.0):
    B, H, W, _ = a.shape
    g = _geom(conv, B, H, W)
    z = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data if conv.bias is not None else None, act=act, slope=slope)
    return g, z


def _conv_wgrad(net, conv, g, a, dz, need_p=True, bias_done=False):
    """Accumulate weight/bias gradients into net's flat buffer (bias_done: the bias gradient already came out of the BatchNorm
    backward's apply pass — ops.bn_act_bwd / bn_bwd_partial with dcol=)."""
    if need_p and conv.weight.requires_grad:
        gw, acc = net._grad_view(conv.weight)
        ops.conv2d_wgrad(g, a, dz, ops.ohwi(gw), acc)
        if conv.bias is not None and not bias_done:
            gb, accb = net._grad_view(conv.bias)
            ops.colsum(dz.numel() // conv.out_channels, conv.out_channels, dz, gb, accb)


def _conv_bwd(net, conv, g, a, dz, need_p, need_x):
    """Accumulate weight/bias gradients into net's flat buffer; return grad wrt the conv input (or None)."""
    _conv_wgrad(net, conv, g, a, dz, need_p)
    return ops.conv2d_dgrad(g, dz, ops.ohwi(conv.weight.data)) if need_x else None


def _dgrad_act(g, dz, w, a_below, act, slope):
    """conv_dgrad(dz, w) * act'(a_below): one launch when the layer is an MFMA layer, grad-input + pcg_act_bwd otherwise."""
    res = ops.conv_bwd_data_fused(g, dz, w, False, act, slope, a_below=a_below) if FUSE_BACKWARD_EPILOGUE else None
    if res is not None:
        return res[0]
    d = ops.conv2d_dgrad(g, dz, w)
    return ops.act_bwd(d, a_below.view(d.shape), act, slope, out=d)


S1_DGRAD_AS_FWD = os.environ.get("PCG_S1_DGRAD_AS_FWD", "1") != "0"   # A/B switch: stride-1 grad-inputs on the forward kernel (adjoint weight)
FUSE_SKIP_BNSUM = os.environ.get("PCG_SKIP_BNSUM", "1") != "0"   # A/B switch: bn2's backward column sums out of the previous block's skip-add grad-input epilogue
DEFER_SLAB_REDUCTIONS = os.environ.get("PCG_SLAB_DEFER", "0") != "0"   # opt-in A/B switch: one slab-reduction launch per backward sweep (ops.slab_reductions_deferred; 26.68 -> 26.64 ms)
GRAD_INPUT_LABEL_CHANNEL_ONLY = True   # A/B switch: conv_in's grad-input for the label-map channel only (see _run_backward)
FUSE_BIAS_COLSUM = True         # A/B switch: conv-bias gradients in front of a BatchNorm out of the BatchNorm backward's apply pass
FUSE_BACKWARD_EPILOGUE = True   # A/B switch for the tests: activation derivative / BatchNorm-backward sums / skip-connection add in
                                # the grad-input kernel's epilogue (ops.conv_bwd_data_fused, conv2d_dgrad_add) vs separate passes


def _as_rows(t, B):
    """[B,1,H,W] / [B,H,W] tensor as a contiguous fp32 [B, H*W] view (C == 1: NCHW and NHWC are the same bytes)."""
    v = t.reshape(B, -1)
    if not v.is_contiguous():
        v = v.contiguous()
    if v.dtype != torch.float32:
        raise PcgError(f"expected float32, got {v.dtype}")
    return v


# ---- small autograd nodes for the trainer's elementwise glue (trainer.py:97,99,119) ---------------------------------
class _ClampAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, lo, hi):
        xc, rc = x.contiguous(), r.contiguous()
        ctx.save_for_backward(xc, rc)
        ctx.lo, ctx.hi = lo, hi
        return ops.clamp_add_fwd(xc, rc, lo, hi)

    @staticmethod
    def backward(ctx, dy):
        x, r = ctx.saved_tensors
        return None, ops.clamp_add_bwd(dy.contiguous(), x, r, ctx.lo, ctx.hi), None, None


def clamp_add(x, r, lo=-1.0, hi=1.0):
    """torch.clamp(x + r, lo, hi) with gradient to r only (x is data)."""
    return _ClampAdd.apply(x, r, lo, hi)


class _AbsMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, m, one_minus):
        ac = a.contiguous()
        mc = m.contiguous() if m is not None else None
        ctx.save_for_backward(ac, mc)
        ctx.one_minus = one_minus
        return ops.abs_mean_fwd(ac, mc, one_minus).view(())

    @staticmethod
    def backward(ctx, g):
        a, m = ctx.saved_tensors
        return ops.abs_mean_bwd(a, m, ctx.one_minus, g.contiguous().view(1)), None, None


def abs_mean(a, m=None, one_minus=False):
    """mean(|a * w|) with w = m, (1 - m) or 1."""
    return _AbsMean.apply(a, m, one_minus)


class _BCELogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, target_const):
        zc = z.contiguous()
        ctx.save_for_backward(zc)
        ctx.t = target_const
        loss, _ = ops.bce_logits_fwd_bwd(zc, target_const, need_grad=False)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        _, dz = ops.bce_logits_fwd_bwd(z, ctx.t, need_loss=False, grad_out=g.contiguous().view(1))
        return dz, None


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() against an all-ones / all-zeros target (trainer.py:106-107,117 use ones_like / zeros_like)."""

    def forward(self, input, target):
        t = float(target) if not torch.is_tensor(target) else None
        if t is None:
            raise PcgError("BCEWithLogitsLoss here takes the constant target 0.0 or 1.0 (ones_like/zeros_like in the reference)")
        return _BCELogitsFn.apply(input, t)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        zc = logits.contiguous()
        ctx.save_for_backward(zc, target)
        loss, _ = ops.cross_entropy_fwd_bwd(zc, target, need_grad=False)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        z, target = ctx.saved_tensors
        _, dz = ops.cross_entropy_fwd_bwd(z, target, need_loss=False, grad_out=g.contiguous().view(1))
        return dz, None


class CrossEntropyLoss(nn.Module):
    def forward(self, input, target):
        return _CEFn.apply(input, target)


# ---- generator -----------------------------------------------------------------------------------------------------
class _ResBlock(nn.Module):
    """generator.py:5-22 (parameter container; executed by ResidualGenerator)."""

    def __init__(self, channels, activation):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, channels, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(channels)
        self.act = activation
        self.conv2 = nn.Conv2d(channels, channels, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(channels)


class _GFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, target, mask, *params):
        raw, masked, saved = net._run_forward(x, target, mask)
        ctx.net, ctx.saved = net, saved
        return raw, masked

    @staticmethod
    def backward(ctx, d_raw, d_masked):
        with ops.slab_reductions_deferred(DEFER_SLAB_REDUCTIONS):
            ctx.net._run_backward(ctx.saved, d_raw, d_masked, any(ctx.needs_input_grad[4:]))
        return (None,) * len(ctx.needs_input_grad)


class ResidualGenerator(FlatModule):
    """generator.py:25-86 — returns (raw_residual, masked_residual)."""

    honours_conv_precision = True   # conv_precision = "bf16" 

    def __init__(self, img_shape=(1, 28, 28), num_classes=10, base_ch=64, n_resblocks=6, residual_scaling=0.1):
        super().__init__()
        C, H, W = img_shape
        if C != 1:
            raise PcgError("ResidualGenerator: single-channel images only (the reference's MNIST configuration)")
        self.embed = nn.Embedding(num_classes, H * W)
        self.conv_in = nn.Conv2d(C + 2, base_ch, kernel_size=3, padding=1)
        self.act = nn.LeakyReLU(0.2, inplace=True)
        self.resblocks = nn.Sequential(*[_ResBlock(base_ch, self.act) for _ in range(n_resblocks)])
        self.conv_mid = nn.Conv2d(base_ch, base_ch, kernel_size=3, padding=1)
        self.conv_out = nn.Conv2d(base_ch, 1, kernel_size=3, padding=1)
        self.residual_scaling = residual_scaling
        self._hw = (H, W)
        self._fold_cache = None
        self._init_weights()

    # -- eval-mode BatchNorm folded into conv1 of every block (forward_queries) ----------------------------------
    def train(self, mode=True):
        # as CNNClassifier.train: the optimizer kernel updates parameters without touching torch's version counters
        self._fold_cache = None
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._fold_cache = None
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._fold_cache = None
        return super()._apply(fn, *args, **kwargs)

    def _fold_key(self):
        ts = [t for blk in self.resblocks for t in (blk.conv1.weight, blk.conv1.bias, blk.bn1.weight, blk.bn1.bias, blk.bn1.running_mean,
                                                    blk.bn1.running_var) if t is not None]
        return tuple((t.data_ptr(), t._version) for t in ts)

    def folded_conv1(self):
        """Per block (w' OHWI, b') with bn1's eval-mode affine folded into conv1: w' = w * s, b' = (b - mean) * s + beta,
        s = gamma / sqrt(var + eps) per output channel, computed in float64 and rounded once.  Cached on the module; the cache is
        dropped by train() / eval(), load_state_dict(), .to() and any change of a parameter's or buffer's storage or version."""
        if any(blk.bn1.training for blk in self.resblocks):
            raise PcgError("ResidualGenerator.folded_conv1: BatchNorm in training mode has no fixed affine to fold; call .eval()")
        key = self._fold_key()
        if self._fold_cache is not None and self._fold_cache[0] == key:
            return self._fold_cache[1]
        folded = []
        with torch.no_grad():
            for blk in self.resblocks:
                conv, bn = blk.conv1, blk.bn1
                s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
                w = (conv.weight.permute(0, 2, 3, 1).double() * s.view(-1, 1, 1, 1)).float().contiguous()
                b0 = conv.bias.double() if conv.bias is not None else torch.zeros_like(s)
                folded.append((w, ((b0 - bn.running_mean.double()) * s + bn.bias.double()).float().contiguous()))
        self._fold_cache = (key, folded)
        return folded

    @in_conv_precision
    def forward_queries(self, x, targets, mask, mask_mode="row", T=None, q0=0, nq=None, fold_eval_bn=True, want_residuals=True, out=None):
        """The eval-mode forward over the window [q0, q0 + nq) of the queries q = t * B + b (generator.py:71-84 + eval_utils.py:57).
        x [B,1,H,W] / [B,HW]; targets None: the sweep, query (t, b) asks for class t of T (default num_classes), or [B] int64 with
        T = 1; mask per mask_mode: "shared" [HW], "row" [B][HW], "query" [T*B][HW] — neither x nor the mask is replicated.
        One entry launch, the convolutions, one tail launch.  bn1 of every block runs folded into conv1's weights and LeakyReLU
        epilogue (fold_eval_bn=False: the conv + bn_apply_act chain of _run_forward); bn2 + skip stays one bn_apply_act pass.
        Returns {"x_cf" [nq,HW], "raw", "masked" ([nq,HW] or None), "sums" [nq,3]: sum |x_cf - x|, |raw * m|, |raw * (1 - m)|};
        `out`: preallocated tensors under those names."""
        if self.training or any(blk.bn1.training or blk.bn2.training for blk in self.resblocks):
            raise PcgError("ResidualGenerator.forward_queries is the eval-mode forward: call .eval() first")
        if not (torch.is_tensor(x) and x.is_cuda):
            raise PcgError(f"ResidualGenerator.forward_queries: x is on {getattr(x, 'device', type(x))}; libpcgan_hip has no CPU path")
        self._ensure_flat()
        H, W = self._hw
        B = x.shape[0]
        xr = _as_rows(x, B)
        if xr.shape[1] != H * W:
            raise PcgError(f"x: expected {H * W} pixels per row, got shape {tuple(x.shape)}")
        T = (self.embed.num_embeddings if targets is None else 1) if T is None else int(T)
        slope = float(self.act.negative_slope)
        if not torch.is_tensor(mask):
            raise PcgError("ResidualGenerator.forward_queries: a mask tensor is required")
        mk = mask.contiguous()
        inp = ops.mnist_cf_entry(xr, targets, self.embed.weight.data, mk, mask_mode, T, q0, nq)
        n = inp.shape[0]
        h = _conv_fwd(self.conv_in, inp.view(n, H, W, 3), ACT_LRELU, slope)[1]
        folded = self.folded_conv1() if fold_eval_bn else None
        for i, blk in enumerate(self.resblocks):
            if folded is not None:
                a1 = ops.conv2d_fwd(_geom(blk.conv1, n, H, W), h, folded[i][0], folded[i][1], act=ACT_LRELU, slope=slope)
            else:
                a1 = self._conv_bn(blk.conv1, blk.bn1, h, ACT_LRELU, slope)[2]
            h = self._conv_bn(blk.conv2, blk.bn2, a1, ACT_NONE, 0.0, residual=h, alpha=0.1)[2]                     # x + 0.1*out (:20)
        hm = _conv_fwd(self.conv_mid, h, ACT_LRELU, slope)[1]
        c = _conv_fwd(self.conv_out, hm)[1]
        x_cf, raw, masked, sums = ops.mnist_cf_tail(c.view(n, H * W), xr, mk, mask_mode, self.residual_scaling, T, q0, n,
                                                    want_residuals=want_residuals, out=out)
        return {"x_cf": x_cf, "raw": raw, "masked": masked, "sums": sums}

    def _init_weights(self):
        """generator.py:58-69."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, a=0.2)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, mean=0.0, std=0.01)

    def forward(self, x, target, mask=None):
        if mask is None:
            raise PcgError("ResidualGenerator: a mask is required (the reference only warns and then fails in torch.cat)")
        self._ensure_flat()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raw, masked = _GFn.apply(self, x, target, mask, *self.parameters())
        else:
            raw, masked, _ = self._run_forward(x, target, mask, keep=False)
        return raw, masked

    def _conv_bn(self, conv, bn, a, act, slope, residual=None, alpha=1.0):
        """conv -> BatchNorm (training: statistics fused into the conv epilogue) -> act, y = residual + alpha*act(bn(z))."""
        B, H, W, _ = a.shape
        g = _geom(conv, B, H, W)
        C = bn.num_features
        w, bias = ops.ohwi(conv.weight.data), (conv.bias.data if conv.bias is not None else None)
        if bn.training:
            z, mean, invstd = ops.conv_bn_train(g, a, w, bias, False, bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                                                bn.num_batches_tracked)
            y = ops.bn_apply_act(z, C, mean, invstd, bn.weight.data, bn.bias.data, act, slope, residual=residual, alpha=alpha)
            return g, z, y, mean, invstd
        z = ops.conv2d_fwd(g, a, w, bias)
        y = ops.bn_apply_act(z, C, bn.running_mean, bn.running_var, bn.weight.data, bn.bias.data, act, slope, var_eps=bn.eps,
                             residual=residual, alpha=alpha)
        return g, z, y, None, None

    @in_conv_precision
    def _run_forward(self, x, target, mask, keep=True):
        B = x.shape[0]
        H, W = self._hw
        xr, mr = _as_rows(x, B), _as_rows(mask, B)
        slope = float(self.act.negative_slope)
        inp = ops.embed_concat_fwd(xr, target, self.embed.weight.data, mr).view(B, H, W, 3)
        g_in, h = _conv_fwd(self.conv_in, inp, ACT_LRELU, slope)
        blocks = []
        for blk in self.resblocks:
            g1, z1, a1, m1, s1 = self._conv_bn(blk.conv1, blk.bn1, h, ACT_LRELU, slope)
            g2, z2, hn, m2, s2 = self._conv_bn(blk.conv2, blk.bn2, a1, ACT_NONE, 0.0, residual=h, alpha=0.1)   # x + 0.1*out (:20)
            if keep:
                blocks.append((g1, h, z1, a1, m1, s1, g2, z2, m2, s2))
            h = hn
        g_mid, hm = _conv_fwd(self.conv_mid, h, ACT_LRELU, slope)
        g_out, c = _conv_fwd(self.conv_out, hm)
        raw, masked = ops.scale_mask_fwd(c, mr, self.residual_scaling)
        saved = (inp, g_in, blocks, h, g_mid, hm, g_out, mr, target) if keep else None
        shp = (B, 1, H, W)
        return raw.view(shp), masked.view(shp), saved

    @in_conv_precision
    def _run_backward(self, saved, d_raw, d_masked, need_p):
        inp, g_in, blocks, h_last, g_mid, hm, g_out, mr, target = saved
        if not need_p:
            return
        if any(blk.bn1.training is False for blk in self.resblocks):
            raise PcgError("backward through an eval-mode BatchNorm2d is not implemented")
        slope = float(self.act.negative_slope)
        B = inp.shape[0]
        dr = d_raw.contiguous() if d_raw is not None else None
        dm = d_masked.contiguous() if d_masked is not None else None
        dc = ops.scale_mask_bwd(dr, dm, mr, self.residual_scaling, like=mr).view(g_out.B, g_out.OH, g_out.OW, 1)
        _conv_wgrad(self, self.conv_out, g_out, hm, dc, True)
        d = _dgrad_act(g_out, dc, ops.ohwi(self.conv_out.weight.data), hm, ACT_LRELU, slope)     # the mask rides in the thin expand kernel
        order = list(zip(reversed(self.resblocks), reversed(blocks)))
        # adjoint weights of every stride-1 conv whose grad-input runs on the forward kernel: ONE launch for all of them (r04; was one
        # 6 us launch in front of each of the 12 grad-inputs)
        adjw = {}
        if FUSE_BACKWARD_EPILOGUE and S1_DGRAD_AS_FWD:
            convs = [c for blk, sv in order for c, g_ in ((blk.conv2, sv[6]), (blk.conv1, sv[0])) if g_.stride == 1 and ops.xform_ok(g_, "x")]
            if FUSE_SKIP_BNSUM and order and g_mid.stride == 1 and ops.xform_ok(g_mid, "x"):
                convs.append(self.conv_mid)
            shapes = {tuple(c.weight.shape) for c in convs}
            if convs and len(shapes) == 1 and len(convs) <= 16:
                for c, wa in zip(convs, ops.conv_weight_adjoint_many([ops.ohwi(c.weight.data) for c in convs])):
                    adjw[id(c)] = wa

        def adjoint_of(conv):
            wa = adjw.get(id(conv))
            return wa if wa is not None else ops.conv_weight_adjoint(ops.ohwi(conv.weight.data))
        pending = None      # (partial, nparts): bn2's backward sums of the gradient `dh`, left by the previous block's skip-add epilogue
        # conv_mid's backward: weight / bias gradients, then its grad-input `dh` = the gradient of the last block's output — with the column
        # sums that block's bn2 backward needs, out of the same epilogue (r04: the head of the chain takes the no-addend form)
        _conv_wgrad(self, self.conv_mid, g_mid, h_last, d, True)
        head = order[0][1] if order else None
        adjm = FUSE_BACKWARD_EPILOGUE and S1_DGRAD_AS_FWD and FUSE_SKIP_BNSUM and head is not None and g_mid.stride == 1 and ops.xform_ok(g_mid, "x")
        if adjm:
            dh, part, nparts = ops.conv2d_dgrad_add(ops.adjoint_geom(g_mid), d, adjoint_of(self.conv_mid), None,
                                                    bnsum=(head[7], head[8], head[9], 0.1), transposed=True)
            pending = (part, nparts)
        else:
            dh = ops.conv2d_dgrad(g_mid, d, ops.ohwi(self.conv_mid.weight.data))
        h0_masked = False
        for bi, (blk, (g1, h, z1, a1, m1, s1, g2, z2, m2, s2)) in enumerate(order):
            C = blk.bn2.num_features
            dg2, acc = self._grad_view(blk.bn2.weight)
            db2, _ = self._grad_view(blk.bn2.bias)
            # the conv biases in front of the BatchNorms: their gradient is the column sum of dz, taken in the apply pass
            cb2, accb2 = self._grad_view(blk.conv2.bias) if (blk.conv2.bias is not None and FUSE_BIAS_COLSUM) else (None, False)
            if pending is not None:     # sums of 0.1*dh and 0.1*dh*xhat2 came with dh: no reduction pass over (dh, z2)
                dz2 = ops.bn_bwd_partial(dh, z2, C, m2, s2, blk.bn2.weight.data, pending[0], pending[1], dg2, db2, acc, dcol=cb2,
                                         accumulate_col=accb2, dm_scale=0.1)
            else:
                dz2 = ops.bn_act_bwd(dh, z2, None, C, m2, s2, blk.bn2.weight.data, ACT_NONE, 0.0, dg2, db2, acc, dy_scale=0.1,
                                     dcol=cb2, accumulate_col=accb2)
            pending = None
            _conv_wgrad(self, blk.conv2, g2, a1, dz2, bias_done=cb2 is not None)
            dg1, acc = self._grad_view(blk.bn1.weight)
            db1, _ = self._grad_view(blk.bn1.bias)
            # stride-1 layers: the grad-input runs on the FORWARD kernel with the adjoint weight (both operands K-major)
            adj = FUSE_BACKWARD_EPILOGUE and S1_DGRAD_AS_FWD and g2.stride == 1 and ops.xform_ok(g2, "x")
            if adj:
                res = ops.conv_bwd_data_fused(ops.adjoint_geom(g2), dz2, adjoint_of(blk.conv2), True,
                                              ACT_LRELU, slope, z_below=z1, bn=(m1, s1, blk.bn1.weight.data, blk.bn1.bias.data))
            else:
                res = (ops.conv_bwd_data_fused(g2, dz2, ops.ohwi(blk.conv2.weight.data), False, ACT_LRELU, slope, z_below=z1,
                                               bn=(m1, s1, blk.bn1.weight.data, blk.bn1.bias.data)) if FUSE_BACKWARD_EPILOGUE else None)
            cb1, accb1 = self._grad_view(blk.conv1.bias) if (blk.conv1.bias is not None and FUSE_BIAS_COLSUM) else (None, False)
            if res is not None:      # LeakyReLU mask + BatchNorm-backward column sums came out of conv2's grad-input epilogue
                dz1 = ops.bn_bwd_partial(res[0], z1, C, m1, s1, blk.bn1.weight.data, res[1], res[2], dg1, db1, acc, out=res[0],
                                         dcol=cb1, accumulate_col=accb1)
            else:
                da1 = ops.conv2d_dgrad(g2, dz2, ops.ohwi(blk.conv2.weight.data))
                dz1 = ops.bn_act_bwd(da1, z1, None, C, m1, s1, blk.bn1.weight.data, ACT_LRELU, slope, dg1, db1, acc, beta=blk.bn1.bias.data,
                                     dcol=cb1, accumulate_col=accb1)
            _conv_wgrad(self, blk.conv1, g1, h, dz1, bias_done=cb1 is not None)
            if FUSE_BACKWARD_EPILOGUE:   # skip path + block path: the add happens in conv1's grad-input epilogue, in place
                nxt = order[bi + 1][1] if (bi + 1 < len(order) and FUSE_SKIP_BNSUM) else None
                adj1 = S1_DGRAD_AS_FWD and g1.stride == 1 and ops.xform_ok(g1, "x")
                ga, wa = ((ops.adjoint_geom(g1), adjoint_of(blk.conv1)) if adj1
                          else (g1, ops.ohwi(blk.conv1.weight.data)))
                if nxt is not None:      # ... together with the BatchNorm-backward sums the NEXT block's bn2 needs from this sum
                    dh, part, nparts = ops.conv2d_dgrad_add(ga, dz1, wa, dh, out=dh, bnsum=(nxt[7], nxt[8], nxt[9], 0.1), transposed=adj1)
                    pending = (part, nparts)
                elif bi + 1 == len(order):   # the chain's last sum is the gradient w.r.t. h0 = LeakyReLU(conv_in(inp)): its mask in the same epilogue
                    dh = ops.conv2d_dgrad_add_mask(ga, dz1, wa, dh, h, ACT_LRELU, slope, out=dh, transposed=adj1)
                    h0_masked = True
                else:
                    dh = ops.conv2d_dgrad_add(ga, dz1, wa, dh, out=dh, transposed=adj1)
            else:
                dconv = ops.conv2d_dgrad(g1, dz1, ops.ohwi(blk.conv1.weight.data))
                dh = ops.axpby(1.0, dh, 1.0, dconv, out=dconv)
        if not h0_masked:
            ops.act_bwd(dh, blocks[0][1] if blocks else h_last, ACT_LRELU, slope, out=dh)   # h0 = LeakyReLU(conv_in(inp))
        _conv_wgrad(self, self.conv_in, g_in, inp, dh, True)
        ge, acc = self._grad_view(self.embed.weight)
        if GRAD_INPUT_LABEL_CHANNEL_ONLY and g_in.Cin == 3:
            # of conv_in's three input channels (image, label map, mask: generator.py:73-74) only the label map has a consumer — the
            # embedding table.  Its grad-input is the one-channel convolution with that channel's weights: 9 tap products per pixel
            # instead of 27 (r04 census: 118 + 46 us -> 55 + 26)
            g1 = ops.conv_geom(g_in.B, g_in.IH, g_in.IW, 1, g_in.Cout, g_in.KH, g_in.KW, g_in.stride, g_in.pad)
            d1 = ops.conv2d_dgrad(g1, dh, ops.gather_channel(ops.ohwi(self.conv_in.weight.data), 1))
            ops.embed_table_grad(d1, target, 1, 0, self.embed.num_embeddings, ge, accumulate=acc)
        else:
            dinp = ops.conv2d_dgrad(g_in, dh, ops.ohwi(self.conv_in.weight.data))
            ops.embed_concat_bwd(dinp, target, 3, self.embed.num_embeddings, dtable=ge, accumulate=acc)


# ---- discriminator ----------------------------------------------------------------------------------------------------
class _DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, cond_idx, *params):
        out, saved = net._run_forward(x, cond_idx)
        ctx.net, ctx.saved = net, saved
        return out

    @staticmethod
    def backward(ctx, dlogits):
        with ops.slab_reductions_deferred(DEFER_SLAB_REDUCTIONS):
            dx = ctx.net._run_backward(ctx.saved, dlogits, ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:]))
        return (None, dx) + (None,) * (len(ctx.needs_input_grad) - 2)


class Discriminator(FlatModule):
    """discriminator.py:5-38 — logits [B, 1]."""

    honours_conv_precision = True   # conv_precision = "bf16" 

    def __init__(self, img_shape=(1, 28, 28), num_classes=Config.num_classes):
        super().__init__()
        C, H, W = img_shape
        self.cond_embed = nn.Embedding(num_classes, H * W)
        self.img_channel = 2
        self.d_hidden = 64
        d = self.d_hidden
        self.main = nn.Sequential(
            nn.Conv2d(self.img_channel, d, 3, 2, 1, bias=False), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(d, d * 2, 3, 2, 1, bias=False), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(d * 2, d * 4, 3, 2, 1, bias=False), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(d * 4, d * 4, 3, 2, 1, bias=False), nn.LeakyReLU(0.2, inplace=True),
            nn.AdaptiveAvgPool2d(1),
        )
        self.flatten = nn.Flatten()
        self.adv_head = nn.Linear(d * 4, 1)
        self._hw = (H, W)

    def _convs(self):
        return [m for m in self.main if isinstance(m, nn.Conv2d)]

    def forward(self, x, cond_idx):
        self._ensure_flat()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _DFn.apply(self, x, cond_idx, *self.parameters())
        return self._run_forward(x, cond_idx, keep=False)[0]

    @in_conv_precision
    def _run_forward(self, x, cond_idx, keep=True):
        B = x.shape[0]
        H, W = self._hw
        a = ops.embed_concat_fwd(_as_rows(x, B), cond_idx, self.cond_embed.weight.data, None).view(B, H, W, 2)
        layers = []
        for conv in self._convs():
            g, z = _conv_fwd(conv, a, ACT_LRELU, 0.2)
            if keep:
                layers.append((g, a, z))
            a = z
        Bq, Hq, Wq, Cq = a.shape
        pooled = ops.avgpool_fwd(a, B, Hq * Wq, Cq)
        gl = ops.conv_geom(B, 1, 1, Cq, 1, 1, 1, 1, 0)
        logits = ops.conv2d_fwd(gl, pooled, self.adv_head.weight.data, self.adv_head.bias.data).view(B, 1)
        saved = (layers, pooled, gl, (Hq * Wq, Cq), cond_idx) if keep else None
        return logits, saved

    @in_conv_precision
    def _run_backward(self, saved, dlogits, need_x, need_p):
        layers, pooled, gl, (HWq, Cq), cond_idx = saved
        B = pooled.shape[0]
        dl = dlogits.contiguous()
        head = self.adv_head
        if need_p and head.weight.requires_grad:
            gw, acc = self._grad_view(head.weight)
            ops.conv2d_wgrad(gl, pooled, dl, gw, acc)
            gb, accb = self._grad_view(head.bias)
            ops.colsum(B, 1, dl, gb, accb)
        dpool = ops.conv2d_dgrad(gl, dl, head.weight.data)
        d = ops.avgpool_bwd(dpool, B, HWq, Cq).view(layers[-1][2].shape)
        convs = self._convs()
        masked = False          # d already carries the LeakyReLU derivative of layer i (applied in layer i+1's grad-input epilogue)
        for i in range(len(convs) - 1, -1, -1):
            g, a, y = layers[i]
            if not masked:
                ops.act_bwd(d, y, ACT_LRELU, 0.2, out=d)
            last = i == 0
            need_in = (not last) or need_x or (need_p and self.cond_embed.weight.requires_grad)
            _conv_wgrad(self, convs[i], g, a, d, need_p)
            masked = False
            if not need_in:
                d = None
                continue
            w = ops.ohwi(convs[i].weight.data)
            if last and not need_x and GRAD_INPUT_LABEL_CHANNEL_ONLY and g.Cin == 2:
                # D(real) / D(fake.detach()): of the entry conv's two input channels (image, label map: discriminator.py:35-36) only
                # the label map has a consumer, the embedding table — 9 tap products per pixel instead of 18
                g1 = ops.conv_geom(g.B, g.IH, g.IW, 1, g.Cout, g.KH, g.KW, g.stride, g.pad)
                d1 = ops.conv2d_dgrad(g1, d, ops.gather_channel(w, 1))
                ge, acc = self._grad_view(self.cond_embed.weight)
                ops.embed_table_grad(d1, cond_idx, 1, 0, self.cond_embed.num_embeddings, ge, accumulate=acc)
                return None
            res = ops.conv_bwd_data_fused(g, d, w, False, ACT_LRELU, 0.2, a_below=a) if (not last and FUSE_BACKWARD_EPILOGUE) else None
            if res is not None:
                d, masked = res[0], True
            else:
                d = ops.conv2d_dgrad(g, d, w)
        if d is None:
            return None
        ge, acc = (self._grad_view(self.cond_embed.weight) if need_p and self.cond_embed.weight.requires_grad else (None, False))
        dx = ops.embed_concat_bwd(d, cond_idx, 2, self.cond_embed.num_embeddings, dtable=ge, accumulate=acc, need_dx=need_x)
        H, W = self._hw
        return dx.view(B, 1, H, W) if need_x else None


# ---- frozen classifier -----------------------------------------------------------------------------------------------
class CNNClassifier(FrozenClassifier):
    """classifier.py:4-28.  In the GAN step it is frozen and in eval mode (main.py:30-33): forward and the gradient with
    respect to the input image, on packed weights.  In training mode (pre-training, trainer.py:8-39 — SURVEY.md section 8f
    item 3) it is a regular trainable net: Dropout2d(0.25) / Dropout(0.5) masks come from `self.rng` (a device Philox
    stream) or, for runs that must reproduce given draws, from `self.dropout_masks = [mask2d [B,128], mask [B,256]]`."""

    honours_conv_precision = True   # conv_precision = "bf16" 

    def __init__(self, num_classes=10):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(1, 32, 3, 1, 1), nn.ReLU(),
            nn.Conv2d(32, 64, 3, 2, 1), nn.ReLU(),
            nn.Conv2d(64, 128, 3, 2, 1), nn.ReLU(),
            nn.Dropout2d(0.25),
        )
        self.fc = nn.Sequential(nn.Flatten(), nn.Linear(128 * 7 * 7, 256), nn.ReLU(), nn.Dropout(0.5), nn.Linear(256, num_classes))
        self.num_classes = num_classes

    def _pack(self):
        """NHWC / 4-aligned images of the frozen weights (rebuilt if the parameters change): conv weights OHWI; fc1 columns
        re-ordered from (c,h,w) to (h,w,c) so it consumes the NHWC activation; fc2 padded from 10 to 12 outputs (16-byte
        rows).  One-time setup copies, not part of the step."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        if self.training:
            raise PcgError("CNNClassifier: only eval mode is implemented (the GAN step uses the frozen classifier)")
        convs = [m for m in self.conv if isinstance(m, nn.Conv2d)]
        fc1, fc2 = self.fc[1], self.fc[4]
        with torch.no_grad():
            cw = [(c, c.weight.permute(0, 2, 3, 1).contiguous(), c.bias.contiguous()) for c in convs]
            w1 = fc1.weight.view(fc1.out_features, 128, 7, 7).permute(0, 2, 3, 1).contiguous().view(fc1.out_features, -1)
            kp = (self.num_classes + 3) // 4 * 4
            w2 = torch.zeros(kp, fc2.in_features, device=fc2.weight.device)
            w2[: self.num_classes] = fc2.weight
            b2 = torch.zeros(kp, device=fc2.weight.device)
            b2[: self.num_classes] = fc2.bias
        packed = (cw, w1, fc1.bias.contiguous(), w2, b2, kp)
        self._packed = (key, packed)
        return packed

    def _draw_dropout_masks(self, x):
        B = x.shape[0]
        return [self.rng.bernoulli((B, 128), x.device, 0.75), self.rng.bernoulli((B, 256), x.device, 0.5)]

    # -- training mode (trainer.py:15-20) ------------------------------------------------------------------------------------
    @in_conv_precision
    def _train_forward(self, x, masks):
        from .nn import linear_fwd
        B = x.shape[0]
        a = _as_rows(x, B).view(B, 28, 28, 1)
        layers = []
        for conv in (m for m in self.conv if isinstance(m, nn.Conv2d)):
            g, y = _conv_fwd(conv, a, ACT_RELU)
            layers.append((conv, g, a, y))
            a = y
        m2d, m1 = masks
        HW, C = a.shape[1] * a.shape[2], a.shape[3]
        ad = ops.dropout_apply(a, m2d.contiguous(), 0.25, inner=HW, C=C)                       # Dropout2d(0.25) :13
        flat = ops.nhwc_to_nchw_flat(ad, B, HW, C).view(B, HW * C)                            # nn.Flatten of the NCHW tensor :16
        fc1, fc2 = self.fc[1], self.fc[4]
        h = linear_fwd(fc1, flat)
        ops.act_fwd(h, ACT_RELU, 0.0, out=h)
        hd = ops.dropout_apply(h, m1.contiguous(), 0.5)                                       # Dropout(0.5) :19
        logits = linear_fwd(fc2, hd)
        return logits, (layers, m2d, m1, flat, h, hd, (HW, C))

    @in_conv_precision
    def _train_backward(self, saved, dlogits):
        from .nn import linear_dgrad, linear_wgrad
        layers, m2d, m1, flat, h, hd, (HW, C) = saved
        B = flat.shape[0]
        fc1, fc2 = self.fc[1], self.fc[4]
        dl = dlogits.contiguous()
        linear_wgrad(self, fc2, hd, dl)
        d = linear_dgrad(fc2.weight.data, dl, B)
        d = ops.dropout_apply(d, m1.contiguous(), 0.5, out=d)
        ops.act_bwd(d, h, ACT_RELU, 0.0, out=d)
        linear_wgrad(self, fc1, flat, d)
        d = linear_dgrad(fc1.weight.data, d, B)
        d = ops.nhwc_to_nchw_flat(d, B, HW, C, inverse=True).view(layers[-1][3].shape)
        d = ops.dropout_apply(d, m2d.contiguous(), 0.25, inner=HW, C=C, out=d)
        for i in range(len(layers) - 1, -1, -1):
            conv, g, a, y = layers[i]
            ops.act_bwd(d, y, ACT_RELU, 0.0, out=d)
            d = _conv_bwd(self, conv, g, a, d, True, i > 0)

    @in_conv_precision
    def _run_forward(self, x, keep=True):
        cw, w1, b1, w2, b2, kp = self._pack()
        B = x.shape[0]
        a = _as_rows(x, B).view(B, 28, 28, 1)
        layers = []
        for conv, w, b in cw:
            Bq, H, W, _ = a.shape
            g = _geom(conv, B, H, W)
            z = ops.conv2d_fwd(g, a, w, b, act=ACT_RELU)
            if keep:
                layers.append((g, w, z))
            a = z
        feat = a.numel() // B
        g1 = ops.conv_geom(B, 1, 1, feat, w1.shape[0], 1, 1, 1, 0)
        h = ops.conv2d_fwd(g1, a.view(B, 1, 1, feat), w1, b1, act=ACT_RELU)
        g2 = ops.conv_geom(B, 1, 1, w1.shape[0], kp, 1, 1, 1, 0)
        logits = ops.conv2d_fwd(g2, h, w2, b2).view(B, kp)[:, : self.num_classes]
        saved = (layers, g1, w1, h, g2, w2, kp) if keep else None
        return logits, saved

    @in_conv_precision
    def _run_backward(self, saved, dlogits):
        layers, g1, w1, h, g2, w2, kp = saved
        B = dlogits.shape[0]
        dl = torch.empty((B, kp), dtype=torch.float32, device=dlogits.device)
        ops.fill(dl, 0.0)
        dl[:, : self.num_classes].copy_(dlogits)      # pad 10 -> 12 columns (tiny strided copy)
        d = _dgrad_act(g2, dl, w2, h, ACT_RELU, 0.0)
        d = _dgrad_act(g1, d, w1, layers[-1][2], ACT_RELU, 0.0)
        for idx in range(len(layers) - 1, -1, -1):
            g, w, y = layers[idx]
            d = d.view(y.shape)
            d = _dgrad_act(g, d, w, layers[idx - 1][2], ACT_RELU, 0.0) if idx > 0 else ops.conv2d_dgrad(g, d, w)
        return d.view(B, 1, 28, 28)


# ---- the max-pool classifier of countergan2.py / gan_train.py (modules/classifier.py) ---------------------------------------------
class Classifier(FrozenClassifier):
    """modules/classifier.py:4-21 — Conv(1->32, k3 p1), ReLU, MaxPool2d(2), Conv(32->64, k3 p1), ReLU, MaxPool2d(2), Flatten,
    Linear(3136->128), ReLU, Linear(128->10) under `self.net`, the reference's nn.Sequential: state_dict() keys `net.{0,3,7,9}.*` and
    shapes are the reference's, so the shipped models/classifier.pt loads with strict=True and ours loads into the reference's module.
    ReLU + MaxPool2d are one launch each way (ops.relu_maxpool2_fwd / _bwd): the forward keeps the pooled tensor and
    the window positions, never the un-pooled convolution output.  Frozen / eval: forward and input gradient in six launches each, on
    packed weights.  Training mode: a regular trainable net (fit_pool_classifier); it has no Dropout."""

    honours_conv_precision = True   # conv2 and fc1 are implicit-GEMM layers; the pooling kernels are fp32 either way

    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
            nn.Flatten(), nn.Linear(64 * 7 * 7, 128), nn.ReLU(), nn.Linear(128, 10),
        )
        self.num_classes = 10

    def _pack(self):
        """Images of the frozen weights (rebuilt if the parameters change): conv weights OHWI; net.7's columns re-ordered from
        (c,h,w) to (h,w,c) so it consumes the NHWC pooled tensor with no flatten launch; net.9 padded from 10 to 12 outputs
        (16-byte rows), as CNNClassifier pads its head.  One-time setup copies, not part of the step."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        if self.training:
            raise PcgError("Classifier: the packed path is the eval path (training mode runs on the trainable parameters)")
        c1, c2, fc1, fc2 = self.net[0], self.net[3], self.net[7], self.net[9]
        with torch.no_grad():
            cw = [(c, c.weight.permute(0, 2, 3, 1).contiguous(), c.bias.contiguous()) for c in (c1, c2)]
            w1 = fc1.weight.view(fc1.out_features, 64, 7, 7).permute(0, 2, 3, 1).contiguous().view(fc1.out_features, -1)
            kp = (self.num_classes + 3) // 4 * 4
            w2 = torch.zeros(kp, fc2.in_features, device=fc2.weight.device)
            w2[: self.num_classes] = fc2.weight
            b2 = torch.zeros(kp, device=fc2.weight.device)
            b2[: self.num_classes] = fc2.bias
        packed = (cw, w1, fc1.bias.contiguous(), w2, b2, kp)
        self._packed = (key, packed)
        return packed

    def _draw_dropout_masks(self, x):
        return []                                     # the net has no Dropout

    # -- frozen / eval -----------------------------------------------------------------------------------------------------------
    def _logits_padded(self, a, keep, out=None):
        """Six launches from the NHWC image a [B, 28, 28, 1] to the padded logits [B, kp]: conv1 (thin), pool, conv2, pool, fc1 as a
        1x1 convolution with ReLU, fc2.  The convolutions write their raw output; the pooling kernel applies the ReLU."""
        cw, w1, b1, w2, b2, kp = self._pack()
        B = a.shape[0]
        pooled = []
        for conv, w, b in cw:
            g = _geom(conv, B, a.shape[1], a.shape[2])
            p, idx = ops.relu_maxpool2_fwd(ops.conv2d_fwd(g, a, w, b))
            pooled.append((g, w, p, idx))
            a = p
        feat = a.numel() // B
        g1 = ops.conv_geom(B, 1, 1, feat, w1.shape[0], 1, 1, 1, 0)
        h = ops.conv2d_fwd(g1, a.view(B, 1, 1, feat), w1, b1, act=ACT_RELU)
        g2 = ops.conv_geom(B, 1, 1, w1.shape[0], kp, 1, 1, 1, 0)
        logits = ops.conv2d_fwd(g2, h, w2, b2, out=out).view(B, kp)
        if not keep:
            return logits, None
        (gc1, wc1, p1, idx1), (gc2, wc2, p2, idx2) = pooled
        return logits, dict(p1=p1, idx1=idx1, p2=p2, idx2=idx2, h=h, geoms=(gc1, gc2, g1, g2), weights=(wc1, wc2, w1, w2), kp=kp)

    @in_conv_precision
    def _run_forward(self, x, keep=True):
        B = x.shape[0]
        logits, saved = self._logits_padded(_as_rows(x, B).view(B, 28, 28, 1), keep)
        return logits[:, : self.num_classes], saved

    @in_conv_precision
    def padded_logits(self, rows, out=None):
        """The eval forward on image rows [n, 784] with the padded columns kept ([n, kp], kp = 12) and an optional destination:
        what the counterfactual front ends' score kernel reads."""
        n = rows.shape[0]
        return self._logits_padded(rows.view(n, 28, 28, 1), False, out=out)[0]

    @in_conv_precision
    def _run_backward(self, saved, dlogits):
        """The input gradient in six launches: fc2 grad-input with h's ReLU, fc1 grad-input, pool backward, conv2 grad-input, pool
        backward, conv1 grad-input.  The pool backward applies the ReLU mask of the layer below it (p > 0), so the grad-inputs that
        feed it carry no activation."""
        gc1, gc2, g1, g2 = saved["geoms"]
        wc1, wc2, w1, w2 = saved["weights"]
        kp = saved["kp"]
        B = dlogits.shape[0]
        dl = torch.empty((B, kp), dtype=torch.float32, device=dlogits.device)
        ops.fill(dl, 0.0)
        dl[:, : self.num_classes].copy_(dlogits)      # pad 10 -> 12 columns (tiny strided copy)
        d = _dgrad_act(g2, dl, w2, saved["h"], ACT_RELU, 0.0)
        d = ops.conv2d_dgrad(g1, d, w1).view(saved["p2"].shape)
        d = ops.relu_maxpool2_bwd(d, saved["p2"], saved["idx2"], (gc2.OH, gc2.OW))
        d = ops.conv2d_dgrad(gc2, d, wc2).view(saved["p1"].shape)
        d = ops.relu_maxpool2_bwd(d, saved["p1"], saved["idx1"], (gc1.OH, gc1.OW))
        return ops.conv2d_dgrad(gc1, d, wc1).view(B, 1, 28, 28)

    # -- training mode (countergan2.py:127-136) -------------------------------------------------------------------------------------
    @in_conv_precision
    def _train_forward(self, x, masks):
        from .nn import linear_fwd
        B = x.shape[0]
        c1, c2, fc1, fc2 = self.net[0], self.net[3], self.net[7], self.net[9]
        a0 = _as_rows(x, B).view(B, 28, 28, 1)
        g1, z1 = _conv_fwd(c1, a0)
        p1, idx1 = ops.relu_maxpool2_fwd(z1)
        g2, z2 = _conv_fwd(c2, p1)
        p2, idx2 = ops.relu_maxpool2_fwd(z2)
        HW, C = p2.shape[1] * p2.shape[2], p2.shape[3]
        flat = ops.nhwc_to_nchw_flat(p2, B, HW, C).view(B, HW * C)        # nn.Flatten of the NCHW tensor: net.7's own column order
        h = linear_fwd(fc1, flat, act=ACT_RELU)
        logits = linear_fwd(fc2, h)
        return logits, (a0, g1, p1, idx1, g2, p2, idx2, flat, h)

    @in_conv_precision
    def _train_backward(self, saved, dlogits):
        from .nn import linear_dgrad, linear_wgrad
        a0, g1, p1, idx1, g2, p2, idx2, flat, h = saved
        B = flat.shape[0]
        c1, c2, fc1, fc2 = self.net[0], self.net[3], self.net[7], self.net[9]
        dl = dlogits.contiguous()
        linear_wgrad(self, fc2, h, dl)
        d = linear_dgrad(fc2.weight.data, dl, B)
        ops.act_bwd(d, h, ACT_RELU, 0.0, out=d)
        linear_wgrad(self, fc1, flat, d)
        d = linear_dgrad(fc1.weight.data, d, B)
        d = ops.nhwc_to_nchw_flat(d, B, p2.shape[1] * p2.shape[2], p2.shape[3], inverse=True).view(p2.shape)
        d = ops.relu_maxpool2_bwd(d, p2, idx2, (g2.OH, g2.OW))
        d = _conv_bwd(self, c2, g2, p1, d, True, True).view(p1.shape)
        d = ops.relu_maxpool2_bwd(d, p1, idx1, (g1.OH, g1.OW))
        _conv_bwd(self, c1, g1, a0, d, True, False)


def save_classifier(model, path):
    """modules/classifier.py:23-24."""
    torch.save({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}, path)


def load_classifier(path, device):
    """modules/classifier.py:26-30: a Classifier with the checkpoint's weights, on `device`, in eval mode."""
    model = Classifier()
    model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=True)
    return model.to(device).eval()


def pool_fit_step(classifier, optimizer, x, y, ones, tally, loss_out=None):
    """One iteration of countergan2.py:129-136: forward, mean cross-entropy, backward, Adam.  The loss, its gradient and the epoch's
    running sum (tally += loss * rows, hits, rows) come out of one launch; nothing is read back."""
    optimizer.zero_grad()
    logits = classifier(x)
    lc = logits.detach().contiguous()
    dl = torch.empty_like(lc)
    ops.ce_weighted_tally(lc, y, ones, tally, dlogits=dl, seg_loss=loss_out)
    logits.backward(dl)
    optimizer.step()


def fit_pool_classifier(classifier, train_loader, valid_loader, epochs=10, lr=1e-3, device=Config.device):
    """countergan2.py:120-151 — Adam(lr), CrossEntropyLoss, per-epoch train and validation loss (sum of loss * rows / rows).  The
    sums stay on the device (ops.ce_weighted_tally) and each epoch makes ONE host read.  Returns (train_losses, valid_losses)."""
    classifier.to(device)
    optimizer = Adam(classifier.parameters(), lr=lr)
    ones = torch.ones(classifier.num_classes, dtype=torch.float32, device=device)
    tallies = torch.zeros(2, 3, dtype=torch.float64, device=device)
    train_losses, valid_losses = [], []
    for epoch in range(epochs):
        ops.fill(tallies.view(torch.float32), 0.0)
        classifier.train()
        for x, y in train_loader:
            pool_fit_step(classifier, optimizer, x.to(device), y.to(device), ones, tallies[0])
        classifier.eval()
        with torch.no_grad():
            for x, y in valid_loader:
                ops.ce_weighted_tally(classifier(x.to(device)).contiguous(), y.to(device), ones, tallies[1])
        t = tallies.cpu()                                                          # the epoch's one host read
        train_losses.append(float(t[0, 0] / max(float(t[0, 2]), 1.0)))
        valid_losses.append(float(t[1, 0] / max(float(t[1, 2]), 1.0)))
        print(f"Epoch {epoch + 1} - Train loss: {train_losses[-1]:.4f} | Valid loss: {valid_losses[-1]:.4f}")
    return train_losses, valid_losses


def get_pool_classifier(path, train_loader=None, valid_loader=None, epochs=10, lr=1e-3, device=Config.device):
    """gan_train.py:49-88 — load the classifier if `path` exists, else fit one (fit_pool_classifier) and save it there.  Returns the
    net in eval mode."""
    if os.path.exists(path):
        return load_classifier(path, device)
    if train_loader is None or valid_loader is None:
        raise PcgError(f"get_pool_classifier: {path} does not exist and no loaders were given to fit a classifier")
    classifier = Classifier().to(device)
    fit_pool_classifier(classifier, train_loader, valid_loader, epochs=epochs, lr=lr, device=device)
    save_classifier(classifier, path)
    return classifier.eval()


# ---- trainer ------------------------------------------------------------------------------------------------------------
def build_mask(x, patch_size, device, num_modifiable_patches=None):
    """trainer.py:45-72 — same draws from torch's RNG as the reference (host loop over the batch; moving this to the
    device is SURVEY.md §8f item 1)."""
    bs, c, h, w = x.shape
    nph, npw = h // patch_size, w // patch_size
    total = nph * npw
    patch_mask = torch.zeros((bs, 1, nph, npw), device=device)
    if num_modifiable_patches is None or num_modifiable_patches >= total:
        patch_mask = torch.randint(0, 2, patch_mask.shape, device=device).float()
    else:
        for b in range(bs):
            idx = torch.randperm(total, device=device)[:num_modifiable_patches]
            patch_mask.view(bs, -1)[b, idx] = 1.0
    return F.interpolate(patch_mask, size=(h, w), mode="nearest").repeat(1, c, 1, 1)


def build_mask_device(rng, x, patch_size, num_modifiable_patches):
    """build_mask on the GPU (one kernel instead of a host loop of B randperm calls): same distribution — every sample
    gets exactly `num_modifiable_patches` distinct patches, uniformly — from the engine's Philox stream `rng`
    (ops.DeviceRNG) rather than torch's generator."""
    bs, c, h, w = x.shape
    if c != 1:
        raise PcgError("build_mask_device: single-channel images only")
    total = (h // patch_size) * (w // patch_size)
    if num_modifiable_patches is None or num_modifiable_patches >= total:
        raise PcgError("build_mask_device: the Bernoulli-per-patch branch (trainer.py:58-60) is not implemented")
    return rng.patch_mask(bs, h, w, patch_size, num_modifiable_patches, x.device)


def evaluate_counterfactuals(generator, classifier, x, y_true, y_target, device=None):
    """eval_utils.py:46-79 — eval-mode generator with an all-ones mask, clamp to [-1, 1], classifier; returns
    ({class_flip_rate, prediction_gain, actionability}, (x_vis, x_cf_vis) in [0, 1])."""
    classifier.eval(); generator.eval()
    device = device if device is not None else next(generator.parameters()).device
    x, y_true, y_target = x.to(device), y_true.to(device), y_target.to(device)
    with torch.no_grad():
        ones = torch.empty_like(x)
        ops.fill(ones, 1.0)
        residual = generator(x, y_target, ones)[1]                                          # :55
        x_cf = clamp_add(x, residual, -1.0, 1.0)                                            # :57
        logits = classifier(x_cf)                                                           # :58
        m = ops.cf_metrics(logits.contiguous(), y_target, other=y_true).cpu()               # :61-64
        diff = ops.axpby(1.0, x_cf, -1.0, x.contiguous())
        actionability = abs_mean(diff).item()                                               # :66
        x_vis = ops.axpby(0.5, x.contiguous(), out=None).add_(0.5).cpu()                    # :69-70 ([-1,1] -> [0,1]; host-side view)
        x_cf_vis = ops.axpby(0.5, x_cf).add_(0.5).cpu()
    return {"class_flip_rate": float(m[0]), "prediction_gain": float(m[1]), "actionability": actionability}, (x_vis, x_cf_vis)


def generate_counterfactuals(generator, classifier, x, y, y_target, mask, device=None):
    """eval_utils.py:489-497."""
    generator.eval(); classifier.eval()
    with torch.no_grad():
        raw_residual, masked_residual = generator(x, y_target, mask)
        x_cf = clamp_add(x, masked_residual, -1.0, 1.0)
    return raw_residual, masked_residual, x_cf


_fused_fallback_warned = False


def _warn_fused_fallback(why):
    global _fused_fallback_warned
    if not _fused_fallback_warned:
        import warnings
        warnings.warn(f"train_classifier(fused=True): {why}; running the op chain instead", RuntimeWarning, stacklevel=3)
        _fused_fallback_warned = True


class ClassifierFit(BatchWalkFit):
    """The classifier pre-training step (trainer.py:16-21) with fused launches around the three convolutions (csrc/mnist_clf.hip;
    DESIGN.md §3.17): the batch gather with the two Dropout masks, conv1..3 with their ReLU, Dropout2d + Flatten, fc1 with its ReLU,
    the head (Dropout, fc2, loss, tally and their backward down to fc1's pre-activation), fc1's weight gradient and grad-input, the
    backward of Dropout2d + Flatten + ReLU, the conv backwards and Adam -- captured once as a single-stream, strictly linear HIP
    graph, so a step is one replay.  The training set, the epoch's permutation, the activations and the tally (sum of loss * rows,
    correct rows, rows) live on the device; nothing is read back inside an epoch.  One graph for the full batch, one for the tail
    N % batch_size (a tail of one row is valid: there is no BatchNorm).  Gradients are overwritten every step: no zero_grad.
    graph=False: the same entries called eagerly with by-value draws (what the replays must equal).  The walk over the epoch, the
    capture and the tally readers are _graphed.BatchWalkFit's."""

    CHANNELS = [1, 32, 64, 128]
    HW_IN, FEAT, HIDDEN, MAX_K, MAX_ROWS = 28, 128 * 7 * 7, 256, 16, 128

    @staticmethod
    def unsupported(classifier, batch_size):
        """None, or why this net / batch cannot take the fused path."""
        convs = [m for m in getattr(classifier, "conv", []) if isinstance(m, nn.Conv2d)]
        fcs = [m for m in getattr(classifier, "fc", []) if isinstance(m, nn.Linear)]
        want = [(1, 32, 1), (32, 64, 2), (64, 128, 2)]
        got = [(c.in_channels, c.out_channels, c.stride[0]) for c in convs]
        if got != want or any(c.kernel_size != (3, 3) or c.padding != (1, 1) or c.bias is None for c in convs):
            return f"convolutions {got} are not the reference's 3x3 {want} on 28x28"
        if len(fcs) != 2 or (fcs[0].in_features, fcs[0].out_features, fcs[1].in_features) != (ClassifierFit.FEAT, ClassifierFit.HIDDEN,
                                                                                             ClassifierFit.HIDDEN):
            return f"linear layers {[(f.in_features, f.out_features) for f in fcs]} are not 6272 -> 256 -> K"
        if fcs[1].out_features > ClassifierFit.MAX_K:
            return f"{fcs[1].out_features} classes are above the {ClassifierFit.MAX_K} one MFMA tile holds"
        if batch_size > ClassifierFit.MAX_ROWS:
            return f"batch size {batch_size} is above the {ClassifierFit.MAX_ROWS} rows one workgroup holds"
        prec = getattr(classifier, "conv_precision", "fp32")
        if prec != "fp32":
            return f"conv_precision {prec!r}: the fused fit is fp32 only"
        return None

    def __init__(self, classifier, x_train, y_train, batch_size, lr=Config.cls_lr, rng=None, graph=True):
        why = self.unsupported(classifier, batch_size)
        if why is not None:
            raise PcgError(f"ClassifierFit: {why}")
        dev = next(classifier.parameters()).device
        if dev.type != "cuda":
            raise PcgError(f"ClassifierFit: the classifier is on {dev}; libpcgan_hip has no CPU path")
        self.classifier = classifier
        X = torch.as_tensor(x_train).to(dev, torch.float32)
        super().__init__(X.shape[0], batch_size)
        D = self.HW_IN * self.HW_IN
        if self.N < 1 or self.B < 1 or X.numel() != self.N * D:
            raise PcgError(f"ClassifierFit: need x [N, 1, {self.HW_IN}, {self.HW_IN}] and y [N]")
        self.X = X.reshape(self.N, D).contiguous()
        self.Y = torch.as_tensor(y_train).to(dev, torch.int64).contiguous()
        if self.Y.shape != (self.N,):
            raise PcgError(f"ClassifierFit: need x [N, 1, {self.HW_IN}, {self.HW_IN}] and y [N]")
        self.rng = rng if rng is not None else ops.DeviceRNG(seed=0)
        classifier.train()
        classifier._ensure_flat()
        classifier.zero_grad()                                # attaches the .grad views; every step OVERWRITES them (no zero_grad)
        self.optimizer = Adam(classifier.parameters(), lr=lr)
        self._convs = [m for m in classifier.conv if isinstance(m, nn.Conv2d)]
        self._fc1, self._fc2 = classifier.fc[1], classifier.fc[4]
        self._p2d, self._p1 = classifier.conv[6].p, classifier.fc[3].p
        self.K = self._fc2.out_features
        self._start(classifier, dev, graph)

    def _buffers(self, R):
        dev = self.X.device
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)      # noqa: E731
        C = self.CHANNELS
        geoms, hw = [], self.HW_IN
        for conv in self._convs:
            geoms.append(_geom(conv, R, hw, hw))
            hw = geoms[-1].OH
        return {"x": f32(R, self.HW_IN * self.HW_IN), "y": torch.zeros((R,), dtype=torch.int64, device=dev), "m": [f32(R, C[3]), f32(R, self.HIDDEN)],
                "g": geoms, "a": [f32(R, g.OH, g.OW, g.Cout) for g in geoms], "flat": f32(R, self.FEAT), "h": f32(R, self.HIDDEN),
                "logits": f32(R, self.K), "loss": f32(1), "dh": f32(R, self.HIDDEN), "dflat": f32(R, self.FEAT),
                "d3": f32(R, geoms[2].OH, geoms[2].OW, C[3])}

    def _span(self, R):
        return ops.DeviceRNG.mnist_clf_batch_span(R, [self.CHANNELS[3], self.HIDDEN])

    def _launches(self, b, cursor=None):
        """One step, Adam included, over the buffer set b; cursor None: offsets and rows from the device counter (the captured form)."""
        self.rng.mnist_clf_batch(self.X, self.Y, self.perm, (b["x"], b["y"]), b["m"], [1.0 - self._p2d, 1.0 - self._p1],
                                 counter=self._ctr if cursor is None else None, cursor=cursor or 0)
        self._forward_backward(b)
        self.optimizer.step()

    def _forward_backward(self, b):
        from .nn import _lin_mfma
        fc1, fc2, convs, geoms = self._fc1, self._fc2, self._convs, b["g"]
        R = b["x"].shape[0]
        a = b["x"].view(R, self.HW_IN, self.HW_IN, 1)
        for conv, g, out in zip(convs, geoms, b["a"]):
            a = ops.conv2d_fwd(g, a, ops.ohwi(conv.weight.data), conv.bias.data, act=ACT_RELU, out=out)
        HW, C = geoms[2].OH * geoms[2].OW, geoms[2].Cout
        ops.drop2d_flatten_fwd(b["a"][2], b["m"][0], self._p2d, R, HW, C, out=b["flat"])
        # fc1 with its ReLU in the launch, on the route nn.linear_fwd takes for these sizes (a 1x1 convolution on the matrix cores from
        # 11 rows up); pcg_dense_rows_fwd would give each of its 16 workgroups all of W1's 6.4 MB panel rows to stream alone
        mfma = _lin_mfma(R, self.FEAT, self.HIDDEN)
        g1 = ops.conv_geom(R, 1, 1, self.FEAT, self.HIDDEN, 1, 1, 1, 0)
        if mfma:
            ops.conv2d_fwd(g1, b["flat"], fc1.weight.data, fc1.bias.data, act=ACT_RELU, out=b["h"])
        else:
            ops.gemm(b["flat"], fc1.weight.data, R, self.HIDDEN, self.FEAT, transB=True, bias=fc1.bias.data, out=b["h"], act=ACT_RELU)
        ops.mnist_clf_head(b["h"], b["m"][1], self._p1, fc2.weight.data, fc2.bias.data, b["y"], self.tally, logits=b["logits"], loss=b["loss"],
                           dW2=fc2.weight.grad, db2=fc2.bias.grad, dh=b["dh"], db1=fc1.bias.grad)
        if mfma:
            ops.conv2d_wgrad(g1, b["flat"], b["dh"], fc1.weight.grad, False)
            ops.conv2d_dgrad(g1, b["dh"], fc1.weight.data, out=b["dflat"])
        else:
            ops.linear_wgrad(b["dh"], b["flat"], R, self.HIDDEN, self.FEAT, fc1.weight.grad)
            ops.gemm(b["dh"], fc1.weight.data, R, self.FEAT, self.HIDDEN, out=b["dflat"])
        d = ops.drop2d_flatten_bwd(b["dflat"], b["m"][0], self._p2d, b["a"][2], R, HW, C, act=ACT_RELU, out=b["d3"])
        for i in (2, 1, 0):
            conv, g = convs[i], geoms[i]
            below = b["a"][i - 1] if i > 0 else b["x"]
            ops.conv2d_wgrad(g, below, d, ops.ohwi(conv.weight.grad), False)
            ops.colsum(d.numel() // conv.out_channels, conv.out_channels, d, conv.bias.grad, False)
            if i > 0:
                d = _dgrad_act(g, d, ops.ohwi(conv.weight.data), below, ACT_RELU, 0.0)


VAL_CHUNK = 4096   # rows per eval-mode forward of train_classifier(fused=True)'s validation


def train_classifier(classifier, train_loader, valid_loader, cfg, device, save=True, fused=False):
    """trainer.py:8-39 — Adam(cls_lr), CrossEntropyLoss, per-epoch validation accuracy, best state saved to
    cfg.classifier_path.  fused=True (train_loader a data.DeviceLoader, the reference's net, batch <= 128): the batches run through
    ClassifierFit -- one graph replay per step, in the order and with the Dropout masks the chain sees for the same loader seed and
    classifier.rng -- the validation is eval-mode forwards of at most VAL_CHUNK rows, each tallied on the device, and the epoch makes
    ONE host read.  Anything else warns once and runs the op chain."""
    from .data import DeviceLoader
    fit = None
    if fused:
        why = None
        if not isinstance(train_loader, DeviceLoader):
            why = "train_loader is not a data.DeviceLoader (the fit needs the training set resident on the device)"
        elif not train_loader.shuffle:
            why = "the training loader does not shuffle"
        else:
            why = ClassifierFit.unsupported(classifier, train_loader.batch_size)
        if why is None:
            if classifier.rng is None:
                classifier.rng = ops.DeviceRNG(seed=0)                                        # the stream CNNClassifier.forward draws from
            fit = ClassifierFit(classifier, train_loader.x, train_loader.y, train_loader.batch_size, lr=cfg.cls_lr, rng=classifier.rng)
            ones = torch.ones(fit.K, dtype=torch.float32, device=fit.X.device)
            xv, yv = (valid_loader.x, valid_loader.y) if isinstance(valid_loader, DeviceLoader) else \
                (torch.cat(t) for t in zip(*((x, y) for x, y in valid_loader)))               # setup: the validation set, resident
            xv, yv = xv.to(device, torch.float32).contiguous(), yv.to(device, torch.int64).contiguous()
        else:
            _warn_fused_fallback(why)
    optimizer = fit.optimizer if fit is not None else Adam(classifier.parameters(), lr=cfg.cls_lr)
    criterion = CrossEntropyLoss()
    best_acc, history = 0.0, []
    for epoch in range(cfg.num_epochs_clf):
        classifier.train()
        for x, y in (train_loader if fit is None else ()):
            x, y = x.to(device), y.to(device)
            optimizer.zero_grad()
            loss = criterion(classifier(x), y)
            loss.backward()
            optimizer.step()
        if fit is not None:
            fit.epoch(train_loader.epoch_order())                                             # the order train_loader would walk
        classifier.eval()
        correct, total = 0.0, 0
        with torch.no_grad():
            if fit is not None:
                classifier._packed = None        # the in-place optimizer kernel bumps no tensor version: _pack would serve the old image
                for i in range(0, xv.shape[0], VAL_CHUNK):
                    ops.ce_weighted_tally(classifier(xv[i:i + VAL_CHUNK]).contiguous(), yv[i:i + VAL_CHUNK], ones, fit.val_tally,
                                          seg=VAL_CHUNK)
                correct, total = fit.read_tallies()[4:6]                                      # the epoch's one host read
            for x, y in (valid_loader if fit is None else ()):
                x, y = x.to(device), y.to(device)
                acc_b = ops.cf_metrics(classifier(x).contiguous(), y, other=y)[0].item()     # mean(argmax == y)
                correct += acc_b * y.size(0)
                total += y.size(0)
        acc = correct / max(total, 1)
        history.append(acc)
        print(f"[Classifier] Epoch {epoch + 1}/{cfg.num_epochs_clf} | Val Acc: {acc:.4f}")
        if acc > best_acc:
            best_acc = acc
            if save and getattr(cfg, "classifier_path", None):
                torch.save({k: v.detach().cpu().contiguous() for k, v in classifier.state_dict().items()}, cfg.classifier_path)
    return history


def grad_norm(net):
    """trainer.py:41-42 — sqrt(sum ||p.grad||^2) over a net's parameters (per-epoch diagnostic, :142-143): one launch over
    the flat gradient buffer (its alignment padding is zero), one host read."""
    out = torch.empty(1, dtype=torch.float32, device=net.flat_grads.device)
    ops.sumsq(net.flat_grads, out)
    return float(out.item()) ** 0.5


def make_optimizers(generator, discriminator, cfg=Config):
    """trainer.py:77-80."""
    opt_g = Adam(generator.parameters(), lr=cfg.g_lr)
    opt_d = Adam(discriminator.parameters(), lr=cfg.d_lr)
    return opt_g, opt_d, BCEWithLogitsLoss(), CrossEntropyLoss()


def train_step(generator, discriminator, classifier, opt_g, opt_d, bce, ce, x, y, target_y, mask, cfg=Config, dp=None,
               skip_dead_d_wgrad=True):
    """One iteration of train_countergan's loop body (trainer.py:89-123) for a batch already on the GPU; `target_y`
    (:94) and `mask` (:95) are passed in.  Returns device tensors; the reference's `.item()` calls are the caller's.

    dp (parallel.GradSync): D's bucket is averaged in stream order (Adam(D) needs it at once); G's bucket + Adam(G) run on the
    side stream and overlap with the NEXT iteration's D(real) forward — which is therefore issued before the generator forward
    when data-parallel (it reads only x, y and D's weights; D has no BatchNorm, so the hoist changes no number)."""
    d_real_logits = None
    if dp is not None:
        d_real_logits = discriminator(x, y)                                            # :103, hoisted above the wait
        dp.wait(generator)                                                             # previous iteration's G all-reduce + Adam(G)
    raw_residual, masked_residual = generator(x, target_y, mask)                       # :96
    x_cf = clamp_add(x, masked_residual, -1.0, 1.0)                                    # :97
    mask_penalty_pre = abs_mean(raw_residual, mask, one_minus=True)                    # :99
    # Discriminator update
    opt_d.zero_grad()                                                                  # :102
    if d_real_logits is None:
        d_real_logits = discriminator(x, y)                                            # :103
    d_fake_logits = discriminator(x_cf.detach(), target_y)                             # :104
    d_loss = weighted_sum([bce(d_real_logits, 1.0), bce(d_fake_logits, 0.0)], [1.0, 1.0])   # :106-107 (one launch each way, no ATen add)
    d_loss.backward()                                                                  # :111
    if dp is not None:
        dp.sync_now(discriminator)
    opt_d.step()                                                                       # :112
    # Generator update
    opt_g.zero_grad()                                                                  # :115
    if skip_dead_d_wgrad:
        for p in discriminator.parameters():
            p.requires_grad_(False)
    try:
        g_fake_logits = discriminator(x_cf, target_y)                                  # :116
        g_adv = bce(g_fake_logits, 1.0)                                                # :117
        g_cls = ce(classifier(x_cf), target_y)                                         # :118
        reg_l1 = abs_mean(masked_residual)                                             # :119
        g_loss = weighted_sum([g_adv, g_cls, reg_l1, mask_penalty_pre],
                              [cfg.lambda_adv, cfg.lambda_cls, cfg.lambda_reg, cfg.lambda_mask])   # :121 (was seven ATen mul / add launches)
        g_loss.backward()                                                              # :122
    finally:
        if skip_dead_d_wgrad:
            for p in discriminator.parameters():
                p.requires_grad_(True)
    if dp is not None:
        dp.sync_then(generator, opt_g.step)                                            # overlapped with the next D(real) forward
    else:
        opt_g.step()                                                                   # :123
    return {"d_loss": d_loss, "g_loss": g_loss, "g_adv": g_adv, "g_cls": g_cls, "reg_l1": reg_l1, "mask_pen": mask_penalty_pre,
            "d_real_logits": d_real_logits, "d_fake_logits": d_fake_logits, "x_cf": x_cf}


def _lookahead(it):
    """(item, is_last) over any iterable — the loader is `any iterable of (x, y)`, it need not have a length."""
    it = iter(it)
    try:
        prev = next(it)
    except StopIteration:
        return
    for cur in it:
        yield prev, False
        prev = cur
    yield prev, True


def train_countergan(generator, discriminator, classifier, train_loader, cfg, device, log_every=100, device_rng=None, draws=None,
                     save=True, verbose=True):
    """conditional_counteRGAN/mnist/trainer.py:76-163 `train_countergan(generator, discriminator, classifier, train_loader, cfg,
    device)`: the same loop, the same per-epoch means (:139-141), the per-epoch `G_grad` / `D_grad` line (:142-147 — the one place
    grad_norm :41-42 is used), `residual_mean` in the batch log line (:137) and the generator checkpoint (:162); the loss-curve PNG
    (:149-160) is plotting and is left out.

    D's .grad at the epoch summary = the D step's gradients + the generator step's critic weight gradients (no zeroing between :111
    and :122): the LAST iteration of an epoch runs with skip_dead_d_wgrad=False, every other one skips that dead work.
    Host reads: the reference calls .item() five times per iteration; here the per-iteration scalars stay on the device and are
    read once per epoch (and at the log lines), summed in the same order.
    device_rng: an ops.DeviceRNG — draw targets and masks on the GPU instead of torch's RNG;
    draws(epoch, batch_idx, x) -> (target_y, mask): supplied draws (parity runs).  Returns the per-epoch history:
    {"g_losses", "d_losses", "g_cls_losses", "G_grad", "D_grad"}."""
    opt_g, opt_d, bce, ce = make_optimizers(generator, discriminator, cfg)                     # :77-80
    hist = {k: [] for k in ("g_losses", "d_losses", "g_cls_losses", "G_grad", "D_grad")}
    for epoch in range(cfg.num_epochs_gan):                                                    # :84
        pending = []
        for batch_idx, ((x, y), last) in enumerate(_lookahead(train_loader)):                  # :89
            x, y = x.to(device), y.to(device)                                                  # :90
            bs = x.size(0)
            if draws is not None:
                target_y, mask = (t.to(device) for t in draws(epoch, batch_idx, x))
            elif device_rng is not None:
                target_y = device_rng.randint(0, cfg.num_classes, bs, x.device)                # :94
                mask = build_mask_device(device_rng, x, cfg.patch_size, cfg.num_modifiable_patches)   # :95
            else:
                target_y = torch.randint(0, cfg.num_classes, (bs,), device=device)             # :94
                mask = build_mask(x, cfg.patch_size, device, cfg.num_modifiable_patches)       # :95
            out = train_step(generator, discriminator, classifier, opt_g, opt_d, bce, ce, x, y, target_y, mask, cfg,
                             skip_dead_d_wgrad=not last)                                        # :96-123
            # :130-132, read at the epoch's end.  Detached: a scalar with its grad_fn would keep every custom node's saved
            # activations (ctx.saved is a plain attribute, not released by backward) alive until the epoch ends — 0.67 GB per
            # iteration at the reference batch
            pending.append((out["g_loss"].detach(), out["d_loss"].detach(), out["g_cls"].detach()))
            if verbose and batch_idx % log_every == 0:                                         # :134-137
                reg = out["reg_l1"].item()
                print(f"[Epoch {epoch + 1}/{cfg.num_epochs_gan}] batch {batch_idx} :: "
                      f"D(real)={torch.sigmoid(out['d_real_logits']).mean().item():.3f}, "
                      f"D(fake)={torch.sigmoid(out['d_fake_logits']).mean().item():.3f}, g_adv={out['g_adv'].item():.4f}, "
                      f"g_cls={out['g_cls'].item():.4f}, reg={reg:.6f}, residual_mean={reg:.4f}")   # masked_residual.abs().mean() IS reg_l1 (:119)
        n = len(pending)
        if n == 0:
            raise PcgError("train_countergan: the loader yielded no batch")
        g_epoch = d_epoch = cls_epoch = 0.0                                                    # same order of additions as :130-132
        for g_l, d_l, c_l in pending:
            g_epoch += g_l.item(); d_epoch += d_l.item(); cls_epoch += c_l.item()
        hist["g_losses"].append(g_epoch / n); hist["d_losses"].append(d_epoch / n); hist["g_cls_losses"].append(cls_epoch / n)   # :139-141
        hist["G_grad"].append(grad_norm(generator)); hist["D_grad"].append(grad_norm(discriminator))                           # :142-143
        if verbose:
            print(f"[GAN] Epoch {epoch + 1}/{cfg.num_epochs_gan} | G: {hist['g_losses'][-1]:.4f}, D: {hist['d_losses'][-1]:.4f}, "
                  f"G_cls: {hist['g_cls_losses'][-1]:.4f}, G_grad: {hist['G_grad'][-1]:.4f}, D_grad: {hist['D_grad'][-1]:.4f}")   # :145-147
    if save and getattr(cfg, "generator_path", None):
        import os
        os.makedirs(os.path.dirname(os.path.abspath(cfg.generator_path)) or ".", exist_ok=True)
        torch.save({k: v.detach().cpu().contiguous() for k, v in generator.state_dict().items()}, cfg.generator_path)         # :162
        if verbose:
            print(f"Generator saved to {cfg.generator_path}")
    return hist


# ---- the promptable half: patch prompts, queries and per-target evaluation (eval_utils.py, gradio_app.py:234-259) ----
SUM_FIELDS = ("flips", "flip_max", "gain_cf", "gain_orig", "abs_change", "abs_allowed", "abs_forbidden", "count")   # pcg_mnist_cf_score's group sums
PER_CLASS_FIELDS = ("class_flip_rate", "prediction_gain", "actionability")
MASKED_METRIC_KEYS = ("Class_flip_rate_mean", "Class_flip_rate_max", "Residual_L1_norm_in_allowed_patches", "Prediction_gain",
                      "Actionability (overall L1 norm)", "mask_penalty_pre")


def patch_bits(patches, total):
    """One 64-bit word (as a signed Python int, the value an int64 tensor holds) with bit p set for every patch p of `patches` inside
    [0, total); an index outside is ignored, as create_mask_from_indices does (eval_utils.py:251-252)."""
    if not 1 <= total <= 64:
        raise PcgError(f"patch_bits: {total} patches do not fit a 64-bit word")
    word = 0
    for p in patches:
        p = int(p)
        if 0 <= p < total:
            word |= 1 << p
    return word - (1 << 64) if word >= 1 << 63 else word


def _patch_grid(H, W, patch_size):
    patch_size = int(patch_size)
    if patch_size < 1 or H // patch_size < 1 or W // patch_size < 1:
        raise PcgError(f"patch size {patch_size} gives no patch on a {H} x {W} image")
    return H // patch_size, W // patch_size


def _masks_from_lists(lists, H, W, patch_size, device):
    """[len(lists), 1, H, W] masks on the GPU from lists of patch indices: the host packs bits, the device expands them
    (pcg_patch_mask_bits).  More than 64 patches do not fit a word: those masks are built on the host and uploaded."""
    device = torch.device(device)
    if device.type != "cuda":
        raise PcgError(f"patch masks are built on the GPU, got device {device}; libpcgan_hip has no CPU path")
    nph, npw = _patch_grid(H, W, patch_size)
    total = nph * npw
    if total <= 64:
        bits = torch.tensor([patch_bits(c, total) for c in lists], dtype=torch.int64).to(device)
        return ops.patch_mask_bits(bits, H, W, patch_size)
    import numpy as np
    m = np.zeros((len(lists), 1, H, W), np.float32)
    for r, chosen in enumerate(lists):
        for idx in chosen:
            if 0 <= idx < total:
                i, j = divmod(int(idx), npw)
                m[r, 0, i * patch_size:(i + 1) * patch_size, j * patch_size:(j + 1) * patch_size] = 1.0
    return torch.from_numpy(m).to(device)


def choose_patches(bs, total_patches, shared_per_batch=False, modifiable_patches=None, randomize_per_sample=True, min_patches=5,
                   max_patches=None):
    """The patch selection of build_patch_mask_for_batch (eval_utils.py:239-282) on the host, with the same np.random calls in the
    same order: one list for a shared mask, else one per sample.  Pure host."""
    import numpy as np
    if max_patches is None:
        max_patches = total_patches // 2                                                       # :240-241
    min_patches = max(1, int(min_patches))
    max_patches = min(total_patches, int(max_patches))
    if min_patches > max_patches:
        min_patches = max_patches
    use_random = (modifiable_patches is None) or randomize_per_sample                          # :260

    def draw():
        if not use_random:
            return list(modifiable_patches)                                                    # :269, :281
        k = np.random.randint(min_patches, max_patches + 1)                                    # :265, :277
        return np.random.choice(range(total_patches), size=k, replace=False).tolist()          # :266, :278
    return [draw() for _ in range(1 if shared_per_batch else bs)]


def build_patch_mask_for_batch(x, patch_size=5, device=None, shared_per_batch=False, modifiable_patches=None, return_single_mask=True,
                               randomize_per_sample=True, min_patches=5, max_patches=None):
    """eval_utils.py:204-288, the reference's signature and draws (choose_patches); the masks are expanded on the GPU.  Returns
    (batch_mask [B,C,H,W], single_mask [1,C,H,W]) or batch_mask; a shared mask and C > 1 are broadcast views, not copies."""
    device = x.device if device is None else device
    bs, C, H, W = x.shape
    nph, npw = _patch_grid(H, W, patch_size)
    chosen = choose_patches(bs, nph * npw, shared_per_batch, modifiable_patches, randomize_per_sample, min_patches, max_patches)
    masks = _masks_from_lists(chosen, H, W, patch_size, device)
    batch_mask = masks.expand(bs, C, H, W)
    single_mask = masks[0:1].expand(1, C, H, W)
    return (batch_mask, single_mask) if return_single_mask else batch_mask


def make_mask_from_patch_list(x_batch, patch_size, allowed_patches, device=None):
    """gradio_app.py:234-240: the single mask [1,C,H,W] of a user's patch list."""
    return build_patch_mask_for_batch(x_batch, patch_size=patch_size, device=device, shared_per_batch=True, modifiable_patches=allowed_patches,
                                      return_single_mask=True, randomize_per_sample=False)[1]


def _padded_logits(classifier, rows, out=None):
    """The frozen classifier's logits [n, kp] (kp = num_classes padded to a multiple of 4) of image rows [n, 784]: CNNClassifier's
    eval forward with the padded columns kept (the score kernel reads rows of kp floats) and an optional destination.  A classifier
    with a `padded_logits(rows, out)` method of its own (Classifier) supplies them itself."""
    if hasattr(classifier, "padded_logits"):
        return classifier.padded_logits(rows, out=out)
    with ops.conv_precision(classifier.conv_precision):
        cw, w1, b1, w2, b2, kp = classifier._pack()
        n = rows.shape[0]
        a = rows.view(n, 28, 28, 1)
        for conv, w, b in cw:
            a = ops.conv2d_fwd(_geom(conv, n, a.shape[1], a.shape[2]), a, w, b, act=ACT_RELU)
        feat = a.numel() // n
        h = ops.conv2d_fwd(ops.conv_geom(n, 1, 1, feat, w1.shape[0], 1, 1, 1, 0), a.view(n, 1, 1, feat), w1, b1, act=ACT_RELU)
        logits = ops.conv2d_fwd(ops.conv_geom(n, 1, 1, w1.shape[0], kp, 1, 1, 1, 0), h, w2, b2, out=out)
    return logits.view(n, kp)


def _prompt_mask(x, T, patches, mask, patch_size):
    """(mask tensor, mask_mode, the mask in the shape the caller gets back) from a patch prompt or a dense mask."""
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    HW = H * W
    if patches is not None and mask is not None:
        raise PcgError("give the prompt as `patches` or as `mask`, not both")
    if patches is not None:
        patches = list(patches)
        per_row = len(patches) > 0 and isinstance(patches[0], (list, tuple))
        if per_row and len(patches) != B:
            raise PcgError(f"patches: {len(patches)} lists for {B} rows")
        m = _masks_from_lists(patches if per_row else [patches], H, W, patch_size, x.device)
        return m, ("row" if per_row else "shared"), m
    if mask is None:                                       # no prompt: every pixel may change (eval_utils.py:55)
        m = torch.empty((1, 1, H, W), dtype=torch.float32, device=x.device)
        ops.fill(m, 1.0)
        return m, "shared", m
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise PcgError(f"mask: expected a tensor on the GPU, got {getattr(mask, 'device', type(mask))}")
    modes = {}                                             # the smaller reading wins where two sizes coincide (B == 1 or T == 1)
    for n, v in ((T * B * HW, ("query", (T, B, 1, H, W))), (B * HW, ("row", (B, 1, H, W))), (HW, ("shared", (1, 1, H, W)))):
        modes[n] = v
    if mask.numel() not in modes or mask.shape[-1] != W:
        raise PcgError(f"mask: expected {HW} (shared), {B * HW} (per row) or {T * B * HW} (per query) values of [.., {H}, {W}], got {tuple(mask.shape)}")
    mode, shape = modes[mask.numel()]
    m = mask.contiguous()
    return m, mode, m.view(shape)


def _run_queries(generator, classifier, x, targets, T, m, mode, y_true=None, group_rows=None, query_chunk=2048, keep=True, with_orig=True,
                 fold_eval_bn=True, outputs=ops.SCORE_FIELDS):
    """All T * B queries of a batch: generator + classifier over windows of `query_chunk` queries, then ONE score launch."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise PcgError(f"x is on {getattr(x, 'device', type(x))}; libpcgan_hip has no CPU path")
    if int(query_chunk) < 1:
        raise PcgError(f"query_chunk {query_chunk}")
    B = x.shape[0]
    xr = _as_rows(x, B)
    HW, K, TB, dev = xr.shape[1], classifier.num_classes, T * B, x.device
    kp = (K + 3) // 4 * 4
    f32 = dict(dtype=torch.float32, device=dev)
    logits, sums = torch.empty((TB, kp), **f32), torch.empty((TB, 3), **f32)
    full = {k: torch.empty((TB, HW), **f32) for k in ("x_cf", "raw", "masked")} if keep else None
    for q0 in range(0, TB, int(query_chunk)):
        nq = min(int(query_chunk), TB - q0)
        out = {"sums": sums[q0:q0 + nq]}
        if keep:
            out.update({k: v[q0:q0 + nq] for k, v in full.items()})
        r = generator.forward_queries(xr, targets, m, mode, T=T, q0=q0, nq=nq, fold_eval_bn=fold_eval_bn, want_residuals=keep, out=out)
        _padded_logits(classifier, r["x_cf"], out=logits[q0:q0 + nq])
    logits_orig = _padded_logits(classifier, xr) if (with_orig and y_true is not None) else None
    res = ops.mnist_cf_score(logits, K, B, T, target=targets, y_true=y_true, logits_orig=logits_orig, tail_sums=sums, group_rows=group_rows,
                             outputs=outputs)
    res.update(sums=sums, logits=logits)
    if keep:
        res.update(full)
    return res


def _labels(v, B, device, name):
    if v is None:
        return None
    t = torch.full((B,), int(v), dtype=torch.int64) if not torch.is_tensor(v) else v.reshape(-1).to(torch.int64)
    if t.numel() != B:
        raise PcgError(f"{name}: expected {B} labels, got {t.numel()}")
    return t.to(device).contiguous()


def counterfactuals(generator, classifier, x, target, patches=None, mask=None, patch_size=Config.patch_size, query_chunk=2048, y_true=None):
    """The prompted query (gradio_app.py:242-259 run_transformation / eval_utils.py:498-530 without the plot): "turn these images
    into `target` (an int or one class per row), touching only `patches`" — a list of patch indices for every row, one list per row,
    or a dense `mask`; neither: every pixel may change.  Both nets must be in eval mode.  Returns device tensors: x_cf, raw_residual,
    masked_residual [B,1,H,W], mask (as used), pred (int64), conf, p_target, p_true / p_orig_true (with y_true) [B], and sums [B,3]:
    sum |x_cf - x|, sum |raw * mask|, sum |raw * (1 - mask)| over the pixels."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise PcgError(f"x: expected a [B,1,H,W] tensor on the GPU, got {getattr(x, 'device', type(x))}")
    B, _, H, W = x.shape
    m, mode, m_out = _prompt_mask(x, 1, patches, mask, patch_size)
    res = _run_queries(generator, classifier, x, _labels(target, B, x.device, "target"), 1, m, mode, y_true=_labels(y_true, B, x.device, "y_true"),
                       query_chunk=query_chunk)
    shp = (B, 1, H, W)
    out = {"x_cf": res["x_cf"].view(shp), "raw_residual": res["raw"].view(shp), "masked_residual": res["masked"].view(shp), "mask": m_out,
           "sums": res["sums"], "group_sums": res["group_sums"]}
    out.update({k: res[k] for k in ops.SCORE_FIELDS})
    return out


def counterfactual_sweep(generator, classifier, x, y_true=None, patches=None, mask=None, patch_size=Config.patch_size, query_chunk=2048,
                         group_rows=None):
    """counterfactuals() for ALL num_classes targets of every row in one pass: results shaped [T,B,...] (x_cf, raw_residual,
    masked_residual [T,B,1,H,W]; pred ... flip [T,B]; sums [T,B,3]) and group_sums [T, ceil(B / group_rows), 8] (SUM_FIELDS)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise PcgError(f"x: expected a [B,1,H,W] tensor on the GPU, got {getattr(x, 'device', type(x))}")
    B, _, H, W = x.shape
    T = generator.embed.num_embeddings
    m, mode, m_out = _prompt_mask(x, T, patches, mask, patch_size)
    res = _run_queries(generator, classifier, x, None, T, m, mode, y_true=_labels(y_true, B, x.device, "y_true"), group_rows=group_rows,
                       query_chunk=query_chunk)
    shp = (T, B, 1, H, W)
    out = {"x_cf": res["x_cf"].view(shp), "raw_residual": res["raw"].view(shp), "masked_residual": res["masked"].view(shp), "mask": m_out,
           "sums": res["sums"].view(T, B, 3), "group_sums": res["group_sums"]}
    out.update({k: res[k].view(T, B) for k in ops.SCORE_FIELDS})
    return out


def metrics_from_sums(sums, hw):
    """Pure host.  Group sums [..., 8] (SUM_FIELDS) -> the per-group means in float64: class_flip_rate, class_flip_max, prediction_gain
    (eval_utils.py:63-64, both probabilities from the counterfactual's softmax), prediction_gain_orig (:314-316), actionability,
    allowed_l1, mask_penalty_pre (per pixel) and count.  An empty group gives nan."""
    import numpy as np
    s = np.asarray(sums, np.float64)
    if s.shape[-1] != len(SUM_FIELDS):
        raise PcgError(f"metrics_from_sums: expected [..., {len(SUM_FIELDS)}] sums, got {s.shape}")
    n = s[..., 7]
    with np.errstate(invalid="ignore", divide="ignore"):
        rows, pix = np.where(n > 0, n, np.nan), np.where(n > 0, n, np.nan) * float(hw)
        return {"class_flip_rate": s[..., 0] / rows, "class_flip_max": np.where(n > 0, s[..., 1], np.nan), "prediction_gain": s[..., 2] / rows,
                "prediction_gain_orig": s[..., 3] / rows, "actionability": s[..., 4] / pix, "allowed_l1": s[..., 5] / pix,
                "mask_penalty_pre": s[..., 6] / pix, "count": n}


def fold_groups(group_sums, hw):
    """Pure host.  [T][J][8] group sums (J loader batches) -> per target the mean over the batches of the per-batch means, the order
    of eval_utils.py:97-102 (a ragged last batch weighs as much as a full one), in float64.  Empty groups are left out."""
    import numpy as np
    per = metrics_from_sums(group_sums, hw)
    if per["count"].ndim != 2:
        raise PcgError(f"fold_groups: expected [T][J][8] sums, got {np.asarray(group_sums).shape}")
    live = per["count"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        return {k: np.where(live, v, 0.0).sum(axis=1) / live.sum(axis=1) for k, v in per.items() if k != "count"}


def compute_masked_metrics(raw_residual, masked_residual, x, x_cf, mask, classifier, y_true, y_target, device=None):
    """eval_utils.py:292-344, the reference's signature and six keys.  The sums over the allowed and the forbidden pixels come from
    the tail kernel on `raw_residual`, the flip rate and the prediction gain (p_cf[target] - p_orig[y_true], :314-316) from the score
    kernel; two host reads."""
    B = x.shape[0]
    xr, rr = _as_rows(x, B), _as_rows(raw_residual, B)
    HW = xr.shape[1]
    mr = mask if mask.numel() == HW else _as_rows(mask, B)
    _, _, _, sums = ops.mnist_cf_tail(rr, xr, mr.contiguous(), "shared" if mask.numel() == HW else "row", 1.0, want_residuals=False)
    xc = _as_rows(x_cf, B)
    res = ops.mnist_cf_score(_padded_logits(classifier, xc), classifier.num_classes, B, 1, target=_labels(y_target, B, x.device, "y_target"),
                             y_true=_labels(y_true, B, x.device, "y_true"), logits_orig=_padded_logits(classifier, xr), tail_sums=sums, outputs=())
    m = metrics_from_sums(res["group_sums"].cpu().numpy()[0, 0], HW)
    actionability = abs_mean(ops.axpby(1.0, xc, -1.0, xr)).item()                                                   # :335, of the x_cf given
    return dict(zip(MASKED_METRIC_KEYS, (float(m["class_flip_rate"]), float(m["class_flip_max"]), float(m["allowed_l1"]),
                                         float(m["prediction_gain_orig"]), actionability, float(m["mask_penalty_pre"]))))


def per_class_csv(avg_results, fields=PER_CLASS_FIELDS):
    """The text of DataFrame.from_dict(avg_results, orient="index").to_csv() (eval_utils.py:104-107): an empty first header cell, one
    row per target class, floats in their shortest repr."""
    lines = ["," + ",".join(fields)]
    for cls in avg_results:
        lines.append(f"{cls}," + ",".join(repr(float(avg_results[cls][f])) for f in fields))
    return "\n".join(lines) + "\n"


def evaluate_generator_per_target(generator, classifier, test_loader, config, one_pass=True, query_chunk=2048, fold_eval_bn=True, verbose=True):
    """eval_utils.py:78-110: class flip rate, prediction gain and actionability per target class, the mean over the loader's batches of
    the per-batch means; countergan_metrics_per_class.csv under config.save_dir.  one_pass: all num_classes targets of a loader batch
    in ONE generator pass (chunked by query_chunk) with the all-ones mask shared, the sums read once at the end; one_pass=False: one
    evaluate_counterfactuals call per (batch, target), the reference's own loop.  Host arithmetic in float64.  Returns
    {target class: {metric: value}}."""
    import numpy as np
    device, T = torch.device(config.device), config.num_classes
    generator.eval(); classifier.eval()                                                                             # :81-82
    if one_pass:
        ones, groups = None, []
        with torch.no_grad():
            for x, y in test_loader:                                                                                    # :87
                x, y = x.to(device), y.to(device)
                B = x.shape[0]
                if ones is None:
                    ones = torch.empty(x[0].numel(), dtype=torch.float32, device=device)
                    ops.fill(ones, 1.0)
                res = _run_queries(generator, classifier, x, None, T, ones, "shared", y_true=_labels(y, B, device, "y"), group_rows=B,
                                   query_chunk=query_chunk, keep=False, with_orig=False, fold_eval_bn=fold_eval_bn, outputs=())
                groups.append(res["group_sums"])
        if not groups:
            raise PcgError("evaluate_generator_per_target: the loader yielded no batch")
        sums = np.stack([g.cpu().numpy()[:, 0, :] for g in groups], axis=1)                                             # [T][J][8]
        folded = fold_groups(sums, ones.numel())
        avg_results = {cls: {k: float(folded[k][cls]) for k in PER_CLASS_FIELDS} for cls in range(T)}
    else:
        results = {cls: {k: [] for k in PER_CLASS_FIELDS} for cls in range(T)}
        for x, y in test_loader:
            x, y = x.to(device), y.to(device)
            for cls in range(T):                                                                                        # :91-95
                metrics, _ = evaluate_counterfactuals(generator, classifier, x, y, torch.full_like(y, cls), device)
                for k in PER_CLASS_FIELDS:
                    results[cls][k].append(metrics[k])
        avg_results = {cls: {k: float(np.mean(np.asarray(v, np.float64))) for k, v in m.items()} for cls, m in results.items()}   # :98-102
    if getattr(config, "save_dir", None):
        os.makedirs(config.save_dir, exist_ok=True)
        csv_path = os.path.join(config.save_dir, "countergan_metrics_per_class.csv")
        with open(csv_path, "w") as f:
            f.write(per_class_csv(avg_results))
        if verbose:
            print(f"Saved per-class CounterGAN metrics to {csv_path}")
    if verbose:
        print(per_class_csv(avg_results), end="")
    return avg_results


def evaluate_classifier(classifier, dataloader, device, save_dir=None, prefix="classifier", verbose=True):
    """eval_utils.py:15-43 without the heat map: accuracy and confusion matrix [true][pred] over the loader; the predictions are the
    score kernel's first maxima, read once at the end.  With save_dir the matrix goes to <prefix>_confusion_matrix.csv."""
    import numpy as np
    classifier.eval()
    K = classifier.num_classes
    preds, labels = [], []
    with torch.no_grad():
        for x, y in dataloader:
            x = x.to(device)
            B = x.shape[0]
            preds.append(ops.mnist_cf_score(_padded_logits(classifier, _as_rows(x, B)), K, B, 1, target=None, outputs=("pred",), group_sums=False)["pred"])
            labels.append(y)
    if not preds:
        raise PcgError("evaluate_classifier: the loader yielded no batch")
    all_preds = np.concatenate([p.cpu().numpy() for p in preds])
    all_labels = np.concatenate([np.asarray(t.cpu().numpy(), np.int64).reshape(-1) for t in labels])
    acc = float((all_preds == all_labels).mean())
    cm = np.zeros((K, K), np.int64)
    np.add.at(cm, (all_labels, all_preds), 1)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, f"{prefix}_confusion_matrix.csv"), "w") as f:
            f.write(confusion_csv(cm))
    if verbose:
        print(f"{prefix} Test Accuracy: {acc:.4f}")
    return acc, cm


# ---- the report figures' numbers and pixels (eval_utils.py:113-201, gr.py:346-441, :498-568; csrc/cf_report.hip) ------
def _dataset_chunks(dataset, chunk, device):
    """(N, H, W, resident, chunks, fetch) of a data set given as a pair of tensors (X [N,1,H,W] / [N,H,W], Y [N]), on the host or the
    device, or as anything with __len__ / __getitem__ that yields (x, y).  chunks(stop, with_x) yields (row0, rows [n, H*W] fp32 on
    the GPU or None, labels [n] int64 on the GPU) over the rows below `stop`; fetch(rows) returns those rows [len(rows), H*W] on the
    GPU; resident: X as [N, H*W] rows where the whole data set already lies on the GPU, else None."""
    chunk = int(chunk)
    if chunk < 1:
        raise PcgError(f"chunk {chunk}: a chunk holds at least one row")
    if isinstance(dataset, (tuple, list)) and len(dataset) == 2 and all(torch.is_tensor(t) for t in dataset):
        X, Y = dataset
        N = X.shape[0]
        if N < 1 or X.dim() < 3 or Y.numel() != N or Y.dtype.is_floating_point:
            raise PcgError(f"dataset: expected (X [N,1,H,W], Y [N] integers) with N >= 1, got {tuple(X.shape)} and {tuple(Y.shape)} {Y.dtype}")
        H, W = X.shape[-2], X.shape[-1]
        if X.numel() != N * H * W:
            raise PcgError(f"dataset: one-channel images expected, got {tuple(X.shape)}")
        Xr, Yr = _as_rows(X, N), Y.reshape(-1).to(torch.int64)

        def chunks(stop, with_x=True):
            for r0 in range(0, stop, chunk):
                r1 = min(stop, r0 + chunk)
                yield r0, (Xr[r0:r1].to(device).contiguous() if with_x else None), Yr[r0:r1].to(device).contiguous()

        def fetch(rows):
            return Xr[torch.as_tensor(rows, dtype=torch.int64)].to(device).contiguous()      # (host rows: a host gather)
        return N, H, W, (Xr if Xr.is_cuda else None), chunks, fetch
    if not (hasattr(dataset, "__len__") and hasattr(dataset, "__getitem__")):
        raise PcgError(f"dataset: expected a pair of tensors (X, Y) or a map-style data set, got {type(dataset).__name__}")
    N = len(dataset)
    if N < 1:
        raise PcgError("dataset: no rows")
    x0 = torch.as_tensor(dataset[0][0])
    H, W = x0.shape[-2], x0.shape[-1]

    def fetch(rows):
        return torch.stack([torch.as_tensor(dataset[int(i)][0], dtype=torch.float32).reshape(H * W) for i in rows]).to(device).contiguous()

    def chunks(stop, with_x=True):
        for r0 in range(0, stop, chunk):
            items = [dataset[i] for i in range(r0, min(stop, r0 + chunk))]
            xs = torch.stack([torch.as_tensor(x, dtype=torch.float32).reshape(H * W) for x, _ in items]) if with_x else None
            ys = torch.as_tensor([int(y) for _, y in items], dtype=torch.int64)
            yield r0, (xs.to(device).contiguous() if with_x else None), ys.to(device)
    return N, H, W, None, chunks, fetch


def _pick_words(state, K, what):
    """One host read of a pick's K keys -> the picked row per class; a class without a row raises."""
    words = state.cpu().numpy().view("uint64")
    absent = [k for k in range(K) if words[k] == 0]
    if absent:
        raise PcgError(f"{what}: the data set has no row of class(es) {absent}")
    return [int(0xFFFFFFFF - (int(w) & 0xFFFFFFFF)) for w in words]


def pick_sources(classifier, dataset, pick_best_source=False, chunk=2048, full_scan=False):
    """The source pick of visualize_counterfactual_grid (eval_utils.py:135-149): one row per class, the first one of the data set or,
    with pick_best_source, the one whose own label the classifier is most confident about (ties: the lowest row, the strict `>` of
    :143).  The data set is walked in chunks of `chunk` rows, each folded into ONE device state (ops.class_pick): "best" runs the
    classifier's padded logits per chunk, "first" does no classifier work at all.
    The reference's `break` (:148-149) stands after the if / else, so its "best" scan too ends at the row that completes the set of
    classes: the most confident row is chosen among the rows up to there.  That is the default here: a "first" pass over the labels
    finds where the scan ends (one host read of K keys), the "best" pass covers those rows only (a second read at the end).
    full_scan=True scans the whole data set instead — what the reference's docstring promises — with one host read at the end.
    dataset: see _dataset_chunks.  Returns (sources [K,1,H,W], rows [K] int64, conf [K] fp32 — 0 in "first" mode), all on the GPU.
    A class without a row raises (the reference fails on None.to)."""
    K = classifier.num_classes
    device = next(classifier.parameters()).device
    if device.type != "cuda":
        raise PcgError(f"pick_sources: the classifier is on {device}; libpcgan_hip has no CPU path")
    mode = "best" if pick_best_source else "first"
    classifier.eval()                                                                                               # :125
    N, H, W, resident, chunks, fetch = _dataset_chunks(dataset, chunk, device)
    if N > ops.PICK_MAX_ROW:
        raise PcgError(f"pick_sources: {N} rows do not fit the 32-bit row of a key")
    with torch.no_grad():
        stop = N
        if pick_best_source and not full_scan:
            first = ops.class_pick_state(K, device)
            for r0, _, y in chunks(N, with_x=False):
                ops.class_pick(first, y, K, row0=r0, mode="first")
            stop = max(_pick_words(first, K, "pick_sources")) + 1                                                   # :148-149
        state = ops.class_pick_state(K, device)
        for r0, xr, y in chunks(stop, with_x=pick_best_source):
            ops.class_pick(state, y, K, row0=r0, logits=_padded_logits(classifier, xr) if pick_best_source else None, mode=mode)
        rows, conf, sources = ops.class_pick_gather(state, K, mode, X=resident)
    picked = _pick_words(state, K, "pick_sources")
    if sources is None:
        sources = fetch(picked)
    return sources.view(K, 1, H, W), rows, conf


def _grid_report(sources, rows, conf, sweep):
    """The grid of a sweep over the K sources: the [source][target] views of the sweep's [target][row] results, the reference's own
    annotation on the diagonal (eval_utils.py:176-178: pred = the class, conf = 1.0) and the two images (ops.cf_panels, grid mode)."""
    import numpy as np
    K, _, H, W = sources.shape
    x_cf = sweep["x_cf"]
    T = x_cf.shape[0]
    image, image_u8 = ops.cf_panels(sources.view(K, H * W), x_cf.view(T, K, H * W), H, W, mode="grid")
    pred = sweep["pred"].cpu().numpy().T.copy()                                                                     # [source][target]
    cf = sweep["conf"].cpu().numpy().T.copy()
    hit = pred == np.arange(T)[None, :]                                                                              # :193
    d = np.arange(min(K, T))
    pred[d, d], cf[d, d], hit[d, d] = d, 1.0, True                                                                   # :176-178
    return {"sources": sources, "source_rows": rows, "source_conf": conf, "x_cf": x_cf.transpose(0, 1), "pred": pred, "conf": cf, "hit": hit,
            "image": image, "image_u8": image_u8}


def counterfactual_grid(generator, classifier, dataset, pick_best_source=False, patches=None, mask=None, chunk=2048, full_scan=False):
    """visualize_counterfactual_grid (eval_utils.py:113-201) without the figure: pick_sources, ONE counterfactual_sweep over the K
    sources (K x K queries; the default prompt is the all-ones mask of :183) and the grid image.  Returns sources [K,1,H,W],
    source_rows, source_conf [K]; x_cf [K,K,1,H,W] (a view, [source][target]); pred, conf, hit [K,K] (host arrays, [source][target],
    the diagonal as the reference annotates it: pred = r, conf = 1.0, hit); image [K*H, K*W] fp32 in [0, 1] with the sources on the
    diagonal, and image_u8."""
    generator.eval()                                                                                                # :124
    sources, rows, conf = pick_sources(classifier, dataset, pick_best_source, chunk, full_scan)
    with torch.no_grad():
        sweep = counterfactual_sweep(generator, classifier, sources, patches=patches, mask=mask)
    return _grid_report(sources, rows, conf, sweep)


def grid_csv(grid):
    """The text of cf_grid.csv: one line per cell, columns source, target, pred, conf, hit."""
    K, T = grid["pred"].shape
    lines = ["source,target,pred,conf,hit"]
    lines += [f"{r},{c},{int(grid['pred'][r, c])},{float(grid['conf'][r, c])!r},{int(grid['hit'][r, c])}" for r in range(K) for c in range(T)]
    return "\n".join(lines) + "\n"


def heatmap_batch(x, x_cf, mask, classifier=None, max_samples=16):
    """The data half of make_and_save_heatmaps (gr.py:346-441): for the first max_samples rows the four panels original,
    counterfactual, |difference| and mask, [n,4,H,W] in [0, 1] (:370-372), and vmax [1], the batch maximum of the difference (:399),
    both on the GPU.  x, x_cf [B,1,H,W] in [-1, 1]; mask [1,1,H,W] (shared) or [B,1,H,W].  With a classifier also pred (int64) and
    conf [n] of the counterfactuals."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise PcgError(f"x: expected a [B,1,H,W] tensor on the GPU, got {getattr(x, 'device', type(x))}")
    B, _, H, W = x.shape
    n = min(int(max_samples), B)
    if n < 1 or tuple(x_cf.shape) != tuple(x.shape):
        raise PcgError(f"heatmap_batch: max_samples {max_samples}, x {tuple(x.shape)}, x_cf {tuple(x_cf.shape)}")
    HW = H * W
    xr, cr = _as_rows(x, B)[:n], _as_rows(x_cf, B)[:n]
    m = mask.reshape(-1, HW) if torch.is_tensor(mask) else None
    if m is None or m.shape[0] not in (1, B):
        raise PcgError(f"mask: expected [1,1,{H},{W}] or [{B},1,{H},{W}] on the GPU, got {getattr(mask, 'shape', type(mask))}")
    m = (m if m.shape[0] == 1 else m[:n]).contiguous()
    panels, vmax = ops.cf_panels(xr, cr, H, W, mask=m, mode="panels")
    out = {"panels": panels, "vmax": vmax}
    if classifier is not None:
        with torch.no_grad():
            res = ops.mnist_cf_score(_padded_logits(classifier, cr), classifier.num_classes, n, 1, target=None, outputs=("pred", "conf"),
                                     group_sums=False)
        out.update(pred=res["pred"], conf=res["conf"])
    return out


def user_modification_example(x, patches, generator, classifier, target, patch_size=Config.patch_size):
    """save_user_modification_example (gr.py:498-568) without the figure: the first row of x, "turn it into `target`, touching only
    `patches`" (counterfactuals(..., patches=patches), :498-530), then its four panels.  Returns panels [1,4,H,W], vmax [1], pred,
    conf [1], mask [1,1,H,W] and x_cf [1,1,H,W], on the GPU."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise PcgError(f"x: expected a [B,1,H,W] tensor on the GPU, got {getattr(x, 'device', type(x))}")
    x1 = x[0:1].contiguous()
    with torch.no_grad():
        res = counterfactuals(generator, classifier, x1, int(target), patches=list(patches), patch_size=patch_size)
    out = heatmap_batch(x1, res["x_cf"], res["mask"], max_samples=1)
    out.update(pred=res["pred"], conf=res["conf"], mask=res["mask"], x_cf=res["x_cf"])
    return out


def evaluate_pipeline(generator, classifier, full_dataset, test_loader, config, verbose=True, grid=False):
    """eval_utils.py:572-647, the live lines (:577-610, :643): a patch prompt per sample of the first test batch, targets that differ
    from the labels, the counterfactuals, evaluate_counterfactuals on that batch (countergan_metrics.csv) and the per-target table.
    grid=True: also the counterfactual grid of :626-629 over `full_dataset` (counterfactual_grid, pick_best_source=False as there):
    cf_grid.npy (the float image), cf_grid.png (8-bit grayscale) and cf_grid.csv (source, target, pred, conf, hit) under
    config.save_dir; rendering the annotated figure stays out.  Returns (metrics, per-target table)."""
    device = torch.device(config.device)
    x, y = next(iter(test_loader))                                                                                  # :577
    x, y = x.to(device), y.to(device)
    batch_mask, single_mask = build_patch_mask_for_batch(                                                           # :585-595
        x, patch_size=config.patch_size, device=device, shared_per_batch=False, modifiable_patches=None, return_single_mask=True,
        randomize_per_sample=(config.user_input_patches is None), min_patches=config.min_modifiable_patches,
        max_patches=config.max_modifiable_patches)
    y_target = torch.randint(0, config.num_classes, y.shape, device=device)                                         # :598
    y_target[y_target == y] = (y_target[y_target == y] + 1) % config.num_classes                                    # :599
    generate_counterfactuals(generator, classifier, x, y, y_target, batch_mask.contiguous(), device)                # :602-604
    metrics_without_mask = evaluate_counterfactuals(generator, classifier, x, y, y_target, device)[0]               # :609
    table = evaluate_generator_per_target(generator, classifier, test_loader, config, verbose=verbose)              # :610
    os.makedirs(config.save_dir, exist_ok=True)
    path = os.path.join(config.save_dir, "countergan_metrics.csv")
    with open(path, "w") as f:
        f.write(per_class_csv({0: metrics_without_mask}))                                                           # :643
    if verbose:
        print(f"Countergan metrics: {metrics_without_mask}\nSaved to: {path}")
    if grid:                                                                                                        # :626-629
        import numpy as np
        g = counterfactual_grid(generator, classifier, full_dataset)
        np.save(os.path.join(config.save_dir, "cf_grid.npy"), g["image"].cpu().numpy())
        write_png_gray(os.path.join(config.save_dir, "cf_grid.png"), g["image_u8"].cpu().numpy())
        with open(os.path.join(config.save_dir, "cf_grid.csv"), "w") as f:
            f.write(grid_csv(g))
        if verbose:
            print(f"Saved CF grid: {os.path.join(config.save_dir, 'cf_grid.png')}")
    return metrics_without_mask, table
