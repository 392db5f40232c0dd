"""Host-side mirror of `simple_gan/mnist/mnist_gan.py` on the whole-batch dense kernels (csrc/dense_rows.hip):
the MLP GAN on flattened 28x28 MNIST, Generator 100→128→256→512→1024→784 with BatchNorm1d(·, 0.8) on three layers, Discriminator
784→512→256→1, batch 64, BCELoss, two Adam(2e-4, (0.5, 0.999)).

    args :22-32 -> config;  Generator :41-63, Discriminator :65-83 (same state_dict keys);  loop body :116-134 -> train_step;
    epochs loop :113-139 -> train.  Image grids, the GIF and the loss plot (:140-157) stay out of scope.

Every Linear (+ BatchNorm1d) (+ activation) is ONE launch forward (`ops.dense_rows_fwd`), every layer's backward is two: the
grad-input GEMM whose epilogue is the activation derivative and BatchNorm backward of the layer below (`ops.dense_rows_dgrad`), and
the weight + bias gradient (`ops.dense_rows_wgrad`).  `use_fused = False` on a net runs the same layers as a chain of the older ops
(linear_fwd / linear_dgrad / linear_wgrad, bn_train_stats / bn_apply_act / bn_act_bwd, act_fwd / act_bwd): the in-project baseline.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import sheets
from ._lib import ACT_LRELU, ACT_NONE, ACT_SIGMOID, ACT_TANH, PcgError
from .nn import FlatModule, GraphedStep, linear_dgrad, linear_fwd, linear_wgrad
from .optim import Adam

config = {"epochs": 200, "batch_size": 64, "learning_rate": 0.0002, "b1": 0.5, "b2": 0.999, "latent_dim": 100, "img_size": 28,
          "channels": 1}                                                                                                    # :22-31
MAX_FUSED_BATCH = 64      # D's backward runs on the stacked [real | fake] rows: 2 * batch <= 128, the kernels' row limit


def img_shape(cfg=config):
    return (cfg["channels"], cfg["img_size"], cfg["img_size"])                                                             # :34


class _Layer:
    def __init__(self, lin, bn, act, slope):
        self.lin, self.bn, self.act, self.slope = lin, bn, act, slope


class _DenseNet(FlatModule):
    """An nn.Sequential of Linear / BatchNorm1d / LeakyReLU / Tanh / Sigmoid under `self.model`, run layer by layer on the GPU."""
    use_fused = True

    def _layers(self):
        if "_compiled" not in self.__dict__:
            out, mods, i = [], list(self.model), 0
            while i < len(mods):
                lin = mods[i]
                if not isinstance(lin, nn.Linear):
                    raise PcgError(f"expected nn.Linear at model.{i}, found {type(lin).__name__}")
                i += 1
                bn, act, slope = None, ACT_NONE, 0.0
                if i < len(mods) and isinstance(mods[i], nn.BatchNorm1d):
                    bn = mods[i]
                    i += 1
                if i < len(mods) and isinstance(mods[i], (nn.LeakyReLU, nn.Tanh, nn.Sigmoid)):
                    m = mods[i]
                    act = ACT_LRELU if isinstance(m, nn.LeakyReLU) else ACT_TANH if isinstance(m, nn.Tanh) else ACT_SIGMOID
                    slope = float(getattr(m, "negative_slope", 0.0))
                    i += 1
                out.append(_Layer(lin, bn, act, slope))
            self.__dict__["_compiled"] = out
        return self.__dict__["_compiled"]

    def _dense_bn(self, bn, training, save=None):
        mean, invstd, xhat = save if save is not None else (None, None, None)
        return ops.DenseBN(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps,
                           bn.momentum if bn.momentum is not None else 0.1, training, mean, invstd, xhat)

    def _layer_fwd(self, L, x, training, out=None, keep=None):
        """One layer forward; keep: dict that receives what the backward reads ('xhat' fused / 'z' chain, 'mean', 'invstd')."""
        lin, bn = L.lin, L.bn
        if self.use_fused:
            d = None
            if bn is not None:
                d = self._dense_bn(bn, training, (keep.get("mean"), keep.get("invstd"), keep.get("xhat")) if keep is not None else None)
            y = ops.dense_rows_fwd(x, lin.weight.data, lin.bias.data if lin.bias is not None else None, L.act, L.slope, d, out=out)
            if keep is not None and d is not None and training:
                keep.update(mean=d.save_mean, invstd=d.save_invstd, xhat=d.xhat)
            return y
        C = lin.out_features
        if bn is None:
            if L.act in (ACT_NONE, ACT_LRELU) and out is None:
                return linear_fwd(lin, x, act=L.act, slope=L.slope)
            return ops.act_fwd(linear_fwd(lin, x), L.act, L.slope, out=out)
        z = linear_fwd(lin, x)
        if training:
            mean, invstd = ops.bn_train_stats(z, C, bn.eps, bn.momentum if bn.momentum is not None else 0.1, bn.running_mean, bn.running_var,
                                              bn.num_batches_tracked)
            if keep is not None:
                keep.update(mean=mean, invstd=invstd, z=z)
            return ops.bn_apply_act(z, C, mean, invstd, bn.weight.data, bn.bias.data, L.act, L.slope, out=out)
        return ops.bn_apply_act(z, C, bn.running_mean, bn.running_var, bn.weight.data, bn.bias.data, L.act, L.slope, var_eps=bn.eps, out=out)

    def _layer_dgrad(self, L, dz, below, y_below, keep_below, out=None):
        """Gradient w.r.t. the pre-activation (pre-BatchNorm) output of layer `below` (None: plain dx), given dz of layer L."""
        w = L.lin.weight.data
        act, slope = (below.act, below.slope) if below is not None else (ACT_NONE, 0.0)
        bnb = below.bn if below is not None else None
        if self.use_fused:
            bn = None
            if bnb is not None:
                gg, _ = self._grad_view(bnb.weight)
                gb, _ = self._grad_view(bnb.bias)
                bn = (keep_below["xhat"], bnb.weight.data, keep_below["invstd"], gg, gb, False)
            return ops.dense_rows_dgrad(dz, w, act, slope, y_below if act != ACT_NONE else None, bn, out=out)
        dx = linear_dgrad(w, dz, dz.shape[0])
        if bnb is not None:
            gg, _ = self._grad_view(bnb.weight)
            gb, _ = self._grad_view(bnb.bias)
            return ops.bn_act_bwd(dx, keep_below["z"], y_below, bnb.num_features, keep_below["mean"], keep_below["invstd"], bnb.weight.data, act,
                                  slope, gg, gb, False, out=out)
        if act != ACT_NONE:
            return ops.act_bwd(dx, y_below, act, slope, out=out)
        return dx

    def _layer_wgrad(self, L, dz, x):
        if self.use_fused:
            gw, _ = self._grad_view(L.lin.weight)
            gb = self._grad_view(L.lin.bias)[0] if L.lin.bias is not None else None
            ops.dense_rows_wgrad(dz, x, gw, gb, accumulate=False)
        else:
            linear_wgrad(self, L.lin, x, dz)

    def _run(self, x, training, out=None, acts=None, keeps=None, rows=None):
        """Forward through every layer.  acts / keeps: per-layer output buffers and backward records (train_step's workspace);
        rows: the row slice of stacked buffers this pass writes."""
        layers = self._layers()
        for i, L in enumerate(layers):
            last = i == len(layers) - 1
            o = out if last else (acts[i][rows] if acts is not None and rows is not None else acts[i] if acts is not None else None)
            if not self.use_fused and acts is not None and not last:
                o = None                              # the op chain allocates its own outputs (the MFMA linear has no `out`)
            y = self._layer_fwd(L, x, training, out=o, keep=keeps[i] if keeps is not None else None)
            if not self.use_fused and acts is not None and not last:
                acts[i] = y
            x = y
        return x

    def _check_input(self, x, features):
        if not x.is_cuda:
            raise PcgError(f"input is on {x.device}; libpcgan_hip has no CPU path — move the module and its input to the GPU")
        x = x.reshape(x.shape[0], -1)
        if x.shape[1] != features:
            raise PcgError(f"expected {features} features per row, got {x.shape[1]}")
        self._ensure_flat()
        return x.contiguous().float()

    @torch.no_grad()
    def _forward(self, x, features):
        x = self._check_input(x, features)
        return self._run(x, self.training)


class Generator(_DenseNet):
    """mnist_gan.py:41-63.  forward() runs the kernels without recording autograd (training mode updates the BatchNorm buffers
    like torch does); gradients are train_step's job."""

    def __init__(self, cfg=config):
        super().__init__()
        self.cfg = dict(cfg)

        def layer_block(input_size, output_size, normalize=True):                                                          # :45-50
            layers = [nn.Linear(input_size, output_size)]
            if normalize:
                layers.append(nn.BatchNorm1d(output_size, 0.8))     # 0.8 lands in the eps slot, as in the reference (:48)
            layers.append(nn.LeakyReLU(0.2, inplace=True))
            return layers

        self.model = nn.Sequential(                                                                                         # :52-59
            *layer_block(cfg["latent_dim"], 128, normalize=False),
            *layer_block(128, 256),
            *layer_block(256, 512),
            *layer_block(512, 1024),
            nn.Linear(1024, int(np.prod(img_shape(cfg)))),
            nn.Tanh())

    def forward(self, z):
        img = self._forward(z, self.cfg["latent_dim"])
        return img.view(img.size(0), *img_shape(self.cfg))                                                                  # :64


class Discriminator(_DenseNet):
    """mnist_gan.py:65-83."""

    def __init__(self, cfg=config):
        super().__init__()
        self.cfg = dict(cfg)
        self.model = nn.Sequential(                                                                                         # :70-77
            nn.Linear(int(np.prod(img_shape(cfg))), 512), nn.LeakyReLU(0.2, inplace=True),
            nn.Linear(512, 256), nn.LeakyReLU(0.2, inplace=True),
            nn.Linear(256, 1), nn.Sigmoid())

    def forward(self, img):
        return self._forward(img, int(np.prod(img_shape(self.cfg))))                                                        # :80-82


def make_optimizers(generator, discriminator, cfg=config):
    kw = dict(lr=cfg["learning_rate"], betas=(cfg["b1"], cfg["b2"]))
    return Adam(generator.parameters(), **kw), Adam(discriminator.parameters(), **kw)                                       # :108-109


class _Workspace:
    """The step's activation and gradient buffers for one batch size: static addresses, so a captured step can be replayed."""

    def __init__(self, G, D, R, dev):
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        gl, dl = G._layers(), D._layers()
        self.R = R
        self.g_acts = [e(R, L.lin.out_features) for L in gl[:-1]]
        self.g_keep = [dict(mean=e(L.lin.out_features), invstd=e(L.lin.out_features), xhat=e(R, L.lin.out_features)) if L.bn is not None else {}
                       for L in gl]
        self.g_dz = [e(R, L.lin.out_features) for L in gl]
        self.X = e(2 * R, dl[0].lin.in_features)              # rows [0, R): the real batch, [R, 2R): the generated batch
        self.d_acts = [e(2 * R, L.lin.out_features) for L in dl]
        self.d_dz = [e(2 * R, L.lin.out_features) for L in dl]
        self.d_dp = e(2 * R, 1)
        self.half = torch.full((1,), 0.5, dtype=torch.float32, device=dev)


def _workspace(G, D, R, dev):
    cache = G.__dict__.setdefault("_step_ws", {})
    key = (R, str(dev), id(D))
    if key not in cache:
        cache[key] = _Workspace(G, D, R, dev)
    return cache[key]


def train_step(generator, discriminator, opt_g, opt_d, real, z, record=None):
    """One batch of mnist_gan.py:116-134, in the reference's statement order: the generator is updated first, against the
    not-yet-updated discriminator; the discriminator step then reuses the same generated batch, detached, and takes the mean of
    its two losses.  Returns (generator_loss, discriminator_loss), one-element device tensors.

    Two pieces of the reference's work are not done because their results are not used (both nets `use_fused`):
      * D's forward on the generated batch in the D step (:131) — D has not changed since :124, so it is bit-identical to the one
        the G step did; its activations are kept in the lower half of the stacked [real | fake] buffers;
      * D's weight gradients in the G step's backward (:125) — `optimizer_discriminator.zero_grad()` (:129) discards them.
    The op chain (`use_fused = False`) takes the second skip only: it reruns D on the stacked [real | fake] rows.

    record: a dict that receives copies of the hidden activations of the three passes (`g_acts`: the generator's LeakyReLU outputs;
    `d_acts_g_step`: D's on the generated batch inside the G step; `d_acts_d_step`: D's on the stacked [real | fake] rows of the D
    step) — which side of each LeakyReLU kink this run took; diagnostics and tests only, it adds copies to the step."""
    G, D = generator, discriminator
    if not real.is_cuda or not z.is_cuda:
        raise PcgError("train_step: real and z must be on the GPU; libpcgan_hip has no CPU path")
    R = real.shape[0]
    if 2 * R > 128 or R < 2:
        raise PcgError(f"train_step: batch of {R} rows; the whole-batch kernels take 2 <= batch <= {MAX_FUSED_BATCH} "
                       "(the discriminator's backward runs on the stacked real and generated rows)")
    if G.use_fused != D.use_fused:
        raise PcgError("train_step: generator.use_fused and discriminator.use_fused must agree")
    G._ensure_flat(); D._ensure_flat()
    dev = real.device
    real = real.reshape(R, -1)
    ws = _workspace(G, D, R, dev)
    gl, dl = G._layers(), D._layers()
    fused = G.use_fused
    lo, hi = slice(0, R), slice(R, 2 * R)
    fake = ws.X[hi]

    # ---- Training Generator (:120-126) ----
    G.drop_grads()                                                                           # optimizer_generator.zero_grad() :121
    g_acts, g_keep = list(ws.g_acts), ws.g_keep
    G._run(z, True, out=fake, acts=g_acts, keeps=g_keep)                                     # generated_images = generator(z) :123
    d_acts = list(ws.d_acts)
    if fused:
        D._run(fake, True, out=ws.d_acts[-1][hi], acts=d_acts, rows=hi)                      # discriminator(generated_images) :124
        f_acts = [a[hi] for a in ws.d_acts]
    else:
        f_acts = [None] * len(dl)
        f_acts[-1] = D._run(fake, True, acts=f_acts)
    g_loss, dp = ops.bce_fwd_bwd(f_acts[-1].view(-1), None, 1.0)                             # adversarial_loss(·, real_output) :124
    dzl = ops.act_bwd(dp.view(R, 1), f_acts[-1], ACT_SIGMOID)                                # generator_loss.backward() :125
    for i in range(len(dl) - 1, 0, -1):                                                      # through D: data gradients only
        dzl = D._layer_dgrad(dl[i], dzl, dl[i - 1], f_acts[i - 1], None)
    dzl = D._layer_dgrad(dl[0], dzl, gl[-1], fake, None, out=ws.g_dz[-1])                    # d/d(pre-Tanh) of the generator's last layer
    for i in range(len(gl) - 1, -1, -1):
        x_in = g_acts[i - 1] if i > 0 else z
        G._layer_wgrad(gl[i], dzl, x_in)
        if i > 0:
            dzl = G._layer_dgrad(gl[i], dzl, gl[i - 1], g_acts[i - 1], g_keep[i - 1], out=ws.g_dz[i - 1])
    if record is not None:
        record["g_acts"] = [t.clone() for t in g_acts]
        record["d_acts_g_step"] = [t.clone() for t in f_acts[:-1]]
    opt_g.step()                                                                             # :126

    # ---- Training Discriminator (:128-134) ----
    D.drop_grads()                                                                           # optimizer_discriminator.zero_grad() :129
    ws.X[lo].copy_(real)
    if fused:
        D._run(ws.X[lo], True, out=ws.d_acts[-1][lo], acts=d_acts, rows=lo)                  # discriminator(real_images) :130; (:131) kept
        s_acts = ws.d_acts
    else:
        s_acts = [None] * len(dl)
        s_acts[-1] = D._run(ws.X, True, acts=s_acts)                                         # real and generated rows in one pass
    loss3, dp = ops.bce_pair(s_acts[-1].view(-1), R, 1.0, 0.0, need_grad=True, cotangents=(None, None, ws.half))   # :130-132
    d_loss = ops.axpby(0.5, loss3[2:3])
    dzl = ops.act_bwd(dp.view(2 * R, 1), s_acts[-1], ACT_SIGMOID)                            # discriminator_loss.backward() :133
    for i in range(len(dl) - 1, -1, -1):
        x_in = s_acts[i - 1] if i > 0 else ws.X
        D._layer_wgrad(dl[i], dzl, x_in)
        if i > 0:
            dzl = D._layer_dgrad(dl[i], dzl, dl[i - 1], s_acts[i - 1], None, out=ws.d_dz[i - 1] if fused else None)
    if record is not None:
        record["d_acts_d_step"] = [t.clone() for t in s_acts[:-1]]
    opt_d.step()                                                                             # :134
    return g_loss, d_loss


def train(generator, discriminator, loader, cfg=config, opt_g=None, opt_d=None, epochs=None, seed=0, draws=None, graphed=False,
          image_dir=None):
    """The epochs loop (:111-139) over a `data.DeviceLoader` (reshuffled every epoch, last short batch kept, like the reference's
    DataLoader).  z is drawn on the device (pcg_randn); `draws(epoch, i, rows)` overrides it with a host array or tensor
    [rows, latent_dim] — the reference draws z with np.random.normal on the host (:122), parity runs pass the same numbers.
    graphed: replay the step through nn.GraphedStep, one graph per distinct batch size.  image_dir (a path): after every epoch the
    first 25 rows of the epoch's last generated batch are written to `{image_dir}/{epoch}.png` as the reference does (:140-141:
    `save_image(generated_images.data[:25], ..., nrow=5, normalize=True)`), the sheet made on the device (pcgan_amd.sheets).  Returns
    the per-epoch (generator_loss, discriminator_loss) of the epoch's last batch (:139), read back once at the end."""
    G, D = generator, discriminator
    if opt_g is None or opt_d is None:
        opt_g, opt_d = make_optimizers(G, D, cfg)
    rng = ops.DeviceRNG(seed)
    dev = next(G.parameters()).device
    if dev.type != "cuda":
        raise PcgError(f"train: the generator is on {dev}; libpcgan_hip has no CPU path")
    graphs = G.__dict__.setdefault("_step_graphs", {}).setdefault((id(D), id(opt_g), id(opt_d)), {})   # kept across calls: one capture per size
    losses = []
    for epoch in range(1, (epochs if epochs is not None else cfg["epochs"]) + 1):
        last = None
        for i, (images, _) in enumerate(loader):
            R = images.shape[0]
            if draws is not None:
                zz = draws(epoch, i, R)
                z = (torch.from_numpy(np.ascontiguousarray(zz, dtype=np.float32)) if not torch.is_tensor(zz) else zz).to(dev, torch.float32)
            else:
                z = rng.randn((R, cfg["latent_dim"]), dev)
            real = images.reshape(R, -1)
            if graphed:
                if R not in graphs:
                    sr, sz = real.clone(), z.clone()
                    graphs[R] = GraphedStep(lambda sr=sr, sz=sz: train_step(G, D, opt_g, opt_d, sr, sz), {"real": sr, "z": sz}, [G, D],
                                            [opt_g, opt_d])
                graphs[R].load(real=real, z=z)
                last = graphs[R].replay()
            else:
                last = train_step(G, D, opt_g, opt_d, real, z)
        if last is not None:
            losses.append((last[0].clone(), last[1].clone()))                                # :139
            if image_dir is not None:                                                        # :140-141; the step left the batch in X[R:]
                generated = _workspace(G, D, R, dev).X[R:2 * R][:25].view(-1, *img_shape(cfg))
                sheets.save_image(generated, os.path.join(image_dir, f"{epoch}.png"), nrow=5, normalize=True)
    return [(float(a.item()), float(b.item())) for a, b in losses]


@torch.no_grad()
def sample(generator, z):
    """Evaluation-mode images for the latent rows z (at most 128 per call): BatchNorm uses the running statistics."""
    was = generator.training
    generator.eval()
    try:
        return generator(z)
    finally:
        generator.train(was)
