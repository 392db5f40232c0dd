"""Host-side mirror of `conditional_counteRGAN/house_sales_kc_usa/` (the tabular, "prompted" CounteRGAN) on the HIP kernels.

    reference                                              here
    ---------------------------------------------------    -----------------------------------------------------
    config.py                          :13-82               CONFIG (the fields the step reads)
    models/generator.py  FiLM :6-16, ResidualBlock :19-35   FiLM, ResidualBlock (parameter containers)
    models/generator.py  ResidualGenerator :38-92           ResidualGenerator (same ctor args, same state_dict keys)
    models/discriminator.py Discriminator :5-20             Discriminator (spectral-norm keys weight_orig / weight_u / weight_v)
    models/nn_classifier.py NNClassifier :4-32              NNClassifier (frozen / eval use: forward + grad-input)
    trainer.py  cat_norm_maps :205-223                      cat_norm_maps
    trainer.py  train_countergan loop body :241-316         make_optimizers + train_step
    trainer.py  train_countergan :186-378                   train_countergan(generator, config, X_train, y_train, clf_model)
    trainer.py  train_classifier :18-180                    train_classifier(..., fused=False); fused=True: ClassifierFit, 16 whole-batch
                                                            launches as one graph replay + AdamW per step
    gradio_app.py  :144-169                                 prompt_mask + counterfactuals (this row, that class, these features)
    eval_utils.py  :185-289, :351-434, :673-728             compute_metrics_per_target(one_launch=True), analyze_class_pair_sensitivity,
                                                            evaluate_pipeline: ONE launch of pcg_house_cf_eval each
    eval_utils.py  :292-348, :436-493                       analyze_feature_shift_importance, evaluate_classifier (tables; no plots)

Every network is one autograd node that sequences C-ABI calls (csrc/tabular.hip + the BatchNorm / activation / loss kernels)
and accumulates parameter gradients straight into the FlatModule's flat gradient buffer.  The categorical heads are packed
side by side: `logits` / `samples` are [B, T] with T = sum of category counts (70 for the King-County config), head s
occupying columns seg[s]..seg[s+1]; the reference's dict views are column slices of those.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import _cfeval, ops
from . import checkpoint as _ckpt
from ._cfeval import confusion_matrix, metric_rows, save_table, upload  # noqa: F401  (public here: the host side is _cfeval's)
from ._graphed import BatchWalkFit, Held, capture_steps
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, PcgError
from .countergan import CrossEntropyLoss, abs_mean, grad_norm  # noqa: F401  (same loss kernels)
from .nn import FlatModule, FrozenClassifier, affine_fwd, in_conv_precision, linear_dgrad as _lin_dgrad, linear_fwd as _lin_fwd, linear_wgrad as _lin_wgrad, mean, weighted_sum  # noqa: F401
from .optim import Adam

FEATURES = ["bedrooms", "bathrooms", "sqft_living", "sqft_lot", "floors", "waterfront", "view", "condition", "grade",
            "sqft_above", "sqft_basement", "yr_built", "yr_renovated", "lat", "long", "sqft_living15", "sqft_lot15"]
# config.py:13-82 — category counts of the shipped dataset; `raw_values` come from the data loader (data_utils.py) at run time
CONFIG = {
    "input_dim": 17, "num_classes": 4, "hidden_dim": 32, "lr_G": 1e-3, "lr_D": 1e-3, "batch_size": 128, "epochs": 60,
    "lambda_cls": 2.0, "lambda_reg": 1.0, "lambda_mask": 1.0, "gumbel_tau": 0.5,
    "immutable_idx": [FEATURES.index(f) for f in ("lat", "long", "yr_built", "yr_renovated")],
    "categorical_info": {FEATURES.index(f): {"n": n} for f, n in
                         (("bedrooms", 9), ("bathrooms", 30), ("floors", 6), ("waterfront", 2), ("view", 5), ("condition", 5),
                          ("grade", 13))},
}
CONFIG["continuous_idx"] = [i for i in range(17) if i not in CONFIG["categorical_info"]]


def _ncat(info):
    return int(info["n"]) if isinstance(info, dict) else int(info)


# ---- generator -------------------------------------------------------------------------------------------------------
class FiLM(nn.Module):
    """generator.py:6-16 (container; the arithmetic is pcg_film_fwd/bwd)."""

    def __init__(self, hidden_dim, cond_dim):
        super().__init__()
        self.gamma = nn.Linear(cond_dim, hidden_dim)
        self.beta = nn.Linear(cond_dim, hidden_dim)


class ResidualBlock(nn.Module):
    """generator.py:19-35 (container)."""

    def __init__(self, hidden_dim, cond_dim):
        super().__init__()
        self.fc1 = nn.Linear(hidden_dim, hidden_dim)
        self.bn1 = nn.BatchNorm1d(hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, hidden_dim)
        self.bn2 = nn.BatchNorm1d(hidden_dim)
        self.film = FiLM(hidden_dim, cond_dim)


class _GFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, target_onehot, mask, noise, tau, hard, *params):
        cont, logits, samples, saved = net._run_forward(x, target_onehot, mask, noise, tau, hard)
        ctx.net, ctx.saved = net, saved
        ctx.set_materialize_grads(False)     # unused outputs (the logits, in the training step) arrive as None, not zeros
        return cont, logits, samples

    @staticmethod
    def backward(ctx, d_cont, d_logits, d_samples):
        ctx.net._run_backward(ctx.saved, d_cont, d_logits, d_samples)
        return (None,) * len(ctx.needs_input_grad)


class ResidualGenerator(FlatModule):
    """generator.py:38-92.  forward() returns what the reference returns — (cont_residual [B, n_cont], {idx: logits},
    {idx: Gumbel-softmax samples}) — the dict entries being column slices of the packed tensors `forward_packed` returns.

    Gumbel noise: `F.gumbel_softmax` draws it from torch's global generator (:90); here it is an explicit input —
    `gumbel=` (a packed [B, T] tensor or a dict idx -> [B, n]) or, when omitted, a draw from `self.rng` (ops.DeviceRNG)."""

    def __init__(self, input_dim, hidden_dim, num_classes, continuous_idx, categorical_info, n_blocks=5, residual_scaling=0.1, tau=0.5):
        super().__init__()
        self.input_dim = input_dim
        self.num_classes = num_classes
        self.continuous_idx = list(continuous_idx)
        self.categorical_info = dict(categorical_info)
        self.cond_dim = input_dim + num_classes
        self.fc_in = nn.Linear(input_dim + self.cond_dim, hidden_dim)
        self.blocks = nn.ModuleList([ResidualBlock(hidden_dim, self.cond_dim) for _ in range(n_blocks)])
        self.fc_cont = nn.Linear(hidden_dim, len(self.continuous_idx))
        self.fc_cat_logits = nn.ModuleDict({str(idx): nn.Linear(hidden_dim, _ncat(info)) for idx, info in self.categorical_info.items()})
        self.residual_scaling = residual_scaling
        self.tau = tau
        self.hidden_dim = hidden_dim
        self.cat_idx = [int(k) for k in self.fc_cat_logits.keys()]
        sizes = [self.fc_cat_logits[str(i)].out_features for i in self.cat_idx]
        self.seg = [0] + [int(v) for v in np.cumsum(sizes)]
        self.total_cat = int(self.seg[-1])
        self.rng = None
        self._idx_dev = None
        self.use_fused = True        # fused segment kernels (csrc/house_fused.hip) when the configuration allows it
        self._fdesc = None

    # -- fused path -------------------------------------------------------------------------------------------------------------
    def _eval_dims_ok(self):
        """The dimensions of _fused_ok (below) without its training clause: what the one-launch evaluation kernel is built for."""
        bn = self.blocks[0].bn1 if len(self.blocks) else None
        return (self.hidden_dim == 32 and len(self.blocks) == 5 and bn is not None
                and self.input_dim == 17 and self.num_classes == 4 and 1 <= self.total_cat <= 96 and len(self.cat_idx) <= 8
                and self.total_cat + len(self.continuous_idx) <= 96 and all(b_ - a_ <= 32 for a_, b_ in zip(self.seg, self.seg[1:]))
                and 1 <= len(self.continuous_idx) <= 32 and all(b_.bn1.eps == bn.eps and b_.bn2.eps == bn.eps for b_ in self.blocks))

    def _fused_ok(self):
        bn = self.blocks[0].bn1 if len(self.blocks) else None
        return (self.use_fused and self.hidden_dim == 32 and len(self.blocks) == 5 and self.training and bn is not None
                and self.input_dim == 17 and self.num_classes == 4 and 1 <= self.total_cat <= 96 and len(self.cat_idx) <= 8
                and self.total_cat + len(self.continuous_idx) <= 96 and all(b_ - a_ <= 32 for a_, b_ in zip(self.seg, self.seg[1:]))
                and 1 <= len(self.continuous_idx) <= 32 and all(b_.bn1.momentum == bn.momentum and b_.bn2.eps == bn.eps for b_ in self.blocks))

    def _fused_desc(self):
        """Element offsets of every parameter in the flat buffer (rebuilt when the module is re-flattened)."""
        from ._lib import HouseGDesc
        key = self._flat.data_ptr()
        if self._fdesc is not None and self._fdesc[0] == key:
            return self._fdesc[1]
        off = {id(p): o for p, o, _ in self._seg}
        d = HouseGDesc()
        d.fc_in_w, d.fc_in_b = off[id(self.fc_in.weight)], off[id(self.fc_in.bias)]
        for k, blk in enumerate(self.blocks):
            d.fc1_w[k], d.fc1_b[k] = off[id(blk.fc1.weight)], off[id(blk.fc1.bias)]
            d.bn1_g[k], d.bn1_b[k] = off[id(blk.bn1.weight)], off[id(blk.bn1.bias)]
            d.fc2_w[k], d.fc2_b[k] = off[id(blk.fc2.weight)], off[id(blk.fc2.bias)]
            d.bn2_g[k], d.bn2_b[k] = off[id(blk.bn2.weight)], off[id(blk.bn2.bias)]
            d.film_gamma_w[k], d.film_gamma_b[k] = off[id(blk.film.gamma.weight)], off[id(blk.film.gamma.bias)]
            d.film_beta_w[k], d.film_beta_b[k] = off[id(blk.film.beta.weight)], off[id(blk.film.beta.bias)]
        d.cont_w, d.cont_b = off[id(self.fc_cont.weight)], off[id(self.fc_cont.bias)]
        for s_, f in enumerate(self.cat_idx):
            head = self.fc_cat_logits[str(f)]
            d.head_w[s_], d.head_b[s_] = off[id(head.weight)], off[id(head.bias)]
        for s_, v in enumerate(self.seg):
            d.seg[s_] = v
        d.nheads, d.ncont, d.D, d.NC = len(self.cat_idx), len(self.continuous_idx), self.input_dim, self.num_classes
        d.hidden, d.nblocks = self.hidden_dim, len(self.blocks)
        self._fdesc = (key, d)
        return d

    @in_conv_precision
    def _fused_forward(self, x, target_onehot, mask, noise, tau, hard):
        from ._lib import HouseGFwdArgs
        dev = x.device
        B, T, nc = x.shape[0], self.total_cat, len(self.continuous_idx)
        x, target_onehot, mask, noise = x.contiguous(), target_onehot.contiguous(), mask.contiguous(), noise.contiguous()
        nb = (B + 63) // 64          # PCG_HOUSE_ROWS_PER_BLOCK: one 64-row wave per block
        f32 = dict(dtype=torch.float32, device=dev)
        K = 2 * self.input_dim + self.num_classes
        buf = {"inp": torch.empty((B, K), **f32), "H": torch.empty((6, B, 32), **f32), "Z1": torch.empty((5, B, 32), **f32),
               "Z2": torch.empty((5, B, 32), **f32), "P": torch.empty((10, nb, 2, 32), **f32), "SM": torch.empty((10, 2, 32), **f32),
               "cont": torch.empty((B, nc), **f32), "logits": torch.empty((B, T), **f32), "soft": torch.empty((B, T), **f32),
               "hard": torch.empty((B, T), **f32) if hard else None}
        a = HouseGFwdArgs()
        a.params = self._flat.data_ptr()
        a.x, a.onehot, a.mask, a.noise = x.data_ptr(), target_onehot.data_ptr(), mask.data_ptr(), noise.data_ptr()
        for n in ("inp", "H", "Z1", "Z2", "P", "SM", "cont", "logits", "soft"):
            setattr(a, n, buf[n].data_ptr())
        a.hard = buf["hard"].data_ptr() if hard else None
        for k, blk in enumerate(self.blocks):
            for j, bn in ((2 * k, blk.bn1), (2 * k + 1, blk.bn2)):
                a.running_mean[j], a.running_var[j] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                a.num_batches_tracked[j] = bn.num_batches_tracked.data_ptr()
        bn0 = self.blocks[0].bn1
        a.B, a.eps, a.momentum, a.tau, a.res_scale = B, bn0.eps, bn0.momentum, tau, self.residual_scaling
        ops.house_g_fwd(self._fused_desc(), a)
        saved = ("fused", buf, target_onehot, mask, tau, nb)
        return buf["cont"], buf["logits"], (buf["hard"] if hard else buf["soft"]), saved

    @in_conv_precision
    def _fused_backward(self, saved, d_cont, d_logits, d_samples):
        from ._lib import HouseGBwdArgs
        _, buf, onehot, mask, tau, nb = saved
        B, T, nc = onehot.shape[0], self.total_cat, len(self.continuous_idx)
        f32 = dict(dtype=torch.float32, device=onehot.device)
        g = {n: torch.empty((5, B, 32), **f32) for n in ("DH", "DZ1", "DZ2", "A1", "DG", "DB")}
        g.update({"DN1": torch.empty((B, 32), **f32), "DZIN": torch.empty((B, 32), **f32), "DL": torch.empty((B, T), **f32),
                  "DC": torch.empty((B, nc), **f32), "Q": torch.empty((9 * nb + (B + 15) // 16, 2, 32), **f32)})
        # BatchNorm gamma / beta gradients are written by the kernels; all of them share the accumulate state of the net
        _, acc = self._grad_view(self.blocks[0].bn1.weight)
        for blk in self.blocks:
            for p_ in (blk.bn1.weight, blk.bn1.bias, blk.bn2.weight, blk.bn2.bias):
                self._grad_view(p_)
        a = HouseGBwdArgs()
        a.params, a.grads = self._flat.data_ptr(), self._gflat.data_ptr()
        a.onehot, a.mask = onehot.data_ptr(), mask.data_ptr()
        for n in ("H", "Z1", "Z2", "SM", "soft"):
            setattr(a, n, buf[n].data_ptr())
        keep = [t.contiguous() if t is not None else None for t in (d_cont, d_logits, d_samples)]
        a.d_cont, a.d_logits, a.d_samples = (t.data_ptr() if t is not None else None for t in keep)
        for n, t in g.items():
            setattr(a, n, t.data_ptr())
        a.B, a.accumulate, a.tau, a.res_scale = B, int(acc), tau, self.residual_scaling
        ops.house_g_bwd(self._fused_desc(), a)
        # weight (+ bias) gradients of all 35 Linear layers: ONE launch (deterministic slab reduction per layer)
        inp, K = buf["inp"], buf["inp"].shape[1]
        cond = inp[:, self.input_dim:]
        h_last = buf["H"][5]
        items = []

        def add(lin, x, dy, ldx=None, ldy=None):
            gw, aw = self._grad_view(lin.weight)
            gb, ab = self._grad_view(lin.bias)
            items.append((dy, x, lin.out_features, lin.in_features, gw, gb, ldy if ldy is not None else lin.out_features,
                          ldx if ldx is not None else lin.in_features, aw, ab))
        add(self.fc_in, inp, g["DZIN"])
        for k, blk in enumerate(self.blocks):
            add(blk.fc1, buf["H"][k], g["DZ1"][k])
            add(blk.fc2, g["A1"][k], g["DZ2"][k])
            add(blk.film.gamma, cond, g["DG"][k], ldx=K)
            add(blk.film.beta, cond, g["DB"][k], ldx=K)
        add(self.fc_cont, h_last, g["DC"])
        for s_, f in enumerate(self.cat_idx):
            add(self.fc_cat_logits[str(f)], h_last, g["DL"][:, self.seg[s_]:], ldy=T)
        ops.linear_wgrad_grouped(items, B, onehot.device)
        return g

    # -- small device-side index tables (seg offsets, column indices) -------------------------------------------------
    def index_tables(self, device):
        if self._idx_dev is None or self._idx_dev[0].device != device:
            mk = lambda v: torch.tensor(list(v), dtype=torch.int32, device=device)  # noqa: E731
            self._idx_dev = (mk(self.seg), mk(self.cat_idx), mk(self.continuous_idx))
        return self._idx_dev

    def col_src(self):
        """Per feature column, where residual_full takes it from: the index of a continuous output (>= 0) or -(head + 1)."""
        src = [None] * self.input_dim
        for j, c in enumerate(self.continuous_idx):
            src[c] = j
        for s_, c in enumerate(self.cat_idx):
            src[c] = -(s_ + 1)
        if any(v is None for v in src):
            raise PcgError("ResidualGenerator: continuous_idx and categorical_info must cover every feature column")
        return src

    def pack_noise(self, gumbel):
        """dict idx -> [B, n]  ->  packed [B, T] (setup-time helper for tests / supplied draws)."""
        return torch.cat([gumbel[i] for i in self.cat_idx], dim=1).contiguous()

    def _noise(self, gumbel, B, device):
        if gumbel is None:
            if self.rng is None:
                self.rng = ops.DeviceRNG(seed=0)
            return self.rng.gumbel((B, self.total_cat), device)
        if isinstance(gumbel, dict):
            gumbel = self.pack_noise(gumbel)
        if tuple(gumbel.shape) != (B, self.total_cat):
            raise PcgError(f"gumbel noise must be [B, {self.total_cat}], got {tuple(gumbel.shape)}")
        return gumbel

    def forward_packed(self, x, target_onehot, mask=None, temperature=None, hard=False, gumbel=None):
        self._ensure_flat()
        if not x.is_cuda:
            raise PcgError(f"ResidualGenerator: input is on {x.device}; libpcgan_hip has no CPU path")
        B = x.shape[0]
        if mask is None:
            mask = torch.empty_like(x)
            ops.fill(mask, 1.0)                                                               # :70-71
        tau = self.tau if temperature is None else float(temperature)
        noise = self._noise(gumbel, B, x.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _GFn.apply(self, x, target_onehot, mask, noise, tau, bool(hard), *self.parameters())
        return self._run_forward(x, target_onehot, mask, noise, tau, bool(hard), keep=False)[:3]

    def forward(self, x, target_onehot, mask=None, temperature=None, hard=False, gumbel=None):
        cont, logits, samples = self.forward_packed(x, target_onehot, mask, temperature, hard, gumbel)
        cat_logits = {f: logits[:, self.seg[s]:self.seg[s + 1]] for s, f in enumerate(self.cat_idx)}
        cat_samples = {f: samples[:, self.seg[s]:self.seg[s + 1]] for s, f in enumerate(self.cat_idx)}
        return cont, cat_logits, cat_samples

    # -- one block ----------------------------------------------------------------------------------------------------
    def _bn(self, bn, z):
        C = bn.num_features
        if bn.training:
            mean, invstd = ops.bn_train_stats(z, C, bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked)
            return ops.bn_apply_act(z, C, mean, invstd, bn.weight.data, bn.bias.data, ACT_NONE), mean, invstd
        return ops.bn_apply_act(z, C, bn.running_mean, bn.running_var, bn.weight.data, bn.bias.data, ACT_NONE, var_eps=bn.eps), None, None

    @in_conv_precision
    def _run_forward(self, x, target_onehot, mask, noise, tau, hard, keep=True):
        if keep and self._fused_ok():
            return self._fused_forward(x, target_onehot, mask, noise, tau, hard)
        x = x.contiguous()
        seg, cat_idx, cont_idx = self.index_tables(x.device)
        B = x.shape[0]
        cond = ops.concat_cols(target_onehot.contiguous(), mask.contiguous())                # :73
        inp = ops.concat_cols(x, cond)                                                        # :74
        h = _lin_fwd(self.fc_in, inp)
        ops.act_fwd(h, ACT_RELU, 0.0, out=h)                                                  # :75
        blocks = []
        for blk in self.blocks:
            gam = _lin_fwd(blk.film.gamma, cond)                                              # FiLM :13-14 (one module, used twice)
            bet = _lin_fwd(blk.film.beta, cond)
            z1 = _lin_fwd(blk.fc1, h)                                                         # :28
            n1, m1, s1 = self._bn(blk.bn1, z1)
            a1 = ops.film_fwd(gam, n1, bet)                                                   # :29
            ops.act_fwd(a1, ACT_RELU, 0.0, out=a1)                                            # :30
            z2 = _lin_fwd(blk.fc2, a1)                                                        # :31
            n2, m2, s2 = self._bn(blk.bn2, z2)
            f2 = ops.film_fwd(gam, n2, bet)                                                   # :33
            hn = ops.axpby(1.0, h, 1.0, f2, out=f2)                                           # :34
            if keep:
                blocks.append((h, gam, z1, n1, m1, s1, a1, z2, n2, m2, s2))
            h = hn
        cont_raw = _lin_fwd(self.fc_cont, h)
        cont = ops.axpby(self.residual_scaling, cont_raw, out=cont_raw)                       # :81
        logits = torch.empty((B, self.total_cat), dtype=torch.float32, device=x.device)
        for s, f in enumerate(self.cat_idx):
            _lin_fwd(self.fc_cat_logits[str(f)], h, out=logits[:, self.seg[s]:], ldc=self.total_cat)   # :87
        soft, hard_y = ops.gumbel_softmax_fwd(logits, noise, seg, tau, hard=hard)             # :90
        saved = (cond, inp, blocks, h, soft, seg, tau) if keep else None
        return cont, logits, (hard_y if hard else soft), saved

    @in_conv_precision
    def _run_backward(self, saved, d_cont, d_logits, d_samples):
        if saved[0] == "fused":
            return self._fused_backward(saved, d_cont, d_logits, d_samples)
        cond, inp, blocks, h_last, soft, seg, tau = saved
        if any(not blk.bn1.training for blk in self.blocks):
            raise PcgError("backward through an eval-mode BatchNorm1d is not implemented")
        B = inp.shape[0]
        T = self.total_cat
        dh = None
        if d_samples is not None:
            dl = ops.gumbel_softmax_bwd(d_samples.contiguous(), soft, seg, tau)               # straight-through for hard=True
            if d_logits is not None:
                ops.axpby(1.0, dl, 1.0, d_logits.contiguous(), out=dl)
        else:
            dl = d_logits.contiguous() if d_logits is not None else None
        if dl is not None:
            dh = torch.empty((B, self.hidden_dim), dtype=torch.float32, device=inp.device)
            for s, f in enumerate(self.cat_idx):
                head = self.fc_cat_logits[str(f)]
                dls = dl[:, self.seg[s]:]
                _lin_wgrad(self, head, h_last, dls, ldy=T)
                _lin_dgrad(head.weight.data, dls, B, ldy=T, out=dh, accumulate=s > 0)
        if d_cont is not None:
            dc = ops.axpby(self.residual_scaling, d_cont.contiguous())
            _lin_wgrad(self, self.fc_cont, h_last, dc)
            dh = _lin_dgrad(self.fc_cont.weight.data, dc, B, out=dh, accumulate=dh is not None)
        if dh is None:
            return
        C = self.hidden_dim
        for blk, (h, gam, z1, n1, m1, s1, a1, z2, n2, m2, s2) in zip(reversed(self.blocks), reversed(blocks)):
            dgam2, dn2 = ops.film_bwd(dh, gam, n2)                                            # d f2 = dh (skip keeps dh too)
            gg, acc = self._grad_view(blk.bn2.weight)
            gb, _ = self._grad_view(blk.bn2.bias)
            dz2 = ops.bn_act_bwd(dn2, z2, None, C, m2, s2, blk.bn2.weight.data, ACT_NONE, 0.0, gg, gb, acc)
            _lin_wgrad(self, blk.fc2, a1, dz2)
            da1 = _lin_dgrad(blk.fc2.weight.data, dz2, B)
            ops.act_bwd(da1, a1, ACT_RELU, 0.0, out=da1)                                      # d f1
            dgam1, dn1 = ops.film_bwd(da1, gam, n1)
            gg, acc = self._grad_view(blk.bn1.weight)
            gb, _ = self._grad_view(blk.bn1.bias)
            dz1 = ops.bn_act_bwd(dn1, z1, None, C, m1, s1, blk.bn1.weight.data, ACT_NONE, 0.0, gg, gb, acc)
            _lin_wgrad(self, blk.fc1, h, dz1)
            # FiLM parameters: gamma sees dgam1 + dgam2, beta sees d f1 + d f2
            dgam = ops.axpby(1.0, dgam1, 1.0, dgam2, out=dgam1)
            dbet = ops.axpby(1.0, da1, 1.0, dh, out=dgam2)
            _lin_wgrad(self, blk.film.gamma, cond, dgam)
            _lin_wgrad(self, blk.film.beta, cond, dbet)
            dh = _lin_dgrad(blk.fc1.weight.data, dz1, B, out=dh, accumulate=True)             # block path + skip path
        ops.act_bwd(dh, blocks[0][0] if blocks else h_last, ACT_RELU, 0.0, out=dh)
        _lin_wgrad(self, self.fc_in, inp, dh)


# ---- residual assembly (trainer.py:266-279) -----------------------------------------------------------------------------
class _AssembleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cont, samples, x, tables, norm_vals):
        seg, cat_idx, cont_idx = tables
        ctx.tables, ctx.norm, ctx.shape = tables, norm_vals, (cont.shape[1], samples.shape[1])
        return ops.assemble_residual_fwd(cont.contiguous(), cont_idx, samples.contiguous(), seg, cat_idx, norm_vals, x.contiguous())

    @staticmethod
    def backward(ctx, dres):
        seg, cat_idx, cont_idx = ctx.tables
        dcont, dsamples = ops.assemble_residual_bwd(dres.contiguous(), ctx.shape[0], cont_idx, seg, ctx.shape[1], cat_idx, ctx.norm)
        return dcont, dsamples, None, None, None


def assemble_residual(generator, cont, samples, x, norm_vals):
    """residual_full [B, D]: continuous columns from `cont`, categorical columns = E_sample[normalised value] - x."""
    return _AssembleFn.apply(cont, samples, x, generator.index_tables(x.device), norm_vals)


def cat_norm_maps(generator, config, device):
    """trainer.py:205-223 — packed [T] tensor of normalised category values, head order of the generator."""
    scaler = config.get("scaler", None)
    vals = []
    for f in generator.cat_idx:
        info = config["categorical_info"][f]
        n = _ncat(info)
        if scaler is not None:
            lo, hi = float(scaler.data_min_[f]), float(scaler.data_max_[f])
            raw = np.asarray(info["raw_values"], dtype=float)
            vals.append((raw - lo) / ((hi - lo) + 1e-12))                                      # :211-216
        else:
            vals.append(np.arange(n, dtype=float) / max(1.0, n - 1))                           # :218-223
    return torch.tensor(np.concatenate(vals), dtype=torch.float32, device=device)


class _MaskMulFn(torch.autograd.Function):
    """masked = res * mask; x_cf = x + masked (trainer.py:281-282)."""

    @staticmethod
    def forward(ctx, res, mask, x):
        ctx.mask = mask
        ctx.set_materialize_grads(False)
        _, masked = ops.scale_mask_fwd(res.contiguous(), mask, 1.0)
        x_cf = ops.axpby(1.0, x, 1.0, masked)
        return masked, x_cf

    @staticmethod
    def backward(ctx, d_masked, d_xcf):
        if d_masked is None:
            dsum = d_xcf.contiguous()
        elif d_xcf is None:
            dsum = d_masked.contiguous()
        else:
            dsum = ops.axpby(1.0, d_masked.contiguous(), 1.0, d_xcf.contiguous())
        return ops.scale_mask_bwd(None, dsum, ctx.mask, 1.0, like=ctx.mask), None, None


_ones_cache = {}


def _one(device):
    """A cached scalar 1.0 on the device: `loss.backward(gradient=_one(dev))` spares autograd its ones_like fill launch."""
    t = _ones_cache.get(device)
    if t is None:
        t = ops.fill(torch.empty((), dtype=torch.float32, device=device), 1.0)
        _ones_cache[device] = t
    return t


# ---- discriminator ------------------------------------------------------------------------------------------------------
class _DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, target_onehot, *params):
        out, saved = net._run_forward(x, target_onehot)
        ctx.net, ctx.saved = net, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        dx = ctx.net._run_backward(ctx.saved, dout, ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:]))
        return (None, dx) + (None,) * (len(ctx.needs_input_grad) - 2)


class Discriminator(FlatModule):
    """discriminator.py:5-20 — a Wasserstein-style critic of four spectral-normalised Linears.  The torch spectral_norm
    containers hold the state (`net.{0,2,4,6}.weight_orig / weight_u / weight_v / bias`); the power iteration, the
    division by sigma and its backward run in pcg_spectral_norm_fwd/bwd.  As in torch, every training-mode forward does
    one power iteration and updates u, v in place."""

    def __init__(self, input_dim, hidden_dim, num_classes):
        super().__init__()
        self.net = nn.Sequential(
            spectral_norm(nn.Linear(input_dim + num_classes, hidden_dim)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim, hidden_dim * 2)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim * 2, hidden_dim * 4)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim * 4, 1)))
        self.input_dim = input_dim

    def _linears(self):
        return [m for m in self.net if isinstance(m, nn.Linear)]

    def forward(self, x, target_onehot):
        self._ensure_flat()
        if not x.is_cuda:
            raise PcgError(f"Discriminator: input is on {x.device}; libpcgan_hip has no CPU path")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _DFn.apply(self, x, target_onehot, *self.parameters())
        return self._run_forward(x, target_onehot, keep=False)[0]

    def _fused_ok(self, x, target_onehot):
        lins = self._linears()
        return (getattr(self, "use_fused", True) and [l.out_features for l in lins] == [32, 64, 128, 1] and lins[0].in_features == 21
                and x.shape[1] + target_onehot.shape[1] == 21)

    def _spectral_norm(self):
        """Power iteration (training mode: updates u, v in place) + W / sigma of all four layers: one launch."""
        return ops.spectral_norm_fwd_batched(*self._sn_operands(), self.training)[0]

    @in_conv_precision
    def _run_forward(self, x, target_onehot, keep=True, sn=None):
        lins = self._linears()
        if sn is None:
            sn = self._spectral_norm()
        if self._fused_ok(x, target_onehot):
            # the four layers as ONE launch, one thread per row (csrc/house_critic_fused.hip)
            (acts, out), = ops.house_critic_fwd([(x.contiguous(), target_onehot.contiguous())], [t[0] for t in sn], [l.bias.data for l in lins])
            return out, (("fused", acts, sn) if keep else None)
        a = ops.concat_cols(x.contiguous(), target_onehot.contiguous())                       # :19
        layers = []
        for i, lin in enumerate(lins):
            w_bar, sigma, u, v = sn[i]
            z = _lin_fwd(lin, a, weight=w_bar, act=ACT_LRELU if i + 1 < len(lins) else ACT_NONE, slope=0.2)   # LeakyReLU fused
            if keep:
                layers.append((a, z, w_bar, sigma, u, v))
            a = z
        return a, (layers if keep else None)

    def _sn_operands(self):
        """(w_origs, us, vs, eps) of the spectrally normalised Linears: what a power iteration of this critic reads and updates."""
        lins = self._linears()
        return [l.weight_orig.data for l in lins], [l.weight_u for l in lins], [l.weight_v for l in lins], 1e-12

    @in_conv_precision
    def _run_pair(self, x_a, onehot_a, cot_a, x_b, onehot_b, cot_b, sn=None, defer_sn_bwd=False):
        """The critic step's two passes as one: D(a) then D(b) — two successive power iterations, as two forward calls make them —
        and the backward of cot_b . D(b) followed by that of cot_a . D(a) into the gradient buffer (the order the chained calls
        of train_step use), in FIVE launches instead of ten (four when the caller made the power iterations, three when it also
        takes the last one as a rider): both power iterations, both forwards, both backwards, all sixteen
        weight / bias reductions, both passes through W / sigma.  Per element the arithmetic of the chained calls (same bits).
        Returns (D(a), D(b)).  `sn`: the result of the two power iterations when the caller has already launched them;
        defer_sn_bwd: leave the last launch (the backward through W / sigma) to the caller, as a rider: returns (D(a), D(b), its
        ops.sn_bwd_batch)."""
        lins = self._linears()
        # sn: the two power iterations already made (they rode with the residual block's launch, ops.house_residual_fwd(sn=...))
        sn_a, sn_b = sn if sn is not None else ops.spectral_norm_fwd_batched(*self._sn_operands(), True, reps=2)
        B = x_a.shape[0]
        wb = [t[0] for t in sn_a] + [t[0] for t in sn_b]
        fwd = ops.house_critic_fwd([(x_a.contiguous(), onehot_a.contiguous()), (x_b.contiguous(), onehot_b.contiguous())], wb,
                                   [l.bias.data for l in lins])
        acts, outs = [f[0] for f in fwd], [f[1] for f in fwd]
        d4 = [cot_a.contiguous(), cot_b.contiguous()]
        d3, d2, d1 = zip(*(r[:3] for r in ops.house_critic_bwd(d4, wb, acts, self.input_dim, False)))
        # pass b is the first writer of the gradient buffer, pass a adds (bias: through its own buffer, added behind the b pass)
        items, seq_b, seq_a, dws, accs, bias_adds = [], [], [], [], [], []
        for li, lin in enumerate(lins):
            gb, accb = self._grad_view(lin.bias)
            gw, acc = self._grad_view(lin.weight_orig)
            dw_b, dw_a = torch.empty_like(sn_b[li][0]), torch.empty_like(sn_a[li][0])
            gb_a = torch.empty_like(gb)
            O, I = lin.out_features, lin.in_features
            items.append(((d1, d2, d3, d4)[li][1], acts[1][li], O, I, dw_b, gb, O, I, False, accb))
            items.append(((d1, d2, d3, d4)[li][0], acts[0][li], O, I, dw_a, gb_a, O, I, False, False))
            seq_b.append((dw_b, sn_b[li][0], sn_b[li][2], sn_b[li][3], sn_b[li][1]))
            seq_a.append((dw_a, sn_a[li][0], sn_a[li][2], sn_a[li][3], sn_a[li][1]))
            dws.append(gw); accs.append(acc); bias_adds.append((gb, gb_a))
        ops.linear_wgrad_grouped(items, B, x_a.device)
        if defer_sn_bwd:
            return outs[0], outs[1], ops.sn_bwd_batch([seq_b, seq_a], dws, accs, bias_adds)
        ops.spectral_norm_bwd_batched([seq_b, seq_a], dws, accs, bias_adds)
        return outs[0], outs[1]

    @in_conv_precision
    def _fused_backward(self, saved, dout, need_x, need_p):
        _, acts, sn = saved
        lins = self._linears()
        d4 = dout.contiguous()
        (d3, d2, d1, dx), = ops.house_critic_bwd([d4], [t[0] for t in sn], [acts], self.input_dim, need_x)
        if need_p and lins[0].weight_orig.requires_grad:
            items, seq, dws, accs = [], [], [], []
            for lin, a, d, (w_bar, sigma, u, v) in zip(lins, acts, (d1, d2, d3, d4), sn):
                dwb = torch.empty_like(w_bar)
                gb, accb = self._grad_view(lin.bias)
                gw, acc = self._grad_view(lin.weight_orig)
                items.append((d, a, lin.out_features, lin.in_features, dwb, gb, lin.out_features, lin.in_features, False, accb))
                seq.append((dwb, w_bar, u, v, sigma)); dws.append(gw); accs.append(acc)
            ops.linear_wgrad_grouped(items, d4.shape[0], d4.device)                          # all weight + bias gradients: one launch
            ops.spectral_norm_bwd_batched([seq], dws, accs)                                  # through W / sigma: one launch
        return dx

    @in_conv_precision
    def _run_backward(self, layers, dout, need_x, need_p):
        if layers[0] == "fused":
            return self._fused_backward(layers, dout, need_x, need_p)
        lins = self._linears()
        d = dout.contiguous()
        B = d.shape[0]
        seq, dws, accs = [], [], []
        for i in range(len(lins) - 1, -1, -1):
            lin = lins[i]
            a, z, w_bar, sigma, u, v = layers[i]
            if i + 1 < len(lins):
                d = ops.act_bwd(d, z, ACT_LRELU, 0.2)
            if need_p and lin.weight_orig.requires_grad:
                dwb = torch.empty_like(w_bar)
                _lin_wgrad(self, lin, a, d, dw_out=dwb, weight_param=lin.weight_orig)
                gw, acc = self._grad_view(lin.weight_orig)
                seq.append((dwb, w_bar, u, v, sigma)); dws.append(gw); accs.append(acc)
            if i > 0 or need_x:
                d = _lin_dgrad(w_bar, d, B)
        if seq:
            ops.spectral_norm_bwd_batched([seq], dws, accs)                                  # all layers: one launch
        if not need_x:
            return None
        dx, _ = ops.split_cols(d, self.input_dim, d.shape[1] - self.input_dim, need_b=False)
        return dx


# ---- frozen classifier ------------------------------------------------------------------------------------------------
class NNClassifier(FrozenClassifier):
    """nn_classifier.py:4-32.  In the GAN step: eval mode, parameters frozen (main.py:27-30) — forward and the gradient with
    respect to the input row; each BatchNorm1d is then a per-column affine map folded into the following Linear once (fp64 at
    pack time): 5 GEMMs and 4 LeakyReLUs.  In training mode (pre-training, trainer.py:18-180 — SURVEY.md section 8f item 3):
    Linear -> LeakyReLU(0.1) -> BatchNorm1d (batch statistics) -> Dropout, with the Dropout masks from `self.rng` (device
    Philox stream) or `self.dropout_masks = [m0 [B,256], m1 [B,256], m2 [B,128]]` for runs that must reproduce given draws."""

    def __init__(self, input_dim, output_dim=4):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(input_dim, 256), nn.LeakyReLU(0.1), nn.BatchNorm1d(256), nn.Dropout(0.3),
            nn.Linear(256, 256), nn.LeakyReLU(0.1), nn.BatchNorm1d(256), nn.Dropout(0.2),
            nn.Linear(256, 128), nn.LeakyReLU(0.1), nn.BatchNorm1d(128), nn.Dropout(0.1),
            nn.Linear(128, 64), nn.LeakyReLU(0.1), nn.BatchNorm1d(64),
            nn.Linear(64, output_dim))

    def _pack(self):
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        if self.training:
            raise PcgError("NNClassifier: only eval mode is implemented (the GAN step uses the frozen classifier)")
        packed, scale, shift = [], None, None
        with torch.no_grad():
            for m in self.net:
                if isinstance(m, nn.Linear):
                    w, b = m.weight.double(), m.bias.double()
                    if scale is not None:            # Linear(bn(a)) = a (W diag(s))^T + (W t + b)
                        b = b + w @ shift
                        w = w * scale[None, :]
                        scale = shift = None
                    packed.append((w.float().contiguous(), b.float().contiguous()))
                elif isinstance(m, nn.BatchNorm1d):
                    s = m.weight.double() / torch.sqrt(m.running_var.double() + m.eps)
                    scale, shift = s, m.bias.double() - m.running_mean.double() * s
        self._packed = (key, packed)
        self._kmajor = None
        return packed

    def _fused_ok(self, x):
        dims = [m.in_features for m in self.net if isinstance(m, nn.Linear)] + [self.net[-1].out_features]
        return getattr(self, "use_fused", True) and x.is_cuda and x.shape[1] == 17 and dims == [17, 256, 256, 128, 64, 4]

    def _pack_kmajor(self):
        """Per layer the folded weight transposed ([K][N]: the forward's B operand is then a coalesced read), layer 0 padded with a
        zero rows to a multiple of the MFMA's reduction depth (17 -> 20); the last layer stays as stored.  Built once per pack."""
        packed = self._pack()
        if getattr(self, "_kmajor", None) is None:
            with torch.no_grad():
                km = [w.t().contiguous() for w, _ in packed[:4]]
                km[0] = torch.cat([km[0], torch.zeros((3, km[0].shape[1]), dtype=km[0].dtype, device=km[0].device)], 0).contiguous()   # K 17 -> 20
                km.append(packed[4][0])
            self._kmajor = km
        return self._kmajor

    def _draw_dropout_masks(self, x):
        return [self.rng.bernoulli((x.shape[0], m_.out_features), x.device, 1.0 - p_) for m_, p_ in self._dropout_sites()]

    # -- training mode ------------------------------------------------------------------------------------------------------------
    def _stages(self):
        """[(Linear, BatchNorm1d, dropout p or None)] + the final Linear."""
        mods, stages, i = list(self.net), [], 0
        while i < len(mods) - 1:
            lin, bn = mods[i], mods[i + 2]
            p = mods[i + 3].p if i + 3 < len(mods) and isinstance(mods[i + 3], nn.Dropout) else None
            stages.append((lin, bn, p))
            i += 4 if p is not None else 3
        return stages, mods[-1]

    def _dropout_sites(self):
        return [(lin, p) for lin, _, p in self._stages()[0] if p is not None]

    @in_conv_precision
    def _train_forward(self, x, masks):
        stages, last = self._stages()
        a = x.contiguous()
        saved, mi = [], 0
        for lin, bn, p in stages:
            z = _lin_fwd(lin, a)
            ops.act_fwd(z, ACT_LRELU, 0.1, out=z)                                            # act output (BatchNorm input)
            C = bn.num_features
            mean, invstd = ops.bn_train_stats(z, C, bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked)
            n = ops.bn_apply_act(z, C, mean, invstd, bn.weight.data, bn.bias.data, ACT_NONE)
            mask = None
            if p is not None:
                mask = masks[mi].contiguous(); mi += 1
                n = ops.dropout_apply(n, mask, p, out=n)
            saved.append((lin, bn, p, a, z, mean, invstd, mask))
            a = n
        logits = _lin_fwd(last, a)
        return logits, (saved, last, a)

    @in_conv_precision
    def _train_backward(self, saved_all, dlogits):
        saved, last, a_last = saved_all
        B = a_last.shape[0]
        d = dlogits.contiguous()
        _lin_wgrad(self, last, a_last, d)
        d = _lin_dgrad(last.weight.data, d, B)
        for idx in range(len(saved) - 1, -1, -1):
            lin, bn, p, a, z, mean, invstd, mask = saved[idx]
            if p is not None:
                d = ops.dropout_apply(d, mask, p, out=d)
            gg, acc = self._grad_view(bn.weight)
            gb, _ = self._grad_view(bn.bias)
            d = ops.bn_act_bwd(d, z, None, bn.num_features, mean, invstd, bn.weight.data, ACT_NONE, 0.0, gg, gb, acc)
            ops.act_bwd(d, z, ACT_LRELU, 0.1, out=d)
            _lin_wgrad(self, lin, a, d)
            if idx > 0:
                d = _lin_dgrad(lin.weight.data, d, B)

    @in_conv_precision
    def _run_forward(self, x, keep=True, sn_bwd_rider=None, ce=None):
        """sn_bwd_rider: a spectral-norm backward (ops.sn_bwd_batch) that rides in the fused forward launch (the scheduled tabular
        step: the critic's spectral-norm backward is independent of this classifier).  ce = (target, grad_scale) with a rider: the
        launch also leaves the cross-entropy's gradient and row terms; returns (logits, acts, dlogits, row_loss)."""
        packed = self._pack()
        a = x.contiguous()
        if sn_bwd_rider is not None and not self._fused_ok(a):
            raise PcgError("NNClassifier: a rider needs the fused forward launch")
        if ce is not None and sn_bwd_rider is None:
            raise PcgError("NNClassifier: the cross-entropy tail needs a rider")
        if self._fused_ok(a):
            # the five layers as ONE launch on the matrix cores (csrc/house_classifier_fused.hip)
            out = ops.house_classifier_fwd(a, self._pack_kmajor(), [b for _, b in packed], sn_bwd=sn_bwd_rider, ce=ce)
            return (out[0], out[1] if keep else None) + out[2:]
        acts = []
        for i, (w, b) in enumerate(packed):
            z = affine_fwd(a, w, b, act=ACT_LRELU if i + 1 < len(packed) else ACT_NONE, slope=0.1)
            if i + 1 < len(packed):
                if keep:
                    acts.append(z)
            a = z
        return a, (acts if keep else None)

    @in_conv_precision
    def _run_backward(self, acts, dlogits, sn_fwd_rider=None):
        """sn_fwd_rider: a training-mode spectral normalisation (the batch of ops.sn_fwd_batch) that rides in the fused backward
        launch; the return value is then (dx, its outputs)."""
        packed = self._pack()
        d = dlogits.contiguous()
        B = d.shape[0]
        fused = d.is_cuda and len(acts) == 4 and [t.shape[1] for t in acts] == [256, 256, 128, 64] and getattr(self, "use_fused", True) and d.shape[1] == 4
        if sn_fwd_rider is not None and not fused:
            raise PcgError("NNClassifier: a rider needs the fused backward launch")
        if fused:
            return ops.house_classifier_bwd(d, [w for w, _ in packed], acts, sn_fwd=sn_fwd_rider)
        for i in range(len(packed) - 1, -1, -1):
            if i + 1 < len(packed):
                d = ops.act_bwd(d, acts[i], ACT_LRELU, 0.1, out=d)
            d = _lin_dgrad(packed[i][0], d, B)
        return d


# ---- trainer ------------------------------------------------------------------------------------------------------------
def make_optimizers(generator, discriminator, config=CONFIG):
    """trainer.py:229-230."""
    return Adam(generator.parameters(), lr=config["lr_G"]), Adam(discriminator.parameters(), lr=config["lr_D"])


def train_step(generator, discriminator, classifier, opt_g, opt_d, x, y, target_y, mask, norm_vals, config=CONFIG, gumbel=None,
               ce=None, skip_dead_d_wgrad=True, branch=None, onehots=None, diag=None):
    """One iteration of train_countergan's loop body (trainer.py:241-316) for a batch already on the GPU.  The draws —
    `target_y` (:248-249), `mask` (:253-255) and the Gumbel noise inside G (gumbel=None: generator.rng) — are inputs.
    Returns device tensors; the reference's `.item()` calls are the caller's.

    branch: a second HIP stream.  The step is a chain of ~100 tiny kernels (64 blocks each on a 256-CU chip), i.e. bound by the
    length of its dependency chain; the frozen classifier's pass (trainer.py:301-302: forward, cross-entropy and — in backward —
    the gradient with respect to x_cf; ~25 % of the chain) depends only on x_cf, so it is forked onto `branch` as soon as x_cf
    exists and runs beside the whole critic update; it joins where g_loss is formed.  autograd runs a node's backward on the
    stream its forward ran on, so the classifier's backward overlaps the critic's in the G step too.  Same kernels, same inputs:
    results are bit-identical to the single-stream order; captured in a HIP graph the two streams become parallel branches.

    diag: {"logits_orig": the frozen classifier's logits of the original rows ([B, nc], or [N, nc] of the whole training set with
    "src_rows" [B]), "acc": float64[8] epoch accumulators or None, "eps": 1e-3} — the trainer's per-iteration diagnostics
    (trainer.py:318-343: pred_gain, sparsity, reg_loss_l2, class_flip_rate) as one fused device reduction, returned as out["diag"]
    ([4] device tensor) and summed into `acc` together with D_loss / G_loss (read once per epoch, no .item() per iteration)."""
    if branch is not None:
        return _train_step_branch(generator, discriminator, classifier, opt_g, opt_d, x, y, target_y, mask, norm_vals, config, gumbel,
                                  branch, skip_dead_d_wgrad, onehots, diag)
    nc = config["num_classes"]
    ce = ce if ce is not None else CrossEntropyLoss()
    target_onehot = ops.onehot(target_y, nc)                                                  # :250
    cont, _, samples = generator.forward_packed(x, target_onehot, mask, temperature=config["gumbel_tau"], hard=False,
                                                gumbel=gumbel)                                # :259-261
    residual_full = assemble_residual(generator, cont, samples, x, norm_vals)                 # :266-279
    masked_residual, x_cf = _MaskMulFn.apply(residual_full, mask, x)                          # :281-282
    mask_penalty_pre = abs_mean(residual_full, mask, one_minus=True)                          # :287
    # ---- D step
    d_real = discriminator(x, ops.onehot(y, nc))                                              # :290
    d_fake = discriminator(x_cf.detach(), target_onehot)                                      # :291
    d_loss = weighted_sum([mean(d_fake), mean(d_real)], [1.0, -1.0])                          # :292
    opt_d.zero_grad()
    d_loss.backward(gradient=_one(x.device))
    opt_d.step()                                                                              # :293-295
    # ---- G step
    if skip_dead_d_wgrad:            # the reference computes D's weight gradients here and never uses them (next zero_grad)
        for p in discriminator.parameters():
            p.requires_grad_(False)
    try:
        d_fake_for_g = discriminator(x_cf, target_onehot)                                     # :298
        m_fake = mean(d_fake_for_g)
        clf_preds = classifier(x_cf)                                                          # :301
        g_cls = ce(clf_preds, target_y)                                                       # :302
        am = abs_mean(masked_residual)                                                        # :305  mean_b ||.||_1 = D * mean|.|
        d_feat = float(x.shape[1])
        g_loss = weighted_sum([m_fake, g_cls, am, mask_penalty_pre],
                              [-1.0, config["lambda_cls"], config["lambda_reg"] * d_feat, config["lambda_mask"]])   # :299, :307-312
        with torch.no_grad():                                                                 # logged values
            g_adv = weighted_sum([m_fake], [-1.0])
            g_reg = weighted_sum([am], [d_feat])
        opt_g.zero_grad()
        g_loss.backward(gradient=_one(x.device))                                              # :314-315
    finally:
        if skip_dead_d_wgrad:
            for p in discriminator.parameters():
                p.requires_grad_(True)
    opt_g.step()                                                                              # :316
    out = {"D_loss": d_loss, "G_loss": g_loss, "g_adv": g_adv, "g_cls": g_cls, "reg": g_reg, "mask_pen": mask_penalty_pre,
           "D_real": d_real, "D_fake_forG": d_fake_for_g, "x_cf": x_cf, "masked_residual": masked_residual}
    if diag is not None:                                                                      # :318-343
        with torch.no_grad():
            out["diag"] = ops.house_diag(clf_preds.detach().contiguous(), diag["logits_orig"], target_y, masked_residual.detach().contiguous(),
                                         eps=diag.get("eps", 1e-3), src_rows=diag.get("src_rows"), acc=diag.get("acc"))
            _acc_losses(diag.get("acc"), d_loss, g_loss)
    return out


def _acc_losses(acc, d_loss, g_loss):
    """acc[0] += D_loss, acc[1] += G_loss, acc[6] += 1 (the schedule of train_step(branch=...) does this inside its scalars launch;
    the reference-order step with three tiny device adds — setup / test path, not the benched one)."""
    if acc is not None:
        acc[0] += d_loss.detach().double()
        acc[1] += g_loss.detach().double()
        acc[6] += 1.0


_cot_cache = {}


def _mean_cotangents(B, device):
    """(+1/B, -1/B) as [B, 1] tensors: d(mean(out))/d(out) scaled by the Wasserstein losses' weights (+1 and -1, trainer.py:292, :299).
    They are constants of the step, so the critic's backward can start the moment its forward is done — no loss kernels on the
    chain.  Built once with the very kernels autograd would run (weighted_sum's backward, then mean's backward): same bits."""
    key = (int(B), device)
    c = _cot_cache.get(key)
    if c is None:
        like = torch.empty((B, 1), dtype=torch.float32, device=device)
        gpos, gneg = ops.weighted_sum_bwd((1.0, -1.0), _one(device).view(1), (True, True))
        c = (ops.mean_bwd(gpos.contiguous(), 1.0, like), ops.mean_bwd(gneg.contiguous(), 1.0, like))
        _cot_cache[key] = c
    return c


def _train_step_branch(generator, discriminator, classifier, opt_g, opt_d, x, y, target_y, mask, norm_vals, config, gumbel, branch,
                       skip_dead_d_wgrad, onehots=None, diag=None):
    """train_step scheduled for the length of its dependency chain (the step is a chain of small kernels, 36 launches on one stream): what the
    reference's loop body computes, bit for bit (tests/test_hip_house.py: graph vs eager vs the reference-order autograd step), with

      * no autograd graph: every backward is called directly, in the order autograd would run it;
      * residual assembly, mask, x_cf and both L1 penalties (:266-287, :305) in one launch, and the whole way back from
        dLoss/dx_cf (critic: -1/B through D; classifier: from the branch) to the generator's outputs in one (:314-315);
      * the frozen classifier's whole term (:301-302) — forward, cross-entropy value AND gradient in one launch (grad_scale =
        lambda_cls, exactly the product autograd forms), grad-input sweep — on the `branch` stream beside the critic update,
        the logged scalars (D_loss, G_loss, g_adv, g_reg) there too;
      * the critic step's two passes as one (Discriminator._run_pair): the cotangents of the Wasserstein means are the constants
        +-1/B (_mean_cotangents), the fake pass is the first writer of the gradient buffer, the real pass adds;
      * no gradient zero-fills: every parameter of both nets receives a gradient, the first writer overwrites (0 + g == g);
      * riders (one launch whose blocks split between two independent kernel bodies): the critic step's two power iterations in the
        residual block's forward launch, the logged scalars in its backward launch; on ONE stream also the critic's backward through
        W / sigma in the classifier's forward launch (whose tail is the cross-entropy) and the power iteration of the generator step's
        critic call in its backward launch.
    Captured in a HIP graph the two streams are parallel branches; branch="inline": everything on one stream (the default)."""
    nc, dev, B = config["num_classes"], x.device, x.shape[0]
    if classifier.training or any(p.requires_grad for p in classifier.parameters()):
        raise PcgError("train_step(branch=...): the classifier must be frozen and in eval mode (main.py:27-30)")
    main = torch.cuda.current_stream()
    if isinstance(branch, str):        # "inline": this schedule's kernels, all on the current stream (no fork: every wait is a no-op)
        branch = main
    discriminator._ensure_flat(); generator._ensure_flat()
    cot_pos, cot_neg = _mean_cotangents(B, dev)
    d_feat = float(x.shape[1])
    if not x.is_cuda:
        raise PcgError(f"train_step: input is on {x.device}; libpcgan_hip has no CPU path")
    seg, cat_idx, cont_idx = generator.index_tables(dev)
    x, mask = x.contiguous(), mask.contiguous()
    # onehots = (one_hot(target_y), one_hot(y)) already made (draw_batch_randoms writes them with the draws): two launches less
    target_onehot = onehots[0] if onehots is not None else ops.onehot(target_y, nc)            # :250
    with torch.no_grad():            # no autograd graph anywhere in this schedule: every backward below is called directly
        cont, _, samples, g_saved = generator._run_forward(x, target_onehot, mask, generator._noise(gumbel, B, dev),
                                                           float(config["gumbel_tau"]), False)            # :259-261
        # residual assembly, mask, x_cf and both L1 penalties (:266-287, :305): one launch — and the critic step's two power
        # iterations ride in it (they only read the critic's weights: one launch less on the chain)
        onehot_y = onehots[1] if onehots is not None else ops.onehot(y, nc)
        # (training mode: every critic call of the step makes a power iteration — the batched / riding forms assume it)
        pair = discriminator.training and discriminator._fused_ok(x, onehot_y) and all(p.requires_grad for p in discriminator.parameters())
        rf = ops.house_residual_fwd(cont.contiguous(), samples.contiguous(), seg, norm_vals, x, mask, generator.col_src(),
                                    sn=ops.sn_fwd_batch(*discriminator._sn_operands(), reps=2)[1] if pair else None)
        residual_full, masked_residual, x_cf, mask_penalty_pre, am = rf[:5]
        sn_pair = rf[5] if pair else None
    # the zero-fills of the two gradient buffers are not launched: every parameter of both nets receives a gradient in this step,
    # so the first writer overwrites (0 + g == g)
    discriminator.drop_grads(); generator.drop_grads()
    # One stream and the fused critic pair: the classifier's two launches carry the critic's spectral-norm work that is on the chain
    # at the same time (riders) — its forward the backward through W / sigma of the critic step, its backward the power iteration
    # of the generator step's critic call.  Otherwise the classifier's term runs on the branch beside the critic update.
    xc = x_cf.detach().contiguous()
    riders = pair and branch is main and classifier._fused_ok(xc)
    if not riders:
        # ---- fork
        branch.wait_stream(main)
        with torch.cuda.stream(branch):
            with torch.no_grad():
                logits_c, acts_c = classifier._run_forward(xc, keep=True)                                         # :301
                g_cls, dlog = ops.cross_entropy_fwd_bwd(logits_c.contiguous(), target_y, need_loss=True, need_grad=True,
                                                        grad_scale=float(config["lambda_cls"]))                  # :302
                dx_cls = classifier._run_backward(acts_c, dlog)
                g_cls = g_cls.view(())
        for t in (x_cf, target_y):
            t.record_stream(branch)
    # ---- D step (:290-295)
    xd = x_cf.detach()
    with torch.no_grad():
        if riders:
            d_real, d_fake, sn_bwd = discriminator._run_pair(x, onehot_y, cot_neg, xd, target_onehot, cot_pos, sn=sn_pair,
                                                             defer_sn_bwd=True)                               # :290-294, three launches
            # :301 + the fourth; with the logged scalars riding below, the cross-entropy (:302) is the tail of this launch too
            ce_tail = B <= 16 * 1024
            cf = classifier._run_forward(xc, keep=True, sn_bwd_rider=sn_bwd,
                                         ce=(target_y, float(config["lambda_cls"])) if ce_tail else None)
            logits_c, acts_c = cf[:2]
        elif pair:
            d_real, d_fake = discriminator._run_pair(x, onehot_y, cot_neg, xd, target_onehot, cot_pos, sn=sn_pair)   # :290-294, four launches
        else:
            d_real, sv_r = discriminator._run_forward(x, onehot_y, keep=True)                 # :290
            d_fake, sv_f = discriminator._run_forward(xd, target_onehot, keep=True)           # :291
            discriminator._run_backward(sv_f, cot_pos, False, True)                           # d(mean(d_fake) - mean(d_real))
            discriminator._run_backward(sv_r, cot_neg, False, True)
    opt_d.step()                                                                              # :295
    # ---- G step (:298-316)
    with torch.no_grad():
        sn_g = None
        if riders:
            if ce_tail:
                dlog, g_cls = cf[2], cf[3]        # g_cls: still the row terms; the launch that logs the scalars forms their mean
            else:
                g_cls, dlog = ops.cross_entropy_fwd_bwd(logits_c.contiguous(), target_y, need_loss=True, need_grad=True,
                                                        grad_scale=float(config["lambda_cls"]))              # :302
                g_cls = g_cls.view(())
            dx_cls, sn_out = classifier._run_backward(acts_c, dlog, sn_fwd_rider=ops.sn_fwd_batch(*discriminator._sn_operands())[1])
            sn_g = sn_out[0]                                                                  # the power iteration of the :298 call
        d_fake_for_g, sv_g = discriminator._run_forward(xd, target_onehot, keep=True, sn=sn_g)   # :298
        ride = B <= 16 * 1024  # the five logged scalars ride in the launch of the residual block's backward (same trees, same bits)
        if not ride:
            fwd_done = torch.cuda.Event()
            fwd_done.record(main)
        dx_d = discriminator._run_backward(sv_g, cot_neg, True, not skip_dead_d_wgrad)        # d(-mean(D(x_cf)))/d(x_cf)
    if not ride:               # on the branch, as soon as the last critic forward is out
        branch.wait_event(fwd_done)
        with torch.cuda.stream(branch), torch.no_grad():
            m_fake = ops.mean_fwd(d_fake_for_g.contiguous()).view(())
            d_loss = ops.weighted_sum_fwd([ops.mean_fwd(d_fake.contiguous()), ops.mean_fwd(d_real.contiguous())], [1.0, -1.0]).view(())
            g_loss = ops.weighted_sum_fwd([m_fake, g_cls, am, mask_penalty_pre],
                                          [-1.0, config["lambda_cls"], config["lambda_reg"] * d_feat, config["lambda_mask"]]).view(())
            g_adv = ops.weighted_sum_fwd([m_fake], [-1.0]).view(())
            g_reg = ops.weighted_sum_fwd([am], [d_feat]).view(())
        for t in (d_real, d_fake, d_fake_for_g):
            t.record_stream(branch)
    main.wait_stream(branch)                                                                  # join: dx_cls (and g_cls)
    dx_cls.record_stream(main); g_cls.record_stream(main)
    with torch.no_grad():
        # :314-315 from dLoss/dx_cf = dx_d + dx_cls and the two penalty weights down to the generator's outputs: one launch
        rb = ops.house_residual_bwd(residual_full, masked_residual, mask, dx_d.contiguous(), dx_cls.contiguous(),
                                    config["lambda_mask"], config["lambda_reg"] * d_feat, len(generator.continuous_idx), cont_idx,
                                    seg, generator.total_cat, cat_idx, norm_vals,
                                    losses=(d_real, d_fake, d_fake_for_g, g_cls, am, mask_penalty_pre, float(config["lambda_cls"]),
                                            float(config["lambda_reg"] * d_feat), float(config["lambda_mask"]), d_feat) if ride else None,
                                    diag=(logits_c.contiguous(), diag["logits_orig"], diag.get("src_rows"), target_y, diag.get("eps", 1e-3),
                                          diag.get("acc")) if (ride and diag is not None) else None)
        d_cont, d_samples = rb[:2]
        if ride:
            d_loss, g_loss, g_adv, g_reg = rb[2][0], rb[2][1], rb[2][2], rb[2][3]             # :292, :307-312
            if g_cls.numel() > 1:
                g_cls = rb[2][5]
        generator._run_backward(g_saved, d_cont, None, d_samples)
    opt_g.step()                                                                              # :316
    main.wait_stream(branch)                                                                  # final join
    for t in (d_loss, g_loss, g_adv, g_reg, g_cls):
        t.record_stream(main)
    out = {"D_loss": d_loss, "G_loss": g_loss, "g_adv": g_adv, "g_cls": g_cls, "reg": g_reg, "mask_pen": mask_penalty_pre,
           "D_real": d_real, "D_fake_forG": d_fake_for_g, "x_cf": x_cf, "masked_residual": masked_residual}
    if diag is not None:                                                                      # :318-343
        if ride:
            out["diag"] = rb[3]                      # rode in the residual block's backward launch, with the accumulators
        else:
            with torch.no_grad():
                out["diag"] = ops.house_diag(logits_c.contiguous(), diag["logits_orig"], target_y, masked_residual, eps=diag.get("eps", 1e-3),
                                             src_rows=diag.get("src_rows"), acc=diag.get("acc"))
                _acc_losses(diag.get("acc"), d_loss, g_loss)
    return out


# ---- evaluation ------------------------------------------------------------------------------
def build_counterfactuals(G, x, target_onehot, config, gumbel=None, norm_vals=None):
    """eval_utils.py:25-181 for this generator's output signature: all features modifiable except the immutable ones, hard
    Gumbel-softmax samples (:76-77), residual assembly (:127-171), clamp to [0, 1] (:180).  Returns (masked_residual, x_cf)."""
    device = x.device
    mask = torch.empty_like(x)
    ops.fill(mask, 1.0)
    imm = list(config.get("immutable_idx", []))
    if imm:
        mask[:, imm] = 0.0                                                                  # :48-50 (setup-sized strided fill)
    norm_vals = norm_vals if norm_vals is not None else cat_norm_maps(G, config, device)    # :56-67
    cont, _, samples = G.forward_packed(x, target_onehot, mask, temperature=config.get("gumbel_tau", None), hard=True, gumbel=gumbel)
    residual_full = ops.assemble_residual_fwd(cont.contiguous(), G.index_tables(device)[2], samples.contiguous(),
                                              G.index_tables(device)[0], G.index_tables(device)[1], norm_vals, x.contiguous())
    _, masked = ops.scale_mask_fwd(residual_full, mask, 1.0)                                # :174-177
    x_cf = ops.clamp_add_fwd(x.contiguous(), masked, 0.0, 1.0)                              # :180
    return masked, x_cf


def compute_metrics_per_target(generator, classifier, X, y, config, gumbel_per_call=None, rng=None, max_vis=500, one_launch=False):
    """eval_utils.py:185-289 — per target class: class-flip rate, prediction gain, mean |masked residual| over the samples whose
    class differs from the target, averaged over batches.  X, y: numpy arrays (already MinMax-scaled).  `gumbel_per_call`: an
    iterator of packed noise tensors, one per generator call, for runs that must reproduce given draws; otherwise `rng`.
    one_launch=True: every target class and every loader batch in ONE launch of pcg_house_cf_eval (csrc/house_cf_eval.hip, DESIGN.md
    §3.12) on the same draws — the per-call noise laid into [T][N][Tcat] at the rows each call would have selected — and one read of
    the tile sums; same return type."""
    import numpy as np
    if one_launch:
        return _metrics_one_launch(generator, classifier, X, y, config, gumbel_per_call, rng, max_vis)
    device = next(generator.parameters()).device
    bs_cfg = int(config.get("batch_size", 128))
    X_t, y_t = torch.as_tensor(X, dtype=torch.float32), torch.as_tensor(y, dtype=torch.long)
    num_classes = int(np.unique(np.asarray(y)).size)
    generator.eval(); classifier.eval()
    if gumbel_per_call is None and generator.rng is None:
        generator.rng = rng if rng is not None else ops.DeviceRNG(seed=0)
    norm_vals = cat_norm_maps(generator, config, device)
    noise_it = iter(gumbel_per_call) if gumbel_per_call is not None else None
    results, originals, cfs = [], [], []
    with torch.no_grad():
        for target in range(num_classes):
            flips, gains, actions = [], [], []
            for i in range(0, X_t.shape[0], bs_cfg):
                xb, yb = X_t[i:i + bs_cfg], y_t[i:i + bs_cfg]
                sel = yb != target                                                          # :224-226 (host-side selection)
                if int(sel.sum()) == 0:
                    continue
                x = xb[sel].to(device).contiguous()
                bs = x.shape[0]
                target_vec = torch.full((bs,), target, dtype=torch.long, device=device)
                target_onehot = ops.onehot(target_vec, num_classes)
                noise = next(noise_it) if noise_it is not None else None
                masked, _ = build_counterfactuals(generator, x, target_onehot, config, gumbel=noise, norm_vals=norm_vals)
                x_cf = ops.axpby(1.0, x, 1.0, masked)                                       # :243 (unclamped, as the reference)
                m = ops.cf_metrics(classifier(x_cf).contiguous(), target_vec, logits_ref=classifier(x).contiguous()).cpu()
                flips.append(float(m[0])); gains.append(float(m[1])); actions.append(abs_mean(masked).item())
                if sum(o.shape[0] for o in originals) < max_vis:
                    originals.append(x.cpu()); cfs.append(x_cf.cpu())
            results.append({"target_class": target, "class_flip": float(np.mean(flips)) if flips else float("nan"),
                            "prediction_gain": float(np.mean(gains)) if gains else float("nan"),
                            "avg_actionability": float(np.mean(actions)) if actions else float("nan")})
    originals = torch.cat(originals, 0).numpy() if originals else np.empty((0, X_t.shape[1]))
    cfs = torch.cat(cfs, 0).numpy() if cfs else np.empty((0, X_t.shape[1]))
    return results, originals, cfs


# ---- prompted queries and evaluation in ONE launch (csrc/house_cf_eval.hip) -------------------------------------
CF_ROW_OUTPUTS = ("cont", "logits", "chosen", "masked_residual", "x_cf", "x_cf_raw", "logits_cf", "logits_x", "pred_cf", "pred_x", "gain")
METRIC_FIELDS = _cfeval.METRIC_FIELDS
CF_TILE_ROWS = 16           # rows per workgroup of pcg_house_cf_eval: tiles never straddle a group
CF_QUERY_GROUP = 256        # the group where the caller names no batch size (queries: no sums are read)
_CF_FIELD = {"masked_residual": "masked"}                                     # the argument struct's names where they differ
_CF_CLS_DIMS = [17, 256, 256, 128, 64, 4]


def prompt_mask(config, allowed=None, feature_names=FEATURES):
    """gradio_app.py:150-155 — the feature mask of one request: 1 for the features the prompt allows to move (`allowed`: names from
    feature_names and / or column indices; None: all of them), 0 for the rest and ALWAYS 0 for config['immutable_idx'].
    Returns a float32 ndarray [len(feature_names)]."""
    names = list(feature_names)
    D = len(names)
    mask = np.zeros(D, dtype=np.float32)
    if allowed is None:
        mask[:] = 1.0
    else:
        if isinstance(allowed, (str, int, np.integer)):
            allowed = [allowed]
        for a_ in allowed:
            if isinstance(a_, str):
                if a_ not in names:
                    raise PcgError(f"prompt_mask: unknown feature {a_!r} (known: {names})")
                mask[names.index(a_)] = 1.0
            elif isinstance(a_, (int, np.integer)) and not isinstance(a_, bool):
                if not 0 <= int(a_) < D:
                    raise PcgError(f"prompt_mask: feature index {int(a_)} outside [0, {D})")
                mask[int(a_)] = 1.0
            else:
                raise PcgError(f"prompt_mask: allowed entries are feature names or column indices, got {a_!r}")
    for i in config.get("immutable_idx", []):
        mask[int(i)] = 0.0
    return mask


def _cf_nets(generator, classifier):
    """Host guards of the one-launch evaluation, before anything touches the GPU."""
    if generator.training or classifier.training:
        raise PcgError("the one-launch evaluation uses BatchNorm's running statistics: put the generator and the classifier in eval mode (.eval())")
    if not generator._eval_dims_ok():
        raise PcgError("pcg_house_cf_eval is built for input_dim 17, 4 classes, hidden_dim 32, 5 blocks, at most 8 heads of at most 32 "
                       "categories (96 in all) and one BatchNorm eps; this generator is outside that")
    dims = [m.in_features for m in classifier.net if isinstance(m, nn.Linear)] + [classifier.net[-1].out_features]
    if dims != _CF_CLS_DIMS:
        raise PcgError(f"pcg_house_cf_eval is built for the classifier widths {_CF_CLS_DIMS}, got {dims}")


def _cf_mask(mask, config, N):
    """None: prompt_mask(config); a [17] vector (broadcast) or [N][17] (one mask per row).  Returns (float32 tensor, per-row flag)."""
    if mask is None:
        mask = prompt_mask(config)
    m = mask.detach() if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask, dtype=np.float32))
    if tuple(m.shape) not in ((17,), (N, 17)):
        raise PcgError(f"mask must be [17] or [N][17] (N = {N}), got {tuple(m.shape)}")
    return m.to(torch.float32), m.dim() == 2


def _cf_given_noise(generator, gumbel, T, N):
    """Shape check of supplied Gumbel noise: [T][N][Tcat] (or [N][Tcat] / a dict idx -> [N][n] where T = 1).  None stays None."""
    if gumbel is None:
        return None
    Tc = generator.total_cat
    if isinstance(gumbel, dict):
        gumbel = generator.pack_noise(gumbel)
    if not torch.is_tensor(gumbel):
        gumbel = torch.as_tensor(np.asarray(gumbel, dtype=np.float32))
    if T == 1 and tuple(gumbel.shape) == (N, Tc):
        gumbel = gumbel.reshape(1, N, Tc)
    if tuple(gumbel.shape) != (T, N, Tc):
        raise PcgError(f"gumbel noise must be [{T}][{N}][{Tc}]" + (f" or [{N}][{Tc}]" if T == 1 else "") + f", got {tuple(gumbel.shape)}")
    return gumbel.detach().to(torch.float32)


def _cf_launch(generator, classifier, x, config, T, group, outputs, noise, mask, mask_rows, target=None, y=None, clamp_cls=False,
               tile_sums=False, class_sums=False):
    """ONE pcg_house_cf_eval launch.  x [N][17], noise [T][N][Tcat], mask [17] / [N][17], target / y [N] int64: contiguous tensors on
    the nets' device.  Returns the asked per-row outputs ([T][N]...; logits_x / pred_x [N]...) and the asked sums."""
    import ctypes
    from ._lib import HouseCfEvalArgs, load as _lib_load
    dev, N = x.device, x.shape[0]
    generator._ensure_flat()
    a = HouseCfEvalArgs()
    a.N, a.T, a.group, a.clamp_cls, a.mask_rows = N, T, int(group), int(bool(clamp_cls)), int(bool(mask_rows))
    a.g_flat, a.nG = generator._flat.data_ptr(), generator._flat.numel()
    for k, blk in enumerate(generator.blocks):
        for j, bn in ((2 * k, blk.bn1), (2 * k + 1, blk.bn2)):
            a.bn_mean[j] = ops._chk(bn.running_mean, "running_mean").data_ptr()
            a.bn_var[j] = ops._chk(bn.running_var, "running_var").data_ptr()
    tau = config.get("gumbel_tau", None)                                       # eval_utils.py:76-77
    a.bn_eps, a.tau, a.res_scale = generator.blocks[0].bn1.eps, generator.tau if tau is None else float(tau), generator.residual_scaling
    for f, v in enumerate(generator.col_src()):
        a.col_src[f] = v
    norm_vals = cat_norm_maps(generator, config, dev)                          # :56-67
    if norm_vals.numel() != generator.total_cat:
        raise PcgError(f"config['categorical_info'] lists {norm_vals.numel()} category values, the generator's heads have {generator.total_cat}")
    biases = [b for _, b in classifier._pack()]
    wk, bk = ops._ptr_array(classifier._pack_kmajor()), ops._ptr_array(biases)
    a.norm_vals, a.c_w_kmajor, a.c_bias = norm_vals.data_ptr(), wk, bk
    a.x, a.mask, a.noise = ops._chk(x, "x").data_ptr(), ops._chk(mask, "mask").data_ptr(), ops._chk(noise, "gumbel noise").data_ptr()
    if target is not None:
        a.target = ops._chk(target, "target", torch.int64).data_ptr()
    if y is not None:
        a.y = ops._chk(y, "y", torch.int64).data_ptr()
    shape = {"cont": (len(generator.continuous_idx),), "logits": (generator.total_cat,), "chosen": (len(generator.cat_idx),),
             "masked_residual": (17,), "x_cf": (17,), "x_cf_raw": (17,), "logits_cf": (4,), "logits_x": (4,), "pred_cf": (), "pred_x": (), "gain": ()}
    out = {}
    for name in outputs:
        lead = (N,) if name in ("logits_x", "pred_x") else (T, N)
        dt = torch.int32 if name == "chosen" else (torch.int64 if name.startswith("pred") else torch.float32)
        out[name] = torch.empty(lead + shape[name], dtype=dt, device=dev)
        setattr(a, _CF_FIELD.get(name, name), out[name].data_ptr())
    n_tiles = -(-N // int(group)) * -(-min(int(group), N) // CF_TILE_ROWS)
    if tile_sums:
        out["tile_sums"] = torch.empty((T, n_tiles, 4), dtype=torch.float32, device=dev)
        a.tile_sums = out["tile_sums"].data_ptr()
    if class_sums:
        out["class_sums"] = torch.empty((T, n_tiles, 4, 17), dtype=torch.float32, device=dev)
        out["class_counts"] = torch.empty((T, n_tiles, 4), dtype=torch.float32, device=dev)
        a.class_sums, a.class_counts = out["class_sums"].data_ptr(), out["class_counts"].data_ptr()
    ops.check(_lib_load().pcg_house_cf_eval(ctypes.byref(generator._fused_desc()), ctypes.byref(a), ops._stream()), "pcg_house_cf_eval")
    return out


def _cf_draw(generator, rng, shape, dev):
    """The Gumbel noise of a call that was given none: ONE DeviceRNG.gumbel launch (rng, else generator.rng, else a fresh seed-0 one)."""
    if rng is None:
        if generator.rng is None:
            generator.rng = ops.DeviceRNG(seed=0)
        rng = generator.rng
    return rng.gumbel(shape, dev)


def _cf_group(batch_size, config):
    group = int(config.get("batch_size", 128) if batch_size is None else batch_size)
    if not 1 <= group < 2 ** 31:
        raise PcgError(f"batch_size must be a positive 32-bit integer, got {group}")
    return group


def counterfactuals(generator, classifier, x, target, config, mask=None, gumbel=None, rng=None):
    """gradio_app.py:144-169 for N rows at once — this house, that price class, only these features may move: x [N][17] (a tensor
    or an ndarray), target an int or [N] integers in [0, 4), mask None (prompt_mask(config): everything but the immutable columns),
    [17] or [N][17] (one prompt per row).  The classifier sees the clamped counterfactual, as the app's query does (:163-169).
    gumbel: the hard Gumbel-softmax noise [N][Tcat] (or a dict idx -> [N][n]); None: one draw from rng / generator.rng.  Both nets
    must be in eval mode.  ONE launch.  Returns a dict of device tensors, the names of CF_ROW_OUTPUTS, leading dimension N."""
    _cf_nets(generator, classifier)
    x = _cfeval.rows_arg(x, 17, floats_only=True, detach=True)[0]
    N = x.shape[0]
    target = _cfeval.targets_arg(target, N, generator.num_classes, refuse_bool=True)
    mask, mask_rows = _cf_mask(mask, config, N)
    noise = _cf_given_noise(generator, gumbel, 1, N)
    dev = _cfeval.one_gpu(generator, classifier, who="house evaluation")
    with torch.no_grad():
        if noise is None:
            noise = _cf_draw(generator, rng, (1, N, generator.total_cat), dev)
        out = _cf_launch(generator, classifier, upload(x, dev), config, 1, CF_QUERY_GROUP, CF_ROW_OUTPUTS, upload(noise, dev),
                         upload(mask, dev), mask_rows, target=upload(target, dev, torch.int64), clamp_cls=True)
    return {k: (v if k in ("logits_x", "pred_x") else v[0]) for k, v in out.items()}


def counterfactual_sweep(generator, classifier, X, y=None, config=CONFIG, mask=None, batch_size=None, gumbel=None, rng=None, outputs=(),
                         clamp_cls=False, class_sums=False):
    """Every target class x every row in ONE launch: the loops of eval_utils.py:219-267 with the row selection (:226) folded into
    the sums.  y [N] or None (every row counts); mask as in `counterfactuals`; batch_size: the loader's (default
    config['batch_size']); gumbel [4][N][Tcat] or None (one draw); clamp_cls False: the classifier sees x + masked_residual as the
    metrics do (:245).  Returns {"tile_sums": [4][n_tiles][4] (included rows, rows with pred_cf == target, sum of gain, sum of
    |masked_residual| over the 17 columns; metrics_from_sums folds them), with class_sums=True also "class_sums" [4][n_tiles][4][17]
    and "class_counts" [4][n_tiles][4] (per source class; needs y), and the per-row `outputs` asked for ([4][N]...; logits_x,
    pred_x [N]...)} as device tensors."""
    _cf_nets(generator, classifier)
    X = _cfeval.rows_arg(X, 17, "X", floats_only=True, detach=True)[0]
    N, T = X.shape[0], generator.num_classes
    group = _cf_group(batch_size, config)
    _cfeval.check_outputs(outputs, CF_ROW_OUTPUTS)
    y = _cfeval.labels_arg(y, N)
    if y is None and class_sums:
        raise PcgError("class_sums splits the rows by their class: y is required")
    mask, mask_rows = _cf_mask(mask, config, N)
    noise = _cf_given_noise(generator, gumbel, T, N)
    dev = _cfeval.one_gpu(generator, classifier, who="house evaluation")
    with torch.no_grad():
        if noise is None:
            noise = _cf_draw(generator, rng, (T, N, generator.total_cat), dev)
        return _cf_launch(generator, classifier, upload(X, dev), config, T, group, tuple(outputs), upload(noise, dev), upload(mask, dev),
                          mask_rows, y=None if y is None else upload(y, dev, torch.int64), clamp_cls=clamp_cls, tile_sums=True,
                          class_sums=class_sums)


def fold_tiles(sums, group):
    """Pure host.  sums [T][n_tiles]... -> [T][n_groups]... in float64: the tiles of each group added in ascending order.  A group
    has ceil(group / 16) tiles; fewer tiles than that in all means the rows did not fill one group."""
    s = np.asarray(sums, dtype=np.float64)
    group = int(group)
    if s.ndim < 2 or group < 1:
        raise PcgError(f"fold_tiles: sums must be [T][n_tiles]... and group positive, got {s.shape}, {group}")
    tpg = -(-group // CF_TILE_ROWS)
    n_tiles = s.shape[1]
    if n_tiles <= tpg:
        tpg = max(n_tiles, 1)
    elif n_tiles % tpg:
        raise PcgError(f"fold_tiles: {n_tiles} tiles are no whole number of groups of {group} rows ({tpg} tiles each)")
    out = np.zeros((s.shape[0], n_tiles // tpg) + s.shape[2:])
    for j in range(tpg):                                                       # ascending tile order inside every group
        out += s[:, j::tpg][:, :out.shape[1]]
    return out


def metrics_from_sums(tile_sums, group):
    """Pure host.  tile_sums [T][n_tiles][4] of pcg_house_cf_eval -> [T][3] (METRIC_FIELDS) as eval_utils.py:253-278 forms them:
    per group with a row in it the mean over its rows (actionability over all 17 columns: / (17 count)), then the mean over those
    groups — the mean of the per-batch means.  A target without such a group: nan."""
    g = fold_tiles(tile_sums, group)
    if g.ndim != 3 or g.shape[2] != 4:
        raise PcgError(f"metrics_from_sums: tile_sums must be [T][n_tiles][4], got {np.shape(tile_sums)}")
    return _cfeval.batch_mean_metrics(g, 17)


def _metrics_one_launch(generator, classifier, X, y, config, gumbel_per_call, rng, max_vis):
    """compute_metrics_per_target(one_launch=True): the chain's (target, batch) calls become rows of one sweep.  Call (t, batch) of
    the chain selects the batch's rows with y != t in ascending order, and the calls of a target come in ascending batch order, so
    their noise tensors, concatenated, are the noise of the included rows of slot t in ascending row order."""
    X_t, y_np = torch.as_tensor(np.asarray(X), dtype=torch.float32), np.asarray(y)
    num_classes = int(np.unique(y_np).size)
    generator.eval(); classifier.eval()
    _cf_nets(generator, classifier)
    X_t = _cfeval.rows_arg(X_t, 17, "X", floats_only=True, detach=True)[0]
    N, Tc = X_t.shape[0], generator.total_cat
    if y_np.shape != (N,) or num_classes != generator.num_classes or y_np.min() < 0 or y_np.max() >= num_classes:
        raise PcgError(f"y must be [N] labels covering the generator's {generator.num_classes} classes, got shape {y_np.shape}, "
                       f"{num_classes} distinct values")
    bs = _cf_group(None, config)
    dev = _cfeval.one_gpu(generator, classifier, who="house evaluation")
    if gumbel_per_call is None and generator.rng is None:
        generator.rng = rng if rng is not None else ops.DeviceRNG(seed=0)
    noise_it = iter(gumbel_per_call) if gumbel_per_call is not None else None
    vis, seen = [], 0
    with torch.no_grad():
        noise = ops.fill(torch.empty((num_classes, N, Tc), dtype=torch.float32, device=dev), 0.0)   # excluded rows: not read back
        for t in range(num_classes):
            rows_t, parts = np.nonzero(y_np != t)[0], []
            stage = torch.empty((len(rows_t), Tc), dtype=torch.float32, device=dev) if noise_it is None else None
            done = 0
            for i in range(0, N, bs):
                n_sel = int((y_np[i:i + bs] != t).sum())
                if n_sel == 0:
                    continue
                if noise_it is not None:
                    part = next(noise_it)
                    part = generator.pack_noise(part) if isinstance(part, dict) else part
                    if tuple(part.shape) != (n_sel, Tc):
                        raise PcgError(f"gumbel noise of call (target {t}, rows {i}..) must be [{n_sel}, {Tc}], got {tuple(part.shape)}")
                    parts.append(part.to(dev, torch.float32))
                else:
                    generator.rng.gumbel(None, dev, out=stage[done:done + n_sel])   # the chain's draw of this call
                if seen < max_vis:                                             # :270-272 (whole calls, while under max_vis)
                    vis.append(t * N + rows_t[done:done + n_sel])
                    seen += n_sel
                done += n_sel
            if len(rows_t):
                noise[t].index_copy_(0, torch.from_numpy(rows_t).to(dev), torch.cat(parts) if noise_it is not None else stage)
        res = _cf_launch(generator, classifier, upload(X_t, dev), config, num_classes, bs, ("x_cf_raw",), noise,
                         torch.from_numpy(prompt_mask(config)).to(dev), False, y=torch.from_numpy(y_np.astype(np.int64)).to(dev),
                         tile_sums=True)
        table = metrics_from_sums(res["tile_sums"].cpu().numpy(), bs)          # the one read of the sums
        if vis:
            idx = np.concatenate(vis)
            cfs = res["x_cf_raw"].view(num_classes * N, 17).index_select(0, torch.from_numpy(idx).to(dev)).cpu().numpy()
            originals = X_t[torch.from_numpy(idx % N)].numpy()
        else:
            originals, cfs = np.empty((0, X_t.shape[1])), np.empty((0, X_t.shape[1]))
    return metric_rows(table), originals, cfs


def analyze_class_pair_sensitivity(G, clf, X, y, config, gumbel=None, rng=None):
    """eval_utils.py:351-434 — deltas [NC][NC][17]: for every source class s and target t != s the mean |masked residual| per
    feature over the rows of class s (diagonal and absent classes: 0), from ONE sweep launch (the reference makes NC (NC - 1)
    generator passes).  gumbel: [NC][N][Tcat] — the noise of pass (s, t) at the rows of class s in slot t — or None (one draw).
    The heat maps are plotting: left out."""
    G.eval(); clf.eval()
    y_np = np.asarray(y.detach().cpu() if torch.is_tensor(y) else y)
    N = len(y_np)
    res = counterfactual_sweep(G, clf, X, y_np, config, batch_size=max(N, 1), gumbel=gumbel, rng=rng, class_sums=True)
    sums = fold_tiles(res["class_sums"].cpu().numpy(), N)[:, 0]                # [t][s][17]
    counts = fold_tiles(res["class_counts"].cpu().numpy(), N)[:, 0]            # [t][s]
    NC = sums.shape[0]
    deltas = np.zeros((NC, NC, sums.shape[2]), dtype=float)
    for s_ in range(NC):
        for t in range(NC):
            if s_ != t and counts[t, s_] > 0:
                deltas[s_, t] = sums[t, s_] / counts[t, s_]
    return deltas


def analyze_feature_shift_importance(X_orig, X_cf, feature_names, scaler=None):
    """eval_utils.py:292-324 — the table of the global feature-shift plot as a list of dicts, sorted by mean_abs_change_norm
    descending (ties keep the feature order): feature, mean_abs_change_norm = mean |X_cf - X_orig| per feature,
    mean_pct_of_range = 100 x that, and with a scaler mean_abs_change_denorm = that x (data_max_ - data_min_) of the row's own
    feature (the reference assigns this column after the sort, in unsorted order: not repeated here).  Empty inputs: the
    reference's zero table (:305-307)."""
    X_orig, X_cf, names = np.asarray(X_orig), np.asarray(X_cf), list(feature_names)
    if X_orig.size == 0 or X_cf.size == 0:
        return [{"feature": f, "mean_abs_change_norm": 0.0} for f in names]
    if X_orig.shape != X_cf.shape or X_orig.ndim != 2 or X_orig.shape[1] != len(names):
        raise PcgError(f"analyze_feature_shift_importance: X_orig {X_orig.shape} and X_cf {X_cf.shape} must be [n][{len(names)}]")
    delta = np.mean(np.abs(X_cf - X_orig), axis=0)                             # :309
    rng_ = None
    if scaler is not None and hasattr(scaler, "data_min_") and hasattr(scaler, "data_max_"):
        rng_ = (np.asarray(scaler.data_max_) - np.asarray(scaler.data_min_)).astype(float)   # :319
    rows = []
    for i in np.argsort(-delta, kind="stable"):                                # :314
        row = {"feature": names[i], "mean_abs_change_norm": float(delta[i]), "mean_pct_of_range": float(delta[i] * 100.0)}
        if rng_ is not None:
            row["mean_abs_change_denorm"] = float(delta[i] * rng_[i])
        rows.append(row)
    return rows


SAMPLE_FIELDS = ("sample_idx_in_vis", "source_pred", "intended_target", "cf_pred", "success", "prediction_gain", "num_changed",
                 "frac_changed", "sparsity", "L1_sum_norm", "L1_mean_norm", "L2_norm", "topk_features", "topk_vals_pct_of_range")
AGGREGATE_FIELDS = ("n_samples_used", "class_flip_rate", "mean_prediction_gain", "median_prediction_gain", "mean_L1_sum_norm", "mean_L2_norm",
                    "mean_num_changed", "mean_frac_changed", "mean_sparsity", "topk_features_global", "topk_features_global_mean_pct")


def case_study_rows(N, n_samples=20, random_seed=42):
    """The rows generate_case_study_report_from_vis draws (eval_utils.py:528-530): the same call, so the same rows."""
    n = min(int(n_samples), int(N))
    return np.random.default_rng(random_seed).choice(np.arange(int(N)), size=n, replace=False)


def case_study_tables(probs_orig, probs_cf, originals, cfs, feature_names, scaler=None, n_samples=20, eps=1e-3, random_seed=42,
                      top_k_features=5):
    """eval_utils.py:525-660 on the host, NumPy only, the reference's own expressions on the arrays' own dtypes.  probs_orig, probs_cf
    [n][NC]: the classifier's probabilities of the CHOSEN rows (case_study_rows) of originals / cfs [N][d].  Returns
    (sample_rows, feature_rows, aggregate, per_sample_feature_tables) as lists of dicts (aggregate: one dict): the rows of
    case_study_sample_summary.csv (SAMPLE_FIELDS), of case_study_feature_summary.csv sorted by mean_abs_delta_norm descending, the
    aggregate (AGGREGATE_FIELDS), and per chosen row {"sample_idx", "source_pred", "intended_target", "rows"}.
    Two departures from the reference, both on purpose: the feature summary's mean_abs_delta_denorm is each row's own feature's value
    (the reference assigns the column after sort_values, in unsorted order, :636-638), and both sorts are stable."""
    originals, cfs, names = np.asarray(originals), np.asarray(cfs), list(feature_names)
    if originals.ndim != 2 or originals.shape != cfs.shape or originals.shape[0] < 1 or originals.shape[1] != len(names):
        raise PcgError(f"case_study_tables: originals {originals.shape} and cfs {cfs.shape} must be [N][{len(names)}] with N >= 1")
    N, d = originals.shape
    idxs = case_study_rows(N, n_samples, random_seed)                                                              # :528-530
    n = len(idxs)
    probs_orig, probs_cf = np.asarray(probs_orig), np.asarray(probs_cf)
    if probs_orig.ndim != 2 or probs_orig.shape != probs_cf.shape or probs_orig.shape[0] != n:
        raise PcgError(f"case_study_tables: probs_orig {probs_orig.shape} and probs_cf {probs_cf.shape} must be [{n}][classes]: the chosen rows'")
    preds_orig, preds_cf = np.argmax(probs_orig, axis=1), np.argmax(probs_cf, axis=1)                              # :544-545
    intended = np.argmax(probs_cf - probs_orig, axis=1)                                                            # :548-549
    abs_diff = np.abs(cfs[idxs] - originals[idxs])                                                                 # :551
    num_changed = (abs_diff > eps).sum(axis=1)
    frac_changed = num_changed / float(d)
    sparsity = 1.0 - frac_changed
    L1_sum, L1_mean, L2 = np.sum(abs_diff, axis=1), np.mean(abs_diff, axis=1), np.linalg.norm(abs_diff, axis=1)    # :555-557
    gain = probs_cf[np.arange(n), intended] - probs_orig[np.arange(n), intended]                                   # :559
    success = (preds_cf == intended).astype(int)
    orig_dn = cf_dn = abs_dn = frange = None
    if scaler is not None:                                                                                         # :564-572
        try:
            orig_dn, cf_dn = scaler.inverse_transform(originals[idxs]), scaler.inverse_transform(cfs[idxs])
            abs_dn = np.abs(cf_dn - orig_dn)
            if hasattr(scaler, "data_max_") and hasattr(scaler, "data_min_"):
                frange = (np.asarray(scaler.data_max_) - np.asarray(scaler.data_min_)).astype(float)
        except Exception:
            orig_dn = cf_dn = abs_dn = frange = None
    sample_rows, per_sample = [], []
    for i, g in enumerate(idxs):                                                                                   # :575-620
        topk = np.argsort(-abs_diff[i], kind="stable")[:top_k_features]                                            # :597
        sample_rows.append({
            "sample_idx_in_vis": int(g), "source_pred": int(preds_orig[i]), "intended_target": int(intended[i]), "cf_pred": int(preds_cf[i]),
            "success": int(success[i]), "prediction_gain": float(gain[i]), "num_changed": int(num_changed[i]),
            "frac_changed": float(frac_changed[i]), "sparsity": float(sparsity[i]), "L1_sum_norm": float(L1_sum[i]),
            "L1_mean_norm": float(L1_mean[i]), "L2_norm": float(L2[i]), "topk_features": ";".join(names[j] for j in topk),
            "topk_vals_pct_of_range": ";".join(map(str, (abs_diff[i, topk] * 100.0).round(6).tolist()))})           # :599-601
        cols = {"orig_norm": originals[g], "cf_norm": cfs[g], "abs_delta_norm": abs_diff[i], "pct_of_range": abs_diff[i] * 100.0}   # :604-610
        if orig_dn is not None:
            cols.update(orig_denorm=orig_dn[i], cf_denorm=cf_dn[i], abs_delta_denorm=abs_dn[i])
            if frange is not None:
                cols["pct_of_range_denorm"] = (abs_dn[i] / (frange + 1e-12)) * 100.0                               # :616
        rows = [dict({"feature": names[j]}, **{k: float(v[j]) for k, v in cols.items()}) for j in range(d)]
        per_sample.append({"sample_idx": int(g), "source_pred": int(preds_orig[i]), "intended_target": int(intended[i]), "rows": rows})
    mean_abs = abs_diff.mean(axis=0)                                                                               # :625-627
    change_freq = (abs_diff > eps).mean(axis=0)
    mean_abs_dn = abs_dn.mean(axis=0) if abs_dn is not None else None
    feature_rows = []
    for j in np.argsort(-mean_abs, kind="stable"):                                                                 # :634
        row = {"feature": names[j], "mean_abs_delta_norm": float(mean_abs[j]), "mean_pct_of_range": float(mean_abs[j] * 100.0),
               "change_freq": float(change_freq[j])}
        if mean_abs_dn is not None:
            row["mean_abs_delta_denorm"] = float(mean_abs_dn[j])
        feature_rows.append(row)
    col = lambda k: np.asarray([r[k] for r in sample_rows], dtype=np.float64)     # noqa: E731
    aggregate = {"n_samples_used": int(n), "class_flip_rate": float(col("success").mean()),                        # :644-654
                 "mean_prediction_gain": float(col("prediction_gain").mean()), "median_prediction_gain": float(np.median(col("prediction_gain"))),
                 "mean_L1_sum_norm": float(col("L1_sum_norm").mean()), "mean_L2_norm": float(col("L2_norm").mean()),
                 "mean_num_changed": float(col("num_changed").mean()), "mean_frac_changed": float(col("frac_changed").mean()),
                 "mean_sparsity": float(col("sparsity").mean())}
    top = np.argsort(-mean_abs, kind="stable")[:top_k_features]                                                    # :657-659
    aggregate["topk_features_global"] = ",".join(names[j] for j in top)
    aggregate["topk_features_global_mean_pct"] = ",".join(f"{(mean_abs[j] * 100.0):.3f}" for j in top)
    return sample_rows, feature_rows, aggregate, per_sample


def _csv_quote(v):
    return '"' + v.replace('"', '""') + '"' if isinstance(v, str) and any(c in v for c in ',"\n') else v


def case_studies(classifier, originals, cfs, config, scaler=None, n_samples=20, eps=1e-3, random_seed=42, top_k_features=5, save_dir=None):
    """generate_case_study_report_from_vis (eval_utils.py:496-664): the chosen rows' probabilities from ONE fused classifier launch
    (originals and counterfactuals stacked, the softmax of the 2n x NC logits on the host in fp32), then case_study_tables.  With
    save_dir the reference's tree: case_study_sample_summary.csv, case_study_feature_summary.csv, case_study_aggregate_summary.csv and
    samples/src{S}_tgt{T}/sample_{i}_features.csv.  Returns what case_study_tables returns."""
    import os
    originals, cfs = np.asarray(originals), np.asarray(cfs)
    if originals.ndim != 2 or originals.shape != cfs.shape or originals.shape[0] < 1:
        raise PcgError(f"case_studies: originals {originals.shape} and cfs {cfs.shape} must be the same [N][d] with N >= 1")
    names = config.get("feature_names", [f"feat_{i}" for i in range(originals.shape[1])])
    idxs = case_study_rows(originals.shape[0], n_samples, random_seed)
    n = len(idxs)
    classifier.eval()
    dev = next(classifier.parameters()).device
    with torch.no_grad():
        both = np.concatenate([originals[idxs], cfs[idxs]], axis=0)
        logits = classifier(torch.as_tensor(both, dtype=torch.float32).to(dev).contiguous()).cpu().numpy().astype(np.float32)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))                                                         # :542-543
    probs = e / e.sum(axis=1, keepdims=True)
    tables = case_study_tables(probs[:n], probs[n:], originals, cfs, names, scaler=scaler, n_samples=n_samples, eps=eps,
                               random_seed=random_seed, top_k_features=top_k_features)
    if save_dir:
        sample_rows, feature_rows, aggregate, per_sample = tables
        quoted = lambda rows: [{k: _csv_quote(v) for k, v in r.items()} for r in rows]     # noqa: E731
        save_table(quoted(sample_rows), os.path.join(save_dir, "case_study_sample_summary.csv"), SAMPLE_FIELDS)
        save_table(quoted(feature_rows), os.path.join(save_dir, "case_study_feature_summary.csv"), tuple(feature_rows[0].keys()))
        save_table(quoted([aggregate]), os.path.join(save_dir, "case_study_aggregate_summary.csv"), AGGREGATE_FIELDS)
        for s in per_sample:
            path = os.path.join(save_dir, "samples", f"src{s['source_pred']}_tgt{s['intended_target']}", f"sample_{s['sample_idx']}_features.csv")
            save_table(quoted(s["rows"]), path, tuple(s["rows"][0].keys()))
        print(f"[case_study] Saved {n} per-sample CSVs (grouped by src->tgt), sample_summary, feature_summary and aggregate to {save_dir}")
    return tables


_case_studies = case_studies      # evaluate_pipeline's keyword has the function's name


def weighted_scores(cm):
    """Pure host.  accuracy and sklearn's precision / recall / f1 with average='weighted', zero_division=0, from a confusion matrix
    (rows true, columns predicted): per class tp / column sum, tp / row sum and their harmonic mean (0 where a denominator is 0),
    weighted by the class's support (its row sum)."""
    cm = np.asarray(cm, dtype=np.float64)
    tp, support, predicted = np.diag(cm), cm.sum(1), cm.sum(0)
    total = support.sum()
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or total <= 0:
        raise PcgError(f"weighted_scores: a square confusion matrix with at least one sample is required, got {cm.shape}")
    prec = np.divide(tp, predicted, out=np.zeros_like(tp), where=predicted > 0)
    rec = np.divide(tp, support, out=np.zeros_like(tp), where=support > 0)
    f1 = np.divide(2 * prec * rec, prec + rec, out=np.zeros_like(tp), where=(prec + rec) > 0)
    w = support / total
    return {"accuracy": float(tp.sum() / total), "precision": float((w * prec).sum()), "recall": float((w * rec).sum()),
            "f1": float((w * f1).sum()), "per_class": {"precision": prec, "recall": rec, "f1": f1, "support": support.astype(np.int64)}}


def evaluate_classifier(classifier, X_test, y_test, class_names=None):
    """eval_utils.py:436-493 — accuracy, weighted precision / recall / F1 (zero_division=0), the confusion matrix and a text report
    of the per-class scores; one fused classifier launch, the scores on the host without scikit-learn.  The confusion-matrix
    picture is plotting: left out."""
    classifier.eval()
    dev = next(classifier.parameters()).device
    with torch.no_grad():
        logits = classifier(torch.as_tensor(np.asarray(X_test), dtype=torch.float32).to(dev).contiguous())
        preds = logits.argmax(1).cpu().numpy()                                # :455
    y_true = np.asarray(y_test, dtype=int)
    cm = confusion_matrix(y_true, preds)
    sc = weighted_scores(cm)
    labels = np.unique(np.concatenate([y_true, preds]))
    names = [str(n) for n in class_names] if class_names is not None else [str(v) for v in labels]
    pc = sc.pop("per_class")
    lines = [f"{'':>12} {'precision':>9} {'recall':>9} {'f1-score':>9} {'support':>9}"]
    lines += [f"{names[i] if i < len(names) else labels[i]:>12} {pc['precision'][i]:9.4f} {pc['recall'][i]:9.4f} {pc['f1'][i]:9.4f} {pc['support'][i]:9d}"
              for i in range(len(labels))]
    lines.append(f"{'weighted avg':>12} {sc['precision']:9.4f} {sc['recall']:9.4f} {sc['f1']:9.4f} {int(pc['support'].sum()):9d}")
    return dict(sc, confusion_matrix=cm, report="\n".join(lines) + "\n")


def evaluate_pipeline(generator, classifier, X_test, y_test, config, case_studies=False):
    """eval_utils.py:673-728 — compute_metrics_per_target on the one-launch path -> <out_dir>/countergan_metrics.csv (the
    reference's layout); the feature-shift table -> feature_shift_importance.csv and the class-pair sensitivity array ->
    class_pair_sensitivity/deltas.npy, where the reference saves their pictures.  case_studies=True: also the case-study tables of
    :711-719 under <out_dir>/case_studies (case_studies(), config["case_study_n"] rows, 20 by default).  Figure rendering and t-SNE
    stay out.  Returns the metric rows."""
    import os
    out = config.get("out_dir", ".")
    os.makedirs(out, exist_ok=True)
    print("[pipeline] Computing per-target CounterGAN metrics ...")
    rows, originals, cfs = compute_metrics_per_target(generator, classifier, X_test, y_test, config, one_launch=True)   # :687
    save_table(rows, os.path.join(out, "countergan_metrics.csv"), ("target_class",) + METRIC_FIELDS)                     # :688
    print(f"[metrics] Saved metrics to {os.path.join(out, 'countergan_metrics.csv')}")
    names = config.get("feature_names", [f"feat_{i}" for i in range(np.asarray(X_test).shape[1])])
    shift = analyze_feature_shift_importance(originals, cfs, names, scaler=config.get("scaler", None))                   # :691-697
    save_table(shift, os.path.join(out, "feature_shift_importance.csv"), tuple(shift[0].keys()) if shift else ("feature",))
    deltas = analyze_class_pair_sensitivity(generator, classifier, X_test, y_test, config)                               # :700-708
    os.makedirs(os.path.join(out, "class_pair_sensitivity"), exist_ok=True)
    np.save(os.path.join(out, "class_pair_sensitivity", "deltas.npy"), deltas)
    if case_studies:                                                                                                     # :711-719
        _case_studies(classifier, originals, cfs, config, scaler=config.get("scaler", None), n_samples=config.get("case_study_n", 20),
                      save_dir=os.path.join(out, "case_studies"))
    return rows


class GraphedTrainStep:
    """The whole training step — G forward, critic step, G step, both Adam updates: ~400 kernels as an op chain, 36 as scheduled by
    train_step(branch=...) — captured once in a HIP graph and replayed with one host call: this path is latency bound (SURVEY.md
    section 8a row a15), and the graph removes the per-kernel host cost.  overlap="inline" (default): the scheduled step on one
    stream; True: the frozen classifier's term on a parallel graph branch (a graph with branches is launched node by node by the
    host, a chain is not: 0.28 vs 0.03 ms of host time per replay; wall 0.434 vs 0.422 ms at batch 4096 once the classifier term
    itself was down to 47 us); False: the reference-order autograd step.  All bit-identical; any other value is refused.
    Inputs live in static device buffers (`x, y, target_y, mask, noise`): write the next batch into them (`load(...)`, or draw
    straight into them) and call `replay()`; outputs are the static tensors in `out`.
    Capture needs warm-up executions of real steps; the parameters, buffers and optimizer state are snapshotted before and
    restored after, so constructing this object does not advance training."""

    def __init__(self, generator, discriminator, classifier, opt_g, opt_d, norm_vals, batch, config=CONFIG, warmup=3, overlap="inline",
                 rng=None, dataset=None, diag=None, with_critic_wgrad_variant=False):
        """with_critic_wgrad_variant: also capture the step WITH the critic weight gradients of the generator step
        (skip_dead_d_wgrad=False: what the reference's autograd computes, :314) as a second graph over the same static buffers —
        `replay(full=True)`; the trainer runs it as the last iteration of an epoch, whose D.grad the epoch summary prints (:362).
        dataset = (X [N, D] float32, Y [N] int64) resident on the device (needs rng): the draws launch also TAKES the batch — rows
        perm[cursor .. cursor + batch) of the epoch's permutation (`new_epoch(perm)` uploads it and rewinds the cursor) — so a replay
        needs no host-side copy (trainer.py:198's DataLoader(shuffle=True, drop_last=True) without collation / PCIe / copy launches).
        diag = {"logits_orig": [N, nc] (dataset mode: gathered through the batch's source rows) or [batch, nc], "acc": float64[8] or
        None, "eps": 1e-3}: the trainer's per-iteration diagnostics + epoch accumulators ride in the step (train_step(diag=...)).
        rng (an ops.DeviceRNG): the per-iteration draws (draw_batch_randoms: target class, feature mask, Gumbel noise, one-hot rows) are
        the first launch of the captured step, their Philox offsets read from a device counter that the launch advances itself — write x
        and y into the static buffers (`load_batch`) and replay(); the numbers are those draw_batch_randoms(rng, ...) would have drawn
        before each eager step, and rng.offset is kept in step on the host."""
        if overlap not in ("inline", True, False):
            raise PcgError(f'GraphedTrainStep: overlap must be "inline", True or False, got {overlap!r}')
        dev = norm_vals.device
        # train_step's parallel branch: the classifier term and the logged sums
        self.branch = "inline" if overlap == "inline" else (torch.cuda.Stream(device=dev) if overlap else None)
        D_in, T = config["input_dim"], generator.total_cat
        self.x = torch.zeros((batch, D_in), dtype=torch.float32, device=dev)
        self.y = torch.zeros((batch,), dtype=torch.int64, device=dev)
        self.target_y = torch.ones((batch,), dtype=torch.int64, device=dev)
        self.mask = torch.ones((batch, D_in), dtype=torch.float32, device=dev)
        self.noise = torch.zeros((batch, T), dtype=torch.float32, device=dev)
        for n in (generator, discriminator):
            n._ensure_flat()

        nc = config["num_classes"]
        # one-hot rows of target_y and y: static inputs of the scheduled step (draw_batch_randoms(onehots=self.onehots) fills them with
        # the draws; load() computes them)
        self.onehots = (torch.zeros((batch, nc), dtype=torch.float32, device=dev), torch.zeros((batch, nc), dtype=torch.float32, device=dev))
        ops.onehot(self.target_y, nc, out=self.onehots[0]); ops.onehot(self.y, nc, out=self.onehots[1])

        self._rng = rng
        self._span = ops.DeviceRNG.house_draws_span(batch, D_in, T)
        self._dataset = dataset
        if dataset is not None and rng is None:
            raise PcgError("GraphedTrainStep(dataset=...) needs rng: the batch is taken by the draws launch")
        self._ctr = rng.device_counter(dev, cursor=dataset is not None) if rng is not None else None
        self.src = self.perm = None
        if dataset is not None:
            X, Y = dataset
            if X.dtype != torch.float32 or Y.dtype != torch.int64 or X.shape[1] != D_in or X.shape[0] != Y.shape[0] or X.shape[0] < batch:
                raise PcgError(f"GraphedTrainStep(dataset=...): need X [N >= {batch}, {D_in}] float32 and Y [N] int64 on the device")
            self.src = torch.zeros((batch,), dtype=torch.int64, device=dev)
            self.perm = torch.arange((X.shape[0] // batch) * batch, dtype=torch.int64, device=dev)      # identity until new_epoch()
            self._imm = torch.tensor(list(config.get("immutable_idx", [])), dtype=torch.int32, device=dev)
        sdiag = None
        if diag is not None:
            sdiag = dict(diag)
            if dataset is not None and diag["logits_orig"].shape[0] != batch:
                sdiag["src_rows"] = self.src
        self._diag = sdiag

        def step(skip_dead=True):
            if dataset is not None:
                rng.house_batch_draws(dataset[0], dataset[1], self.perm, nc, T, self._imm if self._imm.numel() else None,
                                      (self.x, self.y, self.target_y, self.mask, self.noise), self.onehots, self._ctr, src_out=self.src)
            elif rng is not None:
                draw_batch_randoms(rng, generator, self.y, config, dev, out=(self.target_y, self.mask, self.noise),
                                   onehots=self.onehots if self.branch is not None else None, counter=self._ctr)
            return train_step(generator, discriminator, classifier, opt_g, opt_d, self.x, self.y, self.target_y, self.mask, norm_vals,
                              config, gumbel=self.noise, branch=self.branch, onehots=self.onehots if self.branch is not None else None,
                              diag=sdiag, skip_dead_d_wgrad=skip_dead)
        self._nc = nc
        # the warm-up steps draw from the counter (and walk the cursor) and add to the epoch accumulators: held with the nets and Adam
        held = Held((generator, discriminator), (opt_g, opt_d), (self._ctr, sdiag.get("acc") if sdiag is not None else None))
        runs = [(step, max(1, warmup))] + ([(lambda: step(False), 1)] if with_critic_wgrad_variant else [])
        got = capture_steps(runs, held, dev, collect=True)
        (self.graph, self.out), (self.graph_full, self.out_full) = got[0], got[1] if with_critic_wgrad_variant else (None, None)

    def new_epoch(self, perm):
        """dataset mode: upload this epoch's row order (int64, at least steps * batch entries; only whole batches are used —
        drop_last) and rewind the cursor.  Two small copies per EPOCH; the replays in between touch no host memory."""
        if self._dataset is None:
            raise PcgError("new_epoch: this GraphedTrainStep was not built with dataset=...")
        n = self.perm.numel()
        if perm.numel() < n:
            raise PcgError(f"new_epoch: permutation of {perm.numel()} entries, {n} needed")
        self.perm.copy_(perm[:n].to(torch.int64), non_blocking=False)
        self._ctr[2:3].zero_()

    @property
    def steps_per_epoch(self):
        return self.perm.numel() // self.x.shape[0] if self.perm is not None else None

    def load_batch(self, x, y):
        """With rng: the data half of a batch (the draws are made by the replay)."""
        self.x.copy_(x); self.y.copy_(y)

    def load(self, x, y, target_y, mask, noise):
        self.x.copy_(x); self.y.copy_(y); self.target_y.copy_(target_y); self.mask.copy_(mask); self.noise.copy_(noise)
        ops.onehot(self.target_y, self._nc, out=self.onehots[0]); ops.onehot(self.y, self._nc, out=self.onehots[1])

    def replay(self, full=False):
        """full=True: the variant that also computes the generator step's critic weight gradients (with_critic_wgrad_variant)."""
        if full:
            if self.graph_full is None:
                raise PcgError("replay(full=True): build the GraphedTrainStep with with_critic_wgrad_variant=True")
            self.graph_full.replay()
        else:
            self.graph.replay()
        if self._rng is not None:
            self._rng.offset += self._span       # the host-side mirror of the device counter
        return self.out_full if full else self.out


class WeightedCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=class_weights) (trainer.py:55-57)."""

    def __init__(self, weight):
        super().__init__()
        self.register_buffer("weight", weight)

    def forward(self, input, target):
        return _WCEFn.apply(input, target, self.weight)


class _WCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight):
        zc = logits.contiguous()
        ctx.save_for_backward(zc, target, weight)
        loss, _ = ops.cross_entropy_weighted_fwd_bwd(zc, target, weight, need_grad=False)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        z, target, weight = ctx.saved_tensors
        _, dz = ops.cross_entropy_weighted_fwd_bwd(z, target, weight, need_loss=False, grad_out=g.contiguous().view(1))
        return dz, None, None


_fused_fallback_warned = False


def _warn_fused_fallback(why):
    global _fused_fallback_warned
    if not _fused_fallback_warned:
        import warnings
        warnings.warn(f"train_classifier(fused=True): {why}; running the op chain instead", RuntimeWarning, stacklevel=3)
        _fused_fallback_warned = True


class ClassifierFit(BatchWalkFit):
    """The classifier pre-training step (trainer.py:78-91) as whole-batch dense launches (csrc/dense_rows.hip): the batch
    gather with the three Dropout masks, four post-activation forward stages, the logits, the loss head with its tally, four stage
    backwards, five weight gradients -- 16 launches captured once as a single-stream, strictly linear HIP graph -- and AdamW, launched
    eagerly after each replay (its lr is a by-value argument that ReduceLROnPlateau changes).  The training set, the epoch's
    permutation, the saved activations and the tally (sum of loss * rows, correct rows, rows) live on the device; nothing is read
    back inside an epoch.  One graph for the full batch, one for the tail N % batch_size; a tail of one row is refused, as
    BatchNorm1d refuses it.  graph=False: the same entries called eagerly with by-value draws (what the replays must equal).  The walk
    over the epoch, the capture and the tally readers are _graphed.BatchWalkFit's."""

    DIMS = [17, 256, 256, 128, 64, 4]

    @staticmethod
    def unsupported(model, batch_size):
        """None, or why this net / batch cannot take the fused path."""
        dims = [m.in_features for m in model.net if isinstance(m, nn.Linear)] + [model.net[-1].out_features]
        if dims != ClassifierFit.DIMS:
            return f"layer widths {dims} are not {ClassifierFit.DIMS}"
        if batch_size > 128:
            return f"batch size {batch_size} is above the 128 rows one workgroup holds"
        return None

    def __init__(self, model, X_train, y_train, class_weight, batch_size, lr=1e-3, weight_decay=1e-4, rng=None, graph=True):
        from .optim import AdamW
        why = self.unsupported(model, batch_size)
        if why is not None:
            raise PcgError(f"ClassifierFit: {why}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise PcgError(f"ClassifierFit: the model is on {dev}; libpcgan_hip has no CPU path")
        self.model = model
        self.X = torch.as_tensor(np.asarray(X_train), dtype=torch.float32).to(dev).contiguous()
        self.Y = torch.as_tensor(np.asarray(y_train), dtype=torch.int64).to(dev).contiguous()
        super().__init__(self.X.shape[0], batch_size)
        if self.X.dim() != 2 or self.X.shape[1] != self.DIMS[0] or self.Y.shape != (self.N,):
            raise PcgError(f"ClassifierFit: need X [N, {self.DIMS[0]}] and y [N]")
        if self.B < 2 or self.N < 2 or self.tail == 1:
            raise PcgError(f"ClassifierFit: {self.N} rows in batches of {self.B} leave a batch of one row; training-mode BatchNorm1d "
                           "needs more than 1 row per batch")
        self.cw = class_weight.to(dev, torch.float32).contiguous()
        self.rng = rng if rng is not None else ops.DeviceRNG(seed=0)
        model.train()
        model._ensure_flat()
        model.zero_grad()                                     # attaches the .grad views; every step OVERWRITES them (no zero_grad)
        self.optimizer = AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
        self._stages, self._last = model._stages()
        self._slopes = [m.negative_slope for m in model.net if isinstance(m, nn.LeakyReLU)]
        self._start(model, dev, graph)       # AdamW stays outside the graphs, and the warm-up: its state is held all the same

    def _buffers(self, R):
        dev = self.X.device
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)      # noqa: E731
        widths = self.DIMS[1:5]
        return {"x": f32(R, self.DIMS[0]), "y": torch.zeros((R,), dtype=torch.int64, device=dev),
                "m": [f32(R, w) for w in widths[:3]], "a": [f32(R, w) for w in widths], "h": [f32(R, w) for w in widths],
                "mean": [f32(w) for w in widths], "invstd": [f32(w) for w in widths], "d": [f32(R, w) for w in widths],
                "logits": f32(R, self.DIMS[5]), "dl": f32(R, self.DIMS[5]), "loss": f32(1)}

    def _after_step(self):
        self.optimizer.step()                # eagerly after every replay: the lr is a by-value argument

    def _span(self, R):
        return ops.DeviceRNG.house_clf_batch_span(R, self.DIMS[1:4])

    def _launches(self, b, cursor=None):
        """One step without AdamW over the buffer set b; cursor None: offsets and rows from the device counter (the captured form)."""
        st, last = self._stages, self._last
        keeps = [1.0 - p for _, _, p in st if p is not None]
        self.rng.house_clf_batch(self.X, self.Y, self.perm, (b["x"], b["y"]), b["m"], keeps, counter=self._ctr if cursor is None else None,
                                 cursor=cursor or 0)
        self._forward_backward(b)

    def _forward_backward(self, b):
        st, last = self._stages, self._last
        h = b["x"]
        for s, (lin, bn, p) in enumerate(st):
            dbn = ops.DenseBN(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum, True,
                              b["mean"][s], b["invstd"][s])
            ops.dense_rows_fwd_post(h, lin.weight.data, lin.bias.data, dbn, ACT_LRELU, self._slopes[s], mask=b["m"][s] if p is not None else None,
                                    p=p or 0.0, a=b["a"][s], out=b["h"][s])
            h = b["h"][s]
        ops.dense_rows_fwd(h, last.weight.data, last.bias.data, out=b["logits"])
        ops.ce_weighted_tally(b["logits"], b["y"], self.cw, self.tally, dlogits=b["dl"], seg_loss=b["loss"], dbias=last.bias.grad)
        d, upper = b["dl"], last
        for s in range(len(st) - 1, -1, -1):
            lin, bn, p = st[s]
            d = ops.dense_rows_dgrad_post(d, upper.weight.data, b["a"][s], b["mean"][s], b["invstd"][s], bn.weight.data, bn.weight.grad, bn.bias.grad,
                                          ACT_LRELU, self._slopes[s], mask=b["m"][s] if p is not None else None, p=p or 0.0, out=b["d"][s],
                                          db=lin.bias.grad)
            upper = lin
        # the bias gradients came from the epilogues above, which hold complete columns: the weight-gradient launches skip theirs
        ops.dense_rows_wgrad(b["dl"], b["h"][-1], last.weight.grad, None)
        for s in range(len(st) - 1, -1, -1):
            ops.dense_rows_wgrad(b["d"][s], b["x"] if s == 0 else b["h"][s - 1], st[s][0].weight.grad, None)


def train_classifier(X_train_all, X_test, y_train_all, y_test, scaler, config, device=None, verbose=True, fused=False):
    """trainer.py:18-180 without the plotting tail: stratified validation split, class-weighted CrossEntropyLoss, AdamW,
    ReduceLROnPlateau(factor 0.5, patience 4), early stopping on the validation loss; returns the model with its best state.
    fused=True: the batches run through ClassifierFit (one graph replay + one AdamW launch per step, no host read inside an epoch),
    the validation is one eval-mode forward over the whole split and one segmented tally launch, and both tallies are read once per
    epoch; the host logic is the same.  A net of other widths or a batch above 128 rows falls back to the op chain with a warning."""
    import copy
    import numpy as np
    from sklearn.model_selection import train_test_split
    from sklearn.utils.class_weight import compute_class_weight
    from torch.utils.data import DataLoader, TensorDataset
    from .optim import AdamW
    device = torch.device(device if device is not None else config.get("cuda", "cuda:0"))
    seed = config.get("seed", 42)
    torch.manual_seed(seed); np.random.seed(seed)                                             # :20-22
    X_train, X_val, y_train, y_val = train_test_split(X_train_all, y_train_all, test_size=config.get("val_frac", 0.10),
                                                      random_state=seed, stratify=y_train_all)   # :29-31
    num_classes = int(np.unique(y_train_all).size)
    bs = config.get("clf_batch_size", config.get("batch_size", 128))
    mk = lambda X, y: TensorDataset(torch.tensor(X, dtype=torch.float32), torch.tensor(y, dtype=torch.long))  # noqa: E731
    train_loader = DataLoader(mk(X_train, y_train), batch_size=bs, shuffle=True, drop_last=False)
    val_loader = DataLoader(mk(X_val, y_val), batch_size=bs, shuffle=False)
    model = NNClassifier(config["input_dim"], output_dim=num_classes).to(device)              # :50
    cw = compute_class_weight("balanced", classes=np.arange(num_classes), y=y_train)          # :53
    criterion = WeightedCrossEntropyLoss(torch.tensor(cw, dtype=torch.float32, device=device))
    fit = None
    if fused:
        why = ClassifierFit.unsupported(model, bs)
        if why is None:
            if model.rng is None:
                model.rng = ops.DeviceRNG(seed=0)                                             # the stream NNClassifier.forward draws from
            fit = ClassifierFit(model, X_train, y_train, criterion.weight, bs, lr=config.get("clf_lr", 1e-3),
                                weight_decay=config.get("clf_wd", 1e-4), rng=model.rng)
            X_val_dev = torch.tensor(X_val, dtype=torch.float32).to(device).contiguous()
            y_val_dev = torch.tensor(y_val, dtype=torch.long).to(device)
        else:
            _warn_fused_fallback(why)
    optimizer = fit.optimizer if fit is not None else \
        AdamW(model.parameters(), lr=config.get("clf_lr", 1e-3), weight_decay=config.get("clf_wd", 1e-4))           # :58
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=4)           # :59
    best_val, best_state, wait = float("inf"), None, 0
    patience, epochs = config.get("clf_early_stopping", 15), config.get("clf_epochs", 100)
    history = []
    for epoch in range(1, epochs + 1):
        model.train()
        run_loss, correct, total = 0.0, 0.0, 0
        for xb, yb in (train_loader if fit is None else ()):
            xb, yb = xb.to(device), yb.to(device)
            optimizer.zero_grad()
            logits = model(xb)
            loss = criterion(logits, yb)
            loss.backward()
            optimizer.step()
            n = xb.size(0)
            run_loss += loss.item() * n
            correct += ops.cf_metrics(logits.detach().contiguous(), yb, other=yb)[0].item() * n
            total += n
        model.eval()
        v_loss, v_correct, v_total = 0.0, 0.0, 0
        if fit is not None:
            fit.epoch(epoch_permutation(fit.N))                                               # the order train_loader walks
        with torch.no_grad():
            if fit is not None:
                model._packed = None             # the in-place optimizer kernel bumps no tensor version: _pack would serve the old image
                torch.empty((), dtype=torch.int64).random_()                                  # val_loader's iterator: its base seed
                ops.ce_weighted_tally(model(X_val_dev).contiguous(), y_val_dev, criterion.weight, fit.val_tally, seg=bs)
                run_loss, correct, total, v_loss, v_correct, v_total = fit.read_tallies()     # the epoch's one host read
            for xb, yb in (val_loader if fit is None else ()):
                xb, yb = xb.to(device), yb.to(device)
                logits = model(xb).contiguous()
                n = xb.size(0)
                v_loss += ops.cross_entropy_weighted_fwd_bwd(logits, yb, criterion.weight, need_grad=False)[0].item() * n
                v_correct += ops.cf_metrics(logits, yb, other=yb)[0].item() * n
                v_total += n
        val_loss = v_loss / v_total
        scheduler.step(val_loss)                                                              # :128
        history.append((run_loss / total, correct / total, val_loss, v_correct / v_total))
        if val_loss < best_val - 1e-6:                                                        # :129-139
            best_val, wait = val_loss, 0
            best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        else:
            wait += 1
        if verbose:
            print(f"[Epoch {epoch}/{epochs}] train_loss={history[-1][0]:.4f}, train_acc={history[-1][1]:.4f} | "
                  f"val_loss={val_loss:.4f}, val_acc={history[-1][3]:.4f} | wait={wait}")
        if wait >= patience:
            break
    if best_state is not None:
        model.load_state_dict(best_state)                                                     # :150-151
    model.history = history
    return model


def draw_batch_randoms(rng, generator, y, config, device, out=None, onehots=None, counter=None):
    """The per-iteration draws of trainer.py:248-255 + generator.py:90 on the device: (target_y != y, feature mask, Gumbel noise).
    out = (target_y, mask, noise): draw straight into these buffers (the static inputs of a GraphedTrainStep).  counter: the device
    counter form of the launch (ops.DeviceRNG.house_draws)."""
    B = y.shape[0]
    imm = getattr(generator, "_imm_dev", None)
    if imm is None or imm.device != device:
        imm = torch.tensor(list(config.get("immutable_idx", [])), dtype=torch.int32, device=device)
        generator._imm_dev = imm
    if out is None:
        out = (torch.empty((B,), dtype=torch.int64, device=device), torch.empty((B, config["input_dim"]), dtype=torch.float32, device=device),
               torch.empty((B, generator.total_cat), dtype=torch.float32, device=device))
    # one launch; the values of randint(exclude=y), feature_mask, gumbel called in this order
    return rng.house_draws(y.contiguous(), config["num_classes"], config["input_dim"], generator.total_cat, imm if imm.numel() else None, out,
                           onehots=onehots, counter=counter)


def grad_norm_sum(net, out=None):
    """trainer.py:182-183 — this trainer's `grad_norm`: the SUM over parameters of ||p.grad||_2 (not the root of the summed squares
    of mnist/trainer.py:41-42).  One launch over the flat gradient buffer (pcg_norm_sum); `out` (a [1] device tensor): leave the
    value there and return it unread (the trainer reads a whole history at once), else one host read."""
    net._ensure_flat()
    seg = getattr(net, "_norm_seg", None)
    if seg is None or seg[0] != net.flat_grads.data_ptr():
        table = torch.tensor([[off, n] for p, off, n in net._seg if p.requires_grad], dtype=torch.int64, device=net.flat_grads.device)
        seg = net._norm_seg = (net.flat_grads.data_ptr(), table)
    if any(p.grad is None for p, _, _ in net._seg if p.requires_grad):
        raise PcgError("grad_norm_sum: a parameter has no gradient yet (call after a training step)")
    res = ops.norm_sum(net.flat_grads, seg[1], out=out)
    return res if out is not None else float(res.item())


def epoch_permutation(n):
    """The row order DataLoader(TensorDataset, shuffle=True) walks in one epoch, with its exact consumption of torch's global CPU
    generator (trainer.py:198): the loader iterator draws its base seed, the RandomSampler a seed for a private generator, and
    that generator the permutation (tests/test_host_logic.py pins this to torch.utils.data.DataLoader itself)."""
    torch.empty((), dtype=torch.int64).random_()                                   # _BaseDataLoaderIter: base seed (unused here)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())                # RandomSampler.__iter__
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


def train_countergan(generator, config, X_train, y_train, clf_model, *, rng=None, draws=None, graph=None, log_every=100, verbose=True,
                     save=True, discriminator=None, checkpoint=None, checkpoint_every=1, resume=None):
    """house_sales_kc_usa/trainer.py:186-378 `train_countergan(generator, config, X_train, y_train, clf_model)` on the HIP kernels —
    same signature, same body:

      :187-189  device = config['cuda'] (default "cuda"); torch.manual_seed / np.random.seed(config.get('seed', 42))
      :191-198  num_classes from y_train, batch size, DataLoader(shuffle=True, drop_last=True) — here the training set is uploaded
                ONCE and stays in HBM; the epoch's row order is DataLoader's (epoch_permutation), batches are taken on the device
      :200-223  cat_norm_maps from config['scaler'] (or the n-1 fallback)
      :226-231  the Discriminator is built HERE, after the seeding (same torch draws as the reference's), Adam x2
      :233-234  classifier to the device, eval()
      :241-316  the iteration = train_step (draws: target class, feature mask, Gumbel noise from `rng`, an ops.DeviceRNG seeded with
                the config seed by default; `draws(epoch, batch_idx, y) -> (target_y, mask, gumbel)` supplies them instead — parity runs)
      :318-343  pred_gain, sparsity, L2 reg, class-flip rate: one fused device reduction riding in the step (pcg_house_diag); the
                classifier's logits of the ORIGINAL rows are evaluated once for the whole training set (the classifier is frozen)
      :345-355  the log line every 100 batches; D_loss / G_loss and the four diagnostics are summed on the device and read ONCE per
                epoch (the reference: eight .item() calls per iteration)
      :357-366  epoch summary with G_grad / D_grad (grad_norm_sum).  D's .grad there = the D step's gradients + the G step's critic
                weight gradients (no zero_grad in between, :293 -> :314): the last iteration of an epoch therefore runs with
                skip_dead_d_wgrad=False, all others skip that dead work
      :369-378  torch.save(generator.state_dict(), config['generator_path']) (the loss-curve PNG is plotting: left out)

    graph (default: when the batch size divides into full batches and no `draws` hook is given): every full-size iteration is ONE
    HIP-graph replay (GraphedTrainStep(dataset=..., diag=...)) — the benched rate through the reference-shaped API.
    checkpoint (a path): the run's whole state (pcgan_amd.checkpoint, DESIGN.md §3.23: both nets, both optimizers, `rng`, torch's CPU
    generator that epoch_permutation draws from, the histories) is written there after every checkpoint_every-th epoch, which reads
    the epochs' results at that point.  resume (a path or a loaded checkpoint): everything is built as always -- the seeding and the
    Discriminator's construction included -- the stored state is restored over it BEFORE the graphed step is built (its device
    counter starts at the restored offset, its warm-up leaves the loaded Adam state alone), and training continues with the next
    epoch.  config['epochs'] may be larger than when the checkpoint was written; batch size, number of rows and seed must be the
    same.  A resume at or past the last epoch returns the stored histories without a launch.
    Returns {"d_losses", "g_losses", "pred_gain", "sparsity", "l2_reg", "class_flip_rate", "G_grad", "D_grad", "discriminator"}
    (per-epoch lists, after a resume the epochs before the interruption included; the reference returns None)."""
    _ckpt.check_args("train_countergan", checkpoint, checkpoint_every, resume)
    device = torch.device(config.get("cuda", "cuda"))
    if device.type != "cuda":
        raise PcgError(f"train_countergan: config['cuda'] = {device}; libpcgan_hip has no CPU path")
    seed = config.get("seed", 42)
    torch.manual_seed(seed)                                                                    # :188
    np.random.seed(seed)                                                                       # :189
    y_np = np.asarray(y_train)
    num_classes = int(np.unique(y_np).size)                                                    # :191
    bs = int(config.get("batch_size", 128))                                                    # :192
    X_t = torch.tensor(np.asarray(X_train), dtype=torch.float32)                               # :195
    y_t = torch.tensor(y_np, dtype=torch.long)                                                 # :196
    N = X_t.shape[0]
    steps = N // bs                                                                            # drop_last (:198)
    if steps < 1:
        raise PcgError(f"train_countergan: {N} rows do not fill one batch of {bs} (drop_last=True leaves no iteration)")
    X_dev, y_dev = X_t.to(device), y_t.to(device)                                              # the whole training set: resident
    cfg = dict(config, num_classes=num_classes)
    norm_vals = cat_norm_maps(generator, cfg, device)                                          # :200-223
    G = generator.to(device)
    D = discriminator if discriminator is not None else Discriminator(config["input_dim"], config["hidden_dim"], num_classes)   # :227
    D = D.to(device)
    opt_g, opt_d = make_optimizers(G, D, cfg)                                                  # :230-231
    clf_model = clf_model.to(device)                                                           # :233
    clf_model.eval()                                                                           # :234
    frozen = not any(p.requires_grad for p in clf_model.parameters())
    rng = rng if rng is not None else ops.DeviceRNG(seed=seed)
    epochs = int(config["epochs"])
    names = ("d_losses", "g_losses", "pred_gain", "sparsity", "l2_reg", "class_flip_rate")
    hist = {k: [] for k in names + ("G_grad", "D_grad")}
    first = 0
    if resume is not None:
        state = _ckpt.open_resume(resume, "train_countergan", batch_size=bs, n_rows=N, seed=seed)
        vals = _ckpt.restore(state, G=G, D=D, opt_g=opt_g, opt_d=opt_d, rng=rng)
        first, hist = vals["epoch"], {k: list(vals["history"][k]) for k in hist}
        if first >= epochs:                                                                    # nothing left to run: no launch
            hist["discriminator"] = D
            return hist
    # the classifier on the original rows (:320): frozen, so ONE evaluation for the whole training set serves every iteration
    with torch.no_grad():
        logits_orig = torch.cat([clf_model(X_dev[i:i + 65536]).detach() for i in range(0, N, 65536)]).contiguous()
    acc = torch.zeros(8, dtype=torch.float64, device=device)
    diag = {"logits_orig": logits_orig, "acc": acc, "eps": 1e-3}
    if graph is None:
        graph = draws is None and frozen
    gs = None
    if graph:
        if draws is not None:
            raise PcgError("train_countergan(graph=True): supplied draws cannot be replayed from a captured step; use graph=False")
        gs = GraphedTrainStep(G, D, clf_model, opt_g, opt_d, norm_vals, bs, cfg, rng=rng, dataset=(X_dev, y_dev), diag=diag,
                              with_critic_wgrad_variant=True)
    # per-epoch results stay on the device until someone needs them: verbose prints (and reads) every epoch like the reference, a
    # checkpoint reads the epochs since the last one, otherwise ONE read after the last epoch — the host never waits for the GPU
    # inside the loop
    acc_hist = torch.zeros((epochs, 8), dtype=torch.float64, device=device)
    gn_hist = torch.zeros((epochs, 2), dtype=torch.float32, device=device)
    unread = first                                                                             # first epoch whose results are still on the device

    def read_epochs(lo, hi):
        a, gn = acc_hist[lo:hi].cpu().numpy(), gn_hist[lo:hi].cpu().numpy()
        for e in range(hi - lo):
            n_it = max(float(a[e, 6]), 1.0)
            for k, v in zip(names, a[e, :6] / n_it):
                hist[k].append(float(v))
            hist["G_grad"].append(float(gn[e, 0])); hist["D_grad"].append(float(gn[e, 1]))

    sched = "inline" if (frozen and not clf_model.training) else None
    for epoch in range(first, epochs):                                                         # :237
        perm = epoch_permutation(N)[:steps * bs]                                               # :241 (the loader's order)
        perm_dev = perm.to(device)
        ops.fill(acc.view(torch.float32), 0.0)
        if gs is not None:
            gs.new_epoch(perm_dev)
        for batch_idx in range(steps):
            last = batch_idx == steps - 1          # keeps the G step's critic weight gradients: D_grad of the epoch summary (:362)
            if gs is not None:
                out = gs.replay(full=last)
            else:
                idx = perm_dev[batch_idx * bs:(batch_idx + 1) * bs]
                x, y = X_dev.index_select(0, idx), y_dev.index_select(0, idx)                  # :242-243
                if draws is not None:
                    target_y, mask, noise = draws(epoch, batch_idx, y)                          # :248-255, generator.py:90
                    target_y, mask = target_y.to(device), mask.to(device)
                    noise = G.pack_noise(noise) if isinstance(noise, dict) else noise.to(device)
                else:
                    target_y, mask, noise = draw_batch_randoms(rng, G, y, cfg, device)
                out = train_step(G, D, clf_model, opt_g, opt_d, x, y, target_y, mask, norm_vals, cfg, gumbel=noise, branch=sched,
                                 diag=dict(diag, src_rows=idx), skip_dead_d_wgrad=not last)
            if verbose and batch_idx % log_every == 0:                                         # :345-348
                print(f"[Epoch {epoch + 1}/{epochs}] batch {batch_idx} :: "
                      f"D(real)={torch.sigmoid(out['D_real']).mean().item():.3f}, D(fake)={torch.sigmoid(out['D_fake_forG']).mean().item():.3f}, "
                      f"g_adv={out['g_adv'].item():.4f}, g_cls={out['g_cls'].item():.4f}, reg={out['reg'].item():.6f}, "
                      f"mask_pen={out['mask_pen'].item():.5f}")
        acc_hist[epoch].copy_(acc)                                                             # :349-355 (device to device, no sync)
        grad_norm_sum(G, out=gn_hist[epoch, 0:1]); grad_norm_sum(D, out=gn_hist[epoch, 1:2])   # :362
        if verbose:
            read_epochs(epoch, epoch + 1)
            unread = epoch + 1
            print(f"[{epoch + 1}/{epochs}] D: {hist['d_losses'][-1]:.4f}, G: {hist['g_losses'][-1]:.4f}, "
                  f"pred_gain={hist['pred_gain'][-1]:.4f}, sparsity={hist['sparsity'][-1]:.4f}, l2_reg={hist['l2_reg'][-1]:.4f}, "
                  f"class_flip_rate={hist['class_flip_rate'][-1]:.4f} | G_grad: {hist['G_grad'][-1]:.4f}, D_grad: {hist['D_grad'][-1]:.4f}")
        if _ckpt.due(checkpoint, checkpoint_every, epoch):
            if unread <= epoch:
                read_epochs(unread, epoch + 1)
                unread = epoch + 1
            _ckpt.save(checkpoint, _ckpt.capture(G=G, D=D, opt_g=opt_g, opt_d=opt_d, rng=rng, epoch=epoch + 1, history=hist,
                                                 run={"batch_size": bs, "n_rows": N, "seed": seed}))
    if unread < epochs:
        read_epochs(unread, epochs)
    if save and config.get("generator_path"):
        import os
        os.makedirs(os.path.dirname(os.path.abspath(config["generator_path"])) or ".", exist_ok=True)
        torch.save({k: v.detach().cpu().contiguous() for k, v in generator.state_dict().items()}, config["generator_path"])   # :377
        if verbose:
            print(f"Saved generator model to {config['generator_path']}")
    hist["discriminator"] = D
    return hist


def train_countergan_loop(generator, discriminator, classifier, loader, config, device, rng=None, log_every=50):
    """The bare loop over a user-supplied iterable of (x, y) batches (r01 form; the reference-shaped entry point is train_countergan):
    per-epoch means of D and G loss."""
    opt_g, opt_d = make_optimizers(generator, discriminator, config)
    norm_vals = cat_norm_maps(generator, config, device)
    rng = rng if rng is not None else ops.DeviceRNG(seed=0)
    classifier.eval()
    history = []
    for epoch in range(config["epochs"]):
        pending = []
        for batch_idx, (x, y) in enumerate(loader):
            x, y = x.to(device), y.to(device)
            target_y, mask, noise = draw_batch_randoms(rng, generator, y, config, device)
            out = train_step(generator, discriminator, classifier, opt_g, opt_d, x, y, target_y, mask, norm_vals, config, gumbel=noise)
            pending.append((out["D_loss"].detach(), out["G_loss"].detach()))   # no grad_fn kept alive over the epoch
            if batch_idx % log_every == 0:
                print(f"[Epoch {epoch + 1}/{config['epochs']}] batch {batch_idx}: D_loss={out['D_loss'].item():.4f}, "
                      f"G_loss={out['G_loss'].item():.4f}, g_adv={out['g_adv'].item():.4f}, g_cls={out['g_cls'].item():.4f}, "
                      f"reg={out['reg'].item():.4f}, mask_pen={out['mask_pen'].item():.6f}")
        n = max(len(pending), 1)
        history.append((sum(d.item() for d, _ in pending) / n, sum(g.item() for _, g in pending) / n))
    return history


def build(device, config=CONFIG, seed=0):
    """(G, D, clf) on `device`, constructed in the reference's order (main.py: classifier, generator; trainer.py:227: D)."""
    torch.manual_seed(seed)
    clf = NNClassifier(config["input_dim"], config["num_classes"])
    G = ResidualGenerator(config["input_dim"], config["hidden_dim"], config["num_classes"], config["continuous_idx"],
                          config["categorical_info"], tau=config["gumbel_tau"])
    D = Discriminator(config["input_dim"], config["hidden_dim"], config["num_classes"])
    clf.eval()
    for p in clf.parameters():
        p.requires_grad = False
    return G.to(device), D.to(device), clf.to(device)
