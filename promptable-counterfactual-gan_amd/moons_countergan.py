"""conditional_counteRGAN/moons on the HIP kernels — the way house.py mirrors house_sales_kc_usa:

    config.py                   -> config (same keys and defaults; "cuda" defaults to "cuda")
    data_utils.py:7-22          -> load_and_preprocess (make_moons / MinMaxScaler / train_test_split restated, bit-identical)
    models/generator.py:4-24    -> ResidualGenerator      (Linear-BatchNorm1d-ReLU x3, Linear; state_dict keys net.{0,1,3,4,6,7,9})
    models/discriminator.py:6-22-> Discriminator          (four spectral-norm Linears, LeakyReLU 0.2; net.{0,2,4,6}.weight_orig/_u/_v/bias)
    models/nn_classifier.py:3-15-> NNClassifier           (Linear-ReLU-Linear-ReLU-Linear; net.{0,2,4})
    trainer.py:13-29, main.py:14-40 -> train_classifier / get_classifier; with one_launch=True the 1000 Adam steps of trainer.py:22-25
                                   run in ONE launch of pcg_moons_clf_fit (csrc/moons_clf.hip): fit_classifier /
                                   ClassifierFit.  The default stays the op chain (_fit_classifier)
    trainer.py:31-128           -> train_countergan: one epoch = ONE launch of pcg_moons_cf_train_steps (csrc/moons_cf.hip), which
                                   runs every iteration of the batch loop (:58-113) inside one workgroup

    gradio_app.py:79-95         -> counterfactuals: this point, that target class, these features allowed to move (MASKS)
    eval_utils.py:10-26         -> evaluate_classifier (accuracy, confusion matrix, classifier_confusion.csv)
    eval_utils.py:29-106        -> compute_metrics_per_target: every mask, target class and loader batch in ONE launch of
                                   pcg_moons_cf_eval (csrc/moons_cf_eval.hip), one read of the group sums
    eval_utils.py:196-206       -> decision_regions: the 200 x 200 grid in one launch
    eval_utils.py:227-268, main.py:42-60 -> evaluate_pipeline, main

The modules' `forward` runs the HIP forward kernel (pcg_moons_cf_forward) without autograd: backward through the single modules is
not provided — training goes through train_countergan / TrainSteps.  The evaluation returns lists of dicts and numpy arrays and writes
its CSV files with plain Python (no pandas / scikit-learn on the product path); the plots are left out.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import _cfeval, _epoch, ops
from . import checkpoint as _ckpt
from ._cfeval import confusion_csv, confusion_matrix, metric_rows, upload  # noqa: F401  (public here: the host side is _cfeval's)
from ._epoch import no_autograd, on_gpu
from ._lib import (MoonsCfDesc, MoonsCfEvalArgs, MoonsCfFwdArgs, MoonsCfTrainArgs, MoonsClfFitArgs, MoonsClfFitDesc, PcgError,
                   load as _lib_load)
from .countergan import CrossEntropyLoss
from .data import MinMax, _split_indices
from .house import epoch_permutation
from .nn import FlatModule, HipSequential
from .optim import Adam

config = {                                                                    # config.py:1-17
    "seed": 42,
    "epochs": 500,
    "batch_size": 64,
    "lr_G": 1e-3,
    "lr_D": 1e-3,
    "lambda_cls": 2.0,
    "lambda_reg_l1": 5.0,
    "lambda_reg_l2": 5.0,
    "lambda_mask": 3.0,
    "input_dim": 2,
    "hidden_dim": 32,
    "out_dir": "results",
    "clf_model_path": "results/classifier.pt",
    "generator_path": "results/generator.pt",
    "cuda": "cuda",
}

HIDDEN_DIMS = (32, 64)          # the kernel's instantiations
INPUT_DIM, NUM_CLASSES, CLF_HIDDEN = 2, 3, 32
MAX_BATCH = 512
MAX_FIT_ROWS = 4096             # pcg_moons_clf_fit: one workgroup walks the whole training set
LOG_FIELDS = ("D_loss", "G_loss", "D_real_p", "D_fake_p", "g_adv", "g_cls", "reg_l1", "reg_l2", "mask_pen")


# ---- data (data_utils.py) ------------------------------------------------------------------------------------------------------
def make_moons(n_samples, noise):
    """sklearn.datasets.make_moons(n_samples, noise=noise) with random_state=None: the global numpy generator — the two half
    circles from linspace, one shuffle of the rows (sklearn.utils.shuffle: RandomState.shuffle of an index vector), then the noise."""
    n_out = n_samples // 2
    n_in = n_samples - n_out
    outer_x = np.cos(np.linspace(0, np.pi, n_out))
    outer_y = np.sin(np.linspace(0, np.pi, n_out))
    inner_x = 1 - np.cos(np.linspace(0, np.pi, n_in))
    inner_y = 1 - np.sin(np.linspace(0, np.pi, n_in)) - 0.5
    X = np.vstack([np.append(outer_x, inner_x), np.append(outer_y, inner_y)]).T
    y = np.hstack([np.zeros(n_out, dtype=np.intp), np.ones(n_in, dtype=np.intp)])
    idx = np.arange(n_samples)
    np.random.shuffle(idx)
    X, y = X[idx], y[idx]
    X += np.random.normal(scale=noise, size=X.shape)
    return X, y


def load_and_preprocess(seed=42):
    """data_utils.py:7-22: 800 moons points (noise 0.1) and a 400-point rectangle class, MinMax fitted on ALL 1200 points, 80/20
    split with random_state=seed.  Returns (X_train, X_test, y_train, y_test), bit-identical to the reference's arrays."""
    np.random.seed(seed)                                                      # :8
    X_moons, y_moons = make_moons(800, noise=0.1)                             # :9
    X_rect = np.random.uniform(low=[-2, 2], high=[2, 4], size=(400, 2))       # :12
    y_rect = np.full(400, 2)                                                  # :13
    X = np.vstack([X_moons, X_rect])                                          # :15
    y = np.concatenate([y_moons, y_rect])                                     # :16
    X = MinMax().fit_transform(X)                                             # :18-19
    tr, te = _split_indices(len(X), 0.2, seed)                                # :21
    return X[tr], X[te], y[tr], y[te]


# ---- modules ---------------------------------------------------------------------------------------------------------------------
def _check_dims(input_dim, hidden_dim, num_classes, clf_hidden=CLF_HIDDEN, batch=None):
    """The shapes the kernels are built for; anything else is refused here, before a launch."""
    if input_dim != INPUT_DIM or num_classes != NUM_CLASSES:
        raise PcgError(f"moons CounteRGAN kernels are built for input_dim {INPUT_DIM} and {NUM_CLASSES} classes, "
                       f"got input_dim {input_dim}, num_classes {num_classes}")
    if hidden_dim not in HIDDEN_DIMS:
        raise PcgError(f"moons CounteRGAN kernels are built for hidden_dim in {HIDDEN_DIMS}, got {hidden_dim}")
    if clf_hidden != CLF_HIDDEN:
        raise PcgError(f"moons CounteRGAN kernels are built for a classifier of hidden width {CLF_HIDDEN}, got {clf_hidden}")
    if batch is not None and not 2 <= batch <= MAX_BATCH:
        raise PcgError(f"moons CounteRGAN kernels take a batch of 2..{MAX_BATCH} rows, got {batch}")


def _offsets(net, names):
    net._ensure_flat()
    by_id = {id(p): off for p, off, _ in net._seg}
    params = dict(net.named_parameters())
    return [by_id[id(params[n])] for n in names]


_G_NAMES = [f"net.{i}.{k}" for i in (0, 1, 3, 4, 6, 7, 9) for k in ("weight", "bias")]
_D_NAMES = [f"net.{i}.weight_orig" for i in (0, 2, 4, 6)] + [f"net.{i}.bias" for i in (0, 2, 4, 6)]
_C_NAMES = [f"net.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]


def _desc(hidden, B, G=None, D=None, C=None, N=0):
    d = MoonsCfDesc()
    d.hidden, d.clf_hidden, d.B, d.N = hidden, CLF_HIDDEN, B, N
    d.nG = d.nD = d.nC = 1
    if G is not None:
        d.g_off[:] = _offsets(G, _G_NAMES)
        d.nG = d.nG_adam = G.flat_params.numel()
    if D is not None:
        d.d_off[:] = _offsets(D, _D_NAMES)
        d.nD = d.nD_adam = D.flat_params.numel()
    if C is not None:
        d.c_off[:] = _offsets(C, _C_NAMES)
        d.nC = C.flat_params.numel()
    d.bn_eps, d.bn_momentum, d.sn_eps, d.slope = 1e-5, 0.1, 1e-12, 0.2
    return d


def _bn_layers(G):
    return [G.net[i] for i in (1, 4, 7)]


def _sn_layers(D):
    return [D.net[i] for i in (0, 2, 4, 6)]


def _fill_state(args, G=None, D=None):
    if G is not None:
        for i, bn in enumerate(_bn_layers(G)):
            args.bn_mean[i], args.bn_var[i], args.bn_nbt[i] = (bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                                             bn.num_batches_tracked.data_ptr())
    if D is not None:
        for i, lin in enumerate(_sn_layers(D)):
            args.sn_u[i], args.sn_v[i] = lin.weight_u.data_ptr(), lin.weight_v.data_ptr()


def _forward(which, net, hidden, train, x, onehot=None, mask=None, G=None, D=None, C=None):
    """One pcg_moons_cf_forward launch (B <= 512 rows)."""
    B = x.shape[0]
    dev = net.flat_params.device
    x = ops._chk(x.contiguous(), "x")
    f32 = dict(dtype=torch.float32, device=dev)
    desc = _desc(hidden, B, G=G, D=D, C=C)
    a = MoonsCfFwdArgs()
    a.which, a.train, a.B = which, int(bool(train)), B
    a.x, a.params = x.data_ptr(), net.flat_params.data_ptr()
    if onehot is not None:
        onehot = ops._chk(onehot.contiguous(), "target_onehot")
        a.onehot = onehot.data_ptr()
    if mask is not None:
        mask = ops._chk(mask.contiguous(), "mask")
        a.mask = mask.data_ptr()
    _fill_state(a, G=G, D=D)
    out0 = torch.empty((B, (INPUT_DIM, 1, NUM_CLASSES)[which]), **f32)
    out1 = torch.empty((B, INPUT_DIM), **f32) if which == 0 else None
    a.out0 = out0.data_ptr()
    a.out1 = out1.data_ptr() if out1 is not None else None
    lib = _lib_load()
    nbytes = lib.pcg_moons_cf_scratch_bytes(ctypes.byref(desc), 1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), nbytes
    ops.check(lib.pcg_moons_cf_forward(ctypes.byref(desc), ctypes.byref(a), ops._stream()), "pcg_moons_cf_forward")
    return out0, out1


def _chunks(B, can_split):
    if B <= MAX_BATCH:
        return [(0, B)]
    if not can_split:
        raise PcgError(f"a training-mode forward takes at most {MAX_BATCH} rows (batch statistics / one power iteration), got {B}")
    return [(i, min(i + MAX_BATCH, B)) for i in range(0, B, MAX_BATCH)]


class ResidualGenerator(FlatModule):
    """models/generator.py:4-24.  forward(x, target_onehot, mask) -> (raw_residual, masked_residual); training mode uses the batch
    statistics and updates the running ones (momentum 0.1, unbiased variance, num_batches_tracked + 1), eval mode the running ones."""

    def __init__(self, input_dim, hidden_dim, num_classes):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(input_dim + num_classes + input_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim // 2), nn.BatchNorm1d(hidden_dim // 2), nn.ReLU(),
            nn.Linear(hidden_dim // 2, input_dim))
        self.input_dim, self.hidden_dim, self.num_classes = input_dim, hidden_dim, num_classes

    def forward(self, x, target_onehot, mask=None):
        _check_dims(self.input_dim, self.hidden_dim, self.num_classes, batch=x.shape[0] if self.training else None)
        if mask is None:
            raise PcgError("ResidualGenerator.forward: mask is required (generator.py:21 concatenates it)")
        on_gpu(self, x)
        no_autograd(self, x, target_onehot, mask)
        outs = [_forward(0, self, self.hidden_dim, self.training, x[i:j], target_onehot[i:j], mask[i:j], G=self)
                for i, j in _chunks(x.shape[0], not self.training)]
        return torch.cat([o[0] for o in outs]) if len(outs) > 1 else outs[0][0], torch.cat([o[1] for o in outs]) if len(outs) > 1 else outs[0][1]


class Discriminator(FlatModule):
    """models/discriminator.py:6-22.  As torch's spectral_norm: a training-mode forward does one power iteration and updates
    weight_u / weight_v in place; eval mode uses the stored vectors."""

    def __init__(self, input_dim, hidden_dim, num_classes):
        super().__init__()
        self.net = nn.Sequential(
            spectral_norm(nn.Linear(input_dim + num_classes, hidden_dim)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim, hidden_dim // 2)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim // 2, hidden_dim // 2)), nn.LeakyReLU(0.2, inplace=True),
            spectral_norm(nn.Linear(hidden_dim // 2, 1)))
        self.input_dim, self.hidden_dim, self.num_classes = input_dim, hidden_dim, num_classes

    def forward(self, x, target_onehot):
        _check_dims(self.input_dim, self.hidden_dim, self.num_classes, batch=x.shape[0] if self.training else None)
        on_gpu(self, x)
        no_autograd(self, x, target_onehot)
        outs = [_forward(1, self, self.hidden_dim, self.training, x[i:j], target_onehot[i:j], D=self)[0]
                for i, j in _chunks(x.shape[0], not self.training)]
        return torch.cat(outs) if len(outs) > 1 else outs[0]


class NNClassifier(FlatModule):
    """models/nn_classifier.py:3-15 (no dropout, no BatchNorm: train and eval mode compute the same)."""

    def __init__(self, input_dim, hidden_dim=32, num_classes=3):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, num_classes))
        self.input_dim, self.hidden_dim, self.num_classes = input_dim, hidden_dim, num_classes

    def forward(self, x):
        _check_dims(self.input_dim, HIDDEN_DIMS[0], self.num_classes, clf_hidden=self.hidden_dim)
        on_gpu(self, x)
        no_autograd(self, x)
        outs = [_forward(2, self, HIDDEN_DIMS[0], False, x[i:j], C=self)[0] for i, j in _chunks(x.shape[0], True)]
        return torch.cat(outs) if len(outs) > 1 else outs[0]


# ---- classifier (trainer.py:13-29, main.py:14-40) -------------------------------------------------------------------------------
def _fit_classifier(clf, X_train, y_train, device):
    """1000 full-batch Adam(1e-2) steps of cross-entropy (trainer.py:22-25) through the generic HIP MLP (HipSequential), then the
    weights into `clf`."""
    mlp = HipSequential(nn.Linear(clf.input_dim, clf.hidden_dim), nn.ReLU(), nn.Linear(clf.hidden_dim, clf.hidden_dim), nn.ReLU(),
                        nn.Linear(clf.hidden_dim, clf.num_classes))
    mlp.load_state_dict({k[4:]: v for k, v in clf.state_dict().items()})
    mlp.to(device)
    opt = Adam(mlp.parameters(), lr=1e-2)
    loss_fn = CrossEntropyLoss()
    X_t = torch.tensor(np.asarray(X_train), dtype=torch.float32).to(device)
    y_t = torch.tensor(np.asarray(y_train), dtype=torch.long).to(device)
    for _ in range(1000):
        preds = mlp(X_t)
        loss = loss_fn(preds, y_t)
        opt.zero_grad(); loss.backward(); opt.step()
    clf.load_state_dict({"net." + k: v.detach() for k, v in mlp.state_dict().items()})
    return clf


class ClassifierFit:
    """Runs iterations of trainer.py:22-25 (full-batch cross-entropy, Adam) on the GPU, n per launch (pcg_moons_clf_fit).  Holds the
    training set in HBM.  run(n, count_correct=False) -> losses [n] (the loss before each update, a device tensor), and with
    count_correct the number of training rows the final weights classify as their label ([1] int32 on the device).

    After a run `clf` and `opt` hold what the reference's objects hold after n iterations: weights, exp_avg / exp_avg_sq / step, so
    an eager opt.step() continues at step n + 1.  The contents of the parameters' .grad are NOT specified after a run."""

    def __init__(self, clf, X_train, y_train, lr=1e-2, opt=None):
        _check_dims(clf.input_dim, HIDDEN_DIMS[0], clf.num_classes, clf_hidden=clf.hidden_dim)
        if any(not p.requires_grad for p in clf.parameters()):
            raise PcgError("ClassifierFit: every parameter of the classifier must have requires_grad=True (the kernel updates all of them)")
        X, y = np.asarray(X_train), np.asarray(y_train)
        if X.ndim != 2 or X.shape[1] != INPUT_DIM or y.shape != (X.shape[0],):
            raise PcgError(f"ClassifierFit: X_train must be [N][{INPUT_DIM}] and y_train [N], got {X.shape} and {y.shape}")
        if not 1 <= X.shape[0] <= MAX_FIT_ROWS:
            raise PcgError(f"ClassifierFit: N = {X.shape[0]} rows; one launch takes 1..{MAX_FIT_ROWS}")
        if y.dtype.kind not in "iu" or y.min() < 0 or y.max() >= NUM_CLASSES:
            raise PcgError(f"ClassifierFit: labels must be integers in [0, {NUM_CLASSES})")
        if opt is None:
            opt = Adam(clf.parameters(), lr=lr)
        if type(opt) is not Adam:
            raise PcgError("ClassifierFit: the fused step implements pcgan_amd.optim.Adam only")
        if len(opt.param_groups) != 1 or opt.param_groups[0]["weight_decay"] != 0.0 or opt.param_groups[0].get("amsgrad", False):
            raise PcgError("ClassifierFit: the optimizer must be one parameter group with weight decay 0 and no amsgrad")
        dev = _epoch.one_gpu(clf, who="ClassifierFit")
        self.clf, self.device, self.N = clf, dev, X.shape[0]
        self.X, self.Y = _epoch.resident(X, torch.float32, dev), _epoch.resident(y, torch.int64, dev)
        self.opt, self.seg = opt, opt.flat_segment(clf, "ClassifierFit")
        self.scratch, self.scratch_bytes = _epoch.alloc_scratch(_lib_load().pcg_moons_clf_fit_scratch_bytes(ctypes.byref(self._make_desc())), dev)

    def _make_desc(self):
        d = MoonsClfFitDesc()
        d.hidden, d.N, d.nC, d.nC_adam = self.clf.hidden_dim, self.N, self.clf.flat_params.numel(), self.seg["n"]
        d.c_off[:] = _offsets(self.clf, _C_NAMES)
        g = self.opt.param_groups[0]              # read per launch: a changed learning rate takes effect at the next one
        d.lr, d.beta1, d.beta2, d.adam_eps = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        return d

    def run(self, n, count_correct=False):
        n = int(n)
        if n < 1:
            raise PcgError(f"ClassifierFit.run: n = {n} steps")
        losses = torch.empty(n, dtype=torch.float32, device=self.device)
        correct = torch.zeros(1, dtype=torch.int32, device=self.device) if count_correct else None
        a = MoonsClfFitArgs()
        a.X, a.Y, a.c_flat = self.X.data_ptr(), self.Y.data_ptr(), self.clf.flat_params.data_ptr()
        a.exp_avg, a.exp_avg_sq, a.step = self.seg["exp_avg"].data_ptr(), self.seg["exp_avg_sq"].data_ptr(), self.seg["step"].data_ptr()
        a.losses = losses.data_ptr()
        a.correct = correct.data_ptr() if count_correct else None
        a.scratch, a.scratch_bytes = (self.scratch.data_ptr() if self.scratch_bytes else None), self.scratch_bytes
        ops.check(_lib_load().pcg_moons_clf_fit(ctypes.byref(self._make_desc()), ctypes.byref(a), n, ops._stream()), "pcg_moons_clf_fit")
        return (losses, correct) if count_correct else losses


def fit_classifier(clf, X_train, y_train, steps=1000, lr=1e-2, steps_per_launch=None):
    """trainer.py:22-25, `steps` iterations in one launch (or in launches of steps_per_launch: bit-identical).  Returns
    {"losses": [steps] device tensor, "optimizer": the Adam that holds the moments, "train_correct": rows of the training set the
    final weights classify as their label (an int; the one host read)}."""
    steps = int(steps)
    per = steps if steps_per_launch is None else int(steps_per_launch)
    if steps < 1 or per < 1:
        raise PcgError(f"fit_classifier: steps = {steps}, steps_per_launch = {steps_per_launch}")
    fit = ClassifierFit(clf, X_train, y_train, lr=lr)
    losses, correct = [], None
    for done in range(0, steps, per):
        n = min(per, steps - done)
        if done + n == steps:
            part, correct = fit.run(n, count_correct=True)
        else:
            part = fit.run(n)
        losses.append(part)
    return {"losses": torch.cat(losses) if len(losses) > 1 else losses[0], "optimizer": fit.opt, "train_correct": int(correct.item())}


def _fit(clf, X_train, y_train, device, one_launch):
    if one_launch:
        fit_classifier(clf, X_train, y_train)
        return clf
    return _fit_classifier(clf, X_train, y_train, device)


def train_classifier(X_train, y_train, config, one_launch=False):
    """trainer.py:13-29: a fresh NNClassifier trained and saved as {"model_state_dict": ...} at config['clf_model_path'].
    one_launch=True: the 1000 steps in one launch (fit_classifier) instead of the op chain."""
    device = config["cuda"]
    clf = NNClassifier(config["input_dim"]).to(device)
    _fit(clf, X_train, y_train, device, one_launch)
    os.makedirs(config["out_dir"], exist_ok=True)
    torch.save({"model_state_dict": clf.state_dict()}, config["clf_model_path"])
    return clf


def get_classifier(X_train, y_train, config, one_launch=False):
    """main.py:14-40: load config['clf_model_path'] if it exists, else train 1000 steps and save the state_dict there.
    one_launch=True: the 1000 steps in one launch (fit_classifier) instead of the op chain."""
    device = config["cuda"]
    clf = NNClassifier(config["input_dim"]).to(device)
    clf_path = config["clf_model_path"]
    if os.path.exists(clf_path):
        print(f"Loading existing classifier from {clf_path}")
        clf.load_state_dict(torch.load(clf_path, map_location=device))
        clf.eval()
        return clf
    print("Training new classifier...")
    _fit(clf, X_train, y_train, device, one_launch)
    os.makedirs(os.path.dirname(clf_path), exist_ok=True)
    torch.save(clf.state_dict(), clf_path)
    print(f"Saved classifier to {clf_path}")
    return clf


# ---- the fused training iterations -------------------------------------------------------------------------------------------
class TrainSteps:
    """Runs iterations of trainer.py:58-113 on the GPU, n per launch (pcg_moons_cf_train_steps).  Holds the training set in HBM and the
    activation scratch.  run(rows [n][B] int64, target_y [n][B] int64, mask [n][B][2] float32) -> logs [n][9] (LOG_FIELDS).

    After a run the modules hold exactly what the reference's objects hold after n iterations: weights, BatchNorm running
    statistics and num_batches_tracked, spectral-norm u / v, and the optimizers' exp_avg / exp_avg_sq / step.  The contents of the
    parameters' .grad are NOT specified after a run (the kernel keeps gradients in LDS; the reference's D .grad would also hold the
    generator step's critic gradients, which nothing reads)."""

    def __init__(self, G, D, C, opt_G, opt_D, X_train, y_train, config):
        B = int(config["batch_size"])
        _check_dims(G.input_dim, G.hidden_dim, G.num_classes, batch=B)
        _check_dims(D.input_dim, D.hidden_dim, D.num_classes, clf_hidden=C.hidden_dim)
        if D.hidden_dim != G.hidden_dim:
            raise PcgError(f"TrainSteps: generator hidden {G.hidden_dim} and critic hidden {D.hidden_dim} differ (the kernel takes one)")
        dev = _epoch.one_gpu(G, D, C)
        self.G, self.D, self.C, self.B, self.device = G, D, C, B, dev
        self.X, self.Y = _epoch.resident(X_train, torch.float32, dev), _epoch.resident(y_train, torch.int64, dev)
        if self.X.dim() != 2 or self.X.shape[1] != INPUT_DIM or self.Y.shape != (self.X.shape[0],):
            raise PcgError(f"TrainSteps: X_train must be [N][{INPUT_DIM}] and y_train [N]")
        self.N = self.X.shape[0]
        _epoch.check_adam_pair(opt_G, opt_D)
        self.sg, self.sd = opt_G.flat_segment(G, "opt_G"), opt_D.flat_segment(D, "opt_D")
        self.opt_G, self.opt_D = opt_G, opt_D
        self.config = config
        self.scratch, self.scratch_bytes = _epoch.alloc_scratch(_lib_load().pcg_moons_cf_scratch_bytes(ctypes.byref(self._make_desc()), 0), dev)

    def _make_desc(self):
        G, D, C, cfg = self.G, self.D, self.C, self.config
        d = _desc(G.hidden_dim, self.B, G=G, D=D, C=C, N=self.N)
        _epoch.fill_adam_desc(d, self.opt_G, self.opt_D, self.sg, self.sd)
        d.lambda_cls, d.lambda_l1 = float(cfg["lambda_cls"]), float(cfg["lambda_reg_l1"])
        d.lambda_l2, d.lambda_mask = float(cfg["lambda_reg_l2"]), float(cfg["lambda_mask"])
        return d

    def run(self, rows, target_y, mask, check=True):
        n, B = rows.shape[0], self.B
        dev = self.device
        rows = rows.to(dev, torch.int64).contiguous()
        target_y = target_y.to(dev, torch.int64).contiguous()
        mask = mask.to(dev, torch.float32).contiguous()
        if rows.shape != (n, B) or target_y.shape != (n, B) or mask.shape != (n, B, INPUT_DIM) or n < 1:
            raise PcgError(f"TrainSteps.run: expected rows / target_y [n][{B}] and mask [n][{B}][{INPUT_DIM}], got "
                           f"{tuple(rows.shape)}, {tuple(target_y.shape)}, {tuple(mask.shape)}")
        if check:   # indices feed address arithmetic in the kernel: refuse out-of-range ones here (one host read)
            lo = torch.stack([rows.min(), target_y.min()]).cpu()
            hi = torch.stack([rows.max(), target_y.max()]).cpu()
            if lo.min() < 0 or hi[0] >= self.N or hi[1] >= NUM_CLASSES:
                raise PcgError(f"TrainSteps.run: row indices must lie in [0, {self.N}) and targets in [0, {NUM_CLASSES})")
        # the descriptor is rebuilt per run: a changed learning rate (param_groups) takes effect at the next launch
        d = self._make_desc()
        logs = torch.empty((n, len(LOG_FIELDS)), dtype=torch.float32, device=dev)
        a = MoonsCfTrainArgs()
        a.X, a.Y, a.rows, a.target_y, a.mask = (self.X.data_ptr(), self.Y.data_ptr(), rows.data_ptr(), target_y.data_ptr(),
                                                mask.data_ptr())
        _epoch.fill_state_args(a, self.G, self.D, self.sg, self.sd, self.scratch, self.scratch_bytes)
        a.c_flat = self.C.flat_params.data_ptr()
        _fill_state(a, G=self.G, D=self.D)
        a.logs = logs.data_ptr()
        ops.check(_lib_load().pcg_moons_cf_train_steps(ctypes.byref(d), ctypes.byref(a), n, ops._stream()), "pcg_moons_cf_train_steps")
        return logs


def log_now(epoch, batch_idx, epochs):
    """trainer.py:109, the same float expression: (epoch+1) % (epochs*0.1) == 0 and batch_idx % 5 == 0."""
    return (epoch + 1) % (epochs * 0.1) == 0 and batch_idx % 5 == 0


def train_countergan(generator, config, X_train, y_train, clf_model, *, draws=None, log_every=5, verbose=True, save=True,
                     checkpoint=None, checkpoint_every=1, resume=None):
    """trainer.py:31-128 `train_countergan(generator, config, X_train, y_train, clf_model)` — same signature, same body order:

      :32-35   device = config['cuda']; torch.manual_seed / np.random.seed(config['seed'])
      :37-42   num_classes from y_train; DataLoader(shuffle=True, drop_last=True) — the training set is uploaded once, the epoch's row
               order is DataLoader's (house.epoch_permutation, the same draws from torch's CPU generator)
      :45-48   the Discriminator built here, after the seeding (the reference's init draws), Adam x2
      :50-51   classifier to the device, eval()
      :58-113  per epoch: the draws of all its iterations (target class != y: ONE pcg_randint with exclude = y, the reference's
               collision rule; the feature masks: ONE pcg_feature_mask), from an ops.DeviceRNG seeded with config['seed'] —
               `draws(epoch, batch_idx, y) -> (target_y, mask)` supplies them instead (parity runs) — then ONE launch of
               pcg_moons_cf_train_steps for every iteration of the epoch; the nine logged scalars are read once per epoch
      :109-119 the reference's print lines and conditions (log_every: the `batch_idx % 5` of :109)
      :127-128 torch.save(G.state_dict(), config['generator_path'])  (the loss-curve PNG is plotting: left out)

    checkpoint (a path): the run's whole state (pcgan_amd.checkpoint) is written there after every checkpoint_every-th
    epoch.  resume (a path or a loaded checkpoint): everything above is built as always -- the seeding and the Discriminator's
    construction included -- then the stored state is restored over it and training continues with the next epoch;
    config['epochs'] may be larger than when the checkpoint was written; batch size, number of rows and seed must be the same.  The
    kernel's Adam counters are the optimizers' own segments, so restoring the optimizers restores them.

    Returns {"d_losses", "g_losses" (per-epoch means, as the reference collects them; after a resume the epochs before the
    interruption included), "logs" (the last epoch's [iterations][9]; None if a resume found nothing left to do), "discriminator"}.
    The parameters' .grad are not specified afterwards (see TrainSteps)."""
    _ckpt.check_args("train_countergan", checkpoint, checkpoint_every, resume)
    device = torch.device(config.get("cuda", "cuda"))
    if device.type != "cuda":
        raise PcgError(f"train_countergan: config['cuda'] = {device}; libpcgan_hip has no CPU path")
    seed = config["seed"]
    torch.manual_seed(seed)                                                    # :34
    np.random.seed(seed)                                                       # :35
    y_np = np.asarray(y_train)
    num_classes = int(np.unique(y_np).size)                                    # :37
    _check_dims(config["input_dim"], config["hidden_dim"], num_classes, batch=int(config["batch_size"]))
    X_t = torch.tensor(np.asarray(X_train), dtype=torch.float32)               # :39
    N = X_t.shape[0]
    bs = int(config["batch_size"])
    steps = N // bs                                                            # drop_last (:42)
    if steps < 1:
        raise PcgError(f"train_countergan: {N} rows do not fill one batch of {bs} (drop_last=True leaves no iteration)")
    G = generator.to(device)                                                   # :44
    D = Discriminator(config["input_dim"], config["hidden_dim"], num_classes).to(device)   # :45
    opt_G = Adam(G.parameters(), lr=config["lr_G"])                            # :47
    opt_D = Adam(D.parameters(), lr=config["lr_D"])                            # :48
    clf_model = clf_model.to(device)                                           # :50
    clf_model.eval()                                                           # :51
    rng = ops.DeviceRNG(seed=seed)
    epochs = config["epochs"]
    d_losses, g_losses = [], []
    logs = None
    first = 0
    if resume is not None:
        # the optimizers have no segments yet: the loaded moments wait in them until TrainSteps asks for the flat segments below
        state = _ckpt.open_resume(resume, "train_countergan", batch_size=bs, n_rows=N, seed=seed)
        vals = _ckpt.restore(state, G=G, D=D, opt_G=opt_G, opt_D=opt_D, rng=rng)
        first, d_losses, g_losses = vals["epoch"], vals["history"]["d_losses"], vals["history"]["g_losses"]
        if first >= epochs:                                                    # nothing left to run: no launch
            return {"d_losses": d_losses, "g_losses": g_losses, "logs": None, "discriminator": D}
    runner = TrainSteps(G, D, clf_model, opt_G, opt_D, X_t.numpy(), y_np, config)
    y_cpu = torch.as_tensor(y_np, dtype=torch.int64)
    for epoch in range(first, epochs):                                         # :56
        perm = epoch_permutation(N)[:steps * bs]                               # :58 (the loader's order)
        rows = perm.view(steps, bs)
        if draws is None:
            rows_dev = rows.to(device)
            y_rows = runner.Y.index_select(0, rows_dev.view(-1))
            target_y = rng.randint(0, num_classes, steps * bs, device, exclude=y_rows)          # :64-65
            mask = rng.feature_mask(steps * bs, config["input_dim"], device)                    # :69
            logs = runner.run(rows_dev, target_y.view(steps, bs), mask.view(steps, bs, -1), check=False)
        else:
            tys, masks = [], []
            for batch_idx in range(steps):
                t, m = draws(epoch, batch_idx, y_cpu[rows[batch_idx]])
                tys.append(torch.as_tensor(t).to(torch.int64).cpu()); masks.append(torch.as_tensor(m).to(torch.float32).cpu())
            logs = runner.run(rows, torch.stack(tys), torch.stack(masks))
        L = logs.cpu().numpy()                                                 # the one read of the epoch
        for batch_idx in range(steps):
            if verbose and (epoch + 1) % (epochs * 0.1) == 0 and batch_idx % log_every == 0:   # :109
                lg = L[batch_idx]
                print(f"[Epoch {epoch+1}/{config['epochs']}] batch {batch_idx} :: "
                      f"D(real)={float(lg[2]):.3f}, D(fake)={float(lg[3]):.3f}, "
                      f"g_adv={float(lg[4]):.4f}, g_cls={float(lg[5]):.4f}, "
                      f"reg_l1={float(lg[6]):.5f}, reg_l2= {float(lg[7]):.5f}, mask_pen={float(lg[8]):.5f}")
        d_losses.append(np.mean([float(v) for v in L[:, 0]]))                  # :115
        g_losses.append(np.mean([float(v) for v in L[:, 1]]))                  # :116
        if verbose and (epoch + 1) % (epochs * 0.2) == 0:                      # :118
            print(f"[{epoch+1}/{config['epochs']}] D: {d_losses[-1]:.4f}, G: {g_losses[-1]:.4f}")
        if _ckpt.due(checkpoint, checkpoint_every, epoch):
            _ckpt.save(checkpoint, _ckpt.capture(G=G, D=D, opt_G=opt_G, opt_D=opt_D, rng=rng, epoch=epoch + 1,
                                                 history={"d_losses": d_losses, "g_losses": g_losses},
                                                 run={"batch_size": bs, "n_rows": N, "seed": seed}))
    if save:
        os.makedirs(config["out_dir"], exist_ok=True)                          # :121
        torch.save({k: v.detach().cpu().contiguous() for k, v in G.state_dict().items()}, config["generator_path"])   # :127
        if verbose:
            print(f"Generator saved to {config['generator_path']}")
    return {"d_losses": d_losses, "g_losses": g_losses, "logs": logs, "discriminator": D}


# ---- counterfactual queries and evaluation (eval_utils.py, gradio_app.py:79-95): one launch of pcg_moons_cf_eval ---------------
MASKS = {                                                                     # eval_utils.py:231-236, gradio_app.py:85-90
    "both": np.array([1, 1], dtype=np.float32),
    "none": np.array([0, 0], dtype=np.float32),
    "x_only": np.array([1, 0], dtype=np.float32),
    "y_only": np.array([0, 1], dtype=np.float32),
}
METRIC_FIELDS = _cfeval.METRIC_FIELDS
ROW_OUTPUTS = ("raw_residual", "masked_residual", "x_cf", "logits_cf", "logits_x", "pred_cf", "pred_x", "gain")
EVAL_GROUP = 256        # rows per workgroup where the caller names no batch size (queries, the classifier alone)
_OUT_FIELD = {"raw_residual": "raw", "masked_residual": "masked"}             # the argument struct's names where they differ
_OUT_SHAPE = {"raw_residual": (INPUT_DIM,), "masked_residual": (INPUT_DIM,), "x_cf": (INPUT_DIM,), "logits_cf": (NUM_CLASSES,),
              "logits_x": (NUM_CLASSES,), "pred_cf": (), "pred_x": (), "gain": ()}


def _mask_vector(mask, what="mask"):
    """A name from MASKS or a (2,) vector -> float32 ndarray (2,)."""
    if mask is None:
        raise PcgError(f"{what} is required (generator.py:21 concatenates it): a name from MASKS or a ({INPUT_DIM},) vector")
    if isinstance(mask, str):
        if mask not in MASKS:
            raise PcgError(f"{what} {mask!r} is not one of {sorted(MASKS)}")
        return MASKS[mask]
    m = np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask, dtype=np.float32)
    if m.shape != (INPUT_DIM,):
        raise PcgError(f"{what} must be a name from MASKS or a ({INPUT_DIM},) vector, got shape {m.shape}")
    return m


def _eval_dims(generator, classifier):
    if generator is not None:
        _check_dims(generator.input_dim, generator.hidden_dim, generator.num_classes, clf_hidden=classifier.hidden_dim)
    _check_dims(classifier.input_dim, HIDDEN_DIMS[0], classifier.num_classes, clf_hidden=classifier.hidden_dim)


def _eval_launch(generator, classifier, x, group, outputs, y=None, masks=None, target=None, row_mask=None, sums=False):
    """ONE pcg_moons_cf_eval launch.  x [N][2] float32 on the nets' device; generator None: the classifier alone.  Returns the asked
    per-row outputs ([M][3][N]... in the sweep form, [N]... otherwise) and "sums" [M][3][n_groups][4]."""
    dev = x.device
    N = x.shape[0]
    M = masks.shape[0] if masks is not None else 1
    T = NUM_CLASSES if masks is not None else 1
    d = _desc(generator.hidden_dim if generator is not None else HIDDEN_DIMS[0], 2, G=generator, C=classifier)
    a = MoonsCfEvalArgs()
    a.N, a.M, a.T, a.group = N, M, T, int(group)
    keep = [ops._chk(x, "x")]
    a.x, a.c_flat = x.data_ptr(), classifier.flat_params.data_ptr()
    for name, t in (("y", y), ("masks", masks), ("target", target), ("row_mask", row_mask)):
        if t is not None:
            keep.append(t)
            setattr(a, name, t.data_ptr())
    if generator is not None:
        a.g_flat = generator.flat_params.data_ptr()
        for i, bn in enumerate(_bn_layers(generator)):
            a.bn_mean[i], a.bn_var[i] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    lead = (M, T, N) if masks is not None else (N,)
    out = {}
    for name in outputs:
        per_x = name in ("logits_x", "pred_x")
        out[name] = torch.empty(((N,) if per_x else lead) + _OUT_SHAPE[name], dtype=torch.int64 if name.startswith("pred") else torch.float32,
                                device=dev)
        setattr(a, _OUT_FIELD.get(name, name), out[name].data_ptr())
    if sums:
        out["sums"] = torch.empty((M, T, -(-N // int(group)), 4), dtype=torch.float32, device=dev)
        a.sums = out["sums"].data_ptr()
    ops.check(_lib_load().pcg_moons_cf_eval(ctypes.byref(d), ctypes.byref(a), ops._stream()), "pcg_moons_cf_eval")
    return out


def _guard(nets, x, given, *others):
    """The module forwards' guards: a tensor input must already be on the GPU (an ndarray is uploaded), the nets must be there, and
    nothing may ask for autograd."""
    dev = _epoch.one_gpu(*nets, who="moons_countergan evaluation")
    for net in nets:
        if given:
            on_gpu(net, x)
        no_autograd(net, x, *[o for o in others if torch.is_tensor(o) and o.is_floating_point()])
    return dev


def counterfactuals(generator, classifier, x, target, mask):
    """gradio_app.py:79-95 for N points at once: x [N][2] (a tensor on the GPU, or an ndarray), target an int or [N], mask a name
    from MASKS, a (2,) vector or [N][2].  The kernel always uses BatchNorm's running statistics (eval mode, as the reference's app
    sets it).  One launch.  Returns device tensors: x_cf, masked_residual, raw_residual [N][2], logits_cf, logits_x [N][3], pred_cf,
    pred_x [N] (int64), gain [N] = softmax(logits_cf)[target] - softmax(logits_x)[target]."""
    _eval_dims(generator, classifier)
    x, given = _cfeval.rows_arg(x, INPUT_DIM)
    N = x.shape[0]
    if mask is not None and not isinstance(mask, str) and np.ndim(mask) == 2:
        row_mask = mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask), dtype=torch.float32)
        if tuple(row_mask.shape) != (N, INPUT_DIM):
            raise PcgError(f"mask must be a name from MASKS, a ({INPUT_DIM},) vector or [N][{INPUT_DIM}] (N = {N}), got {tuple(row_mask.shape)}")
    else:
        row_mask = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(_mask_vector(mask), (N, INPUT_DIM))))
    target = _cfeval.targets_arg(target, N, NUM_CLASSES)
    dev = _guard((generator, classifier), x, given, row_mask)
    return _eval_launch(generator, classifier, upload(x, dev), EVAL_GROUP, ROW_OUTPUTS, target=upload(target, dev, torch.int64),
                        row_mask=upload(row_mask, dev))


def counterfactual_sweep(generator, classifier, X, y=None, masks=MASKS, batch_size=64, outputs=()):
    """Every mask x every target class x every row in ONE launch: the loops of eval_utils.py:48-97 with the row selection (:57) folded
    into the group sums.  masks: {name: name-or-vector} or a sequence of them; y [N] or None (every row counts); batch_size: the
    loader's (one group of rows per workgroup), any positive integer.  Returns {"sums": [M][3][ceil(N / batch_size)][4] (included
    rows, rows with pred_cf == target, sum of gain, sum of |masked residual| over both features), and the per-row `outputs` asked for
    (names of ROW_OUTPUTS; [M][3][N]..., logits_x / pred_x [N]...)} as device tensors.  Eval mode is the caller's to set."""
    _eval_dims(generator, classifier)
    X, given = _cfeval.rows_arg(X, INPUT_DIM, "X")
    N = X.shape[0]
    vecs = [_mask_vector(m) for m in (masks.values() if isinstance(masks, dict) else masks)]
    if not vecs:
        raise PcgError("counterfactual_sweep: no mask")
    group = int(batch_size)
    if group < 1:
        raise PcgError(f"batch_size must be positive, got {batch_size}")
    _cfeval.check_outputs(outputs, ROW_OUTPUTS)
    y = _cfeval.labels_arg(y, N)
    dev = _guard((generator, classifier), X, given)
    return _eval_launch(generator, classifier, upload(X, dev), group, tuple(outputs), y=None if y is None else upload(y, dev, torch.int64),
                        masks=upload(torch.from_numpy(np.stack(vecs)), dev), sums=True)


def metrics_from_sums(sums):
    """Pure host.  sums [..., n_groups, 4] -> [..., 3] (METRIC_FIELDS) as eval_utils.py:83-103 forms them: per group with a row in
    it the mean over its rows (actionability over both features: / (2 count)), then np.mean over those groups — the mean of the
    per-batch means, so rows of a short batch weigh more.  No such group: nan."""
    return _cfeval.batch_mean_metrics(sums, INPUT_DIM)


def compute_metrics_per_target(generator, classifier, X, y, config, mask=None):
    """eval_utils.py:29-106: per target class the class-flip rate, the prediction gain and the mean |masked residual| over the rows
    whose class differs from the target, averaged over the loader's batches (config['batch_size']).  mask: a name from MASKS or a
    (2,) vector -> a list of dicts (the DataFrame's rows); a dict {name: mask} -> {name: rows}, all of them from ONE launch.
    mask=None is refused, as the module forward refuses it (the reference's torch.cat fails on it, generator.py:21)."""
    if mask is None:
        raise PcgError("compute_metrics_per_target: mask is required (generator.py:21 concatenates it)")
    many = isinstance(mask, dict)
    generator.eval()                                                           # :45
    classifier.eval()                                                          # :46
    with torch.no_grad():                                                      # :47
        res = counterfactual_sweep(generator, classifier, X, y, mask if many else [mask], config["batch_size"])
    table = metrics_from_sums(res["sums"].cpu().numpy())                       # the one read
    if many:
        return {name: metric_rows(table[i]) for i, name in enumerate(mask)}
    return metric_rows(table[0])


def _classify(classifier, X):
    X, given = _cfeval.rows_arg(X, INPUT_DIM, "X")
    _eval_dims(None, classifier)
    dev = _guard((classifier,), X, given)
    return _eval_launch(None, classifier, upload(X, dev), EVAL_GROUP, ("pred_x",))["pred_x"]


def evaluate_classifier(clf, X_test, y_test, config):
    """eval_utils.py:10-26: accuracy and confusion matrix on the test split (one classifier-only launch), classifier_confusion.csv in
    config['out_dir'], the reference's print line.  Returns (acc, cm), which the reference computes and drops."""
    with torch.no_grad():
        preds = _classify(clf, X_test).cpu().numpy()
    y_test = np.asarray(y_test)
    acc = float(np.mean(preds == y_test))
    cm = confusion_matrix(y_test, preds)
    save_path = os.path.join(config["out_dir"], "classifier_confusion.csv")
    os.makedirs(config["out_dir"], exist_ok=True)
    with open(save_path, "w") as f:
        f.write(confusion_csv(cm))
    print(f"Classifier accuracy: {acc:.4f}, confusion matrix saved to {save_path}")
    return acc, cm


def decision_regions(classifier, X, n=200, pad=0.1):
    """eval_utils.py:196-206 (and :114-124): the classifier's class at every point of an n x n grid over X's bounding box widened by
    pad, in one launch.  Returns (xx, yy, Z) as numpy arrays, Z [n][n] int64 — what the reference hands to contourf."""
    X = np.asarray(X)
    x_min, x_max = X[:, 0].min() - pad, X[:, 0].max() + pad
    y_min, y_max = X[:, 1].min() - pad, X[:, 1].max() + pad
    xx, yy = np.meshgrid(np.linspace(x_min, x_max, n), np.linspace(y_min, y_max, n))
    grid = np.c_[xx.ravel(), yy.ravel()]
    with torch.no_grad():
        Z = _classify(classifier, grid).cpu().numpy()
    return xx, yy, Z.reshape(xx.shape)


def save_metrics(rows, save_path, columns=("target_class",) + METRIC_FIELDS):
    """eval_utils.py:187-190: the rows as CSV (DataFrame.to_csv(index=False): shortest float repr, nan as an empty field)."""
    _cfeval.save_table(rows, save_path, columns)
    print(f"Saved metrics to {save_path}")


def evaluate_pipeline(generator, classifier, X_test, y_test, config, masks=None):
    """eval_utils.py:227-268.  As the reference ships it (masks=None): evaluate_classifier and the decision grid of
    plot_decision_boundaries_only — its arrays go to decision_boundaries_no_cfs.npz (xx, yy, Z) where the reference saves the
    picture — and None is returned.  masks=MASKS (or any {name: mask}) also runs the per-mask evaluation the reference keeps
    commented out (:242-264): mask_<name>/metrics.csv and metrics_all_masks.csv, all masks from one launch; returns {name: rows}."""
    base_out = config["out_dir"]
    evaluate_classifier(classifier, X_test, y_test, config)                    # :239
    all_metrics = None
    if masks:
        all_metrics = compute_metrics_per_target(generator, classifier, X_test, y_test, config, mask=dict(masks))
        summary = []
        for name, rows in all_metrics.items():
            print(f"Evaluating mask: {name}")
            save_metrics(rows, os.path.join(base_out, f"mask_{name}", "metrics.csv"))
            summary += [dict(r, mask=name) for r in rows]
        save_metrics(summary, os.path.join(base_out, "metrics_all_masks.csv"), ("target_class",) + METRIC_FIELDS + ("mask",))
    xx, yy, Z = decision_regions(classifier, X_test)                           # :265
    save_path = os.path.join(base_out, "decision_boundaries_no_cfs.npz")
    np.savez_compressed(save_path, xx=xx, yy=yy, Z=Z)
    print(f"Saved decision regions: {save_path}")
    return all_metrics


def main(config=config, one_launch=False):
    """main.py:42-60: the data, the classifier (loaded or trained), the generator (loaded or trained, then frozen), evaluate_pipeline.
    one_launch: the classifier's fit in one launch (get_classifier)."""
    X_train, X_test, y_train, y_test = load_and_preprocess(config["seed"])
    clf = get_classifier(X_train, y_train, config, one_launch=one_launch)
    num_classes = int(np.unique(y_train).size)
    generator = ResidualGenerator(config["input_dim"], config["hidden_dim"], num_classes=num_classes).to(config["cuda"])
    generator_path = config["generator_path"]
    if os.path.exists(generator_path):
        print(f"Loading pretrained generator from {generator_path}...")
    else:
        print("Training CounterGAN and saving generator...")
        train_countergan(generator, config, X_train, y_train, clf)
    generator.load_state_dict(torch.load(generator_path, map_location=config["cuda"]))
    generator.eval()
    for p in generator.parameters():
        p.requires_grad = False
    metrics = evaluate_pipeline(generator, clf, X_test, y_test, config)
    print(metrics)
    return metrics


if __name__ == "__main__":
    main()
