"""conditional_counteRGAN/moons on the HIP kernels — the way house.py mirrors house_sales_kc_usa:

    config.py                   -> config (same keys and defaults; "cuda" defaults to "cuda")
    data_utils.py:7-22          -> load_and_preprocess (make_moons / MinMaxScaler / train_test_split restated, bit-identical)
    models/generator.py:4-24    -> ResidualGenerator      (Linear-BatchNorm1d-ReLU x3, Linear; state_dict keys net.{0,1,3,4,6,7,9})
    models/discriminator.py:6-22-> Discriminator          (four spectral-norm Linears, LeakyReLU 0.2; net.{0,2,4,6}.weight_orig/_u/_v/bias)
    models/nn_classifier.py:3-15-> NNClassifier           (Linear-ReLU-Linear-ReLU-Linear; net.{0,2,4})
    trainer.py:13-29, main.py:14-40 -> train_classifier / get_classifier
    trainer.py:31-128           -> train_countergan: one epoch = ONE launch of pcg_moons_cf_train_steps (csrc/moons_cf.hip), which
                                   runs every iteration of the batch loop (:58-113) inside one workgroup

The modules' `forward` runs the HIP forward kernel (pcg_moons_cf_forward) without autograd: backward through the single modules is
not provided — training goes through train_countergan / TrainSteps.  evaluate_pipeline (pandas / matplotlib reporting) is not ported.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import _epoch, ops
from ._epoch import no_autograd, on_gpu
from ._lib import MoonsCfDesc, MoonsCfFwdArgs, MoonsCfTrainArgs, PcgError, load as _lib_load
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


def train_classifier(X_train, y_train, config):
    """trainer.py:13-29: a fresh NNClassifier trained and saved as {"model_state_dict": ...} at config['clf_model_path']."""
    device = config["cuda"]
    clf = NNClassifier(config["input_dim"]).to(device)
    _fit_classifier(clf, X_train, y_train, device)
    os.makedirs(config["out_dir"], exist_ok=True)
    torch.save({"model_state_dict": clf.state_dict()}, config["clf_model_path"])
    return clf


def get_classifier(X_train, y_train, config):
    """main.py:14-40: load config['clf_model_path'] if it exists, else train 1000 steps and save the state_dict there."""
    device = config["cuda"]
    clf = NNClassifier(config["input_dim"]).to(device)
    clf_path = config["clf_model_path"]
    if os.path.exists(clf_path):
        print(f"Loading existing classifier from {clf_path}")
        clf.load_state_dict(torch.load(clf_path, map_location=device))
        clf.eval()
        return clf
    print("Training new classifier...")
    _fit_classifier(clf, X_train, y_train, device)
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


def train_countergan(generator, config, X_train, y_train, clf_model, *, draws=None, log_every=5, verbose=True, save=True):
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

    Returns {"d_losses", "g_losses" (per-epoch means, as the reference collects them), "logs" (the last epoch's [iterations][9]),
    "discriminator"}.  The parameters' .grad are not specified afterwards (see TrainSteps)."""
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
    runner = TrainSteps(G, D, clf_model, opt_G, opt_D, X_t.numpy(), y_np, config)
    rng = ops.DeviceRNG(seed=seed)
    y_cpu = torch.as_tensor(y_np, dtype=torch.int64)
    epochs = config["epochs"]
    d_losses, g_losses = [], []
    logs = None
    for epoch in range(epochs):                                                # :56
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
    if save:
        os.makedirs(config["out_dir"], exist_ok=True)                          # :121
        torch.save({k: v.detach().cpu().contiguous() for k, v in G.state_dict().items()}, config["generator_path"])   # :127
        if verbose:
            print(f"Generator saved to {config['generator_path']}")
    return {"d_losses": d_losses, "g_losses": g_losses, "logs": logs, "discriminator": D}
