"""Host-side mirror of `simple_gan/moons/make_moons_gan.py` (BASELINE config 1) on the HIP kernels: the two MLPs are
nn.Sequential stacks of nn.Linear / ReLU / Sigmoid run by SequentialConvNet (a Linear is a 1x1 convolution on a
[B,1,1,F] activation, its [out,in] weight already OHWI), the log losses (:70,:83) are the BCE kernel.

    build_generator :33-38, build_discriminator :40-46, train_gan batch body :62-87 -> train_step
    train_gan :49-93                 -> train_gan: one epoch = ONE launch of pcg_moons_gan_train_steps (csrc/moons_gan.hip, DESIGN.md
                                        §3.10), which runs every iteration of the batch loop inside one workgroup
    save_generated_data :109-112     -> sample (pcg_moons_gan_forward; the plotting is left out)

train_step is the op chain (one launch per layer and loss under autograd); train_gan / TrainSteps are the fused path.  The same
kernels serve the conditional GAN (moons_cgan.py): the simple GAN is that one with label_dim = 0.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _epoch, ops
from ._epoch import no_autograd, on_gpu      # (no_autograd: re-exported, moons.no_autograd)
from ._lib import MoonsGanDesc, MoonsGanFwdArgs, MoonsGanTrainArgs, PcgError, load as _lib_load
from .dcgan import _labels
from .nn import BCELoss, HipSequential, _pad4
from .optim import Adam

config = {"n_samples": 2000, "z_dim": 32, "hidden_dim": 128, "batch_size": 50, "lr": 1e-3, "epochs": 500}   # :9-17


def build_generator(z_dim, hidden_dim):
    return HipSequential(nn.Linear(z_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 2))


def build_discriminator(hidden_dim):
    return HipSequential(nn.Linear(2, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1), nn.Sigmoid())


def make_optimizers(generator, discriminator, cfg=config):
    return Adam(generator.parameters(), lr=cfg["lr"]), Adam(discriminator.parameters(), lr=cfg["lr"])          # :50-51


_bce = BCELoss()


def train_step(generator, discriminator, optimizer_G, optimizer_D, real_batch, z_d, z_g):
    """One batch of train_gan (:62-87); the two noise draws (:64,:79) are passed in.
    -mean(log D_real + log(1 - D_fake)) = BCE(D_real, 1) + BCE(D_fake, 0) and -mean(log D_fake) = BCE(D_fake, 1); the BCE
    kernel clamps log at -100 like torch's BCELoss, the reference's bare torch.log gives inf at D in {0,1}."""
    n = real_batch.shape[0]
    dev = real_batch.device
    ones, zeros = _labels.get(n, 1.0, dev), _labels.get(n, 0.0, dev)
    fake_batch = generator(z_d)                                                   # :65
    D_real = discriminator(real_batch)                                            # :67
    D_fake = discriminator(fake_batch)                                            # :68
    loss_D = _bce(D_real.view(-1), ones) + _bce(D_fake.view(-1), zeros)           # :70
    optimizer_D.zero_grad()                                                       # :72
    loss_D.backward()                                                             # :73
    optimizer_D.step()                                                            # :74
    fake_batch = generator(z_g)                                                   # :80
    D_fake = discriminator(fake_batch)                                            # :81
    loss_G = _bce(D_fake.view(-1), ones)                                          # :83
    optimizer_G.zero_grad()                                                       # :85
    loss_G.backward()                                                             # :86
    optimizer_G.step()                                                            # :87
    return loss_D, loss_G


# ---- the fused path: whole iterations in one launch (csrc/moons_gan.hip) ---------------------------------------------------------
HIDDEN_DIMS = (32, 64, 128)     # the kernel's instantiations
MAX_Z, MAX_BATCH = 64, 256
LABEL_DIMS = (0, 2)


def check_dims(z_dim, hidden_dim, label_dim=0, batch=None):
    """The shapes pcg_moons_gan_* are built for; anything else is refused here, before a launch."""
    if hidden_dim not in HIDDEN_DIMS:
        raise PcgError(f"moons GAN kernels are built for hidden_dim in {HIDDEN_DIMS}, got {hidden_dim}")
    if not (4 <= z_dim <= MAX_Z and z_dim % 4 == 0):
        raise PcgError(f"moons GAN kernels take z_dim a multiple of 4 in [4, {MAX_Z}], got {z_dim}")
    if label_dim not in LABEL_DIMS:
        raise PcgError(f"moons GAN kernels take label_dim in {LABEL_DIMS}, got {label_dim}")
    if batch is not None and not 1 <= batch <= MAX_BATCH:
        raise PcgError(f"moons GAN kernels take a batch of 1..{MAX_BATCH} rows, got {batch}")


def check_epoch(n_samples, batch_size):
    """The reference's fake batch always has batch_size rows, so its loss fails on a shorter tail batch (shape mismatch at
    make_moons_gan.py:69 / make_moons_cgan.py:107): such a configuration is refused up front."""
    if batch_size < 1 or n_samples < batch_size or n_samples % batch_size != 0:
        raise PcgError(f"n_samples {n_samples} is not a positive multiple of batch_size {batch_size}: the reference's loss fails on "
                       "the tail batch (real and fake batch sizes differ)")


def _shapes(net, what):
    ps = list(net.parameters())
    if len(ps) != 4 or [p.dim() for p in ps] != [2, 1, 2, 1] or ps[0].shape[0] != ps[1].shape[0] or ps[2].shape[1] != ps[0].shape[0] \
            or ps[2].shape[0] != ps[3].shape[0]:
        raise PcgError(f"{what}: expected Linear - ReLU - Linear (four parameters), got {[tuple(p.shape) for p in ps]}")
    return ps


def net_dims(G=None, D=None, label_dim=None):
    """(z_dim, hidden_dim, label_dim) read off the nets' parameter shapes.  A generator alone does not tell z_dim from label_dim:
    pass label_dim then (default 0)."""
    hidden = None
    if D is not None:
        v1, _, v2, _ = _shapes(D, "discriminator")
        if v2.shape[0] != 1:
            raise PcgError(f"discriminator: the second Linear has {v2.shape[0]} outputs, expected 1")
        hidden, ld = v1.shape[0], v1.shape[1] - 2
        if label_dim is not None and label_dim != ld:
            raise PcgError(f"discriminator: input width {v1.shape[1]} does not match label_dim {label_dim}")
        label_dim = ld
    label_dim = 0 if label_dim is None else label_dim
    z_dim = None
    if G is not None:
        w1, _, w2, _ = _shapes(G, "generator")
        if w2.shape[0] != 2:
            raise PcgError(f"generator: the second Linear has {w2.shape[0]} outputs, expected 2")
        if hidden is not None and w1.shape[0] != hidden:
            raise PcgError(f"generator hidden {w1.shape[0]} and discriminator hidden {hidden} differ (the kernel takes one)")
        hidden, z_dim = w1.shape[0], w1.shape[1] - label_dim
    return z_dim, hidden, label_dim


def _gan_desc(z_dim, hidden, label_dim, G=None, D=None, B=1, N=1):
    """pcg_moons_gan_desc; a net that is not given gets the offsets FlatModule would give it (the kernel checks both)."""
    d = MoonsGanDesc()
    d.hidden, d.z_dim, d.label_dim, d.B, d.N = hidden, z_dim, label_dim, B, N
    for net, sizes, off, tag in ((G, (hidden * (z_dim + label_dim), hidden, 2 * hidden, 2), d.g_off, "nG"),
                                 (D, (hidden * (2 + label_dim), hidden, hidden, 1), d.d_off, "nD")):
        if net is None:
            o = 0
            for k, n in enumerate(sizes):
                off[k] = o
                o += _pad4(n)
            total = o
        else:
            net._ensure_flat()
            off[:] = [o for _, o, _ in net._seg]
            total = net.flat_params.numel()
        setattr(d, tag, total)
        setattr(d, tag + "_adam", total)
    d.beta1, d.beta2, d.adam_eps = 0.9, 0.999, 1e-8
    return d


def gan_forward(net, which, x, onehot=None, label_dim=0):
    """One pcg_moons_gan_forward launch over all rows of x: which = 0 generator (x = z [R][z_dim] -> [R][2]), 1 discriminator
    (x [R][2] -> probabilities [R][1]).  onehot [R][label_dim] when label_dim > 0.  No autograd."""
    on_gpu(net, x)
    dev = net.flat_params.device
    z_dim, hidden, label_dim = net_dims(G=net, label_dim=label_dim) if which == 0 else net_dims(D=net, label_dim=label_dim)
    z_dim = 4 if z_dim is None else z_dim
    check_dims(z_dim, hidden, label_dim)
    x = ops._chk(x.contiguous(), "x")
    R = x.shape[0]
    if x.dim() != 2 or x.shape[1] != (z_dim if which == 0 else 2) or R < 1:
        raise PcgError(f"{type(net).__name__}: expected input [R][{z_dim if which == 0 else 2}], got {tuple(x.shape)}")
    a = MoonsGanFwdArgs()
    if label_dim:
        if onehot is None or tuple(onehot.shape) != (R, label_dim):
            raise PcgError(f"{type(net).__name__}: expected a one-hot [R][{label_dim}]")
        onehot = ops._chk(onehot.contiguous(), "label_onehot")
        a.onehot = onehot.data_ptr()
    d = _gan_desc(z_dim, hidden, label_dim, G=net if which == 0 else None, D=net if which == 1 else None)
    out = torch.empty((R, 2 if which == 0 else 1), dtype=torch.float32, device=dev)
    a.which, a.R, a.x, a.params, a.out = which, R, x.data_ptr(), net.flat_params.data_ptr(), out.data_ptr()
    ops.check(_lib_load().pcg_moons_gan_forward(ctypes.byref(d), ctypes.byref(a), ops._stream()), "pcg_moons_gan_forward")
    return out


class TrainSteps:
    """Runs iterations of the batch loop (make_moons_gan.py:62-87; with labels make_moons_cgan.py:91-129) on the GPU, n per launch
    (pcg_moons_gan_train_steps).  Holds the training set (and its labels) in HBM.

        run(rows [n][B] int64, z [n][2][B][z_dim] float32, labels [n][2][B] int64 = None) -> logs [n][2] = loss_D, loss_G

    rows: the real batch of every iteration as rows of X; z[:, 0] / labels[:, 0] are the D step's draws, z[:, 1] / labels[:, 1] the G
    step's.  After a run the modules and optimizers hold what the reference's hold after n iterations: weights, exp_avg, exp_avg_sq,
    step.  Where D saturates the reference's bare torch.log gives inf / nan; the kernel takes both losses and their gradients from
    D's logit (-log D = softplus(-a), -log(1 - D) = softplus(a)) and stays finite; everywhere else the two agree to rounding.
    The contents of the parameters' .grad are NOT specified after a run (the kernel keeps gradients in LDS)."""

    def __init__(self, G, D, opt_G, opt_D, X, y=None, batch_size=50):
        z_dim, hidden, label_dim = net_dims(G, D)
        B = int(batch_size)
        check_dims(z_dim, hidden, label_dim, batch=B)
        _epoch.check_adam_pair(opt_G, opt_D)                       # (what needs no device is refused before the device is touched)
        dev = _epoch.one_gpu(G, D)
        self.sg, self.sd = opt_G.flat_segment(G, "opt_G"), opt_D.flat_segment(D, "opt_D")
        self.G, self.D, self.opt_G, self.opt_D, self.B, self.device = G, D, opt_G, opt_D, B, dev
        self.z_dim, self.hidden, self.label_dim = z_dim, hidden, label_dim
        self.X = _epoch.resident(X, torch.float32, dev)
        if self.X.dim() != 2 or self.X.shape[1] != 2 or self.X.shape[0] < 1:
            raise PcgError("TrainSteps: X must be [N][2]")
        self.N = self.X.shape[0]
        self.Y = None
        if label_dim:
            if y is None:
                raise PcgError(f"TrainSteps: label_dim {label_dim} needs the labels y [N]")
            y = torch.as_tensor(np.asarray(y), dtype=torch.int64).contiguous()
            if y.shape != (self.N,) or int(y.min()) < 0 or int(y.max()) >= label_dim:
                raise PcgError(f"TrainSteps: y must be [N] with values in [0, {label_dim})")
            self.Y = y.to(dev)
        self.launches = 0
        self.scratch, self.scratch_bytes = _epoch.alloc_scratch(_lib_load().pcg_moons_gan_scratch_bytes(ctypes.byref(self._make_desc())), dev)

    def _make_desc(self):
        d = _gan_desc(self.z_dim, self.hidden, self.label_dim, G=self.G, D=self.D, B=self.B, N=self.N)
        _epoch.fill_adam_desc(d, self.opt_G, self.opt_D, self.sg, self.sd)
        return d

    def run(self, rows, z, labels=None, check=True):
        n, B, L, dev = rows.shape[0], self.B, self.label_dim, self.device
        if tuple(rows.shape) != (n, B) or tuple(z.shape) != (n, 2, B, self.z_dim) or n < 1 or \
                (L and (labels is None or tuple(labels.shape) != (n, 2, B))):
            raise PcgError(f"TrainSteps.run: expected rows [n][{B}], z [n][2][{B}][{self.z_dim}]" + (f", labels [n][2][{B}]" if L else "") +
                           f", got {tuple(rows.shape)}, {tuple(z.shape)}" + (f", {None if labels is None else tuple(labels.shape)}" if L else ""))
        if check:   # rows feed address arithmetic in the kernel: refuse out-of-range ones here, before anything is launched
            r = torch.as_tensor(rows)
            if int(r.min()) < 0 or int(r.max()) >= self.N:
                raise PcgError(f"TrainSteps.run: row indices must lie in [0, {self.N})")
            if L:
                q = torch.as_tensor(labels)
                if int(q.min()) < 0 or int(q.max()) >= L:
                    raise PcgError(f"TrainSteps.run: labels must lie in [0, {L})")
        rows = torch.as_tensor(rows).to(dev, torch.int64).contiguous()
        z = torch.as_tensor(z).to(dev, torch.float32).contiguous()
        # the descriptor is rebuilt per run: a changed learning rate (param_groups) takes effect at the next launch
        d = self._make_desc()
        logs = torch.empty((n, 2), dtype=torch.float32, device=dev)
        a = MoonsGanTrainArgs()
        a.X, a.rows, a.z = self.X.data_ptr(), rows.data_ptr(), z.data_ptr()
        if L:
            labels = torch.as_tensor(labels).to(dev, torch.int64).contiguous()
            a.Y, a.labels = self.Y.data_ptr(), labels.data_ptr()
        _epoch.fill_state_args(a, self.G, self.D, self.sg, self.sd, self.scratch, self.scratch_bytes)
        a.logs = logs.data_ptr()
        ops.check(_lib_load().pcg_moons_gan_train_steps(ctypes.byref(d), ctypes.byref(a), n, ops._stream()), "pcg_moons_gan_train_steps")
        self.launches += 1
        return logs


def run_epochs(runner, epochs, steps, order_of, draws, rng, on_epoch=None):
    """The epoch loop both scripts share: per epoch one row order (order_of(epoch) -> [N] indices into the resident set), the epoch's
    draws (device: one randn launch, and one randint launch with labels; or the `draws` hook), ONE step launch, one read of the logs.
    Returns the per-epoch loss totals, summed in Python as the reference sums its .item()s."""
    B, L, Z, dev = runner.B, runner.label_dim, runner.z_dim, runner.device
    loss_D_values, loss_G_values = [], []
    for epoch in range(epochs):
        rows = torch.as_tensor(np.ascontiguousarray(order_of(epoch)[:steps * B]), dtype=torch.int64).view(steps, B)
        labels = None
        if draws is None:
            z = rng.randn((steps, 2, B, Z), dev)
            if L:
                # make_moons_cgan.py:98 draws the D step's fake labels with randint(0, 1): always class 0; :117 from [0, label_dim)
                labels = torch.zeros((steps, 2, B), dtype=torch.int64, device=dev)
                labels[:, 1] = rng.randint(0, L, steps * B, dev).view(steps, B)
            logs = runner.run(rows, z, labels, check=False)     # rows come from a permutation, labels from randint: in range
        else:
            zs, ls = [], []
            for batch_idx in range(steps):
                dr = draws(epoch, batch_idx)
                if L:
                    z_d, l_d, z_g, l_g = dr
                    ls.append(torch.stack([torch.as_tensor(l_d).to(torch.int64).cpu(), torch.as_tensor(l_g).to(torch.int64).cpu()]))
                else:
                    z_d, z_g = dr
                zs.append(torch.stack([torch.as_tensor(z_d).float().cpu(), torch.as_tensor(z_g).float().cpu()]))
            logs = runner.run(rows, torch.stack(zs), torch.stack(ls) if L else None)
        Lg = logs.cpu().numpy()                                 # the one read of the epoch
        loss_D_total, loss_G_total = 0, 0
        for batch_idx in range(steps):
            loss_D_total += float(Lg[batch_idx, 0])
            loss_G_total += float(Lg[batch_idx, 1])
        loss_D_values.append(loss_D_total)
        loss_G_values.append(loss_G_total)
        if on_epoch is not None:
            on_epoch(epoch, loss_D_total, loss_G_total)
    return loss_D_values, loss_G_values


def train_gan(X, generator, discriminator, config, *, draws=None, perm=None, seed=0, verbose=False):
    """make_moons_gan.py:49-93 `train_gan(X, generator, discriminator, config)` — same signature, same return value
    (loss_D_values, loss_G_values: per-epoch sums of the per-iteration losses):

      :50-51  Adam x2 (pcgan_amd.optim.Adam, torch defaults)
      :56     np.random.shuffle(X) — the caller's array IS shuffled in place, epoch after epoch, as the reference does (its caller
              sees that); the training set itself is uploaded once and the epoch's order goes to the kernel as row indices.
              `perm(epoch) -> [N] indices` replaces numpy's draw (X <- X[perm]) for parity runs.
      :61-88  ONE launch of pcg_moons_gan_train_steps for all n_samples / batch_size iterations; the epoch's 2 x iterations noise
              draws come from ONE randn launch of an ops.DeviceRNG seeded with `seed` — `draws(epoch, batch_idx) -> (z_d, z_g)`
              supplies them instead; the logged losses are read once per epoch.
    The nets may be moons.build_generator / build_discriminator (or any FlatModule of that shape) on the GPU.  Where D saturates
    the losses stay finite (see TrainSteps).  The parameters' .grad are not specified afterwards."""
    X = np.asarray(X) if not isinstance(X, np.ndarray) else X
    B = int(config["batch_size"])
    check_epoch(X.shape[0], B)
    for net in (generator, discriminator):
        if next(net.parameters()).device.type != "cuda":
            raise PcgError(f"train_gan: the nets are on {next(net.parameters()).device}; libpcgan_hip has no CPU path")
    optimizer_G = Adam(generator.parameters(), lr=config["lr"])               # :50
    optimizer_D = Adam(discriminator.parameters(), lr=config["lr"])           # :51
    X0 = X.copy()
    runner = TrainSteps(generator, discriminator, optimizer_G, optimizer_D, X0, batch_size=B)
    order = np.arange(X.shape[0])

    def order_of(epoch):
        nonlocal order
        if perm is None:
            np.random.shuffle(order)          # the draws np.random.shuffle(X) makes (:56): one Fisher-Yates pass over the first axis
        else:
            order = order[np.asarray(perm(epoch))]
        X[:] = X0[order]
        return order

    def on_epoch(epoch, lD, lG):
        if verbose:
            print(f"Epoch [{epoch}/{config['epochs']}], Loss D: {lD:.4f}, Loss G: {lG:.4f}")

    return run_epochs(runner, config["epochs"], X.shape[0] // B, order_of, draws, ops.DeviceRNG(seed=seed), on_epoch)


def sample(generator, n, z=None, seed=0):
    """save_generated_data's draw (:111-112): n generated points [n][2] (a device tensor); z [n][z_dim] or drawn from
    ops.DeviceRNG(seed)."""
    z_dim, _, _ = net_dims(G=generator)
    dev = next(generator.parameters()).device
    if z is None:
        z = ops.DeviceRNG(seed=seed).randn((n, z_dim), dev)
    with torch.no_grad():
        return gan_forward(generator, 0, z)
