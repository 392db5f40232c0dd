"""conditional_gan/moons/make_moons_cgan.py (one-hot conditional MLP GAN on moons) on the HIP kernels:

    config :10-19                    -> config (the same dict)
    Generator :35-46                 -> Generator      (Linear(z_dim + label_dim, hidden) ReLU Linear(hidden, 2); keys net.0.*, net.2.*)
    Discriminator :48-60             -> Discriminator  (Linear(2 + label_dim, hidden) ReLU Linear(hidden, 1) Sigmoid; keys net.0.*, net.2.*)
    one_hot_encode :62-63            -> one_hot_encode
    optimizers :77-78                -> make_optimizers
    the training loop :81-135        -> train: one epoch = ONE launch of pcg_moons_gan_train_steps (csrc/moons_gan.hip)
    save_generated_data :150-155     -> sample (the plotting is left out)

The modules' `forward` runs pcg_moons_gan_forward without autograd: backward through the single modules is not provided — training
goes through train / moons.TrainSteps.  There is no CPU path."""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import PcgError
from ._epoch import no_autograd, on_gpu
from .moons import TrainSteps, check_dims, check_epoch, gan_forward, run_epochs
from .nn import FlatModule
from .optim import Adam

config = {                                                                    # :10-19
    "n_samples": 2000,
    "z_dim": 32,
    "hidden_dim": 128,
    "label_dim": 2,
    "batch_size": 50,
    "lr": 1e-3,
    "epochs": 500,
    "scale_factor": 10,
}


class Generator(FlatModule):
    """:35-46.  forward(z, label_onehot) -> [R][2]."""

    def __init__(self, z_dim, label_dim, hidden_dim):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(z_dim + label_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 2))
        self.z_dim, self.label_dim, self.hidden_dim = z_dim, label_dim, hidden_dim

    def forward(self, z, label_onehot):
        check_dims(self.z_dim, self.hidden_dim, self.label_dim)
        on_gpu(self, z)
        no_autograd(self, z, label_onehot)
        return gan_forward(self, 0, z, label_onehot, label_dim=self.label_dim)


class Discriminator(FlatModule):
    """:48-60.  forward(x, label_onehot) -> probabilities [R][1]."""

    def __init__(self, label_dim, hidden_dim):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(2 + label_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1), nn.Sigmoid())
        self.label_dim, self.hidden_dim = label_dim, hidden_dim

    def forward(self, x, label_onehot):
        check_dims(4, self.hidden_dim, self.label_dim)
        on_gpu(self, x)
        no_autograd(self, x, label_onehot)
        return gan_forward(self, 1, x, label_onehot, label_dim=self.label_dim)


def one_hot_encode(labels, num_classes):
    """:62-63 F.one_hot(labels, num_classes).float(), through pcg_onehot: [n] int64 on the GPU -> [n][num_classes] float32."""
    if not labels.is_cuda:
        raise PcgError(f"one_hot_encode: labels are on {labels.device}; libpcgan_hip has no CPU path")
    return ops.onehot(labels.to(torch.int64).contiguous(), num_classes)


def make_optimizers(generator, discriminator, cfg=config):
    return Adam(generator.parameters(), lr=cfg["lr"]), Adam(discriminator.parameters(), lr=cfg["lr"])          # :77-78


def train(real_samples, real_labels, generator, discriminator, config, *, optimizers=None, draws=None, perm=None, seed=0, verbose=True):
    """The script's training loop (:81-135) as a function; returns (loss_D_values, loss_G_values), the per-epoch sums of :131-132.

      :77-78   `optimizers` = (optimizer_G, optimizer_D), built by make_optimizers when not given
      :85-86   indices = np.random.permutation(n_samples); the samples and labels are re-indexed cumulatively, epoch after epoch (the
               caller's tensors are not modified: the script rebinds its names).  The set is uploaded once; the epoch's order goes to
               the kernel as row indices.  `perm(epoch) -> [N] indices` replaces numpy's draw for parity runs.
      :90-129  ONE launch of pcg_moons_gan_train_steps for all n_samples / batch_size iterations.  The noise of the epoch is ONE randn
               launch and the G step's labels ONE randint launch of an ops.DeviceRNG seeded with `seed`.  The D step's fake labels
               are drawn with randint(0, 1) at :98, i.e. always class 0: that is kept.  `draws(epoch, batch_idx) -> (z_d, labels_d,
               z_g, labels_g)` supplies all four instead.
      :134-135 the print every 100 epochs (verbose)
    Where D saturates the reference's bare torch.log gives inf / nan; the kernel forms the losses from D's logit and stays finite
    (moons.TrainSteps).  The parameters' .grad are not specified afterwards."""
    X = np.asarray(torch.as_tensor(real_samples).detach().cpu().numpy(), dtype=np.float32)
    Y = np.asarray(torch.as_tensor(real_labels).detach().cpu().numpy(), dtype=np.int64)
    B, N = int(config["batch_size"]), X.shape[0]
    check_epoch(N, B)
    for net in (generator, discriminator):
        if next(net.parameters()).device.type != "cuda":
            raise PcgError(f"moons_cgan.train: the nets are on {next(net.parameters()).device}; libpcgan_hip has no CPU path")
    optimizer_G, optimizer_D = optimizers if optimizers is not None else make_optimizers(generator, discriminator, config)
    runner = TrainSteps(generator, discriminator, optimizer_G, optimizer_D, X, Y, batch_size=B)
    if runner.label_dim != config["label_dim"]:
        raise PcgError(f"moons_cgan.train: the nets were built for label_dim {runner.label_dim}, config says {config['label_dim']}")
    order = np.arange(N)

    def order_of(epoch):
        nonlocal order
        indices = np.random.permutation(N) if perm is None else np.asarray(perm(epoch))     # :85
        order = order[indices]                                                              # :86
        return order

    def on_epoch(epoch, lD, lG):
        if verbose and epoch % 100 == 0:                                                    # :134
            print(f"Epoch [{epoch}/{config['epochs']}], Loss D: {lD:.4f}, Loss G: {lG:.4f}")

    return run_epochs(runner, config["epochs"], N // B, order_of, draws, ops.DeviceRNG(seed=seed), on_epoch)


def sample(generator, n, labels=None, z=None, seed=0):
    """save_generated_data's draws (:151-155): (samples [n][2], labels [n]); labels / z given or drawn from ops.DeviceRNG(seed)."""
    dev = next(generator.parameters()).device
    rng = ops.DeviceRNG(seed=seed)
    if z is None:
        z = rng.randn((n, generator.z_dim), dev)
    if labels is None:
        labels = rng.randint(0, generator.label_dim, n, dev)
    labels = labels.to(dev, torch.int64)
    with torch.no_grad():
        return generator(z, one_hot_encode(labels, generator.label_dim)), labels
