"""What the whole-epoch-per-launch trainers share on the host side (moons.TrainSteps over csrc/moons_gan.hip, moons_countergan.TrainSteps
over csrc/moons_cf.hip; the device side they share is csrc/epoch_wg.h): the refusals, the Adam part of the descriptor, and the
flat-parameter / Adam-state / scratch part of the argument struct, whose field names are the same in both ABIs."""
import numpy as np
import torch

from ._lib import PcgError
from .optim import Adam


def no_autograd(net, *xs):
    if torch.is_grad_enabled() and (any(p.requires_grad for p in net.parameters()) or any(x is not None and x.requires_grad for x in xs)):
        raise PcgError(f"{type(net).__name__}: the fused forward has no autograd backward: call it under torch.no_grad() (or with "
                       "requires_grad off); train through the module's train function / TrainSteps")


def on_gpu(net, x):
    net._ensure_flat()
    if not x.is_cuda:
        raise PcgError(f"{type(net).__name__}: input is on {x.device}; libpcgan_hip has no CPU path")


def check_adam_pair(opt_G, opt_D):
    """What the kernels' Adam cannot do, refused without touching a device."""
    for opt, what in ((opt_G, "opt_G"), (opt_D, "opt_D")):
        if type(opt) is not Adam:
            raise PcgError(f"{what}: the fused step implements pcgan_amd.optim.Adam only")
        if any(g["weight_decay"] != 0.0 for g in opt.param_groups):
            raise PcgError(f"{what}: weight decay is not implemented in the fused step (the reference uses none)")
    gg, gd = opt_G.param_groups[0], opt_D.param_groups[0]
    if tuple(gg["betas"]) != tuple(gd["betas"]) or gg["eps"] != gd["eps"]:
        raise PcgError("TrainSteps: opt_G and opt_D must share betas and eps")


def one_gpu(*nets, who="TrainSteps"):
    """The nets' common device, read from their parameters (nothing is flattened or moved): one GPU, or a refusal in `who`'s name."""
    devs = {next(net.parameters()).device for net in nets}
    if len(devs) != 1:
        raise PcgError(f"{who}: the nets must be on one GPU, got {sorted(map(str, devs))}")
    dev = devs.pop()
    if dev.type != "cuda":
        raise PcgError(f"{who}: the nets are on {dev}; libpcgan_hip has no CPU path")
    return dev


def resident(a, dtype, dev):
    """The training set (or its labels) in HBM for the lifetime of the trainer."""
    return torch.as_tensor(np.asarray(a), dtype=dtype).contiguous().to(dev)


def alloc_scratch(nbytes, dev):
    """The activation scratch a pcg_*_scratch_bytes query asked for (0: the activations fit in LDS; the buffer is then never read)."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev), nbytes


def fill_adam_desc(d, opt_G, opt_D, seg_G, seg_D):
    """Read per launch: a changed learning rate (param_groups) takes effect at the next one."""
    gg, gd = opt_G.param_groups[0], opt_D.param_groups[0]
    d.nG_adam, d.nD_adam = seg_G["n"], seg_D["n"]
    d.lr_G, d.lr_D = float(gg["lr"]), float(gd["lr"])
    d.beta1, d.beta2, d.adam_eps = float(gg["betas"][0]), float(gg["betas"][1]), float(gg["eps"])


def fill_state_args(a, G, D, seg_G, seg_D, scratch, scratch_bytes):
    a.g_flat, a.d_flat = G.flat_params.data_ptr(), D.flat_params.data_ptr()
    a.g_exp_avg, a.g_exp_avg_sq, a.g_step = seg_G["exp_avg"].data_ptr(), seg_G["exp_avg_sq"].data_ptr(), seg_G["step"].data_ptr()
    a.d_exp_avg, a.d_exp_avg_sq, a.d_step = seg_D["exp_avg"].data_ptr(), seg_D["exp_avg_sq"].data_ptr(), seg_D["step"].data_ptr()
    a.scratch, a.scratch_bytes = (scratch.data_ptr() if scratch_bytes else None), scratch_bytes
