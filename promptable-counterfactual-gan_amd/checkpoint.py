"""Everything that decides a run's next iteration, in one file.

    state = checkpoint.capture(netG=netG, netD=netD, opt_g=opt_g, opt_d=opt_d, rng=rng, epoch=3, history={"d_losses": [...]})
    checkpoint.save(path, state)
    ...
    values = checkpoint.restore(checkpoint.load(path), netG=netG, netD=netD, opt_g=opt_g, opt_d=opt_d, rng=rng)
    epoch, history = values["epoch"], values["history"]

Objects: nn.Module (its state_dict, loaded strictly), optimizers (pcgan_amd.optim.Adam / AdamW in torch's format, or any
torch.optim.Optimizer), ops.DeviceRNG, data.DeviceLoader, tensors (copied back in place), and plain values: numbers, strings, None,
lists and str-keyed dicts of them, which restore() returns (a list or dict handed to restore() is also refilled in place).  torch's
CPU RNG state and numpy's global RNG state are always stored and put back, and so is a format version.

The file is ONE torch.save dict of CPU tensors and plain values: it loads with torch.load(path, weights_only=True), and it is
written under a temporary name and moved into place with os.replace, so an interrupted write leaves the previous file whole.
A state that was captured can be restored without the file (`resume=` of the trainers takes the dict as well as the path).

Host code only: capture() reads the device (one copy per tensor), restore() writes it; neither launches a kernel of the library.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import PcgError
from .data import DeviceLoader

FORMAT_VERSION = 1


def _cpu(v):
    """Tensors anywhere in a nest of dicts / lists / tuples -> detached contiguous CPU copies; everything else as it is."""
    if torch.is_tensor(v):
        return v.detach().to("cpu", copy=True).contiguous()
    if isinstance(v, dict):
        return {k: _cpu(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_cpu(x) for x in v)
    return v


def _plain(v, name):
    """A copy of a plain value: numbers, strings, None, lists (tuples become lists) and str-keyed dicts of them."""
    if isinstance(v, (np.integer, np.floating, np.bool_)):    # first: np.float64 is a float, and no plain value to weights_only=True
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [_plain(x, name) for x in v]
    if isinstance(v, dict) and all(isinstance(k, str) for k in v):
        return {k: _plain(x, name) for k, x in v.items()}
    raise PcgError(f"checkpoint.capture: {name}: a {type(v).__name__} is none of nn.Module, optimizer, DeviceRNG, DeviceLoader, tensor, "
                   "number, string, list or str-keyed dict of those plain values")


def _capture_one(name, obj):
    if isinstance(obj, torch.nn.Module):
        return {"kind": "module", "state": _cpu(dict(obj.state_dict()))}
    if isinstance(obj, torch.optim.Optimizer):
        return {"kind": "optimizer", "state": _cpu(obj.state_dict())}
    if isinstance(obj, ops.DeviceRNG):
        return {"kind": "rng", "state": obj.get_state()}
    if isinstance(obj, DeviceLoader):
        return {"kind": "loader", "state": _cpu(obj.state_dict())}
    if torch.is_tensor(obj):
        return {"kind": "tensor", "value": _cpu(obj)}
    return {"kind": "value", "value": _plain(obj, name)}


def capture(**objects):
    """The state of the named objects plus torch's CPU and numpy's global RNG state, as one dict of CPU tensors and plain values."""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"format_version": FORMAT_VERSION,
            "torch_rng": torch.get_rng_state().clone(),
            "numpy_rng": {"kind": str(kind), "keys": [int(k) for k in keys], "pos": int(pos), "has_gauss": int(has_gauss),
                          "cached_gaussian": float(cached)},
            "objects": {name: _capture_one(name, obj) for name, obj in objects.items()}}


def _check_version(state, who):
    if not isinstance(state, dict) or "format_version" not in state or "objects" not in state:
        raise PcgError(f"{who}: not a checkpoint written by pcgan_amd.checkpoint (no format_version)")
    if state["format_version"] != FORMAT_VERSION:
        raise PcgError(f"{who}: checkpoint format version {state['format_version']}, this build reads version {FORMAT_VERSION}")


def restore(state, **objects):
    """Put a captured state back into the named objects (each must have been captured under that name, as the same kind) and into
    torch's CPU and numpy's global RNG.  Modules, optimizers, the DeviceRNG, the DeviceLoader and tensors are written in place.
    Returns {name: value} of EVERY plain value the state holds, named here or not."""
    _check_version(state, "checkpoint.restore")
    stored = state["objects"]
    for name, obj in objects.items():
        if name not in stored:
            raise PcgError(f"checkpoint.restore: the checkpoint holds no {name!r} (it holds {sorted(stored)})")
        ent = stored[name]
        want = _capture_kind(obj)
        if ent["kind"] != want:
            raise PcgError(f"checkpoint.restore: {name!r} was captured as a {ent['kind']}, and a {want} ({type(obj).__name__}) is to take it")
        if want == "module":
            obj.load_state_dict(ent["state"], strict=True)
        elif want == "optimizer":
            obj.load_state_dict(ent["state"])
        elif want == "rng":
            obj.set_state(ent["state"])
        elif want == "loader":
            obj.load_state_dict(ent["state"])
        elif want == "tensor":
            if tuple(obj.shape) != tuple(ent["value"].shape) or obj.dtype != ent["value"].dtype:
                raise PcgError(f"checkpoint.restore: tensor {name!r} is {tuple(obj.shape)} {obj.dtype}, the stored one "
                               f"{tuple(ent['value'].shape)} {ent['value'].dtype}")
            with torch.no_grad():
                obj.copy_(ent["value"])
        elif isinstance(obj, list):
            obj[:] = _plain(ent["value"], name)
        elif isinstance(obj, dict):
            obj.clear(); obj.update(_plain(ent["value"], name))
    torch.set_rng_state(torch.as_tensor(state["torch_rng"], dtype=torch.uint8).cpu())
    n = state["numpy_rng"]
    np.random.set_state((n["kind"], np.asarray(n["keys"], dtype=np.uint32), int(n["pos"]), int(n["has_gauss"]), float(n["cached_gaussian"])))
    return {name: _plain(ent["value"], name) for name, ent in stored.items() if ent["kind"] == "value"}


def _capture_kind(obj):
    if isinstance(obj, torch.nn.Module):
        return "module"
    if isinstance(obj, torch.optim.Optimizer):
        return "optimizer"
    if isinstance(obj, ops.DeviceRNG):
        return "rng"
    if isinstance(obj, DeviceLoader):
        return "loader"
    return "tensor" if torch.is_tensor(obj) else "value"


def value(state, name, default=None):
    """A stored plain value, without restoring anything."""
    ent = state["objects"].get(name)
    return _plain(ent["value"], name) if ent is not None and ent["kind"] == "value" else default


def save(path, state):
    """One torch.save file, written under a temporary name next to `path` and moved into place (os.replace)."""
    _check_version(state, "checkpoint.save")
    path = os.fspath(path)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load(path):
    """The dict save() wrote, on the CPU, through torch.load(weights_only=True)."""
    state = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    _check_version(state, f"checkpoint.load({os.fspath(path)!r})")
    return state


# ---- what the trainers share (dcgan.train, house.train_countergan, moons_countergan.train_countergan, gan_train.train_gan) ------------
def open_resume(resume, who, **run):
    """`resume` (a path or a loaded dict) -> the state, after comparing the run's fields (batch_size, n_rows, seed) with the stored ones:
    a checkpoint continues the run it was written by, and a mismatch is refused by the field's name."""
    state = load(resume) if isinstance(resume, (str, os.PathLike)) else resume
    _check_version(state, who)
    stored = value(state, "run", {})
    for k, v in run.items():
        if k not in stored or stored[k] != _plain(v, k):
            raise PcgError(f"{who}: resume: {k} is {v!r} here, but the checkpoint was written with {k} = {stored.get(k)!r}")
    return state


def loader_rows(loader):
    """The number of training rows behind a loader, where it says (a DeviceLoader, a torch DataLoader), else None."""
    if isinstance(loader, DeviceLoader):
        return int(loader.x.shape[0])
    try:
        return len(loader.dataset)
    except (AttributeError, TypeError):
        return None


def due(checkpoint, checkpoint_every, epoch):
    """Whether the trainers write `checkpoint` after this (0-based) epoch."""
    return checkpoint is not None and (epoch + 1) % int(checkpoint_every) == 0


def check_args(who, checkpoint, checkpoint_every, resume):
    if checkpoint is not None and int(checkpoint_every) < 1:
        raise PcgError(f"{who}: checkpoint_every = {checkpoint_every}")
    if resume is not None and not isinstance(resume, (str, os.PathLike, dict)):
        raise PcgError(f"{who}: resume is a path or a loaded checkpoint dict, not a {type(resume).__name__}")
