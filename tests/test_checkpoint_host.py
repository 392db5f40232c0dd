"""Host side of resuming a run, no GPU: the torch-format state of optim.Adam / AdamW over CPU parameters (a loaded
state waits, pending, for segments that only a GPU step would build), the checkpoint file, the random streams, and the refusals."""
import numpy as np
import pytest
import torch

import pcgan_amd
from pcgan_amd import PcgError, checkpoint, ops
from pcgan_amd.data import DeviceLoader
from pcgan_amd.optim import Adam, AdamW


def _torch_state(torch_cls, **kw):
    """A torch optimizer's state after three steps on two parameters, and the parameters."""
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(3, 4, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]
    opt = torch_cls(params, lr=1e-2, **kw)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict(), params


def _same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"])
    for i in a["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i])
        for k, v in a["state"][i].items():
            w = b["state"][i][k]
            assert v.dtype == w.dtype and v.shape == w.shape and torch.equal(v, w), (i, k)


@pytest.mark.parametrize("torch_cls,cls,kw", [(torch.optim.Adam, Adam, {"betas": (0.5, 0.999)}),
                                               (torch.optim.AdamW, AdamW, {"betas": (0.0, 0.9), "weight_decay": 0.01})])
def test_state_round_trip(torch_cls, cls, kw):
    sd, params = _torch_state(torch_cls, **kw)
    assert len(sd["state"]) == 2 and float(sd["state"][0]["step"]) == 3.0
    opt = cls([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-2, **kw)
    assert opt.state_dict()["state"] == {}                    # never stepped: no entry, as in torch
    opt.load_state_dict(sd)
    back = opt.state_dict()
    _same_state(sd, back)                                     # bit for bit, with torch's param_groups keys
    assert opt.state == {}                                    # the moments never live in self.state
    # what comes back is a copy: writing into it does not reach the pending state
    back["state"][0]["exp_avg"].zero_()
    _same_state(sd, opt.state_dict())
    # ... and it loads into torch, whose next step runs
    t2 = torch_cls(params, lr=1e-2, **kw)
    t2.load_state_dict(opt.state_dict())
    for p in params:
        p.grad = torch.ones_like(p)
    t2.step()
    assert float(t2.state_dict()["state"][0]["step"]) == 4.0


def test_param_groups_carry_torch_defaults():
    for cls, torch_cls in ((Adam, torch.optim.Adam), (AdamW, torch.optim.AdamW)):
        g = cls([torch.nn.Parameter(torch.zeros(3))], lr=3e-4).state_dict()["param_groups"][0]
        want = torch_cls([torch.zeros(1)]).defaults
        assert set(want) <= set(g) and g["amsgrad"] is False and g["maximize"] is False and g["lr"] == 3e-4
        assert g["params"] == [0]


def test_snapshot_restore_keep_a_pending_state():
    sd, params = _torch_state(torch.optim.Adam)
    opt = Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-2)
    opt.load_state_dict(sd)
    snap = opt.snapshot()
    assert snap is not None                                   # None would make the graphed steppers zero the moments after warm-up
    opt._pending = None                                       # what the warm-up's first step does when it builds the segments
    opt.restore(snap)
    _same_state(sd, opt.state_dict())


def _segment_of_two():
    """Two CPU parameters that are adjacent in one flat buffer, gradients likewise: ONE segment, as FlatModule lays nets out."""
    flat, gflat = torch.zeros(8), torch.zeros(8)
    a, b = torch.nn.Parameter(flat[0:3]), torch.nn.Parameter(flat[4:8])
    a.grad, b.grad = gflat[0:3], gflat[4:8]
    return Adam([a, b])


def _entry(step, n):
    return {"step": torch.tensor(float(step)), "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}


def _groups(**kw):
    return [dict(torch.optim.Adam([torch.zeros(1)]).defaults, params=[0, 1], **kw)]


@pytest.mark.parametrize("state,groups,names", [
    ({}, _groups(amsgrad=True), "amsgrad"),
    ({}, _groups(maximize=True), "maximize"),
    ({0: _entry(3, 3), 1: _entry(2, 4)}, _groups(), "differing step"),
    ({0: _entry(3, 3), 1: _entry(3, 5)}, _groups(), "shape mismatch"),
    ({0: _entry(3, 3)}, _groups(), "some but not all parameters of a segment"),
])
def test_refusals(state, groups, names):
    opt = _segment_of_two()
    with pytest.raises(PcgError, match=names):
        opt.load_state_dict({"state": state, "param_groups": groups})
    assert opt.state_dict()["state"] == {}                    # a refused state is not kept
    opt.load_state_dict({"state": {0: _entry(3, 3), 1: _entry(3, 4)}, "param_groups": _groups()})
    assert sorted(opt.state_dict()["state"]) == [0, 1]


def test_constructor_still_refuses_amsgrad():
    with pytest.raises(PcgError, match="amsgrad"):
        Adam([torch.nn.Parameter(torch.zeros(2))], amsgrad=True)


def test_file_round_trip(tmp_path):
    sd, params = _torch_state(torch.optim.Adam)
    opt = Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-2)
    opt.load_state_dict(sd)
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    rng = ops.DeviceRNG(seed=2**63 + 11)
    rng.offset = 12345
    t = torch.arange(6, dtype=torch.float32).view(2, 3)
    hist = {"d_losses": [0.5, 0.25], "g_losses": [1.0, np.float64(2.0)]}
    state = checkpoint.capture(net=net, opt=opt, rng=rng, t=t, epoch=2, note="abc", history=hist)
    path = tmp_path / "run.pt"
    checkpoint.save(path, state)
    assert [p.name for p in tmp_path.iterdir()] == ["run.pt"]                 # the temporary name is gone
    raw = torch.load(path, weights_only=True)                                 # CPU tensors and plain values only
    assert raw["format_version"] == checkpoint.FORMAT_VERSION
    loaded = checkpoint.load(path)
    net2 = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    opt2 = Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-2)
    rng2, t2 = ops.DeviceRNG(seed=0), torch.zeros(2, 3)
    vals = checkpoint.restore(loaded, net=net2, opt=opt2, rng=rng2, t=t2)
    assert vals == {"epoch": 2, "note": "abc", "history": {"d_losses": [0.5, 0.25], "g_losses": [1.0, 2.0]}}
    for (k, v), (k2, v2) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    _same_state(sd, opt2.state_dict())
    assert rng2.get_state() == {"seed": 2**63 + 11, "offset": 12345} and torch.equal(t, t2)
    # strict: a module with other keys is refused by load_state_dict
    with pytest.raises(RuntimeError):
        checkpoint.restore(loaded, net=torch.nn.Linear(3, 2))
    with pytest.raises(PcgError, match="'nothing'"):
        checkpoint.restore(loaded, nothing=net2)
    with pytest.raises(PcgError, match="format version"):
        checkpoint.restore(dict(loaded, format_version=99))
    with pytest.raises(PcgError, match="set"):
        checkpoint.capture(bad={1, 2})


def test_rng_streams_are_restored():
    torch.manual_seed(7); np.random.seed(7)
    torch.randperm(10); np.random.rand(3)
    loader = DeviceLoader(torch.zeros(10, 2), torch.zeros(10), 4, shuffle=True, seed=3)
    loader.epoch_order()
    state = checkpoint.capture(loader=loader)
    want = torch.randperm(50), np.random.rand(4), loader.epoch_order()
    torch.randperm(9); np.random.rand(2); loader.epoch_order()               # the streams move on
    checkpoint.restore(state, loader=loader)
    assert torch.equal(torch.randperm(50), want[0])                          # the next torch.randperm repeats
    assert np.array_equal(np.random.rand(4), want[1])
    assert torch.equal(loader.epoch_order(), want[2])


def test_device_rng_state():
    rng = ops.DeviceRNG(seed=42)
    rng.offset = 7
    other = ops.DeviceRNG(seed=1)
    other.set_state(rng.get_state())
    assert (other.seed, other.offset) == (42, 7)
    with pytest.raises(PcgError, match="offset"):
        other.set_state({"seed": 1, "offset": -1})


def test_resume_refuses_another_run():
    state = checkpoint.capture(epoch=1, run={"batch_size": 64, "n_rows": 200, "seed": 42})
    assert checkpoint.open_resume(state, "trainer", batch_size=64, n_rows=200, seed=42) is state
    for field, v in (("batch_size", 32), ("n_rows", 100), ("seed", 1)):
        with pytest.raises(PcgError, match=field):
            checkpoint.open_resume(state, "trainer", **dict({"batch_size": 64, "n_rows": 200, "seed": 42}, **{field: v}))


def test_dcgan_refuses_checkpoints_of_a_data_parallel_run():
    from pcgan_amd import dcgan
    for kw in ({"checkpoint": "x.pt"}, {"resume": "x.pt"}):
        with pytest.raises(PcgError, match="data-parallel"):
            dcgan.train([], netG=object(), netD=object(), dp=object(), **kw)
