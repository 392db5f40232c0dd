"""optim.Adam / AdamW: state_dict() / load_state_dict() in torch's format, both directions, on the device.

The net is a FlatModule with a Conv2d(3, 5, 3) -- its 4-D weight is a permuted view of the flat buffer (physical [o, kh, kw, i]) --
a Linear(7, 3) whose element counts (21, 3) are no multiples of 4, so the pad4 gaps lie inside the one segment, and a Linear(3, 1)
with a one-element bias.  Gradients are fixed random tensors, one set per step: the moments of the conv weight are not symmetric
under the two layouts, so a layout slip is an O(1) error.  Tolerances against torch are those of tests/test_hip_ops.py::test_adam."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CASES = [("Adam", {"betas": (0.5, 0.999)}), ("AdamW", {"betas": (0.0, 0.9), "weight_decay": 0.01})]
LR = 2e-3


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd


def dev():
    return torch.device("cuda:0")


def _layers(m):
    m.conv, m.l1, m.l2 = nn.Conv2d(3, 5, 3), nn.Linear(7, 3), nn.Linear(3, 1)


class TorchNet(nn.Module):
    def __init__(self):
        super().__init__()
        _layers(self)


def make_net(values):
    from pcgan_amd.nn import FlatModule

    class Net(FlatModule):
        def __init__(self):
            super().__init__()
            _layers(self)

    net = Net()
    net.load_state_dict(values)
    net.to(dev())
    net.zero_grad()                                           # flattens; attaches the .grad views
    return net


@pytest.fixture(scope="module")
def fixed():
    """Initial values and five sets of gradients (CPU), shared and never written."""
    torch.manual_seed(11)
    ref = TorchNet()
    values = {k: v.clone() for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    grads = [[torch.randn(p.shape, generator=g) for p in ref.parameters()] for _ in range(5)]
    return values, grads


def step_ours(net, opt, grads):
    for p, g in zip(net.parameters(), grads):
        p.grad.copy_(g)
    opt.step()


def torch_side(fixed, name, kw, steps):
    values, grads = fixed
    net = TorchNet()
    net.load_state_dict(values)
    opt = getattr(torch.optim, name)(net.parameters(), lr=LR, **kw)
    for s in range(steps):
        for p, g in zip(net.parameters(), grads[s]):
            p.grad = g.clone()
        opt.step()
    return net, opt


def ours_side(pcg, fixed, name, kw, steps):
    from pcgan_amd import optim
    values, grads = fixed
    net = make_net(values)
    opt = getattr(optim, name)(net.parameters(), lr=LR, **kw)
    for s in range(steps):
        step_ours(net, opt, grads[s])
    return net, opt


@pytest.mark.parametrize("name,kw", CASES)
def test_ours_to_torch(pcg, fixed, name, kw):
    net, opt = ours_side(pcg, fixed, name, kw, 3)
    assert opt.num_segments() == 1                             # the padding gaps are inside the segment
    sd = opt.state_dict()
    tnet, topt = torch_side(fixed, name, kw, 3)
    want = topt.state_dict()
    assert sorted(sd["state"]) == sorted(want["state"]) == list(range(6))
    for i, p in enumerate(tnet.parameters()):
        s = sd["state"][i]
        assert s["step"].dtype == torch.float32 and s["step"].dim() == 0 and float(s["step"]) == 3.0
        for k, atol in (("exp_avg", 1e-7), ("exp_avg_sq", 1e-9)):
            assert s[k].is_cuda and s[k].is_contiguous() and s[k].shape == p.shape
            np.testing.assert_allclose(s[k].cpu().numpy(), want["state"][i][k].numpy(), rtol=1e-5, atol=atol, err_msg=f"{k} of parameter {i}")
    # the dict loads into the torch optimizer over a CPU copy of the module, and torch's next step runs
    cpu_sd = {"state": {i: {k: v.cpu() for k, v in s.items()} for i, s in sd["state"].items()}, "param_groups": sd["param_groups"]}
    fresh = getattr(torch.optim, name)(tnet.parameters(), lr=LR, **kw)
    fresh.load_state_dict(cpu_sd)
    for p, g in zip(tnet.parameters(), fixed[1][3]):
        p.grad = g.clone()
    fresh.step()
    assert float(fresh.state_dict()["state"][0]["step"]) == 4.0


@pytest.mark.parametrize("name,kw", CASES)
def test_torch_to_ours(pcg, fixed, name, kw):
    tnet, topt = torch_side(fixed, name, kw, 3)
    net, opt = ours_side(pcg, fixed, name, kw, 0)
    net.load_state_dict(tnet.state_dict())
    opt.load_state_dict(topt.state_dict())                    # before its first step: pending until the segments exist
    assert opt._segments is None and float(opt.state_dict()["state"][0]["step"]) == 3.0
    step_ours(net, opt, fixed[1][3])
    for p, g in zip(tnet.parameters(), fixed[1][3]):
        p.grad = g.clone()
    topt.step()
    for (k, p), q in zip(net.named_parameters(), tnet.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0


@pytest.mark.parametrize("name,kw", CASES)
def test_ours_to_ours(pcg, fixed, name, kw):
    net5, opt5 = ours_side(pcg, fixed, name, kw, 5)
    net3, opt3 = ours_side(pcg, fixed, name, kw, 3)
    sd, values = opt3.state_dict(), {k: v.cpu() for k, v in net3.state_dict().items()}
    net, opt = ours_side(pcg, fixed, name, kw, 0)             # a fresh module and a fresh optimizer
    net.load_state_dict(values)
    opt.load_state_dict(sd)
    for s in (3, 4):
        step_ours(net, opt, fixed[1][s])
    assert torch.equal(net.flat_params, net5.flat_params)
    a, b = opt.state_dict()["state"], opt5.state_dict()["state"]
    assert sorted(a) == sorted(b) == list(range(6))
    for i in a:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[i][k], b[i][k]), (i, k)
    assert float(a[0]["step"]) == 5.0
    for sa, sb in zip(opt._segments[0], opt5._segments[0]):
        assert torch.equal(sa["step"], sb["step"]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


@pytest.mark.parametrize("name,kw", CASES)
def test_live_load_keeps_the_addresses(pcg, fixed, name, kw):
    _, src = ours_side(pcg, fixed, name, kw, 3)
    net, opt = ours_side(pcg, fixed, name, kw, 1)             # built: a captured graph would hold these addresses
    segs = [st for b in opt._segments for st in b]
    before = [(st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()) for st in segs]
    opt.load_state_dict(src.state_dict())
    segs2 = [st for b in opt._segments for st in b]
    assert [(st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()) for st in segs2] == before
    assert opt._pending is None
    for sa, sb in zip(segs2, [st for b in src._segments for st in b]):
        assert torch.equal(sa["step"], sb["step"]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    # a state without entries (a never-stepped optimizer's) puts a built one back to 'never stepped', still in place
    _, empty = ours_side(pcg, fixed, name, kw, 0)
    opt.load_state_dict(empty.state_dict())
    assert int(segs2[0]["step"].item()) == 0 and not segs2[0]["exp_avg"].any() and opt.state_dict()["state"] == {}


@pytest.mark.parametrize("name,kw", CASES)
def test_snapshot_keeps_a_pending_state(pcg, fixed, name, kw):
    """What every Graphed*Step does around its warm-up: snapshot(), real steps, restore()."""
    _, src = ours_side(pcg, fixed, name, kw, 3)
    sd = src.state_dict()
    net, opt = ours_side(pcg, fixed, name, kw, 0)
    opt.load_state_dict(sd)
    snap = opt.snapshot()
    for s in (3, 4):                                          # two throw-away steps: the first builds the segments
        step_ours(net, opt, fixed[1][s])
    assert float(opt.state_dict()["state"][0]["step"]) == 5.0
    opt.restore(snap)
    back = opt.state_dict()["state"]
    for i in sd["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back[i][k], sd["state"][i][k]), (i, k)
