"""GPU: the additive-delta MNIST CounteRGAN step (pcgan_amd.gan_train) against the reference's recorded runs
(tests/golden/delta_gan_ref.npz, written by tests/golden/make_golden_delta_gan.py) and the float64 restatement
(tests/delta_gan_restate.py).

The rule.  A quantity passes against float64 if (a) rtol 1e-4, atol 2e-5 * max|reference|, or (b) it is within 3x the recorded
distance of the reference's own fp32 run from its float64 run.  Parameter gradients are compared with the float64 restatement whose
classifier routing (max-pool positions idx1 / idx2, ReLU masks p > 0 and h > 0) is pinned to the routing the GPU used; that routing
must itself equal the float64 run's wherever §3.18's gap bound decides, and at most 0.2 % of a layer's live windows may fall under it.
Parameters after Adam are not compared with float64 directly (Adam's sign noise on near-zero gradients: up to 5e-4 * max|p| between
the reference's own two runs); instead every step's new parameters must equal a float64 Adam update of the GPU's own previous
parameters and state with the GPU's own gradients, to the tolerance of tests/test_hip_ops.py::test_adam (rtol 1e-6, atol 1e-7), and
the losses of steps 2 and 3 must match the float64 recording by rule (a) -- a step that failed to update D, or fed the G step the stale
label map, moves loss_D / loss_adv far outside it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_gan_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR_CAP = 0.002
PATHS = ("chain", "eager", "graph")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "delta_gan_ref.npz")))


@pytest.fixture(scope="module")
def T():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import gan_train
    return gan_train


def _nets(T):
    from pcgan_amd import countergan as K
    torch.manual_seed(RS.SEED_GAN)
    G, D = T.Generator(), T.Discriminator()
    C = K.Classifier()
    C.load_state_dict(PR.seeded_state(PR.SEED), strict=True)
    return G.to(DEV), D.to(DEV), C.to(DEV).eval()


def _params(**kw):
    from pcgan_amd import gan_train
    return dict(gan_train.params, **kw)


def _grads(net):
    return {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}


def _routing(C, x_cf):
    """The classifier routing the GPU uses on x_cf (NCHW, CPU): (idx1, p1 > 0, idx2, p2 > 0, h > 0).  The kernels are deterministic, so
    this forward repeats the one inside the step bit for bit."""
    _, saved = C._run_forward(x_cf, keep=True)
    B = x_cf.shape[0]
    return (PR.nchw(saved["idx1"].cpu()), PR.nchw(saved["p1"].cpu()) > 0, PR.nchw(saved["idx2"].cpu()), PR.nchw(saved["p2"].cpu()) > 0,
            saved["h"].cpu().view(B, 128) > 0)


_cache = {}


def _step1(T, B, path):
    """Step 1 from the fixture's state through one path; everything the tests read, as CPU tensors."""
    if (B, path) in _cache:
        return _cache[(B, path)]
    G, D, C = _nets(T)
    x, y = RS.batches(B)[0]
    xd, yd = x.to(DEV), y.to(DEV)
    td = torch.full_like(yd, RS.TARGET_CLASS)
    with torch.no_grad():                                                       # the forward tensors of the untouched state
        x_cf, delta = G(xd, td)
        fwd = {"x_cf": x_cf.cpu(), "delta": delta.cpu(), "d_real": D(xd, yd).cpu(), "d_fake": D(x_cf, td).cpu(), "cls_logits": C(x_cf).cpu()}
        pins = _routing(C, x_cf)
    if path == "chain":
        opt_g, opt_d = T.make_optimizers(G, D, _params())
        out = T.train_step(G, D, C, opt_g, opt_d, xd, yd, td, _params())
    else:
        stepper = T.GraphedTrainStep(G, D, C, B, _params(), graph=path == "graph")
        out = stepper.step(xd, yd, td)
        b = stepper._bufs[B]
        fused = {"x_cf": b["x_cf"].view(B, 1, 28, 28), "delta": b["h"][3].view(B, 1, 28, 28), "d_real": b["logits_d"][:B].view(B, 1),
                 "d_fake": b["logits_d"][B:].view(B, 1), "d_fake_g": b["logits_g"].view(B, 1), "cls_logits": b["cls_logits"]}
        for k, v in fused.items():
            fwd["step." + k] = v.cpu()
    torch.cuda.synchronize()
    res = {"losses": {k: float(out[k].cpu()) for k in RS.LOSSES}, "fwd": fwd, "pins": pins, "grad_G": _grads(G), "grad_D": _grads(D),
           "nets": (G, D)}                                                      # after the step: D as the G step saw it
    _cache[(B, path)] = res
    return res


def _rule(got, want64, dist, what):
    want64 = np.asarray(want64, np.float64)
    atol = max(2e-5 * float(np.abs(want64).max()), 3.0 * float(np.max(dist)))
    err = float(np.abs(np.asarray(got, np.float64) - want64).max())
    print(f"{what}: max error {err:.3e}, atol {atol:.3e} (rule a {2e-5 * float(np.abs(want64).max()):.3e}, rule b {3.0 * float(np.max(dist)):.3e})")
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=atol, err_msg=what)


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("B", [4, 3])
def test_step_one_losses_and_forward_tensors(T, gold, B, path):
    r = _step1(T, B, path)
    for name in RS.LOSSES:
        _rule(r["losses"][name], gold[f"B{B}.{name}.f64"][0], gold[f"B{B}.{name}.dist"][0], name)
    for name in ("delta", "x_cf", "d_real", "d_fake", "cls_logits"):
        _rule(r["fwd"][name].numpy(), gold[f"B{B}.{name}.f64"], gold[f"B{B}.{name}.dist"], name)
    if path != "chain":                                                         # the step's own buffers, d_fake_g (after Adam(D)) among them
        for name in ("delta", "x_cf", "d_real", "d_fake", "d_fake_g", "cls_logits"):
            _rule(r["fwd"]["step." + name].numpy(), gold[f"B{B}.{name}.f64"], gold[f"B{B}.{name}.dist"], "step " + name)
        assert torch.equal(r["fwd"]["step.x_cf"], r["fwd"]["x_cf"]) and torch.equal(r["fwd"]["step.delta"], r["fwd"]["delta"])


@pytest.mark.parametrize("B", [4, 3])
def test_gpu_routing_is_the_float64_runs_where_it_decides(T, gold, B):
    idx1, live1, idx2, live2, _ = _step1(T, B, "eager")["pins"]
    for layer, idx, livep in ((1, idx1, live1), (2, idx2, live2)):
        live, near = gold[f"B{B}.live{layer}"], gold[f"B{B}.near{layer}"]
        frac = near.sum() / live.sum()
        print(f"B {B} pool {layer}: {int(near.sum())} of {int(live.sum())} live windows under the bound {float(gold[f'B{B}.bound{layer}']):.1e}")
        assert frac <= NEAR_CAP
        pinned = live & ~near
        np.testing.assert_array_equal(idx.numpy()[pinned], gold[f"B{B}.idx{layer}"][pinned])
        assert livep.numpy()[pinned].all()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("B", [4, 3])
def test_step_one_parameter_gradients_against_the_pinned_float64_restatement(T, gold, B, path):
    r = _step1(T, B, path)
    G64, D64 = RS.seeded_nets(torch.float64)
    x, y = RS.batches(B)[0]
    ref = RS.iteration(G64, D64, RS.classifier_state(torch.float64), *RS.make_optimizers(G64, D64), x.double(), y,
                       torch.full_like(y, RS.TARGET_CLASS), pins=r["pins"])    # with its Adam steps: :134 runs on the updated D
    for net, keys in (("G", RS.G_KEYS), ("D", RS.D_KEYS)):
        for k in keys:
            want = ref[f"grad_{net}"][k].numpy()
            assert np.abs(want).max() > 0, (net, k)
            _rule(r[f"grad_{net}"][k].numpy(), want, gold[f"B{B}.grad.{net}.{k}.dist"], f"{path} grad {net} {k}")


@pytest.mark.parametrize("B", [4, 3])
def test_op_chain_and_fused_step_agree_on_step_one_gradients(T, B):
    chain, fused, graph = (_step1(T, B, p) for p in PATHS)
    for net, keys in (("G", RS.G_KEYS), ("D", RS.D_KEYS)):
        for k in keys:
            a, b = chain[f"grad_{net}"][k].numpy(), fused[f"grad_{net}"][k].numpy()
            np.testing.assert_allclose(b, a, rtol=1e-4, atol=2e-5 * float(np.abs(a).max()), err_msg=f"{net} {k}")
            assert torch.equal(fused[f"grad_{net}"][k], graph[f"grad_{net}"][k]), f"replay differs from the eager entries: {net} {k}"
    assert fused["losses"] == graph["losses"]


# ---- Adam wiring over three steps ------------------------------------------------------------------------------------------------------------
def _segments(opt):
    return [st for built in opt._segments for st in built]


@pytest.mark.parametrize("B", [4, 3])
def test_three_steps_adam_wiring_and_losses(T, gold, B):
    G, D, C = _nets(T)
    stepper = T.GraphedTrainStep(G, D, C, B, _params(), graph=True)
    prev = None
    for i, (x, y) in enumerate(RS.batches(B)):
        xd, yd = x.to(DEV), y.to(DEV)
        out = stepper.step(xd, yd, torch.full_like(yd, RS.TARGET_CLASS))
        torch.cuda.synchronize()
        losses = {k: float(out[k].cpu()) for k in RS.LOSSES}
        now = []
        for opt in (stepper.opt_g, stepper.opt_d):
            segs = _segments(opt)
            assert len(segs) == 1, "one flat segment per net"
            st = segs[0]
            assert int(st["step"].cpu()) == i + 1
            now.append({k: st[k].detach().cpu().double().numpy() for k in ("param", "grad", "exp_avg", "exp_avg_sq")})
        if prev is None:                                                         # the state before step 1: the seeded weights, zero moments
            G0, D0, _ = _nets(T)
            prev = [{"param": n.flat_params.cpu().double().numpy()[:len(s["param"])], "exp_avg": 0.0 * s["exp_avg"], "exp_avg_sq": 0.0 * s["exp_avg_sq"]}
                    for n, s in zip((G0, D0), now)]
        for name, p, n in zip("GD", prev, now):
            want_p, want_m, want_v = RS.adam_f64(p["param"], n["grad"], p["exp_avg"], p["exp_avg_sq"], i + 1)
            np.testing.assert_allclose(n["param"], want_p, rtol=1e-6, atol=1e-7, err_msg=f"step {i + 1} {name} parameters")
            np.testing.assert_allclose(n["exp_avg"], want_m, rtol=1e-5, atol=1e-7, err_msg=f"step {i + 1} {name} exp_avg")
            np.testing.assert_allclose(n["exp_avg_sq"], want_v, rtol=1e-5, atol=1e-9, err_msg=f"step {i + 1} {name} exp_avg_sq")
            assert np.abs(n["param"] - p["param"]).max() > 0, f"step {i + 1}: {name} did not move"
        prev = now
        for name in RS.LOSSES:
            want = float(gold[f"B{B}.{name}.f64"][i])
            print(f"step {i + 1} {name}: {losses[name]:.7f}  float64 {want:.7f}  fp32 reference {float(gold[f'B{B}.{name}.f32'][i]):.7f}")
            if i == 0:
                _rule(losses[name], want, gold[f"B{B}.{name}.dist"][0], name)
            else:
                np.testing.assert_allclose(losses[name], want, rtol=1e-4, atol=2e-5 * abs(want), err_msg=f"step {i + 1} {name}")


# ---- graphs, the loop, the pictures -----------------------------------------------------------------------------------------------------------
def _loader():
    gen = torch.Generator().manual_seed(3)
    x = (2 * torch.rand(11, 1, 28, 28, generator=gen) - 1).to(DEV)
    y = torch.randint(0, 10, (11,), generator=gen).to(DEV)
    return [(x[i:i + 4], y[i:i + 4]) for i in range(0, 11, 4)]                   # two full batches and a tail of 3


def _run_epochs(T, graph, epochs):
    G, D, C = _nets(T)
    stepper = T.GraphedTrainStep(G, D, C, 4, _params(), graph=graph)
    rec = []
    for _ in range(epochs):
        for x, y in _loader():
            out = stepper.step(x, y, torch.full_like(y, RS.TARGET_CLASS))
            rec.append(torch.cat([out[k] for k in RS.LOSSES]).clone())
    torch.cuda.synchronize()
    return G.flat_params.clone(), D.flat_params.clone(), torch.stack(rec).cpu(), stepper


def test_replays_equal_the_eager_entries_bit_for_bit_with_a_tail(T):
    g1, d1, l1, s1 = _run_epochs(T, True, 1)
    g0, d0, l0, _ = _run_epochs(T, False, 1)
    assert sorted(s1._graphs) == [3, 4], "one graph per batch size met: the full batch and the tail"
    assert torch.equal(l1, l0), (l1, l0)
    assert torch.equal(g1, g0) and torch.equal(d1, d0)
    assert bool(torch.isfinite(l1).all()) and l1.shape == (3, 5)


def test_train_gan_fused_makes_one_host_read_per_epoch(T, monkeypatch, capsys):
    import warnings
    _, _, want, _ = _run_epochs(T, False, 2)
    G, D, C = _nets(T)
    reads = {"cpu": 0, "item": 0}
    for name in ("cpu", "item"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda self, *a, **k: (reads.__setitem__(name, reads[name] + 1), real(self, *a, **k))[1])(real, name))
    T._fused_fallback_warned = False
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*op chain.*")                 # the reference's nets in fp32 must not fall back
        hist = T.train_gan(G, D, C, _loader(), _params(batch_size=4, epochs_gan=2), fused=True)
    monkeypatch.undo()
    print(f"host reads {reads}; {hist}")
    assert reads == {"cpu": 2, "item": 0}, "one host read per epoch"
    assert capsys.readouterr().out.count("[GAN] Epoch") == 2
    assert hist["d_losses"] == [float(want[2, 0]), float(want[5, 0])] and hist["g_losses"] == [float(want[2, 1]), float(want[5, 1])]


def test_train_gan_falls_back_with_a_warning(T):
    G, D, C = _nets(T)

    class Wider(T.Generator):                                                   # not the reference's generator: the fused step refuses it
        pass

    G2 = Wider()
    G2.load_state_dict(G.state_dict())
    G = G2.to(DEV)
    T._fused_fallback_warned = False
    with pytest.warns(RuntimeWarning, match="op chain"):
        hist = T.train_gan(G, D, C, _loader()[:1], _params(batch_size=4, epochs_gan=1), fused=True, verbose=False)
    assert len(hist["g_losses"]) == 1 and np.isfinite(hist["g_losses"] + hist["d_losses"]).all()


def test_counterfactual_batch_is_the_clamped_forward(T):
    G, _, _ = _nets(T)
    x, y = _loader()[0]
    x = (x * 1.5).contiguous()                                                  # some pixels beyond [-1, 1]: the clamp acts
    t = torch.full_like(y, RS.TARGET_CLASS)
    cf, delta = T.counterfactual_batch(G, x, t)
    with torch.no_grad():
        x_cf, delta2 = G(x, t)
    assert torch.equal(delta, delta2) and torch.equal(cf, torch.clamp(x_cf, -1, 1))
    assert float(x_cf.abs().max()) > 1.0 and float(cf.abs().max()) <= 1.0
    assert not cf.requires_grad and not delta.requires_grad
