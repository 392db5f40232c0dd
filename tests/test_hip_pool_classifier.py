"""GPU: countergan.Classifier, the max-pool MNIST classifier (modules/classifier.py), against the reference's recorded
float64 results (tests/golden/mnist_pool_clf_ref.npz, made by make_golden_mnist_pool_clf.py from the reference's own module) and the
float64 restatement tests/pool_clf_restate.py.

Weights.  A checkpoint of this net is larger than a committed file may be, so the golden runs use the reference's module built after
torch.manual_seed(seed); the tests rebuild those weights from the seed and check them against the recorded per-tensor sums.

Tolerances.  Logits and parameters: the project's rule (_tol of tests/test_hip_mnist_cf_eval.py) -- rtol 1e-4, atol 2e-5 * max|value|, or
3x the CPU fp32 run's own distance from float64 where that is larger.  Predictions: equal wherever the float64 top-two probability gap
exceeds the golden file's `undecided` bound (at most 1 row of 16 may fall under it).
Routing.  idx1 / idx2 equal the float64 run's choice in every live window (float64 maximum > 0) whose float64 top-two gap is at least
max(1e-5, 100 * max|z_fp32 - z_fp64|) of its layer -- both of those runs are the reference's, on the CPU.  At most 0.2 % of a layer's
live windows may fall under that bound; the test fails if more do, it does not mask more.
Input and weight gradients.  A near-tie sends the gradient to another pixel: a discontinuity, not an error.  So gradients are compared
with a float64 backward PINNED to the routing the GPU used (pool_clf_restate.pinned_forward under autograd: windows gathered with the
GPU's idx1 / idx2, multiplied by the GPU's p > 0 and h > 0 masks): rtol 1e-4, atol 2e-5 * max|gradient|.  With the routing test this
pins the whole gradient."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_clf_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR_CAP = 0.002


@pytest.fixture(scope="module")
def K():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import countergan
    return countergan


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mnist_pool_clf_ref.npz")))


@pytest.fixture(scope="module")
def sd(ref):
    sd = R.seeded_state(int(ref["seed"]))
    sums = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    np.testing.assert_allclose(sums, ref["weight_sums"], rtol=1e-12, atol=1e-12, err_msg="the seeded weights are not the golden file's")
    return sd


@pytest.fixture(scope="module")
def net(K, sd):
    C = K.Classifier()
    C.load_state_dict(sd, strict=True)
    return C.to(DEV).eval()


@pytest.fixture(scope="module")
def run(net, ref):
    """One eval forward + input gradient of the 16 golden rows through _run_forward / _run_backward; everything as CPU tensors (NCHW)."""
    x, target = torch.from_numpy(ref["x"]).to(DEV), torch.from_numpy(ref["target"]).to(DEV)
    logits, saved = net._run_forward(x, keep=True)
    dlogits = torch.softmax(logits.double(), 1)
    dlogits[torch.arange(16), target] -= 1.0                                     # d/dlogits of CrossEntropyLoss(reduction="sum")
    dl32 = dlogits.float().contiguous()
    dx = net._run_backward(saved, dl32)
    torch.cuda.synchronize()
    out = {k: R.nchw(saved[k].cpu()) for k in ("p1", "idx1", "p2", "idx2")}
    out.update(h=saved["h"].cpu().view(16, 128), logits=logits.cpu(), dlogits=dl32.cpu(), dx=dx.cpu(), saved=saved)
    return out


def _tol(got, ref64, cpu32, scale):
    """rtol 1e-4, atol 2e-5 * scale -- or 3x the CPU fp32 run's own distance from float64 where that is larger."""
    floor = 3.0 * float(np.abs(np.asarray(cpu32, np.float64) - ref64).max())
    np.testing.assert_allclose(got, ref64, rtol=1e-4, atol=max(2e-5 * scale, floor))


def _pinned(sd, run, x):
    """(float64 state with requires_grad, logits of the forward pinned to the GPU run's routing)."""
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    return sd64, R.pinned_forward(sd64, x, run["idx1"], run["p1"] > 0, run["idx2"], run["p2"] > 0, run["h"] > 0)


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_on_the_device(K, net, sd, tmp_path):
    assert tuple(net.state_dict()) == R.KEYS and len(R.KEYS) == 8
    path = str(tmp_path / "classifier.pt")
    K.save_classifier(net, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(back) == R.KEYS and all(torch.equal(back[k], sd[k]) for k in R.KEYS)
    R.TorchClassifier().load_state_dict(back, strict=True)                      # the reference's layer list takes it
    loaded = K.load_classifier(path, DEV)                                       # strict=True inside
    assert not loaded.training and next(loaded.parameters()).is_cuda
    x = torch.linspace(-1.0, 1.0, 2 * 784, device=DEV).view(2, 1, 28, 28)
    assert torch.equal(loaded(x), net(x))
    assert K.get_pool_classifier(path, device=DEV)(x).equal(net(x))


# ---- logits, predictions -------------------------------------------------------------------------------------------------------------------
def test_logits_against_float64(run, ref):
    l64 = ref["logits64"]
    _tol(run["logits"].numpy(), l64, ref["logits32"], float(np.abs(l64).max()))


def test_predictions_where_the_reference_decides(run, ref):
    und = ref["undecided"]
    assert und.sum() <= 1
    got = run["logits"].argmax(1).numpy()
    np.testing.assert_array_equal(got[~und], ref["pred"][~und])


# ---- routing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", [1, 2])
def test_routing_is_the_float64_runs_where_it_decides(run, ref, layer):
    live, near = ref[f"live{layer}"], ref[f"near{layer}"]
    frac = near.sum() / live.sum()
    print(f"pool {layer}: {int(near.sum())} of {int(live.sum())} live windows under the bound {float(ref[f'bound{layer}']):.1e}")
    assert frac <= NEAR_CAP, f"pool {layer}: {frac:.2%} of the live windows are undecided"
    pinned = live & ~near
    got, want = run[f"idx{layer}"].numpy(), ref[f"idx{layer}"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    np.testing.assert_array_equal(got[pinned], want[pinned])
    # and the masks agree there: a pinned live window is live on the GPU
    assert (run[f"p{layer}"].numpy()[pinned] > 0).all()


def test_saved_holds_pooled_tensors_only(run):
    saved = run["saved"]
    assert tuple(saved["p1"].shape) == (16, 14, 14, 32) and tuple(saved["p2"].shape) == (16, 7, 7, 64)
    assert saved["idx1"].dtype == torch.uint8 and saved["idx2"].dtype == torch.uint8
    biggest = max(v.numel() for v in saved.values() if torch.is_tensor(v))
    assert biggest == 16 * 14 * 14 * 32                                         # no un-pooled conv output (16 * 28 * 28 * 32) is kept


# ---- input gradient --------------------------------------------------------------------------------------------------------------------------
def test_input_gradient_against_the_routing_pinned_float64_backward(run, ref, sd):
    x = torch.from_numpy(ref["x"]).double().requires_grad_(True)
    _, logits = _pinned(sd, run, x)
    np.testing.assert_allclose(logits.detach().numpy(), run["logits"].double().numpy(), rtol=1e-4, atol=2e-5 * float(np.abs(ref["logits64"]).max()))
    logits.backward(run["dlogits"].double())                                    # the cotangent the GPU backward was given
    want = x.grad.numpy()
    np.testing.assert_allclose(run["dx"].double().numpy(), want, rtol=1e-4, atol=2e-5 * float(np.abs(want).max()))
    assert np.abs(want).max() > 0


def test_autograd_wiring(net, run, ref):
    x = torch.from_numpy(ref["x"]).to(DEV).requires_grad_(True)
    logits = net(x)
    assert logits.requires_grad and torch.equal(logits.detach().cpu(), run["logits"])
    logits.backward(run["dlogits"].to(DEV))
    assert torch.equal(x.grad.cpu(), run["dx"])
    with torch.no_grad():
        assert net._run_forward(x.detach(), keep=False)[1] is None
        y = net(x.detach())
    assert not y.requires_grad and y.grad_fn is None and torch.equal(y.cpu(), run["logits"])


def test_bf16_conv_precision_is_honoured(K, sd, run, ref):
    """conv_precision = "bf16" through the existing decorator: the project's bf16 rule (tests/test_hip_step_bf16.py) -- within relative
    L2 5e-2 of float64, and FURTHER from float64 than the fp32 run: the implicit-GEMM layers really ran on bf16 operands."""
    C = K.Classifier()
    C.load_state_dict(sd, strict=True)
    C = C.to(DEV).eval()
    C.conv_precision = "bf16"
    with torch.no_grad():
        got = C(torch.from_numpy(ref["x"]).to(DEV)).cpu().double().numpy()
    l64 = ref["logits64"]
    e16 = np.linalg.norm(got - l64) / np.linalg.norm(l64)
    e32 = np.linalg.norm(run["logits"].double().numpy() - l64) / np.linalg.norm(l64)
    print(f"logits rel-L2 from float64: bf16 {e16:.2e}, fp32 {e32:.2e}")
    assert e32 < e16 <= 5e-2


# ---- training mode -------------------------------------------------------------------------------------------------------------------------
def _fresh(K, sd):
    C = K.Classifier()
    C.load_state_dict(sd, strict=True)
    return C.to(DEV).train()


def test_three_adam_steps_against_float64(K, sd, ref):
    from pcgan_amd.optim import Adam
    x, y = torch.from_numpy(ref["x"][:8]), torch.from_numpy(ref["target"][:8])
    batches = [(x, y)] * 3
    l64, s64 = R.adam_steps(R.cast(sd, torch.float64), [(a.double(), b) for a, b in batches])
    l32, s32 = R.adam_steps(sd, batches)
    C = _fresh(K, sd)
    opt = Adam(C.parameters(), lr=1e-3)
    ones = torch.ones(10, device=DEV)
    tally = torch.zeros(3, dtype=torch.float64, device=DEV)
    step_loss = torch.zeros(3, device=DEV)
    for i in range(3):
        K.pool_fit_step(C, opt, x.to(DEV), y.to(DEV), ones, tally, loss_out=step_loss[i:i + 1])
    torch.cuda.synchronize()
    got = step_loss.cpu().double().numpy()
    print("losses", got, l64, "fp32 cpu", l32)
    np.testing.assert_allclose(got, l64, rtol=1e-4)
    t = tally.cpu().numpy()
    np.testing.assert_allclose(t[0], 8.0 * l64.sum(), rtol=1e-4)
    assert t[2] == 24.0
    for k, v in C.state_dict().items():
        w64 = s64[k].numpy()
        _tol(v.detach().cpu().double().numpy(), w64, s32[k].numpy(), float(np.abs(w64).max()))


def test_weight_gradients_against_the_routing_pinned_float64_backward(K, sd, ref):
    x, y = torch.from_numpy(ref["x"][:8]), torch.from_numpy(ref["target"][:8])
    C = _fresh(K, sd)
    C.zero_grad()
    C._ensure_flat()
    xd = x.to(DEV)
    logits, saved = C._train_forward(xd, [])
    a0, g1, p1, idx1, g2, p2, idx2, flat, h = saved
    dl = (torch.softmax(logits.double(), 1) - F.one_hot(y, 10).to(DEV)).div(8.0).float().contiguous()      # mean cross-entropy
    for p in C.parameters():
        p.grad = None
    C._train_backward(saved, dl)
    torch.cuda.synchronize()
    gpu = dict(idx1=R.nchw(idx1.cpu()), p1=R.nchw(p1.cpu()), idx2=R.nchw(idx2.cpu()), p2=R.nchw(p2.cpu()), h=h.cpu())
    sd64, pinned = _pinned(sd, gpu, x.double())
    np.testing.assert_allclose(pinned.detach().numpy(), logits.cpu().double().numpy(), rtol=1e-4, atol=2e-5 * float(pinned.detach().abs().max()))
    pinned.backward(dl.cpu().double())
    for k, p in C.named_parameters():
        want = sd64[k].grad.numpy()
        np.testing.assert_allclose(p.grad.detach().cpu().double().numpy(), want, rtol=1e-4, atol=2e-5 * float(np.abs(want).max()), err_msg=k)


def test_fit_returns_epoch_losses_with_one_read_per_epoch(K, sd, ref, capsys):
    x, y = torch.from_numpy(ref["x"]), torch.from_numpy(ref["target"])
    train = [(x[:8], y[:8]), (x[8:14], y[8:14])]
    valid = [(x[14:], y[14:])]
    C = _fresh(K, sd)
    tr, va = K.fit_pool_classifier(C, train, valid, epochs=2, lr=1e-3, device=DEV)
    assert len(tr) == len(va) == 2 and np.isfinite(tr + va).all() and tr[1] < tr[0]
    # against the float64 steps on the same batches: sum of loss * rows / rows per epoch (countergan2.py:136-137), the validation loss of
    # the state each epoch ends with
    b64 = [(a.double(), b) for a, b in train]
    l64, s4 = R.adam_steps(R.cast(sd, torch.float64), b64 * 2)
    _, s2 = R.adam_steps(R.cast(sd, torch.float64), b64)
    np.testing.assert_allclose(tr, [(8 * l64[0] + 6 * l64[1]) / 14, (8 * l64[2] + 6 * l64[3]) / 14], rtol=1e-4)
    v64 = [float(F.cross_entropy(R.forward(s, x[14:].double())["logits"], y[14:])) for s in (s2, s4)]
    np.testing.assert_allclose(va, v64, rtol=1e-4)
    assert "Epoch 2 - Train loss" in capsys.readouterr().out


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator(K, golden_dir):
    G = K.ResidualGenerator()
    G.load_state_dict(torch.load(os.path.join(golden_dir, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    return G.to(DEV).eval()


class _Cfg:
    device, num_classes = DEV, 10

    def __init__(self, save_dir):
        self.save_dir = str(save_dir)


def test_padded_logits_are_the_forward_bit_for_bit(K, net, ref):
    x = torch.from_numpy(ref["x"]).to(DEV)
    with torch.no_grad():
        want = net(x)
        rows = x.view(16, 784)
        got = net.padded_logits(rows)
        dst = torch.full((16, 12), 7.0, device=DEV)
        K._padded_logits(net, rows, out=dst)
    assert tuple(got.shape) == (16, 12) and torch.equal(got[:, :10], want) and torch.equal(dst, got)
    assert (got[:, 10:] == 0).all()


def test_counterfactual_front_ends_accept_the_net(K, generator, net, ref, tmp_path):
    x, y = torch.from_numpy(ref["x"][:6]).to(DEV), torch.from_numpy(ref["target"][:6]).to(DEV)
    with torch.no_grad():
        for t in range(10):
            out = K.counterfactuals(generator, net, x, t, y_true=y)
            probs = torch.softmax(net(out["x_cf"]).double(), 1).cpu().numpy()
            np.testing.assert_array_equal(out["pred"].cpu().numpy(), probs.argmax(1))
            np.testing.assert_allclose(out["p_target"].cpu().numpy(), probs[:, t], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(out["conf"].cpu().numpy(), probs.max(1), rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(out["p_true"].cpu().numpy(), probs[np.arange(6), y.cpu().numpy()], rtol=1e-5, atol=1e-7)
        sweep = K.counterfactual_sweep(generator, net, x, y_true=y)
        probs = torch.softmax(net(sweep["x_cf"].reshape(60, 1, 28, 28)).double(), 1).cpu().numpy().reshape(10, 6, 10)
        np.testing.assert_allclose(sweep["p_target"].cpu().numpy(), probs[np.arange(10)[:, None], np.arange(6)[None, :], np.arange(10)[:, None]],
                                   rtol=1e-5, atol=1e-7)
        loader = [(x[:4].cpu(), y[:4].cpu()), (x[4:].cpu(), y[4:].cpu())]
        one = K.evaluate_generator_per_target(generator, net, loader, _Cfg(tmp_path / "one"), one_pass=True, verbose=False)
        loop = K.evaluate_generator_per_target(generator, net, loader, _Cfg(tmp_path / "loop"), one_pass=False, verbose=False)
    # the table's flip rate from the sweep's own flips: per batch means, averaged over the batches
    flip = sweep["flip"].cpu().double().numpy()
    for t in range(10):
        flips = np.mean([flip[t, :4].mean(), flip[t, 4:].mean()])
        np.testing.assert_allclose(one[t]["class_flip_rate"], flips, rtol=1e-6, atol=1e-7)
        for k in K.PER_CLASS_FIELDS:
            np.testing.assert_allclose(one[t][k], loop[t][k], rtol=2e-4, atol=2e-6, err_msg=f"{k} target {t}")


def test_evaluate_classifier_and_masked_metrics_accept_the_net(K, generator, net, run, ref):
    x, y = torch.from_numpy(ref["x"]), torch.from_numpy(ref["target"])
    acc, cm = K.evaluate_classifier(net, [(x[:9], y[:9]), (x[9:], y[9:])], DEV, verbose=False)
    pred = run["logits"].argmax(1).numpy()
    want = np.zeros((10, 10), np.int64)
    np.add.at(want, (y.numpy(), pred), 1)
    np.testing.assert_array_equal(cm, want)
    assert acc == float((pred == y.numpy()).mean())
    xs, ys, t = x[:6].to(DEV), y[:6].to(DEV), torch.full((6,), 3, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        out = K.counterfactuals(generator, net, xs, t, patches=[1, 5, 10, 12, 13, 14], y_true=ys)
        met = K.compute_masked_metrics(out["raw_residual"], out["masked_residual"], xs, out["x_cf"], out["mask"], net, ys, t)
        p_cf = torch.softmax(net(out["x_cf"]).double(), 1).cpu().numpy()
        p_or = torch.softmax(net(xs).double(), 1).cpu().numpy()
    assert tuple(met) == K.MASKED_METRIC_KEYS
    np.testing.assert_allclose(met["Class_flip_rate_mean"], float((p_cf.argmax(1) == 3).mean()), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(met["Prediction_gain"], float((p_cf[:, 3] - p_or[np.arange(6), ys.cpu().numpy()]).mean()), rtol=1e-4, atol=1e-6)


def test_train_step_takes_the_net_as_guidance(K, net, sd):
    from oracle import countergan_ref as CR
    torch.manual_seed(0)
    G, D = K.ResidualGenerator().to(DEV), K.Discriminator().to(DEV)
    x, y, t, m = (a.to(DEV) for a in CR.synthetic_batch(4, seed=2))
    opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
    out = K.train_step(G, D, net, opt_g, opt_d, bce, ce, x, y, t, m)
    torch.cuda.synchronize()
    assert np.isfinite(out["g_cls"].item()) and out["g_cls"].item() > 0
    for n, p in G.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert any(float(p.grad.abs().max()) > 0 for p in G.parameters())
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    assert all(p.grad is None for p in net.parameters())
    # the classifier term of the step is the cross-entropy of the net's own logits on the step's counterfactuals
    with torch.no_grad():
        want = F.cross_entropy(net(out["x_cf"].detach()).double(), t).item()
    np.testing.assert_allclose(out["g_cls"].item(), want, rtol=1e-5)
