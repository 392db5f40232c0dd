"""GPU: the moons CounteRGAN's classifier fit in one launch (csrc/moons_clf.hip through pcgan_amd.moons_countergan.ClassifierFit /
fit_classifier) against the float64 restatement (tests/moons_clf_restate.py, pinned to the reference's recorded run
by tests/test_moons_clf_fit_host.py) and against that recording (tests/golden/moons_clf_ref.npz).

Tolerances are the project's (tests/test_hip_moons_cf.py): scalars rtol 1e-5, atol 1e-7; parameters and moments rtol 1e-4,
atol 1e-6 + 1e-5 max|ref|.  Weights after 1000 steps are never compared: rounding alone separates the trajectories by then
(dist1000 of the fixture, 3e-2); the long run is held to conditions every arithmetic variant of the reference's run met."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moons_clf_restate as RS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 512                                    # rows per chunk of the kernel (csrc/moons_clf.hip: CH)


@pytest.fixture(scope="module")
def M():
    import pcgan_amd
    from pcgan_amd import moons_countergan
    pcgan_amd.load()
    return moons_countergan


@pytest.fixture(scope="module")
def gold():
    g, data = RS.fixture()
    g["X"], g["y"], g["X_test"], g["y_test"] = (data[f"data.{k}"] for k in ("X_train", "y_train", "X_test", "y_test"))
    return g


# ---- rig: the fused side with loadable state -------------------------------------------------------------------------------------
class Rig:
    def __init__(self, M, params, X, y, moments=None, lr=RS.LR):
        self.M = M
        self.clf = M.NNClassifier(2)
        self.clf.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in params.items()})
        self.clf.to(DEV)
        self.fit = M.ClassifierFit(self.clf, X, y, lr=lr)
        self.off = dict(zip(RS.KEYS, M._offsets(self.clf, list(RS.KEYS))))
        if moments is not None:
            m, v, t = moments
            for k in RS.KEYS:
                n = int(np.prod(RS.SHAPES[k]))
                self.fit.seg["exp_avg"][self.off[k]:self.off[k] + n] = torch.from_numpy(np.asarray(m[k], np.float32).ravel().copy()).to(DEV)
                self.fit.seg["exp_avg_sq"][self.off[k]:self.off[k] + n] = torch.from_numpy(np.asarray(v[k], np.float32).ravel().copy()).to(DEV)
            self.fit.seg["step"].fill_(t)

    def params(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.clf.state_dict().items()}

    def _flat(self, name):
        t = self.fit.seg[name].cpu().numpy()
        return {k: t[self.off[k]:self.off[k] + int(np.prod(RS.SHAPES[k]))].reshape(RS.SHAPES[k]).copy() for k in RS.KEYS}

    def moments(self):
        return self._flat("exp_avg"), self._flat("exp_avg_sq"), int(self.fit.seg["step"].item())

    def raw(self):
        """Everything a launch writes, as bytes-comparable arrays."""
        return [self.clf.flat_params.detach().cpu().numpy().copy(), self.fit.seg["exp_avg"].cpu().numpy().copy(),
                self.fit.seg["exp_avg_sq"].cpu().numpy().copy(), self.fit.seg["step"].cpu().numpy().copy()]


def close_scalar(a, b, what, rtol=1e-5, atol=1e-7):
    print(f"{what}: {np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))):.3e} (max |.|, ref scale {np.max(np.abs(b)):.3e})")
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def close_state(got, ref, what, floor=0.0, keep=None):
    """Parameters or moments {key: array} at the project's state tolerance (atol at least `floor`); keep: {key: bool mask}."""
    worst = 0.0
    for k in RS.KEYS:
        rtol, atol = RS.state_tol(ref[k])
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if keep is not None:
            a, b = a[keep[k]], b[keep[k]]
        worst = max(worst, float(np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=rtol, atol=max(atol, floor), err_msg=f"{what} {k}")
    print(f"{what}: max |fused - float64| = {worst:.3e}")
    return worst


def both(M, params, X, y, moments=None, lr=RS.LR):
    return Rig(M, params, X, y, moments, lr), RS.Fit(params, np.asarray(X, np.float32), y, moments=moments, lr=lr)


def compare_after(rig, ref, what, keep=None):
    close_state(rig.params(), ref.params(), what + " parameters", keep=keep)
    gm, gv, gt = rig.moments()
    rm, rv, rt = ref.moments()
    close_state(gm, rm, what + " exp_avg")
    close_state(gv, rv, what + " exp_avg_sq")
    assert gt == rt, (what, gt, rt)


# ---- 1. teacher-forced single steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 10, 100])
def test_single_step_from_the_recorded_state(M, gold, k):
    """Both sides start from the reference's recorded fp32 state before step k (moments and counter included) and take one step."""
    params, moments = RS.gold_state(gold, k - 1), RS.gold_moments(gold, k - 1)
    rig, ref = both(M, params, gold["X"], gold["y"], moments)
    loss = rig.fit.run(1).cpu().numpy()
    ref_loss = ref.step()
    close_scalar(loss, [ref_loss], f"step {k} loss")
    close_scalar(loss, gold["losses"][k - 1:k], f"step {k} loss against the recording")
    keep = None
    if k == 1:
        # a fresh Adam moves an element by lr * sign(g) whatever |g|: where the float64 gradient is below 1e-6 of its tensor's
        # largest, fp32 rounding decides the sign.  Such elements are left out; at most 1 % of a tensor may be.  (An exact 0 — a
        # hidden unit that is dead on every row — is no such element: it moves nothing on either side, and stays in.)
        grads = ref.grads()
        keep = {key: (np.abs(g) >= 1e-6 * np.abs(g).max()) | (g == 0) for key, g in grads.items()}
        for key, m in keep.items():
            print(f"step 1 {key}: {int((~m).sum())} of {m.size} elements left out")
            assert (~m).sum() <= 0.01 * m.size, key
    compare_after(rig, ref, f"step {k}", keep)
    assert rig.moments()[2] == k


# ---- 2. free run -----------------------------------------------------------------------------------------------------------------
def test_free_run_of_100_steps_in_one_launch(M, gold):
    rig = Rig(M, RS.gold_state(gold, 0), gold["X"], gold["y"])
    losses = rig.fit.run(100).cpu().numpy()
    close_scalar(losses, gold["losses64"][:100], "100 losses against float64", rtol=1e-4, atol=0.0)
    d100 = float(gold["dist100"])
    worst = close_state(rig.params(), RS.gold_state(gold, 100, "C64"), "free run, step 100", floor=3 * d100)
    print(f"the reference's own fp32 run lies {d100:.3e} from float64 at step 100; the kernel {worst:.3e}")
    assert rig.moments()[2] == 100


# ---- 3. one launch equals many -----------------------------------------------------------------------------------------------------
def _split_run(M, gold, split):
    rig = Rig(M, RS.gold_state(gold, 0), gold["X"], gold["y"])
    losses = torch.cat([rig.fit.run(n) for n in split]).cpu().numpy()
    return [losses] + rig.raw()


def test_one_launch_equals_many_bit_for_bit(M, gold):
    runs = {split: _split_run(M, gold, split) for split in ((30,), (1,) * 30, (7, 23))}
    again = _split_run(M, gold, (30,))
    base = runs[(30,)]
    assert int(base[4][0]) == 30 and np.isfinite(base[0]).all()
    for split, r in list(runs.items()) + [("again", again)]:
        for a, b, what in zip(base, r, ("losses", "parameters", "exp_avg", "exp_avg_sq", "step")):
            assert a.tobytes() == b.tobytes(), (split, what)


# ---- 4. the reference-sized fit ----------------------------------------------------------------------------------------------------
def _fresh(M, gold):
    clf = M.NNClassifier(2)
    clf.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in RS.gold_state(gold, 0).items()})
    return clf.to(DEV)


def _accuracy(clf, X, y):
    with torch.no_grad():
        pred = clf(torch.from_numpy(np.asarray(X, np.float32)).to(DEV)).argmax(1).cpu().numpy()
    return int((pred == np.asarray(y)).sum()), len(y)


def test_reference_sized_fit(M, gold):
    clf = _fresh(M, gold)
    out = M.fit_classifier(clf, gold["X"], gold["y"], steps=1000)
    losses = out["losses"].cpu().numpy()
    seg = out["optimizer"].flat_segment(clf)
    assert int(seg["step"].item()) == 1000 and losses.shape == (1000,)
    assert np.isfinite(losses).all() and all(torch.isfinite(t).all() for t in (clf.flat_params, seg["exp_avg"], seg["exp_avg_sq"]))
    n_ok, n = _accuracy(clf, gold["X"], gold["y"])
    n_test, nt = _accuracy(clf, gold["X_test"], gold["y_test"])
    print(f"train {n_ok}/{n}, test {n_test}/{nt}, losses[-1] {losses[-1]:.3e}, max(losses[900:]) {losses[900:].max():.3e}")
    assert out["train_correct"] == n_ok
    assert n_ok / n >= 0.99 and n_test / nt >= 0.98
    assert losses[-1] < 5e-3 and losses[900:].max() < 5e-3
    clf10 = _fresh(M, gold)
    out10 = M.fit_classifier(clf10, gold["X"], gold["y"], steps=1000, steps_per_launch=100)
    assert out10["losses"].cpu().numpy().tobytes() == losses.tobytes() and out10["train_correct"] == out["train_correct"]
    assert clf10.flat_params.cpu().numpy().tobytes() == clf.flat_params.cpu().numpy().tobytes()
    seg10 = out10["optimizer"].flat_segment(clf10)
    for k in ("exp_avg", "exp_avg_sq", "step"):
        assert seg10[k].cpu().numpy().tobytes() == seg[k].cpu().numpy().tobytes(), k


# ---- 5. row counts where the row mapping can go wrong ------------------------------------------------------------------------------
def _warm(m=0.0, v=1e-4, t=10):
    return ({k: np.full(RS.SHAPES[k], m, np.float32) for k in RS.KEYS}, {k: np.full(RS.SHAPES[k], v, np.float32) for k in RS.KEYS}, t)


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 960, 4096])
def test_row_counts(M, gold, N):
    idx = np.random.RandomState(100 + N).randint(0, 960, N)
    X, y = gold["X"][idx], gold["y"][idx]
    rig, ref = both(M, RS.gold_state(gold, 10), X, y, _warm())
    losses, correct = rig.fit.run(2, count_correct=True)
    close_scalar(losses.cpu().numpy(), ref.run(2), f"N = {N} losses")
    compare_after(rig, ref, f"N = {N}")
    assert all(np.isfinite(v).all() for v in rig.params().values())
    with torch.no_grad():                      # (the eval kernel: NNClassifier.forward takes no batch of one row)
        pred = M._classify(rig.clf, X.astype(np.float32)).cpu().numpy()
    assert int(correct.item()) == int((pred == y).sum())
    assert rig.moments()[2] == 12


# ---- 6. corners ----------------------------------------------------------------------------------------------------------------------
DEAD = 5


def _dead_unit(gold):
    p = {k: v.copy() for k, v in RS.gold_state(gold, 0).items()}
    p["net.0.bias"][DEAD] = -10.0                 # x lies in [0, 1]^2 and |W1| < 0.71: the pre-activation stays below -8
    return p


def test_dead_hidden_unit_fresh_optimizer_never_moves(M, gold):
    p = _dead_unit(gold)
    rig = Rig(M, p, gold["X"], gold["y"])
    assert np.isfinite(rig.fit.run(5).cpu().numpy()).all()
    q = rig.params()
    assert q["net.0.weight"][DEAD].tobytes() == p["net.0.weight"][DEAD].tobytes() and q["net.0.bias"][DEAD] == p["net.0.bias"][DEAD]
    assert q["net.2.weight"][:, DEAD].tobytes() == p["net.2.weight"][:, DEAD].tobytes()
    m, v, _ = rig.moments()
    assert not m["net.0.weight"][DEAD].any() and not v["net.2.weight"][:, DEAD].any()
    assert (q["net.2.weight"][:, DEAD - 1] != p["net.2.weight"][:, DEAD - 1]).any(), "its neighbours do move"


def test_dead_hidden_unit_warm_moments_follow_float64(M, gold):
    rig, ref = both(M, _dead_unit(gold), gold["X"], gold["y"], _warm(m=0.01))
    close_scalar(rig.fit.run(2).cpu().numpy(), ref.run(2), "dead unit, warm: losses")
    compare_after(rig, ref, "dead unit, warm")


def test_saturated_softmax(M, gold):
    p = {k: v * np.float32(1e3) for k, v in RS.gold_state(gold, 0).items()}
    rig, ref = both(M, p, gold["X"], gold["y"])
    loss = rig.fit.run(1).cpu().numpy()
    assert np.isfinite(loss).all() and loss[0] > 1e3
    close_scalar(loss, [ref.step()], "saturated softmax: loss")
    assert all(np.isfinite(v).all() for v in rig.params().values())
    assert np.isfinite(rig.fit.run(3).cpu().numpy()).all() and all(np.isfinite(v).all() for v in rig.params().values())


def test_all_rows_of_one_class(M, gold):
    y = np.zeros_like(gold["y"])
    rig, ref = both(M, RS.gold_state(gold, 10), gold["X"], y, _warm())
    close_scalar(rig.fit.run(2).cpu().numpy(), ref.run(2), "one class: losses")
    compare_after(rig, ref, "one class")


def test_correct_count_with_two_tied_logits(M, gold):
    """Classes 0 and 1 get bit-identical logits on every row, class 2 a lower one: argmax is 0, the lower index, as torch.argmax.
    lr = 0 keeps the weights (p - 0 * m / denom = p), so the count is of exactly these weights."""
    p = {k: v.copy() for k, v in RS.gold_state(gold, 0).items()}
    p["net.4.weight"][1] = p["net.4.weight"][0]
    p["net.4.bias"][1] = p["net.4.bias"][0]
    p["net.4.bias"][2] = -100.0
    X = gold["X"][:700].astype(np.float32)
    for label, want in ((0, 700), (1, 0), (2, 0)):
        rig = Rig(M, p, X, np.full(700, label), lr=0.0)
        _, correct = rig.fit.run(1, count_correct=True)
        assert rig.params()["net.4.weight"].tobytes() == p["net.4.weight"].tobytes()
        with torch.no_grad():
            logits = rig.clf(torch.from_numpy(X).to(DEV))
        assert torch.equal(logits[:, 0], logits[:, 1]) and int((logits.argmax(1) == label).sum()) == want
        assert int(correct.item()) == want, (label, int(correct.item()))


# ---- 7. interop ----------------------------------------------------------------------------------------------------------------------
def test_eager_adam_step_continues_after_fused_launch(M, gold):
    rig, ref = both(M, RS.gold_state(gold, 0), gold["X"], gold["y"])
    rig.fit.run(3)
    ref.run(3)
    g = torch.Generator().manual_seed(3)
    grads = {k: (torch.randn(RS.SHAPES[k], generator=g, dtype=torch.float64) * 1e-2).numpy() for k in RS.KEYS}
    for name, p in rig.clf.named_parameters():
        p.grad.copy_(torch.from_numpy(grads[name]).float().to(DEV))
    rig.fit.opt.step()
    ref.eager_step(grads)
    compare_after(rig, ref, "eager step after 3 fused ones")
    assert rig.moments()[2] == 4


class RefShaped(nn.Module):
    """The reference's NNClassifier (models/nn_classifier.py) by shape: state_dict keys net.{0,2,4}.{weight,bias}."""

    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3))

    def forward(self, x):
        return self.net(x)


def _cfg(M, tmp_path, **kw):
    return dict(M.config, cuda=DEV, out_dir=str(tmp_path), clf_model_path=str(tmp_path / "clf" / "classifier.pt"),
                generator_path=str(tmp_path / "generator.pt"), **kw)


def test_checkpoints_and_downstream_users(M, gold, tmp_path):
    cfg = _cfg(M, tmp_path, epochs=1)
    os.makedirs(tmp_path / "clf")
    with contextlib.redirect_stdout(io.StringIO()):
        clf = M.train_classifier(gold["X"], gold["y"], cfg, one_launch=True)
    saved = torch.load(cfg["clf_model_path"], map_location="cpu")
    assert list(saved) == ["model_state_dict"] and list(saved["model_state_dict"]) == list(RS.KEYS)
    ref = RefShaped()
    ref.load_state_dict(saved["model_state_dict"])
    with torch.no_grad():
        pred = ref(torch.from_numpy(gold["X_test"].astype(np.float32))).argmax(1).numpy()
    assert (pred == gold["y_test"]).mean() >= 0.98
    again = M.NNClassifier(2)
    again.load_state_dict(saved["model_state_dict"])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(again.state_dict().values(), clf.state_dict().values()))
    os.remove(cfg["clf_model_path"])
    with contextlib.redirect_stdout(io.StringIO()):
        clf2 = M.get_classifier(gold["X"], gold["y"], cfg, one_launch=True)
        bare = torch.load(cfg["clf_model_path"], map_location="cpu")
        assert list(bare) == list(RS.KEYS), "main.py:38 saves the bare state_dict"
        clf3 = M.get_classifier(gold["X"], gold["y"], cfg, one_launch=True)          # now it loads what it saved
        assert all(torch.equal(a, b) for a, b in zip(clf2.state_dict().values(), clf3.state_dict().values()))
        acc, cm = M.evaluate_classifier(clf2, gold["X_test"], gold["y_test"], cfg)
        assert acc >= 0.98 and cm.shape == (3, 3)
        torch.manual_seed(0)
        G = M.ResidualGenerator(2, 32, 3)
        res = M.train_countergan(G, cfg, gold["X"], gold["y"], clf2, verbose=False, save=False)
    assert np.isfinite(res["d_losses"]).all() and np.isfinite(res["g_losses"]).all()


# ---- 8. launch count -------------------------------------------------------------------------------------------------------------------
def test_launch_count(M, gold, tmp_path, monkeypatch):
    calls = []
    real_check = M.ops.check
    monkeypatch.setattr(M.ops, "check", lambda rc, what="": (calls.append(what), real_check(rc, what))[1])
    seen = {}
    for one_launch in (True, False):
        cfg = _cfg(M, tmp_path / str(one_launch))
        del calls[:]
        with contextlib.redirect_stdout(io.StringIO()):
            M.get_classifier(gold["X"], gold["y"], cfg, one_launch=one_launch)
        seen[one_launch] = list(calls)
    # what every step of the op chain launches; pcg_fill (zero_grad there) also zeroes the fresh Adam moments of either path
    chain_ops = {w for w in set(seen[False]) if seen[False].count(w) >= 1000} - {"pcg_fill"}
    print(f"one launch: {seen[True]}; op chain: {len(seen[False])} calls, per step {sorted(chain_ops)}")
    assert seen[True].count("pcg_moons_clf_fit") == 1 and set(seen[True]) <= {"pcg_moons_clf_fit", "pcg_fill"} and not chain_ops & set(seen[True])
    assert "pcg_moons_clf_fit" not in seen[False] and len(chain_ops) >= 3
