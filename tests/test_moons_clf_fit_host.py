"""Host-side checks (no GPU) of the one-launch classifier fit of the moons CounteRGAN (csrc/moons_clf.hip): the ABI
additions, the entry point's refusals, the Python refusals (before any launch), and the restatement (tests/moons_clf_restate.py)
pinned to the reference's recorded run (tests/golden/moons_clf_ref.npz)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moons_clf_restate as RS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pcg_moons_clf_fit_scratch_bytes", "pcg_moons_clf_fit")
NEW_STRUCTS = {"pcg_moons_clf_fit_desc": "MoonsClfFitDesc", "pcg_moons_clf_fit_args": "MoonsClfFitArgs"}
OFFSETS = (0, 64, 96, 1120, 1152, 1248)       # the six tensors in FlatModule's flat buffer (each padded to 4 floats): 1252 floats
FAKE = 0x10000                                # a non-null, 16-byte aligned address: every call below is refused before it is used


def _header():
    with open(os.path.join(ROOT, "include", "pcgan_hip.h")) as f:
        return f.read()


def test_new_symbols_declared_and_exported():
    from pcgan_amd import _lib
    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name + "(" in header, f"{name} is not declared in include/pcgan_hip.h"
    assert "trainer.py:13-29" in header and "main.py:14-40" in header
    assert _lib.load().pcg_abi_version() == 7, "the additions are additive"


def _header_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(",")]
        for d in [first.split()[-1]] + rest:
            fields.append(re.sub(r"\[.*\]", "", d.lstrip("*")))
    return fields


def test_ctypes_structs_match_the_header():
    from pcgan_amd import _lib
    header, lib = _header(), _lib.load()
    for name, cls in NEW_STRUCTS.items():
        S = getattr(_lib, cls)
        assert _lib.STRUCTS[name] is S
        assert lib.pcg_abi_struct_bytes(name.encode()) == ctypes.sizeof(S), name
        assert [f for f, _ in S._fields_] == _header_fields(header, name), name
    assert ctypes.sizeof(_lib.MoonsClfFitDesc) == 4 * 4 + 6 * 4 + 4 * 8
    assert ctypes.sizeof(_lib.MoonsClfFitArgs) == 10 * 8


def _valid(**kw):
    from pcgan_amd import _lib
    d, a = _lib.MoonsClfFitDesc(), _lib.MoonsClfFitArgs()
    d.hidden, d.N, d.nC, d.nC_adam = 32, 960, 1252, 1252
    d.c_off[:] = OFFSETS
    d.lr, d.beta1, d.beta2, d.adam_eps = 1e-2, 0.9, 0.999, 1e-8
    for f in ("X", "Y", "c_flat", "exp_avg", "exp_avg_sq", "step", "losses"):
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k.startswith("c_off"):
            d.c_off[int(k[5:])] = v
        elif hasattr(d, k):
            setattr(d, k, v)
        else:
            setattr(a, k, v)
    return d, a


REFUSED = [(dict(hidden=64), "hidden"), (dict(hidden=0), "hidden"), (dict(N=0), "N "), (dict(N=4097), "N "), (dict(N=-5), "N "),
           (dict(nC=0), "nC"), (dict(nC=1 << 20), "nC"), (dict(nC=1200), "c_off"),
           (dict(c_off0=-4), "c_off[0]"), (dict(c_off1=60), "c_off[1]"), (dict(c_off2=98), "c_off[2]"), (dict(c_off3=1100), "c_off[3]"),
           (dict(c_off4=1300), "c_off[4]"), (dict(c_off5=1250), "c_off[5]"), (dict(c_off5=1 << 30), "c_off[5]"),
           (dict(nC_adam=1253), "nC_adam"), (dict(nC_adam=-1), "nC_adam"),
           (dict(X=None), "X"), (dict(Y=None), "Y"), (dict(c_flat=None), "c_flat"), (dict(exp_avg=None), "exp_avg"),
           (dict(exp_avg_sq=None), "exp_avg_sq"), (dict(step=None), "step"), (dict(losses=None), "losses"), (dict(X=FAKE + 4), "X"),
           (dict(scratch=FAKE + 8, scratch_bytes=64), "scratch"), (dict(scratch=None, scratch_bytes=64), "scratch")]


@pytest.mark.parametrize("kw, field", REFUSED, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in REFUSED])
def test_entry_refuses_before_any_gpu_call(kw, field):
    """Each invalid descriptor or argument: a status other than PCG_OK and the field's name in pcg_last_error().  The pointers are
    never dereferenced (they are fake): a refusal that came after a GPU call would crash here, not fail."""
    from pcgan_amd import _lib
    lib = _lib.load()
    d, a = _valid(**kw)
    rc = lib.pcg_moons_clf_fit(ctypes.byref(d), ctypes.byref(a), 1, None)
    assert rc != _lib.PCG_OK and field in lib.pcg_last_error().decode(), (kw, rc, lib.pcg_last_error())


def test_entry_refuses_null_structs_and_step_counts():
    from pcgan_amd import _lib
    lib = _lib.load()
    d, a = _valid()
    assert lib.pcg_moons_clf_fit(None, ctypes.byref(a), 1, None) != _lib.PCG_OK and b"desc" in lib.pcg_last_error()
    assert lib.pcg_moons_clf_fit(ctypes.byref(d), None, 1, None) != _lib.PCG_OK and b"args" in lib.pcg_last_error()
    for n in (0, -3):
        assert lib.pcg_moons_clf_fit(ctypes.byref(d), ctypes.byref(a), n, None) != _lib.PCG_OK and b"n_steps" in lib.pcg_last_error()
    # the rows are walked in chunks that live in LDS: no global scratch at any N, so none can be too small
    for N in (1, 960, 4096):
        assert lib.pcg_moons_clf_fit_scratch_bytes(ctypes.byref(_valid(N=N)[0])) == 0


def test_python_refusals_happen_before_any_launch(monkeypatch):
    from pcgan_amd import PcgError, moons_countergan as M
    from pcgan_amd.optim import Adam
    calls = []
    monkeypatch.setattr(M.ops, "check", lambda rc, what="": calls.append(what))
    X, y = np.random.RandomState(0).rand(50, 2).astype(np.float32), np.arange(50) % 3
    clf = M.NNClassifier(2)
    cases = [(lambda: M.ClassifierFit(clf, X[:0], y[:0]), "rows"),
             (lambda: M.ClassifierFit(clf, np.zeros((4097, 2), np.float32), np.zeros(4097, np.int64)), "rows"),
             (lambda: M.ClassifierFit(clf, np.zeros((50, 3), np.float32), y), r"\[N\]\[2\]"),
             (lambda: M.ClassifierFit(clf, X.ravel(), y), r"\[N\]\[2\]"),
             (lambda: M.ClassifierFit(clf, X, y[:49]), r"\[N\]\[2\]"),
             (lambda: M.ClassifierFit(clf, X, y + 1), "labels"),
             (lambda: M.ClassifierFit(clf, X, y - 1), "labels"),
             (lambda: M.ClassifierFit(clf, X, y.astype(np.float32)), "labels"),
             (lambda: M.ClassifierFit(M.NNClassifier(2, hidden_dim=64), X, y), "hidden width 32"),
             (lambda: M.ClassifierFit(M.NNClassifier(3), X, y), "input_dim"),
             (lambda: M.ClassifierFit(clf, X, y, opt=torch.optim.Adam(clf.parameters())), "pcgan_amd.optim.Adam only"),
             (lambda: M.ClassifierFit(clf, X, y, opt=Adam(clf.parameters(), weight_decay=1e-2)), "weight decay"),
             (lambda: M.ClassifierFit(clf, X, y, opt=Adam([{"params": [clf.net[0].weight]}, {"params": [clf.net[0].bias]}])), "one parameter group"),
             (lambda: Adam(clf.parameters(), amsgrad=True), "amsgrad"),
             (lambda: M.ClassifierFit(clf, X, y), "CPU"),                                     # everything else in order: the device
             (lambda: M.fit_classifier(clf, X, y, steps=0), "steps"),
             (lambda: M.fit_classifier(clf, X, y, steps=10, steps_per_launch=0), "steps"),
             (lambda: M.fit_classifier(clf, X, y), "CPU")]
    for fn, what in cases:
        with pytest.raises(PcgError, match=what):
            fn()
    frozen = M.NNClassifier(2)
    frozen.net[2].bias.requires_grad = False
    with pytest.raises(PcgError, match="requires_grad"):
        M.ClassifierFit(frozen, X, y)
    assert calls == [], calls
    import inspect
    for fn in (M.train_classifier, M.get_classifier, M.main):
        assert inspect.signature(fn).parameters["one_launch"].default is False, "a feature changes no default"


@pytest.fixture(scope="module")
def gold():
    return RS.fixture()


def test_fixture_holds_what_the_tests_rely_on(gold):
    g, data = gold
    assert data["data.X_train"].shape == (960, 2) and set(np.unique(data["data.y_train"])) == {0, 1, 2}
    assert g["losses"].shape == (1000,) and g["losses64"].shape == (1000,) and g["losses"].dtype == np.float32
    for k in (1, 2, 3, 9, 10, 99, 100, 1000):
        for key in RS.KEYS:
            assert g[f"it{k}.C.{key}"].shape == RS.SHAPES[key] and g[f"it{k}.C64.{key}"].dtype == np.float64
            assert g[f"it{k}.opt.{key}.exp_avg"].shape == RS.SHAPES[key] and g[f"it{k}.opt.{key}.exp_avg_sq"].shape == RS.SHAPES[key]
        assert int(g[f"it{k}.opt.step"]) == k
        d = max(float(np.abs(g[f"it{k}.C.{key}"] - g[f"it{k}.C64.{key}"]).max()) for key in RS.KEYS)
        assert d == float(g[f"dist{k}"])
    assert float(g["dist100"]) < 5e-6 < 1e-2 < float(g["dist1000"]), "the trajectories agree at step 100 and have separated at 1000"
    for tag in ("", "64"):
        assert float(g[f"acc{tag}.train"]) == 1.0 and float(g[f"acc{tag}.test"]) >= 0.995 and float(g[f"final_loss{tag}"]) < 1e-3
    assert float(g["losses"][900:].max()) < 1e-3


def test_restatement_in_fp32_reproduces_the_recording(gold):
    """Pins tests/moons_clf_restate.py to the reference's own train_classifier: the same losses over the first 100 steps and the
    same weights after them."""
    g, data = gold
    fit = RS.Fit(RS.gold_state(g, 0), data["data.X_train"], data["data.y_train"], dtype=torch.float32)
    losses = fit.run(100)
    np.testing.assert_allclose(losses, g["losses"][:100], rtol=1e-5)
    for key, v in fit.params().items():
        rtol, atol = RS.state_tol(g[f"it100.C.{key}"])
        np.testing.assert_allclose(v, g[f"it100.C.{key}"], rtol=rtol, atol=atol, err_msg=key)
    m, v, t = fit.moments()
    assert t == 100
    # and in float64 it is the recorded float64 rerun
    fit = RS.Fit(RS.gold_state(g, 0), data["data.X_train"], data["data.y_train"])
    np.testing.assert_allclose(fit.run(100), g["losses64"][:100], rtol=1e-9)
    for key, v in fit.params().items():
        np.testing.assert_allclose(v, g[f"it100.C64.{key}"], rtol=1e-7, atol=1e-10, err_msg=key)
