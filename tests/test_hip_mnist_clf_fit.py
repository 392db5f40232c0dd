"""GPU: the MNIST classifier fit on fused launches around the convolutions -- pcg_drop2d_flatten_fwd / _bwd,
pcg_mnist_clf_head, pcg_mnist_clf_batch(_counter), countergan.ClassifierFit and countergan.train_classifier(fused=True).

Bounds.  The flatten entries and the batch entry are bit-exact against the launches / the host model they replace.  The head against
float64 (tests/mnist_clf_restate.py): every output within max(1e-4 x max|truth|, 3 x the distance of the same restatement run in
float32 on the CPU, 1e-8) -- the teacher-forced rule of tests/test_hip_countergan.py::test_classifier_pretraining_matches_reference,
which also supplies the pass conditions of the golden steps.  No bound looks at the HIP result.  Figures are printed before they are
asserted (pytest -s shows them)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnist_clf_restate as RS  # noqa: E402
from oracle import countergan_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77.0


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import countergan, data  # noqa: F401
    pcgan_amd.load()
    return pcgan_amd


@pytest.fixture(scope="module")
def ops(pcg):
    return pcg.ops


def _dev(t):
    return t.to(DEV).contiguous()


def _padded(shape, extra=3, dtype=torch.float32):
    """A view of `shape` at the head of a sentinel-filled buffer with `extra` more leading rows: (view, the rows behind it)."""
    buf = torch.full((shape[0] + extra,) + tuple(shape[1:]), SENT, device=DEV, dtype=dtype)
    return buf[:shape[0]], buf[shape[0]:]


def _digest(t, nsamples=64):
    a = np.asarray(t.detach().cpu().numpy(), dtype=np.float64).ravel()
    idx = np.linspace(0, a.size - 1, num=min(nsamples, a.size)).astype(np.int64)
    return np.concatenate([[a.sum(), np.abs(a).sum(), (a * a).sum()], a[idx]])


# ---- 1. Dropout2d + Flatten, forward and backward: the bits of the launch chains ---------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 128])
@pytest.mark.parametrize("shape", [(49, 128), (5, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flatten_entries_are_bit_identical_to_the_chains(ops, R, shape):
    HW, C = shape
    rs = np.random.RandomState(13 * R + HW + C)
    t = lambda a: _dev(torch.from_numpy(a.astype(np.float32)))     # noqa: E731
    a = t(rs.normal(0, 1, (R, HW, C)))
    y = t(np.maximum(rs.normal(0, 1, (R, HW, C)), 0))
    m = t(rs.random_sample((R, C)) < 0.75)
    dflat = t(rs.normal(0, 1, (R, C * HW)))
    out, tail = _padded((R, C * HW))
    ops.drop2d_flatten_fwd(a, m, 0.25, R, HW, C, out=out)
    want = ops.nhwc_to_nchw_flat(ops.dropout_apply(a, m, 0.25, inner=HW, C=C), R, HW, C).view(R, C * HW)
    assert torch.equal(out, want) and bool((tail == SENT).all())
    assert float(out.abs().max()) > 0 and abs(float(out[R - 1, 3 * HW + 2]) - float(a[R - 1, 2, 3]) * float(m[R - 1, 3]) / 0.75) <= 1e-6
    for act, slope in ((ops.ACT_RELU, 0.0), (ops.ACT_LRELU, 0.2)):
        d, dtail = _padded((R, HW, C))
        ops.drop2d_flatten_bwd(dflat, m, 0.25, y, R, HW, C, act=act, slope=slope, out=d)
        w = ops.nhwc_to_nchw_flat(dflat, R, HW, C, inverse=True).view(R, HW, C)
        w = ops.dropout_apply(w, m, 0.25, inner=HW, C=C, out=w)
        w = ops.act_bwd(w, y, act, slope, out=w)
        assert torch.equal(d, w) and bool((dtail == SENT).all())
        assert float(d.abs().max()) > 0


# ---- 2. the head against float64 ----------------------------------------------------------------------------------------------------
def _head_data(R, K, seed):
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32))      # noqa: E731
    return dict(h=t(np.maximum(rs.normal(0, 1, (R, 256)), 0)), m1=t(rs.random_sample((R, 256)) < 0.5), W2=t(rs.uniform(-1, 1, (K, 256)) / 16),
                b2=t(rs.uniform(-0.1, 0.1, K)), y=torch.from_numpy(rs.randint(0, K, R)))


def _run_head(ops, d, tally0=(1.5, 2.0, 3.0)):
    R, K = d["h"].shape[0], d["W2"].shape[0]
    bufs = {n: _padded(s) for n, s in (("logits", (R, K)), ("loss", (1,)), ("dW2", (K, 256)), ("db2", (K,)), ("dh", (R, 256)), ("db1", (256,)))}
    tally, ttail = _padded((3,), dtype=torch.float64)
    tally.copy_(torch.tensor(tally0, dtype=torch.float64))
    ops.mnist_clf_head(_dev(d["h"]), _dev(d["m1"]), 0.5, _dev(d["W2"]), _dev(d["b2"]), _dev(d["y"]), tally, **{n: v for n, (v, _) in bufs.items()})
    assert all(bool((tl == SENT).all()) for _, tl in bufs.values()) and bool((ttail == SENT).all()), "wrote outside its outputs"
    return {n: v.clone() for n, (v, _) in bufs.items()}, tally.clone()


@pytest.mark.parametrize("K", [3, 10, 16])
@pytest.mark.parametrize("R", [1, 5, 8, 15, 16, 17, 127, 128])           # 15, 16, 17, 127: the 16-row m-tile edges of mnist_clf_head_kernel
def test_head_against_float64(ops, R, K):
    d = _head_data(R, K, 17 * R + K)
    r64 = RS.head(d["h"].double(), d["m1"], 0.5, d["W2"].double(), d["b2"].double(), d["y"])
    r32 = RS.head(d["h"], d["m1"], 0.5, d["W2"], d["b2"], d["y"])
    (got, tally), (again, tally2) = _run_head(ops, d), _run_head(ops, d)
    assert all(torch.equal(got[n], again[n]) for n in got) and torch.equal(tally, tally2), "two runs differ"
    l64, l32, lm = float(r64["loss"]), float(r32["loss"]), float(got["loss"])
    print(f"head R{R} K{K}: loss {lm:.7f}  float64 {l64:.7f}  fp32 cpu {l32:.7f}")
    assert abs(lm - l64) <= max(2e-5, 3 * abs(l32 - l64))
    for n in ("logits", "dW2", "db2", "dh", "db1"):
        truth = r64[n]
        tol = max(1e-4 * float(truth.abs().max()), 3 * float((r32[n].double() - truth).abs().max()), 1e-8)
        err = float((got[n].cpu().double() - truth).abs().max())
        print(f"  {n}: err {err:.2e}  tol {tol:.2e}")
        assert np.isfinite(err) and err <= tol, (n, err, tol)
    hits = int((got["logits"].cpu().argmax(1) == d["y"]).sum())
    assert hits == r64["hits"], "a near-tie between fp32 and float64: choose another seed"
    t = tally.cpu().tolist()
    assert t[1] == 2.0 + hits and t[2] == 3.0 + R and abs(t[0] - 1.5 - lm * R) <= 1e-12 * max(1.0, lm * R)


def test_head_counts_a_tie_for_the_lower_index(ops):
    d = _head_data(5, 3, 99)
    d["W2"][1] = d["W2"][0]                                    # classes 0 and 1 tie exactly in every row: same operands, same order
    d["b2"] = torch.tensor([5.0, 5.0, -5.0])
    d["y"] = torch.tensor([0, 1, 0, 1, 2])
    got, tally = _run_head(ops, d, tally0=(0.0, 0.0, 0.0))
    lg = got["logits"].cpu()
    assert torch.equal(lg[:, 0], lg[:, 1]) and bool((lg[:, 0] > lg[:, 2]).all())
    assert tally.cpu().tolist()[1:] == [2.0, 5.0]              # the rows labelled 0; the rows labelled 1 lose the tie


def test_head_refuses_what_one_workgroup_cannot_hold(pcg, ops):
    for R, K, why in ((129, 10, "129 rows"), (128, 17, "17 classes")):
        d = _head_data(R, K, 1)
        with pytest.raises(pcg.PcgError, match=why):
            ops.mnist_clf_head(_dev(d["h"]), _dev(d["m1"]), 0.5, _dev(d["W2"]), _dev(d["b2"]), _dev(d["y"]), torch.zeros(3, dtype=torch.float64, device=DEV))


# ---- 3. batch entry -------------------------------------------------------------------------------------------------------------------
def test_batch_launch_rows_masks_and_counter(pcg, ops):
    rs = np.random.RandomState(5)
    N, D, seed = 166, 50, 21
    Xh, Yh, permh = rs.random_sample((N, D)).astype(np.float32), rs.randint(0, 10, N), rs.permutation(N)
    X, Y, perm = _dev(torch.from_numpy(Xh)), _dev(torch.from_numpy(Yh)), _dev(torch.from_numpy(permh))
    bufs = lambda B: ((torch.empty((B, D), device=DEV), torch.empty((B,), dtype=torch.int64, device=DEV)),      # noqa: E731
                      [torch.empty((B, w), device=DEV) for w in RS.WIDTHS])
    a, b = ops.DeviceRNG(seed), ops.DeviceRNG(seed)
    for r in (a, b):
        r.rand((7,), DEV)                                      # the stream does not start at offset 0
    ctr = a.device_counter(DEV, cursor=True)
    cur, off = 0, 2
    for B in (73, 73, 20):                                     # 166 = 73 + 73 + a short tail
        (x1, y1), m1 = bufs(B)
        a.mnist_clf_batch(X, Y, perm, (x1, y1), m1, RS.KEEPS, counter=ctr)
        (x2, y2), m2 = bufs(B)
        b.mnist_clf_batch(X, Y, perm, (x2, y2), m2, RS.KEEPS, cursor=cur)
        hx, hy, hm, off = RS.batch_host(Xh, Yh, permh, cur, B, seed, off)
        cur += B
        assert torch.equal(x1, x2) and torch.equal(y1, y2) and all(torch.equal(u, v) for u, v in zip(m1, m2))
        assert np.array_equal(x2.cpu().numpy(), hx) and np.array_equal(y2.cpu().numpy(), hy)
        assert all(np.array_equal(u.cpu().numpy(), v) for u, v in zip(m2, hm))
        assert ctr.tolist() == [off, 0, cur, 0] and b.offset == off
    assert a.offset == 2                                       # the counter form leaves the host offset alone (rand((7,)) took 2)
    with pytest.raises(pcg.PcgError, match="permutation of"):
        b.mnist_clf_batch(X, Y, perm, bufs(73)[0], bufs(73)[1], RS.KEEPS, cursor=N - 73 + 1)


# ---- 4. the reference's own steps -----------------------------------------------------------------------------------------------------
def test_golden_steps_teacher_forced_and_free_run(pcg, golden_dir):
    K = pcg.countergan
    gold = dict(np.load(os.path.join(golden_dir, "classifier_pretrain_mnist.npz")))
    torch.manual_seed(5)
    o64 = CR.CNNClassifier()
    init = {k: v.clone() for k, v in o64.state_dict().items()}
    for k, v in init.items():
        np.testing.assert_array_equal(_digest(v), gold[f"init.{k}"], err_msg=k)
    o32 = CR.CNNClassifier(); o32.load_state_dict(init)
    o64 = o64.double()
    opt64 = torch.optim.Adam(o64.parameters(), lr=1e-3)
    mine = K.CNNClassifier(); mine.load_state_dict(init)
    mine = mine.to(DEV)
    fit = K.ClassifierFit(mine, gold["x0"], gold["y0"], 8, lr=1e-3, graph=False)
    batches = [(torch.from_numpy(gold[f"x{i}"]), torch.from_numpy(gold[f"y{i}"]),
                (torch.from_numpy(gold[f"mask{2 * i}"]), torch.from_numpy(gold[f"mask{2 * i + 1}"]))) for i in range(2)]
    for i, (x, y, masks) in enumerate(batches):
        sd = {k: v.float() for k, v in o64.state_dict().items()}
        o32.load_state_dict(sd); mine.load_state_dict(sd)                       # teacher forcing: same starting point
        o32.train(); o32.zero_grad()
        l32 = F.cross_entropy(CR.classifier_forward_train(o32, x, masks), y); l32.backward()
        l64 = CR.classifier_train_step(o64, opt64, x.double(), y, masks)       # advances the teacher
        lm = fit.run_batch(_dev(x), _dev(y), [_dev(m) for m in masks]).item()
        print(f"step {i}: loss {lm:.7f}  float64 {l64:.7f}  fp32 oracle {l32.item():.7f}")
        assert abs(lm - l64) <= max(2e-5, 3 * abs(l32.item() - l64)), (i, lm, l64)
        named = list(zip(mine.named_parameters(), o32.named_parameters(), o64.named_parameters()))
        assert len(named) == 10
        for (n, p), (_, q32), (_, q64) in named:
            truth = q64.grad
            tol = max(1e-4 * float(truth.abs().max()), 3 * float((q32.grad.double() - truth).abs().max()), 1e-8)
            err = float((p.grad.cpu().double() - truth).abs().max())
            print(f"  grad {n}: err {err:.2e}  tol {tol:.2e}")
            assert err <= tol, (f"step {i} grad {n}", err, tol)
    assert fit.read_tally()[2] == 16.0
    mine.load_state_dict(init)                                                  # free run from the initial state, Adam included
    for x, y, masks in batches:
        fit.run_batch(_dev(x), _dev(y), [_dev(m) for m in masks])
        fit.optimizer.step()
    for k in ("fc.4.weight", "conv.0.weight"):
        assert float(np.abs(mine.state_dict()[k].cpu().numpy() - gold[f"final.{k}.full"]).max()) <= 2.2 * 1e-3 * 2 + 1e-5, k
    for k, v in mine.state_dict().items():
        np.testing.assert_allclose(_digest(v)[3:], gold[f"final.{k}"][3:], rtol=0, atol=2.2 * 1e-3 * 2 + 1e-5, err_msg=k)


# ---- 5. replay equals eager -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 257])                       # 128 + 128 + 44; 128 + 128 + a tail of ONE row
def test_replays_equal_the_eager_entries(pcg, N):
    K, ops = pcg.countergan, pcg.ops
    rs = np.random.RandomState(6)
    X, y = rs.uniform(-1, 1, (N, 1, 28, 28)).astype(np.float32), rs.randint(0, 10, N)
    perm = torch.from_numpy(rs.permutation(N))
    torch.manual_seed(3)
    init = {k: v.clone() for k, v in K.CNNClassifier().state_dict().items()}
    states = []
    for graph in (True, False):
        model = K.CNNClassifier()
        model.load_state_dict(init)
        model = model.to(DEV)
        rng = ops.DeviceRNG(9)
        rng.rand((5,), DEV)
        fit = K.ClassifierFit(model, X, y, 128, rng=rng, graph=graph)
        assert fit.steps_per_epoch == 3 and rng.offset == 2, "building the fit must not advance the stream"
        assert all(torch.equal(v.cpu(), init[k]) for k, v in model.state_dict().items()), "building the fit must not move the parameters"
        fit.new_epoch(perm)
        recs = []
        for _ in range(3):
            rec = {}
            fit.step(record=rec)
            recs.append(rec)
        with pytest.raises(pcg.PcgError, match="used up"):
            fit.step()
        states.append(({k: v.clone() for k, v in model.state_dict().items()}, recs, fit.read_tally(), rng.offset))
    (sa, ra, ta, oa), (sb, rb, tb, ob) = states
    assert ta == tb and ta[2] == float(N) and oa == ob == 2 + 2 * RS.batch_span(128) + RS.batch_span(N - 256)
    for u, v in zip(ra, rb):
        assert torch.equal(u["x"], v["x"]) and torch.equal(u["y"], v["y"]) and torch.equal(u["loss"], v["loss"])
        assert all(torch.equal(p, q) for p, q in zip(u["masks"], v["masks"]))
        assert bool(torch.isfinite(u["loss"]).all())
    assert torch.equal(ra[0]["x"].cpu(), torch.from_numpy(X).reshape(N, -1)[perm[:128]]) and ra[2]["x"].shape[0] == N - 256
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        assert not torch.equal(sa[k].cpu(), init[k]), f"{k} did not move"


# ---- 6. the chain's batches and masks --------------------------------------------------------------------------------------------------
def test_same_batches_and_masks_as_the_chain(pcg):
    K, ops, data = pcg.countergan, pcg.ops, pcg.data
    rs = np.random.RandomState(8)
    N, seed = 300, 4
    X, y = _dev(torch.from_numpy(rs.uniform(-1, 1, (N, 1, 28, 28)).astype(np.float32))), _dev(torch.from_numpy(rs.randint(0, 10, N)))
    chain_rng, chain = ops.DeviceRNG(11), []
    for xb, yb in data.DeviceLoader(X, y, 128, True, seed):     # what train_classifier's loop sees, and what CNNClassifier.forward draws
        B = xb.shape[0]
        chain.append((xb, yb, chain_rng.bernoulli((B, 128), DEV, 0.75), chain_rng.bernoulli((B, 256), DEV, 0.5)))
    fit = K.ClassifierFit(K.CNNClassifier().to(DEV), X, y, 128, rng=ops.DeviceRNG(11), graph=False)
    fit.new_epoch(data.DeviceLoader(X, y, 128, True, seed).epoch_order())
    assert len(chain) == fit.steps_per_epoch == 3
    for xb, yb, m0, m1 in chain:
        rec = {}
        fit.step(record=rec)
        assert torch.equal(rec["x"], xb.reshape(xb.shape[0], -1)) and torch.equal(rec["y"], yb)
        assert torch.equal(rec["masks"][0], m0) and torch.equal(rec["masks"][1], m1)
    assert fit.rng.offset == chain_rng.offset


# ---- 7. countergan.train_classifier(fused=True) ----------------------------------------------------------------------------------------
def _digits(n, seed):
    """Ten fixed templates (7x7 blocks of +-1, upsampled to 28x28) plus noise, in [-1, 1]: separable, so three short epochs learn it."""
    y = np.random.RandomState(seed).randint(0, 10, n)
    blocks = np.random.RandomState(0).choice([-1.0, 1.0], size=(10, 7, 7))
    t = np.kron(blocks, np.ones((4, 4)))
    x = np.clip(t[y] + 0.3 * np.random.RandomState(seed + 1).standard_normal((n, 28, 28)), -1, 1)
    return torch.from_numpy(x[:, None].astype(np.float32)), torch.from_numpy(y)


class _Cfg:
    cls_lr, num_epochs_clf, classifier_path = 1e-3, 3, None


def _chain_eval_hits(K, state, xv, yv):
    c = K.CNNClassifier()
    c.load_state_dict(state)
    c = c.to(DEV).eval()
    with torch.no_grad():
        return int((c(xv).cpu().argmax(1) == yv.cpu()).sum())


def test_train_classifier_fused_learns_with_one_host_read_per_epoch(pcg, monkeypatch, capsys):
    K, data = pcg.countergan, pcg.data
    (xt, yt), (xv, yv) = _digits(600, 1), _digits(200, 7)
    xt, yt, xv, yv = _dev(xt), _dev(yt), _dev(xv), _dev(yv)
    torch.manual_seed(2)
    clf = K.CNNClassifier().to(DEV)
    states, reads = [], {"cpu": 0, "item": 0}
    real_read = K.ClassifierFit.read_tallies

    def read_tallies(self):
        states.append({k: v.clone() for k, v in self.classifier.state_dict().items()})
        return real_read(self)

    monkeypatch.setattr(K.ClassifierFit, "read_tallies", read_tallies)
    for name in ("cpu", "item"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda self, *a, **k: (reads.__setitem__(name, reads[name] + 1), real(self, *a, **k))[1])(real, name))
    K._fused_fallback_warned = False
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*op chain.*")  # the reference's net at batch 128 must not fall back
        hist = K.train_classifier(clf, data.DeviceLoader(xt, yt, 128, True, 3), data.DeviceLoader(xv, yv, 128, False), _Cfg, DEV, save=False, fused=True)
    monkeypatch.undo()
    print(f"validation accuracies {hist}; host reads {reads}")
    assert reads == {"cpu": 3, "item": 0}, "one host read per epoch, through read_tallies"
    assert len(hist) == len(states) == 3 and capsys.readouterr().out.count("[Classifier] Epoch") == 3
    for acc, st in zip(hist, states):
        assert acc == _chain_eval_hits(K, st, xv, yv) / 200.0
    assert hist[-1] > 0.9
    assert all(torch.equal(v, states[-1][k]) for k, v in clf.state_dict().items())
    ref = CR.CNNClassifier()
    ref.load_state_dict({k: v.cpu() for k, v in clf.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        assert float((ref(xv.cpu()).argmax(1) == yv.cpu()).float().mean()) > 0.9


@pytest.mark.parametrize("case", ["plain list", "batch 160"])
def test_fallback_warns_and_runs_the_chain(pcg, case):
    K, data = pcg.countergan, pcg.data
    (xt, yt), (xv, yv) = _digits(320, 1), _digits(64, 7)
    xt, yt, xv, yv = _dev(xt), _dev(yt), _dev(xv), _dev(yv)
    train = [(xt[:160], yt[:160]), (xt[160:], yt[160:])] if case == "plain list" else data.DeviceLoader(xt, yt, 160, True, 3)

    class Cfg(_Cfg):
        num_epochs_clf = 1

    K._fused_fallback_warned = False
    with pytest.warns(RuntimeWarning, match="op chain"):
        hist = K.train_classifier(K.CNNClassifier().to(DEV), train, data.DeviceLoader(xv, yv, 64, False), Cfg, DEV, save=False, fused=True)
    assert len(hist) == 1 and 0.0 <= hist[0] <= 1.0


# ---- 8. launch census --------------------------------------------------------------------------------------------------------------------
def test_launch_census(pcg, monkeypatch):
    K, ops = pcg.countergan, pcg.ops
    calls = []
    real_check = ops.check
    monkeypatch.setattr(ops, "check", lambda rc, what="": (calls.append(what), real_check(rc, what))[1])
    rs = np.random.RandomState(9)
    N = 300
    X, y = rs.uniform(-1, 1, (N, 1, 28, 28)).astype(np.float32), rs.randint(0, 10, N)
    fit = K.ClassifierFit(K.CNNClassifier().to(DEV), X, y, 128, graph=False)
    del calls[:]
    fit.new_epoch(torch.arange(N))
    per_step = []
    for _ in range(3):
        n0 = len(calls)
        fit.step()
        per_step.append(calls[n0:])
    print(f"eager epoch of 3 batches: {len(calls)} library calls; step 2: {per_step[1]}")
    for w in ("pcg_mnist_clf_batch", "pcg_drop2d_flatten_fwd", "pcg_drop2d_flatten_bwd", "pcg_mnist_clf_head", "pcg_adam_step_capturable"):
        assert calls.count(w) == 3 and all(s.count(w) == 1 for s in per_step), w
    gone = ("pcg_dropout_apply", "pcg_rand_bernoulli", "pcg_nhwc_to_nchw_flat", "pcg_act_fwd", "pcg_cross_entropy_fwd_bwd", "pcg_fill")
    assert not [w for s in per_step[1:] for w in s if w in gone]
    assert not [w for w in calls if w in gone and w != "pcg_fill"]          # (pcg_fill: the fresh Adam moments, in the first step)
    assert per_step[0].count("pcg_conv2d fwd") == 4 and per_step[2].count("pcg_conv2d fwd") == 4      # conv1..3 and fc1 as a 1x1
