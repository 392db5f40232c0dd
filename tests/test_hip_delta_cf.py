"""GPU: the prompted half of the additive-delta MNIST CounteRGAN and its random-target training (pcgan_amd.gan_train)
against the reference's recorded runs (tests/golden/delta_cf_ref.npz, written by tests/golden/make_golden_delta_cf.py).

The rule is tests/test_hip_delta_gan.py's.  A quantity passes against float64 if (a) rtol 1e-4, atol 2e-5 * max|reference|, or (b) it is
within 3x the recorded distance of the reference's own fp32 run from its float64 run.  Discrete outputs (pred, flip) are compared
outside the recorded near set -- the queries whose float64 top-two probability gap is under max(1e-6, 100 * max|p_fp32 - p_fp64|), at
most 5 % of them -- and a group's flip sum may differ by at most its number of near queries.  Everything runs on the seeded nets of
tests/delta_gan_restate.py at B = 4 and B = 3; training is three steps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_cf_restate as CR  # noqa: E402
import delta_gan_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCORE = ("pred", "conf", "p_target", "p_true", "p_orig_true", "flip")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "delta_cf_ref.npz")))


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


def _params(T, **kw):
    return dict(T.params_random_target, **kw)


def _rule(got, want64, dist, what):
    want64 = np.asarray(want64, np.float64)
    atol = max(2e-5 * float(np.abs(want64).max()), 3.0 * float(np.max(dist)))
    err = float(np.abs(np.asarray(got, np.float64) - want64).max())
    print(f"{what}: max error {err:.3e}, atol {atol:.3e} (rule a {2e-5 * float(np.abs(want64).max()):.3e}, rule b {3.0 * float(np.max(dist)):.3e})")
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=atol, err_msg=what)


def _batch(B):
    x, y = RS.batches(B)[0]
    return x.to(DEV), y.to(DEV), x, y


_orig = {}


def _p_orig_true(B):
    """float64 softmax of the classifier on the original rows at the true class: what p_orig_true restates."""
    if B not in _orig:
        x, y = RS.batches(B)[0]
        p = torch.softmax(PR.forward(RS.classifier_state(torch.float64), x.double())["logits"], dim=1)
        _orig[B] = p[torch.arange(B), y].numpy()
    return _orig[B]


def _check_scores(res, gold, B, tq, bq, near, what):
    """The score fields of queries (tq[i], bq[i]) against the recorded float64 sweep."""
    probs, y = gold[f"B{B}.sweep.probs.f64"], gold[f"B{B}.y"]
    pd = gold[f"B{B}.sweep.probs.dist"]
    want_p = probs[tq, bq]
    _rule(res["conf"].cpu().numpy().reshape(-1), gold[f"B{B}.sweep.confs.f64"][tq, bq], gold[f"B{B}.sweep.confs.dist"], what + " conf")
    _rule(res["p_target"].cpu().numpy().reshape(-1), want_p[np.arange(len(tq)), tq], pd, what + " p_target")
    _rule(res["p_true"].cpu().numpy().reshape(-1), want_p[np.arange(len(tq)), y[bq]], pd, what + " p_true")
    _rule(res["p_orig_true"].cpu().numpy().reshape(-1), _p_orig_true(B)[bq], pd, what + " p_orig_true")
    pred64 = gold[f"B{B}.sweep.preds.f64"][tq, bq]
    pred, flip = res["pred"].cpu().numpy().reshape(-1), res["flip"].cpu().numpy().reshape(-1)
    assert res["pred"].dtype == torch.int64
    np.testing.assert_array_equal(pred[~near], pred64[~near], err_msg=what + " pred outside the near set")
    np.testing.assert_array_equal(flip[~near], (pred64 == tq).astype(np.float32)[~near], err_msg=what + " flip outside the near set")
    np.testing.assert_array_equal(flip, (pred == tq).astype(np.float32))
    _rule(res["sums"].cpu().numpy().reshape(-1, 3), gold[f"B{B}.sweep.sums.f64"][tq, bq], gold[f"B{B}.sweep.sums.dist"], what + " sums")


# ---- counterfactuals and the sweep against the float64 recording --------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 3])
def test_per_row_query_with_a_hit_and_a_miss_against_float64(T, gold, B):
    G, _, C = _nets(T)
    xd, yd, x, y = _batch(B)
    pred64, near = gold[f"B{B}.sweep.preds.f64"], gold[f"B{B}.sweep.near"]
    hits = (pred64 == np.arange(CR.K)[:, None]) & ~near
    assert hits.any()
    t_hit, b_hit = (int(v[0]) for v in np.nonzero(hits))
    targets = np.asarray([(3 * b + 1) % CR.K for b in range(B)])                # any classes; then one sure hit, and a sure miss beside it
    targets[b_hit] = t_hit
    b_miss = (b_hit + 1) % B
    targets[b_miss] = next(t for t in range(CR.K) if pred64[t, b_miss] != t and not near[t, b_miss])
    bq = np.arange(B)
    res = T.counterfactuals(G, C, xd, torch.from_numpy(targets), y_true=yd)
    assert res["x_cf"].shape == res["delta"].shape == (B, 1, 28, 28) and res["sums"].shape == (B, 3) and res["group_sums"].shape == (1, 1, 8)
    _check_scores(res, gold, B, targets, bq, near[targets, bq], "per-row")
    flip = res["flip"].cpu().numpy()
    assert flip[b_hit] == 1.0 and flip[b_miss] == 0.0 and int(res["pred"][b_hit]) == t_hit
    if B == 4:
        d64 = gold["B4.sweep.delta.f64"][targets, bq]
        _rule(res["delta"].cpu().numpy(), d64, gold["B4.sweep.delta.dist"], "delta")
        _rule(res["x_cf"].cpu().numpy(), np.clip(x.double().numpy() + d64, -1, 1), gold["B4.sweep.x_cf.dist"], "x_cf")
    one = T.counterfactuals(G, C, xd, int(t_hit), y_true=yd)                    # an int: that class for every row
    _check_scores(one, gold, B, np.full(B, t_hit), bq, near[t_hit], "one class")


@pytest.mark.parametrize("B", [4, 3])
def test_random_target_query_against_the_recorded_lines_162_to_172(T, gold, B):
    G, _, C = _nets(T)
    xd, _, _, _ = _batch(B)
    targets = torch.from_numpy(gold[f"B{B}.query.targets"])
    got_t, x_cf, delta, pred, conf = T.evaluate_examples(G, C, xd, targets=targets)
    assert torch.equal(got_t.cpu(), targets)
    for name, got in (("x_cf", x_cf), ("delta", delta), ("confs", conf)):
        _rule(got.cpu().numpy(), gold[f"B{B}.query.{name}.f64"], gold[f"B{B}.query.{name}.dist"], "query " + name)
    near = gold[f"B{B}.query.near"]
    np.testing.assert_array_equal(pred.cpu().numpy()[~near], gold[f"B{B}.query.preds.f64"][~near])
    assert float(x_cf.abs().max()) <= 1.0
    from pcgan_amd import ops
    rng = ops.DeviceRNG(9)
    drawn, _, _, pred2, _ = T.evaluate_examples(G, C, xd, rng=rng)             # :162 on the device
    assert rng.offset == 1 and drawn.shape == (B,) and int(drawn.min()) >= 0 and int(drawn.max()) < CR.K and pred2.shape == (B,)


@pytest.mark.parametrize("B", [4, 3])
def test_sweep_against_float64(T, gold, B):
    G, _, C = _nets(T)
    xd, yd, x, _ = _batch(B)
    res = T.counterfactual_sweep(G, C, xd, y_true=yd)
    Tn = CR.K
    assert res["x_cf"].shape == (Tn, B, 1, 28, 28) and res["pred"].shape == (Tn, B) and res["sums"].shape == (Tn, B, 3)
    assert res["group_sums"].shape == (Tn, 1, 8)
    tq, bq = np.repeat(np.arange(Tn), B), np.tile(np.arange(B), Tn)
    near = gold[f"B{B}.sweep.near"]
    _check_scores(res, gold, B, tq, bq, near.reshape(-1), "sweep")
    if B == 4:
        d64 = gold["B4.sweep.delta.f64"]
        _rule(res["delta"].cpu().numpy(), d64, gold["B4.sweep.delta.dist"], "delta")
        _rule(res["x_cf"].cpu().numpy(), np.clip(x.double().numpy()[None] + d64, -1, 1), gold["B4.sweep.x_cf.dist"], "x_cf")
    gs = res["group_sums"].cpu().double().numpy()[:, 0]
    pred64, probs, y = gold[f"B{B}.sweep.preds.f64"], gold[f"B{B}.sweep.probs.f64"], gold[f"B{B}.y"]
    flips64 = (pred64 == np.arange(Tn)[:, None]).sum(1)
    assert (np.abs(gs[:, 0] - flips64) <= near.sum(1)).all(), "a group's flip sum differs by at most its near queries"
    np.testing.assert_array_equal(gs[:, 7], np.full(Tn, B))
    gain = (probs[np.arange(Tn)[:, None], np.arange(B)[None], np.arange(Tn)[:, None]] - probs[:, np.arange(B), y]).sum(1)
    _rule(gs[:, 2], gain, B * gold[f"B{B}.sweep.probs.dist"] * 2, "group gain")
    _rule(gs[:, 4:7], gold[f"B{B}.sweep.sums.f64"].sum(1), B * gold[f"B{B}.sweep.sums.dist"], "group tail sums")
    two = T.counterfactual_sweep(G, C, xd, y_true=yd, group_rows=2)["group_sums"]
    assert two.shape == (Tn, (B + 1) // 2, 8) and torch.equal(two[..., 7].sum(1), res["group_sums"][:, 0, 7])


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------------------
def test_sweep_equals_ten_queries_chunks_equal_one_window_and_the_batch_helper(T):
    G, _, C = _nets(T)
    B = 5
    gen = torch.Generator().manual_seed(21)
    x = (1.5 * (2 * torch.rand(B, 1, 28, 28, generator=gen) - 1)).to(DEV)       # some pixels beyond [-1, 1]: the clamp acts
    y = torch.randint(0, CR.K, (B,), generator=gen).to(DEV)
    sw = T.counterfactual_sweep(G, C, x, y_true=y)
    keys = ("x_cf", "delta", "sums") + SCORE
    for t in range(CR.K):
        one = T.counterfactuals(G, C, x, t, y_true=y)
        for k in keys:
            assert torch.equal(sw[k][t], one[k]), (t, k)
        assert torch.equal(sw["group_sums"][t], one["group_sums"][0]), t
    for chunk in (7, 1):
        ch = T.counterfactual_sweep(G, C, x, y_true=y, query_chunk=chunk)
        for k in keys + ("group_sums",):
            assert torch.equal(ch[k], sw[k]), (chunk, k)
    targets = torch.tensor([5, 0, 9, 5, 2], device=DEV)
    q = T.counterfactuals(G, C, x, targets, query_chunk=2)
    cf, delta = T.counterfactual_batch(G, x, targets)
    assert torch.equal(q["x_cf"], cf) and torch.equal(q["delta"], delta)
    assert float((x + delta).abs().max()) > 1.0 and float(cf.abs().max()) <= 1.0
    assert not q["x_cf"].requires_grad


# ---- per-target evaluation over a ragged loader -----------------------------------------------------------------------------------------------
def _count_reads(monkeypatch):
    reads = {"cpu": 0, "item": 0, "tolist": 0}
    for name in reads:
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda self, *a, **k: (
            reads.__setitem__(name, reads[name] + (1 if self.is_cuda else 0)), real(self, *a, **k))[1])(real, name))
    return reads


def test_evaluate_per_target_over_a_ragged_loader(T, gold, monkeypatch, capsys):
    G, _, C = _nets(T)
    loader = [_batch(4)[:2], _batch(3)[:2]]
    reads = _count_reads(monkeypatch)
    got = T.evaluate_per_target(G, C, loader, one_pass=True)
    monkeypatch.undo()
    print(f"device-to-host reads {reads}")
    assert reads == {"cpu": 1, "item": 0, "tolist": 0}, "one device-to-host read for the whole loader"
    from pcgan_amd import countergan as CG
    assert capsys.readouterr().out.startswith(CG.per_class_csv(got, fields=T.EVAL_FIELDS))
    want = CR.fold([{k: gold[f"B{B}.sweep.{k}.f64"] for k in CR.METRICS} for B in (4, 3)])
    for k in CR.METRICS:
        g = np.asarray([got[t][k] for t in range(CR.K)])
        dist = max(float(gold[f"B{B}.sweep.{k}.dist"].max()) for B in (4, 3))
        if k == "class_flip_rate":                                             # discrete: a batch's rate may move by its near queries
            slack = np.mean([gold[f"B{B}.sweep.near"].sum(1) / B for B in (4, 3)], axis=0)
            print(f"class_flip_rate: {g} against {want[k]}, slack {slack}")
            assert (np.abs(g - want[k]) <= slack + 1e-12).all()
        else:
            _rule(g, want[k], dist, k)
    loop = T.evaluate_per_target(G, C, loader, one_pass=False, verbose=False)
    for t in range(CR.K):
        np.testing.assert_allclose([got[t][k] for k in T.EVAL_FIELDS], [loop[t][k] for k in T.EVAL_FIELDS], rtol=1e-6, atol=0.0, err_msg=str(t))
    chunked = T.evaluate_per_target(G, C, loader, query_chunk=7, verbose=False)
    assert chunked == got


# ---- random-target training ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 3])
def test_three_fused_steps_with_the_recorded_classes_match_float64(T, gold, B):
    G, D, C = _nets(T)
    stepper = T.GraphedTrainStep(G, D, C, B, _params(T), graph=True)
    classes = gold[f"B{B}.classes"].tolist()
    for i, ((x, y), c) in enumerate(zip(RS.batches(B), classes)):
        out = stepper.step(x.to(DEV), y.to(DEV), torch.full((B,), c, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        for name in CR.LOSSES:
            _rule(float(out[name].cpu()), gold[f"B{B}.{name}.f64"][i], gold[f"B{B}.{name}.dist"][i], f"step {i + 1} {name}")


def _loader():
    gen = torch.Generator().manual_seed(3)
    x = (2 * torch.rand(11, 1, 28, 28, generator=gen) - 1).to(DEV)
    y = torch.randint(0, 10, (11,), generator=gen).to(DEV)
    return [(x[i:i + 4], y[i:i + 4]) for i in range(0, 11, 4)]                   # two full batches and a tail of 3


def _model_classes(seed, n, start=0):
    from oracle import rng_np
    return [int(rng_np.randint(1, 0, CR.K, seed, start + i)[0][0]) for i in range(n)]


def _epochs(T, epochs, seed=None, classes=None, graph=True, start=0):
    """The loader `epochs` times through one stepper: drawn by the step itself (seed) or with `classes` passed explicitly."""
    from pcgan_amd import ops
    G, D, C = _nets(T)
    rng = ops.DeviceRNG(seed if seed is not None else 0)
    rng.offset = start
    stepper = T.GraphedTrainStep(G, D, C, 4, _params(T), graph=graph, rng=rng)
    rec, it = [], iter(classes or [])
    for _ in range(epochs):
        for x, y in _loader():
            target = None if classes is None else torch.full_like(y, next(it))
            out = stepper.step(x, y, target)
            rec.append(torch.cat([out[k] for k in CR.LOSSES]).clone())
    torch.cuda.synchronize()
    return G.flat_params.clone(), D.flat_params.clone(), torch.stack(rec).cpu(), stepper, rng


def test_drawn_replays_equal_the_host_models_classes_passed_explicitly(T):
    seed, start = 41, 2 ** 32 - 2                                                # the counter's low word wraps inside the run
    classes = _model_classes(seed, 6, start)
    assert len(set(classes)) > 1
    g1, d1, l1, s1, rng = _epochs(T, 2, seed=seed, start=start)
    assert sorted(s1._draw_graphs) == [3, 4] and not s1._graphs, "one drawn graph per batch size met"
    assert rng.offset == start + 6 and s1._ctr.cpu().tolist() == [start + 6, 0], "rng.offset is the device counter after the epochs"
    assert s1._bufs[3]["t"].cpu().tolist() == [classes[5]] * 3 and s1._bufs[4]["t"].cpu().tolist() == [classes[4]] * 4
    g2, d2, l2, s2, rng2 = _epochs(T, 2, seed=seed, classes=classes, start=start)
    assert sorted(s2._graphs) == [3, 4] and not s2._draw_graphs and rng2.offset == start
    assert torch.equal(l1, l2), (l1, l2)
    assert torch.equal(g1, g2) and torch.equal(d1, d2)
    g3, d3, l3, _, _ = _epochs(T, 2, seed=seed, graph=False, start=start)       # the same entries issued eagerly
    assert torch.equal(l1, l3) and torch.equal(g1, g3) and torch.equal(d1, d3)
    assert bool(torch.isfinite(l1).all()) and l1.shape == (6, 5)


def test_train_gan_random_target_fused_chain_and_given_targets(T, monkeypatch):
    import warnings
    from pcgan_amd import PcgError, ops
    seed = 41
    classes = _model_classes(seed, 6)
    _, _, want, _, _ = _epochs(T, 2, seed=seed)
    p = _params(T, batch_size=4, epochs_gan=2)
    G, D, C = _nets(T)
    rng = ops.DeviceRNG(seed)
    reads = _count_reads(monkeypatch)
    T._fused_fallback_warned = False
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*op chain.*")
        hist = T.train_gan(G, D, C, _loader(), p, fused=True, rng=rng, verbose=False)
    monkeypatch.undo()
    assert reads == {"cpu": 2, "item": 0, "tolist": 0}, "one host read per epoch"
    assert rng.offset == 6
    assert hist["d_losses"] == [float(want[2, 0]), float(want[5, 0])] and hist["g_losses"] == [float(want[2, 1]), float(want[5, 1])]
    G, D, C = _nets(T)                                                          # targets= replaces the draws: the same numbers, no rng
    given = T.train_gan(G, D, C, _loader(), p, fused=True, targets=classes, verbose=False)
    assert given == hist
    G, D, C = _nets(T)                                                          # the op chain: offset by value, rng.offset advances
    rng = ops.DeviceRNG(seed)
    chain = T.train_gan(G, D, C, _loader(), p, rng=rng, verbose=False)
    G, D, C = _nets(T)
    chain_given = T.train_gan(G, D, C, _loader(), p, targets=classes, verbose=False)
    assert rng.offset == 6 and chain == chain_given
    np.testing.assert_allclose(chain["d_losses"] + chain["g_losses"], hist["d_losses"] + hist["g_losses"], rtol=1e-4)
    G, D, C = _nets(T)
    with pytest.raises(PcgError, match="ran out at iteration 6"):
        T.train_gan(G, D, C, _loader(), p, targets=classes[:5], verbose=False)
    with pytest.raises(PcgError, match="needs rng"):
        T.train_gan(G, D, C, _loader(), p, fused=True, verbose=False)
    with pytest.raises(PcgError, match="without rng"):
        T.GraphedTrainStep(G, D, C, 4, p).step(*_loader()[0])


def _library_calls(ops, run):
    calls, real = [], ops.check
    ops.check = lambda rc, what="": (calls.append(what), real(rc, what))[1]
    try:
        run()
    finally:
        ops.check = real
    torch.cuda.synchronize()
    return [c for c in calls if c != "pcg_conv_precision_set"]                  # host-only


def test_fixed_target_keeps_its_64_launches_and_the_drawn_step_has_65(T):
    from pcgan_amd import ops
    x, y = _loader()[0]
    G, D, C = _nets(T)
    fixed = T.GraphedTrainStep(G, D, C, 4, dict(T.params), graph=False)
    t5 = torch.full_like(y, 5)
    fixed.step(x, y, t5)                                                        # first step: builds the Adam state
    calls = _library_calls(ops, lambda: fixed.step(x, y, t5))
    assert len(calls) == 64 and "pcg_delta_gan_target_draw" not in calls, (len(calls), calls)
    G, D, C = _nets(T)
    drawn = T.GraphedTrainStep(G, D, C, 4, _params(T), graph=False, rng=ops.DeviceRNG(1))
    drawn.step(x, y)
    calls2 = _library_calls(ops, lambda: drawn.step(x, y))
    assert len(calls2) == 65 and calls2[0] == "pcg_delta_gan_target_draw" and calls2[1:] == calls, (len(calls2), calls2)
    # train_gan with target_class = 5 and an rng at hand: the fixed path, graphs without a draw, the rng untouched
    G, D, C = _nets(T)
    rng = ops.DeviceRNG(1)
    seen = []
    real = T.GraphedTrainStep.step
    T.GraphedTrainStep.step = lambda self, *a, **k: (seen.append(self), real(self, *a, **k))[1]
    try:
        calls3 = _library_calls(ops, lambda: T.train_gan(G, D, C, _loader(), dict(T.params, batch_size=4, epochs_gan=1), fused=True, rng=rng,
                                                         verbose=False))
    finally:
        T.GraphedTrainStep.step = real
    assert "pcg_delta_gan_target_draw" not in calls3 and rng.offset == 0
    assert sorted(seen[0]._graphs) == [3, 4] and not seen[0]._draw_graphs and seen[0]._rng is None
