"""GPU: the moons CounteRGAN's counterfactual queries and evaluation in one launch (csrc/moons_cf_eval.hip through
pcgan_amd.moons_countergan) against the reference's own recorded evaluation (tests/golden/moons_cf_eval_ref.npz) and against a
float64 oracle written here: the generator and the classifier as torch modules in .double() on the CPU, eval mode.

Tolerances.  Per-row values: test_hip_moons_cf.py's state form, rtol 1e-5, atol 1e-6 + 1e-5 max|ref|.  A group sum: the sum of its
rows' tolerances.  Metrics against the reference: class_flip atol 1e-6 (the reference rounds each batch mean to fp32), prediction_gain
and avg_actionability rtol 1e-4, atol 1e-6 (the trainer's logged scalars).  A predicted class is compared wherever the float64 top-2
logit margin is >= 1e-3."""
import csv
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-3
H64_SEED = 0
OUTS = ("raw_residual", "masked_residual", "x_cf", "logits_cf", "logits_x", "pred_cf", "pred_x", "gain")


# ---- float64 oracle ----------------------------------------------------------------------------------------------------------
class Net(nn.Module):
    def __init__(self, seq):
        super().__init__()
        self.net = seq


def o_generator(H):
    return Net(nn.Sequential(nn.Linear(7, H), nn.BatchNorm1d(H), nn.ReLU(), nn.Linear(H, H), nn.BatchNorm1d(H), nn.ReLU(),
                             nn.Linear(H, H // 2), nn.BatchNorm1d(H // 2), nn.ReLU(), nn.Linear(H // 2, 2))).double().eval()


def o_classifier():
    return Net(nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3))).double().eval()


def margin(logits):
    top = torch.topk(logits, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).numpy()


def oracle(oG, oC, x, t, mk):
    """x [N][2] float32, t [N] int64, mk [N][2] float32 (numpy) -> the per-row values in float64 (numpy)."""
    with torch.no_grad():
        xd, m, tt = torch.from_numpy(x).double(), torch.from_numpy(mk).double(), torch.from_numpy(t)
        raw = oG.net(torch.cat([xd, F.one_hot(tt, 3).double(), m], 1))
        masked = raw * m
        x_cf = xd + masked
        lcf, lx = oC.net(x_cf), oC.net(xd)
        ar = torch.arange(len(tt))
        gain = F.softmax(lcf, 1)[ar, tt] - F.softmax(lx, 1)[ar, tt]
        return {"raw_residual": raw.numpy(), "masked_residual": masked.numpy(), "x_cf": x_cf.numpy(), "logits_cf": lcf.numpy(),
                "logits_x": lx.numpy(), "pred_cf": lcf.argmax(1).numpy(), "pred_x": lx.argmax(1).numpy(), "gain": gain.numpy(),
                "margin_cf": margin(lcf), "margin_x": margin(lx)}


def row_tol(ref):
    return 1e-5 * np.abs(ref) + 1e-6 + 1e-5 * np.abs(ref).max()


def assert_rows(ours, ref, what, max_skipped=0.0):
    """Every per-row output against the oracle; returns the number of rows whose class was not compared."""
    for k in ("raw_residual", "masked_residual", "x_cf", "logits_cf", "logits_x", "gain"):
        got = ours[k].cpu().numpy()
        err = np.abs(got - ref[k])
        print(f"{what} {k}: max error / tolerance = {(err / row_tol(ref[k])).max():.3f}")
        assert (err <= row_tol(ref[k])).all(), f"{what} {k}: max error {err.max():.3e}"
    skipped = 0
    for k, mg in (("pred_cf", "margin_cf"), ("pred_x", "margin_x")):
        sure = ref[mg] >= MARGIN
        assert np.array_equal(ours[k].cpu().numpy()[sure], ref[k][sure]), f"{what} {k}"
        skipped = max(skipped, int((~sure).sum()))
    print(f"{what}: {skipped} of {len(ref['gain'])} rows under the margin")
    assert skipped <= max_skipped * len(ref["gain"]), f"{what}: {skipped} rows under the margin"
    return skipped


def h64_states(seed=H64_SEED):
    """A seeded hidden-64 generator with randomised BatchNorm running statistics, gamma and beta, as float32 state_dict values."""
    torch.manual_seed(seed)
    oG = o_generator(64)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (1, 4, 7):
            bn = oG.net[i]
            n = bn.num_features
            bn.running_mean.copy_(torch.randn(n, generator=g, dtype=torch.float64) * 0.5)
            bn.running_var.copy_(torch.rand(n, generator=g, dtype=torch.float64) * 1.5 + 0.5)
            bn.weight.copy_(torch.rand(n, generator=g, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.randn(n, generator=g, dtype=torch.float64) * 0.3)
            bn.num_batches_tracked.fill_(17)
    return {k: v.float() if v.is_floating_point() else v.clone() for k, v in oG.state_dict().items()}


def queries(N, seed):
    """Seeded per-row targets and masks (0 / 1, and a fractional one in every fourth row)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 3, (N,), generator=g)
    mk = torch.randint(0, 2, (N, 2), generator=g).float()
    mk[::4] = torch.rand(mk[::4].shape, generator=g)
    return t.numpy(), mk.numpy()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "moons_cf_eval_ref.npz")))


@pytest.fixture(scope="module")
def data():
    d = np.load(os.path.join(GOLD, "moons_cf_ref.npz"))
    return {k: d[f"data.{k}"] for k in ("X_train", "X_test", "y_train", "y_test")}


@pytest.fixture(scope="module")
def M():
    import pcgan_amd
    from pcgan_amd import moons_countergan
    pcgan_amd.load()
    return moons_countergan


def frozen(net):
    net.to(DEV).eval()
    for p in net.parameters():
        p.requires_grad = False
    return net


def pair(M, H, g_state, c_state):
    """(HIP generator, HIP classifier, float64 generator, float64 classifier) holding the same float32 values."""
    G, C = M.ResidualGenerator(2, H, 3), M.NNClassifier(2)
    G.load_state_dict(g_state); C.load_state_dict(c_state)
    oG, oC = o_generator(H), o_classifier()
    oG.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in g_state.items()})
    oC.load_state_dict({k: v.double() for k, v in c_state.items()})
    return frozen(G), frozen(C), oG, oC


@pytest.fixture(scope="module")
def shipped(M):
    return pair(M, 32, torch.load(os.path.join(GOLD, "moons_cf_generator_trained.pt"), map_location="cpu"),
                torch.load(os.path.join(GOLD, "moons_cf_classifier_trained.pt"), map_location="cpu"))


@pytest.fixture(scope="module")
def wide(M):
    return pair(M, 64, h64_states(), torch.load(os.path.join(GOLD, "moons_cf_classifier_trained.pt"), map_location="cpu"))


@pytest.fixture(scope="module")
def all_rows(data):
    """1200 rows: the training split, then the test split, float32."""
    return (np.concatenate([data["X_train"], data["X_test"]]).astype(np.float32),
            np.concatenate([data["y_train"], data["y_test"]]).astype(np.int64))


@pytest.fixture(scope="module")
def sweep_oracle(M, shipped, all_rows):
    """The float64 per-row values of every (mask, target, row) of the 1200 rows, computed once: {key: [4][3][1200]...}."""
    _, _, oG, oC = shipped
    X, _ = all_rows
    N = len(X)
    per = [[oracle(oG, oC, X, np.full(N, t, np.int64), np.broadcast_to(mv, (N, 2)).astype(np.float32).copy()) for t in range(3)]
           for mv in M.MASKS.values()]
    return {k: np.stack([np.stack([per[m][t][k] for t in range(3)]) for m in range(4)]) for k in per[0][0]}


def expected_sums(ref, y, N, group):
    """The group sums the oracle's per-row values give for the first N rows: (counts, flips sure, flips possible, gain, |masked|,
    and the tolerance of the two float sums), each [4][3][n_groups]."""
    ng = -(-N // group)
    shape = (4, 3, ng)
    cnt, lo, hi = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    gain, act, gtol, atol = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    gt, mt = row_tol(ref["gain"][:, :, :N]), row_tol(ref["masked_residual"][:, :, :N])
    for t in range(3):
        for g in range(ng):
            rows = np.arange(g * group, min((g + 1) * group, N))
            if y is not None:
                rows = rows[y[rows] != t]
            for m in range(4):
                hit, sure = ref["pred_cf"][m, t, rows] == t, ref["margin_cf"][m, t, rows] >= MARGIN
                cnt[m, t, g], lo[m, t, g], hi[m, t, g] = len(rows), (hit & sure).sum(), (hit | ~sure).sum()
                gain[m, t, g], act[m, t, g] = ref["gain"][m, t, rows].sum(), np.abs(ref["masked_residual"][m, t, rows]).sum()
                gtol[m, t, g], atol[m, t, g] = gt[m, t, rows].sum(), mt[m, t, rows].sum()
    return cnt, lo, hi, gain, act, gtol, atol


def assert_sums(sums, exp, what):
    cnt, lo, hi, gain, act, gtol, atol = exp
    s = sums.cpu().numpy().astype(np.float64)
    assert s.shape == cnt.shape + (4,), (what, s.shape)
    assert np.array_equal(s[..., 0], cnt), f"{what}: included counts"
    assert ((s[..., 1] >= lo) & (s[..., 1] <= hi)).all(), f"{what}: flip counts"
    assert (np.abs(s[..., 2] - gain) <= gtol + 1e-12).all(), f"{what}: gain sums, max error {np.abs(s[..., 2] - gain).max():.3e}"
    assert (np.abs(s[..., 3] - act) <= atol + 1e-12).all(), f"{what}: |masked| sums, max error {np.abs(s[..., 3] - act).max():.3e}"


def table(rows_by_mask, M):
    return np.array([[[r[k] for k in M.METRIC_FIELDS] for r in rows_by_mask[name]] for name in M.MASKS])


def assert_metrics(ours, gold_metrics):
    np.testing.assert_allclose(ours[..., 0], gold_metrics[..., 0], rtol=0, atol=1e-6, err_msg="class_flip")
    np.testing.assert_allclose(ours[..., 1:], gold_metrics[..., 1:], rtol=1e-4, atol=1e-6, err_msg="prediction_gain / avg_actionability")


CFG = {"batch_size": 64, "cuda": DEV}


# ---- 1. the reference's own metrics --------------------------------------------------------------------------------------------
def test_four_mask_metrics_follow_reference(M, gold, data, shipped):
    G, C, _, _ = shipped
    assert list(M.MASKS) == [str(n) for n in gold["mask_names"]]
    res = M.counterfactual_sweep(G, C, data["X_test"], data["y_test"], M.MASKS, 64)
    s = res["sums"].cpu().numpy()
    assert s.shape == (4, 3, 4, 4)
    assert np.array_equal(s[..., 0], gold["counts"]) and np.array_equal(s[..., 1], gold["flips"])
    ours = table(M.compute_metrics_per_target(G, C, data["X_test"], data["y_test"], CFG, mask=M.MASKS), M)
    print("metrics, max |ours - reference|:", np.abs(ours - gold["metrics"]).max(axis=(0, 1)))
    assert_metrics(ours, gold["metrics"])
    for i, name in enumerate(M.MASKS):                                       # one mask at a time: a list of rows, the same numbers
        rows = M.compute_metrics_per_target(G, C, data["X_test"], data["y_test"], CFG, mask=name)
        assert [r["target_class"] for r in rows] == [0, 1, 2]
        assert np.array_equal(np.array([[r[k] for k in M.METRIC_FIELDS] for r in rows]), ours[i])
    np.testing.assert_allclose(M.metrics_from_sums(s), ours, rtol=0, atol=0)


# ---- 2. the `none` mask ----------------------------------------------------------------------------------------------------------
def test_none_mask_moves_nothing(M, data, shipped):
    G, C, _, _ = shipped
    x = torch.tensor(data["X_test"], dtype=torch.float32, device=DEV)
    res = M.counterfactual_sweep(G, C, x, data["y_test"], {"none": "none"}, 64, outputs=("x_cf", "gain", "masked_residual"))
    for t in range(3):
        assert torch.equal(res["x_cf"][0, t].view(torch.int32), x.view(torch.int32))
    assert torch.all(res["gain"] == 0.0).item() and torch.all(res["masked_residual"] == 0.0).item()
    assert torch.all(res["sums"][..., 2:] == 0.0).item()
    for r in M.compute_metrics_per_target(G, C, data["X_test"], data["y_test"], CFG, mask="none"):
        assert r["prediction_gain"] == 0.0 and r["avg_actionability"] == 0.0
    out = M.counterfactuals(G, C, x, 1, "none")
    assert torch.equal(out["x_cf"].view(torch.int32), x.view(torch.int32)) and torch.all(out["gain"] == 0.0).item()


# ---- 3. per-row outputs against float64 ----------------------------------------------------------------------------------------
def test_rows_vs_float64_shipped_nets(M, data, shipped):
    G, C, oG, oC = shipped
    x = data["X_test"].astype(np.float32)
    t, mk = queries(len(x), 11)
    ours = M.counterfactuals(G, C, x, t, mk)
    assert set(ours) == set(OUTS) and ours["pred_cf"].dtype == torch.int64
    assert_rows(ours, oracle(oG, oC, x, t, mk), "hidden 32", max_skipped=0.0)


def test_rows_vs_float64_hidden_64(M, data, wide):
    G, C, oG, oC = wide
    x = data["X_test"].astype(np.float32)
    t, mk = queries(len(x), 12)
    ref = oracle(oG, oC, x, t, mk)
    assert np.abs(ref["raw_residual"]).max() > 0.05, "the seeded generator must move the points"
    ours = M.counterfactuals(G, C, torch.from_numpy(x).to(DEV), torch.from_numpy(t), torch.from_numpy(mk).to(DEV))
    assert_rows(ours, ref, "hidden 64", max_skipped=0.01)


# ---- 4. consistency ------------------------------------------------------------------------------------------------------------
def test_forms_agree_and_nothing_is_written(M, data, shipped, wide):
    for G, C, _, _ in (shipped, wide):
        before = [{k: v.clone() for k, v in net.state_dict().items()} for net in (G, C)]
        x = torch.tensor(data["X_test"], dtype=torch.float32, device=DEV)
        N = x.shape[0]
        runs = [M.counterfactual_sweep(G, C, x, data["y_test"], M.MASKS, 64, outputs=OUTS) for _ in range(2)]
        for k in runs[0]:                                                    # two runs: bitwise, the sums included
            assert torch.equal(runs[0][k], runs[1][k]), k
        sw = runs[0]
        for m, (name, mv) in enumerate(M.MASKS.items()):
            for t in range(3):
                per = M.counterfactuals(G, C, x, t, name if t else mv)
                for k in OUTS:
                    want = sw[k] if k in ("logits_x", "pred_x") else sw[k][m, t]
                    assert torch.equal(per[k], want), (name, t, k)
                # the module forwards, eval mode
                oh = F.one_hot(torch.full((N,), t, device=DEV), 3).float()
                mk = torch.from_numpy(mv).to(DEV).expand(N, 2).contiguous()
                raw, masked = G(x, oh, mk)
                for k, ref in (("raw_residual", raw), ("masked_residual", masked), ("logits_cf", C((x + masked).contiguous())),
                               ("logits_x", C(x))):
                    ref = ref.cpu().numpy().astype(np.float64)
                    assert (np.abs(per[k].cpu().numpy() - ref) <= row_tol(ref)).all(), (name, t, k)
        for net, sd in zip((G, C), before):
            for k, v in net.state_dict().items():
                assert torch.equal(v, sd[k]), k


# ---- 5. shapes -----------------------------------------------------------------------------------------------------------------
SHAPES = [(N, g) for N in (1, 63, 64, 65, 240) for g in (1, 64, 512)] + [(1200, 600)]


@pytest.mark.parametrize("N,group", SHAPES)
def test_group_sums_vs_float64(M, shipped, all_rows, sweep_oracle, N, group):
    G, C, _, _ = shipped
    X, y = all_rows
    res = M.counterfactual_sweep(G, C, X[:N], y[:N], M.MASKS, group, outputs=("gain", "pred_cf"))
    assert_sums(res["sums"], expected_sums(sweep_oracle, y, N, group), f"N {N} group {group}")
    assert res["gain"].shape == (4, 3, N) and res["pred_cf"].shape == (4, 3, N)


def test_empty_groups_and_one_class(M, shipped, all_rows, sweep_oracle):
    G, C, _, _ = shipped
    X, y = all_rows
    N, group = 130, 64                                                       # groups of 64, 64 and a tail of two rows
    y1 = y[:N].copy()
    y1[:64] = 1                                                              # group 0 holds no row for target 1
    res = M.counterfactual_sweep(G, C, X[:N], y1, M.MASKS, group)
    exp = expected_sums(sweep_oracle, y1, N, group)
    assert (exp[0][:, 1, 0] == 0).all() and (exp[0][:, 1, 1:] > 0).all()
    assert_sums(res["sums"], exp, "empty group")
    s = res["sums"].cpu().numpy().astype(np.float64)
    assert (s[:, 1, 0] == 0.0).all()
    want = np.mean(s[:, 1, 1:, 1] / s[:, 1, 1:, 0], axis=-1)                 # the mean over the two groups that have rows
    got = table(M.compute_metrics_per_target(G, C, X[:N], y1, dict(CFG, batch_size=group), mask=M.MASKS), M)
    np.testing.assert_allclose(got[:, 1, 0], want, rtol=0, atol=1e-12)
    y2 = np.full(N, 2, np.int64)                                             # one class: nothing to flip to class 2
    rows = M.compute_metrics_per_target(G, C, X[:N], y2, dict(CFG, batch_size=group), mask="both")
    assert all(math.isnan(rows[2][k]) for k in M.METRIC_FIELDS) and rows[2]["target_class"] == 2
    assert all(np.isfinite(rows[t][k]) for t in (0, 1) for k in M.METRIC_FIELDS)
    assert_sums(M.counterfactual_sweep(G, C, X[:N], None, M.MASKS, group)["sums"], expected_sums(sweep_oracle, None, N, group), "y = None")


# ---- 6. the decision grid ------------------------------------------------------------------------------------------------------
def test_decision_grid_follows_reference(M, gold, data, shipped):
    _, C, _, _ = shipped
    xx, yy, Z = M.decision_regions(C, data["X_test"])
    assert xx.shape == yy.shape == Z.shape == (200, 200)
    sure = gold["grid_margin"] >= MARGIN
    assert int((~sure).sum()) <= 1
    assert np.array_equal(Z[sure], gold["grid_Z"][sure].astype(np.int64))
    X = data["X_test"]
    assert xx[0, 0] == X[:, 0].min() - 0.1 and yy[-1, 0] == X[:, 1].max() + 0.1


# ---- 7. evaluate_classifier, evaluate_pipeline ---------------------------------------------------------------------------------
def test_evaluate_classifier_and_pipeline_files(M, gold, data, shipped, tmp_path, capsys):
    G, C, _, _ = shipped
    cfg = dict(CFG, out_dir=str(tmp_path / "results"))
    acc, cm = M.evaluate_classifier(C, data["X_test"], data["y_test"], cfg)
    assert acc == 239 / 240 == float(gold["accuracy"])
    assert np.array_equal(cm, gold["confusion"])
    path = os.path.join(cfg["out_dir"], "classifier_confusion.csv")
    assert open(path).read() == str(gold["confusion_csv"])
    assert f"Classifier accuracy: {acc:.4f}, confusion matrix saved to {path}" in capsys.readouterr().out
    assert M.evaluate_pipeline(G, C, data["X_test"], data["y_test"], dict(cfg, out_dir=str(tmp_path / "plain"))) is None
    assert sorted(os.listdir(tmp_path / "plain")) == ["classifier_confusion.csv", "decision_boundaries_no_cfs.npz"]
    grid = np.load(tmp_path / "plain" / "decision_boundaries_no_cfs.npz")
    sure = gold["grid_margin"] >= MARGIN
    assert np.array_equal(grid["Z"][sure], gold["grid_Z"][sure])
    metrics = M.evaluate_pipeline(G, C, data["X_test"], data["y_test"], cfg, masks=M.MASKS)
    assert_metrics(table(metrics, M), gold["metrics"])
    head = ["target_class", "class_flip", "prediction_gain", "avg_actionability"]
    for i, name in enumerate(M.MASKS):
        rows = list(csv.reader(open(os.path.join(cfg["out_dir"], f"mask_{name}", "metrics.csv"))))
        assert rows[0] == head and [r[0] for r in rows[1:]] == ["0", "1", "2"]
        assert_metrics(np.array([[float(v) for v in r[1:]] for r in rows[1:]]), gold["metrics"][i])
    rows = list(csv.reader(open(os.path.join(cfg["out_dir"], "metrics_all_masks.csv"))))
    assert rows[0] == head + ["mask"] and [r[-1] for r in rows[1:]] == [n for n in M.MASKS for _ in range(3)]
    assert_metrics(np.array([[float(v) for v in r[1:4]] for r in rows[1:]]).reshape(4, 3, 3), gold["metrics"])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(M, data, shipped):
    G, C, _, _ = shipped
    x = torch.tensor(data["X_test"][:8], dtype=torch.float32, device=DEV)
    with pytest.raises(M.PcgError, match="hidden_dim"):
        M.counterfactuals(frozen(M.ResidualGenerator(2, 48, 3)), C, x, 0, "both")
    for bad in (3, -1, torch.tensor([0, 1, 2, 3, 0, 1, 2, 0]), np.array([0, 1, 2, -1, 0, 1, 2, 0])):
        with pytest.raises(M.PcgError, match="targets"):
            M.counterfactuals(G, C, x, bad, "both")
    for bad in (np.ones(3, np.float32), np.ones((7, 2), np.float32), np.ones((8, 3), np.float32), "z_only"):
        with pytest.raises(M.PcgError, match="mask"):
            M.counterfactuals(G, C, x, 0, bad)
    with pytest.raises(M.PcgError, match="mask"):
        M.counterfactual_sweep(G, C, x, None, [np.ones((8, 2), np.float32)], 64)
    for empty in (x[:0], np.zeros((0, 2), np.float32)):
        with pytest.raises(M.PcgError, match="N >= 1"):
            M.counterfactuals(G, C, empty, 0, "both")
    with pytest.raises(M.PcgError, match="mask is required"):
        M.counterfactuals(G, C, x, 0, None)
    with pytest.raises(M.PcgError, match="mask is required"):
        M.compute_metrics_per_target(G, C, data["X_test"], data["y_test"], CFG, mask=None)
    with pytest.raises(M.PcgError, match="no CPU path"):
        M.counterfactuals(G, C, x.cpu(), 0, "both")
    with pytest.raises(M.PcgError, match="batch_size"):
        M.counterfactual_sweep(G, C, x, None, M.MASKS, 0)
    G2 = M.ResidualGenerator(2, 32, 3).to(DEV).eval()                         # parameters that require grad, grad mode on
    with pytest.raises(M.PcgError, match="autograd"):
        M.counterfactuals(G2, C, x, 0, "both")
    with torch.no_grad():
        assert M.counterfactuals(G2, C, x, 0, "both")["x_cf"].shape == (8, 2)
