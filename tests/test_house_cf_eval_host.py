"""CPU: the host side of the tabular CounteRGAN's one-launch evaluation (pcgan_amd.house) — the prompt mask, the
fold of the tile sums into the reference's metrics, the feature-shift table, the weighted classifier scores, and every guard,
which must raise PcgError before anything touches a GPU."""
import numpy as np
import pytest
import torch

import pcgan_amd
from pcgan_amd import house as H

PcgError = pcgan_amd.PcgError
IMM = [11, 12, 13, 14]                       # yr_built, yr_renovated, lat, long


def nets():
    G = H.ResidualGenerator(17, 32, 4, H.CONFIG["continuous_idx"], H.CONFIG["categorical_info"], tau=0.5)
    return G.eval(), H.NNClassifier(17, 4).eval()


# ---- prompt_mask (gradio_app.py:150-155) -------------------------------------------------------------------------------------------
def test_prompt_mask_none_allows_everything_but_the_immutable_columns():
    m = H.prompt_mask(H.CONFIG)
    assert m.dtype == np.float32 and m.shape == (17,)
    want = np.ones(17, np.float32)
    want[IMM] = 0
    np.testing.assert_array_equal(m, want)


def test_prompt_mask_names_and_indices():
    m = H.prompt_mask(H.CONFIG, ["sqft_living", 8, "bathrooms"])
    assert sorted(np.nonzero(m)[0]) == [1, 2, 8]
    assert H.prompt_mask(H.CONFIG, "grade").nonzero()[0].tolist() == [8]
    assert H.prompt_mask(H.CONFIG, []).sum() == 0


def test_prompt_mask_immutable_wins_over_the_prompt():
    m = H.prompt_mask(H.CONFIG, ["lat", "grade", 11])
    assert m.nonzero()[0].tolist() == [8]
    assert H.prompt_mask({"immutable_idx": []}, ["lat"]).nonzero()[0].tolist() == [13]


def test_prompt_mask_other_feature_names():
    m = H.prompt_mask({"immutable_idx": [0]}, ["b", "a"], feature_names=["a", "b", "c"])
    np.testing.assert_array_equal(m, [0, 1, 0])


@pytest.mark.parametrize("bad", [["garage"], [17], [-1], [1.5], [True]])
def test_prompt_mask_refuses_unknown_features(bad):
    with pytest.raises(PcgError):
        H.prompt_mask(H.CONFIG, bad)


# ---- metrics_from_sums -------------------------------------------------------------------------------------------------------------
def test_metrics_from_sums_against_numpy():
    rs = np.random.RandomState(3)
    group, n_groups = 40, 3                                  # 3 tiles per group
    cnt = rs.randint(0, 17, (4, n_groups * 3)).astype(np.float64)
    cnt[1] = 0                                               # target 1: no row at all -> nan
    cnt[2, 3:6] = 0                                          # target 2: its middle group is empty -> left out of the mean
    sums = np.stack([cnt, np.floor(cnt * rs.rand(*cnt.shape)), cnt * rs.randn(*cnt.shape) * 0.1, cnt * rs.rand(*cnt.shape) * 3], -1)
    got = H.metrics_from_sums(sums.astype(np.float32), group)
    assert got.shape == (4, 3)
    s32 = sums.astype(np.float32).astype(np.float64)
    for t in range(4):
        per_group = []
        for g in range(n_groups):
            c, f, ga, ab = s32[t, 3 * g:3 * g + 3].sum(0)
            if c > 0:
                per_group.append((f / c, ga / c, ab / (17 * c)))
        if per_group:
            np.testing.assert_allclose(got[t], np.mean(per_group, 0), rtol=1e-12)
        else:
            assert np.isnan(got[t]).all()
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3]]).any()


def test_metrics_from_sums_one_short_group_and_bad_shapes():
    sums = np.array([[[16, 8, 1.6, 17 * 1.6], [3, 0, 0.3, 1.0]]])            # 19 rows, group 128: the rows fill no whole group
    np.testing.assert_allclose(H.metrics_from_sums(sums, 128), [[8 / 19, 1.9 / 19, (17 * 1.6 + 1.0) / (17 * 19)]], rtol=1e-12)
    np.testing.assert_allclose(H.metrics_from_sums(np.concatenate([sums, sums], 1), 19)[0, 0], 8 / 19)   # two groups of 19 rows
    with pytest.raises(PcgError):
        H.metrics_from_sums(np.zeros((4, 5, 4)), 19)         # 5 tiles are no whole number of 2-tile groups
    with pytest.raises(PcgError):
        H.metrics_from_sums(np.zeros((4, 4, 3)), 19)


# ---- analyze_feature_shift_importance (eval_utils.py:292-324) -----------------------------------------------------------------------
def test_feature_shift_importance_rows_and_order():
    X = np.zeros((4, 3))
    Xc = np.array([[0.1, -0.4, 0.0], [0.3, 0.4, 0.0], [-0.1, 0.0, 0.0], [0.1, 0.0, 0.0]])
    rows = H.analyze_feature_shift_importance(X, Xc, ["a", "b", "c"])
    assert [r["feature"] for r in rows] == ["b", "a", "c"]
    np.testing.assert_allclose([r["mean_abs_change_norm"] for r in rows], [0.2, 0.15, 0.0])
    np.testing.assert_allclose([r["mean_pct_of_range"] for r in rows], [20.0, 15.0, 0.0])
    assert "mean_abs_change_denorm" not in rows[0]

    class S:
        data_min_, data_max_ = np.array([0.0, 10.0, 5.0]), np.array([2.0, 110.0, 6.0])
    rows = H.analyze_feature_shift_importance(X, Xc, ["a", "b", "c"], scaler=S())
    np.testing.assert_allclose([r["mean_abs_change_denorm"] for r in rows], [0.2 * 100, 0.15 * 2, 0.0])
    ties = H.analyze_feature_shift_importance(np.zeros((1, 3)), np.array([[0.5, 0.7, 0.5]]), ["a", "b", "c"])
    assert [r["feature"] for r in ties] == ["b", "a", "c"]  # ties keep the feature order
    empty = H.analyze_feature_shift_importance(np.empty((0, 3)), np.empty((0, 3)), ["a", "b", "c"])
    assert empty == [{"feature": f, "mean_abs_change_norm": 0.0} for f in "abc"]
    with pytest.raises(PcgError):
        H.analyze_feature_shift_importance(np.zeros((2, 3)), np.zeros((3, 3)), ["a", "b", "c"])


# ---- evaluate_classifier's scores ---------------------------------------------------------------------------------------------------
def test_weighted_scores_hand_checked():
    # true 0: 5 right, 1 as class 1; true 1: 2 as class 0, 2 right; true 2: 3 rows, never predicted right and class 2 never predicted
    cm = np.array([[5, 1, 0], [2, 2, 0], [1, 2, 0]])
    s = H.weighted_scores(cm)
    p = [5 / 8, 2 / 5, 0.0]                                  # column sums 8, 5, 0 (zero_division=0)
    r = [5 / 6, 2 / 4, 0.0]
    f = [2 * p[0] * r[0] / (p[0] + r[0]), 2 * p[1] * r[1] / (p[1] + r[1]), 0.0]
    w = np.array([6, 4, 3]) / 13
    assert s["accuracy"] == pytest.approx(7 / 13)
    assert s["precision"] == pytest.approx(float(w @ p))
    assert s["recall"] == pytest.approx(float(w @ r)) and s["recall"] == pytest.approx(s["accuracy"])
    assert s["f1"] == pytest.approx(float(w @ f))
    np.testing.assert_array_equal(s["per_class"]["support"], [6, 4, 3])
    with pytest.raises(PcgError):
        H.weighted_scores(np.zeros((2, 2)))


def test_confusion_matrix_labels_are_the_values_that_occur():
    cm = H.confusion_matrix([0, 0, 2, 2, 3], [0, 2, 2, 3, 3])
    np.testing.assert_array_equal(cm, [[1, 1, 0], [0, 1, 1], [0, 0, 1]])


# ---- guards: PcgError on the host, no GPU needed -------------------------------------------------------------------------------------
X3 = np.full((3, 17), 0.5, np.float32)


def test_guard_training_mode():
    G, C = nets()
    with pytest.raises(PcgError, match="eval"):
        H.counterfactuals(G.train(), C, X3, 1, H.CONFIG)
    G, C = nets()
    with pytest.raises(PcgError, match="eval"):
        H.counterfactual_sweep(G, C.train(), X3, None, H.CONFIG)


@pytest.mark.parametrize("target", [4, -1, np.array([0, 1, 4]), np.array([0, 1]), np.array([0.0, 1.0, 2.0]), torch.tensor([True, False, True])])
def test_guard_targets(target):
    G, C = nets()
    with pytest.raises(PcgError, match="target"):
        H.counterfactuals(G, C, X3, target, H.CONFIG)


@pytest.mark.parametrize("mask", [np.ones(16), np.ones((2, 17)), np.ones((3, 17, 1))])
def test_guard_mask_shapes(mask):
    G, C = nets()
    with pytest.raises(PcgError, match="mask"):
        H.counterfactuals(G, C, X3, 1, H.CONFIG, mask=mask)
    with pytest.raises(PcgError, match="mask"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG, mask=mask)


def test_guard_noise_and_row_shapes():
    G, C = nets()
    with pytest.raises(PcgError, match="gumbel"):
        H.counterfactuals(G, C, X3, 1, H.CONFIG, gumbel=torch.zeros(3, 69))
    with pytest.raises(PcgError, match="gumbel"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG, gumbel=torch.zeros(3, 3, 70))
    with pytest.raises(PcgError, match=r"\[N\]\[17\]"):
        H.counterfactuals(G, C, np.zeros((3, 16), np.float32), 1, H.CONFIG)
    with pytest.raises(PcgError, match="outputs"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG, outputs=("x_cf", "nope"))
    with pytest.raises(PcgError, match="y must"):
        H.counterfactual_sweep(G, C, X3, np.zeros(2, np.int64), H.CONFIG)
    with pytest.raises(PcgError, match="y is required"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG, class_sums=True)
    with pytest.raises(PcgError, match="batch_size"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG, batch_size=0)


def test_guard_unsupported_configurations():
    C = H.NNClassifier(17, 4).eval()
    G = H.ResidualGenerator(17, 64, 4, H.CONFIG["continuous_idx"], H.CONFIG["categorical_info"]).eval()
    with pytest.raises(PcgError, match="built for"):
        H.counterfactuals(G, C, X3, 1, H.CONFIG)
    G = H.ResidualGenerator(17, 32, 4, H.CONFIG["continuous_idx"], H.CONFIG["categorical_info"], n_blocks=3).eval()
    with pytest.raises(PcgError, match="built for"):
        H.counterfactual_sweep(G, C, X3, None, H.CONFIG)
    G, _ = nets()
    with pytest.raises(PcgError, match="classifier widths"):
        H.counterfactuals(G, H.NNClassifier(17, 3).eval(), X3, 1, H.CONFIG)


def test_guards_of_the_one_launch_metrics_and_no_cpu_path():
    G, C = nets()
    y = np.array([0, 1, 2])                                  # three classes for a four-class generator
    with pytest.raises(PcgError, match="classes"):
        H.compute_metrics_per_target(G, C, X3, y, H.CONFIG, one_launch=True)
    # the nets are on the CPU: refused before any launch, with or without a GPU in the machine
    with pytest.raises(PcgError, match="no CPU path"):
        H.counterfactuals(G, C, X3, 1, H.CONFIG)
    with pytest.raises(PcgError, match="no CPU path"):
        H.compute_metrics_per_target(G, C, np.tile(X3, (2, 1))[:4], np.arange(4), H.CONFIG, one_launch=True)
    with pytest.raises(PcgError, match="no CPU path"):
        H.analyze_class_pair_sensitivity(G, C, np.tile(X3, (2, 1))[:4], np.arange(4), H.CONFIG)
    with pytest.raises(PcgError, match="no CPU path"):
        H.evaluate_classifier(C, X3, [0, 1, 2])


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """pcg_house_cf_eval's own checks (PCG_ERR_INVALID and a pcg_last_error text): they return before the launch, so no GPU is needed."""
    import ctypes
    from pcgan_amd import _lib
    lib = pcgan_amd.load()

    def call(d, a):
        rc = lib.pcg_house_cf_eval(ctypes.byref(d) if d is not None else None, ctypes.byref(a) if a is not None else None, None)
        return rc, lib.pcg_last_error().decode()

    assert lib.pcg_abi_struct_bytes(b"pcg_house_cf_eval_args") == ctypes.sizeof(_lib.HouseCfEvalArgs)
    rc, msg = call(None, None)
    assert rc != 0 and "null descriptor" in msg
    d, a = _lib.HouseGDesc(), _lib.HouseCfEvalArgs()
    d.D, d.NC, d.hidden, d.nblocks = 17, 4, 64, 5
    rc, msg = call(d, a)
    assert rc != 0 and "hidden 32" in msg
    d.hidden, d.nheads, d.ncont = 32, 7, 9                      # 16 columns for 17 features
    rc, msg = call(d, a)
    assert rc != 0 and "must cover" in msg
    d.ncont = 10
    for s_, v in enumerate([0, 9, 39, 45, 47, 52, 57, 120]):   # 120 packed categories
        d.seg[s_] = v
    rc, msg = call(d, a)
    assert rc != 0 and "packed categories" in msg
    d.seg[7] = 70
    a.N, a.group, a.T = 5, 2, 5
    rc, msg = call(d, a)
    assert rc != 0 and "T 5" in msg
    a.T = 1
    rc, msg = call(d, a)
    assert rc != 0 and "null generator" in msg
