"""CPU: the host side of the moons CounteRGAN's evaluation (pcgan_amd.moons_countergan): the reduction of the kernel's group sums on
the reference's recorded per-batch numbers (tests/golden/moons_cf_eval_ref.npz), the CSV writers, the MASKS table and the argument
checks that need no device.  No GPU call is made here."""
import csv
import math
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "moons_cf_eval_ref.npz")))


@pytest.fixture(scope="module")
def M():
    from pcgan_amd import moons_countergan
    return moons_countergan


def sums_from_batches(gold):
    """The kernel's sums layout [M][T][groups][4] from the reference's per-batch count, flips and means."""
    c = gold["counts"].astype(np.float64)
    return np.stack([c, gold["flips"].astype(np.float64), gold["batch_means"][..., 1] * c, gold["batch_means"][..., 2] * 2 * c], -1)


def test_masks_table(M, gold):
    assert list(M.MASKS) == ["both", "none", "x_only", "y_only"] == [str(n) for n in gold["mask_names"]]
    want = {"both": [1, 1], "none": [0, 0], "x_only": [1, 0], "y_only": [0, 1]}
    for i, (name, v) in enumerate(M.MASKS.items()):
        assert v.dtype == np.float32 and v.tolist() == want[name] == gold["masks"][i].tolist()


def test_reduction_reproduces_reference_tables(M, gold):
    s = sums_from_batches(gold)
    np.testing.assert_allclose(gold["batch_means"][..., 0], s[..., 1] / s[..., 0], rtol=0, atol=1e-6)   # fp32-rounded batch means
    table = M.metrics_from_sums(s)
    assert table.shape == (4, 3, 3)
    np.testing.assert_allclose(table[..., 0], gold["metrics"][..., 0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(table[..., 1:], gold["metrics"][..., 1:], rtol=1e-12, atol=1e-15)
    rows = M.metric_rows(table[0])
    assert [r["target_class"] for r in rows] == [0, 1, 2] and list(rows[0]) == ["target_class"] + list(M.METRIC_FIELDS)
    assert all(type(r[k]) is float for r in rows for k in M.METRIC_FIELDS)


def test_reduction_is_the_mean_of_batch_means_and_skips_empty_groups(M):
    # two groups, 3 rows and 1 row: rows do not weigh equally; a third group without rows is left out
    s = np.array([[3, 3, 0.6, 1.2], [1, 0, 0.1, 0.8], [0, 0, 0.0, 0.0]], np.float32)
    flip, gain, act = M.metrics_from_sums(s)
    assert flip == pytest.approx(np.mean([1.0, 0.0])) and flip != pytest.approx(3 / 4)
    assert gain == pytest.approx(np.mean([np.float32(0.6) / 3, np.float32(0.1)]))
    assert act == pytest.approx(np.mean([np.float32(1.2) / 6, np.float32(0.8) / 2]))
    np.testing.assert_array_equal(M.metrics_from_sums(s[:2]), M.metrics_from_sums(s))
    empty = M.metrics_from_sums(np.zeros((2, 3, 4, 4), np.float32))                 # no group has a row: nan, as the reference
    assert empty.shape == (2, 3, 3) and np.isnan(empty).all()
    rows = M.metric_rows(empty[0])
    assert all(math.isnan(r[k]) for r in rows for k in M.METRIC_FIELDS)


def test_confusion_matrix_and_csv_text(M, gold):
    cm = gold["confusion"]
    assert M.confusion_csv(cm) == str(gold["confusion_csv"])
    y = np.repeat(np.arange(3), cm.sum(1))
    pred = np.concatenate([np.repeat(np.arange(3), row) for row in cm])
    assert np.array_equal(M.confusion_matrix(y, pred), cm)
    # sklearn's label rule: the sorted values that occur in either vector
    assert np.array_equal(M.confusion_matrix([0, 0, 2], [0, 2, 2]), [[1, 1], [0, 1]])
    assert np.array_equal(M.confusion_matrix([1, 1], [0, 1]), [[0, 0], [1, 1]])


def test_save_metrics_writes_reference_columns(M, gold, tmp_path, capsys):
    rows = M.metric_rows(gold["metrics"][0])
    path = str(tmp_path / "mask_both" / "metrics.csv")
    M.save_metrics(rows, path)
    assert capsys.readouterr().out == f"Saved metrics to {path}\n"
    got = list(csv.reader(open(path)))
    assert got[0] == ["target_class", "class_flip", "prediction_gain", "avg_actionability"]
    assert [int(r[0]) for r in got[1:]] == [0, 1, 2]
    assert np.array_equal(np.array([[float(v) for v in r[1:]] for r in got[1:]]), gold["metrics"][0])      # repr round-trips
    nan_rows = M.metric_rows(np.full((3, 3), np.nan))
    M.save_metrics([dict(r, mask="both") for r in nan_rows], path, ("target_class",) + M.METRIC_FIELDS + ("mask",))
    assert open(path).read().splitlines()[1] == "0,,,,both"                                               # pandas writes nan as empty


def test_argument_checks_need_no_device(M):
    G, C = M.ResidualGenerator(2, 32, 3), M.NNClassifier(2)
    x = np.zeros((5, 2), np.float32)
    with pytest.raises(M.PcgError, match="hidden_dim"):
        M.counterfactuals(M.ResidualGenerator(2, 48, 3), C, x, 0, "both")
    with pytest.raises(M.PcgError, match="hidden width"):
        M.counterfactuals(G, M.NNClassifier(2, hidden_dim=16), x, 0, "both")
    for bad in (3, -1, [0, 1, 2, 3, 0], torch.tensor([0, -1, 0, 0, 0])):
        with pytest.raises(M.PcgError, match="targets must lie"):
            M.counterfactuals(G, C, x, bad, "both")
    for bad in ([0, 1], np.zeros(5), torch.zeros(5, 2, dtype=torch.long)[:, 0].float()):
        with pytest.raises(M.PcgError, match="target must be"):
            M.counterfactuals(G, C, x, bad, "both")
    for bad in (np.ones(3), np.ones((4, 2)), np.ones((5, 3)), "diagonal", np.ones((1, 5, 2))):
        with pytest.raises(M.PcgError, match="mask"):
            M.counterfactuals(G, C, x, 0, bad)
    for bad in (None, ):
        with pytest.raises(M.PcgError, match="mask is required"):
            M.counterfactuals(G, C, x, 0, bad)
        with pytest.raises(M.PcgError, match="mask is required"):
            M.compute_metrics_per_target(G, C, x, np.zeros(5, np.int64), {"batch_size": 64}, mask=bad)
    for bad in (np.zeros((0, 2), np.float32), np.zeros((5, 3), np.float32), np.zeros(5, np.float32), torch.zeros(0, 2)):
        with pytest.raises(M.PcgError, match=r"must be \[N\]\[2\] with N >= 1"):
            M.counterfactuals(G, C, bad, 0, "both")
    with pytest.raises(M.PcgError, match="batch_size"):
        M.counterfactual_sweep(G, C, x, None, M.MASKS, 0)
    with pytest.raises(M.PcgError, match="outputs"):
        M.counterfactual_sweep(G, C, x, None, M.MASKS, 64, outputs=("x_cf", "jacobian"))
    with pytest.raises(M.PcgError, match="y must be"):
        M.counterfactual_sweep(G, C, x, np.zeros(4, np.int64), M.MASKS, 64)
    with pytest.raises(M.PcgError, match="no mask"):
        M.counterfactual_sweep(G, C, x, None, {}, 64)
    # everything valid: the nets are on the CPU, and there is no CPU path
    with pytest.raises(M.PcgError, match="no CPU path"):
        M.counterfactuals(G, C, x, 0, "both")
    with pytest.raises(M.PcgError, match="no CPU path"):
        M.decision_regions(C, x, n=4)
