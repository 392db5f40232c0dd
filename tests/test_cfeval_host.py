"""CPU: the host code the counterfactual-evaluation front ends share (pcgan_amd._cfeval, _epoch.one_gpu, nn.FrozenClassifier): one
definition of each piece, the fold of the group sums bit for bit against the reference's three expressions, every refusal of the
argument guards under both settings of the keywords that carry the ports' differences, and the CSV text.  No GPU call, no library."""
import types

import numpy as np
import pytest
import torch

from pcgan_amd import PcgError, _cfeval, _epoch, countergan, house, moons_countergan
from pcgan_amd import nn as pnn


# ---- one definition each ---------------------------------------------------------------------------------------------------------------
def test_shared_pieces_have_one_definition():
    assert house.confusion_matrix is moons_countergan.confusion_matrix is _cfeval.confusion_matrix
    assert house.metric_rows is moons_countergan.metric_rows is _cfeval.metric_rows
    assert house.METRIC_FIELDS is moons_countergan.METRIC_FIELDS is _cfeval.METRIC_FIELDS
    assert moons_countergan.confusion_csv is countergan.confusion_csv is _cfeval.confusion_csv
    assert house.save_table is _cfeval.save_table
    assert house.upload is moons_countergan.upload is _cfeval.upload
    assert _cfeval.one_gpu is _epoch.one_gpu
    for mod in (house, moons_countergan):
        for gone in ("_rows_arg", "_cf_rows", "_eval_device", "_cf_device", "_upload", "_csv_value"):
            assert not hasattr(mod, gone), (mod.__name__, gone)
    for mod in (house, countergan):
        assert not hasattr(mod, "_CFn") and not hasattr(mod, "_CTrainFn")
    assert issubclass(house.NNClassifier, pnn.FrozenClassifier) and issubclass(countergan.CNNClassifier, pnn.FrozenClassifier)
    for cls in (house.NNClassifier, countergan.CNNClassifier):
        assert cls.forward is pnn.FrozenClassifier.forward and cls.train is pnn.FrozenClassifier.train
    assert not issubclass(moons_countergan.NNClassifier, pnn.FrozenClassifier)      # a different design: it stays out


# ---- batch_mean_metrics ----------------------------------------------------------------------------------------------------------------
def restated(s, D):
    """The reference's expressions, one [n_groups][4] block at a time."""
    s = np.asarray(s, dtype=np.float64)
    out = np.full(s.shape[:-2] + (3,), np.nan)
    for idx in np.ndindex(*s.shape[:-2]):
        g = s[idx][s[idx][:, 0] > 0]
        if len(g):
            out[idx] = (np.mean(g[:, 1] / g[:, 0]), np.mean(g[:, 2] / g[:, 0]), np.mean(g[:, 3] / (D * g[:, 0])))
    return out


def group_sums(lead, n_groups=5, dtype=np.float64, seed=0):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 20, size=lead + (n_groups,)).astype(np.float64)
    cnt[..., 1] = 0                                                            # a group with no included row
    s = np.stack([cnt, np.floor(cnt * rs.rand(*cnt.shape)), cnt * rs.randn(*cnt.shape) * 0.1, cnt * rs.rand(*cnt.shape) * 3], -1)
    return s.astype(dtype)


@pytest.mark.parametrize("D", [2, 17])
@pytest.mark.parametrize("lead", [(), (3,), (2, 3)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_mean_metrics_bit_for_bit(D, lead, dtype):
    s = group_sums(lead, dtype=dtype)
    if lead:
        s[(0,) * len(lead)][:, 0] = 0                                          # a target with no live group
    got = _cfeval.batch_mean_metrics(s, D)
    assert got.dtype == np.float64 and got.shape == lead + (3,)
    assert np.array_equal(got, restated(s, D), equal_nan=True)
    if lead:
        assert np.isnan(got[(0,) * len(lead)]).all() and not np.isnan(got[(-1,) * len(lead)]).any()
    else:
        g = s.astype(np.float64)[[0, 2, 3, 4]]                                  # (the empty group left out by hand)
        assert np.array_equal(got, [np.mean(g[:, 1] / g[:, 0]), np.mean(g[:, 2] / g[:, 0]), np.mean(g[:, 3] / (D * g[:, 0]))])
    assert np.isnan(_cfeval.batch_mean_metrics(np.zeros(lead + (4, 4), dtype), D)).all()


def test_front_ends_fold_through_batch_mean_metrics():
    # 37 rows in groups of 16: groups of 16, 16 and 5 rows
    cnt = np.array([16.0, 16.0, 5.0])
    rs = np.random.RandomState(1)
    s = np.stack([np.stack([cnt - t, np.floor((cnt - t) * rs.rand(3)), rs.randn(3), 4 * rs.rand(3)], -1) for t in range(3)]).astype(np.float32)
    assert np.array_equal(moons_countergan.metrics_from_sums(s), _cfeval.batch_mean_metrics(s, 2))
    assert np.array_equal(moons_countergan.metrics_from_sums(s[None]), _cfeval.batch_mean_metrics(s, 2)[None])
    # the house form: tiles of 16 rows, so a group of 16 is one tile and 37 rows are 3 groups x 1 tile
    got = house.metrics_from_sums(s, 16)
    assert house.fold_tiles(s, 16).shape == (3, 3, 4)
    assert np.array_equal(got, _cfeval.batch_mean_metrics(house.fold_tiles(s, 16), 17))
    assert not np.array_equal(got[:, 2], _cfeval.batch_mean_metrics(s, 2)[:, 2])   # D reaches the actionability
    with pytest.raises(PcgError, match="tile_sums must be"):
        house.metrics_from_sums(s[..., :3], 16)


def test_metric_rows():
    rows = _cfeval.metric_rows(np.array([[0.5, 0.25, np.nan], [1, 2, 3]]), ("a", "b", "c"))
    assert rows[1] == {"target_class": 1, "a": 1.0, "b": 2.0, "c": 3.0} and list(rows[0]) == ["target_class", "a", "b", "c"]
    assert all(type(v) is float for r in rows for k, v in r.items() if k != "target_class") and np.isnan(rows[0]["c"])
    assert list(_cfeval.metric_rows(np.zeros((1, 3)))[0]) == ["target_class", "class_flip", "prediction_gain", "avg_actionability"]


# ---- argument guards -------------------------------------------------------------------------------------------------------------------
def test_targets_arg_forms():
    for t in (2, np.int64(2), np.int32(2)):
        got = _cfeval.targets_arg(t, 4, 3)
        assert got.dtype == torch.int64 and got.tolist() == [2, 2, 2, 2]
    for t in (torch.tensor([0, 1, 2, 0]), torch.tensor([0, 1, 2, 0], dtype=torch.int32), np.array([0, 1, 2, 0]), [0, 1, 2, 0]):
        got = _cfeval.targets_arg(t, 4, 3, refuse_bool=True)
        assert got.dtype == torch.int64 and got.tolist() == [0, 1, 2, 0]
    assert _cfeval.targets_arg(True, 2, 3).tolist() == [1, 1]                  # a Python bool is an int unless refused


@pytest.mark.parametrize("refuse_bool", [False, True])
def test_targets_arg_refusals(refuse_bool):
    def call(t, N=4, K=3):
        return _cfeval.targets_arg(t, N, K, refuse_bool=refuse_bool)
    for bad in ([0, 1, 2], torch.zeros(5, dtype=torch.int64), np.zeros((4, 1), np.int64),               # wrong length / shape
                np.zeros(4), torch.zeros(4), torch.tensor([True, False, True, False]), np.ones(4, bool)):  # float and bool dtypes
        with pytest.raises(PcgError, match=r"target must be an int or \[N\] integers \(N = 4\), got"):
            call(bad)
    for bad, lo, hi in ((3, 3, 3), (-1, -1, -1), (np.int64(7), 7, 7), ([0, 1, 2, 3], 0, 3), (torch.tensor([0, -2, 1, 0]), -2, 1)):
        with pytest.raises(PcgError, match=rf"targets must lie in \[0, 3\), got \[{lo}, {hi}\]"):
            call(bad)
    if refuse_bool:
        with pytest.raises(PcgError, match=r"target must be an int or \[N\] integers \(N = 4\), got \(\) torch.bool"):
            call(True)
    else:
        assert call(True).tolist() == [1, 1, 1, 1]


def test_rows_arg():
    x, given = _cfeval.rows_arg(np.zeros((5, 2)), 2)
    assert not given and x.dtype == torch.float32 and tuple(x.shape) == (5, 2)   # an ndarray is taken as float32
    t = torch.zeros(5, 2, requires_grad=True)
    x, given = _cfeval.rows_arg(t, 2)
    assert given and x is t                                                     # kept as given: the caller's autograd refusal sees it
    x, given = _cfeval.rows_arg(t, 2, detach=True)
    assert given and not x.requires_grad and x.data_ptr() == t.data_ptr()
    ints = torch.zeros(5, 2, dtype=torch.int64)
    assert _cfeval.rows_arg(ints, 2)[0] is ints                                 # any dtype ...
    with pytest.raises(PcgError, match=r"X must be \[N\]\[2\] floats with N >= 1, got \(5, 2\) torch.int64"):
        _cfeval.rows_arg(ints, 2, "X", floats_only=True)                        # ... unless floats only
    assert _cfeval.rows_arg(np.zeros((5, 17), np.int64), 17, floats_only=True)[0].dtype == torch.float32
    for bad in (np.zeros((0, 2)), np.zeros((5, 3)), np.zeros(5), np.zeros((1, 5, 2)), torch.zeros(0, 2)):
        with pytest.raises(PcgError, match=r"^x must be \[N\]\[2\] with N >= 1, got \("):
            _cfeval.rows_arg(bad, 2)
        with pytest.raises(PcgError, match=r"^X must be \[N\]\[2\] floats with N >= 1, got \(.*\) torch.float"):
            _cfeval.rows_arg(bad, 2, "X", floats_only=True)


def test_labels_arg_and_check_outputs():
    assert _cfeval.labels_arg(None, 4) is None
    for y in (np.arange(4), [0, 1, 2, 3], torch.arange(4), torch.arange(4, dtype=torch.int32), np.ones(4, bool)):
        assert tuple(_cfeval.labels_arg(y, 4).shape) == (4,)
    for bad in (np.arange(3), np.zeros(4), torch.zeros(4), np.zeros((4, 1), np.int64)):
        with pytest.raises(PcgError, match=r"y must be \[N\] integers \(N = 4\), got"):
            _cfeval.labels_arg(bad, 4)
    assert _cfeval.check_outputs((), ("a", "b")) is None and _cfeval.check_outputs(["b", "a"], ("a", "b")) is None
    with pytest.raises(PcgError, match=r"outputs \['c', 'd'\] are not among \('a', 'b'\)"):
        _cfeval.check_outputs(("a", "c", "d"), ("a", "b"))


def test_upload_and_one_gpu_on_the_cpu():
    t = torch.arange(6, dtype=torch.int32).view(2, 3).t()
    got = _cfeval.upload(t, torch.device("cpu"))
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, t.float())
    assert _cfeval.upload(t, torch.device("cpu"), torch.int64).dtype == torch.int64
    a, b = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    with pytest.raises(PcgError, match=r"^TrainSteps: the nets are on cpu; libpcgan_hip has no CPU path"):
        _epoch.one_gpu(a, b)
    with pytest.raises(PcgError, match=r"^the sweep: .*no CPU path"):
        _epoch.one_gpu(a, who="the sweep")
    with pytest.raises(PcgError, match=r"^the sweep: the nets must be on one GPU"):
        _epoch.one_gpu(a, b.to("meta"), who="the sweep")


# ---- CSV text --------------------------------------------------------------------------------------------------------------------------
def test_confusion_csv_and_save_table_text(tmp_path, capsys, monkeypatch):
    assert _cfeval.confusion_csv(np.array([[5, 1], [0, 7]])) == ",pred_0,pred_1\ntrue_0,5,1\ntrue_1,0,7\n"
    assert _cfeval.confusion_csv(_cfeval.confusion_matrix([0, 0, 2], [0, 2, 2])) == ",pred_0,pred_1\ntrue_0,1,1\ntrue_1,0,1\n"
    assert [_cfeval.csv_value(v) for v in (float("nan"), 0.1, 1e-07, 3, "both", 2.0)] == ["", "0.1", "1e-07", "3", "both", "2.0"]
    rows = [{"target_class": 0, "gain": 0.1 + 0.2, "flip": float("nan"), "mask": "both"}, {"target_class": 1, "gain": 1e-07, "flip": 1.0, "mask": "none"}]
    path = tmp_path / "deeper" / "table.csv"
    _cfeval.save_table(rows, str(path), ("target_class", "flip", "gain", "mask"))
    assert path.read_text() == "target_class,flip,gain,mask\n0,,0.30000000000000004,both\n1,1.0,1e-07,none\n"
    monkeypatch.chdir(tmp_path)
    _cfeval.save_table(rows[:1], "bare.csv", ("mask",))                          # no directory part
    assert (tmp_path / "bare.csv").read_text() == "mask\nboth\n"
    assert capsys.readouterr().out == ""                                         # it does not print; moons' save_metrics does
    moons_countergan.save_metrics(rows, str(path), ("target_class", "gain"))
    assert capsys.readouterr().out == f"Saved metrics to {path}\n"
    assert path.read_text() == "target_class,gain\n0,0.30000000000000004\n1,1e-07\n"


# ---- FrozenClassifier ------------------------------------------------------------------------------------------------------------------
class Recorder(pnn.FrozenClassifier):
    def __init__(self):
        super().__init__()
        self.lin, self.calls = torch.nn.Linear(2, 2), []

    def _run_forward(self, x, keep=True):
        self.calls.append(("run_forward", keep)); return "logits", "saved"

    def _run_backward(self, saved, d):
        self.calls.append(("run_backward",))

    def _train_forward(self, x, masks):
        self.calls.append(("train_forward",)); return "logits", "saved"

    def _train_backward(self, saved, d):
        self.calls.append(("train_backward",))


def test_frozen_classifier_scaffold_on_the_cpu():
    net = Recorder()
    assert net.rng is None and net.dropout_masks is None and net._packed is None
    for mode in (True, False):
        net.train(mode)
        with pytest.raises(PcgError, match=r"^Recorder: input is on cpu; libpcgan_hip has no CPU path$"):
            net(torch.zeros(3, 2))
    assert net.calls == [] and net.rng is None                                  # refused before anything is drawn or run
    for mode in (False, True):
        net._packed = ("key", "image")
        assert net.train(mode) is net and net._packed is None and net.training is mode
    net._packed = ("key", "image")
    assert net.eval()._packed is None
    # eval mode, nothing asks for a gradient: the plain forward without saved activations
    on_gpu = types.SimpleNamespace(is_cuda=True, requires_grad=False)
    assert net(on_gpu) == "logits" and net.calls == [("run_forward", False)]
    for cls in (house.NNClassifier(17, 4), countergan.CNNClassifier()):
        with pytest.raises(PcgError, match=rf"^{type(cls).__name__}: input is on cpu; libpcgan_hip has no CPU path$"):
            cls(torch.zeros(2, 17))
