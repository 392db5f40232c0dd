"""CPU: the host half of the evaluation reports.  The header declares the three entries of csrc/cf_report.hip and
the built library exports them; house.case_study_tables against the reference's own recorded tables
(tests/golden/cf_report_ref.npz, written by tests/golden/make_golden_cf_report.py); _cfeval.write_png_gray through Pillow; the rules of
the restated pick (tests/cf_report_restate.py) and its pixel arithmetic against the reference's recorded cells."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cf_report_restate as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcg_class_pick", "pcg_class_pick_gather", "pcg_cf_panels")
INT_COLS = ("sample_idx_in_vis", "source_pred", "intended_target", "cf_pred", "success", "num_changed")
STR_COLS = ("topk_features", "topk_vals_pct_of_range")
FLOAT_COLS = ("prediction_gain", "frac_changed", "sparsity", "L1_sum_norm", "L1_mean_norm", "L2_norm")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cf_report_ref.npz")))


class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi

    def inverse_transform(self, X):
        return np.asarray(X) * (self.data_max_ - self.data_min_) + self.data_min_


def case_tables(gold, H, probs_orig=None, probs_cf=None):
    names = json.loads(str(gold["case.feature_names"]))
    return names, H.case_study_tables(gold["case.probs_orig"] if probs_orig is None else probs_orig,
                                      gold["case.probs_cf"] if probs_cf is None else probs_cf, gold["case.originals"], gold["case.cfs"], names,
                                      scaler=_Scaler(gold["case.data_min"], gold["case.data_max"]), n_samples=20)


def check_case_tables(gold, names, tables, skip_rows=(), gain_tol=None):
    """Our tables against the recorded ones: integer and string columns, column order and row order exact, float columns to 1e-6
    relative; `skip_rows`: sample rows whose classifier decisions are left out; gain_tol: (rtol, atol) of prediction_gain where the
    probabilities are not the recorded ones."""
    sample_rows, feature_rows, aggregate, per_sample = tables
    want = json.loads(str(gold["case.sample_rows"]))
    assert [r["sample_idx_in_vis"] for r in sample_rows] == [int(i) for i in gold["case.idxs"]] == [w["sample_idx_in_vis"] for w in want]
    for i, (got, w) in enumerate(zip(sample_rows, want)):
        assert list(got) == list(w), "column order"
        for c in INT_COLS + STR_COLS:
            if i in skip_rows and c in ("source_pred", "intended_target", "cf_pred", "success"):
                continue
            assert got[c] == w[c] and type(got[c]) is type(w[c]), (i, c, got[c], w[c])
        for c in FLOAT_COLS:
            rtol, atol = gain_tol if (c == "prediction_gain" and gain_tol) else (1e-6, 0.0)
            np.testing.assert_allclose(got[c], w[c], rtol=rtol, atol=atol, err_msg=f"{i} {c}")
    wf = json.loads(str(gold["case.feature_rows"]))
    assert [r["feature"] for r in feature_rows] == [w["feature"] for w in wf], "row order of the feature summary"
    # the reference assigns mean_abs_delta_denorm after the sort, in unsorted order: its k-th value belongs to feature k
    denorm_of = {names[k]: w["mean_abs_delta_denorm"] for k, w in enumerate(wf)}
    for got, w in zip(feature_rows, wf):
        assert list(got) == list(w)
        for c in ("mean_abs_delta_norm", "mean_pct_of_range", "change_freq"):
            np.testing.assert_allclose(got[c], w[c], rtol=1e-6, err_msg=f"{got['feature']} {c}")
        np.testing.assert_allclose(got["mean_abs_delta_denorm"], denorm_of[got["feature"]], rtol=1e-6, err_msg=got["feature"])
    assert any(abs(g["mean_abs_delta_denorm"] - w["mean_abs_delta_denorm"]) > 1e-6 * abs(w["mean_abs_delta_denorm"]) for g, w in zip(feature_rows, wf)), \
        "the fixture must show the reference's misplaced column"
    wa = json.loads(str(gold["case.aggregate"]))
    assert list(aggregate) == list(wa)
    for k, v in wa.items():
        if isinstance(v, str) or k == "n_samples_used":
            assert aggregate[k] == v, k
        elif skip_rows or gain_tol:
            if k not in ("class_flip_rate", "mean_prediction_gain", "median_prediction_gain"):
                np.testing.assert_allclose(aggregate[k], v, rtol=1e-6, err_msg=k)
        else:
            np.testing.assert_allclose(aggregate[k], v, rtol=1e-6, err_msg=k)
    assert len(per_sample) == 20 and all(len(s["rows"]) == len(names) for s in per_sample)
    assert list(per_sample[0]["rows"][0]) == ["feature", "orig_norm", "cf_norm", "abs_delta_norm", "pct_of_range", "orig_denorm", "cf_denorm",
                                              "abs_delta_denorm", "pct_of_range_denorm"]


def expected_files(gold):
    return json.loads(str(gold["case.files"]))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_report_entries():
    import pcgan_amd
    from pcgan_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcgan_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcg_[a-z0-9_]+)\s*\(", text))
    pcgan_amd.load()
    raw = ctypes.CDLL(pcgan_amd.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in pcgan_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by libpcgan_hip.so"
        assert name in _lib.PROTOTYPES
    for macro, value in (("PCG_CLASS_PICK_FIRST", _lib.CLASS_PICK_FIRST), ("PCG_CLASS_PICK_BEST", _lib.CLASS_PICK_BEST),
                         ("PCG_CLASS_PICK_KMAX", _lib.CLASS_PICK_KMAX), ("PCG_CF_PANELS_GRID", _lib.CF_PANELS_GRID),
                         ("PCG_CF_PANELS_PANELS", _lib.CF_PANELS_PANELS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value, macro


# ---- the case-study tables -----------------------------------------------------------------------------------------------------------------
def test_case_study_tables_reproduce_the_reference(gold):
    from pcgan_amd import house as H
    assert not gold["case.undecided"].any()
    names, tables = case_tables(gold, H)
    check_case_tables(gold, names, tables)
    assert np.array_equal(H.case_study_rows(60, 20, 42), gold["case.idxs"])
    with pytest.raises(H.PcgError, match="chosen rows"):
        H.case_study_tables(gold["case.probs_orig"][:5], gold["case.probs_cf"][:5], gold["case.originals"], gold["case.cfs"], names)
    with pytest.raises(H.PcgError, match="originals"):
        H.case_study_tables(gold["case.probs_orig"], gold["case.probs_cf"], gold["case.originals"], gold["case.cfs"][:, :3], names)


def test_case_study_tables_without_a_scaler_and_with_fewer_rows_than_asked(gold):
    from pcgan_amd import house as H
    names = json.loads(str(gold["case.feature_names"]))
    o, c = gold["case.originals"][:7], gold["case.cfs"][:7]
    p = np.tile(np.array([[0.7, 0.1, 0.1, 0.1]], np.float32), (7, 1))
    q = np.tile(np.array([[0.1, 0.6, 0.2, 0.1]], np.float32), (7, 1))
    sample_rows, feature_rows, aggregate, per_sample = H.case_study_tables(p, q, o, c, names, n_samples=20)
    assert aggregate["n_samples_used"] == 7 and len(sample_rows) == 7 and "mean_abs_delta_denorm" not in feature_rows[0]
    assert all(r["source_pred"] == 0 and r["intended_target"] == 1 and r["cf_pred"] == 1 and r["success"] == 1 for r in sample_rows)
    assert list(per_sample[0]["rows"][0]) == ["feature", "orig_norm", "cf_norm", "abs_delta_norm", "pct_of_range"]


# ---- the PNG writer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (28, 30), (280, 280)])
def test_write_png_gray_round_trips_through_pillow(tmp_path, shape):
    from PIL import Image
    from pcgan_amd import _cfeval
    a = np.random.RandomState(shape[1]).randint(0, 256, shape).astype(np.uint8)
    a.flat[0], a.flat[-1] = 255, 0
    path = str(tmp_path / "sub" / "g.png")
    _cfeval.write_png_gray(path, a)
    with Image.open(path) as im:
        assert im.mode == "L" and im.size == (shape[1], shape[0])
        np.testing.assert_array_equal(np.asarray(im), a)
    with pytest.raises(_cfeval.PcgError):
        _cfeval.write_png_gray(path, a.astype(np.float32))


# ---- the restated pick ---------------------------------------------------------------------------------------------------------------------
def test_restated_pick_rules():
    labels = np.array([2, 0, 1, 0, 1, 7, -1, 1, 0, 2])                        # K = 4: class 3 absent, 7 and -1 out of range
    conf = np.array([0.5, 0.3, 0.9, 0.6, 0.9, 1.0, 1.0, np.nan, 0.6, 0.25])
    rows, c = RR.pick(labels, 4, conf)
    assert rows.tolist() == [3, 2, 0, RR.ABSENT] and c.tolist() == [0.6, 0.9, 0.5, 0.0]   # ties (0.6, 0.9) go to the lower row; NaN skipped
    first, c0 = RR.pick(labels, 4)
    assert first.tolist() == [1, 2, 0, RR.ABSENT] and not c0.any()
    for chunks in ([(0, 4), (4, 4), (8, 2)], [(8, 2), (4, 4), (0, 4)], [(4, 4), (0, 4), (8, 2)]):
        assert RR.pick(labels, 4, conf, chunks)[0].tolist() == rows.tolist(), chunks
        assert RR.pick(labels, 4, chunks=chunks)[0].tolist() == first.tolist(), chunks
    assert RR.scan_end(labels, 4) == 10 and RR.scan_end(labels, 3) == 3
    lg = np.array([[0.0, 1.0, 2.0, -1.0], [3.0, 3.0, 3.0, 3.0]])
    got = RR.confidences(lg, np.array([2, 9]))
    np.testing.assert_allclose(got[0], np.exp(2.0) / np.exp(lg[0]).sum(), rtol=1e-15)
    assert np.isnan(got[1])


def test_restated_pixels_are_the_references_cells(gold):
    """(x + 1) / 2 of the recorded sources is the diagonal the reference drew, bit for bit; the uint8 convention at its edges."""
    x = gold["grid.x"]
    for mode in ("first", "best", "late"):
        rows, cells = gold[f"grid.{mode}.rows"], gold[f"grid.{mode}.cells"]
        src = x[rows, 0]
        x_cf = np.transpose(cells, (1, 0, 2, 3)) * 2.0 - 1.0                    # off the diagonal only the layout matters here
        img, u8 = RR.grid_image(src, x_cf.astype(np.float32))
        for r in range(10):
            np.testing.assert_array_equal(img[r * 28:(r + 1) * 28, r * 28:(r + 1) * 28], cells[r, r])
        assert img.shape == (280, 280) and u8.dtype == np.uint8
    assert RR.to_u8(np.array([0.0, 1.0, 0.5, 0.499 / 255, 0.5 / 255, 1.2, -0.3], np.float32)).tolist() == [0, 255, 128, 0, 1, 255, 0]
    p, vmax = RR.panels(np.array([[[-1.0, 0.0]]], np.float32), np.array([[[1.0, 0.25]]], np.float32), np.array([[1.0, 0.0]], np.float32))
    assert p.shape == (1, 4, 1, 2) and p[0, :, 0, :].tolist() == [[0.0, 0.5], [1.0, 0.625], [1.0, 0.125], [1.0, 0.0]] and vmax == 1.0
