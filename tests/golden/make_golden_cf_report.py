"""Golden fixtures for the evaluation reports: the reference's own `visualize_counterfactual_grid`
(conditional_counteRGAN/mnist/eval_utils.py:113-201) and `generate_case_study_report_from_vis`
(conditional_counteRGAN/house_sales_kc_usa/eval_utils.py:496-664), lifted from the syntax tree the way make_golden_mnist_cf_eval.py and
make_golden_house_cf_eval.py lift theirs (the modules import seaborn) and run on the CPU in fp32 and in float64.  `plt` is bound to a
recording stub whose `imshow` keeps the array it is given: the grid's cells.  Writes tests/golden/cf_report_ref.npz.

    python tests/golden/make_golden_cf_report.py <path of the reference repository> [output directory]

MNIST: the reference ResidualGenerator with tests/golden/countergan_generator_trained.pt, the seeded CNNClassifier
(torch.manual_seed(3)), a 40-row data set on the 1/8 grid in [-1, 1] (torch seed SEED_MNIST) with labels i % 10; both pick_best_source
values ("first", "best"), and pick_best_source=True on the same rows with the labels grid.y_late (i % 9 below row 30, so class 9 first
shows up at row 39, the scan reaches the last row and every class has four candidates: mode "late").  Recorded per mode:
  grid.x [40][1][28][28], grid.y [40]
  grid.<mode>.rows [10]                 the data-set row the function picked per class (found by matching the diagonal cell)
  grid.<mode>.cells [10][10][28][28]    what imshow was given, [source][target] (the diagonal: the source)
  grid.<mode>.pred, .conf [10][10]      :187-188 of every off-diagonal cell (the classifier is wrapped); the diagonal holds r and 1.0
  grid.<mode>.probs [10][10][10]        the fp32 softmax of every off-diagonal cell, .undecided [10][10]
  grid.<mode>.raw_scale                 max |raw residual| over the cells (the generator is wrapped): the scale of the query tests' atol
  grid.best|late.row_conf [n]           the fp32 confidence :142 computed per scanned row, .pick_undecided [10].  The `break`
                                        of :148-149 stands after the if / else, so the "best" scan too ends at the row that completes the
                                        set of classes: n = 10 in "best" (the most confident row is chosen among those rows only), n = 40 in "late".
House: the reference NNClassifier with tests/golden/house_classifier_trained.pt; originals = the first 60 rows of X_test of
tests/golden/house_preprocess.npz clipped to [0, 1] as fp32; cfs = clip(originals + planted changes) (numpy seed SEED_HOUSE): 6-9
changed features per row, each by 0.05 + 0.013 j for distinct j (so every change is >= 0.05 and two of a row differ by >= 0.01), unchanged
features bit-equal.  Recorded: case.originals, case.cfs [60][17], case.feature_names (JSON), case.data_min / data_max [17], case.idxs
[20], case.probs_orig, case.probs_cf [20][4], case.sample_rows / feature_rows / aggregate (JSON records of the three tables),
case.files (JSON, the relative paths written), case.undecided [20].

A grid cell or a case row is UNDECIDED when the float64 run's top-two probability gap is under max(1e-5, 100 * max|p_fp32 - p_fp64|);
in "best" mode a class's pick is undecided when its top-two float64 confidences are closer than that bound.  The script asserts at most
5 % of the 90 cells of a mode, 0 of the 10 picks and 0 of the 20 case rows."""
import ast
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_MNIST, SEED_HOUSE = 41, 7
N_GRID, N_CASE = 40, 60


def lift(path, names, ns):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(defs) == len(names), (path, [d.name for d in defs])
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


class _Ax:
    spines = {}

    def __init__(self, cells, rc):
        self.cells, self.rc = cells, rc

    def imshow(self, img, **kw):
        self.cells[self.rc] = np.array(img, copy=True)

    def axis(self, *a, **k):
        pass


class _Axes:
    def __init__(self, cells):
        self.cells = cells

    def __getitem__(self, rc):
        return _Ax(self.cells, rc)


class _Plt:
    """Stands in for matplotlib.pyplot: subplots hands out axes whose imshow records its array; everything else does nothing."""

    def __init__(self):
        self.cells = {}

    def subplots(self, *a, **k):
        return None, _Axes(self.cells)

    def __getattr__(self, name):
        return lambda *a, **k: None


class _Recorded(torch.nn.Module):
    """The classifier, with the softmax of every call kept."""

    def __init__(self, net):
        super().__init__()
        self.net, self.probs = net, []

    def forward(self, x):
        logits = self.net(x.to(next(self.net.parameters()).dtype))      # (:129 probes with fp32 zeros whatever the net's dtype)
        self.probs.append(torch.softmax(logits, dim=1)[0].detach().numpy().copy())
        return logits


class _RecordedG(torch.nn.Module):
    """The generator, with the largest |raw residual| of its calls kept: the scale of the query tests' absolute tolerance."""

    def __init__(self, net):
        super().__init__()
        self.net, self.raw_max = net, 0.0

    def forward(self, x, t, m):
        raw, masked = self.net(x, t, m)
        self.raw_max = max(self.raw_max, float(raw.abs().max()))
        return raw, masked


class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi

    def inverse_transform(self, X):                  # sklearn's MinMaxScaler(feature_range=(0, 1))
        return np.asarray(X) * (self.data_max_ - self.data_min_) + self.data_min_


def bound_of(p32, p64):
    return max(1e-5, 100.0 * float(np.abs(np.asarray(p32, np.float64) - p64).max()))


def gap_of(p64):
    top = np.sort(p64, axis=-1)
    return top[..., -1] - top[..., -2]


def run_grid(fn, G, C, x, y, best, dtype):
    """One call of the lifted function -> (rows [10], cells [10][10][28][28], probs [10][10][10] (diagonal 0), row_conf or None, max |raw|)."""
    plt, rec, G = _Plt(), _Recorded(C), _RecordedG(G)
    fn.__globals__["plt"] = plt
    data = [(x[i].to(dtype), y[i]) for i in range(len(y))]
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        fn(G, rec, data, "cpu", save_path=os.path.join(tempfile.mkdtemp(), "cf_grid.png"), pick_best_source=best)
    calls = rec.probs[1:]                                            # the first call infers num_classes (:129)
    n_pick = len(calls) - 90
    # the `break` of :148-149 stands after the if / else, so the "best" scan too ends at the row that completes the set of classes
    seen_all = 1 + max(int(np.flatnonzero(y.numpy() == k)[0]) for k in range(10))
    assert n_pick == (seen_all if best else 0), n_pick
    row_conf = np.array([calls[i][int(y[i])] for i in range(n_pick)]) if best else None
    probs, k = np.zeros((10, 10, 10), np.float64), n_pick
    for r in range(10):
        for c in range(10):
            if r != c:
                probs[r, c] = calls[k]
                k += 1
    cells = np.stack([np.stack([plt.cells[r, c] for c in range(10)]) for r in range(10)])
    xv = (x.to(dtype).numpy()[:, 0] + 1.0) / 2.0
    rows = np.array([int(np.flatnonzero([np.array_equal(xv[i], cells[r, r]) for i in range(len(y))])[0]) for r in range(10)])
    return rows, cells, probs, row_conf, G.raw_max


def mnist_part(ref_root, out):
    import importlib
    import pandas as pd
    from typing import Dict, Tuple
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "mnist")
    sys.path.insert(0, mdir)
    gen_mod = importlib.import_module("models.generator")
    clf_mod = importlib.import_module("models.classifier")
    ns = {"torch": torch, "np": np, "F": F, "os": os, "pd": pd, "Dict": Dict, "Tuple": Tuple}
    fn = lift(os.path.join(mdir, "eval_utils.py"), ("visualize_counterfactual_grid",), ns)["visualize_counterfactual_grid"]
    G = gen_mod.ResidualGenerator()
    G.load_state_dict(torch.load(os.path.join(HERE, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    torch.manual_seed(3)
    C = clf_mod.CNNClassifier()
    G.eval(); C.eval()
    G64, C64 = copy.deepcopy(G).double(), copy.deepcopy(C).double()
    g = torch.Generator().manual_seed(SEED_MNIST)
    x = torch.randint(-8, 9, (N_GRID, 1, 28, 28), generator=g).float() / 8.0
    y = torch.arange(N_GRID) % 10
    # with labels i % 10 the reference's scan ends after 10 rows and "best" can only repeat "first"; the "late" labels hold class 9
    # back to row 39, so the same rows are scanned to the end and every class has four candidates: a recording that tells a best pick
    # from a first one
    y_late = torch.where(torch.arange(N_GRID) < 30, torch.arange(N_GRID) % 9, y)
    out["grid.x"], out["grid.y"], out["grid.y_late"] = x.numpy(), y.numpy(), y_late.numpy()
    report = []
    for mode, best, y in (("first", False, y), ("best", True, y), ("late", True, y_late)):
        rows, cells, p32, rc32, raw_max = run_grid(fn, G, C, x, y, best, torch.float32)
        rows64, _, p64, rc64, _ = run_grid(fn, G64, C64, x, y, best, torch.float64)
        assert np.array_equal(rows, rows64), (mode, rows, rows64)
        off = ~np.eye(10, dtype=bool)
        bound = bound_of(p32[off], p64[off])
        if best:
            bound = max(bound, bound_of(rc32, rc64))
        und = (gap_of(p64) < bound) & off
        assert und.sum() <= 0.05 * 90, f"{mode}: {int(und.sum())} of 90 cells undecided (bound {bound:.1e}): pick another seed"
        pred = p32.argmax(-1)
        conf = np.take_along_axis(p32, pred[..., None], -1)[..., 0].astype(np.float32)
        d = np.arange(10)
        pred[d, d], conf[d, d] = d, 1.0
        out[f"grid.{mode}.rows"], out[f"grid.{mode}.cells"] = rows, cells.astype(np.float32)
        out[f"grid.{mode}.pred"], out[f"grid.{mode}.conf"] = pred, conf
        out[f"grid.{mode}.probs"], out[f"grid.{mode}.undecided"] = p32.astype(np.float32), und
        out[f"grid.{mode}.undecided_bound"], out[f"grid.{mode}.raw_scale"] = np.float64(bound), np.float64(raw_max)
        if best:
            pick_und, ys = np.zeros(10, bool), y.numpy()[:len(rc32)]            # the rows the scan reached
            for k in range(10):
                c = np.sort(rc64[ys == k])
                pick_und[k] = len(c) > 1 and (c[-1] - c[-2]) < bound
                assert int(np.argmax(np.where(ys == k, rc32, -1.0))) == rows[k]
            assert not pick_und.any(), f"best: picks {np.flatnonzero(pick_und)} undecided (bound {bound:.1e}): pick another seed"
            out[f"grid.{mode}.row_conf"], out[f"grid.{mode}.pick_undecided"] = rc32.astype(np.float32), pick_und
            if mode == "late":
                assert len(rc32) == N_GRID and (rows != np.array([int(np.flatnonzero(ys == k)[0]) for k in range(10)])).sum() >= 5, rows
        else:
            assert np.array_equal(rows, np.arange(10))
        report.append(f"{mode}: {int(und.sum())} / 90 cells undecided (bound {bound:.1e})")
    return report


def house_part(ref_root, out):
    from typing import Optional
    import pandas as pd
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "house_sales_kc_usa")
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())                     # the reference's config.py creates its results directories in the cwd
    try:
        for m in [m for m in sys.modules if m == "models" or m.startswith("models.") or m == "config"]:
            del sys.modules[m]                        # the MNIST half imported its own `models` package
        sys.path.insert(0, mdir)
        import importlib
        cfg = dict(importlib.import_module("config").config)
        clf_mod = importlib.import_module("models.nn_classifier")
        ns = {"torch": torch, "np": np, "F": F, "os": os, "pd": pd, "Optional": Optional}
        fn = lift(os.path.join(mdir, "eval_utils.py"), ("generate_case_study_report_from_vis",), ns)["generate_case_study_report_from_vis"]
        clf = clf_mod.NNClassifier(cfg["input_dim"], output_dim=cfg["num_classes"])
        clf.load_state_dict(torch.load(os.path.join(HERE, "house_classifier_trained.pt"), map_location="cpu", weights_only=True))
        clf.eval()
        pre = np.load(os.path.join(HERE, "house_preprocess.npz"))
        names = list(cfg["feature_names"])
        originals = np.clip(pre["X_test"][:N_CASE], 0.0, 1.0).astype(np.float32)
        rng = np.random.default_rng(SEED_HOUSE)
        change = np.zeros_like(originals)
        for i in range(N_CASE):
            m = int(rng.integers(6, 10))
            feats = rng.choice(originals.shape[1], size=m, replace=False)
            mags = 0.05 + 0.013 * rng.permutation(m)
            change[i, feats] = np.where(originals[i, feats] + mags <= 1.0, mags, -mags)
        cfs = np.clip(originals + change, 0.0, 1.0).astype(np.float32)
        moved = change != 0
        assert np.array_equal(cfs[~moved], originals[~moved]) and np.abs(cfs - originals)[moved].min() >= 0.0499
        scaler = _Scaler(pre["data_min"], pre["data_max"])
        save_dir = tempfile.mkdtemp()
        c2 = {"out_dir": save_dir, "feature_names": names, "cuda": "cpu"}
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            df, feat, agg = fn(clf, originals, cfs, c2, scaler=scaler, n_samples=20, save_dir=save_dir)
        idxs = df["sample_idx_in_vis"].to_numpy()
        assert np.array_equal(idxs, np.random.default_rng(42).choice(np.arange(N_CASE), size=20, replace=False))
        clf64 = copy.deepcopy(clf).double()
        with torch.no_grad():
            po = F.softmax(clf(torch.tensor(originals[idxs])), dim=1).numpy()
            pc = F.softmax(clf(torch.tensor(cfs[idxs])), dim=1).numpy()
            po64 = F.softmax(clf64(torch.tensor(originals[idxs]).double()), dim=1).numpy()
            pc64 = F.softmax(clf64(torch.tensor(cfs[idxs]).double()), dim=1).numpy()
        bound = max(bound_of(po, po64), bound_of(pc, pc64))
        und = (gap_of(po64) < bound) | (gap_of(pc64) < bound) | (gap_of(pc64 - po64) < bound)
        assert not und.any(), f"case rows {np.flatnonzero(und)} undecided (bound {bound:.1e}): pick another seed"
        ad = np.abs(cfs[idxs] - originals[idxs])
        for row in ad:                                # the top-k order and the `> eps` count are decided
            s = np.sort(row[row > 0])
            assert len(s) >= 5 and np.diff(s).min() >= 0.0099, s
        assert np.diff(np.sort(ad.mean(0))).min() > 1e-6, "the feature summary's sort has a tie: pick another seed"
        files = sorted(os.path.relpath(os.path.join(d, f), save_dir) for d, _, fs in os.walk(save_dir) for f in fs)
        out.update({"case.originals": originals, "case.cfs": cfs, "case.feature_names": np.array(json.dumps(names)),
                    "case.data_min": pre["data_min"], "case.data_max": pre["data_max"], "case.idxs": idxs, "case.probs_orig": po,
                    "case.probs_cf": pc, "case.sample_rows": np.array(json.dumps(df.to_dict(orient="records"))),
                    "case.feature_rows": np.array(json.dumps(feat.to_dict(orient="records"))), "case.aggregate": np.array(json.dumps(agg)),
                    "case.files": np.array(json.dumps(files)), "case.undecided": und, "case.undecided_bound": np.float64(bound)})
        return [f"case studies: 0 / 20 rows undecided (bound {bound:.1e}), {len(files)} files"]
    finally:
        os.chdir(cwd)


def main(ref_root, out_dir=HERE):
    ref_root, out_dir = os.path.abspath(ref_root), os.path.abspath(out_dir)
    out = {}
    report = mnist_part(ref_root, out) + house_part(ref_root, out)
    path = os.path.join(out_dir, "cf_report_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.0f} kB; " + "; ".join(report))


if __name__ == "__main__":
    main(sys.argv[1], *(sys.argv[2:3]))
