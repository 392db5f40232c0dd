"""Golden fixtures for the moons CounteRGAN's evaluation (conditional_counteRGAN/moons/eval_utils.py): the reference's own eval_utils
and models run on the CPU, unmodified — pandas, scikit-learn and matplotlib (Agg) must be importable.  Reads the test split of
tests/golden/moons_cf_ref.npz and the two shipped checkpoints next to it; writes tests/golden/moons_cf_eval_ref.npz.

    python tests/golden/make_golden_moons_cf_eval.py <path of the reference repository> [output directory]

Recorded (M = 4 masks in MASKS' order both / none / x_only / y_only, T = 3 targets, N = 240 rows, batch_size 64: 4 loader batches):
  mask_names [4], masks [4][2]
  metrics [4][3][3]                      compute_metrics_per_target's table per mask: class_flip, prediction_gain, avg_actionability
  counts, flips [4][3][4] int64          per (mask, target, batch): rows with y != target, and those the classifier puts in the target
  batch_means [4][3][4][3]               the three per-batch means as the function appends them (its locals at eval_utils.py:95)
  x_cf, masked [4][3][240][2], logits_cf [4][3][240][3], logits_x [240][3]
                                         the reference's models on every row (fp32); on the rows the function evaluates they are
                                         checked here against its own locals
  cf_margin64 [4][3][240]                top-2 margin of the counterfactual's logits, nets in float64
  confusion_csv (text), confusion [3][3], accuracy
                                         evaluate_classifier's classifier_confusion.csv, sklearn's matrix and accuracy
  grid_Z [200][200] int8, grid_margin [200][200] float32
                                         plot_decision_boundaries_only's Z (eval_utils.py:196-206) and the float64 nets' top-2 logit
                                         margin at every grid point (computed in float64, stored rounded to float32)
"""
import copy
import os
import shutil
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
MASKS = (("both", (1, 1)), ("none", (0, 0)), ("x_only", (1, 0)), ("y_only", (0, 1)))       # eval_utils.py:231-236


def margin(logits):
    top = torch.topk(logits, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).numpy()


def main(ref_root, out_dir=HERE):
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "moons")
    sys.path.insert(0, mdir)
    import eval_utils
    from models.generator import ResidualGenerator
    from models.nn_classifier import NNClassifier

    data = np.load(os.path.join(HERE, "moons_cf_ref.npz"))
    X, y = data["data.X_test"], data["data.y_test"]
    G = ResidualGenerator(2, 32, num_classes=3)
    G.load_state_dict(torch.load(os.path.join(HERE, "moons_cf_generator_trained.pt"), map_location="cpu"))
    clf = NNClassifier(2)
    clf.load_state_dict(torch.load(os.path.join(HERE, "moons_cf_classifier_trained.pt"), map_location="cpu"))
    G.eval(); clf.eval()
    G64, clf64 = copy.deepcopy(G).double().eval(), copy.deepcopy(clf).double().eval()
    tmp = tempfile.mkdtemp()
    cfg = {"cuda": "cpu", "batch_size": 64, "out_dir": tmp}
    N, M, T, bs = len(X), len(MASKS), 3, cfg["batch_size"]
    nb = (N + bs - 1) // bs
    out = {"mask_names": np.array([n for n, _ in MASKS]), "masks": np.array([m for _, m in MASKS], np.float32)}

    # ---- compute_metrics_per_target, traced at the line that appends the per-batch means ---------------------------------------
    code = eval_utils.compute_metrics_per_target.__code__
    rec = []
    state = {"batch": -1}

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(fr, ev, ar):
            if ev == "line":
                if fr.f_lineno == 49:                          # `flips_per_batch = []`: a new target
                    state["batch"] = -1
                elif fr.f_lineno == 54:                        # `x_batch = x_batch.to(device)`: the next loader batch
                    state["batch"] += 1
                elif fr.f_lineno == 95:                        # `flips_per_batch.append(flip_rate)`
                    loc = fr.f_locals
                    rec.append({"target": loc["target"], "batch": state["batch"], "count": loc["bs"],
                                "flips": int((loc["cf_preds"] == loc["target_vec"]).sum()),
                                "means": (loc["flip_rate"], loc["pred_gain"], loc["actionability"]),
                                "sel": loc["mask_samples"].numpy().copy(), "cf": loc["cf"].numpy().copy(),
                                "masked": loc["masked_residual"].numpy().copy(), "cf_logits": loc["cf_logits"].numpy().copy()})
            return local
        return local

    metrics = np.zeros((M, T, 3))
    counts, flips = np.zeros((M, T, nb), np.int64), np.zeros((M, T, nb), np.int64)
    batch_means = np.full((M, T, nb, 3), np.nan)
    x_cf, masked = np.zeros((M, T, N, 2), np.float32), np.zeros((M, T, N, 2), np.float32)
    logits_cf, cf_margin64 = np.zeros((M, T, N, 3), np.float32), np.zeros((M, T, N))
    xt = torch.tensor(X, dtype=torch.float32)
    with torch.no_grad():
        out["logits_x"] = clf(xt).numpy()
    for mi, (name, mk) in enumerate(MASKS):
        mk = np.array(mk, np.float32)
        del rec[:]
        sys.settrace(tracer)
        try:
            df = eval_utils.compute_metrics_per_target(G, clf, X, y, cfg, mask=mk)
        finally:
            sys.settrace(None)
        assert list(df["target_class"]) == [0, 1, 2]
        metrics[mi] = df[["class_flip", "prediction_gain", "avg_actionability"]].to_numpy()
        with torch.no_grad():
            for t in range(T):
                oh = F.one_hot(torch.full((N,), t), 3).float()
                mt = torch.tensor(mk).unsqueeze(0).expand(N, -1)
                _, md = G(xt, oh, mask=mt)
                cf = xt + md
                x_cf[mi, t], masked[mi, t], logits_cf[mi, t] = cf.numpy(), md.numpy(), clf(cf).numpy()
                _, md64 = G64(xt.double(), oh.double(), mask=mt.double())
                cf_margin64[mi, t] = margin(clf64(xt.double() + md64))
        for r in rec:
            t, b = r["target"], r["batch"]
            counts[mi, t, b], flips[mi, t, b], batch_means[mi, t, b] = r["count"], r["flips"], r["means"]
            rows = np.arange(b * bs, min((b + 1) * bs, N))[r["sel"]]
            assert np.array_equal(y[rows] != t, np.ones(len(rows), bool)) and len(rows) == r["count"]
            for ours, theirs in ((x_cf, r["cf"]), (masked, r["masked"]), (logits_cf, r["cf_logits"])):
                np.testing.assert_allclose(ours[mi, t][rows], theirs, rtol=1e-5, atol=1e-6)
        assert len(rec) == T * nb, "a (target, batch) without rows: record it as count 0"
    out.update(metrics=metrics, counts=counts, flips=flips, batch_means=batch_means, x_cf=x_cf, masked=masked, logits_cf=logits_cf,
               cf_margin64=cf_margin64)

    # ---- evaluate_classifier ---------------------------------------------------------------------------------------------------
    from sklearn.metrics import accuracy_score, confusion_matrix
    eval_utils.evaluate_classifier(clf, X, y, cfg)
    out["confusion_csv"] = np.array(open(os.path.join(tmp, "classifier_confusion.csv")).read())
    with torch.no_grad():
        preds = clf(xt).argmax(1).numpy()
    out["confusion"] = confusion_matrix(y, preds).astype(np.int64)
    out["accuracy"] = np.array(accuracy_score(y, preds))
    out["x_margin64"] = margin(clf64(xt.double()).detach())

    # ---- the decision grid (plot_decision_boundaries_only) -------------------------------------------------------------------
    holder = {}
    real_contourf = eval_utils.plt.contourf

    def rec_contourf(xx, yy, Z, *a, **k):
        holder.update(xx=np.array(xx), yy=np.array(yy), Z=np.array(Z))
        return real_contourf(xx, yy, Z, *a, **k)

    eval_utils.plt.contourf = rec_contourf
    try:
        eval_utils.plot_decision_boundaries_only(clf, X, y, cfg, save_name="grid.png")
    finally:
        eval_utils.plt.contourf = real_contourf
    grid = torch.tensor(np.c_[holder["xx"].ravel(), holder["yy"].ravel()], dtype=torch.float32)
    out["grid_Z"] = holder["Z"].astype(np.int8)
    with torch.no_grad():
        out["grid_margin"] = margin(clf64(grid.double())).reshape(holder["Z"].shape).astype(np.float32)
    shutil.rmtree(tmp, ignore_errors=True)

    np.savez_compressed(os.path.join(out_dir, "moons_cf_eval_ref.npz"), **out)
    print(f"wrote {len(out)} arrays to {os.path.join(out_dir, 'moons_cf_eval_ref.npz')}")
    print("min float64 margin: counterfactuals", cf_margin64.min(), "test rows", out["x_margin64"].min(), "grid", out["grid_margin"].min(),
          "grid points below 1e-3:", int((out["grid_margin"] < 1e-3).sum()))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
