"""Restatement of the evaluation reports' data half in NumPy / torch on the CPU: the source pick of
conditional_counteRGAN/mnist/eval_utils.py:135-149 from given confidences, the pixel arithmetic of the counterfactual grid (:175, :190,
with the 8-bit convention of torchvision's save_image) and of the four heat-map panels (gr.py:370-372, :399), and the grid of the
additive-delta generators, for which the reference has no function: the pick + gan_train_copy.py:161-172 per cell
(tests/delta_cf_restate.py's query).  The references of tests/test_hip_cf_report.py; tests/test_cf_report_host.py checks the pick's
rules here and pins the pixel arithmetic to the reference's recorded cells (tests/golden/cf_report_ref.npz)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ABSENT = -1


def confidences(logits, labels):
    """softmax(logits[i, :K])[labels[i]] per row in the dtype given, max-subtracted; a label outside [0, K) gives nan (never picked)."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    K = logits.shape[1]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    ok = (labels >= 0) & (labels < K)
    out = np.full(len(labels), np.nan, p.dtype)
    out[ok] = p[np.flatnonzero(ok), labels[ok]]
    return out


def pick(labels, K, conf=None, chunks=None):
    """The reference's scan in data-set order over the rows of `chunks` — a list of (row0, n), any order; default: one chunk of all
    rows: conf None ("first"): the lowest row of every class; else ("best") the strict `conf > best_conf[idx]` of :143, so a tie goes
    to the lower row.  A row whose label is outside [0, K) or whose confidence is not finite is skipped.  -> (rows [K] int64, ABSENT
    for a class without a row; conf [K] float64, 0 in "first" mode and for an absent class).  The result is the per-class maximum of
    (conf, -row), so the order of the chunks cannot matter; the scan below visits them as given to show it."""
    labels = np.asarray(labels)
    rows, best = np.full(K, ABSENT, np.int64), np.full(K, -1.0)
    for r0, n in (chunks if chunks is not None else [(0, len(labels))]):
        for i in range(r0, r0 + n):
            k = int(labels[i])
            if not 0 <= k < K:
                continue
            if conf is None:
                if rows[k] == ABSENT or i < rows[k]:
                    rows[k] = i
                continue
            c = float(conf[i])
            if not np.isfinite(c):
                continue
            if c > best[k] or (c == best[k] and i < rows[k]):          # the second clause only fires when chunks come out of order
                rows[k], best[k] = i, c
    return rows, np.where(rows == ABSENT, 0.0, np.maximum(best, 0.0)) if conf is not None else np.zeros(K)


def scan_end(labels, K):
    """The number of rows the reference's loop visits: its `break` (:148-149) fires at the row that completes the set of classes
    (in "best" mode too: the statement stands after the if / else).  All rows when a class is absent."""
    first, _ = pick(labels, K)
    return len(labels) if (first == ABSENT).any() else int(first.max()) + 1


def to_unit(x):
    """(x + 1.0) / 2.0 in fp32, one rounding per operation (:175, :190; gr.py:370-371)."""
    x = np.asarray(x, np.float32)
    return (x + np.float32(1.0)) / np.float32(2.0)


def to_u8(v):
    """min(255, max(0, floor(v * 255 + 0.5))) in fp32: torchvision's save_image (mul(255).add_(0.5).clamp_(0, 255).to(uint8))."""
    v = np.asarray(v, np.float32)
    return np.minimum(np.float32(255), np.maximum(np.float32(0), np.floor(v * np.float32(255) + np.float32(0.5)))).astype(np.uint8)


def grid_image(sources, x_cf):
    """sources [K][H][W], x_cf [T][K][H][W] ([target][row]) in [-1, 1] -> the [K*H][T*W] fp32 image: cell (r, c) = to_unit(x_cf[c][r]),
    the diagonal to_unit(sources[r]); and the same image as uint8."""
    sources, x_cf = np.asarray(sources, np.float32), np.asarray(x_cf, np.float32)
    K, H, W = sources.shape
    T = x_cf.shape[0]
    img = np.zeros((K * H, T * W), np.float32)
    for r in range(K):
        for c in range(T):
            img[r * H:(r + 1) * H, c * W:(c + 1) * W] = to_unit(sources[r] if r == c else x_cf[c, r])
    return img, to_u8(img)


def panels(x, x_cf, mask):
    """x, x_cf [n][H][W] in [-1, 1], mask [H][W] or [n][H][W] -> ([n][4][H][W] fp32: xv, cv, |cv - xv| from the two rounded values,
    mask; vmax, the maximum of the third panel) (gr.py:370-372, :399)."""
    xv, cv = to_unit(x), to_unit(x_cf)
    d = np.abs(cv - xv)
    m = np.broadcast_to(np.asarray(mask, np.float32), xv.shape)
    return np.stack([xv, cv, d, m], axis=1), np.float32(d.max())


def delta_grid(G, Csd, X, Y, best, dtype, full_scan=False):
    """The grid of an additive-delta generator in `dtype`: the pick over (X [N,1,28,28], Y [N]) — in "best" mode from the restated
    max-pool classifier's softmax, over the rows the reference's scan reaches unless full_scan — then one query per cell.
    -> dict(rows [K], x_cf [T][K][1][28][28], probs [T][K][10], preds, confs [T][K])."""
    import delta_cf_restate as CR
    import pool_clf_restate as PR
    X = X.to(dtype)
    K = CR.K
    conf = None
    if best:
        with torch.no_grad():
            p = torch.softmax(PR.forward(Csd, X)["logits"], dim=1).numpy()
        conf = p[np.arange(len(Y)), np.asarray(Y)]
        n = len(Y) if full_scan else scan_end(np.asarray(Y), K)
        rows, _ = pick(np.asarray(Y)[:n], K, conf[:n])
    else:
        rows, _ = pick(np.asarray(Y), K)
    sw = CR.sweep(G, Csd, X[torch.as_tensor(rows)])
    return {"rows": rows, "x_cf": sw["x_cf"].numpy(), "probs": sw["probs"].numpy(), "preds": sw["preds"].numpy(), "confs": sw["confs"].numpy()}
