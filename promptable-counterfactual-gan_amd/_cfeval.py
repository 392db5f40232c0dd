"""What the counterfactual-evaluation front ends share on the host side (moons_countergan over csrc/moons_cf_eval.hip, house over
csrc/house_cf_eval.hip, and the CSV text of countergan's classifier evaluation): the argument guards that run before anything touches
the GPU, the fold of the kernels' group sums into the reference's metric table, the CSV writers and the grayscale PNG writer of the
counterfactual grid.  Pure host code: nothing here loads the library.  Where the ports differ, the difference is a keyword."""
import math
import os

import numpy as np
import torch

from ._epoch import one_gpu  # noqa: F401  (the "all nets on one GPU" rule of the evaluation calls is the trainers')
from ._lib import PcgError


# ---- argument guards ------------------------------------------------------------------------------------------------------------------
def rows_arg(x, D, what="x", floats_only=False, detach=False):
    """[N][D] rows, a tensor or an ndarray (taken as float32): the shape is checked on the host.  floats_only: a tensor of another
    dtype is refused; detach: a tensor is cut from its graph (the call runs without autograd whatever it is given).  Returns
    (rows, given as a tensor)."""
    given = torch.is_tensor(x)
    if not given:
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    bad_shape = x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1
    if floats_only and (bad_shape or not x.dtype.is_floating_point):
        raise PcgError(f"{what} must be [N][{D}] floats with N >= 1, got {tuple(x.shape)} {x.dtype}")
    if bad_shape:
        raise PcgError(f"{what} must be [N][{D}] with N >= 1, got {tuple(x.shape)}")
    return (x.detach() if detach else x), given


def targets_arg(target, N, K, refuse_bool=False):
    """The target class of N queries, an int (every row) or [N] integers -> int64 [N].  It selects the one-hot input of the generator,
    so its range [0, K) is checked here, on the host.  refuse_bool: a Python bool is no int."""
    if isinstance(target, (int, np.integer)) and not (refuse_bool and isinstance(target, bool)):
        target = torch.full((N,), int(target), dtype=torch.int64)
    else:
        target = target.detach() if torch.is_tensor(target) else torch.as_tensor(np.asarray(target))
        if tuple(target.shape) != (N,) or target.dtype.is_floating_point or target.dtype == torch.bool:
            raise PcgError(f"target must be an int or [N] integers (N = {N}), got {tuple(target.shape)} {target.dtype}")
    lo, hi = int(target.min()), int(target.max())
    if lo < 0 or hi >= K:
        raise PcgError(f"targets must lie in [0, {K}), got [{lo}, {hi}]")
    return target.to(torch.int64)


def labels_arg(y, N):
    """The rows' own classes, [N] integers, or None (every row counts): None stays None."""
    if y is None:
        return None
    y = y.detach() if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))
    if tuple(y.shape) != (N,) or y.dtype.is_floating_point:
        raise PcgError(f"y must be [N] integers (N = {N}), got {tuple(y.shape)} {y.dtype}")
    return y


def check_outputs(outputs, allowed):
    bad = [o for o in outputs if o not in allowed]
    if bad:
        raise PcgError(f"outputs {bad} are not among {allowed}")


def upload(t, dev, dtype=torch.float32):
    return t.to(dev, dtype).contiguous()


# ---- the kernels' group sums -> the reference's metric table ---------------------------------------------------------------------------
def batch_mean_metrics(group_sums, D):
    """group_sums [..., n_groups, 4] (included rows, rows with pred_cf == target, sum of gain, sum of |masked residual| over the D
    columns) -> [..., 3] (class_flip, prediction_gain, avg_actionability) in float64, as the reference's eval loops form them: per
    group with a row in it the mean over its rows (actionability over all columns: / (D count)), then np.mean over those groups — the
    mean of the per-batch means, so rows of a short batch weigh more.  No such group: nan."""
    s = np.asarray(group_sums, dtype=np.float64)
    out = np.full(s.shape[:-2] + (3,), np.nan)
    for idx in np.ndindex(*s.shape[:-2]):
        g = s[idx]
        g = g[g[:, 0] > 0]
        if len(g):
            out[idx] = (np.mean(g[:, 1] / g[:, 0]), np.mean(g[:, 2] / g[:, 0]), np.mean(g[:, 3] / (D * g[:, 0])))
    return out


METRIC_FIELDS = ("class_flip", "prediction_gain", "avg_actionability")    # the columns of batch_mean_metrics


def metric_rows(table, fields=METRIC_FIELDS):
    """[T targets][len(fields)] -> the rows of the reference's DataFrame as a list of dicts."""
    return [dict({"target_class": t}, **{k: float(v) for k, v in zip(fields, row)}) for t, row in enumerate(table)]


# ---- confusion matrix and CSV text ------------------------------------------------------------------------------------------------------
def confusion_matrix(y_true, y_pred):
    """sklearn.metrics.confusion_matrix(y_true, y_pred): labels = the sorted values that occur in either, rows true, columns predicted."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    labels = np.unique(np.concatenate([y_true, y_pred]))
    cm = np.zeros((len(labels), len(labels)), dtype=np.int64)
    np.add.at(cm, (np.searchsorted(labels, y_true), np.searchsorted(labels, y_pred)), 1)
    return cm


def confusion_csv(cm):
    """The text of the reference's confusion DataFrame.to_csv: a header of pred_j columns, one true_i row per class."""
    lines = ["," + ",".join(f"pred_{j}" for j in range(cm.shape[1]))]
    lines += [f"true_{i}," + ",".join(str(int(v)) for v in row) for i, row in enumerate(cm)]
    return "\n".join(lines) + "\n"


def csv_value(v):
    return "" if isinstance(v, float) and math.isnan(v) else (repr(v) if isinstance(v, float) else str(v))


def write_png_gray(path, u8):
    """An [H][W] uint8 array as an 8-bit grayscale PNG (zlib + struct only): signature, IHDR, one IDAT of the rows each behind a
    filter byte 0, IEND."""
    import struct
    import zlib
    a = np.asarray(u8)
    if a.ndim != 2 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise PcgError(f"write_png_gray: expected a non-empty [H][W] uint8 array, got {a.shape} {a.dtype}")
    h, w = a.shape

    def block(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a], axis=1).tobytes()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + block(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + block(b"IDAT", zlib.compress(raw, 9)) +
                block(b"IEND", b""))


def write_png_rgb(path, u8):
    """An [H][W][3] uint8 array as an 8-bit RGB PNG (colour type 2), built like write_png_gray's: what the image sheets
    (pcgan_amd.sheets.save_image) write."""
    import struct
    import zlib
    a = np.asarray(u8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise PcgError(f"write_png_rgb: expected a non-empty [H][W][3] uint8 array, got {a.shape} {a.dtype}")
    h, w = a.shape[:2]

    def block(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, 3 * w)], axis=1).tobytes()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + block(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + block(b"IDAT", zlib.compress(raw, 9)) +
                block(b"IEND", b""))


def save_table(rows, save_path, columns):
    """DataFrame.to_csv(index=False) of a list of dicts: shortest float repr, nan as an empty field."""
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    with open(save_path, "w") as f:
        f.write(",".join(columns) + "\n")
        for r in rows:
            f.write(",".join(csv_value(r[c]) for c in columns) + "\n")
