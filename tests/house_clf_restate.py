"""Restatement of one training step of the house-sales classifier (house_sales_kc_usa/models/nn_classifier.py:8-32 in training mode,
trainer.py:55-57,78-91) stage by stage, with the backward written out by hand: the reference of tests/test_hip_house_clf_fit.py for
the fused stage kernels (pcg_dense_rows_fwd_post / _dgrad_post) and the tally (pcg_ce_weighted_tally).  Plain torch on the CPU, in
whatever dtype its inputs have: float64 is the truth, float32 the yardstick of what fp32 arithmetic in another order gives.
tests/test_house_clf_fit_host.py pins it to the oracle's autograd step."""
import torch

SLOPE, EPS, MOMENTUM = 0.1, 1e-5, 0.1
DROPOUT = (0.3, 0.2, 0.1, None)
DIMS = (17, 256, 256, 128, 64, 4)


def stage_fwd(x, W, b, gamma, beta, mask=None, p=0.0, slope=SLOPE, eps=EPS):
    """Linear -> LeakyReLU -> BatchNorm1d (batch statistics) -> Dropout.  Returns y, a (the saved activation), mean, invstd, the
    unbiased variance (for the running statistics)."""
    z = x @ W.T + b
    a = torch.where(z > 0, z, slope * z)
    mean, var = a.mean(0), a.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    n = (a - mean) * invstd * gamma + beta
    y = n * mask.to(n.dtype) / (1.0 - p) if mask is not None else n
    return y, a, mean, invstd, a.var(0, unbiased=True)


def stage_bwd(g, a, mean, invstd, gamma, mask=None, p=0.0, slope=SLOPE):
    """g: the gradient with respect to the stage's output.  Returns (dz, dgamma, dbeta): Dropout', BatchNorm1d', LeakyReLU'."""
    R = a.shape[0]
    dn = g * mask.to(g.dtype) / (1.0 - p) if mask is not None else g
    xh = (a - mean) * invstd
    dbeta, dgamma = dn.sum(0), (dn * xh).sum(0)
    da = gamma * invstd * (dn - dbeta / R - xh * dgamma / R)
    return da * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope)), dgamma, dbeta


def ce_segment(logits, y, w):
    """nn.CrossEntropyLoss(weight=w) on one batch: (loss, dlogits, rows whose first maximum is the target)."""
    lse = torch.logsumexp(logits, 1)
    wt = w[y]
    nll = lse - logits.gather(1, y[:, None])[:, 0]
    wsum = wt.sum()
    onehot = torch.zeros_like(logits).scatter_(1, y[:, None], 1.0)
    dl = wt[:, None] * (torch.exp(logits - lse[:, None]) - onehot) / wsum
    return (wt * nll).sum() / wsum, dl, int((logits.argmax(1) == y).sum())


def ce_tally(logits, y, w, seg):
    """(sum_s L_s n_s, correct rows, rows) over runs of seg rows, and the L_s: trainer.py:89-91 / :110-112."""
    tot, hits, losses = 0.0, 0, []
    for s0 in range(0, logits.shape[0], seg):
        L, _, h = ce_segment(logits[s0:s0 + seg], y[s0:s0 + seg], w)
        n = min(seg, logits.shape[0] - s0)
        losses.append(float(L)); tot += float(L) * n; hits += h
    return (tot, hits, logits.shape[0]), losses


def train_grads(sd, x, y, masks, cw):
    """Loss and every parameter gradient of one step from state_dict `sd` (keys of NNClassifier: net.0.weight, ...), Dropout masks
    supplied.  Returns (loss, {name: grad}, {running statistics after the step})."""
    lin, bn = (0, 4, 8, 12, 15), (2, 6, 10, 14)
    h, saved, run = x, [], {}
    for s in range(4):
        W, b, g_, be = sd[f"net.{lin[s]}.weight"], sd[f"net.{lin[s]}.bias"], sd[f"net.{bn[s]}.weight"], sd[f"net.{bn[s]}.bias"]
        m, p = (masks[s], DROPOUT[s]) if DROPOUT[s] is not None else (None, 0.0)
        y_, a, mean, invstd, var_u = stage_fwd(h, W, b, g_, be, m, p)
        run[f"net.{bn[s]}.running_mean"] = (1 - MOMENTUM) * sd[f"net.{bn[s]}.running_mean"] + MOMENTUM * mean
        run[f"net.{bn[s]}.running_var"] = (1 - MOMENTUM) * sd[f"net.{bn[s]}.running_var"] + MOMENTUM * var_u
        saved.append((h, a, mean, invstd, g_, m, p))
        h = y_
    logits = h @ sd["net.15.weight"].T + sd["net.15.bias"]
    loss, d, _ = ce_segment(logits, y, cw)
    grads = {"net.15.weight": d.T @ h, "net.15.bias": d.sum(0)}
    upper = sd["net.15.weight"]
    for s in range(3, -1, -1):
        hin, a, mean, invstd, g_, m, p = saved[s]
        d, dgamma, dbeta = stage_bwd(d @ upper, a, mean, invstd, g_, m, p)
        grads[f"net.{bn[s]}.weight"], grads[f"net.{bn[s]}.bias"] = dgamma, dbeta
        grads[f"net.{lin[s]}.weight"], grads[f"net.{lin[s]}.bias"] = d.T @ hin, d.sum(0)
        upper = sd[f"net.{lin[s]}.weight"]
    return float(loss), grads, run
