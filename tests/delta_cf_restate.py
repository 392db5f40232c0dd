"""Restatement of the prompted half of the additive-delta MNIST CounteRGAN (conditional_counteRGAN/mnist/gan_train_copy.py) in plain
torch on the CPU, in whatever dtype it is given: the query of :164-172, the all-targets sweep, the per-target metrics of
mnist/eval_utils.py:58-66 folded as :97-102 folds them, and the random-target iteration of :119-146.  float64 is the truth, float32 the
yardstick.  The nets, the classifier and the batches are tests/delta_gan_restate.py's; tests/test_delta_cf_host.py pins this file to the
reference's own recorded runs (tests/golden/delta_cf_ref.npz, written by tests/golden/make_golden_delta_cf.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_gan_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

K = 10
SEED_DRAW = 11                                         # torch.manual_seed before the training loop: the classes of :119
SEED_QUERY = 13                                        # torch.manual_seed before :162: the random target per image
LAMBDA_CLS, LAMBDA_REG, LR_G, LR_D = 2.0, 0.01, 5e-5, 1e-5      # gan_train_copy.py:21-25
LOSSES = RS.LOSSES
METRICS = ("class_flip_rate", "prediction_gain", "actionability", "mean_abs_delta", "l2")
NEAR_CAP = 0.05                                        # at most 5 % of the queries may be near (see near_set)


def drawn_classes(steps, seed=SEED_DRAW):
    """The classes :119 draws in `steps` iterations after torch.manual_seed(seed) (nothing else in the loop draws: no dropout)."""
    torch.manual_seed(seed)
    return [int(torch.randint(0, 10, (1,)).item()) for _ in range(steps)]


def query_targets(B, seed=SEED_QUERY):
    """:162 after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    return torch.randint(0, 10, (B,))


def query(G, Csd, imgs, targets):
    """:164-172 in the dtype of the nets: x_cf (clamped), delta, probs, preds, confs."""
    with torch.no_grad():
        cf, delta = G(imgs, targets)
        cf = torch.clamp(cf, -1, 1)
        probs = torch.softmax(PR.forward(Csd, cf)["logits"], dim=1)
        preds = torch.argmax(probs, dim=1)
        confs = probs[torch.arange(len(preds)), preds]
    return {"x_cf": cf, "delta": delta, "probs": probs, "preds": preds, "confs": confs}


def sweep(G, Csd, imgs):
    """query() for every target class of every row: each value stacked to [T, B, ...]."""
    B = imgs.shape[0]
    per = [query(G, Csd, imgs, torch.full((B,), t, dtype=torch.int64)) for t in range(K)]
    return {k: torch.stack([p[k] for p in per]) for k in per[0]}


def query_sums(x, x_cf, delta):
    """[..., 3] per query: sum |x_cf - x|, sum |delta|, sum (x_cf - x)^2 over the pixels (x broadcasts over a leading target axis)."""
    c = x_cf - x
    flat = lambda t: t.reshape(*t.shape[:-3], -1)      # noqa: E731
    return torch.stack([flat(c.abs()).sum(-1), flat(delta.abs()).sum(-1), flat(c * c).sum(-1)], dim=-1)


def per_target_metrics(x, y, sw):
    """One batch, every target: {metric: float64 [T]}.  class_flip_rate, prediction_gain, actionability as eval_utils.py:58-66;
    mean_abs_delta = mean |delta|; l2 = sqrt(mean over the rows of sum_pixels (x_cf - x)^2)."""
    B = x.shape[0]
    rows = torch.arange(B)
    out = {k: [] for k in METRICS}
    for t in range(K):
        probs, preds, x_cf, delta = sw["probs"][t].double(), sw["preds"][t], sw["x_cf"][t].double(), sw["delta"][t].double()
        out["class_flip_rate"].append(float((preds == t).double().mean()))
        out["prediction_gain"].append(float((probs[rows, t] - probs[rows, y]).mean()))
        out["actionability"].append(float((x_cf - x.double()).abs().mean()))
        out["mean_abs_delta"].append(float(delta.abs().mean()))
        out["l2"].append(float(((x_cf - x.double()) ** 2).reshape(B, -1).sum(1).mean().sqrt()))
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def fold(per_batch):
    """eval_utils.py:97-102: per target the mean over the batches of the per-batch means (a ragged last batch weighs as much as a
    full one)."""
    return {k: np.mean(np.stack([m[k] for m in per_batch]), axis=0) for k in METRICS}


def near_set(p32, p64):
    """The queries whose discrete outputs fp32 and float64 need not agree on: float64 top-two probability gap below
    max(1e-6, 100 * max|p_fp32 - p_fp64|).  -> (near [..] bool, gap, bound)."""
    top = torch.sort(p64, dim=-1).values
    gap = top[..., -1] - top[..., -2]
    bound = max(1e-6, 100.0 * float((p32.double() - p64).abs().max()))
    return gap < bound, gap, bound


def run_random_target(B, dtype, steps=3, classes=None):
    """The recorded training run: seeded nets and classifier, `steps` iterations of :119-146 on RS.batches(B) with the drawn classes.
    -> (classes, per-step results of RS.iteration, G, D)."""
    G, D = RS.seeded_nets(dtype)
    Csd = RS.classifier_state(dtype)
    opt_g, opt_d = torch.optim.Adam(G.parameters(), lr=LR_G), torch.optim.Adam(D.parameters(), lr=LR_D)
    classes = drawn_classes(steps) if classes is None else list(classes)
    res = []
    for (x, y), c in zip(RS.batches(B, steps), classes):
        res.append(RS.iteration(G, D, Csd, opt_g, opt_d, x.to(dtype), y, torch.full_like(y, c), LAMBDA_CLS, LAMBDA_REG))
    return classes, res, G, D


def recorded_queries(B, dtype):
    """The recorded queries on the seeded (untrained) nets: batch 0 of RS.batches(B), the random targets of :162 and the full sweep."""
    G, _ = RS.seeded_nets(dtype)
    Csd = RS.classifier_state(dtype)
    x, y = RS.batches(B)[0]
    x = x.to(dtype)
    return x, y, query(G, Csd, x, query_targets(B)), sweep(G, Csd, x)
