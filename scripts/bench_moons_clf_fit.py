#!/usr/bin/env python3
"""The moons CounteRGAN's classifier fit (conditional_counteRGAN/moons/trainer.py:22-25, 1000 full-batch Adam steps) on one MI355X:
the one-launch path against the op chain and eager PyTorch.

  python scripts/bench_moons_clf_fit.py [--steps 1000] [--rounds 5] [--rows 960 4096] [--out profiles/moons_clf_fit_bench_line.json]

Legs, all in this process on one GPU, per row count, in alternating rounds (`--rounds` times: one launch, chain, eager, ...):
  one_launch  moons_countergan.fit_classifier (upload, one pcg_moons_clf_fit launch, the read of the correct count)
  op_chain    moons_countergan._fit_classifier, unchanged: HipSequential under autograd, CrossEntropyLoss, zero_grad, Adam — the
              default path and the baseline
  eager       the same loop in eager PyTorch on the GPU (torch.nn, torch.optim.Adam)
and the bare kernel per step from device events around launches of `--steps` steps.  At 960 rows the data are the reference's own
training split; at 4096 rows they are the same recipe drawn larger (load_and_preprocess keeps its 1200 points).  Median and
min..max of the rounds per leg.  One JSON line (scripts/_benchlib.py: emit), also written to `--out`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import _benchlib  # noqa: E402


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def rows_of(M, n):
    X_train, _, y_train, _ = M.load_and_preprocess(42)
    if n <= len(X_train):
        return X_train[:n].astype(np.float32), y_train[:n]
    idx = np.random.RandomState(0).randint(0, len(X_train), n)
    X = X_train[idx] + np.random.RandomState(1).normal(scale=0.01, size=(n, 2))
    return X.astype(np.float32), y_train[idx]


def eager_fit(X, y, steps, dev):
    net = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    loss_fn = nn.CrossEntropyLoss()
    X_t, y_t = torch.tensor(X, dtype=torch.float32).to(dev), torch.tensor(y, dtype=torch.long).to(dev)
    for _ in range(steps):
        loss = loss_fn(net(X_t), y_t)
        opt.zero_grad(); loss.backward(); opt.step()
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[960, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moons_clf_fit_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import moons_countergan as M
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    if args.steps != 1000:
        print("note: the op chain always runs its 1000 steps; per-step figures stay comparable", file=sys.stderr)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def fresh():
        torch.manual_seed(0)
        return M.NNClassifier(2).to(dev)

    results = {}
    for n in args.rows:
        X, y = rows_of(M, n)
        legs = {
            "one_launch": (lambda: M.fit_classifier(fresh(), X, y, steps=args.steps), args.steps),
            "op_chain": (lambda: M._fit_classifier(fresh(), X, y, dev), 1000),
            "eager": (lambda: eager_fit(X, y, args.steps, dev), args.steps),
        }
        fit0 = M.ClassifierFit(fresh(), X, y)
        fit0.run(10)
        M._fit_classifier(fresh(), X, y, dev)                  # warm-up of every leg (allocator, first-launch costs)
        eager_fit(X, y, 20, dev)
        ms, us = {k: [] for k in legs}, {k: [] for k in legs}
        out = None
        for _ in range(args.rounds):
            for k, (fn, steps) in legs.items():
                sec, res = timed(fn)
                ms[k].append(sec * 1e3)
                us[k].append(sec * 1e6 / steps)
                if k == "one_launch":
                    out = res
        # the bare kernel: device events around launches of `steps` steps
        fit = M.ClassifierFit(fresh(), X, y)
        fit.run(args.steps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_launch = 5
        e0.record()
        for _ in range(n_launch):
            fit.run(args.steps)
        e1.record()
        torch.cuda.synchronize()
        kernel_us = e0.elapsed_time(e1) * 1e3 / (n_launch * args.steps)
        losses = out["losses"].cpu().numpy()
        if not np.isfinite(losses).all():
            sys.exit(f"non-finite losses at {n} rows")
        f, c, e = (spread(ms[k]) for k in ("one_launch", "op_chain", "eager"))
        results[str(n)] = {
            "fit_ms": {"one_launch": f, "op_chain": c, "eager": e},
            "us_per_step": {k: spread(v) for k, v in us.items()},
            "kernel_us_per_step": round(kernel_us, 2),
            "one_launch_vs_op_chain": round(c["median"] / f["median"], 2), "one_launch_vs_eager": round(e["median"] / f["median"], 2),
            "faster_than_op_chain_by_more_than_the_spread": bool(f["max"] < c["min"]),
            "train_accuracy": round(out["train_correct"] / n, 4), "final_loss": float(losses[-1]),
        }
    first = results[str(args.rows[0])]
    line = {
        "metric": f"classifier fit, moons CounteRGAN (trainer.py:22-25), {args.steps} steps, {args.rows[0]} rows, one launch",
        "value": first["fit_ms"]["one_launch"]["median"], "unit": "ms", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "rows": results, "steps": args.steps, "rounds": args.rounds,
        "config": {"workload": "Linear(2,32)-ReLU-Linear(32,32)-ReLU-Linear(32,3), full-batch cross-entropy, Adam(1e-2)", "parallelism": "dp1"},
        "roofline": {"bound": "vector ALU of one CU", "kernel": "one workgroup runs every step (csrc/moons_clf.hip)"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


if __name__ == "__main__":
    main()
