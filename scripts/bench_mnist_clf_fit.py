#!/usr/bin/env python3
"""The MNIST classifier pre-training (conditional_counteRGAN/mnist/trainer.py:8-39) on one MI355X: the fused path
(countergan.train_classifier(fused=True): ClassifierFit, one graph replay per step) against the op chain
(fused=False, the default and the baseline) and eager PyTorch.

  python scripts/bench_mnist_clf_fit.py [--epochs 2] [--rounds 5] [--rows 54000] [--out profiles/mnist_clf_fit_bench_line.json]

One process, one GPU.  Synthetic 28x28 digits (ten templates plus noise) at the reference's size: 54 000 training rows (421 batches
of 128 and a tail of 112) and 6 000 validation rows, both resident on the device (data.DeviceLoader).  Every leg is run once
untimed, then `--rounds` alternating rounds (fused, chain, eager, fused, ...) of device-synchronised wall time around the whole
fit: median and min..max per leg, and the same per step (train batches only in the divisor; the validation pass is inside the
time).  The per-step library calls of both paths are counted through ops.check, as tests/test_hip_mnist_clf_fit.py::test_launch_census
counts them.  One JSON line (scripts/_benchlib.py: emit), also written to `--out`."""
import argparse
import contextlib
import io
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


def spread(v, digits=3):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def synthetic(n, seed):
    y = np.random.RandomState(seed).randint(0, 10, n)
    t = np.kron(np.random.RandomState(0).choice([-1.0, 1.0], size=(10, 7, 7)), np.ones((4, 4))).astype(np.float32)
    x = np.clip(t[y] + 0.3 * np.random.RandomState(seed + 1).standard_normal((n, 28, 28)).astype(np.float32), -1, 1)
    return torch.from_numpy(x[:, None]), torch.from_numpy(y)


def eager_fit(train, valid, epochs, dev, seed):
    """The reference's loop in eager PyTorch on the GPU: nn.Sequential, nn.CrossEntropyLoss, torch.optim.Adam, the resident loaders."""
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(1, 32, 3, 1, 1), nn.ReLU(), nn.Conv2d(32, 64, 3, 2, 1), nn.ReLU(), nn.Conv2d(64, 128, 3, 2, 1), nn.ReLU(),
                        nn.Dropout2d(0.25), nn.Flatten(), nn.Linear(128 * 7 * 7, 256), nn.ReLU(), nn.Dropout(0.5), nn.Linear(256, 10)).to(dev)
    opt, crit, hist = torch.optim.Adam(net.parameters(), lr=1e-3), nn.CrossEntropyLoss(), []
    for _ in range(epochs):
        net.train()
        for x, y in train:
            opt.zero_grad()
            crit(net(x), y).backward()
            opt.step()
        net.eval()
        correct, total = 0, 0
        with torch.no_grad():
            for x, y in valid:
                correct += (net(x).argmax(1) == y).sum().item()
                total += y.size(0)
        hist.append(correct / total)
    return hist


def calls_per_step(K, ops, dev):
    """Library calls (ops.check) of one training step of either path on a 128-row batch."""
    calls = []
    real = ops.check
    ops.check = lambda rc, what="": (calls.append(what), real(rc, what))[1]
    try:
        x, y = synthetic(256, seed=3)
        x, y = x.to(dev), y.to(dev)
        fit = K.ClassifierFit(K.CNNClassifier().to(dev), x, y, 128, graph=False)
        fit.new_epoch(torch.arange(256)); fit.step()
        del calls[:]
        fit.step()                                              # the second step: no first-use fills
        fused = list(calls)
        from pcgan_amd.optim import Adam
        model = K.CNNClassifier().to(dev).train()
        crit, opt = K.CrossEntropyLoss(), Adam(model.parameters(), lr=1e-3)
        for i in range(2):                                      # the loop body of train_classifier (trainer.py:16-21)
            del calls[:]
            opt.zero_grad()
            loss = crit(model(x[:128]), y[:128])
            loss.backward(); opt.step()
        chain = list(calls)
    finally:
        ops.check = real
    return {"fused": len(fused), "op_chain": len(chain), "fused_by_entry": {w: fused.count(w) for w in sorted(set(fused))},
            "op_chain_by_entry": {w: chain.count(w) for w in sorted(set(chain))},
            "note": "the fused step's calls are captured once; a replayed step is one graph launch"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=54000)
    ap.add_argument("--val-rows", type=int, default=6000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnist_clf_fit_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import countergan as K
    from pcgan_amd.data import DeviceLoader
    pcgan_amd.load()
    ops = pcgan_amd.ops
    dev = torch.device("cuda:0")
    (xt, yt), (xv, yv) = synthetic(args.rows, 1), synthetic(args.val_rows, 7)
    xt, yt, xv, yv = xt.to(dev), yt.to(dev), xv.to(dev), yv.to(dev)
    steps = args.epochs * ((args.rows + 127) // 128)

    class Cfg:
        cls_lr, num_epochs_clf, classifier_path = 1e-3, args.epochs, None

    class Warm(Cfg):
        num_epochs_clf = 1

    def ours(cfg, fused):
        torch.manual_seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            return K.train_classifier(K.CNNClassifier().to(dev), DeviceLoader(xt, yt, 128, True, 3), DeviceLoader(xv, yv, 128, False), cfg, dev,
                                      save=False, fused=fused)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    legs = {
        "fused": lambda: ours(Cfg, True),
        "op_chain": lambda: ours(Cfg, False),
        "eager": lambda: eager_fit(DeviceLoader(xt, yt, 128, True, 3), DeviceLoader(xv, yv, 128, False), args.epochs, dev, 5),
    }
    ours(Warm, True); ours(Warm, False)                         # every leg once, untimed
    eager_fit(DeviceLoader(xt, yt, 128, True, 3), DeviceLoader(xv, yv, 128, False), 1, dev, 5)
    ms, hist = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            sec, hist[k] = timed(fn)
            ms[k].append(sec * 1e3)
    for k, h in hist.items():
        if len(h) != args.epochs or not np.isfinite(np.asarray(h)).all():
            sys.exit(f"{k}: bad history {h}")
    f, c, e = (spread(ms[k]) for k in ("fused", "op_chain", "eager"))
    line = {
        "metric": f"classifier pre-training, MNIST CounteRGAN (mnist/trainer.py:8-39), {args.epochs} epochs of {args.rows} rows at batch 128, "
                  "fused path",
        "value": f["median"], "unit": "ms", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "fit_ms": {"fused": f, "op_chain": c, "eager": e},
        "us_per_step": {k: spread([v * 1e3 / steps for v in ms[k]], 1) for k in legs},
        "train_steps": steps, "epochs": args.epochs, "rounds": args.rounds, "train_rows": args.rows, "val_rows": args.val_rows,
        "fused_vs_op_chain": round(c["median"] / f["median"], 2), "fused_vs_eager": round(e["median"] / f["median"], 2),
        "fused_slowest_round_below_op_chain_fastest": bool(f["max"] < c["min"]),
        "library_calls_per_step": calls_per_step(K, ops, dev),
        "last_epoch_val_acc": {k: round(float(h[-1]), 4) for k, h in hist.items()},
        "config": {"workload": "CNNClassifier 1-32-64-128 convs (3x3, ReLU), Dropout2d(0.25), 6272-256-10, Dropout(0.5), cross-entropy, "
                               "Adam(1e-3), one validation pass per epoch", "parallelism": "dp1"},
        "roofline": {"bound": "the kernels of the replayed step, the convolution and fc1 launches first (DESIGN.md §3.17), not launch latency",
                     "kernel": "one linear HIP graph per step: batch gather, 4 forward GEMMs, 2 flatten launches, the one-workgroup head, the "
                               "conv backwards, Adam (csrc/mnist_clf.hip)"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


if __name__ == "__main__":
    main()
