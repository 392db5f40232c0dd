#!/usr/bin/env python3
"""The house-sales classifier pre-training (house_sales_kc_usa/trainer.py:18-180) on one MI355X: the fused path
(house.train_classifier(fused=True): ClassifierFit, one graph replay + one AdamW launch per step) against the op
chain (fused=False, the default and the baseline) and eager PyTorch.

  python scripts/bench_house_clf_fit.py [--epochs 10] [--rounds 5] [--rows 17290] [--out profiles/house_clf_fit_bench_line.json]

One process, one GPU.  Synthetic 17-column data at the reference's size: 17 290 rows, which the trainer's stratified 10 % split
turns into 15 561 training rows (121 batches of 128 and a tail of 73) and 1 729 validation rows.  A fixed number of epochs, early
stopping disabled.  Every leg is run once untimed, then `--rounds` alternating rounds (fused, chain, eager, fused, ...) of
device-synchronised wall time around the whole fit: median and min..max per leg, and the same per step (train batches only in the
divisor; the validation pass is inside the time).  The per-step library calls of both paths are counted through ops.check, as
tests/test_hip_moons_clf_fit.py::test_launch_count counts them.  One JSON line (scripts/_benchlib.py: emit), also written to `--out`."""
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


def spread(v, digits=3):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def synthetic(n, seed=0):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 4, size=n)
    centers = rs.random_sample((4, 17))
    return np.clip(centers[y] + 0.25 * rs.standard_normal((n, 17)), 0, 1), y


def eager_fit(X, y, cfg, dev):
    """The reference's loop in eager PyTorch on the GPU: nn.Sequential, nn.CrossEntropyLoss(weight), torch.optim.AdamW, DataLoader."""
    from sklearn.model_selection import train_test_split
    from sklearn.utils.class_weight import compute_class_weight
    from torch.utils.data import DataLoader, TensorDataset
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"])
    Xt, Xv, yt, yv = train_test_split(X, y, test_size=0.10, random_state=cfg["seed"], stratify=y)
    mk = lambda a, b: TensorDataset(torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.long))      # noqa: E731
    tl = DataLoader(mk(Xt, yt), batch_size=cfg["batch_size"], shuffle=True)
    vl = DataLoader(mk(Xv, yv), batch_size=cfg["batch_size"], shuffle=False)
    net = nn.Sequential(nn.Linear(17, 256), nn.LeakyReLU(0.1), nn.BatchNorm1d(256), nn.Dropout(0.3),
                        nn.Linear(256, 256), nn.LeakyReLU(0.1), nn.BatchNorm1d(256), nn.Dropout(0.2),
                        nn.Linear(256, 128), nn.LeakyReLU(0.1), nn.BatchNorm1d(128), nn.Dropout(0.1),
                        nn.Linear(128, 64), nn.LeakyReLU(0.1), nn.BatchNorm1d(64), nn.Linear(64, 4)).to(dev)
    cw = torch.tensor(compute_class_weight("balanced", classes=np.arange(4), y=yt), dtype=torch.float32, device=dev)
    crit = nn.CrossEntropyLoss(weight=cw)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
    hist = []
    for _ in range(cfg["clf_epochs"]):
        net.train()
        rl, c, n = 0.0, 0, 0
        for xb, yb in tl:
            xb, yb = xb.to(dev), yb.to(dev)
            opt.zero_grad()
            out = net(xb)
            loss = crit(out, yb)
            loss.backward(); opt.step()
            rl += loss.item() * xb.size(0); c += (out.argmax(1) == yb).sum().item(); n += xb.size(0)
        net.eval()
        vl_, vc, vn = 0.0, 0, 0
        with torch.no_grad():
            for xb, yb in vl:
                xb, yb = xb.to(dev), yb.to(dev)
                out = net(xb)
                vl_ += crit(out, yb).item() * xb.size(0); vc += (out.argmax(1) == yb).sum().item(); vn += xb.size(0)
        hist.append((rl / n, c / n, vl_ / vn, vc / vn))
    return hist


def calls_per_step(H, ops, dev):
    """Library calls (ops.check) of one training step of either path on a 128-row batch."""
    calls = []
    real = ops.check
    ops.check = lambda rc, what="": (calls.append(what), real(rc, what))[1]
    try:
        X, y = synthetic(256, seed=3)
        cw = torch.ones(4, device=dev)
        fit = H.ClassifierFit(H.NNClassifier(17, 4).to(dev), X, y, cw, 128, graph=False)
        fit.new_epoch(torch.arange(256)); fit.step()
        del calls[:]
        fit.step()                                              # the second step: no first-use fills
        fused = list(calls)
        from pcgan_amd.optim import AdamW
        model = H.NNClassifier(17, 4).to(dev).train()
        crit, opt = H.WeightedCrossEntropyLoss(cw), AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        xb, yb = torch.tensor(X[:128], dtype=torch.float32), torch.tensor(y[:128])
        for i in range(2):                                      # the loop body of train_classifier (trainer.py:78-91)
            del calls[:]
            xd, yd = xb.to(dev), yb.to(dev)
            opt.zero_grad()
            logits = model(xd)
            loss = crit(logits, yd)
            loss.backward(); opt.step()
            loss.item(); ops.cf_metrics(logits.detach().contiguous(), yd, other=yd)[0].item()
        chain = list(calls)
    finally:
        ops.check = real
    return {"fused": len(fused), "op_chain": len(chain), "fused_by_entry": {w: fused.count(w) for w in sorted(set(fused))},
            "op_chain_by_entry": {w: chain.count(w) for w in sorted(set(chain))},
            "note": "the fused step's calls are captured once; a replayed step is one graph launch and pcg_adam_step_capturable"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=17290)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "house_clf_fit_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import house as H
    pcgan_amd.load()
    ops = pcgan_amd.ops
    dev = torch.device("cuda:0")
    X, y = synthetic(args.rows)
    cfg = dict(H.CONFIG, clf_epochs=args.epochs, clf_early_stopping=10 ** 9, batch_size=128, seed=42)
    n_train = args.rows - int(np.ceil(args.rows * 0.10))
    steps = args.epochs * ((n_train + 127) // 128)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    legs = {
        "fused": lambda: H.train_classifier(X, None, y, None, None, cfg, device=dev, verbose=False, fused=True).history,
        "op_chain": lambda: H.train_classifier(X, None, y, None, None, cfg, device=dev, verbose=False, fused=False).history,
        "eager": lambda: eager_fit(X, y, cfg, dev),
    }
    warm = dict(cfg, clf_epochs=1)
    H.train_classifier(X, None, y, None, None, warm, device=dev, verbose=False, fused=True)      # every leg once, untimed
    H.train_classifier(X, None, y, None, None, warm, device=dev, verbose=False, fused=False)
    eager_fit(X, y, warm, dev)
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
        "metric": f"classifier pre-training, house-sales CounteRGAN (trainer.py:18-180), {args.epochs} epochs of {n_train} rows at batch 128, "
                  "fused path",
        "value": f["median"], "unit": "ms", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "fit_ms": {"fused": f, "op_chain": c, "eager": e},
        "us_per_step": {k: spread([v * 1e3 / steps for v in ms[k]], 1) for k in legs},
        "train_steps": steps, "epochs": args.epochs, "rounds": args.rounds, "train_rows": n_train, "val_rows": args.rows - n_train,
        "fused_vs_op_chain": round(c["median"] / f["median"], 2), "fused_vs_eager": round(e["median"] / f["median"], 2),
        "fused_slowest_round_below_op_chain_fastest": bool(f["max"] < c["min"]),
        "library_calls_per_step": calls_per_step(H, ops, dev),
        "last_epoch": {k: [round(float(v), 4) for v in h[-1]] for k, h in hist.items()},
        "config": {"workload": "NNClassifier 17-256-256-128-64-4 (Linear, LeakyReLU(0.1), BatchNorm1d, Dropout), weighted cross-entropy, "
                               "AdamW(1e-3, 1e-4), ReduceLROnPlateau, one validation pass per epoch", "parallelism": "dp1"},
        "roofline": {"bound": "launch latency", "kernel": "16 whole-batch launches per step as one linear HIP graph + AdamW (csrc/dense_rows.hip)"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


if __name__ == "__main__":
    main()
