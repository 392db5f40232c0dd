#!/usr/bin/env python3
"""The moons CounteRGAN's evaluation (conditional_counteRGAN/moons/eval_utils.py:29-106, four masks x three targets) and its decision
grid (:196-206) on one MI355X: the one-launch path against the per-batch paths.

  python scripts/bench_moons_cf_eval.py [--rounds 5] [--big-rounds 2] [--big 65536] [--hidden 32]

Legs, all in this process on one GPU, in alternating rounds after a warm-up of every leg:
  one_launch  moons_countergan.compute_metrics_per_target(mask=MASKS): ONE pcg_moons_cf_eval launch and one read of the group sums;
              wall clock to the host read, and the bare kernel by device events around single launches (median)
  forwards    the same metrics through the module forwards (pcg_moons_cf_forward: one generator and two classifier launches per
              batch), host row selection and the small ops for softmax / argmax / means, as the reference's loop does them
  eager       the same loop in eager PyTorch on the GPU (the nets restated here)
at two sizes: the reference's test split (240 rows) and --big rows drawn from a seeded generator, batch_size 64.  The decision grid
(200 x 200 points) the same way, one_launch against forwards (79 classifier launches).
One JSON line, the contract of scripts/bench_moons_cf.py.  The work is launch / latency bound: no MFMA or roofline claim."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BS = 64


def per_batch_metrics(gen, clf, X, y, masks, dev):
    """eval_utils.py:48-104 for every mask; gen(x, onehot, mask) -> masked residual, clf(x) -> logits (HIP modules or eager ones)."""
    X_t, y_t = torch.as_tensor(X, dtype=torch.float32), torch.as_tensor(y, dtype=torch.long)
    out = {}
    with torch.no_grad():
        for name, mv in masks.items():
            m = torch.tensor(mv, dtype=torch.float32, device=dev)
            rows = []
            for target in range(3):
                flips, gains, acts = [], [], []
                for i in range(0, len(X_t), BS):
                    xb, yb = X_t[i:i + BS].to(dev), y_t[i:i + BS].to(dev)
                    sel = yb != target
                    if sel.sum() == 0:
                        continue
                    x = xb[sel].contiguous()
                    bs = x.size(0)
                    tv = torch.full((bs,), target, device=dev, dtype=torch.long)
                    masked = gen(x, F.one_hot(tv, 3).float(), m.unsqueeze(0).expand(bs, -1).contiguous())
                    cf = (x + masked).contiguous()
                    cf_logits = clf(cf)
                    flips.append((cf_logits.argmax(1) == tv).float().mean().item())
                    ar = torch.arange(bs, device=dev)
                    gains.append((F.softmax(cf_logits, 1)[ar, tv] - F.softmax(clf(x), 1)[ar, tv]).mean().item())
                    acts.append(torch.mean(torch.abs(masked)).item())
                rows.append([float(np.mean(v)) if v else float("nan") for v in (flips, gains, acts)])
            out[name] = rows
    return np.array([out[n] for n in masks])


def eager_nets(M, G, C, H, dev):
    eG = nn.Sequential(nn.Linear(7, H), nn.BatchNorm1d(H), nn.ReLU(), nn.Linear(H, H), nn.BatchNorm1d(H), nn.ReLU(),
                       nn.Linear(H, H // 2), nn.BatchNorm1d(H // 2), nn.ReLU(), nn.Linear(H // 2, 2))
    eC = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3))
    eG.load_state_dict({k[4:]: v.detach().cpu() for k, v in G.state_dict().items()})
    eC.load_state_dict({k[4:]: v.detach().cpu() for k, v in C.state_dict().items()})
    return eG.to(dev).eval(), eC.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-rounds", type=int, default=2)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=32)
    args = ap.parse_args()
    import pcgan_amd
    from pcgan_amd import moons_countergan as M
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    H = args.hidden
    gold = os.path.join(ROOT, "tests", "golden")
    G, C = M.ResidualGenerator(2, H, 3), M.NNClassifier(2)
    C.load_state_dict(torch.load(os.path.join(gold, "moons_cf_classifier_trained.pt"), map_location="cpu"))
    if H == 32:
        G.load_state_dict(torch.load(os.path.join(gold, "moons_cf_generator_trained.pt"), map_location="cpu"))
    G.to(dev).eval(); C.to(dev).eval()
    for p in list(G.parameters()) + list(C.parameters()):
        p.requires_grad = False
    eG, eC = eager_nets(M, G, C, H, dev)
    _, X_test, _, y_test = M.load_and_preprocess(42)
    rng = np.random.default_rng(0)
    sizes = {"240": (X_test.astype(np.float32), np.asarray(y_test)),
             str(args.big): (rng.uniform(0.0, 1.0, (args.big, 2)).astype(np.float32), rng.integers(0, 3, args.big))}
    cfg = {"batch_size": BS, "cuda": str(dev)}

    legs = {
        "one_launch": lambda X, y: np.array([[[r[k] for k in M.METRIC_FIELDS] for r in rows] for rows in
                                             M.compute_metrics_per_target(G, C, X, y, cfg, mask=M.MASKS).values()]),
        "forwards": lambda X, y: per_batch_metrics(lambda x, oh, m: G(x, oh, m)[1], C, X, y, M.MASKS, dev),
        "eager": lambda X, y: per_batch_metrics(lambda x, oh, m: eG(torch.cat([x, oh, m], 1)) * m, eC, X, y, M.MASKS, dev),
    }
    result = {}
    for size, (X, y) in sizes.items():
        n = len(X)
        rounds = args.rounds if n <= 4096 else args.big_rounds
        warm = slice(0, min(n, 2048))
        ref = None
        for leg in legs.values():                                             # warm-up: every leg, the batch shapes of the timed run
            leg(X[warm], y[warm])
        secs = {k: [] for k in legs}
        for _ in range(rounds):
            for k, leg in legs.items():
                s, tab = timed(lambda: leg(X, y))
                secs[k].append(s)
                if ref is None:
                    ref = tab
                elif not np.allclose(tab, ref, rtol=1e-4, atol=1e-6, equal_nan=True):
                    sys.exit(f"{k} at {n} rows disagrees with one_launch: max difference {np.nanmax(np.abs(tab - ref)):.3e}")
        # the bare kernel: device events around single launches
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        ev = []
        with torch.no_grad():
            for i in range(25):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                M.counterfactual_sweep(G, C, Xd, yd, M.MASKS, BS)
                e1.record()
                torch.cuda.synchronize()
                if i >= 5:
                    ev.append(e0.elapsed_time(e1) * 1e3)
        batches = -(-n // BS)
        result[size] = {"rows": n, "rounds": rounds,
                        "ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in secs.items()},
                        "ms_all_rounds": {k: [round(s * 1e3, 3) for s in v] for k, v in secs.items()},
                        "kernel_us": round(float(np.median(ev)), 2),
                        "launches": {"one_launch": 1, "forwards": f"{3 * 12 * batches} (+ row selection and ~10 small ops per batch)",
                                     "eager": f"~{12 * batches} batches x ~40 kernels"},
                        "one_launch_vs_forwards": round(float(np.median(secs["forwards"]) / np.median(secs["one_launch"])), 2),
                        "one_launch_vs_eager": round(float(np.median(secs["eager"]) / np.median(secs["one_launch"])), 2)}

    # the decision grid
    def grid_forwards():
        X = np.asarray(X_test)
        xx, yy = np.meshgrid(np.linspace(X[:, 0].min() - 0.1, X[:, 0].max() + 0.1, 200), np.linspace(X[:, 1].min() - 0.1, X[:, 1].max() + 0.1, 200))
        with torch.no_grad():
            return C(torch.tensor(np.c_[xx.ravel(), yy.ravel()], dtype=torch.float32).to(dev)).argmax(1).cpu().numpy().reshape(xx.shape)

    grid_legs = {"one_launch": lambda: M.decision_regions(C, X_test)[2], "forwards": grid_forwards}
    for leg in grid_legs.values():
        leg()
    gsecs = {k: [] for k in grid_legs}
    Z = None
    for _ in range(args.rounds):
        for k, leg in grid_legs.items():
            s, z = timed(leg)
            gsecs[k].append(s)
            if Z is None:
                Z = z
            elif not np.array_equal(z, Z):
                sys.exit(f"decision grid: {k} disagrees with one_launch at {int((z != Z).sum())} points")
    result["grid"] = {"points": 40000, "ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in gsecs.items()},
                      "launches": {"one_launch": 1, "forwards": 79},
                      "one_launch_vs_forwards": round(float(np.median(gsecs["forwards"]) / np.median(gsecs["one_launch"])), 2)}

    small = result["240"]
    print(json.dumps({
        "metric": "four-mask evaluations/sec, moons CounteRGAN compute_metrics_per_target (eval_utils.py:29-106), 240 test rows, one launch; "
                  "launch/latency bound",
        "value": round(1e3 / small["ms"]["one_launch"], 1), "unit": "evaluations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "sizes": result,
        "config": {"workload": f"conditional_counteRGAN/moons eval_utils.py:29-106 and :196-206, hidden {H}, batch_size {BS}, 4 masks x 3 targets",
                   "parallelism": "dp1"},
        "roofline": {"bound": "launch/latency", "kernel": "one work item per (mask, target, row), weights staged in LDS (csrc/moons_cf_eval.hip)"},
    }))


if __name__ == "__main__":
    main()
