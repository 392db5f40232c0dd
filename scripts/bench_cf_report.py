#!/usr/bin/env python3
"""The evaluation reports' two passes, each against a loop built from the parent commit's own pieces, in ONE process,
in alternating rounds:

  python scripts/bench_cf_report.py [--rounds 3] [--rows 60000] [--chunk 2048] [--out profiles/cf_report_bench_line.json]

  pick   countergan.pick_sources(pick_best_source=True, full_scan=True) over --rows synthetic rows resident on the device: the
         classifier's padded logits per chunk, csrc/cf_report.hip's pcg_class_pick into one state, one host read of the 10 keys
    vs   the per-row loop of conditional_counteRGAN/mnist/eval_utils.py:139-144 without its early exit: one batch-1 classifier
         forward (countergan._padded_logits), the score kernel's own-label probability and one host read per row
  grid   countergan.counterfactual_grid: the pick ("first"), ONE sweep of the 10 sources over the 10 targets, the grid image
    vs   the same pick, then 90 single countergan.counterfactuals() calls with one read of (pred, conf) each (:170-195)

Seeded nets (the generator untrained: its weights do not change the work), scripts/bench_delta_gan.py's synthetic rows.  The legs
must agree on the picked rows wherever the loop's top two confidences of a class are more than 1e-5 apart.  Prints ONE JSON line with
the median, the spread and every round of each leg, and writes it to --out."""
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

import bench_delta_gan as BG  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf_report_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import countergan as K, ops
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    G = K.ResidualGenerator().to(dev).eval()
    torch.manual_seed(3)
    C = K.CNNClassifier().to(dev).eval()
    X, Y = BG.synthetic(args.rows, 1)
    X, Y = X.to(dev).contiguous(), Y.to(dev).contiguous()
    rows_x = X.view(args.rows, 784)
    y_host = Y.cpu().numpy()

    def pick_fused():
        _, rows, conf = K.pick_sources(C, (X, Y), pick_best_source=True, chunk=args.chunk, full_scan=True)
        return rows.cpu().numpy(), conf.cpu().numpy()

    def pick_loop():
        rows, best = np.full(10, -1, np.int64), np.full(10, -1.0)
        with torch.no_grad():
            for i in range(args.rows):
                k = int(y_host[i])
                conf = ops.mnist_cf_score(K._padded_logits(C, rows_x[i:i + 1]), 10, 1, 1, y_true=Y[i:i + 1], outputs=("p_true",),
                                          group_sums=False)["p_true"].item()
                if conf > best[k]:
                    rows[k], best[k] = i, conf
        return rows, best

    def grid_fused():
        g = K.counterfactual_grid(G, C, (X, Y), chunk=args.chunk)
        g["image_u8"].cpu()
        return g["pred"], g["conf"]

    def grid_loop():
        src, _, _ = K.pick_sources(C, (X, Y), chunk=args.chunk)
        pred, conf = np.zeros((10, 10), np.int64), np.ones((10, 10), np.float32)
        for r in range(10):
            x = src[r:r + 1].contiguous()
            for c in range(10):
                if r == c:
                    pred[r, c] = r
                    continue
                q = K.counterfactuals(G, C, x, c)
                pred[r, c], conf[r, c] = q["pred"].item(), q["conf"].item()
        return pred, conf

    legs = {"pick": pick_fused, "pick_loop": pick_loop, "grid": grid_fused, "grid_loop": grid_loop}
    grid_fused(); grid_loop(); pick_fused()                                   # warm-up (the per-row loop warms in its first rows)
    secs, res = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            s, res[k] = timed(leg)
            secs[k].append(s)
    rows_f, conf_f = res["pick"]
    rows_l, conf_l = res["pick_loop"]
    if float(np.abs(conf_f - conf_l).max()) > 1e-5:
        sys.exit(f"the pick legs disagree on the confidences: {conf_f} vs {conf_l}")
    agree = int((rows_f == rows_l).sum())
    if float(np.abs(res["grid"][1] - res["grid_loop"][1]).max()) > 1e-4:
        sys.exit("the grid legs disagree on the confidences")

    def stats(v):
        v = np.asarray(v) * 1e3
        return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                "all": [round(float(s), 3) for s in v]}
    ms = {k: stats(v) for k, v in secs.items()}
    spread = {a: max(ms[a]["max"] - ms[a]["min"], ms[b]["max"] - ms[b]["min"]) for a, b in (("pick", "pick_loop"), ("grid", "grid_loop"))}
    line = {
        "metric": f"rows/sec, MNIST CounteRGAN pick_sources(pick_best_source=True, full_scan=True), {args.rows} rows, chunk {args.chunk}",
        "value": round(args.rows / (ms["pick"]["median"] * 1e-3), 1), "unit": "rows/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "ms": ms, "rounds": args.rounds, "round_spread_ms": {k: round(v, 3) for k, v in spread.items()},
        "pick_vs_loop": round(ms["pick_loop"]["median"] / ms["pick"]["median"], 2),
        "grid_vs_loop": round(ms["grid_loop"]["median"] / ms["grid"]["median"], 2),
        "pick_faster_by_more_than_the_spread": bool(ms["pick_loop"]["median"] - ms["pick"]["median"] > spread["pick"]),
        "grid_faster_by_more_than_the_spread": bool(ms["grid_loop"]["median"] - ms["grid"]["median"] > spread["grid"]),
        "picked_rows": rows_f.tolist(), "picked_rows_equal_the_loops": agree,
        "grid_pred_cells_equal": int((res["grid"][0] == res["grid_loop"][0]).sum()),
        "config": {"workload": "seeded CNNClassifier and ResidualGenerator, synthetic rows resident on the device", "parallelism": "dp1",
                   "baseline": "pick: one batch-1 classifier forward + score launch + host read per row; grid: 90 counterfactuals() calls"},
        "roofline": {"bound": "not analysed", "kernel": "the library's convolutions; pcg_class_pick, pcg_cf_panels in csrc/cf_report.hip"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
