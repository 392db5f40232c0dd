#!/usr/bin/env python3
"""The tabular CounteRGAN's evaluation (conditional_counteRGAN/house_sales_kc_usa/eval_utils.py:185-289, four target classes) on one
MI355X: the one-launch path against the op chain and against eager PyTorch.

  python scripts/bench_house_cf_eval.py [--rounds 5] [--big-rounds 2] [--big 65536] [--out profiles/house_cf_eval_bench_line.json]

Legs, all in this process on one GPU, in alternating rounds after a warm-up of every leg, every leg on the same Gumbel draws (a
fresh ops.DeviceRNG(7) per run, drawn per generator call in the chain's order):
  one_launch  house.compute_metrics_per_target(one_launch=True): the per-call draws, then ONE pcg_house_cf_eval launch and one read of
              the tile sums; wall clock to the host read, and the bare kernel by device events around single launches (median)
  chain       house.compute_metrics_per_target(one_launch=False): the op chain per (target class, loader batch) — the parent path,
              unchanged
  eager       the same loop in eager PyTorch on the GPU (the modules of oracle/house_ref.py, fp32, eval mode)
at two sizes: the reference's test split (tests/golden/house_eval.npz, 4323 rows) and --big rows drawn from a seeded generator, batch
size 128.  The legs' metric tables must agree before anything is printed.  Kernel launches per leg are counted with torch.profiler
in one extra run (null where the profiler cannot see them).  Reads only this tree.  One JSON line, the contract of
scripts/bench_moons_cf_eval.py; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BS = 128
FIELDS = ("class_flip", "prediction_gain", "avg_actionability")


class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi


def eager_metrics(R, oG, oC, X, y, cfg, norm_maps, seg, cat_idx, rng, dev):
    """eval_utils.py:218-279 in eager PyTorch; the Gumbel noise of every generator call from `rng`, as the chain draws it."""
    X_t, y_t = torch.as_tensor(X, dtype=torch.float32), torch.as_tensor(y, dtype=torch.long)
    Tc = seg[-1]
    rows = []
    with torch.no_grad():
        for target in range(4):
            flips, gains, acts = [], [], []
            for i in range(0, len(X_t), BS):
                xb, yb = X_t[i:i + BS], y_t[i:i + BS]
                sel = yb != target
                if sel.sum() == 0:
                    continue
                x = xb[sel].to(dev)
                bs = x.size(0)
                tv = torch.full((bs,), target, dtype=torch.long, device=dev)
                noise = rng.gumbel((bs, Tc), dev)
                gd = {f: noise[:, seg[s]:seg[s + 1]] for s, f in enumerate(cat_idx)}
                masked, _ = R.build_counterfactuals(oG, x, F.one_hot(tv, 4).float(), gd, norm_maps, cfg)
                x_cf = x + masked
                probs_orig, logits_cf = F.softmax(oC(x), dim=1), oC(x_cf)
                probs_cf = F.softmax(logits_cf, dim=1)
                ar = torch.arange(bs, device=dev)
                flips.append((logits_cf.argmax(1) == tv).float().mean().item())
                gains.append((probs_cf[ar, tv] - probs_orig[ar, tv]).mean().item())
                acts.append(masked.abs().mean().item())
            rows.append([float(np.mean(v)) if v else float("nan") for v in (flips, gains, acts)])
    return np.array(rows)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def count_launches(fn):
    """GPU kernels launched by one run of fn, or None where the profiler records none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if getattr(ev, "device_type", None) is not None and str(ev.device_type).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-rounds", type=int, default=2)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the profiler run that counts launches")
    args = ap.parse_args()
    import pcgan_amd
    from oracle import house_ref as R
    from pcgan_amd import house as H, ops
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    gdir = os.path.join(ROOT, "tests", "golden")
    gold = dict(np.load(os.path.join(gdir, "house_eval.npz")))
    cfg = dict(H.CONFIG, batch_size=BS)
    cfg["categorical_info"] = {f: {"n": len(gold[f"raw_values.{f}"]), "raw_values": gold[f"raw_values.{f}"].tolist()} for f in H.CONFIG["categorical_info"]}
    cfg["scaler"] = _Scaler(gold["scaler.data_min"], gold["scaler.data_max"])
    sd_g = torch.load(os.path.join(gdir, "house_generator_trained.pt"), map_location="cpu", weights_only=True)
    sd_c = torch.load(os.path.join(gdir, "house_classifier_trained.pt"), map_location="cpu", weights_only=True)
    G, C = H.ResidualGenerator(17, 32, 4, cfg["continuous_idx"], cfg["categorical_info"], tau=0.5), H.NNClassifier(17, 4)
    oG, oC = R.ResidualGenerator(17, 32, 4, R.CONFIG["continuous_idx"], R.CONFIG["categorical_info"], tau=0.5), R.NNClassifier(17, 4)
    for net in (G, C, oG, oC):
        net.load_state_dict(sd_g if net in (G, oG) else sd_c)
        net.to(dev).eval()
        for p in net.parameters():
            p.requires_grad = False
    norm = H.cat_norm_maps(G, cfg, dev)
    norm_maps = {f: norm[G.seg[s]:G.seg[s + 1]] for s, f in enumerate(G.cat_idx)}
    rs = np.random.default_rng(0)
    sizes = {str(len(gold["X_test"])): (gold["X_test"], gold["y_test"]),
             str(args.big): (rs.uniform(0.0, 1.0, (args.big, 17)).astype(np.float32), rs.integers(0, 4, args.big))}

    def table(res):
        return np.array([[r[k] for k in FIELDS] for r in res[0]])

    def house_leg(one_launch):
        def run(X, y):
            G.rng = None
            return table(H.compute_metrics_per_target(G, C, X, y, cfg, rng=ops.DeviceRNG(7), one_launch=one_launch))
        return run

    legs = {"one_launch": house_leg(True), "chain": house_leg(False),
            "eager": lambda X, y: eager_metrics(R, oG, oC, X, y, cfg, norm_maps, G.seg, G.cat_idx, ops.DeviceRNG(7), dev)}
    result = {}
    for size, (X, y) in sizes.items():
        n = len(X)
        rounds = args.rounds if n <= 8192 else args.big_rounds
        warm = slice(0, min(n, 1024))
        for leg in legs.values():                                             # warm-up: every leg, the batch shapes of the timed run
            leg(X[warm], y[warm])
        secs = {k: [] for k in legs}
        ref = None
        for _ in range(rounds):
            for k, leg in legs.items():
                s, tab = timed(lambda: leg(X, y))
                secs[k].append(s)
                if ref is None:
                    ref = tab
                # a row whose top-2 logits are within fp32 noise may flip in one leg: 1 / rows-of-a-batch / batches of class_flip
                elif not np.allclose(tab, ref, rtol=1e-3, atol=1e-4, equal_nan=True):
                    sys.exit(f"{k} at {n} rows disagrees with one_launch: max difference {np.nanmax(np.abs(tab - ref)):.3e}\n{tab}\n{ref}")
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(np.asarray(y)).to(dev)
        noise = ops.DeviceRNG(7).gumbel((4, n, G.total_cat), dev)
        ev = []
        for i in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            H.counterfactual_sweep(G, C, Xd, yd, cfg, batch_size=BS, gumbel=noise)
            e1.record()
            torch.cuda.synchronize()
            if i >= 5:
                ev.append(e0.elapsed_time(e1) * 1e3)
        launches = {k: None for k in legs}
        if not args.no_count and n <= 8192:
            launches = {k: count_launches(lambda: leg(X, y)) for k, leg in legs.items()}
        result[size] = {"rows": n, "rounds": rounds, "metrics": ref.tolist(),
                        "ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in secs.items()},
                        "ms_all_rounds": {k: [round(s * 1e3, 3) for s in v] for k, v in secs.items()},
                        "sweep_call_us": round(float(np.median(ev)), 2), "launches": launches,
                        "one_launch_vs_chain": round(float(np.median(secs["chain"]) / np.median(secs["one_launch"])), 2),
                        "one_launch_vs_eager": round(float(np.median(secs["eager"]) / np.median(secs["one_launch"])), 2)}
    small = result[str(len(gold["X_test"]))]
    line = json.dumps({
        "metric": "evaluations/sec, house-sales CounteRGAN compute_metrics_per_target (eval_utils.py:185-289), 4323 test rows, batch 128, "
                  "4 targets, one launch",
        "value": round(1e3 / small["ms"]["one_launch"], 2), "unit": "evaluations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "sizes": result,
        "config": {"workload": f"conditional_counteRGAN/house_sales_kc_usa eval_utils.py:185-289, shipped checkpoints, batch_size {BS}",
                   "parallelism": "dp1", "baseline": "the chain leg (one_launch=False): the parent path, unchanged"},
        "roofline": {"bound": "not analysed", "kernel": "16-row tiles x all targets per workgroup; generator on the vector ALU, classifier on "
                                                        "v_mfma_f32_16x16x4_f32 (csrc/house_cf_eval.hip)"},
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
