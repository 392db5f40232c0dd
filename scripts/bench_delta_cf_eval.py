#!/usr/bin/env python3
"""The additive-delta MNIST CounteRGAN's per-target evaluation (gan_train.evaluate_per_target; the metrics of
conditional_counteRGAN/mnist/eval_utils.py:58-66 folded as :97-102) and one single-image query, three ways in ONE process, in
alternating rounds:

  python scripts/bench_delta_cf_eval.py [--rounds 5] [--rows 10000] [--batch 128] [--out profiles/delta_cf_eval_bench_line.json]

  one_pass   gan_train.evaluate_per_target(one_pass=True): all 10 targets of a loader batch in one sweep (csrc/delta_cf_eval.hip
             around the library's convolutions), one score launch per batch, the group sums read once for the whole loader
  loop       the per-(batch, target) loop built from the parent commit's pieces: gan_train.counterfactual_batch, the classifier's
             forward, and the three metrics formed on the host side with torch, one read each -- the baseline
  eager      the same loop on the reference-shaped nets in eager PyTorch on the same GPU

Synthetic rows (scripts/bench_delta_gan.py's templates plus noise), seeded nets, the loader's rows already on the device.  The three
legs must agree on the table.  Prints ONE JSON line with the median, the spread and every round of each leg, and writes it to --out."""
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
import torch.nn.functional as F  # noqa: E402

import bench_delta_gan as BG  # noqa: E402

FIELDS = ("class_flip_rate", "prediction_gain", "actionability")


def loop_table(cf_fn, clf, loader):
    """eval_utils.py:58-66 per (batch, target), :97-102 over the batches; cf_fn(x, target) -> the clamped counterfactual."""
    res, n = np.zeros((10, 3)), 0
    with torch.no_grad():
        for x, y in loader:
            ar = torch.arange(len(y), device=x.device)
            for t in range(10):
                tgt = torch.full_like(y, t)
                x_cf = cf_fn(x, tgt)
                logits = clf(x_cf)
                probs = F.softmax(logits, dim=1)
                res[t] += [(logits.argmax(1) == tgt).float().mean().item(), (probs[ar, tgt] - probs[ar, y]).mean().item(),
                           torch.abs(x_cf - x).mean().item()]
            n += 1
    return res / n


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--query-rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delta_cf_eval_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import countergan as K, gan_train as T
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    G = T.Generator().to(dev)
    torch.manual_seed(5)
    C = K.Classifier().to(dev).eval()
    eG, eC = BG.EagerG().to(dev), BG.eager_classifier().to(dev).eval()
    eG.load_state_dict(G.state_dict())
    eC.load_state_dict({k[len("net."):]: v for k, v in C.state_dict().items()})
    for net in (G, C, eG, eC):
        for p in net.parameters():
            p.requires_grad = False
    X, Y = BG.synthetic(args.rows, 1)
    X, Y = X.to(dev), Y.to(dev)
    loader = [(X[i:i + args.batch].contiguous(), Y[i:i + args.batch].contiguous()) for i in range(0, args.rows, args.batch)]

    def one_pass(ld):
        res = T.evaluate_per_target(G, C, ld, one_pass=True, verbose=False)
        return np.array([[res[c][k] for k in FIELDS] for c in range(10)])
    legs = {"one_pass": one_pass,
            "loop": lambda ld: loop_table(lambda x, t: T.counterfactual_batch(G, x, t)[0], C, ld),
            "eager": lambda ld: loop_table(lambda x, t: torch.clamp(eG(x, t)[0], -1, 1), eC, ld)}
    warm = loader[:2] + loader[-1:]                                           # the batch shapes of the timed run, the ragged one included
    for leg in legs.values():
        leg(warm)
    secs, ref, worst = {k: [] for k in legs}, None, 0.0
    for _ in range(args.rounds):
        for k, leg in legs.items():
            s, tab = timed(lambda: leg(loader))
            secs[k].append(s)
            if ref is None:
                ref = tab
            worst = max(worst, float(np.abs(tab - ref).max()))
    if worst > 1e-3:       # a query whose top-two probabilities are within fp32 noise may flip in one leg: 1 / batch / batches each
        sys.exit(f"the legs disagree on the table: max difference {worst:.3e}")
    # one single-image query: "turn this image into a 7"
    x1, t1 = X[:1].contiguous(), torch.tensor([7], device=dev)
    with torch.no_grad():
        q_legs = {"one_pass": lambda: T.counterfactuals(G, C, x1, t1)["pred"].item(),
                  "loop": lambda: C(T.counterfactual_batch(G, x1, t1)[0]).argmax(1).item(),
                  "eager": lambda: eC(torch.clamp(eG(x1, t1)[0], -1, 1)).argmax(1).item()}
        preds = {k: leg() for k, leg in q_legs.items()}
        q_secs = {k: [] for k in q_legs}
        for _ in range(args.query_rounds):
            for k, leg in q_legs.items():
                q_secs[k].append(timed(leg)[0])

    def stats(v, unit):
        v = np.asarray(v) * unit
        return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                "all": [round(float(s), 3) for s in v]}
    ev = {k: stats(v, 1e3) for k, v in secs.items()}
    qu = {k: stats(v, 1e6) for k, v in q_secs.items()}
    for d in qu.values():
        d.pop("all")
    spread = max(ev["one_pass"]["max"] - ev["one_pass"]["min"], ev["loop"]["max"] - ev["loop"]["min"])
    line = {
        "metric": f"evaluations/sec, additive-delta MNIST CounteRGAN evaluate_per_target, {args.rows} rows, batch {args.batch}, 10 targets, "
                  "one sweep per batch",
        "value": round(1e3 / ev["one_pass"]["median"], 3), "unit": "evaluations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "evaluation_ms": ev, "rounds": args.rounds, "round_spread_ms": round(spread, 3),
        "one_pass_vs_loop": round(ev["loop"]["median"] / ev["one_pass"]["median"], 3),
        "one_pass_vs_eager": round(ev["eager"]["median"] / ev["one_pass"]["median"], 3),
        "faster_than_loop_by_more_than_the_spread": bool(ev["loop"]["median"] - ev["one_pass"]["median"] > spread),
        "query_us": qu, "query_pred": preds, "legs_max_table_difference": worst, "metrics": ref.tolist(),
        "config": {"workload": "gan_train_copy.py's generator (seeded), the max-pool classifier (seeded), synthetic rows resident on the device",
                   "parallelism": "dp1", "baseline": "the loop leg: counterfactual_batch + classifier forward + host-side metrics per (batch, target)"},
        "roofline": {"bound": "not analysed", "kernel": "the library's convolutions; entry / tail in csrc/delta_cf_eval.hip, pcg_mnist_cf_score"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
