#!/usr/bin/env python3
"""The additive-delta MNIST CounteRGAN step (conditional_counteRGAN/mnist/gan_train.py:117-144) on one MI355X: the fused step
(gan_train.GraphedTrainStep: fused entry / head / tail launches around the convolutions, one graph replay per step)
against the op chain (gan_train.train_step, the default and the baseline) and the reference-shaped nets in eager PyTorch.

  python scripts/bench_delta_gan.py [--steps 100] [--rounds 7] [--batch 128] [--out profiles/delta_gan_bench_line.json]

One process, one GPU.  Synthetic rows (ten 28x28 templates plus noise) at the reference's batch 128, eight batches resident on the
device and walked round-robin.  Every leg is run once untimed (which also captures the graph), then `--rounds` alternating rounds
(fused, chain, eager, fused, ...) of device-synchronised wall time around `--steps` iterations: median and min..max per leg, per step.
The library calls of one step of both paths are counted through ops.check.  One JSON line (scripts/_benchlib.py: emit), also written
to `--out`.

  python scripts/bench_delta_gan.py --random-target [--out profiles/delta_gan_random_target_bench_line.json]

measures instead the random-target fused step (gan_train_copy.py:119-146: GraphedTrainStep(rng=...), the class draw as the first of 65
captured launches) against the fixed-target fused step (64 launches) under the same parameters, in the same
alternating rounds, and the draw launch on its own (a captured graph of 100 draws, per launch)."""
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


def spread(v, digits=1):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def synthetic(n, seed):
    y = np.random.RandomState(seed).randint(0, 10, n)
    t = np.kron(np.random.RandomState(0).choice([-1.0, 1.0], size=(10, 7, 7)), np.ones((4, 4))).astype(np.float32)
    x = np.clip(t[y] + 0.3 * np.random.RandomState(seed + 1).standard_normal((n, 28, 28)).astype(np.float32), -1, 1)
    return torch.from_numpy(x[:, None]), torch.from_numpy(y)


class EagerG(nn.Module):
    def __init__(self):
        super().__init__()
        self.label_embed = nn.Embedding(10, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(64, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 1, 3, padding=1))

    def forward(self, x, c):
        delta = self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))
        return x + delta, delta


class EagerD(nn.Module):
    def __init__(self):
        super().__init__()
        self.label_embed = nn.Embedding(10, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, stride=2, padding=1), nn.LeakyReLU(0.2), nn.Conv2d(64, 128, 3, stride=2, padding=1),
                                 nn.LeakyReLU(0.2), nn.Conv2d(128, 256, 3, stride=1, padding=1), nn.LeakyReLU(0.2), nn.Flatten(),
                                 nn.Linear(256 * 7 * 7, 1))

    def forward(self, x, c):
        return self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))


def eager_classifier():
    return nn.Sequential(nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
                         nn.Flatten(), nn.Linear(64 * 7 * 7, 128), nn.ReLU(), nn.Linear(128, 10))


def eager_stepper(dev, p):
    """The reference's loop body in eager PyTorch on the GPU."""
    torch.manual_seed(7)
    G, D, C = EagerG().to(dev), EagerD().to(dev), eager_classifier().to(dev).eval()
    for q in C.parameters():
        q.requires_grad = False
    opt_g, opt_d = torch.optim.Adam(G.parameters(), lr=p["lr_G"]), torch.optim.Adam(D.parameters(), lr=p["lr_D"])
    bce, ce = nn.BCEWithLogitsLoss(), nn.CrossEntropyLoss()

    def step(x, y, target):
        x_cf, _ = G(x, target)
        d_real, d_fake = D(x, y), D(x_cf.detach(), target)
        loss_D = bce(d_real, torch.ones_like(d_real)) + bce(d_fake, torch.zeros_like(d_fake))
        opt_d.zero_grad(); loss_D.backward(); opt_d.step()
        x_cf, delta = G(x, target)
        d_fake = D(x_cf, target)
        loss_G = bce(d_fake, torch.ones_like(d_fake)) + p["lambda_cls"] * ce(C(x_cf), target) + p["lambda_reg"] * torch.mean(torch.abs(delta))
        opt_g.zero_grad(); loss_G.backward(); opt_g.step()
        return {"loss_D": loss_D.detach(), "loss_G": loss_G.detach()}
    return step


def random_target(args):
    """The random-target fused step against the fixed-target one: same nets, same parameters, alternating rounds."""
    import pcgan_amd
    from pcgan_amd import countergan as K, gan_train as T
    pcgan_amd.load()
    ops = pcgan_amd.ops
    dev = torch.device("cuda:0")
    B, p = args.batch, dict(T.params, batch_size=args.batch)
    xs, ys = synthetic(8 * B, 1)
    batches = [(xs[i:i + B].to(dev).contiguous(), ys[i:i + B].to(dev).contiguous()) for i in range(0, 8 * B, B)]
    target = torch.full((B,), p["target_class"], dtype=torch.int64, device=dev)

    def stepper(rng):
        torch.manual_seed(7)
        G, D = T.Generator().to(dev), T.Discriminator().to(dev)
        torch.manual_seed(5)
        return T.GraphedTrainStep(G, D, K.Classifier().to(dev).eval(), B, p, rng=rng)
    fixed, drawn = stepper(None), stepper(ops.DeviceRNG(11))
    legs = {"fixed_target": lambda x, y: fixed.step(x, y, target), "random_target": lambda x, y: drawn.step(x, y)}

    def run(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            out = fn(*batches[i % len(batches)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n, out
    for fn in legs.values():
        run(fn, 10)
    # the draw launch on its own: 100 of them captured into one graph, per launch
    rng, n_draw = ops.DeviceRNG(13), 100
    ctr = rng.device_counter(dev)
    tbuf = torch.zeros(B, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rng.delta_gan_target(tbuf, 10, counter=ctr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n_draw):
            rng.delta_gan_target(tbuf, 10, counter=ctr)
    draw_us = []
    for _ in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graph.replay()
        torch.cuda.synchronize()
        draw_us.append((time.perf_counter() - t0) * 1e6 / n_draw)
    draw_us = draw_us[1:]
    us, last = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t, last[k] = run(fn, args.steps)
            us[k].append(t)
    for k, out in last.items():
        v = [float(out["loss_D"].cpu()), float(out["loss_G"].cpu())]
        if not np.isfinite(v).all():
            sys.exit(f"{k}: losses {v}")
    f, r, d = spread(us["fixed_target"]), spread(us["random_target"]), spread(draw_us, 2)
    allowance = f["median"] + d["median"] + (f["max"] - f["min"])
    line = {
        "metric": f"additive-delta MNIST CounteRGAN step at batch {B}, random-target fused step (gan_train_copy.py:119-146)",
        "value": r["median"], "unit": "us", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "us_per_step": {"fixed_target": f, "random_target": r}, "draw_launch_us": d,
        "steps_per_round": args.steps, "rounds": args.rounds, "batch": B,
        "random_minus_fixed_us": round(r["median"] - f["median"], 1), "fixed_round_spread_us": round(f["max"] - f["min"], 1),
        "allowance_us": round(allowance, 1), "random_within_fixed_plus_draw_plus_spread": bool(r["median"] <= allowance),
        "classes_drawn": int(drawn._rng.offset),
        "config": {"workload": "the fused step of scripts/bench_delta_gan.py with the iteration's class drawn by the step's first launch "
                               "(65 captured launches) against a fixed target tensor (64)", "parallelism": "dp1"},
        "roofline": {"bound": "the convolution launches of the replayed step (DESIGN.md §3.19)", "kernel": "delta_gan_target_draw_kernel: one workgroup"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--random-target", action="store_true", help="the random-target fused step against the fixed-target one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "delta_gan_random_target_bench_line.json" if args.random_target else "delta_gan_bench_line.json")
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    if args.random_target:
        return random_target(args)
    import pcgan_amd
    from pcgan_amd import countergan as K, gan_train as T
    pcgan_amd.load()
    ops = pcgan_amd.ops
    dev = torch.device("cuda:0")
    B, p = args.batch, dict(T.params, batch_size=args.batch)
    xs, ys = synthetic(8 * B, 1)
    batches = [(xs[i:i + B].to(dev).contiguous(), ys[i:i + B].to(dev).contiguous()) for i in range(0, 8 * B, B)]
    target = torch.full((B,), p["target_class"], dtype=torch.int64, device=dev)

    def ours():
        torch.manual_seed(7)
        G, D = T.Generator().to(dev), T.Discriminator().to(dev)
        torch.manual_seed(5)
        return G, D, K.Classifier().to(dev).eval()

    G1, D1, C1 = ours()
    fused = T.GraphedTrainStep(G1, D1, C1, B, p)
    G2, D2, C2 = ours()
    opt_g, opt_d = T.make_optimizers(G2, D2, p)
    eager = eager_stepper(dev, p)
    legs = {
        "fused": lambda x, y: fused.step(x, y, target),
        "op_chain": lambda x, y: T.train_step(G2, D2, C2, opt_g, opt_d, x, y, target, p),
        "eager": lambda x, y: eager(x, y, target),
    }

    def run(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            out = fn(*batches[i % len(batches)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n, out

    for fn in legs.values():                                    # every leg once, untimed: graph capture, code objects, allocator
        run(fn, 10)
    # the library calls of one step of either path
    calls, real = [], ops.check
    ops.check = lambda rc, what="": (calls.append(what), real(rc, what))[1]
    try:
        Ge, De, Ce = ours()
        eager_fused = T.GraphedTrainStep(Ge, De, Ce, B, p, graph=False)
        eager_fused.step(*batches[0], target)
        del calls[:]
        eager_fused.step(*batches[1], target)
        fused_calls = list(calls)
        del calls[:]
        legs["op_chain"](*batches[0])
        chain_calls = list(calls)
    finally:
        ops.check = real
    us, last = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t, last[k] = run(fn, args.steps)
            us[k].append(t)
    for k, out in last.items():
        v = [float(out["loss_D"].cpu()), float(out["loss_G"].cpu())]
        if not np.isfinite(v).all():
            sys.exit(f"{k}: losses {v}")
    f, c, e = (spread(us[k]) for k in ("fused", "op_chain", "eager"))
    line = {
        "metric": f"additive-delta MNIST CounteRGAN step (mnist/gan_train.py:117-144) at batch {B}, fused step",
        "value": f["median"], "unit": "us", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "us_per_step": {"fused": f, "op_chain": c, "eager": e},
        "steps_per_round": args.steps, "rounds": args.rounds, "batch": B,
        "fused_vs_op_chain": round(c["median"] / f["median"], 2), "fused_vs_eager": round(e["median"] / f["median"], 2),
        "fused_slowest_round_below_op_chain_fastest": bool(f["max"] < c["min"]),
        "library_calls_per_step": {"fused": len(fused_calls), "op_chain": len(chain_calls),
                                   "fused_by_entry": {w: fused_calls.count(w) for w in sorted(set(fused_calls))},
                                   "op_chain_by_entry": {w: chain_calls.count(w) for w in sorted(set(chain_calls))},
                                   "note": "the fused step's calls are captured once; a replayed step is two input copies and one graph launch"},
        "config": {"workload": "Generator 2-64-64-32-1 (3x3, ReLU), Discriminator 2-64-128-256 (3x3, s2 s2 s1, LeakyReLU 0.2) + Linear(12544, 1), "
                               "frozen max-pool classifier, BCE-with-logits + 3.0 cross-entropy + 0.05 L1, Adam(1e-3) x 2", "parallelism": "dp1"},
        "roofline": {"bound": "the convolution launches of the replayed step (DESIGN.md §3.19), not launch latency",
                     "kernel": "one linear HIP graph per step: entry, G forward, tail, D forward of 2B rows, head, D backward, Adam(D), regather, "
                               "D forward of B rows, head, grad-inputs, classifier guidance, tail backward, G backward, Adam(G)"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


if __name__ == "__main__":
    main()
