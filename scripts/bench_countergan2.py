#!/usr/bin/env python3
"""The full-resolution MNIST CounteRGAN step (conditional_counteRGAN/mnist/countergan2.py:180-205) on one MI355X: the fused step
(countergan2.GraphedTrainStep: fused entry / head / tail launches around the convolutions, one graph replay per step)
against the op chain (countergan2.train_step, the default, existing kernels only) and the reference-shaped nets in eager PyTorch.

  python scripts/bench_countergan2.py [--steps 100] [--rounds 7] [--batch 128] [--out profiles/countergan2_bench_line.json]

One process, one GPU.  Synthetic rows (ten 28x28 templates plus noise) at the reference's batch 128, eight batches resident on the
device and walked round-robin.  Every leg is run once untimed (which also captures the graph), then `--rounds` alternating rounds
(fused, chain, eager, fused, ...) of device-synchronised wall time around `--steps` iterations: median and min..max per leg, per step.
The library calls of one step of both paths are counted through ops.check.

The head alone: pcg_prob_head_fwd at slabs = 1, 2, 4, 8 for R = 2 * batch and R = batch rows of F = 50176 columns, against the pieces of
the op chain it replaces (nhwc_to_nchw_flat, the GEMM, the sigmoid, the loss op), each as a captured graph of `--head-launches`
launches whose activation operand rotates through more buffers than the 256 MB last-level cache holds; per launch, in the same
alternating rounds.  `beats_slabs_1_in_every_round` is what the library's default slab count is chosen from.
One JSON line (scripts/_benchlib.py: emit), also written to `--out`."""
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
from bench_delta_gan import eager_classifier, spread, synthetic  # noqa: E402

F = 64 * 784
SLABS = (1, 2, 4, 8)


class EagerG(nn.Module):
    def __init__(self):
        super().__init__()
        self.label_embed = nn.Embedding(10, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(64, 1, 3, padding=1))

    def forward(self, x, c):
        delta = self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))
        return x + delta, delta


class EagerD(nn.Module):
    def __init__(self):
        super().__init__()
        self.label_embed = nn.Embedding(10, 784)
        self.net = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1), nn.LeakyReLU(0.2), nn.Conv2d(64, 64, 3, padding=1), nn.LeakyReLU(0.2),
                                 nn.Flatten(), nn.Linear(F, 1), nn.Sigmoid())

    def forward(self, x, c):
        return self.net(torch.cat([x, self.label_embed(c).view(-1, 1, 28, 28)], dim=1))


def eager_stepper(dev, p):
    """The reference's loop body in eager PyTorch on the GPU."""
    torch.manual_seed(7)
    G, D, C = EagerG().to(dev), EagerD().to(dev), eager_classifier().to(dev).eval()
    for q in C.parameters():
        q.requires_grad = False
    opt_g, opt_d = torch.optim.Adam(G.parameters(), lr=p["lr_G"]), torch.optim.Adam(D.parameters(), lr=p["lr_D"])
    ce = nn.CrossEntropyLoss()

    def step(x, y, target):
        x_cf, _ = G(x, target)
        d_real, d_fake = D(x, y), D(x_cf.detach(), target)
        loss_D = -torch.mean(torch.log(d_real + 1e-6) + torch.log(1 - d_fake + 1e-6))
        opt_d.zero_grad(); loss_D.backward(); opt_d.step()
        x_cf, delta = G(x, target)
        d_fake = D(x_cf, target)
        loss_G = -torch.mean(torch.log(d_fake + 1e-6)) + p["lambda_cls"] * ce(C(x_cf), target) + p["lambda_reg"] * torch.mean(torch.abs(delta))
        opt_g.zero_grad(); loss_G.backward(); opt_g.step()
        return {"loss_D": loss_D.detach(), "loss_G": loss_G.detach()}
    return step


def head_alone(ops, dev, B, rounds, launches):
    """us per launch of the head at every slab count, and of the op chain's pieces it replaces, for R = 2B (D's step) and R = B (D's
    pass of the G step)."""
    nbuf = 6                                                         # 6 x [2B, F] fp32 at B = 128 = 308 MB: more than the last-level cache
    pool = [torch.randn(2 * B, F, device=dev) * 0.05 for _ in range(nbuf)]
    w = torch.randn(F, device=dev) / F ** 0.5
    w_row = w.view(1, F)
    bias = torch.zeros(1, device=dev)
    out = {}
    for R, mode_g in ((2 * B, False), (B, True)):
        views = [buf[i:i + R] for buf in pool for i in range(0, 2 * B, R)]
        o = {k: torch.empty(R, device=dev) for k in ("logits", "prob", "dlogit")}
        o1 = {k: torch.empty(1, device=dev) for k in ("loss", "db")}
        ws = ops.prob_head_workspace(R, dev, max(SLABS))

        def head(slabs):
            def go(i):
                ops.prob_head_fwd(views[i % len(views)], w, bias, mode_g=mode_g, slabs=slabs, ws=ws, **o, **o1)
            return go

        def pieces(i):
            a = views[i % len(views)]
            flat = ops.nhwc_to_nchw_flat(a.view(R, 28, 28, 64), R, 784, 64).view(R, F)
            z = ops.gemm(flat, w_row, R, 1, F, transB=True, bias=bias)
            prob = ops.act_fwd(z, ops.ACT_SIGMOID)
            ops.log_eps_loss_fwd_bwd(prob.view(-1), mode_g)

        legs = {f"slabs_{s}": head(s) for s in SLABS}
        legs["op_chain_pieces"] = pieces
        graphs = {}
        side = torch.cuda.Stream()
        for k, go in legs.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                go(0)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(launches):
                    go(i)
            graphs[k] = g
            g.replay()                                               # once untimed
        torch.cuda.synchronize()
        us = {k: [] for k in legs}
        for _ in range(rounds):
            for k, g in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.replay()
                torch.cuda.synchronize()
                us[k].append((time.perf_counter() - t0) * 1e6 / launches)
        res = {k: spread(v, 2) for k, v in us.items()}
        res["beats_slabs_1_in_every_round"] = {f"slabs_{s}": bool(all(a < b for a, b in zip(us[f"slabs_{s}"], us["slabs_1"]))) for s in SLABS[1:]}
        res["bytes_read_per_launch"] = 4 * (R * F + F)
        out[f"R{R}"] = res
        del graphs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--head-launches", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "countergan2_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import countergan as K, countergan2 as T
    pcgan_amd.load()
    ops = pcgan_amd.ops
    dev = torch.device("cuda:0")
    B, p = args.batch, dict(T.params(5), batch_size=args.batch)
    xs, ys = synthetic(8 * B, 1)
    batches = [(xs[i:i + B].to(dev).contiguous(), ys[i:i + B].to(dev).contiguous()) for i in range(0, 8 * B, B)]
    target = torch.full((B,), p["target"], dtype=torch.int64, device=dev)

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
    del eager_fused, Ge, De, Ce
    us, last = {k: [] for k in legs}, {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t, last[k] = run(fn, args.steps)
            us[k].append(t)
    for k, out in last.items():
        v = [float(out["loss_D"].cpu()), float(out["loss_G"].cpu())]
        if not np.isfinite(v).all():
            sys.exit(f"{k}: losses {v}")
    head = head_alone(ops, dev, B, args.rounds, args.head_launches)
    f, c, e = (spread(us[k]) for k in ("fused", "op_chain", "eager"))
    line = {
        "metric": f"full-resolution MNIST CounteRGAN step (mnist/countergan2.py:180-205) at batch {B}, fused step",
        "value": f["median"], "unit": "us", "n_gpus": 1, "higher_is_better": False, "dtype": "f32",
        "us_per_step": {"fused": f, "op_chain": c, "eager": e},
        "steps_per_round": args.steps, "rounds": args.rounds, "batch": B,
        "fused_vs_op_chain": round(c["median"] / f["median"], 2), "fused_vs_eager": round(e["median"] / f["median"], 2),
        "fused_slowest_round_below_op_chain_fastest": bool(f["max"] < c["min"]),
        "library_calls_per_step": {"fused": len(fused_calls), "op_chain": len(chain_calls),
                                   "fused_by_entry": {w: fused_calls.count(w) for w in sorted(set(fused_calls))},
                                   "op_chain_by_entry": {w: chain_calls.count(w) for w in sorted(set(chain_calls))},
                                   "note": "the fused step's calls are captured once; a replayed step is two input copies and one graph launch"},
        "head_alone_us_per_launch": head, "head_launches_per_graph": args.head_launches,
        "default_slabs": {f"R{n}": int((ops._lib.load().pcg_prob_head_workspace_bytes(n, 0) - 16) // (4 * n)) for n in (2 * B, B)},
        "config": {"workload": "Generator 2-64-64-1 (3x3, ReLU), Discriminator 2-64-64 (3x3, s1, LeakyReLU 0.2) + Linear(50176, 1) + Sigmoid, "
                               "frozen max-pool classifier, log-eps losses + 3.0 cross-entropy + 0.05 L1, Adam(1e-3) x 2", "parallelism": "dp1"},
        "roofline": {"bound": "the convolution launches of the replayed step (DESIGN.md §3.21), not launch latency",
                     "kernel": "one linear HIP graph per step: entry, G forward, tail, D forward of 2B rows, head, D backward, Adam(D), regather, "
                               "D forward of B rows, head, grad-inputs, classifier guidance, tail backward, G backward, Adam(G)"},
    }
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    _benchlib.emit(line)


if __name__ == "__main__":
    main()
