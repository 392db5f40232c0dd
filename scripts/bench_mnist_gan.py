#!/usr/bin/env python3
"""Training iterations/s of the MNIST MLP GAN (simple_gan/mnist/mnist_gan.py:113-139) on one MI355X at the reference defaults:
batch 64, latent 100, Generator 100-128-256-512-1024-784 with three BatchNorm1d, Discriminator 784-512-256-1, synthetic 8-bit images.

  python scripts/bench_mnist_gan.py [--iters 400] [--rounds 5] [--train-batches 300] [--only fused|chain]

Legs, all in this process on one GPU, timed in interleaved rounds after an untimed warm-up of each:
  fused   pcgan_amd.mnist_gan.train_step on csrc/dense_rows.hip, replayed from a HIP graph; device events around `iters` replays
  chain   the same step with use_fused = False (the older ops, one after the other), replayed from a HIP graph the same way
  eager   the same loop body in eager PyTorch-ROCm fp32 on the GPU (stock nn.Sequential, torch.optim.Adam; z drawn on the device,
          which is kinder to it than the reference's host draw)
and, once, `mnist_gan.train` (graph replay, device draws, shuffled DeviceLoader) for iterations/s by the wall clock.
One JSON line, the contract of scripts/bench_moons_cf.py.  Needs nothing outside this repository."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

G_WIDTHS = (100, 128, 256, 512, 1024, 784)      # mnist_gan.py:52-59
D_WIDTHS = (784, 512, 256, 1)                   # :70-77


def algorithmic_flops(batch):
    """FLOP of one iteration of the loop body (:116-134) as the port computes it: 2 per multiply-add of every GEMM, nothing else
    (BatchNorm, activations, losses and Adam are O(features) or O(parameters), below 1 % of this).  Two pieces of the reference's
    work are counted as NOT done because their results are unused: D's forward on the generated batch in the D step (bit-identical
    to the G step's) and D's weight gradients in the G step's backward (discarded by zero_grad)."""
    pairs = lambda w: [a * b for a, b in zip(w[:-1], w[1:])]
    sg, sd = sum(pairs(G_WIDTHS)), sum(pairs(D_WIDTHS))
    g0, d0 = pairs(G_WIDTHS)[0], pairs(D_WIDTHS)[0]
    macs = batch * (sg                       # G forward
                    + sd                     # D forward on the generated batch (G step)
                    + sd                     # grad-input through D, down to the image
                    + (sg - g0)              # grad-input through G (not into z)
                    + sg                     # G weight gradients
                    + sd                     # D forward on the real batch; the generated rows are kept from the G step
                    + 2 * (sd - d0)          # grad-input through D on the stacked 2 x batch rows (not into the images)
                    + 2 * sd)                # D weight gradients on the stacked rows
    skipped = batch * (sd + sd)              # D forward on the generated batch again, D weight gradients in the G step
    return 2 * macs, 2 * skipped


def eager_nets(dev):
    def block(i, o, normalize=True):
        return [nn.Linear(i, o)] + ([nn.BatchNorm1d(o, 0.8)] if normalize else []) + [nn.LeakyReLU(0.2, inplace=True)]
    w = G_WIDTHS
    G = nn.Sequential(*block(w[0], w[1], False), *block(w[1], w[2]), *block(w[2], w[3]), *block(w[3], w[4]), nn.Linear(w[4], w[5]), nn.Tanh())
    D = nn.Sequential(nn.Linear(784, 512), nn.LeakyReLU(0.2, inplace=True), nn.Linear(512, 256), nn.LeakyReLU(0.2, inplace=True),
                      nn.Linear(256, 1), nn.Sigmoid())
    return G.to(dev), D.to(dev)


def eager_step(G, D, og, od, bce, real, ones, zeros):
    og.zero_grad()
    z = torch.randn(real.shape[0], 100, device=real.device)
    fake = G(z)
    g_loss = bce(D(fake), ones)
    g_loss.backward()
    og.step()
    od.zero_grad()
    d_loss = (bce(D(real), ones) + bce(D(fake.detach()), zeros)) / 2
    d_loss.backward()
    od.step()
    return g_loss, d_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400, help="iterations per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train-batches", type=int, default=300, help="batches per epoch of the train() leg (plus a 32-row tail)")
    ap.add_argument("--only", choices=("fused", "chain"), help="replay that leg alone (a run under rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mnist_gan.py needs the GPU: there is no CPU path and no CPU timing")
    import pcgan_amd
    from pcgan_amd import mnist_gan as M, ops
    from pcgan_amd.data import DeviceLoader
    from pcgan_amd.nn import GraphedStep
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    bs = M.config["batch_size"]
    rs = np.random.RandomState(0)
    n_img = bs * args.train_batches + 32
    images = torch.from_numpy(rs.randint(0, 256, (n_img, 784)).astype(np.uint8)).to(dev).float().div_(255).sub_(0.5).div_(0.5)
    real = images[:bs].contiguous()
    z = torch.from_numpy(rs.normal(0, 1, (bs, 100)).astype(np.float32)).to(dev)

    calls = {"n": 0}
    real_check = ops.check

    def counting_check(rc, what=""):
        calls["n"] += 1
        return real_check(rc, what)

    def hip_leg(fused):
        torch.manual_seed(0)
        G, D = M.Generator().to(dev), M.Discriminator().to(dev)
        G.use_fused = D.use_fused = fused
        og, od = M.make_optimizers(G, D)
        M.train_step(G, D, og, od, real, z)                       # builds the flat buffers, the workspace and Adam's state
        calls["n"] = 0
        ops.check = counting_check
        try:
            M.train_step(G, D, og, od, real, z)
        finally:
            ops.check = real_check
        ncalls = calls["n"]
        sr, sz = real.clone(), z.clone()
        gs = GraphedStep(lambda: M.train_step(G, D, og, od, sr, sz), {"real": sr, "z": sz}, [G, D], [og, od])
        return {"G": G, "D": D, "gs": gs, "library_calls": ncalls, "keep": (og, od)}

    if args.only:
        leg = hip_leg(args.only == "fused")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(50):
            leg["gs"].replay()
        e0.record()
        for _ in range(args.iters):
            leg["gs"].replay()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"leg": args.only, "replays": 50 + args.iters, "steps_before_capture": 5, "library_calls_per_iteration": leg["library_calls"],
                          "step_us_device_events": round(e0.elapsed_time(e1) * 1e3 / args.iters, 2)}))
        return
    legs = {"fused": hip_leg(True), "chain": hip_leg(False)}
    eG, eD = eager_nets(dev)
    eog = torch.optim.Adam(eG.parameters(), lr=2e-4, betas=(0.5, 0.999))
    eod = torch.optim.Adam(eD.parameters(), lr=2e-4, betas=(0.5, 0.999))
    bce = nn.BCELoss()
    ones, zeros = torch.ones(bs, 1, device=dev), torch.zeros(bs, 1, device=dev)

    def run(name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if name == "eager":
            for _ in range(n):
                eager_step(eG, eD, eog, eod, bce, real, ones, zeros)
        else:
            gs = legs[name]["gs"]
            for _ in range(n):
                gs.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n, (time.perf_counter() - t0) * 1e6 / n       # us per iteration: device events, wall

    names = ("fused", "chain", "eager")
    for nme in names:                                             # untimed warm-up of every leg
        run(nme, 50)
    ev = {k: [] for k in names}
    wall = {k: [] for k in names}
    for _ in range(args.rounds):                                  # interleaved A/B/C rounds
        for nme in names:
            a, b = run(nme, args.iters)
            ev[nme].append(a); wall[nme].append(b)

    # the whole loop: mnist_gan.train with graph replay, device draws and a reshuffled loader (a tail batch every epoch)
    torch.manual_seed(0)
    G, D = M.Generator().to(dev), M.Discriminator().to(dev)
    loader = DeviceLoader(images.view(n_img, 1, 28, 28), torch.zeros(n_img, device=dev), bs, shuffle=True, seed=0)
    og, od = M.make_optimizers(G, D)
    M.train(G, D, loader, opt_g=og, opt_d=od, epochs=1, graphed=True)     # warm-up: captures both graphs (64 and 32 rows), kept on G
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = M.train(G, D, loader, opt_g=og, opt_d=od, epochs=2, graphed=True)
    torch.cuda.synchronize()
    train_sec = time.perf_counter() - t0
    train_iters = 2 * len(loader)
    if not all(np.isfinite(v) for pair in losses for v in pair):
        sys.exit(f"non-finite losses: {losses}")

    med = {k: statistics.median(v) for k, v in ev.items()}
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in ev.items()}
    flops, skipped = algorithmic_flops(bs)
    it_s = train_iters / train_sec
    print(json.dumps({
        "metric": "training iterations/sec, MNIST MLP GAN (simple_gan/mnist/mnist_gan.py), batch 64; launch/latency bound",
        "value": round(it_s, 1), "unit": "iterations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "rows_per_sec": round(it_s * bs, 1), "us_per_iteration": round(train_sec * 1e6 / train_iters, 2), "train_iterations": train_iters,
        "step_us_device_events": {k: round(v, 2) for k, v in med.items()}, "step_us_min_max": spread,
        "step_us_wall_median": {k: round(statistics.median(v), 2) for k, v in wall.items()},
        "rounds": args.rounds, "iters_per_window": args.iters,
        "fused_vs_chain": round(med["chain"] / med["fused"], 2), "fused_vs_eager": round(med["eager"] / med["fused"], 2),
        "fused_faster_than_chain": med["fused"] < med["chain"], "fused_faster_than_eager": med["fused"] < med["eager"],
        "library_calls_per_iteration": {k: legs[k]["library_calls"] for k in ("fused", "chain")},
        "aten_copies_per_iteration": 1,
        "fewer_calls_than_chain": legs["fused"]["library_calls"] < legs["chain"]["library_calls"],
        "algorithmic_flop_per_iteration": flops, "reference_flop_not_done": skipped,
        "fused_gflops": round(flops / med["fused"] / 1e3, 1),
        "config": {"workload": "simple_gan/mnist/mnist_gan.py:113-139, reference defaults, synthetic 8-bit images, device draws",
                   "global_batch": bs, "parallelism": "dp1"},
        "roofline": {"bound": "launch/latency", "kernel": "one launch per layer and direction, whole batch per workgroup (csrc/dense_rows.hip)"},
        "final_losses": {"g_loss": losses[-1][0], "d_loss": losses[-1][1]},
    }))


if __name__ == "__main__":
    main()
