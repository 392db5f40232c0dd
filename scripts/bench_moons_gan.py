#!/usr/bin/env python3
"""Training iterations/s of the moons GAN (simple_gan/moons/make_moons_gan.py) and the moons conditional GAN
(conditional_gan/moons/make_moons_cgan.py) on one MI355X, at the reference configuration: batch 50, hidden 128, z_dim 32,
40 iterations per epoch, 500 epochs.

  python scripts/bench_moons_gan.py [--epochs 500] [--batch 50] [--rounds 5] [--round-epochs 10] [--chain-iters 80]

Legs, all in this process on one GPU:
  fused     moons.train_gan / moons_cgan.train (one pcg_moons_gan_train_steps launch per epoch + its draws): wall clock of the full run
  kernel    the bare step kernel at n_steps = one epoch, device events around 20 launches
  rounds    interleaved, `--rounds` times: fused (`--round-epochs` epochs through train_gan / train), the op chain (moons.train_step in
            a loop: every Linear a 1x1 convolution, separate ReLU / Sigmoid / BCE / Adam launches under autograd — the only path
            before the fused one; it has no conditional form, so the conditional GAN is compared against the same, cheaper, chain)
            and eager PyTorch (the scripts' loop bodies restated with torch.nn / torch.optim.Adam, their .item() reads included);
            median and min..max of the rounds per leg
  quality   reported only: mean distance from 2000 generated points to their nearest real point after the full run
One JSON line, the contract of scripts/bench_moons_cf.py.  The step is launch/latency bound: no MFMA or roofline claim."""
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


def eager_nets(Z, L, H, dev):
    G = nn.Sequential(nn.Linear(Z + L, H), nn.ReLU(), nn.Linear(H, 2)).to(dev)
    D = nn.Sequential(nn.Linear(2 + L, H), nn.ReLU(), nn.Linear(H, 1), nn.Sigmoid()).to(dev)
    return G, D, torch.optim.Adam(G.parameters(), lr=1e-3), torch.optim.Adam(D.parameters(), lr=1e-3)


def eager_iters(nets, X, Y, Z, L, bs, n):
    """make_moons_gan.py:62-88 / make_moons_cgan.py:91-129 on the GPU, eager, n iterations."""
    G, D, oG, oD = nets
    dev = X.device
    cat = (lambda a, oh: torch.cat([a, oh], 1)) if L else (lambda a, oh: a)
    tD = tG = 0
    for i in range(n):
        s = (i * bs) % (X.shape[0] - bs + 1)
        real = X[s:s + bs]
        oh_r = F.one_hot(Y[s:s + bs], L).float() if L else None
        z = torch.randn(bs, Z).to(dev)
        oh = F.one_hot(torch.randint(0, 1, (bs,)).to(dev), L).float() if L else None
        fake = G(cat(z, oh))
        loss_D = -torch.mean(torch.log(D(cat(real, oh_r))) + torch.log(1 - D(cat(fake.detach() if L else fake, oh))))
        oD.zero_grad(); loss_D.backward(); oD.step()
        tD += loss_D.item()
        z = torch.randn(bs, Z).to(dev)
        oh = F.one_hot(torch.randint(0, L, (bs,)).to(dev), L).float() if L else None
        loss_G = -torch.mean(torch.log(D(cat(G(cat(z, oh)), oh))))
        oG.zero_grad(); loss_G.backward(); oG.step()
        tG += loss_G.item()
    return tD, tG


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-epochs", type=int, default=10)
    ap.add_argument("--chain-iters", type=int, default=80)
    args = ap.parse_args()
    import pcgan_amd
    from pcgan_amd import moons as M, moons_cgan as C, ops
    from pcgan_amd.moons_countergan import make_moons
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    bs, Z, H = args.batch, 32, 128
    n_samples = 2000 if 2000 % bs == 0 else (2000 // bs + 1) * bs
    per_epoch = n_samples // bs
    np.random.seed(9)
    X64, Y = make_moons(n_samples, noise=0.05)
    Xd, Yd = torch.tensor(X64, dtype=torch.float32, device=dev), torch.tensor(Y, dtype=torch.long, device=dev)
    calls = []
    real_check = ops.check

    def counting_check(rc, what=""):
        calls.append(what)
        return real_check(rc, what)

    def nets(L):
        torch.manual_seed(0)
        if L:
            return C.Generator(Z, L, H).to(dev), C.Discriminator(L, H).to(dev)
        return M.build_generator(Z, H).to(dev), M.build_discriminator(H).to(dev)

    def fused(L, epochs, seed=0):
        G, D = nets(L)
        cfg = dict(C.config if L else M.config, n_samples=n_samples, batch_size=bs, epochs=epochs)
        np.random.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if L:
            lD, lG = C.train(torch.from_numpy(X64).float(), torch.from_numpy(Y), G, D, cfg, seed=seed, verbose=False)
        else:
            lD, lG = M.train_gan(X64.copy(), G, D, cfg, seed=seed)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lD, lG, G

    def chain_setup():
        G, D = nets(0)
        return G, D, *M.make_optimizers(G, D)

    def chain_iters(st, n):
        G, D, oG, oD = st
        tD = tG = 0
        for i in range(n):
            s = (i * bs) % (n_samples - bs + 1)
            lD, lG = M.train_step(G, D, oG, oD, Xd[s:s + bs].contiguous(), torch.randn(bs, Z).to(dev), torch.randn(bs, Z).to(dev))
            tD += lD.item(); tG += lG.item()
        return tD, tG

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {}
    chain = chain_setup()
    eager = {L: eager_nets(Z, L, H, dev) for L in (0, 2)}
    # warm-up of every leg (library load, allocator, first-launch costs), and the library calls of one fused epoch
    chain_iters(chain, 10)
    for L in (0, 2):
        eager_iters(eager[L], Xd, Yd, Z, L, bs, 10)
        fused(L, 2)
        ops.check = counting_check
        del calls[:]
        fused(L, 3)
        ops.check = real_check
        per = {k: calls.count(k) // 3 for k in ("pcg_moons_gan_train_steps", "pcg_randn", "pcg_randint")}
        out[L] = {"library_calls_per_epoch": per}
    rounds = {"fused_gan": [], "fused_cgan": [], "op_chain": [], "eager_gan": [], "eager_cgan": []}
    for _ in range(args.rounds):
        rounds["fused_gan"].append(fused(0, args.round_epochs)[0] * 1e6 / (args.round_epochs * per_epoch))
        rounds["op_chain"].append(timed(lambda: chain_iters(chain, args.chain_iters)) * 1e6 / args.chain_iters)
        rounds["eager_gan"].append(timed(lambda: eager_iters(eager[0], Xd, Yd, Z, 0, bs, args.chain_iters)) * 1e6 / args.chain_iters)
        rounds["fused_cgan"].append(fused(2, args.round_epochs)[0] * 1e6 / (args.round_epochs * per_epoch))
        rounds["eager_cgan"].append(timed(lambda: eager_iters(eager[2], Xd, Yd, Z, 2, bs, args.chain_iters)) * 1e6 / args.chain_iters)
    us = {k: spread(v) for k, v in rounds.items()}

    results = {}
    for L, name in ((0, "gan"), (2, "cgan")):
        sec, lD, lG, G = fused(L, args.epochs)
        iters = args.epochs * per_epoch
        if not (np.isfinite(lD).all() and np.isfinite(lG).all()):
            sys.exit(f"non-finite losses ({name})")
        # the bare kernel, one epoch per launch
        G2, D2 = nets(L)
        ts = M.TrainSteps(G2, D2, *M.make_optimizers(G2, D2), X64, Y if L else None, batch_size=bs)
        g = torch.Generator().manual_seed(1)
        rows = torch.randperm(n_samples, generator=g).view(per_epoch, bs).to(dev)
        z = torch.randn(per_epoch, 2, bs, Z, generator=g).to(dev)
        lab = torch.randint(0, 2, (per_epoch, 2, bs), generator=g).to(dev) if L else None
        for _ in range(3):
            ts.run(rows, z, lab, check=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_launch = 20
        e0.record()
        for _ in range(n_launch):
            ts.run(rows, z, lab, check=False)
        e1.record()
        torch.cuda.synchronize()
        kernel_us = e0.elapsed_time(e1) * 1e3 / (n_launch * per_epoch)
        with torch.no_grad():
            pts = C.sample(G, 2000)[0] if L else M.sample(G, 2000)
            nearest = float(torch.cdist(pts, Xd).min(1).values.mean())
        f, c, e = us["fused_" + name], us["op_chain"], us["eager_" + name]
        results[name] = {
            "iterations_per_sec": round(iters / sec, 1), "us_per_iteration": round(sec * 1e6 / iters, 2),
            "kernel_us_per_iteration": round(kernel_us, 2), "kernel_n_steps": per_epoch, "activation_scratch_bytes": ts.scratch_bytes,
            "rounds_us_per_iteration": {"fused": f, "op_chain": c, "eager": e},
            "fused_vs_op_chain": round(c["median"] / f["median"], 2), "fused_vs_eager": round(e["median"] / f["median"], 2),
            "faster_than_op_chain_by_more_than_the_spread": bool(f["max"] < c["min"]),
            "library_calls_per_epoch": out[L]["library_calls_per_epoch"],
            "copies_per_epoch": {"rows_h2d": 1, "logs_d2h": 1},
            "final_epoch_losses": {"loss_D": round(lD[-1], 4), "loss_G": round(lG[-1], 4)},
            "mean_nearest_real_distance_2000": round(nearest, 4),
        }
    print(json.dumps({
        "metric": f"training iterations/sec, moons GAN (simple_gan/moons), batch {bs}; launch/latency bound",
        "value": results["gan"]["iterations_per_sec"], "unit": "iterations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "gan": results["gan"], "cgan": results["cgan"],
        "epochs": args.epochs, "iterations": args.epochs * per_epoch, "rounds": args.rounds, "round_epochs": args.round_epochs,
        "chain_iters": args.chain_iters,
        "config": {"workload": f"make_moons_gan.py:49-93 and make_moons_cgan.py:81-135, hidden {H}, z_dim {Z}, batch {bs}, {per_epoch} iterations "
                               f"per epoch over {n_samples} rows, per-epoch device draws", "global_batch": bs, "parallelism": "dp1"},
        "roofline": {"bound": "launch/latency", "kernel": "one workgroup runs every iteration of an epoch, six barrier-separated phases each "
                                                          "(csrc/moons_gan.hip)"},
    }))


if __name__ == "__main__":
    main()
