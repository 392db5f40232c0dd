#!/usr/bin/env python3
"""Training iterations/s of the moons CounteRGAN (conditional_counteRGAN/moons/trainer.py:31-128) on one MI355X, at the reference
configuration: batch 64, hidden 32, 15 iterations per epoch, 500 epochs.

  python scripts/bench_moons_cf.py [--epochs 500] [--warmup-epochs 2] [--eager-epochs 20]

Legs, all in this process on one GPU:
  fused    moons_countergan.train_countergan (one pcg_moons_cf_train_steps launch per epoch + its draws), wall clock over the epochs
  kernel   the bare step kernel at n_steps = 15 (one epoch per launch), device events around 20 launches
  eager    the same loop body in eager PyTorch on the GPU (the nets restated here; torch.optim.Adam, nn.utils.spectral_norm)
One JSON line, the contract of scripts/bench_house.py.  The step is launch/latency bound: no MFMA or roofline claim."""
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


def eager_nets(H, dev):
    sn = nn.utils.spectral_norm
    G = nn.Sequential(nn.Linear(7, H), nn.BatchNorm1d(H), nn.ReLU(), nn.Linear(H, H), nn.BatchNorm1d(H), nn.ReLU(),
                      nn.Linear(H, H // 2), nn.BatchNorm1d(H // 2), nn.ReLU(), nn.Linear(H // 2, 2))
    D = nn.Sequential(sn(nn.Linear(5, H)), nn.LeakyReLU(0.2, inplace=True), sn(nn.Linear(H, H // 2)), nn.LeakyReLU(0.2, inplace=True),
                      sn(nn.Linear(H // 2, H // 2)), nn.LeakyReLU(0.2, inplace=True), sn(nn.Linear(H // 2, 1)))
    C = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3))
    return G.to(dev), D.to(dev), C.to(dev).eval()


def eager_epoch(G, D, C, opt_G, opt_D, X, Y, cfg, bs):
    """trainer.py:58-116 on the GPU, eager (the reference's .item() reads included)."""
    N = X.shape[0]
    perm = torch.randperm(N, device=X.device)
    dl, gl = [], []
    for b in range(N // bs):
        idx = perm[b * bs:(b + 1) * bs]
        x, y = X[idx], Y[idx]
        t = torch.randint(0, 3, (bs,), device=X.device)
        t = torch.where(t == y, (t + 1) % 3, t)
        oh = F.one_hot(t, 3).float()
        m = torch.randint(0, 2, (bs, 2), device=X.device).float()
        raw = G(torch.cat([x, oh, m], 1))
        masked = raw * m
        pen = torch.mean(torch.abs(raw * (1.0 - m)))
        x_cf = x + masked
        D_real = D(torch.cat([x, F.one_hot(y, 3).float()], 1))
        D_fake = D(torch.cat([x_cf.detach(), oh], 1))
        D_loss = -D_real.mean() + D_fake.mean()
        opt_D.zero_grad(); D_loss.backward(); opt_D.step()
        adv = -D(torch.cat([x_cf, oh], 1)).mean()
        cls = F.cross_entropy(C(x_cf), t)
        l1 = torch.mean(torch.norm(masked, p=1, dim=1))
        l2 = torch.mean(torch.norm(masked, p=2, dim=1))
        G_loss = adv + cfg["lambda_cls"] * cls + cfg["lambda_reg_l1"] * l1 + cfg["lambda_reg_l2"] * l2 + cfg["lambda_mask"] * pen
        opt_G.zero_grad(); G_loss.backward(); opt_G.step()
        dl.append(D_loss.item()); gl.append(G_loss.item())
        with torch.no_grad():
            torch.sigmoid(D_real).mean().item(); torch.sigmoid(D_fake).mean().item()
        adv.item(); cls.item(); l1.item(); l2.item(); pen.item()
    return float(np.mean(dl)), float(np.mean(gl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--warmup-epochs", type=int, default=2)
    ap.add_argument("--eager-epochs", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=32)
    args = ap.parse_args()
    import pcgan_amd
    from pcgan_amd import moons_countergan as M
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    X_train, _, y_train, _ = M.load_and_preprocess(42)
    bs, H = 64, args.hidden
    per_epoch = len(X_train) // bs
    cfg = dict(M.config, hidden_dim=H, cuda=str(dev))

    def fused(epochs):
        torch.manual_seed(0)
        G, C = M.ResidualGenerator(2, H, 3), M.NNClassifier(2)
        c = dict(cfg, epochs=epochs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = M.train_countergan(G, c, X_train, y_train, C, verbose=False, save=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    fused(args.warmup_epochs)
    sec, res = fused(args.epochs)
    iters = args.epochs * per_epoch
    losses = {"D_loss": res["d_losses"][-1], "G_loss": res["g_losses"][-1]}
    if not all(np.isfinite(v) for v in losses.values()):
        sys.exit(f"non-finite losses: {losses}")

    # bare kernel, one epoch (15 iterations) per launch
    torch.manual_seed(0)
    G, D, C = M.ResidualGenerator(2, H, 3).to(dev), M.Discriminator(2, H, 3).to(dev), M.NNClassifier(2).to(dev)
    ts = M.TrainSteps(G, D, C, M.Adam(G.parameters(), lr=1e-3), M.Adam(D.parameters(), lr=1e-3), X_train, y_train, cfg)
    g = torch.Generator().manual_seed(1)
    rows = torch.randperm(len(X_train), generator=g)[:per_epoch * bs].view(per_epoch, bs).to(dev)
    ty = torch.remainder(ts.Y[rows.view(-1)] + 1, 3).view(per_epoch, bs)
    mk = torch.randint(0, 2, (per_epoch, bs, 2), generator=g).float().to(dev)
    for _ in range(3):
        ts.run(rows, ty, mk, check=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n_launch = 20
    e0.record()
    for _ in range(n_launch):
        ts.run(rows, ty, mk, check=False)
    e1.record()
    torch.cuda.synchronize()
    kernel_us = e0.elapsed_time(e1) * 1e3 / (n_launch * per_epoch)

    # eager PyTorch on the GPU
    torch.manual_seed(0)
    eG, eD, eC = eager_nets(H, dev)
    oG, oD = torch.optim.Adam(eG.parameters(), lr=1e-3), torch.optim.Adam(eD.parameters(), lr=1e-3)
    Xd = torch.tensor(X_train, dtype=torch.float32, device=dev)
    Yd = torch.tensor(y_train, dtype=torch.long, device=dev)
    eager_epoch(eG, eD, eC, oG, oD, Xd, Yd, cfg, bs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.eager_epochs):
        eager_epoch(eG, eD, eC, oG, oD, Xd, Yd, cfg, bs)
    torch.cuda.synchronize()
    eager_sec = (time.perf_counter() - t0) / (args.eager_epochs * per_epoch)

    it_s = iters / sec
    print(json.dumps({
        "metric": "training iterations/sec, moons CounteRGAN (conditional_counteRGAN/moons), batch 64; launch/latency bound",
        "value": round(it_s, 1), "unit": "iterations/sec", "n_gpus": 1, "higher_is_better": True, "dtype": "f32",
        "rows_per_sec": round(it_s * bs, 1), "us_per_iteration": round(sec * 1e6 / iters, 2),
        "kernel_us_per_iteration": round(kernel_us, 2), "kernel_n_steps": per_epoch,
        "launches_per_epoch": {"step_kernel": 1, "draws": 2, "row_gather_index": 1, "copies": 2},
        "eager_iterations_per_sec": round(1.0 / eager_sec, 1), "fused_vs_eager": round(it_s * eager_sec, 2),
        "epochs": args.epochs, "iterations": iters, "eager_epochs": args.eager_epochs,
        "config": {"workload": f"conditional_counteRGAN/moons trainer.py:31-128, hidden {H}, batch {bs}, {per_epoch} iterations per epoch, "
                               "per-epoch device draws", "global_batch": bs, "parallelism": "dp1"},
        "roofline": {"bound": "launch/latency", "kernel": "one workgroup runs every iteration of an epoch (csrc/moons_cf.hip)"},
        "final_losses": losses,
    }))


if __name__ == "__main__":
    main()
