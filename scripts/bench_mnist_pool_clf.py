#!/usr/bin/env python3
"""The max-pool MNIST classifier (conditional_counteRGAN/mnist/modules/classifier.py, countergan2.py:120-151) against
eager PyTorch on the same GPU, in ONE process, in alternating rounds:

  python scripts/bench_mnist_pool_clf.py [--rounds 5] [--batch 1024] [--fit-rows 12800] [--out profiles/mnist_pool_clf_bench_line.json]

  pool      pcg_relu_maxpool2_fwd / _bwd alone at batch 1024 for both pooling layers ([B,28,28,32] and [B,14,14,64]) against eager
            max_pool2d(relu(z), 2) and its autograd backward (NCHW, as the eager module runs them); device events around `--iters`
            back-to-back launches.  Effective bytes per second = the bytes the operation must move (forward: z read, p and idx written;
            backward: dp, p, idx read, dz written) over the time per launch, next to the rate of the project's BatchNorm apply pass from
            profiles/ (bn_apply_act_fast_kernel: r04_pmc_traffic.json bytes over the 28.8 us of pad_clip_kernel_stats.md)
  eval      countergan.Classifier's eval forward and its input gradient (the guidance path of the GAN step) at batch 1024 against the
            eager module
  fit       one epoch of countergan.fit_pool_classifier at batch 128 on synthetic rows against the eager loop of countergan2.py:127-137
            (torch.optim.Adam, loss.item() per step, as the reference has it)

The baseline of every leg is eager PyTorch in the same process and round.  Inputs and weights are seeded (the MNIST files are not
shipped).  Prints ONE JSON line with the median and every round of each leg; --out also writes it to a file."""
import argparse
import contextlib
import io
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

import _benchlib as BL  # noqa: E402

BN_APPLY_US = 28.8                       # profiles/pad_clip_kernel_stats.md, bn_apply_act_fast_kernel<2, false>


def bn_apply_rate():
    """Bytes per second of the BatchNorm apply pass, from the committed profiles."""
    with open(os.path.join(ROOT, "profiles", "r04_pmc_traffic.json")) as f:
        k = json.load(f)["bn_apply_act_fast_kernel<2, false>"]
    return (k["fetch_bytes_per_launch"] + k["write_bytes_per_launch"]) / (BN_APPLY_US * 1e-6)


def eager_module():
    """modules/classifier.py:7-18 in eager PyTorch."""
    return nn.Sequential(nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
                         nn.Flatten(), nn.Linear(64 * 7 * 7, 128), nn.ReLU(), nn.Linear(128, 10))


def event_ms(fn, iters):
    """Milliseconds per call of fn from device events around `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4),
            "all": [round(float(s), 4) for s in v]}


def alternate(legs, rounds, measure):
    """{name: [one measurement per round]}: every round runs every leg once, in the same order."""
    for fn in legs.values():
        measure(fn)                                                             # warm-up: code objects, allocator, algorithm choices
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(measure(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fit-rows", type=int, default=12800)
    ap.add_argument("--fit-batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import countergan as K
    ops = pcgan_amd.ops
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(0)
    result = {}

    # ---- the pooling kernels alone ------------------------------------------------------------------------------------------------------
    for name, (H, W, C) in (("pool1", (28, 28, 32)), ("pool2", (14, 14, 64))):
        z = torch.randn(B, H, W, C, generator=g).to(dev)
        dp = torch.randn(B, H // 2, W // 2, C, generator=g).to(dev)
        p, idx = ops.relu_maxpool2_fwd(z)
        dz = torch.empty_like(z)
        zt = z.permute(0, 3, 1, 2).contiguous().requires_grad_(True)             # the eager module's layout: NCHW
        dpt = dp.permute(0, 3, 1, 2).contiguous()
        pt = F.max_pool2d(torch.relu(zt), 2)
        if not torch.equal(pt.detach().permute(0, 2, 3, 1), p):
            sys.exit(f"{name}: the kernel's pooled tensor is not eager PyTorch's")
        if not torch.equal(torch.autograd.grad(pt, zt, dpt, retain_graph=True)[0].permute(0, 2, 3, 1), ops.relu_maxpool2_bwd(dp, p, idx, (H, W))):
            sys.exit(f"{name}: the kernel's gradient is not eager PyTorch's")
        legs = {"hip_fwd": lambda: ops.relu_maxpool2_fwd(z, out=p, idx=idx),
                "eager_fwd": lambda: F.max_pool2d(torch.relu(zt.detach()), 2),
                "hip_bwd": lambda: ops.relu_maxpool2_bwd(dp, p, idx, (H, W), out=dz),
                "eager_bwd": lambda: torch.autograd.grad(pt, zt, dpt, retain_graph=True)}
        ms = alternate(legs, args.rounds, lambda fn: event_ms(fn, args.iters))
        n, npool = z.numel(), p.numel()
        fwd_bytes, bwd_bytes = 4 * n + 5 * npool, 9 * npool + 4 * n
        st = {k: stats(v) for k, v in ms.items()}
        result[name] = {"shape_nhwc": [B, H, W, C], "ms_per_launch": st, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
                        "hip_fwd_TBps": round(fwd_bytes / st["hip_fwd"]["median"] / 1e9, 3), "hip_bwd_TBps": round(bwd_bytes / st["hip_bwd"]["median"] / 1e9, 3),
                        "fwd_vs_eager": round(st["eager_fwd"]["median"] / st["hip_fwd"]["median"], 3),
                        "bwd_vs_eager": round(st["eager_bwd"]["median"] / st["hip_bwd"]["median"], 3)}

    # ---- eval forward and input gradient at batch 1024 --------------------------------------------------------------------------------------
    torch.manual_seed(5)
    eager = eager_module().to(dev).eval()
    net = K.Classifier()
    net.load_state_dict({"net." + k: v for k, v in eager.state_dict().items()}, strict=True)
    net = net.to(dev).eval()
    for q in list(net.parameters()) + list(eager.parameters()):
        q.requires_grad = False
    x = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).to(dev)
    dl = torch.randn(B, 10, generator=g).to(dev)

    def fwd(m):
        with torch.no_grad():
            return m(x)

    def fwd_bwd(m):
        xi = x.detach().clone().requires_grad_(True)
        m(xi).backward(dl)
        return xi.grad
    if not torch.allclose(fwd(net), fwd(eager), rtol=1e-3, atol=1e-4):
        sys.exit("eval: the logits disagree with the eager module")
    legs = {"hip_forward": lambda: fwd(net), "eager_forward": lambda: fwd(eager),
            "hip_forward_input_grad": lambda: fwd_bwd(net), "eager_forward_input_grad": lambda: fwd_bwd(eager)}
    st = {k: stats(v) for k, v in alternate(legs, args.rounds, lambda fn: event_ms(fn, max(args.iters // 5, 1))).items()}
    result["eval"] = {"batch": B, "ms_per_call": st, "forward_vs_eager": round(st["eager_forward"]["median"] / st["hip_forward"]["median"], 3),
                      "forward_input_grad_vs_eager": round(st["eager_forward_input_grad"]["median"] / st["hip_forward_input_grad"]["median"], 3)}

    # ---- one epoch of the fit at batch 128 ------------------------------------------------------------------------------------------------------
    R, b = args.fit_rows, args.fit_batch
    X = (torch.rand(R, 1, 28, 28, generator=g) * 2 - 1).to(dev)
    Y = torch.randint(0, 10, (R,), generator=g).to(dev)
    train = [(X[i:i + b], Y[i:i + b]) for i in range(0, R, b)]
    valid = train[:max(len(train) // 10, 1)]
    init = {k: v.detach().clone() for k, v in eager.state_dict().items()}

    def hip_fit():
        c = K.Classifier()
        c.load_state_dict({"net." + k: v for k, v in init.items()}, strict=True)
        with contextlib.redirect_stdout(io.StringIO()):
            return K.fit_pool_classifier(c, train, valid, epochs=1, lr=1e-3, device=dev)

    def eager_fit():
        c = eager_module().to(dev)
        c.load_state_dict(init)
        opt, crit = torch.optim.Adam(c.parameters(), lr=1e-3), nn.CrossEntropyLoss()
        c.train()
        tl = vl = 0.0
        for xb, yb in train:
            loss = crit(c(xb), yb)
            opt.zero_grad()
            loss.backward()
            opt.step()
            tl += loss.item() * xb.size(0)
        c.eval()
        with torch.no_grad():
            for xb, yb in valid:
                vl += crit(c(xb), yb).item() * xb.size(0)
        return [tl / R], [vl / sum(len(v[1]) for v in valid)]
    losses = {"hip": hip_fit(), "eager": eager_fit()}
    if not np.allclose(losses["hip"], losses["eager"], rtol=2e-2):
        sys.exit(f"fit: the epoch losses disagree: {losses}")
    st = {k: stats(v) for k, v in alternate({"hip_epoch": hip_fit, "eager_epoch": eager_fit}, args.rounds, wall_ms).items()}
    result["fit"] = {"rows": R, "batch": b, "steps": len(train), "ms_per_epoch": st, "epoch_vs_eager": round(st["eager_epoch"]["median"] / st["hip_epoch"]["median"], 3),
                     "losses_train_valid": {k: [round(float(v[0][0]), 5), round(float(v[1][0]), 5)] for k, v in losses.items()}}

    bn = bn_apply_rate()
    line = json.dumps({
        "metric": f"classifier epochs/sec, max-pool MNIST classifier fit (countergan2.py:120-151), {R} rows, batch {b}",
        "value": round(1e3 / result["fit"]["ms_per_epoch"]["hip_epoch"]["median"], 3), "unit": "epochs/sec", "n_gpus": 1, "higher_is_better": True,
        "dtype": "f32", "rounds": args.rounds, "iters_per_round": args.iters, **result,
        "bn_apply_pass_TBps": round(bn / 1e12, 3),
        "config": {"workload": "conditional_counteRGAN/mnist modules/classifier.py + countergan2.py:120-151, seeded weights and inputs",
                   "parallelism": "dp1", "baseline": "eager PyTorch on the same GPU, same process, alternating rounds"},
        "roofline": {"bound": "hbm", "peak": BL.PEAK_HBM_GBS, "unit": "GB/s", "kernel": "relu_maxpool2_fwd_kernel / relu_maxpool2_bwd_kernel",
                     "achieved": {k: {"fwd": round(result[k]["hip_fwd_TBps"] * 1e3, 1), "bwd": round(result[k]["hip_bwd_TBps"] * 1e3, 1)} for k in ("pool1", "pool2")}},
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
