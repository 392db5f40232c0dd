#!/usr/bin/env python3
"""The image sheets against the two ways to get the same pixels without them, in ONE process, in alternating rounds:

  python scripts/bench_sheets.py [--rounds 5] [--reps 100] [--out profiles/image_sheet_bench_line.json]

  hip     pcgan_amd.sheets.sheet_u8(x, normalize=True): the range pass and the sheet pass of csrc/image_sheet.hip, then ONE download of
          the uint8 image
  eager   the same algorithm in eager torch ops on the GPU: min and max with their two .item() reads, clamp, subtract, divide, the
          channel repeat, a filled grid and one slice copy per image, the quantisation, then the same download
  host    what a user of this package did before: .cpu() of the float batch, then make_grid / save_image's arithmetic on the CPU
          (tests/sheet_restate.py)

for the DCGAN visualisation sheet (64 x 1 x 64 x 64, padding 2: mnist_dcgan.py:190) and the 16-image nrow=4 sheet of the CounteRGANs
(gan_train.py:161).  A round times --reps sheets of every leg; the figure is microseconds per sheet.  The three legs must give the
same pixels.  Prints ONE JSON line with the median, the spread and every round of each leg, and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sheet_restate as SR  # noqa: E402

WORKLOADS = {"dcgan_viz_64x1x64x64": dict(shape=(64, 1, 64, 64), nrow=8, padding=2),
             "countergan_16x1x28x28_nrow4": dict(shape=(16, 1, 28, 28), nrow=4, padding=2)}


def eager_sheet(x, nrow, padding, count=None):
    """make_grid(normalize=True) + save_image's pixels in eager torch ops on the GPU.  count (a list): gets the number of device
    operations issued (kernel launches and the two scalar downloads)."""
    n = 0
    lo, hi = float(x.min().item()), float(x.max().item()); n += 4
    d = torch.full((), max(hi - lo, 1e-5), dtype=torch.float64).to(torch.float32).item()
    t = x.clamp(lo, hi).sub_(lo); n += 2
    t = torch.true_divide(t, torch.full_like(t, d)); n += 2                   # a tensor of divisors: a division, not a reciprocal product
    N, C, H, W = t.shape
    if C == 1:
        t = t.expand(N, 3, H, W)
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    ch, cw = H + padding, W + padding
    grid = torch.zeros((3, ymaps * ch + padding, xmaps * cw + padding), dtype=torch.float32, device=x.device); n += 1
    for k in range(N):
        yy, xx = divmod(k, xmaps)
        grid[:, yy * ch + padding:yy * ch + padding + H, xx * cw + padding:xx * cw + padding + W] = t[k]; n += 1
    u8 = grid.mul(255.0).add_(0.5).clamp_(0.0, 255.0).permute(1, 2, 0).to(torch.uint8).contiguous(); n += 5
    if count is not None:
        count.append(n)
    return u8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_sheet_bench_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: torch.cuda.is_available() is False (there is no CPU path)")
    import pcgan_amd
    from pcgan_amd import sheets
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))

    def stats(v):
        v = np.asarray(v) * 1e6 / args.reps
        return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2),
                "all": [round(float(s), 2) for s in v]}

    out = {}
    for name, w in WORKLOADS.items():
        x = torch.tanh(torch.randn(w["shape"], generator=torch.Generator().manual_seed(1))).to(dev)
        kw = dict(nrow=w["nrow"], padding=w["padding"])
        ops_issued = []
        legs = {"hip": lambda: sheets.sheet_u8(x, normalize=True, **kw).cpu(),
                "eager": lambda: eager_sheet(x, **kw).cpu(),
                "host": lambda: SR.sheet_u8(x.cpu(), normalize=True, **kw)}
        pix = {k: leg() for k, leg in legs.items()}                           # warm-up, and the pixels
        eager_sheet(x, count=ops_issued, **kw)
        if not (torch.equal(pix["hip"], pix["host"]) and torch.equal(pix["eager"], pix["host"])):
            sys.exit(f"{name}: the legs disagree on the pixels")
        secs = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    leg()
                torch.cuda.synchronize()
                secs[k].append(time.perf_counter() - t0)
        us = {k: stats(v) for k, v in secs.items()}
        out[name] = {"us_per_sheet": us, "pixels_equal": True,
                     "launches_per_sheet": {"hip": 2, "eager": ops_issued[0], "host": 0},
                     "host_copies_per_sheet": {"hip": "1 (uint8 image)", "eager": "2 scalar reads + 1 (uint8 image)", "host": "1 (float batch)"},
                     "eager_vs_hip": round(us["eager"]["median"] / us["hip"]["median"], 2),
                     "host_vs_hip": round(us["host"]["median"] / us["hip"]["median"], 2),
                     "hip_faster_than_eager_by_more_than_the_spread":
                         bool(us["eager"]["median"] - us["hip"]["median"] > max(us[k]["max"] - us[k]["min"] for k in ("hip", "eager"))),
                     "hip_faster_than_host_by_more_than_the_spread":
                         bool(us["host"]["median"] - us["hip"]["median"] > max(us[k]["max"] - us[k]["min"] for k in ("hip", "host")))}
    first = out["dcgan_viz_64x1x64x64"]
    line = {"metric": "sheets/sec, make_grid(normalize=True) + uint8 pixels + download, 64 x 1 x 64 x 64, padding 2",
            "value": round(1e6 / first["us_per_sheet"]["hip"]["median"], 1), "unit": "sheets/sec", "n_gpus": 1, "higher_is_better": True,
            "dtype": "f32", "rounds": args.rounds, "reps_per_round": args.reps, "workloads": out,
            "config": {"workload": "tanh of seeded normal draws resident on the device", "parallelism": "dp1",
                       "baseline": "eager: the same algorithm in torch ops on the GPU; host: .cpu() of the float batch + the CPU restatement",
                       "eager launch count": "operations issued by the eager leg, counted in the script, not traced"},
            "roofline": {"bound": "launch latency (about 1 MB in, about 4 MB out for the larger sheet); not analysed further",
                         "kernel": "image_range_kernel, image_sheet_kernel in csrc/image_sheet.hip"}}
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
