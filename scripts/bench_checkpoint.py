#!/usr/bin/env python3
"""Wall time of one checkpoint write and one resume (pcgan_amd.checkpoint) next to a plain torch.save / torch.load
of the same nets' state_dict() plus a torch.optim.Adam state of the same size.

  python scripts/bench_checkpoint.py [--repeats 5] [--dir DIR]

Two pairs of nets: the DCGAN generator + discriminator at the bench widths (g_hidden = d_hidden = 64, z = 100) and the WGAN-GP
critic + generator at the reference width 1024 (the critic: 25 M parameters).  Every optimizer has made one step, so the moments
exist.  time.perf_counter around the call with a device synchronise on both sides; the median of the repeats.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def torch_adam_state(net):
    """A torch.optim.Adam state_dict of the net's size (step 1, moments on the parameters' device)."""
    ps = list(net.parameters())
    state = {i: {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p).contiguous(), "exp_avg_sq": torch.zeros_like(p).contiguous()}
             for i, p in enumerate(ps)}
    return {"state": state, "param_groups": [dict(torch.optim.Adam([torch.zeros(1)]).defaults, params=list(range(len(ps))))]}


def measure(name, nets, opts, repeats, folder):
    from pcgan_amd import checkpoint
    for net, opt in zip(nets, opts):
        net.zero_grad()
        opt.step()                                            # builds the segments: the moments exist (zero gradients: nothing moves)
    named = {f"net{i}": n for i, n in enumerate(nets)}
    named.update({f"opt{i}": o for i, o in enumerate(opts)})
    path, plain = os.path.join(folder, f"{name}.pt"), os.path.join(folder, f"{name}_plain.pt")
    write = timed(lambda: checkpoint.save(path, checkpoint.capture(epoch=1, **named)), repeats)
    resume = timed(lambda: checkpoint.restore(checkpoint.load(path), **named), repeats)
    topts = [torch.optim.Adam(n.parameters()) for n in nets]

    def plain_write():
        torch.save({"nets": [n.state_dict() for n in nets], "opts": [torch_adam_state(n) for n in nets]}, plain)

    def plain_resume():
        d = torch.load(plain, map_location="cpu", weights_only=True)
        for n, o, sd, od in zip(nets, topts, d["nets"], d["opts"]):
            n.load_state_dict(sd)
            o.load_state_dict(od)

    pw, pr = timed(plain_write, repeats), timed(plain_resume, repeats)
    return {"parameters": sum(p.numel() for n in nets for p in n.parameters()), "file_MB": round(os.path.getsize(path) / 1e6, 1),
            "write_ms": round(write, 1), "resume_ms": round(resume, 1), "torch_save_ms": round(pw, 1), "torch_load_ms": round(pr, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    args = ap.parse_args(argv)
    import pcgan_amd
    from pcgan_amd import dcgan, wgan
    pcgan_amd.load()
    dev = torch.device("cuda:0")
    out = {}
    with tempfile.TemporaryDirectory(dir=args.dir) as folder:
        netG, netD = dcgan.build(device=dev, seed=1)
        _, optD, optG = dcgan.make_optimizers(netG, netD)
        out["dcgan"] = measure("dcgan", [netG, netD], [optG, optD], args.repeats, folder)
        critic, generator = wgan.build(dev, wgan.Hyperparameter(critic_size=1024, generator_size=1024, critic_hidden_size=1024))
        c_opt, g_opt = wgan.make_optimizers(critic, generator)
        out["wgan"] = measure("wgan", [critic, generator], [c_opt, g_opt], args.repeats, folder)
    print(json.dumps({"metric": "checkpoint write / resume wall time, median", "unit": "ms", "repeats": args.repeats, **out}))


if __name__ == "__main__":
    main()
