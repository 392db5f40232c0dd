#!/usr/bin/env python3
"""Records tests/golden/moons_cgan_ref.npz from the reference's own code (CPU, fp32, one thread): four iterations of
conditional_gan/moons/make_moons_cgan.py at its own configuration (batch 50, z_dim 32, hidden 128, two labels) on moons-shaped data.

    python tests/golden/make_golden_moons_cgan.py /path/to/reference/checkout

`Generator`, `Discriminator` (:35-60), `one_hot_encode` (:62-63) and the body of the batch loop (:91-129) are lifted out of the script
with `ast` and executed here; the script itself is never imported (it trains and plots at import and pulls scikit-learn and
matplotlib).  No reference text is stored.  The loop body draws z and the fake labels from torch's global generator (:97-98, :116-117):
it is seeded before every iteration and the four draws are replayed first to record them."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import moons_gan_restate as RS  # noqa: E402


def lift(ref):
    path = os.path.join(ref, "conditional_gan/moons/make_moons_cgan.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name in ("Generator", "Discriminator")) or
            (isinstance(n, ast.FunctionDef) and n.name == "one_hot_encode")]
    body = []
    for node in tree.body:
        if isinstance(node, ast.For) and node.lineno == 83:
            inner = [n for n in node.body if isinstance(n, ast.For)]
            assert len(inner) == 1 and inner[0].lineno == 90, "reference layout changed"
            body = [n for n in inner[0].body if 91 <= n.lineno <= 129]
    assert len(defs) == 3 and body and body[0].lineno == 91 and body[-1].end_lineno == 129, "reference layout changed"
    config = {"n_samples": RS.ITERS * RS.BATCH, "z_dim": RS.Z_DIM, "hidden_dim": RS.HIDDEN, "label_dim": RS.LABEL_DIM, "batch_size": RS.BATCH,
              "lr": RS.LR, "epochs": 1, "scale_factor": 10}                                                         # :10-19, a 4-batch set
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "np": np, "config": config, "device": torch.device("cpu")}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns, compile(ast.Module(body=body, type_ignores=[]), path, "exec"), config


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(HERE, "moons_cgan_ref.npz"))
    ap.add_argument("--seed", type=int, default=RS.SEED)
    a = ap.parse_args()
    ns, step_code, config = lift(a.reference)
    torch.set_num_threads(1)                       # the CPU GEMMs' summation order depends on the thread count
    torch.manual_seed(a.seed)
    G = ns["Generator"](config["z_dim"], config["label_dim"], config["hidden_dim"])                  # :74
    D = ns["Discriminator"](config["label_dim"], config["hidden_dim"])                               # :75
    optG = torch.optim.Adam(G.parameters(), lr=config["lr"])                                         # :77
    optD = torch.optim.Adam(D.parameters(), lr=config["lr"])                                         # :78
    consumed = {}
    optG.register_step_pre_hook(lambda opt, args, kwargs: consumed.__setitem__("G", {k: p.grad.detach().numpy().copy() for k, p in G.named_parameters()}))
    optD.register_step_pre_hook(lambda opt, args, kwargs: consumed.__setitem__("D", {k: p.grad.detach().numpy().copy() for k, p in D.named_parameters()}))
    ns.update(generator=G, discriminator=D, optimizer_G=optG, optimizer_D=optD, loss_D_total=0, loss_G_total=0)
    X, Y = RS.moons_data(config["n_samples"], a.seed)
    assert set(np.unique(Y)) == {0, 1}
    out = {"meta.seed": np.int64(a.seed), "X": X, "Y": Y}
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"init.{tag}.{k}"] = v.detach().numpy().copy()
    B, Z, L = config["batch_size"], config["z_dim"], config["label_dim"]
    for it in range(RS.ITERS):
        torch.manual_seed(a.seed + 1 + it)
        out[f"it{it}.z_d"] = torch.randn(B, Z).numpy().copy()                    # :97
        out[f"it{it}.labels_d"] = torch.randint(0, 1, (B,)).numpy().copy()       # :98
        out[f"it{it}.z_g"] = torch.randn(B, Z).numpy().copy()                    # :116
        out[f"it{it}.labels_g"] = torch.randint(0, L, (B,)).numpy().copy()       # :117
        torch.manual_seed(a.seed + 1 + it)                                       # the loop body repeats these draws
        ns["real_batch"] = torch.from_numpy(X[it * B:(it + 1) * B])
        ns["real_batch_labels"] = torch.from_numpy(Y[it * B:(it + 1) * B])
        exec(step_code, ns)
        assert torch.equal(ns["z"], torch.from_numpy(out[f"it{it}.z_g"])) and torch.equal(ns["fake_labels"], torch.from_numpy(out[f"it{it}.labels_g"]))
        out[f"it{it}.loss_D"] = np.float64(ns["loss_D"].item())
        out[f"it{it}.loss_G"] = np.float64(ns["loss_G"].item())
        for tag, net, opt in (("G", G, optG), ("D", D, optD)):
            for k, p in net.named_parameters():
                out[f"it{it}.{tag}.{k}"] = p.detach().numpy().copy()
                out[f"it{it}.{tag}.grad.{k}"] = consumed[tag][k]
                st = opt.state[p]
                out[f"it{it}.{tag}.exp_avg.{k}"] = st["exp_avg"].numpy().copy()
                out[f"it{it}.{tag}.exp_avg_sq.{k}"] = st["exp_avg_sq"].numpy().copy()
                out[f"it{it}.{tag}.step"] = np.int64(int(st["step"]))
    out["loss_D_total"] = np.float64(ns["loss_D_total"])
    out["loss_G_total"] = np.float64(ns["loss_G_total"])
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"final.{tag}.{k}"] = v.detach().numpy().copy()
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
