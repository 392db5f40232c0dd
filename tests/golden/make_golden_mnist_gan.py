#!/usr/bin/env python3
"""Records tests/golden/mnist_gan_ref.npz from the reference's own code (CPU, fp32): six iterations of simple_gan/mnist/mnist_gan.py
on synthetic 8-bit images, five batches of 64 rows and a last one of 32.

    python tests/golden/make_golden_mnist_gan.py /path/to/reference/checkout

`Generator`, `Discriminator` (:41-83) and the loop body (:116-134) are lifted out of the script with `ast` and executed here; the
script itself is never imported (it would pull torchvision and imageio and download MNIST).  No reference text is stored.  The
loop body draws z with np.random.normal (:122): numpy's global generator is seeded per iteration and the draw is replayed to record
it.  Large tensors are stored as digests (mnist_gan_restate.digest): fp64 sum, L2 norm and a fixed strided sample."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mnist_gan_restate as RS  # noqa: E402


def lift(ref):
    path = os.path.join(ref, "simple_gan/mnist/mnist_gan.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("Generator", "Discriminator")]
    body = []
    for node in tree.body:
        if isinstance(node, ast.For) and node.lineno == 113:
            inner = [n for n in node.body if isinstance(n, ast.For)]
            assert len(inner) == 1 and inner[0].lineno == 114, "reference layout changed"
            body = [n for n in inner[0].body if 116 <= n.lineno <= 134]
    assert len(defs) == 2 and body and body[0].lineno == 116 and body[-1].end_lineno == 134, "reference layout changed"
    args = types.SimpleNamespace(epochs=200, batch_size=64, learning_rate=0.0002, b1=0.5, b2=0.999, latent_dim=100, img_size=28, channels=1)  # :22-31
    ns = {"torch": torch, "nn": torch.nn, "np": np, "args": args, "img_shape": (1, 28, 28), "device": torch.device("cpu"),
          "Variable": torch.autograd.Variable, "Tensor": torch.FloatTensor}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns, compile(ast.Module(body=body, type_ignores=[]), path, "exec"), args


def put(out, key, t):
    a = t.detach().cpu().numpy()
    if a.size > RS.LARGE:
        out[key + "#digest"] = RS.digest(a)
    else:
        out[key] = a.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(HERE, "mnist_gan_ref.npz"))
    a = ap.parse_args()
    ns, step_code, args = lift(a.reference)
    torch.set_num_threads(1)                       # the CPU GEMMs' summation order depends on the thread count
    torch.manual_seed(RS.SEED)
    G, D = ns["Generator"](), ns["Discriminator"]()                                              # :85-86
    ns.update(generator=G, discriminator=D, adversarial_loss=torch.nn.BCELoss(),                 # :87
              optimizer_generator=torch.optim.Adam(G.parameters(), lr=args.learning_rate, betas=(args.b1, args.b2)),      # :108
              optimizer_discriminator=torch.optim.Adam(D.parameters(), lr=args.learning_rate, betas=(args.b1, args.b2)))  # :109
    out = {"meta.seed": np.int64(RS.SEED), "meta.sizes": np.asarray(RS.SIZES, np.int64)}
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"init.{tag}.{k}#digest"] = RS.digest(v)
            out[f"shape.{tag}.{k}"] = np.asarray(v.shape, np.int64)
    d_outs = []
    D.register_forward_hook(lambda m, i, o: d_outs.append(o.detach().numpy().copy()))
    rs = np.random.RandomState(RS.SEED)
    for it, n in enumerate(RS.SIZES):
        u8 = rs.randint(0, 256, (n, RS.IMG)).astype(np.uint8)
        zrec = rs.normal(0.0, 1.0, (n, RS.LATENT)).astype(np.float32)          # consumed so that mnist_gan_restate.inputs() stays in step
        np.random.seed(RS.SEED + 1 + it)
        z = np.random.normal(0, 1, (n, args.latent_dim))
        np.random.seed(RS.SEED + 1 + it)                                        # the loop body repeats this draw (:122)
        out[f"real_u8.{it}"] = u8
        out[f"z.{it}"] = z.astype(np.float32)                                   # what Tensor(...) makes of it
        del zrec
        ns["images"] = torch.from_numpy(RS.normalize_u8(u8)).view(n, 1, 28, 28)
        ns["i"] = it
        del d_outs[:]
        exec(step_code, ns)
        assert len(d_outs) == 3
        out[f"it{it}.g_loss"] = np.float64(ns["generator_loss"].item())
        out[f"it{it}.d_loss"] = np.float64(ns["discriminator_loss"].item())
        for j, name in enumerate(("d_fake_g", "d_real", "d_fake")):
            out[f"it{it}.{name}"] = d_outs[j]
        for tag, net in (("G", G), ("D", D)):
            for k, v in net.state_dict().items():
                put(out, f"it{it}.{tag}.{k}", v)
            for k, p in net.named_parameters():
                put(out, f"it{it}.{tag}.grad.{k}", p.grad)      # still what each optimizer consumed: zero_grad runs at the next iteration
    out["last.fake"] = ns["generated_images"].detach().numpy().reshape(RS.SIZES[-1], -1).copy()
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
