"""Writes tests/golden/countergan2_ref.npz: the reference's own full-resolution CounteRGAN iterations on seeded batches.

    python tests/golden/make_golden_countergan2.py <reference root>

Runs on the CPU.  It never imports or executes conditional_counteRGAN/mnist/countergan2.py: that script's top level parses argv and
constructs datasets.MNIST(..., download=True).  Instead it lifts the three class definitions (:57-113), the setup assignments
(:170-173) and the inner loop body (:180-205) out of the file's syntax tree and executes them unmodified, with `args.target` supplied
-- in fp32 and, on the same seeded weights cast up, in float64.  The body is executed in its two halves (:180-191, the discriminator;
:194-205, the generator) so that D's gradients of :190 and the d_fake of :187 can be recorded before :204 adds to the one and :195
rebinds the other.  Seeds, batches and the layout of the file: tests/countergan2_restate.py, which restates the same iteration and is
pinned to this file by tests/test_countergan2_host.py.  No weights are stored: the tests rebuild them from the seeds and check the
recorded per-tensor sums."""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import countergan2_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

FULL_MAX = 1024            # tensors up to this many elements are stored whole, larger ones as RS.digest
NEAR_CAP = 0.002           # at most 0.2 % of a layer's live windows under the gap bound


def _lift(ref_root):
    path = os.path.join(ref_root, "conditional_counteRGAN/mnist/countergan2.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    classes = [n for n in tree.body if isinstance(n, ast.ClassDef)]
    assert [(c.name, c.lineno) for c in classes] == [("Generator", 57), ("Discriminator", 76), ("Classifier", 96)], "reference layout changed"
    assert classes[-1].end_lineno == 113, "reference layout changed"
    setup = [n for n in tree.body if isinstance(n, ast.Assign) and 170 <= n.lineno <= 173]
    loops = [n for n in tree.body if isinstance(n, ast.For) and n.lineno == 178]
    assert len(setup) == 4 and len(loops) == 1, "reference layout changed"
    inner = [n for n in loops[0].body if isinstance(n, ast.For)]
    assert len(inner) == 1 and inner[0].lineno == 179, "reference layout changed"
    body = inner[0].body
    assert body[0].lineno == 180 and body[-1].end_lineno == 205, "reference layout changed"
    d_half = [n for n in body if n.end_lineno <= 191]
    g_half = [n for n in body if n.lineno >= 194]
    assert len(d_half) + len(g_half) == len(body)
    comp = lambda nodes: compile(ast.Module(body=nodes, type_ignores=[]), path, "exec")      # noqa: E731
    return comp(classes), comp(setup), comp(d_half), comp(g_half)


def _store(out, key, t):
    v = t.detach().double().numpy()
    out[key + (".full" if v.size <= FULL_MAX else ".digest")] = v if v.size <= FULL_MAX else RS.digest(t)


def _run(B, dtype, codes):
    classes, setup, d_half, g_half = codes
    ns = {"torch": torch, "nn": torch.nn, "optim": torch.optim, "F": torch.nn.functional}
    exec(classes, ns)
    torch.manual_seed(RS.SEED_GAN)
    G, D = ns["Generator"](), ns["Discriminator"]()
    torch.manual_seed(PR.SEED)
    C = ns["Classifier"]().eval()
    G, D, C = G.to(dtype), D.to(dtype), C.to(dtype)
    for p in C.parameters():
        p.requires_grad = False                                                    # countergan2.py:166-167
    params = {"lr_G": RS.LR, "lr_D": RS.LR, "lambda_cls": RS.LAMBDA_CLS, "lambda_reg": RS.LAMBDA_REG, "device": "cpu"}
    ns.update(params=params, args=types.SimpleNamespace(target=RS.TARGET_CLASS), G=G, D=D, C=C)
    init = {"G": {k: v.detach().clone() for k, v in G.state_dict().items()}, "D": {k: v.detach().clone() for k, v in D.state_dict().items()},
            "C": {k: v.detach().clone() for k, v in C.state_dict().items()}}
    exec(setup, ns)
    steps = []
    for x, y in RS.batches(B):
        ns["x"], ns["y"] = x.to(dtype), y
        exec(d_half, ns)
        rec = {"loss_D": float(ns["loss_D"].detach()), "d_real": ns["d_real"].detach().clone(), "d_fake": ns["d_fake"].detach().clone(),
               "grad_D": {k: p.grad.detach().clone() for k, p in D.named_parameters()}}
        exec(g_half, ns)
        rec.update({k: float(ns[k].detach()) for k in ("loss_G", "loss_adv", "loss_cls", "loss_reg")})
        rec.update(delta=ns["delta"].detach().clone(), x_cf=ns["x_cf"].detach().clone(), d_fake_g=ns["d_fake"].detach().clone(),
                   cls_logits=ns["cls_pred"].detach().clone(), grad_G={k: p.grad.detach().clone() for k, p in G.named_parameters()})
        steps.append(rec)
    return steps, G, D, init


def _routing_check(B, x_cf32, x_cf64):
    """DESIGN.md section 3.18's precondition on the classifier's max-pool routing for the rows the GAN step feeds it: the windows whose
    float64 top-two gap is under max(1e-5, 100 * max|z_fp32 - z_fp64|) are at most 0.2 % of the live ones."""
    f32, f64 = PR.forward(PR.seeded_state(PR.SEED), x_cf32), PR.forward(PR.cast(PR.seeded_state(PR.SEED), torch.float64), x_cf64)
    out = {}
    for layer in (1, 2):
        z32, z64 = f32[f"z{layer}"], f64[f"z{layer}"]
        bound = max(1e-5, 100.0 * float((z32.double() - z64).abs().max()))
        live = f64[f"p{layer}"] > 0
        near = live & (PR.top2_gap(z64) < bound)
        frac = float(near.sum()) / float(live.sum())
        print(f"B {B} pool {layer}: {int(near.sum())} of {int(live.sum())} live windows under the bound {bound:.1e}")
        assert frac <= NEAR_CAP, (B, layer, frac)
        out[f"B{B}.bound{layer}"] = np.float64(bound)
        out[f"B{B}.live{layer}"] = live.numpy()
        out[f"B{B}.near{layer}"] = near.numpy()
        out[f"B{B}.idx{layer}"] = f64[f"idx{layer}"].numpy()
    return out


def main(ref_root):
    codes = _lift(ref_root)
    out = {"meta.seed_gan": np.int64(RS.SEED_GAN), "meta.seed_clf": np.int64(PR.SEED), "meta.seed_batches": np.int64(RS.SEED_BATCHES),
           "meta.target_class": np.int64(RS.TARGET_CLASS), "meta.steps": np.int64(3), "meta.batch_sizes": np.asarray([4, 3], np.int64)}
    worst_loss = worst_grad = 0.0
    for B in (4, 3):
        s32, G32, D32, init = _run(B, torch.float32, codes)
        s64, G64, D64, _ = _run(B, torch.float64, codes)
        if B == 4:
            for net in ("G", "D", "C"):
                for k, v in init[net].items():
                    out[f"init.{net}.{k}.sum"] = np.float64(v.double().sum())
                    out[f"init.{net}.{k}.abssum"] = np.float64(v.double().abs().sum())
        for i, (x, y) in enumerate(RS.batches(B)):
            out[f"B{B}.step{i}.x"], out[f"B{B}.step{i}.y"] = x.numpy(), y.numpy()
        for name in RS.LOSSES:
            l32, l64 = np.asarray([s[name] for s in s32]), np.asarray([s[name] for s in s64])
            out[f"B{B}.{name}.f32"], out[f"B{B}.{name}.f64"] = l32, l64
            out[f"B{B}.{name}.dist"] = np.abs(l32 - l64)
            worst_loss = max(worst_loss, float((np.abs(l32 - l64) / np.abs(l64)).max()))
            assert (np.abs(l32 - l64) <= 2e-6 * np.abs(l64)).all(), (B, name, l32, l64)
        for name in RS.FORWARD:
            out[f"B{B}.{name}.f64"] = s64[0][name].numpy()
            out[f"B{B}.{name}.dist"] = np.float64((s32[0][name].double() - s64[0][name]).abs().max())
        for net, keys in (("G", RS.G_KEYS), ("D", RS.D_KEYS)):
            for k in keys:
                g32, g64 = s32[0][f"grad_{net}"][k], s64[0][f"grad_{net}"][k]
                dist = float((g32.double() - g64).abs().max())
                worst_grad = max(worst_grad, dist / float(g64.abs().max()))
                assert dist <= 2.5e-5 * float(g64.abs().max()), (B, net, k, dist, float(g64.abs().max()))
                _store(out, f"B{B}.grad.{net}.{k}", g64)
                out[f"B{B}.grad.{net}.{k}.dist"] = np.float64(dist)
                out[f"B{B}.grad.{net}.{k}.max"] = np.float64(g64.abs().max())
            m32, m64 = (G32, G64) if net == "G" else (D32, D64)
            for (k, p32), (_, p64) in zip(m32.state_dict().items(), m64.state_dict().items()):
                _store(out, f"B{B}.final.{net}.{k}", p64)
                out[f"B{B}.final.{net}.{k}.dist"] = np.float64((p32.double() - p64).abs().max())
        out.update(_routing_check(B, s32[0]["x_cf"], s64[0]["x_cf"]))
    print(f"fp32 against float64: losses within {worst_loss:.2e} relative, gradients within {worst_grad:.2e} * max|g|")
    path = os.path.join(HERE, "countergan2_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
