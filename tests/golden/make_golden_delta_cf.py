"""Writes tests/golden/delta_cf_ref.npz: the reference's own random-target iterations and prompted queries on seeded batches.

    python tests/golden/make_golden_delta_cf.py <reference root>

Runs on the CPU.  It imports the reference's modules/generator.py, modules/discriminator.py and modules/classifier.py and lifts, out of
the syntax tree of conditional_counteRGAN/mnist/gan_train_copy.py, the parameters (:17-29), the setup statements (:105-109), the loop
body from the class draw to the generator's Adam step (:119-146) and the query (:162 the random targets, :164-172 the clamped
counterfactuals and the classifier's verdict), and executes them unmodified -- in fp32 and, on the same seeded weights cast up, in
float64.  Training: three iterations at B = 4 and B = 3 on tests/delta_gan_restate.py's seeded nets, classifier and batches, the classes
drawn by :119 after torch.manual_seed(SEED_DRAW).  Queries: on the seeded (untrained) nets and batch 0, once with :162's random targets
and once per target class (the sweep: the :164-172 block with `targets` bound to one class for every row).  Seeds and the derived
quantities (sums, per-target metrics, the near set): tests/delta_cf_restate.py, which restates the same computations and is pinned to
this file by tests/test_delta_cf_host.py.  No weights are stored."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import delta_cf_restate as CR  # noqa: E402
import delta_gan_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402
from make_golden_delta_gan import _routing_check  # noqa: E402

STEPS = 3


def _lift(ref_root):
    path = os.path.join(ref_root, "conditional_counteRGAN/mnist/gan_train_copy.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    par = [n for n in tree.body if isinstance(n, ast.Assign) and n.lineno == 17 and n.end_lineno == 29]
    setup = [n for n in tree.body if isinstance(n, ast.Assign) and 105 <= n.lineno <= 109]
    loops = [n for n in tree.body if isinstance(n, ast.For) and n.lineno == 114]
    assert len(par) == 1 and len(setup) == 4 and len(loops) == 1, "reference layout changed"
    inner = [n for n in loops[0].body if isinstance(n, ast.For)]
    assert len(inner) == 1 and inner[0].lineno == 115, "reference layout changed"
    body = [n for n in inner[0].body if n.lineno >= 119]
    assert body[0].lineno == 119 and body[-1].end_lineno == 146 and len(body) + 2 == len(inner[0].body), "reference layout changed"
    draw = [n for n in tree.body if isinstance(n, ast.Assign) and n.lineno == 162]
    query = [n for n in tree.body if isinstance(n, ast.With) and n.lineno == 164 and n.end_lineno == 172]
    assert len(draw) == 1 and len(query) == 1, "reference layout changed"
    comp = lambda nodes: compile(ast.Module(body=nodes, type_ignores=[]), path, "exec")      # noqa: E731
    return comp(par), comp(setup), comp(body), comp(draw), comp(query)


def _nets(mods, dtype):
    torch.manual_seed(RS.SEED_GAN)
    G, D = mods["Generator"](), mods["Discriminator"]()
    torch.manual_seed(PR.SEED)
    C = mods["Classifier"]().eval()
    G, D, C = G.to(dtype), D.to(dtype), C.to(dtype)
    for p in C.parameters():
        p.requires_grad = False                                                    # gan_train_copy.py:98-99
    return G, D, C


def _params(code):
    ns = {"torch": torch}
    exec(code, ns)
    params = dict(ns["params"], device="cpu")
    assert (params["lambda_cls"], params["lambda_reg"], params["lr_G"], params["lr_D"]) == (CR.LAMBDA_CLS, CR.LAMBDA_REG, CR.LR_G, CR.LR_D)
    assert "target_class" not in params
    return params


def _train(B, dtype, codes, mods):
    par, setup, body, _, _ = codes
    G, D, C = _nets(mods, dtype)
    ns = {"torch": torch, "nn": torch.nn, "optim": torch.optim, "params": _params(par), "G": G, "D": D, "C": C}
    exec(setup, ns)
    torch.manual_seed(CR.SEED_DRAW)
    classes, losses = [], []
    for x, y in RS.batches(B, STEPS):
        ns["x"], ns["y_true"] = x.to(dtype), y
        exec(body, ns)
        classes.append(int(ns["random_class"]))
        assert bool((ns["target"] == classes[-1]).all())
        losses.append({k: float(ns[k].detach()) for k in CR.LOSSES})
    return classes, losses


def _queries(B, dtype, codes, mods):
    """The lifted :162 and :164-172 on the seeded nets: the random-target query, then the block once per target class."""
    _, _, _, draw, query = codes
    G, _, C = _nets(mods, dtype)
    x, y = RS.batches(B)[0]
    ns = {"torch": torch, "params": {"device": "cpu"}, "G": G, "C": C, "imgs": x.to(dtype), "labels": y}
    keys = {"x_cf": "cf_imgs", "delta": "deltas", "probs": "probs", "preds": "preds", "confs": "confs"}
    torch.manual_seed(CR.SEED_QUERY)
    exec(draw, ns)
    targets = ns["targets"].clone()
    exec(query, ns)
    rand = {k: ns[v].detach().clone() for k, v in keys.items()}
    per = []
    for t in range(CR.K):
        ns["targets"] = torch.full_like(y, t)
        exec(query, ns)
        per.append({k: ns[v].detach().clone() for k, v in keys.items()})
    return x, y, targets, rand, {k: torch.stack([p[k] for p in per]) for k in keys}


def _dist(a32, a64):
    return np.float64((a32.double() - a64.double()).abs().max())


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "conditional_counteRGAN/mnist"))
    from modules.classifier import Classifier
    from modules.discriminator import Discriminator
    from modules.generator import Generator
    mods = {"Generator": Generator, "Discriminator": Discriminator, "Classifier": Classifier}
    codes = _lift(ref_root)
    out = {"meta.seed_gan": np.int64(RS.SEED_GAN), "meta.seed_clf": np.int64(PR.SEED), "meta.seed_batches": np.int64(RS.SEED_BATCHES),
           "meta.seed_draw": np.int64(CR.SEED_DRAW), "meta.seed_query": np.int64(CR.SEED_QUERY), "meta.steps": np.int64(STEPS),
           "meta.batch_sizes": np.asarray([4, 3], np.int64)}
    for B in (4, 3):
        # ---- training: :119-146 ----
        c32, l32 = _train(B, torch.float32, codes, mods)
        c64, l64 = _train(B, torch.float64, codes, mods)
        assert c32 == c64, "the draw of :119 does not depend on the dtype"
        out[f"B{B}.classes"] = np.asarray(c64, np.int64)
        for name in CR.LOSSES:
            a32, a64 = np.asarray([s[name] for s in l32]), np.asarray([s[name] for s in l64])
            out[f"B{B}.{name}.f32"], out[f"B{B}.{name}.f64"], out[f"B{B}.{name}.dist"] = a32, a64, np.abs(a32 - a64)
            assert (np.abs(a32 - a64) <= 2e-6 * np.abs(a64)).all(), (B, name, a32, a64)
        # ---- queries: :162-172 and the sweep ----
        x, y, targets, r32, s32 = _queries(B, torch.float32, codes, mods)
        _, _, t64, r64, s64 = _queries(B, torch.float64, codes, mods)
        assert torch.equal(targets, t64)
        out[f"B{B}.x"], out[f"B{B}.y"], out[f"B{B}.query.targets"] = x.numpy(), y.numpy(), targets.numpy()
        for k in ("x_cf", "delta", "probs", "confs"):
            out[f"B{B}.query.{k}.f64"], out[f"B{B}.query.{k}.dist"] = r64[k].numpy(), _dist(r32[k], r64[k])
        out[f"B{B}.query.preds.f64"], out[f"B{B}.query.preds.f32"] = r64["preds"].numpy(), r32["preds"].numpy()
        near_q, gap_q, bound_q = CR.near_set(r32["probs"], r64["probs"])
        out[f"B{B}.query.near"], out[f"B{B}.query.gap"], out[f"B{B}.query.bound"] = near_q.numpy(), gap_q.numpy(), np.float64(bound_q)
        # the sweep: delta is stored whole at B = 4 only (x_cf is clamp(x + delta) of it: the tests rebuild it); everything else at both
        if B == 4:
            out[f"B{B}.sweep.delta.f64"] = s64["delta"].numpy()
        for k in ("x_cf", "delta", "probs", "confs"):
            out[f"B{B}.sweep.{k}.dist"] = _dist(s32[k], s64[k])
        assert torch.equal(s64["x_cf"], torch.clamp(x.double() + s64["delta"], -1, 1))
        out[f"B{B}.sweep.probs.f64"], out[f"B{B}.sweep.confs.f64"] = s64["probs"].numpy(), s64["confs"].numpy()
        out[f"B{B}.sweep.preds.f64"], out[f"B{B}.sweep.preds.f32"] = s64["preds"].numpy(), s32["preds"].numpy()
        sums32, sums64 = CR.query_sums(x, s32["x_cf"], s32["delta"]), CR.query_sums(x.double(), s64["x_cf"], s64["delta"])
        out[f"B{B}.sweep.sums.f64"] = sums64.numpy()
        out[f"B{B}.sweep.sums.dist"] = (sums32.double() - sums64).abs().reshape(-1, 3).max(0).values.numpy()
        m32, m64 = CR.per_target_metrics(x, y, s32), CR.per_target_metrics(x.double(), y, s64)
        for k in CR.METRICS:
            out[f"B{B}.sweep.{k}.f64"], out[f"B{B}.sweep.{k}.dist"] = m64[k], np.abs(m32[k] - m64[k])
        # ---- the condition on discrete outputs ----
        near, gap, bound = CR.near_set(s32["probs"], s64["probs"])
        n_near, n_q = int(near.sum()) + int(near_q.sum()), near.numel() + near_q.numel()
        assert n_near <= CR.NEAR_CAP * n_q, (B, n_near, n_q)
        out[f"B{B}.sweep.near"], out[f"B{B}.sweep.gap"], out[f"B{B}.sweep.bound"] = near.numpy(), gap.numpy(), np.float64(bound)
        agree = s32["preds"] == s64["preds"]
        assert bool(agree[~near].all()), "fp32 and float64 predictions differ outside the near set"
        hits = s64["preds"] == torch.arange(CR.K)[:, None]
        print(f"B {B}: classes {c64}; {int(near.sum())} of {near.numel()} sweep queries near (bound {bound:.2e}, smallest gaps "
              f"{np.sort(gap.numpy().ravel())[:2]}); predictions agree on {int(agree.sum())}; float64 predicts classes "
              f"{sorted(set(s64['preds'].reshape(-1).tolist()))}, {int(hits.sum())} hits")
        # ---- section 3.18's max-pool routing precondition on the query rows ----
        rows32, rows64 = s32["x_cf"].reshape(-1, 1, 28, 28), s64["x_cf"].reshape(-1, 1, 28, 28)
        rc = _routing_check(B, rows32, rows64)
        for layer in (1, 2):
            live, nearw = rc[f"B{B}.live{layer}"], rc[f"B{B}.near{layer}"]
            out[f"B{B}.sweep.routing.bound{layer}"] = rc[f"B{B}.bound{layer}"]
            out[f"B{B}.sweep.routing.near{layer}"], out[f"B{B}.sweep.routing.live{layer}"] = np.int64(nearw.sum()), np.int64(live.sum())
            print(f"B {B} pool {layer}: {int(nearw.sum())} of {int(live.sum())} live windows of the query rows under the bound")
    path = os.path.join(HERE, "delta_cf_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
