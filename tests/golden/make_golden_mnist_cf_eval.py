"""Golden fixtures for the MNIST CounteRGAN's prompted queries and per-target evaluation (conditional_counteRGAN/mnist): the
reference's own `build_patch_mask_for_batch` (eval_utils.py:204-288), `compute_masked_metrics` (:292-344), `evaluate_counterfactuals`
(:46-76) and `evaluate_generator_per_target` (:78-110), lifted from the syntax tree the way make_golden.py lifts them (the module
imports seaborn) and run on the CPU with the reference's generator and classifier modules, the generator checkpoint in tests/golden
(the shipped results/generator.pt) and a seeded CNNClassifier (torch.manual_seed(3); the trained one is not shipped).  Writes
tests/golden/mnist_cf_eval_ref.npz.

    python tests/golden/make_golden_mnist_cf_eval.py <path of the reference repository> [output directory]

Recorded:
  sel.cases (JSON)                      name -> {seed, bs, patch_size, kwargs}: the calls of build_patch_mask_for_batch below
  sel.<name>.mask [n][28][28] uint8     its batch mask (n = bs; the shared and the user-list cases repeat one mask)
  sel.<name>.chosen [n][total] uint8    1 where patch p of mask n is modifiable (decoded from the mask)
  x [11][1][28][28], y [11]             seeded inputs on a 1/8 grid in [-1, 1] (so both clamps fire), seeded labels
  sweep.*                               rows 0..5 x 10 targets with Config.user_input_patches at patch size 7: mask [28][28], raw, masked,
                                        x_cf [10][6][784], probs_cf [10][6][10], probs_orig [6][10], pred [10][6], masked_metrics
                                        [10][6] (compute_masked_metrics per target, MASKED_KEYS order), undecided [10][6]
  table.*                               evaluate_generator_per_target on the 11 rows in batches of 4: metrics [10][3], csv (its file),
                                        undecided [10][3] (per target and batch), counts [3]
A query is UNDECIDED when the float64 run's top-two probability gap is under max(1e-5, 100 * max|p_fp32 - p_fp64|) (both runs are
the reference's, on the CPU): its argmax is not pinned by the reference itself.  At most 5 % of a case's queries may be undecided;
the script asserts it."""
import ast
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
MASKED_KEYS = ("Class_flip_rate_mean", "Class_flip_rate_max", "Residual_L1_norm_in_allowed_patches", "Prediction_gain",
               "Actionability (overall L1 norm)", "mask_penalty_pre")
USER = [1, 5, 10, 12, 13, 14]                   # config.py:20 user_input_patches
SEL_CASES = {
    "shared7": dict(seed=11, bs=4, patch_size=7, kwargs=dict(shared_per_batch=True)),
    "sample7": dict(seed=12, bs=4, patch_size=7, kwargs=dict(shared_per_batch=False, min_patches=6, max_patches=15)),
    "user7": dict(seed=13, bs=4, patch_size=7, kwargs=dict(shared_per_batch=True, modifiable_patches=USER, randomize_per_sample=False)),
    "userrows7": dict(seed=14, bs=3, patch_size=7, kwargs=dict(shared_per_batch=False, modifiable_patches=USER, randomize_per_sample=False)),
    "userignored7": dict(seed=15, bs=3, patch_size=7, kwargs=dict(shared_per_batch=False, modifiable_patches=USER)),   # :260: the list loses
    "shared5": dict(seed=16, bs=4, patch_size=5, kwargs=dict(shared_per_batch=True)),
    "sample5": dict(seed=17, bs=4, patch_size=5, kwargs=dict(shared_per_batch=False)),
    "user5": dict(seed=18, bs=2, patch_size=5, kwargs=dict(shared_per_batch=True, modifiable_patches=[0, 4, 12, 20, 24], randomize_per_sample=False)),
    "user4": dict(seed=19, bs=2, patch_size=4, kwargs=dict(shared_per_batch=True, modifiable_patches=[0, 31, 32, 40, 48, 49, 60, -1],
                                                           randomize_per_sample=False)),
    "empty7": dict(seed=20, bs=2, patch_size=7, kwargs=dict(shared_per_batch=True, modifiable_patches=[], randomize_per_sample=False)),
}


def lift(path, names, ns):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(defs) == len(names), (path, [d.name for d in defs])
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def undecided(p32, p64):
    """[...] bool from probabilities [..., K] of the fp32 and the float64 run, and the bound used."""
    bound = max(1e-5, 100.0 * float(np.abs(p32.astype(np.float64) - p64).max()))
    top = np.sort(p64, axis=-1)
    return (top[..., -1] - top[..., -2]) < bound, bound


def main(ref_root, out_dir=HERE):
    import importlib
    import pandas as pd
    from typing import Dict, Tuple
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "mnist")
    sys.path.insert(0, mdir)
    gen_mod = importlib.import_module("models.generator")
    clf_mod = importlib.import_module("models.classifier")
    ns = {"torch": torch, "np": np, "F": F, "os": os, "pd": pd, "Dict": Dict, "Tuple": Tuple, "tqdm": lambda it, **k: it}
    lift(os.path.join(mdir, "eval_utils.py"), ("build_patch_mask_for_batch", "compute_masked_metrics", "evaluate_counterfactuals",
                                               "evaluate_generator_per_target"), ns)
    G = gen_mod.ResidualGenerator()
    G.load_state_dict(torch.load(os.path.join(HERE, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    torch.manual_seed(3)
    C = clf_mod.CNNClassifier()
    G.eval(); C.eval()
    G64, C64 = copy.deepcopy(G).double(), copy.deepcopy(C).double()
    out = {"sel.cases": np.array(json.dumps(SEL_CASES))}

    # ---- patch selection (eval_utils.py:204-288) ---------------------------------------------------------------------------------
    for name, case in SEL_CASES.items():
        ps = case["patch_size"]
        np.random.seed(case["seed"])
        bm, sm = ns["build_patch_mask_for_batch"](torch.zeros(case["bs"], 1, 28, 28), patch_size=ps, device="cpu", **case["kwargs"])
        m = bm[:, 0].numpy()
        assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(sm[0, 0].numpy(), m[0])
        out[f"sel.{name}.mask"] = m.astype(np.uint8)
        n = 28 // ps
        out[f"sel.{name}.chosen"] = m[:, 0:n * ps:ps, 0:n * ps:ps].reshape(len(m), n * n).astype(np.uint8)

    # ---- inputs --------------------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(31)
    x = torch.randint(-8, 9, (11, 1, 28, 28), generator=g).float() / 8.0
    y = torch.randint(0, 10, (11,), generator=g)
    out["x"], out["y"] = x.numpy(), y.numpy()

    # ---- the 6-row x 10-target sweep with the user's patches (gradio_app.py:234-259, eval_utils.py:292-344) ---------------------
    xs, ys = x[:6], y[:6]
    mask = ns["build_patch_mask_for_batch"](xs, patch_size=7, device="cpu", shared_per_batch=True, modifiable_patches=USER,
                                            randomize_per_sample=False)[0]
    rec = {k: [] for k in ("raw", "masked", "x_cf", "probs_cf", "pred", "masked_metrics", "p64")}
    with torch.no_grad():
        for t in range(10):
            tgt = torch.full_like(ys, t)
            raw, masked = G(xs, tgt, mask)
            x_cf = torch.clamp(xs + masked, -1.0, 1.0)
            logits = C(x_cf)
            met = ns["compute_masked_metrics"](raw, masked, xs, x_cf, mask, C, ys, tgt, "cpu")
            r64, m64 = G64(xs.double(), tgt, mask.double())
            p64 = F.softmax(C64(torch.clamp(xs.double() + m64, -1.0, 1.0)), dim=1)
            rec["raw"].append(raw.numpy().reshape(6, 784)); rec["masked"].append(masked.numpy().reshape(6, 784))
            rec["x_cf"].append(x_cf.numpy().reshape(6, 784)); rec["probs_cf"].append(F.softmax(logits, dim=1).numpy())
            rec["pred"].append(logits.argmax(1).numpy()); rec["masked_metrics"].append([met[k] for k in MASKED_KEYS]); rec["p64"].append(p64.numpy())
        out["sweep.probs_orig"] = F.softmax(C(xs), dim=1).numpy()
    for k in ("raw", "masked", "x_cf", "probs_cf", "pred"):
        out[f"sweep.{k}"] = np.stack(rec[k])
    out["sweep.mask"] = mask[0, 0].numpy()
    out["sweep.masked_metrics"] = np.asarray(rec["masked_metrics"], np.float64)
    und, bound = undecided(out["sweep.probs_cf"], np.stack(rec["p64"]))
    assert und.mean() <= 0.05, f"sweep: {int(und.sum())} of {und.size} queries undecided (bound {bound:.1e}): pick another seed"
    out["sweep.undecided"], out["sweep.undecided_bound"] = und, np.float64(bound)

    # ---- evaluate_generator_per_target on 11 rows in batches of 4 (eval_utils.py:78-110) -----------------------------------------
    loader = [(x[i:i + 4], y[i:i + 4]) for i in range(0, 11, 4)]
    save_dir = tempfile.mkdtemp()
    cfg = type("Cfg", (), {"device": "cpu", "num_classes": 10, "save_dir": save_dir})
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        ns["evaluate_generator_per_target"](G, C, loader, cfg)
    with open(os.path.join(save_dir, "countergan_metrics_per_class.csv")) as f:
        csv = f.read()
    out["table.csv"] = np.array(csv)
    out["table.metrics"] = pd.read_csv(io.StringIO(csv), index_col=0, float_precision="round_trip")[["class_flip_rate", "prediction_gain", "actionability"]].to_numpy(np.float64)
    und_t, worst = np.zeros((10, len(loader)), np.int64), 0.0
    with torch.no_grad():
        for j, (xb, yb) in enumerate(loader):
            ones = torch.ones_like(xb)
            for t in range(10):
                tgt = torch.full_like(yb, t)
                p32 = F.softmax(C(torch.clamp(xb + G(xb, tgt, ones)[1], -1.0, 1.0)), dim=1).numpy()
                p64 = F.softmax(C64(torch.clamp(xb.double() + G64(xb.double(), tgt, ones.double())[1], -1.0, 1.0)), dim=1).numpy()
                u, b = undecided(p32, p64)
                und_t[t, j], worst = int(u.sum()), max(worst, b)
    assert und_t.sum() <= 0.05 * 110, f"table: {int(und_t.sum())} of 110 queries undecided: pick another seed"
    out["table.undecided"], out["table.counts"], out["table.undecided_bound"] = und_t, np.array([len(b[1]) for b in loader]), np.float64(worst)

    path = os.path.join(out_dir, "mnist_cf_eval_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.0f} kB; undecided: sweep {int(und.sum())} / {und.size} (bound {bound:.1e}), "
          f"table {int(und_t.sum())} / 110 (bound {worst:.1e})")


if __name__ == "__main__":
    main(sys.argv[1], *(sys.argv[2:3]))
