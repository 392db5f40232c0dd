"""Golden fixtures for the prompted queries and the class-pair sensitivity of the tabular CounteRGAN
(conditional_counteRGAN/house_sales_kc_usa): the reference's own `build_counterfactuals` (eval_utils.py:25-181) and
`analyze_class_pair_sensitivity` (:351-434) lifted from the syntax tree the way make_golden.py lifts them (the module imports
seaborn; plotting names are bound to stubs) and run on the CPU with the reference's generator and classifier modules, the two
checkpoints in tests/golden and the scaled test split of tests/golden/house_eval.npz.  The hard Gumbel-softmax draws are recovered
from the RNG state captured right before each generator call.  Writes tests/golden/house_cf_eval_ref.npz.

    python tests/golden/make_golden_house_cf_eval.py <path of the reference repository> [output directory]

Recorded (R = 3 requests, N = 83 rows, Tcat = 70 packed categories, S = 200 rows for the sensitivity):
  gradio.allowed [3] (text), gradio.immutable_mask [3][17]   the request's allowed features; 1 where the per-request immutable_idx
                                         of gradio_app.py:152-155 leaves the feature free
  gradio.target [3][83] int64            the target class of every row (one query per row, gradio_app.py:158-160)
  gradio.gumbel [3][83][70]              the noise F.gumbel_softmax drew, heads packed in the generator's order
  gradio.masked_residual, gradio.x_cf [3][83][17]   build_counterfactuals' two results (:163)
  gradio.probs_x [83][4], gradio.probs_cf [3][83][4]   softmax of the classifier on x and on the clamped x_cf (:167-169)
  sens.deltas [4][4][17]                 analyze_class_pair_sensitivity on the first 200 rows
  sens.gumbel [4][200][70]               slot t, rows of class s: the noise of the pass (s, t); zero elsewhere
"""
import ast
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS, S_ROWS = 83, 200
REQUESTS = (("sqft_living", "grade", "bathrooms"), ("bedrooms", "floors", "view", "condition", "sqft_lot"), None)   # None: every mutable feature


class _Stub:
    """Stands in for matplotlib.pyplot / seaborn: every attribute is a callable that returns the stub."""

    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi


def lift(path, names, ns):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(defs) == len(names), (path, [d.name for d in defs])
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def replay(G, state, rows):
    """The noise F.gumbel_softmax draws per head (generator.py:90), packed in head order."""
    keep = torch.get_rng_state()
    torch.set_rng_state(state)
    parts = [-torch.empty(rows, head.out_features).exponential_().log() for head in G.fc_cat_logits.values()]
    torch.set_rng_state(keep)
    return torch.cat(parts, 1).numpy()


def main(ref_root, out_dir=HERE):
    from typing import Optional, Tuple
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "house_sales_kc_usa")
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())                     # the reference's config.py creates its results directories in the cwd
    try:
        sys.path.insert(0, mdir)
        import importlib
        cfg = dict(importlib.import_module("config").config)
        gen_mod = importlib.import_module("models.generator")
        clf_mod = importlib.import_module("models.nn_classifier")
        gold = np.load(os.path.join(HERE, "house_eval.npz"))
        X, y = gold["X_test"], gold["y_test"]
        cfg["cuda"] = "cpu"
        cfg["scaler"] = _Scaler(gold["scaler.data_min"], gold["scaler.data_max"])
        cfg["categorical_info"] = {f: {"n": len(gold[f"raw_values.{f}"]), "raw_values": gold[f"raw_values.{f}"].tolist()}
                                   for f in cfg["categorical_info"]}
        names = cfg["feature_names"]
        ns = {"torch": torch, "np": np, "F": F, "os": os, "Tuple": Tuple, "Optional": Optional, "plt": _Stub(), "sns": _Stub()}
        lift(os.path.join(mdir, "eval_utils.py"), ("build_counterfactuals", "analyze_class_pair_sensitivity"), ns)
        G = gen_mod.ResidualGenerator(cfg["input_dim"], cfg["hidden_dim"], cfg["num_classes"], continuous_idx=cfg["continuous_idx"],
                                      categorical_info=cfg["categorical_info"], tau=cfg["gumbel_tau"])
        clf = clf_mod.NNClassifier(cfg["input_dim"], output_dim=cfg["num_classes"])
        G.load_state_dict(torch.load(os.path.join(HERE, "house_generator_trained.pt"), map_location="cpu", weights_only=True))
        clf.load_state_dict(torch.load(os.path.join(HERE, "house_classifier_trained.pt"), map_location="cpu", weights_only=True))
        G.eval(); clf.eval()
        states = []
        hook = G.register_forward_pre_hook(lambda m, a: states.append((torch.get_rng_state(), a[0].shape[0])))
        out = {}

        # ---- gradio_app.py:144-169, one query per row ------------------------------------------------------------------------
        x = torch.tensor(X[:N_ROWS], dtype=torch.float32)
        yy = torch.tensor(y[:N_ROWS], dtype=torch.long)
        rec = {k: [] for k in ("immutable_mask", "target", "gumbel", "masked_residual", "x_cf", "probs_cf")}
        torch.manual_seed(5)
        for r, allowed in enumerate(REQUESTS):
            allowed = set(n for n in names if names.index(n) not in cfg["immutable_idx"]) if allowed is None else set(allowed)
            per_request_immutable = [i for i, feat in enumerate(names) if feat not in allowed]                    # :153
            c2 = dict(cfg)
            c2["immutable_idx"] = per_request_immutable                                                           # :155
            target = (yy + 1 + r) % cfg["num_classes"]
            states.clear()
            with torch.no_grad():
                masked, x_cf = ns["build_counterfactuals"](G, x, F.one_hot(target, cfg["num_classes"]).float(), c2)   # :163
                probs_cf = F.softmax(clf(torch.tensor(x_cf.numpy(), dtype=torch.float32)), dim=1)                  # :169
            assert len(states) == 1
            m = np.ones(len(names), np.float32)
            m[per_request_immutable] = 0.0
            rec["immutable_mask"].append(m); rec["target"].append(target.numpy()); rec["gumbel"].append(replay(G, states[0][0], N_ROWS))
            rec["masked_residual"].append(masked.numpy()); rec["x_cf"].append(x_cf.numpy()); rec["probs_cf"].append(probs_cf.numpy())
        for k, v in rec.items():
            out[f"gradio.{k}"] = np.stack(v)
        out["gradio.allowed"] = np.array([",".join(a) if a is not None else "" for a in REQUESTS])
        with torch.no_grad():
            out["gradio.probs_x"] = F.softmax(clf(x), dim=1).numpy()                                                  # :168

        # ---- eval_utils.py:351-434 on the first S_ROWS rows ------------------------------------------------------------------
        Xs, ys = X[:S_ROWS], y[:S_ROWS]
        states.clear()
        torch.manual_seed(6)
        deltas = ns["analyze_class_pair_sensitivity"](G, clf, Xs, ys, names, cfg, tempfile.mkdtemp())
        hook.remove()
        NC = cfg["num_classes"]
        assert len(states) == NC * (NC - 1)
        noise = np.zeros((NC, S_ROWS, sum(h.out_features for h in G.fc_cat_logits.values())), np.float32)
        calls = iter(states)
        for s in range(NC):                                                                                          # the function's loop order
            rows = np.nonzero(ys == s)[0]
            for t in range(NC):
                if s != t:
                    st, n = next(calls)
                    assert n == len(rows)
                    noise[t, rows] = replay(G, st, n)
        out["sens.deltas"], out["sens.gumbel"] = deltas, noise
        path = os.path.join(out_dir, "house_cf_eval_ref.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {os.path.getsize(path) / 1e3:.0f} kB")
    finally:
        os.chdir(cwd)


if __name__ == "__main__":
    main(sys.argv[1], *(sys.argv[2:3]))
