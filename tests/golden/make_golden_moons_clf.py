"""Golden fixture for the moons CounteRGAN's classifier fit (conditional_counteRGAN/moons/trainer.py:13-29): the reference's own
train_classifier run on the CPU, unmodified and observed through hooks only — matplotlib must be importable (trainer.py imports it).
Writes tests/golden/moons_clf_ref.npz.

    python tests/golden/make_golden_moons_clf.py <path of the reference repository> [output directory]
    python tests/golden/make_golden_moons_clf.py <path of the reference repository> --check     (regenerate, compare every array bit for bit)

The data are data.{X_train,y_train,X_test,y_test} of moons_cf_ref.npz (next to this file); they are not repeated here.

Recorded (torch.manual_seed(0) immediately before the call; one CPU thread):
  init.C.<key>                         the classifier as train_classifier constructs it
  losses [1000]                        the `loss` of every iteration (the loss module's forward, wrapped)
  it{k}.C.<key>                        the state_dict after step k, k in SNAPSHOTS
  it{k}.opt.<key>.{exp_avg,exp_avg_sq}, it{k}.opt.step
  losses64 [1000], it{k}.C64.<key>     the same loop (trainer.py:22-25, lifted from the reference's source with `ast` at run time)
                                       rerun in float64 from the same initial state
  dist{k}                              max |fp32 - float64| over all parameters after step k
  acc.train, acc.test, final_loss      of the fp32 run after step 1000 (final_loss: the cross-entropy of the final weights on the
  acc64.train, acc64.test, final_loss64    training split), and of the float64 run
SNAPSHOTS holds the steps the issue names (1, 2, 3, 10, 100, 1000) and the two states *before* steps 10 and 100 (9, 99), which the
teacher-forced single-step test starts from.
"""
import ast
import inspect
import os
import shutil
import sys
import tempfile
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SNAPSHOTS = (1, 2, 3, 9, 10, 99, 100, 1000)


def record(ref_root):
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "moons")
    sys.path.insert(0, mdir)
    import trainer
    from config import config as ref_config
    from models.nn_classifier import NNClassifier

    torch.set_num_threads(1)
    data = np.load(os.path.join(HERE, "moons_cf_ref.npz"))
    X_train, y_train, X_test, y_test = (data[f"data.{k}"] for k in ("X_train", "y_train", "X_test", "y_test"))
    out, holder = {}, {}

    # ---- hooks ------------------------------------------------------------------------------------------------------------------
    class RecClassifier(NNClassifier):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            holder["C"] = self
            for key, v in self.state_dict().items():
                out[f"init.C.{key}"] = v.detach().clone().numpy()

    class RecAdam(torch.optim.Adam):
        tag, net = "C", None

        def step(self, closure=None):
            r = super().step(closure)
            holder["n" + self.tag] = i = holder.get("n" + self.tag, 0) + 1
            if i in SNAPSHOTS:
                net = self.net if self.net is not None else holder["C"]
                for key, v in net.state_dict().items():
                    out[f"it{i}.{self.tag}.{key}"] = v.detach().clone().numpy()
                if self.tag == "C":
                    for name, p in net.named_parameters():
                        st = self.state[p]
                        out[f"it{i}.opt.{name}.exp_avg"] = st["exp_avg"].clone().numpy()
                        out[f"it{i}.opt.{name}.exp_avg_sq"] = st["exp_avg_sq"].clone().numpy()
                        out[f"it{i}.opt.step"] = np.array(int(st["step"]), np.int64)
            return r

    losses = {"C": [], "C64": []}
    ce_forward = torch.nn.CrossEntropyLoss.forward

    def rec_forward(self, input, target):
        loss = ce_forward(self, input, target)
        losses["C64" if input.dtype == torch.float64 else "C"].append(float(loss.detach()))
        return loss

    def evaluate(net, tag, dtype):
        with torch.no_grad():
            for split, X, y in (("train", X_train, y_train), ("test", X_test, y_test)):
                pred = net(torch.tensor(X, dtype=dtype)).argmax(1).numpy()
                out[f"acc{tag}.{split}"] = np.array(np.mean(pred == y), np.float64)
            logits = net(torch.tensor(X_train, dtype=dtype))
            out[f"final_loss{tag}"] = np.array(float(ce_forward(torch.nn.CrossEntropyLoss(), logits, torch.tensor(y_train, dtype=torch.long))), np.float64)

    cfg = dict(ref_config)
    tmp = tempfile.mkdtemp()
    cfg.update(cuda="cpu", out_dir=tmp, clf_model_path=os.path.join(tmp, "classifier.pt"))
    trainer.NNClassifier, trainer.optim.Adam = RecClassifier, RecAdam
    torch.nn.CrossEntropyLoss.forward = rec_forward
    try:
        torch.manual_seed(0)
        clf = trainer.train_classifier(X_train, y_train, cfg)
        assert clf is holder["C"] and holder["nC"] == 1000 and len(losses["C"]) == 1000
        evaluate(clf, "", torch.float32)

        # ---- the same loop in float64: its lines taken from the reference's source at run time ------------------------------------
        tree = ast.parse(textwrap.dedent(inspect.getsource(trainer.train_classifier)))
        loops = [n for n in ast.walk(tree) if isinstance(n, ast.For)]
        assert len(loops) == 1, "trainer.train_classifier has one loop (trainer.py:22-25)"
        loop = compile(ast.Module(body=loops, type_ignores=[]), "trainer.py:22-25", "exec")
        clf64 = NNClassifier(cfg["input_dim"]).double()
        clf64.load_state_dict({k[len("init.C."):]: torch.tensor(v, dtype=torch.float64) for k, v in out.items() if k.startswith("init.C.")})

        class RecAdam64(RecAdam):
            tag, net = "C64", clf64

        env = {"clf": clf64, "opt": RecAdam64(clf64.parameters(), lr=1e-2), "loss_fn": torch.nn.CrossEntropyLoss(),
               "X_t": torch.tensor(X_train, dtype=torch.float64), "y_t": torch.tensor(y_train, dtype=torch.long)}
        exec(loop, env)
        assert holder["nC64"] == 1000 and len(losses["C64"]) == 1000
        evaluate(clf64, "64", torch.float64)
    finally:
        trainer.NNClassifier, trainer.optim.Adam = NNClassifier, torch.optim.Adam
        torch.nn.CrossEntropyLoss.forward = ce_forward
        shutil.rmtree(tmp, ignore_errors=True)

    out["losses"], out["losses64"] = np.asarray(losses["C"], np.float32), np.asarray(losses["C64"], np.float64)
    keys = [k[len("init.C."):] for k in out if k.startswith("init.C.")]
    for i in SNAPSHOTS:
        out[f"dist{i}"] = np.array(max(float(np.abs(out[f"it{i}.C.{k}"].astype(np.float64) - out[f"it{i}.C64.{k}"]).max()) for k in keys), np.float64)
    return out


def main(ref_root, where=HERE):
    out = record(ref_root)
    path = os.path.join(HERE, "moons_clf_ref.npz")
    if where == "--check":
        have = np.load(path)
        assert sorted(have.files) == sorted(out), "the recorded keys differ"
        bad = [k for k in out if have[k].dtype != out[k].dtype or have[k].tobytes() != out[k].tobytes()]
        assert not bad, f"arrays differ: {bad}"
        print(f"{path}: all {len(out)} arrays regenerate bit for bit")
        return
    np.savez_compressed(os.path.join(where, "moons_clf_ref.npz"), **out)
    print(f"wrote {len(out)} arrays to {os.path.join(where, 'moons_clf_ref.npz')}")
    for i in SNAPSHOTS:
        print(f"  dist{i} = {float(out[f'dist{i}']):.3e}")
    print("  " + ", ".join(f"{k} = {float(out[k]):.6g}" for k in ("acc.train", "acc.test", "final_loss", "acc64.train", "acc64.test", "final_loss64")))
    print(f"  losses[-1] = {out['losses'][-1]:.3e}, max(losses[900:]) = {out['losses'][900:].max():.3e}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
