"""Golden fixtures for the moons CounteRGAN (conditional_counteRGAN/moons): the reference's own data_utils, models and trainer run on
the CPU, unmodified — scikit-learn and matplotlib must be importable.  Writes tests/golden/moons_cf_ref.npz and copies the two
checkpoints the reference ships (results/generator.pt, results/classifier.pt) next to it.

    python tests/golden/make_golden_moons_cf.py <path of the reference repository> [output directory]

Recorded:
  data.{X_train,X_test,y_train,y_test}   load_and_preprocess(42)
  init.{G,D,C}.<key>                     the seeded initial generator (torch.manual_seed(0) before construction), the critic as
                                         train_countergan builds it (after its own seeding), the shipped trained classifier
  rows [15][64], target_y [15][64], mask [15][64][2]
                                         one epoch (batch 64): the DataLoader's row order (RandomSampler.__iter__), and both
                                         torch.randint draws of every iteration (target after the collision rule, mask)
  logs [15][9]                           D_loss, G_loss, mean sigmoid(D_real), mean sigmoid(D_fake), g_adv, g_cls, reg_l1, reg_l2,
                                         mask_pen of every iteration (the trainer's locals at its print condition, trainer.py:109)
  it{i}.{G,D}.<key>                      full state_dicts after iteration i (snapshot at opt_G.step)
  it{i}.opt{G,D}.<param>.{exp_avg,exp_avg_sq}, it{i}.opt{G,D}.step
  eval.{x,onehot,mask,raw,masked,logits} the shipped generator in eval mode on the test split (seeded targets != y and masks), and
                                         the shipped classifier's logits there
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref_root, out_dir=HERE):
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "moons")
    sys.path.insert(0, mdir)
    import data_utils
    import trainer
    from models.discriminator import Discriminator
    from models.generator import ResidualGenerator
    from models.nn_classifier import NNClassifier
    from config import config as ref_config

    out = {}
    X_train, X_test, y_train, y_test = data_utils.load_and_preprocess(42)
    for k, v in zip(("X_train", "X_test", "y_train", "y_test"), (X_train, X_test, y_train, y_test)):
        out[f"data.{k}"] = np.asarray(v)

    clf = NNClassifier(2)
    clf.load_state_dict(torch.load(os.path.join(mdir, "results", "classifier.pt"), map_location="cpu"))
    clf.eval()
    torch.manual_seed(0)
    G = ResidualGenerator(2, 32, num_classes=3)
    for tag, net in (("G", G), ("C", clf)):
        for k, v in net.state_dict().items():
            out[f"init.{tag}.{k}"] = v.detach().clone().numpy()

    # ---- hooks ------------------------------------------------------------------------------------------------------------------
    rec = {"rows": [], "randint": [], "logs": [], "snap": []}
    holder = {}
    sampler_iter = torch.utils.data.RandomSampler.__iter__

    def rec_sampler(self):
        idx = list(sampler_iter(self))
        rec["rows"].append(idx)
        return iter(idx)

    real_randint = torch.randint

    def rec_randint(*a, **k):
        t = real_randint(*a, **k)
        rec["randint"].append(t.clone())
        return t

    class RecDiscriminator(Discriminator):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            holder["D"] = self
            for key, v in self.state_dict().items():
                out[f"init.D.{key}"] = v.detach().clone().numpy()

    class RecAdam(torch.optim.Adam):
        def __init__(self, params, **k):
            params = list(params)
            super().__init__(params, **k)
            self.tag = "G" if "optG" not in holder else "D"
            holder["opt" + self.tag] = self

        def step(self, closure=None):
            r = super().step(closure)
            if self.tag == "G":
                holder.setdefault("n", 0)
                i = holder["n"]
                holder["n"] += 1
                snap = {}
                for tag, net in (("G", G), ("D", holder["D"])):
                    for key, v in net.state_dict().items():
                        snap[f"it{i}.{tag}.{key}"] = v.detach().clone().numpy()
                for tag, net in (("G", G), ("D", holder["D"])):
                    opt = holder["opt" + tag]
                    for name, p in net.named_parameters():
                        st = opt.state[p]
                        snap[f"it{i}.opt{tag}.{name}.exp_avg"] = st["exp_avg"].clone().numpy()
                        snap[f"it{i}.opt{tag}.{name}.exp_avg_sq"] = st["exp_avg_sq"].clone().numpy()
                        snap[f"it{i}.opt{tag}.step"] = np.array(int(st["step"]), np.int64)
                rec["snap"].append(snap)
            return r

    code = trainer.train_countergan.__code__
    names = ("D_loss", "G_loss", "d_real_p", "d_fake_p", "G_adv_loss", "G_cls_loss", "G_reg_loss_l1", "G_reg_loss_l2", "mask_penalty_pre")

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(fr, ev, ar):
            if ev == "line" and fr.f_lineno == 109:          # `if (epoch+1) % (config['epochs']*0.1) == 0 ...`
                loc = fr.f_locals
                rec["logs"].append([float(loc[n].item()) if torch.is_tensor(loc[n]) else float(loc[n]) for n in names])
            return local
        return local

    cfg = dict(ref_config)
    tmp = tempfile.mkdtemp()
    cfg.update(epochs=1, cuda="cpu", out_dir=tmp, generator_path=os.path.join(tmp, "generator.pt"))
    torch.utils.data.RandomSampler.__iter__ = rec_sampler
    torch.randint = rec_randint
    trainer.Discriminator, trainer.optim.Adam = RecDiscriminator, RecAdam
    sys.settrace(tracer)
    try:
        trainer.train_countergan(G, cfg, X_train, y_train, clf)
    finally:
        sys.settrace(None)
        torch.utils.data.RandomSampler.__iter__ = sampler_iter
        torch.randint = real_randint
        trainer.optim.Adam = torch.optim.Adam
        shutil.rmtree(tmp, ignore_errors=True)

    steps = len(X_train) // cfg["batch_size"]
    rows = np.asarray(rec["rows"][0][:steps * cfg["batch_size"]], np.int64).reshape(steps, -1)
    y = np.asarray(y_train)
    ty, mk = [], []
    for i in range(steps):
        t = rec["randint"][2 * i]
        yb = torch.as_tensor(y[rows[i]], dtype=torch.long)
        ty.append(torch.where(t == yb, (t + 1) % 3, t).numpy())
        mk.append(rec["randint"][2 * i + 1].float().numpy())
    out["rows"], out["target_y"], out["mask"] = rows, np.stack(ty).astype(np.int64), np.stack(mk).astype(np.float32)
    out["logs"] = np.asarray(rec["logs"], np.float64)
    assert out["logs"].shape == (steps, 9) and len(rec["snap"]) == steps
    for snap in rec["snap"]:
        out.update(snap)

    # ---- the shipped checkpoints in eval mode on the test split ---------------------------------------------------------------
    Gt = ResidualGenerator(2, 32, num_classes=3)
    Gt.load_state_dict(torch.load(os.path.join(mdir, "results", "generator.pt"), map_location="cpu"))
    Gt.eval()
    g = torch.Generator().manual_seed(7)
    xt = torch.tensor(X_test, dtype=torch.float32)
    yt = torch.as_tensor(np.asarray(y_test), dtype=torch.long)
    tgt = (yt + torch.randint(1, 3, yt.shape, generator=g)) % 3
    onehot = torch.nn.functional.one_hot(tgt, 3).float()
    mask = torch.randint(0, 2, xt.shape, generator=g).float()
    with torch.no_grad():
        raw, masked = Gt(xt, onehot, mask)
        logits = clf(xt)
    for k, v in (("x", xt), ("onehot", onehot), ("mask", mask), ("raw", raw), ("masked", masked), ("logits", logits)):
        out[f"eval.{k}"] = v.numpy()

    np.savez_compressed(os.path.join(out_dir, "moons_cf_ref.npz"), **out)
    shutil.copyfile(os.path.join(mdir, "results", "generator.pt"), os.path.join(out_dir, "moons_cf_generator_trained.pt"))
    shutil.copyfile(os.path.join(mdir, "results", "classifier.pt"), os.path.join(out_dir, "moons_cf_classifier_trained.pt"))
    print(f"wrote {len(out)} arrays to {os.path.join(out_dir, 'moons_cf_ref.npz')}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
