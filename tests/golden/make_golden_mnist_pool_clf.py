"""Golden fixture for the max-pool MNIST classifier (conditional_counteRGAN/mnist/modules/classifier.py, the classifier of countergan2.py
and gan_train.py): the reference's own module, imported from the path on the command line and run on the CPU in fp32 and float64.
Writes tests/golden/mnist_pool_clf_ref.npz.

    python tests/golden/make_golden_mnist_pool_clf.py <path of the reference repository> [output directory]

Weights.  A checkpoint of this net is 1.69 MB (net.7.weight alone is 3136 x 128 floats), over the size a committed file may have, so
the shipped models/classifier.pt is NOT copied into tests/golden.  The recorded runs use the reference's module built after
torch.manual_seed(SEED) (the way mnist_cf_eval_ref.npz seeds its CNNClassifier); the tests rebuild the same weights from the same seed
and check them against the per-tensor sums recorded here.  What the script does with the shipped file, when it is there: load it into
the reference's module and into this project's (strict=True, both directions), and record its keys and shapes.

Recorded:
  seed, keys, shapes, weight_sums [8]    the seed, the state_dict's names and shapes, float64 sum and sum of squares per tensor [8][2]
  shipped_keys, shipped_shapes           the same two lists read from models/classifier.pt (empty when the file is absent)
  x [16][1][28][28], target [16]         the 11 input rows of mnist_cf_eval_ref.npz and 5 rows of randn clamped to [-1, 1] (seed 41);
                                         seeded targets
  logits32, logits64 [16][10]            the reference's logits in fp32 and float64
  pred [16], undecided [16], undecided_bound    float64 argmax; rows whose float64 top-two probability gap is under
                                         max(1e-5, 100 * max|p_fp32 - p_fp64|) (make_golden_mnist_cf_eval.py:62-66).  At most 1 of 16.
  dx64 [16][784]                         float64 gradient of CrossEntropyLoss(reduction="sum")(logits, target) w.r.t. the input
  idx{1,2} [16][C][Hp][Wp] uint8         the float64 run's window choice per pooling layer (0..3 = dh * 2 + dw)
  live{1,2}, near{1,2} (bool)            windows whose float64 maximum is > 0; live windows whose float64 top-two gap of the pre-pool
                                         activations relu(z) is under bound{1,2} = max(1e-5, 100 * max|z_fp32 - z_fp64|) of the layer
  bound{1,2}, min_gap{1,2}               those bounds, and the smallest gap among the live windows
A near window's choice is not pinned by the reference itself.  At most 0.2 % of a layer's live windows may be near; asserted here."""
import copy
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 5
NEAR_CAP = 0.002


def undecided(p32, p64):
    bound = max(1e-5, 100.0 * float(np.abs(p32.astype(np.float64) - p64).max()))
    top = np.sort(p64, axis=-1)
    return (top[..., -1] - top[..., -2]) < bound, bound


def main(ref_root, out_dir=HERE):
    import pool_clf_restate as R                 # window bookkeeping only: every recorded number comes from the reference's module
    mdir = os.path.join(ref_root, "conditional_counteRGAN", "mnist")
    sys.path.insert(0, mdir)
    clf_mod = importlib.import_module("modules.classifier")
    torch.manual_seed(SEED)
    C = clf_mod.Classifier().eval()
    C64 = copy.deepcopy(C).double()
    sd = C.state_dict()
    out = {"seed": np.int64(SEED), "keys": np.array(list(sd)), "shapes": np.array([str(tuple(v.shape)) for v in sd.values()]),
           "weight_sums": np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])}

    shipped = os.path.join(mdir, "models", "classifier.pt")
    keys, shapes = [], []
    if os.path.exists(shipped):
        ck = torch.load(shipped, map_location="cpu", weights_only=True)
        clf_mod.Classifier().load_state_dict(ck, strict=True)
        keys, shapes = list(ck), [str(tuple(v.shape)) for v in ck.values()]
        assert keys == list(sd) and shapes == list(out["shapes"])
        from pcgan_amd import countergan as K    # both directions through this project's module (parameters only: no GPU needed)
        ours = K.Classifier()
        ours.load_state_dict(ck, strict=True)
        back = clf_mod.Classifier()
        back.load_state_dict({k: v.detach().contiguous() for k, v in ours.state_dict().items()}, strict=True)
        assert all(torch.equal(back.state_dict()[k], ck[k]) for k in ck)
    out["shipped_keys"], out["shipped_shapes"] = np.array(keys, dtype=str), np.array(shapes, dtype=str)

    x11 = torch.from_numpy(np.load(os.path.join(HERE, "mnist_cf_eval_ref.npz"))["x"])
    g = torch.Generator().manual_seed(41)
    x = torch.cat([x11, torch.randn(5, 1, 28, 28, generator=g).clamp(-1.0, 1.0)])
    target = torch.randint(0, 10, (16,), generator=g)
    out["x"], out["target"] = x.numpy(), target.numpy()

    with torch.no_grad():
        l32, l64 = C(x), C64(x.double())
        z32 = [C.net[:1](x), C.net[:4](x)]
        z64 = [C64.net[:1](x.double()), C64.net[:4](x.double())]
    out["logits32"], out["logits64"], out["pred"] = l32.numpy(), l64.numpy(), l64.argmax(1).numpy()
    und, bound = undecided(F.softmax(l32, 1).numpy(), F.softmax(l64, 1).numpy())
    assert und.sum() <= 1, f"{int(und.sum())} of 16 rows undecided (bound {bound:.1e}): pick another seed"
    out["undecided"], out["undecided_bound"] = und, np.float64(bound)

    xg = x.double().requires_grad_(True)
    F.cross_entropy(C64(xg), target, reduction="sum").backward()
    out["dx64"] = xg.grad.reshape(16, 784).numpy()

    report = []
    for i, (a32, a64) in enumerate(zip(z32, z64), 1):
        b = max(1e-5, 100.0 * float((a32.double() - a64).abs().max()))
        p, idx = R.relu_pool(a64)
        gap = R.top2_gap(a64)
        live = p > 0
        near = live & (gap < b)
        frac = float(near.sum()) / float(live.sum())
        assert frac <= NEAR_CAP, f"pool {i}: {int(near.sum())} of {int(live.sum())} live windows within {b:.1e}: pick another seed"
        out[f"idx{i}"], out[f"live{i}"], out[f"near{i}"] = idx.numpy(), live.numpy(), near.numpy()
        out[f"bound{i}"], out[f"min_gap{i}"] = np.float64(b), np.float64(gap[live].min())
        report.append(f"pool {i}: {int(near.sum())} of {int(live.sum())} live windows near (bound {b:.1e}, smallest gap {float(gap[live].min()):.1e})")

    path = os.path.join(out_dir, "mnist_pool_clf_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.0f} kB; undecided rows {int(und.sum())} / 16 (bound {bound:.1e}); " + "; ".join(report)
          + f"; shipped checkpoint {'checked' if keys else 'absent'}")


if __name__ == "__main__":
    main(sys.argv[1], *(sys.argv[2:3]))
