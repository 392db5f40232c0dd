"""Resuming a run: for each of the four trainers that take checkpoint= / resume=, and each of their paths, three
uninterrupted epochs equal one epoch, a checkpoint, fresh nets, and a resume to three epochs -- bit for bit.

What is compared is the checkpoint each run writes after its third epoch -- both nets' parameters and buffers, both optimizers'
moments and step counters (the trainers keep their optimizers to themselves; the checkpoint is where they show), the DeviceRNG
offset, torch's CPU and numpy's RNG state, the histories -- plus the nets' flat buffers and the returned histories.  Every case first
runs the uninterrupted training TWICE and requires the same equality between the two: no output of these trainers turned out to
need an allowance (no floating-point atomic feeds what they return), so none is given."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_clf_restate as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import checkpoint, dcgan, gan_train, house, moons_countergan  # noqa: F401
    pcgan_amd.load()
    return pcgan_amd


def same(a, b, where="checkpoint"):
    """Bit-identical nests of dicts / lists / tensors / plain values."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), where
        for k in a:
            same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    else:
        assert a == b, (where, a, b)


def check_case(pcg, tmp_path, run, other_batch_size):
    """run(epochs, checkpoint=None, checkpoint_every=1, resume=None, interrupt_after=None, **over) -> (histories, [flat parameter
    tensors]); a fresh set of nets every call.  interrupt_after=k: the run is to stop after k epochs (a trainer whose last epoch
    differs from the others is interrupted from outside; the others just run k epochs)."""
    ck = pcg.checkpoint
    paths = [str(tmp_path / f"{n}.pt") for n in ("a", "b", "first", "resumed")]
    h_a, p_a = run(3, checkpoint=paths[0], checkpoint_every=3)
    h_b, p_b = run(3, checkpoint=paths[1], checkpoint_every=3)
    full = ck.load(paths[0])
    same(h_a, h_b, "histories of two uninterrupted runs")
    same(p_a, p_b, "parameters of two uninterrupted runs")
    same(full, ck.load(paths[1]), "checkpoints of two uninterrupted runs")
    run(3, checkpoint=paths[2], interrupt_after=1)
    first = ck.load(paths[2])
    assert ck.value(first, "epoch") == 1
    h_r, p_r = run(3, checkpoint=paths[3], resume=paths[2])
    same(h_a, h_r, "returned histories")
    same(p_a, p_r, "flat parameters")
    resumed = ck.load(paths[3])
    assert ck.value(resumed, "epoch") == 3
    same(full, resumed)
    opts = [k for k, e in full["objects"].items() if e["kind"] == "optimizer"]
    assert len(opts) == 2 and all(float(full["objects"][k]["state"]["state"][0]["step"]) > 0 for k in opts)
    # a resume at the last epoch returns the full histories (a loaded dict serves as well as the path)
    h_e, _ = run(3, resume=resumed)
    same(h_a, h_e, "histories of a resume at the last epoch")
    with pytest.raises(pcg.PcgError, match="batch_size"):
        run(3, resume=paths[2], batch_size=other_batch_size)


# ---- moons CounteRGAN: the epoch-per-launch kernel (hidden 32, batch 64, three iterations per epoch) --------------------------------
def test_moons_countergan(pcg, tmp_path):
    M = pcg.moons_countergan
    gold = dict(np.load(os.path.join(GOLD, "moons_cf_ref.npz")))
    X, y = gold["data.X_train"][:200], gold["data.y_train"][:200]
    cfg0 = {"seed": 42, "batch_size": 64, "lr_G": 1e-3, "lr_D": 1e-3, "lambda_cls": 2.0, "lambda_reg_l1": 5.0, "lambda_reg_l2": 5.0,
            "lambda_mask": 3.0, "input_dim": 2, "hidden_dim": 32, "out_dir": str(tmp_path), "clf_model_path": "", "generator_path": "", "cuda": DEV}

    def run(epochs, interrupt_after=None, batch_size=64, **kw):
        G = M.ResidualGenerator(2, 32, 3)
        G.load_state_dict({k[7:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("init.G.")})
        C = M.NNClassifier(2)
        C.load_state_dict({k[7:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("init.C.")})
        cfg = dict(cfg0, epochs=interrupt_after or epochs, batch_size=batch_size)
        res = M.train_countergan(G, cfg, X, y, C, verbose=False, save=False, **kw)
        D = res["discriminator"]
        return {"d_losses": res["d_losses"], "g_losses": res["g_losses"]}, [G.flat_params.clone(), D.flat_params.clone()]

    check_case(pcg, tmp_path, run, other_batch_size=32)


# ---- house-sales CounteRGAN: the small config of tests/test_hip_house.py, graph on and off ------------------------------------------
class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi


@pytest.mark.parametrize("graph", [True, False])
def test_house_countergan(pcg, tmp_path, graph):
    H = pcg.house
    g = dict(np.load(os.path.join(GOLD, "house_loop.npz")))
    cfg0 = dict(H.CONFIG)
    cfg0["categorical_info"] = {f: {"n": len(g[f"raw_values.{f}"]), "raw_values": g[f"raw_values.{f}"].tolist()} for f in H.CONFIG["categorical_info"]}
    cfg0.update({"scaler": _Scaler(g["scaler.data_min"], g["scaler.data_max"]), "seed": int(g["meta.seed"]), "cuda": DEV})

    def run(epochs, interrupt_after=None, batch_size=32, **kw):
        torch.manual_seed(0)
        C = H.NNClassifier(17, 4)
        G = H.ResidualGenerator(17, 32, 4, cfg0["continuous_idx"], cfg0["categorical_info"], tau=0.5)
        G.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("init.G.")})
        C.eval()
        for p in C.parameters():
            p.requires_grad = False
        cfg = dict(cfg0, epochs=interrupt_after or epochs, batch_size=batch_size)
        hist = H.train_countergan(G, cfg, g["data.X"], g["data.y"], C, graph=graph, verbose=False, save=False, **kw)
        D = hist.pop("discriminator")
        return hist, [G.flat_params.clone(), D.flat_params.clone()]

    check_case(pcg, tmp_path, run, other_batch_size=16)


def test_house_stepper_built_from_restored_state(pcg):
    """house.GraphedTrainStep built after a restore: its device counter starts at the restored offset, and the warm-up steps of its
    constructor (snapshot -> real steps -> restore) leave a loaded, still pending optimizer state as it was loaded."""
    H, ops = pcg.house, pcg.ops
    g = dict(np.load(os.path.join(GOLD, "house_loop.npz")))
    cfg = dict(H.CONFIG, num_classes=4, cuda=DEV)
    cfg["categorical_info"] = {f: {"n": len(g[f"raw_values.{f}"]), "raw_values": g[f"raw_values.{f}"].tolist()} for f in H.CONFIG["categorical_info"]}
    cfg["scaler"] = _Scaler(g["scaler.data_min"], g["scaler.data_max"])
    torch.manual_seed(0)
    C = H.NNClassifier(17, 4).to(DEV).eval()
    for p in C.parameters():
        p.requires_grad = False
    G = H.ResidualGenerator(17, 32, 4, cfg["continuous_idx"], cfg["categorical_info"], tau=0.5).to(DEV)
    D = H.Discriminator(cfg["input_dim"], cfg["hidden_dim"], 4).to(DEV)
    opt_g, opt_d = H.make_optimizers(G, D, cfg)
    gen = torch.Generator().manual_seed(1)
    loaded = []
    for net, opt in ((G, opt_g), (D, opt_d)):
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(2.0), "exp_avg": torch.randn(p.shape, generator=gen), "exp_avg_sq": torch.rand(p.shape, generator=gen)}
                       for i, p in enumerate(net.parameters())}
        opt.load_state_dict(sd)
        assert opt._segments is None and opt._pending is not None
        loaded.append(sd["state"])
    src = ops.DeviceRNG(seed=42)
    src.offset = 1234
    rng = ops.DeviceRNG(seed=0)
    rng.set_state(src.get_state())
    gs = H.GraphedTrainStep(G, D, C, opt_g, opt_d, H.cat_norm_maps(G, cfg, torch.device(DEV)), 32, cfg, rng=rng)
    assert int(gs._ctr[0]) == 1234 and rng.offset == 1234 and rng.seed == 42
    for opt, want in zip((opt_g, opt_d), loaded):
        assert opt._segments is not None and opt._pending is None      # the warm-up built the segments and consumed the pending state
        got = opt.state_dict()["state"]
        assert sorted(got) == sorted(want)
        for i in want:
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(got[i][k].cpu(), want[i][k]), (i, k)


# ---- gan_train.train_gan: batch 8, two batches per epoch; op chain, fused, fused with the class drawn inside the step ---------------
@pytest.mark.parametrize("fused,drawn", [(False, False), (True, False), (True, True)])
def test_delta_gan(pcg, tmp_path, fused, drawn):
    T, K, ops = pcg.gan_train, pcg.countergan, pcg.ops
    from pcgan_amd.data import DeviceLoader
    gen = torch.Generator().manual_seed(3)
    x = (2 * torch.rand(16, 1, 28, 28, generator=gen) - 1).to(DEV)
    y = torch.randint(0, 10, (16,), generator=gen).to(DEV)
    base = T.params_random_target if drawn else T.params
    offsets = []

    def run(epochs, interrupt_after=None, batch_size=8, **kw):
        torch.manual_seed(5)
        G, D = T.Generator().to(DEV), T.Discriminator().to(DEV)
        C = K.Classifier()
        C.load_state_dict(PR.seeded_state(PR.SEED), strict=True)
        C = C.to(DEV).eval()
        rng = ops.DeviceRNG(seed=9) if drawn else None
        loader = DeviceLoader(x, y, 8, shuffle=True, seed=4)                    # its generator decides the batches: part of the state
        params = dict(base, batch_size=batch_size, epochs_gan=interrupt_after or epochs, **kw)   # checkpoint / checkpoint_every / resume: keys of params
        hist = T.train_gan(G, D, C, loader, params, fused=fused, rng=rng, verbose=False)
        offsets.append(rng.offset if drawn else None)
        return hist, [G.flat_params.clone(), D.flat_params.clone()]

    check_case(pcg, tmp_path, run, other_batch_size=4)
    if drawn:   # one class per iteration, two iterations per epoch: two full runs, the first epoch, the resumed run, the resume at the end
        assert offsets == [6, 6, 2, 6, 0]


def test_delta_gan_stepper_starts_at_a_restored_offset(pcg):
    """A stepper built from a restored rng makes its device counter from the restored offset."""
    T, K, ops = pcg.gan_train, pcg.countergan, pcg.ops
    src = ops.DeviceRNG(seed=9)
    src.offset = 41
    rng = ops.DeviceRNG(seed=0)
    rng.set_state(src.get_state())
    C = K.Classifier()
    C.load_state_dict(PR.seeded_state(PR.SEED), strict=True)
    stepper = T.GraphedTrainStep(T.Generator().to(DEV), T.Discriminator().to(DEV), C.to(DEV).eval(), 8, T.params_random_target, rng=rng)
    assert stepper._ctr.tolist() == [41, 0] and stepper._rng.seed == 9


# ---- DCGAN: the widths of tests/golden/dcgan_loop_small.npz, two batches per epoch; device noise and host noise ---------------------
class _Interrupted(Exception):
    pass


class _Batches:
    """A loader that is interrupted from outside: it refuses to start one epoch more than `allowed`."""

    def __init__(self, data, allowed=None):
        self.data, self.allowed, self.started = data, allowed, 0

    def __len__(self):
        return len(self.data)

    def __iter__(self):
        if self.allowed is not None and self.started == self.allowed:
            raise _Interrupted()
        self.started += 1
        return iter(self.data)


@pytest.mark.parametrize("device_noise", [True, False])
def test_dcgan(pcg, tmp_path, device_noise):
    """dcgan.train's last epoch ends with a train-mode viz forward that moves the generator's BatchNorm statistics, so the run to
    continue is one that was interrupted after its first epoch (cfg["epochs"] = 3 throughout), not one that ended there."""
    D, ops = pcg.dcgan, pcg.ops
    gold = dict(np.load(os.path.join(GOLD, "dcgan_loop_small.npz")))
    cfg0 = {"g_hidden": int(gold["meta.g_hidden"]), "d_hidden": int(gold["meta.d_hidden"]), "z_dim": int(gold["meta.z_dim"])}
    data = [(torch.from_numpy(gold[f"data.{k}"]),) for k in range(2)]
    imgs = []

    def run(epochs, interrupt_after=None, batch_size=int(gold["meta.batch"]), **kw):
        cfg = dict(cfg0, batch_size=batch_size, epochs=epochs)
        netG, netD = D.Generator(cfg), D.Discriminator(cfg)
        netG.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.G.")})
        netD.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.D.")})
        netG.to(DEV); netD.to(DEV)
        torch.manual_seed(int(gold["meta.loop_seed"]))                          # host noise: torch's global CPU generator
        rng = ops.DeviceRNG(seed=21) if device_noise else None
        args = dict(netG=netG, netD=netD, device=DEV, log=lambda s: None, device_rng=rng, **kw)
        if interrupt_after is not None:
            with pytest.raises(_Interrupted):
                D.train(_Batches(data, allowed=interrupt_after), cfg, **args)
            return None
        out = D.train(_Batches(data), cfg, **args)
        imgs.append(out["img_list"])
        return ({"epoch_G_losses": out["epoch_G_losses"], "epoch_D_losses": out["epoch_D_losses"], "iters": out["iters"]},
                [netG.flat_params.clone(), netD.flat_params.clone()])

    check_case(pcg, tmp_path, run, other_batch_size=2)
    # img_list: the uninterrupted runs hold the viz batch of iteration 0 and the final one, the resumed run only what it made itself
    assert [len(v) for v in imgs] == [2, 2, 1, 0]
    assert torch.equal(imgs[0][1], imgs[2][0]) and torch.equal(imgs[0][1], imgs[1][1])
