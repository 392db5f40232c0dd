"""Host-side checks (no GPU) of the fused moons GAN / conditional GAN path: the ABI additions, the modules' state_dict contract, the
restatement (tests/moons_gan_restate.py) pinned to the reference's recorded runs, the kink precondition of every case the GPU tests
use, and the refusals that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moons_gan_restate as RS  # noqa: E402

NEW_SYMBOLS = ("pcg_moons_gan_scratch_bytes", "pcg_moons_gan_train_steps", "pcg_moons_gan_forward")


def test_new_symbols_declared_and_exported():
    from pcgan_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcgan_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in include/pcgan_hip.h"


def test_cgan_modules_have_the_recorded_keys_and_shapes(golden_dir):
    from pcgan_amd import moons_cgan as C
    gold = np.load(os.path.join(golden_dir, "moons_cgan_ref.npz"))
    G = C.Generator(C.config["z_dim"], C.config["label_dim"], C.config["hidden_dim"])
    D = C.Discriminator(C.config["label_dim"], C.config["hidden_dim"])
    for tag, net in (("G", G), ("D", D)):
        want = [k[len(f"init.{tag}."):] for k in gold.files if k.startswith(f"init.{tag}.")]
        assert list(net.state_dict().keys()) == want == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == gold[f"init.{tag}.{k}"].shape, k
        # a reference-shaped checkpoint goes in, and what comes out loads into the reference's layout (torch modules of its shape)
        net.load_state_dict({k: torch.from_numpy(gold[f"final.{tag}.{k}"].copy()) for k in want})
        for k, v in net.state_dict().items():
            assert np.array_equal(v.numpy(), gold[f"final.{tag}.{k}"])
    import torch.nn as nn

    class RefShaped(nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.net = nn.Sequential(nn.Linear(i, 128), nn.ReLU(), nn.Linear(128, o))
    r = RefShaped(34, 2)
    r.load_state_dict(G.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(r.state_dict().values(), G.state_dict().values()))
    # torch's default nn.Linear initialisation: uniform within 1 / sqrt(fan_in)
    fresh = C.Generator(32, 2, 128)
    assert float(fresh.net[0].weight.detach().abs().max()) <= 1 / np.sqrt(34) and float(fresh.net[2].bias.detach().abs().max()) <= 1 / np.sqrt(128)
    assert C.config == {"n_samples": 2000, "z_dim": 32, "hidden_dim": 128, "label_dim": 2, "batch_size": 50, "lr": 1e-3, "epochs": 500,
                        "scale_factor": 10}


def _gold_params(gold, pre):
    return {t: {k: gold[f"init.{t}.{pre}{k}"] for k in RS.G_KEYS} for t in "GD"}


def _replay_cgan(gold, dtype):
    torch.set_num_threads(1)
    m = RS.Model(_gold_params(gold, "net."), dtype=dtype)
    outs = []
    for it in range(RS.ITERS):
        sl = slice(it * RS.BATCH, (it + 1) * RS.BATCH)
        outs.append(m.step(gold["X"][sl], gold["Y"][sl], gold[f"it{it}.z_d"], gold[f"it{it}.labels_d"], gold[f"it{it}.z_g"], gold[f"it{it}.labels_g"]))
        if dtype == torch.float32:
            for tag in "GD":
                for k in RS.G_KEYS:
                    np.testing.assert_allclose(m.p[tag][k].detach().numpy(), gold[f"it{it}.{tag}.net.{k}"], rtol=1e-6, atol=1e-7, err_msg=f"it{it}.{tag}.{k}")
                    g = outs[-1]["grad_" + tag][k].numpy()
                    np.testing.assert_allclose(g, gold[f"it{it}.{tag}.grad.net.{k}"], rtol=1e-5, atol=1e-8, err_msg=f"it{it}.{tag}.grad.{k}")
    return m, outs


def _replay_moons(gold, dtype):
    torch.set_num_threads(1)
    m = RS.Model(_gold_params(gold, ""), dtype=dtype)
    outs = [m.step(gold["X_shuffled"][50 * i:50 * i + 50], None, gold["z"][2 * i], None, gold["z"][2 * i + 1], None) for i in range(2)]
    return m, outs


def test_restatement_in_fp32_reproduces_the_cgan_recording(golden_dir):
    """Pins tests/moons_gan_restate.py to the reference's own code: same losses, weights, consumed gradients and Adam state as the
    lifted script recorded, iteration by iteration (the same fp32 torch operations: equal to the last bits)."""
    gold = dict(np.load(os.path.join(golden_dir, "moons_cgan_ref.npz")))
    assert int(gold["meta.seed"]) == RS.SEED and set(np.unique(gold["Y"])) == {0, 1}
    assert all(not gold[f"it{i}.labels_d"].any() for i in range(RS.ITERS)), "the D step's fake labels are randint(0, 1): class 0 (:98)"
    assert any(gold[f"it{i}.labels_g"].any() for i in range(RS.ITERS))
    m, outs = _replay_cgan(gold, torch.float32)
    for it, o in enumerate(outs):
        np.testing.assert_allclose(o["loss_D"], float(gold[f"it{it}.loss_D"]), rtol=1e-6)
        np.testing.assert_allclose(o["loss_G"], float(gold[f"it{it}.loss_G"]), rtol=1e-6)
    for tag in "GD":
        for k in RS.G_KEYS:
            np.testing.assert_allclose(m.m[tag][k].numpy(), gold[f"it{RS.ITERS-1}.{tag}.exp_avg.net.{k}"], rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(m.v[tag][k].numpy(), gold[f"it{RS.ITERS-1}.{tag}.exp_avg_sq.net.{k}"], rtol=1e-5, atol=1e-12)
        assert m.t[tag] == int(gold[f"it{RS.ITERS-1}.{tag}.step"]) == RS.ITERS
    assert float(gold["loss_D_total"]) == pytest.approx(sum(float(gold[f"it{i}.loss_D"]) for i in range(RS.ITERS)), rel=1e-12)


def test_restatement_with_no_labels_reproduces_moons_ref(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "moons_ref.npz")))
    m, outs = _replay_moons(gold, torch.float32)
    np.testing.assert_allclose(sum(o["loss_D"] for o in outs), float(gold["loss_D_total"]), rtol=1e-6)
    np.testing.assert_allclose(sum(o["loss_G"] for o in outs), float(gold["loss_G_total"]), rtol=1e-6)
    for tag in "GD":
        for k in RS.G_KEYS:
            np.testing.assert_allclose(m.p[tag][k].detach().numpy(), gold[f"final.{tag}.{k}"], rtol=1e-6, atol=1e-7, err_msg=f"{tag}.{k}")


def test_kink_precondition_of_every_gpu_case(golden_dir):
    """ReLU's gradient jumps at 0: a hidden pre-activation within fp32 rounding of 0 makes an fp32-vs-float64 comparison meaningless.
    On the float64 oracle alone: no hidden pre-activation of any fixture or seed the GPU tests use lies within KINK_BAND x rms of 0.
    No teacher forcing, no excluded elements: the seeds were chosen so that this holds."""
    margins = {}
    _, outs = _replay_cgan(dict(np.load(os.path.join(golden_dir, "moons_cgan_ref.npz"))), torch.float64)
    margins["moons_cgan_ref.npz"] = min(RS.kink_margin(o["pre"]) for o in outs)
    _, outs = _replay_moons(dict(np.load(os.path.join(golden_dir, "moons_ref.npz"))), torch.float64)
    margins["moons_ref.npz"] = min(RS.kink_margin(o["pre"]) for o in outs)
    for B, H, Z, L, seed in RS.STEP_CASES:
        _, outs = RS.run_case(RS.random_case(B, H, Z, L, seed))
        margins[f"step {B}x{H}x{Z} L={L} seed {seed}"] = RS.kink_margin(outs[0]["pre"])
    for L in (0, 2):
        _, _, _, outs = RS.run_loop(RS.loop_case(L))
        margins[f"loop L={L} seed {RS.LOOP_SEEDS[L]}"] = min(RS.kink_margin(o["pre"]) for o in outs)
    for B, H, Z, L, seed, n in RS.MULTI_CASES:
        _, outs = RS.run_case(RS.random_case(B, H, Z, L, seed, iters=n))
        margins[f"{n} steps {B}x{H}x{Z} L={L} seed {seed}"] = min(RS.kink_margin(o["pre"]) for o in outs)
    for k, v in margins.items():
        print(f"{k}: nearest pre-activation at {v:.2e} x rms")
    bad = {k: v for k, v in margins.items() if v < RS.KINK_BAND}
    assert not bad, bad


def _cpu_nets(z=32, L=2, H=128):
    from pcgan_amd import moons_cgan as C
    return C.Generator(z, L, H), C.Discriminator(L, H)


def test_refusals_that_need_no_gpu():
    from pcgan_amd import PcgError, moons as M, moons_cgan as C
    from pcgan_amd.optim import Adam
    X, Y = RS.moons_data(120, 0)
    G, D = _cpu_nets()
    cfg = dict(C.config, n_samples=120, epochs=1)
    with pytest.raises(PcgError, match="multiple of batch_size"):         # 120 % 50 != 0: the reference's loss fails on the tail batch
        C.train(torch.from_numpy(X), torch.from_numpy(Y), G, D, cfg, verbose=False)
    with pytest.raises(PcgError, match="multiple of batch_size"):
        M.train_gan(X.astype(np.float64), M.build_generator(32, 128), M.build_discriminator(128), dict(M.config, epochs=1))
    with pytest.raises(PcgError, match="no CPU path"):                    # a CPU device
        C.train(torch.from_numpy(X[:100]), torch.from_numpy(Y[:100]), G, D, dict(cfg, n_samples=100), verbose=False)
    with pytest.raises(PcgError, match="no CPU path"):
        M.train_gan(X[:100].astype(np.float64), M.build_generator(32, 128), M.build_discriminator(128), dict(M.config, epochs=1))
    with pytest.raises(PcgError, match="no CPU path"):
        G(torch.zeros(3, 32), torch.zeros(3, 2))
    with pytest.raises(PcgError, match="no CPU path"):
        D(torch.zeros(3, 2), torch.zeros(3, 2))
    with pytest.raises(PcgError, match="no CPU path"):
        C.one_hot_encode(torch.zeros(3, dtype=torch.int64), 2)
    ok = Adam(G.parameters(), lr=1e-3), Adam(D.parameters(), lr=1e-3)
    for z, L, H, B, what in ((32, 2, 96, 50, "hidden_dim"), (30, 2, 128, 50, "z_dim"), (68, 2, 128, 50, "z_dim"), (32, 3, 128, 50, "label_dim"),
                             (32, 2, 128, 0, "batch"), (32, 2, 128, 257, "batch")):
        g, d = _cpu_nets(z, L, H)
        with pytest.raises(PcgError, match=what):
            M.TrainSteps(g, d, Adam(g.parameters()), Adam(d.parameters()), X, Y, batch_size=B)
    with pytest.raises(PcgError, match="hidden"):
        M.TrainSteps(G, C.Discriminator(2, 64), *ok, X, Y)
    with pytest.raises(PcgError, match="pcgan_amd.optim.Adam only"):
        M.TrainSteps(G, D, torch.optim.Adam(G.parameters()), ok[1], X, Y)
    with pytest.raises(PcgError, match="pcgan_amd.optim.Adam only"):
        from pcgan_amd.optim import AdamW
        M.TrainSteps(G, D, ok[0], AdamW(D.parameters()), X, Y)
    with pytest.raises(PcgError, match="weight decay"):
        M.TrainSteps(G, D, ok[0], Adam(D.parameters(), weight_decay=1e-2), X, Y)


def test_descriptor_ranges_refused_by_the_library():
    """Sizes outside the stated ranges: PCG_ERR_INVALID and a pcg_last_error text from the C entry points (no launch is attempted)."""
    from pcgan_amd import _lib, moons as M
    lib = _lib.load()
    a = _lib.MoonsGanTrainArgs()
    for kw, what in ((dict(hidden=96), "hidden_dim"), (dict(z_dim=30), "z_dim"), (dict(z_dim=68), "z_dim"), (dict(label_dim=1), "label_dim"),
                     (dict(B=0), "batch"), (dict(B=257), "batch")):
        args = dict(z_dim=32, hidden=128, label_dim=2, B=50)
        args.update(kw)
        d = M._gan_desc(args["z_dim"], args["hidden"], args["label_dim"], B=args["B"], N=100)
        rc = lib.pcg_moons_gan_train_steps(ctypes.byref(d), ctypes.byref(a), 1, None)
        assert rc != _lib.PCG_OK and what.split("_")[0] in lib.pcg_last_error().decode(), (kw, lib.pcg_last_error())
        assert lib.pcg_moons_gan_scratch_bytes(ctypes.byref(d)) == 0
    d = M._gan_desc(32, 128, 2, B=50, N=100)
    assert lib.pcg_moons_gan_scratch_bytes(ctypes.byref(d)) == 0, "the reference's 50 x 128 keeps every activation in LDS"
    assert lib.pcg_moons_gan_scratch_bytes(ctypes.byref(M._gan_desc(32, 128, 2, B=256, N=100))) > 0
    assert lib.pcg_moons_gan_train_steps(ctypes.byref(d), ctypes.byref(a), 1, None) != _lib.PCG_OK      # null pointers
    d.g_off[1] = 0                                                                                       # overlapping tensors
    assert lib.pcg_moons_gan_train_steps(ctypes.byref(d), ctypes.byref(a), 1, None) != _lib.PCG_OK and b"offset" in lib.pcg_last_error()


def test_shuffling_an_index_equals_shuffling_the_rows():
    """train_gan keeps the set resident and shuffles an index with numpy's generator: the same draws as np.random.shuffle(X) (:56)."""
    X = np.random.RandomState(0).randn(2000, 2)
    X0, order = X.copy(), np.arange(2000)
    np.random.seed(5); np.random.shuffle(X); np.random.shuffle(X)
    np.random.seed(5); np.random.shuffle(order); np.random.shuffle(order)
    assert np.array_equal(X, X0[order])
