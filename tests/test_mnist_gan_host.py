"""CPU: the host mirror of simple_gan/mnist/mnist_gan.py (pcgan_amd.mnist_gan) against the fixture recorded from the reference's own
code (tests/golden/mnist_gan_ref.npz, made by tests/golden/make_golden_mnist_gan.py): state_dict layout, checkpoint round trip, the
no-CPU-path error, and the test-side fp32 restatement (tests/mnist_gan_restate.py), which must reproduce the reference run exactly
enough to serve as its float64 twin's definition on the GPU tests."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnist_gan_restate as RS  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_gan_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import mnist_gan
    return mnist_gan


def test_new_entry_points_are_declared_and_bound():
    from pcgan_amd import _lib
    for name in ("pcg_dense_rows_fwd", "pcg_dense_rows_dgrad", "pcg_dense_rows_wgrad"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)


def test_config_is_the_reference_default(M):
    assert M.config == {"epochs": 200, "batch_size": 64, "learning_rate": 0.0002, "b1": 0.5, "b2": 0.999, "latent_dim": 100, "img_size": 28,
                        "channels": 1}


def test_state_dict_keys_and_shapes_equal_the_recorded_ones(M, gold):
    for tag, net in (("G", M.Generator()), ("D", M.Discriminator())):
        want = {k[len(f"shape.{tag}."):]: tuple(int(v) for v in a) for k, a in gold.items() if k.startswith(f"shape.{tag}.")}
        have = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert list(have) == list(want) and have == want
    assert M.Generator().model[3].eps == 0.8           # nn.BatchNorm1d(output_size, 0.8): the eps slot (:48)


def test_reference_shaped_checkpoint_round_trips(M):
    G32, D32 = RS.build(torch.float32)
    G, D = M.Generator(), M.Discriminator()
    G.load_state_dict(G32.state_dict()); D.load_state_dict(D32.state_dict())
    G2, D2 = RS.build(torch.float32, seed=99)
    G2.load_state_dict(G.state_dict()); D2.load_state_dict(D.state_dict())
    for a, b in ((G32, G2), (D32, D2)):
        for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k == k2 and torch.equal(v, v2), k


def test_no_cpu_path(M):
    import pcgan_amd
    G, D = M.Generator(), M.Discriminator()
    with pytest.raises(pcgan_amd.PcgError, match="no CPU path"):
        G(torch.zeros(4, 100))
    with pytest.raises(pcgan_amd.PcgError, match="no CPU path"):
        D(torch.zeros(4, 1, 28, 28))
    with pytest.raises(pcgan_amd.PcgError, match="no CPU path"):
        M.train_step(G, D, None, None, torch.zeros(4, 784), torch.zeros(4, 100))


def test_inputs_are_the_recorded_ones(gold):
    data = RS.inputs()
    assert tuple(int(v) for v in gold["meta.sizes"]) == RS.SIZES and int(gold["meta.seed"]) == RS.SEED
    for it, (real, _) in enumerate(data):
        assert np.array_equal(real, RS.normalize_u8(gold[f"real_u8.{it}"]))
        assert real.min() >= -1.0 and real.max() <= 1.0


def test_initialisation_matches_the_recorded_digests(gold):
    G, D = RS.build(torch.float32)
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            assert np.array_equal(RS.digest(v), gold[f"init.{tag}.{k}#digest"]), f"initialisation of {tag}.{k} differs from the reference run's"


def test_fp32_restatement_reproduces_the_reference_run(gold):
    """Same torch, same operations in the same order, one CPU thread like the recording: the restatement is the reference loop body.
    Bound 1e-5 relative L2 (another CPU's GEMM blocking may reorder sums; fp32 noise of these quantities is below 1e-6).  The six
    gradient-free tensors (mnist_gan_restate.GRADIENT_FREE and the running means that contain them) hold Adam-normalised rounding
    noise: each of the `it + 1` steps moves them by at most 3.2 lr (tests/test_hip_moons_cf.py), so that is their bound."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # summation order of the CPU GEMMs depends on the thread count
    try:
        G, D = RS.build(torch.float32)
        og, od = RS.optimizers(G, D)
        worst = 0.0
        for it, n in enumerate(RS.SIZES):
            real, z = torch.from_numpy(RS.normalize_u8(gold[f"real_u8.{it}"])), torch.from_numpy(gold[f"z.{it}"])
            o = RS.step(G, D, og, od, real, z, keep_grads=True)
            assert abs(o["g_loss"] - float(gold[f"it{it}.g_loss"])) <= 1e-6 and abs(o["d_loss"] - float(gold[f"it{it}.d_loss"])) <= 1e-6
            for name in ("d_fake_g", "d_real", "d_fake"):
                np.testing.assert_allclose(o[name].numpy(), gold[f"it{it}.{name}"], rtol=0, atol=1e-6)
            for tag, net, grads in (("G", G, o["g_grads"]), ("D", D, o["d_grads"])):
                for k, v in list(net.state_dict().items()) + [("grad." + k, g) for k, g in grads.items()]:
                    key = f"it{it}.{tag}.{k}"
                    if tag == "G" and k in RS.GRADIENT_FREE + RS.INHERITS_GRADIENT_FREE:
                        assert np.abs(RS.np64(v) - gold[key]).max() <= (it + 1) * 3.2 * RS.LR, key
                    elif tag == "G" and k[len("grad."):] in RS.GRADIENT_FREE:
                        assert np.abs(gold[key]).max() <= 1e-7, key          # exactly 0 in exact arithmetic
                    else:
                        a, b = (RS.digest(v)[1:], gold[key + "#digest"][1:]) if key + "#digest" in gold else (RS.np64(v), gold[key])
                        worst = max(worst, RS.rel_l2(a, b))
        np.testing.assert_allclose(o["fake"].numpy(), gold["last.fake"], rtol=0, atol=1e-5)
    finally:
        torch.set_num_threads(threads)
    print(f"worst relative L2 distance of the restatement from the recorded run: {worst:.2e}")
    assert worst <= 1e-5
