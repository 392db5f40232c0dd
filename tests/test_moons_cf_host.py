"""CPU: the moons CounteRGAN's host side (pcgan_amd.moons_countergan) against the reference's own arrays and modules
(tests/golden/moons_cf_ref.npz, written by tests/golden/make_golden_moons_cf.py).  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "moons_cf_ref.npz")))


@pytest.fixture(scope="module")
def M():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import moons_countergan
    return moons_countergan


def test_load_and_preprocess_bit_identical(gold, M):
    out = M.load_and_preprocess(42)
    for k, v in zip(("X_train", "X_test", "y_train", "y_test"), out):
        ref = gold[f"data.{k}"]
        assert v.shape == ref.shape and v.dtype.kind == ref.dtype.kind, k
        assert np.array_equal(v, ref), k


def test_state_dict_keys_and_shapes(gold, M):
    nets = {"G": M.ResidualGenerator(2, 32, 3), "D": M.Discriminator(2, 32, 3), "C": M.NNClassifier(2)}
    for tag, net in nets.items():
        ref = {k[len(f"init.{tag}."):]: v for k, v in gold.items() if k.startswith(f"init.{tag}.")}
        sd = net.state_dict()
        assert list(sd) == list(ref), tag
        for k, v in sd.items():
            assert tuple(v.shape) == ref[k].shape, f"{tag}.{k}"


def test_shipped_checkpoints_load_strict(M):
    G = M.ResidualGenerator(2, 32, 3)
    G.load_state_dict(torch.load(os.path.join(GOLD, "moons_cf_generator_trained.pt"), map_location="cpu"), strict=True)
    C = M.NNClassifier(2)
    C.load_state_dict(torch.load(os.path.join(GOLD, "moons_cf_classifier_trained.pt"), map_location="cpu"), strict=True)


def test_discriminator_init_matches_reference_draws(gold, M):
    """train_countergan builds D right after torch.manual_seed(config['seed']): the same constructor draws give the same weights."""
    torch.manual_seed(42)
    np.random.seed(42)
    D = M.Discriminator(2, 32, 3)
    for k, v in D.state_dict().items():
        assert np.array_equal(v.numpy(), gold[f"init.D.{k}"]), k


@pytest.mark.parametrize("hidden,clf_hidden,batch", [(48, 32, 64), (16, 32, 64), (32, 64, 64), (32, 32, 1), (32, 32, 513)])
def test_unsupported_shapes_refused_before_launch(M, hidden, clf_hidden, batch):
    from pcgan_amd import PcgError
    with pytest.raises(PcgError):
        M._check_dims(2, hidden, 3, clf_hidden=clf_hidden, batch=batch)
    if hidden not in (32, 64):
        G = M.ResidualGenerator(2, hidden, 3)
        with torch.no_grad(), pytest.raises(PcgError, match="hidden_dim"):
            G(torch.zeros(4, 2), torch.zeros(4, 3), torch.zeros(4, 2))     # refused before any device work
        D = M.Discriminator(2, hidden, 3)
        with torch.no_grad(), pytest.raises(PcgError, match="hidden_dim"):
            D(torch.zeros(4, 2), torch.zeros(4, 3))
    if clf_hidden != 32:
        C = M.NNClassifier(2, hidden_dim=clf_hidden)
        with torch.no_grad(), pytest.raises(PcgError, match="classifier"):
            C(torch.zeros(4, 2))
    with pytest.raises(PcgError):
        M._check_dims(3, 32, 3)


def test_forward_with_grad_refused(M):
    from pcgan_amd import PcgError
    C = M.NNClassifier(2)
    with pytest.raises(PcgError):
        C(torch.zeros(4, 2))     # on the CPU: refused (no CPU path) before anything else runs


@pytest.mark.parametrize("epochs", [1, 10, 500])
def test_print_condition_matches_reference_expression(M, epochs):
    cfg = {"epochs": epochs}
    for epoch in range(epochs):
        for batch_idx in range(15):
            ref = (epoch + 1) % (cfg["epochs"] * 0.1) == 0 and batch_idx % 5 == 0     # trainer.py:109
            assert M.log_now(epoch, batch_idx, epochs) == ref


def test_config_keys(M):
    assert M.config == {"seed": 42, "epochs": 500, "batch_size": 64, "lr_G": 1e-3, "lr_D": 1e-3, "lambda_cls": 2.0, "lambda_reg_l1": 5.0,
                        "lambda_reg_l2": 5.0, "lambda_mask": 3.0, "input_dim": 2, "hidden_dim": 32, "out_dir": "results",
                        "clf_model_path": "results/classifier.pt", "generator_path": "results/generator.pt", "cuda": "cuda"}
