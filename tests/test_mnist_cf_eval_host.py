"""CPU: the host side of the MNIST CounteRGAN's prompted queries and per-target evaluation (pcgan_amd.countergan) —
the patch selection against the reference's own draws (tests/golden/mnist_cf_eval_ref.npz, made by make_golden_mnist_cf_eval.py),
the bit words, the fold of the group sums into the reference's table, the CSV text, the argument structs and the BatchNorm-fold
cache.  Nothing here touches a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import pcgan_amd
from pcgan_amd import _lib
from pcgan_amd import countergan as K

PcgError = pcgan_amd.PcgError
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLD, "mnist_cf_eval_ref.npz")))


# ---- patch selection (eval_utils.py:239-282) -----------------------------------------------------------------------------------------
def test_choose_patches_selects_the_references_patches(ref):
    """Same np.random calls in the same order: under the same seed every case of the golden file (shared, per sample, a user's list
    honoured and ignored, patch sizes 7, 5 and 4) picks exactly the reference's patches."""
    cases = json.loads(str(ref["sel.cases"]))
    assert {"shared7", "sample7", "user7", "shared5", "sample5", "user4", "empty7"} <= set(cases)
    for name, case in cases.items():
        total = (28 // case["patch_size"]) ** 2
        kw = dict(case["kwargs"])
        np.random.seed(case["seed"])
        lists = K.choose_patches(case["bs"], total, **kw)
        want = ref[f"sel.{name}.chosen"]
        if kw.get("shared_per_batch"):
            assert len(lists) == 1
            lists = lists * case["bs"]
        got = np.zeros_like(want)
        for r, chosen in enumerate(lists):
            for p in chosen:
                if 0 <= p < total:
                    got[r, p] = 1
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_choose_patches_clips_the_counts_as_the_reference_does():
    np.random.seed(0)
    assert all(len(c) == 16 for c in K.choose_patches(3, 16, min_patches=40, max_patches=99))       # min > max -> min = max = total
    np.random.seed(0)
    assert all(1 <= len(c) <= 8 for c in K.choose_patches(5, 16, min_patches=0))                    # max defaults to total // 2, min >= 1
    assert K.choose_patches(2, 16, modifiable_patches=[3, 3, 99], randomize_per_sample=False) == [[3, 3, 99], [3, 3, 99]]


def test_patch_bits():
    assert K.patch_bits([], 16) == 0
    assert K.patch_bits([0, 3, 3], 16) == 0b1001
    assert K.patch_bits([1, 16, -1, 99], 16) == 0b10                       # outside [0, total): ignored (eval_utils.py:251-252)
    assert K.patch_bits([31, 32, 48], 49) == (1 << 31) | (1 << 32) | (1 << 48)
    assert K.patch_bits([63], 64) == -(1 << 63)                            # the int64 an uploaded word holds
    assert torch.tensor([K.patch_bits(range(64), 64)], dtype=torch.int64).item() == -1
    with pytest.raises(PcgError, match="64-bit"):
        K.patch_bits([0], 65)


# ---- the fold of the group sums (eval_utils.py:61-66, :97-102, :313-335) ---------------------------------------------------------------
def _sums():
    """[T = 2][J = 3][8]: batches of 4, 4 and a ragged 3 rows; target 1 has an empty last group."""
    s = np.zeros((2, 3, 8))
    #            flips max gain_cf gain_orig |dx|   |in|   |out|  count
    s[0, 0] = [4.0, 1.0, 2.0, 1.0, 784.0, 392.0, 196.0, 4.0]
    s[0, 1] = [2.0, 1.0, 1.0, -1.0, 1568.0, 0.0, 784.0, 4.0]
    s[0, 2] = [0.0, 0.0, -0.75, 0.3, 235.2, 23.52, 2.352, 3.0]
    s[1, 0] = [1.0, 1.0, 0.4, 0.0, 0.0, 0.0, 0.0, 4.0]
    s[1, 1] = [3.0, 1.0, 0.8, 0.0, 3136.0, 0.0, 0.0, 4.0]
    return s


def test_metrics_from_sums_per_group():
    m = K.metrics_from_sums(_sums(), 784)
    np.testing.assert_allclose(m["class_flip_rate"][0], [1.0, 0.5, 0.0])
    np.testing.assert_allclose(m["class_flip_max"][0], [1.0, 1.0, 0.0])
    np.testing.assert_allclose(m["prediction_gain"][0], [0.5, 0.25, -0.25])
    np.testing.assert_allclose(m["prediction_gain_orig"][0], [0.25, -0.25, 0.1])
    np.testing.assert_allclose(m["actionability"][0], [0.25, 0.5, 0.1])
    np.testing.assert_allclose(m["allowed_l1"][0], [0.125, 0.0, 0.01])
    np.testing.assert_allclose(m["mask_penalty_pre"][0], [0.0625, 0.25, 0.001])
    assert np.isnan(m["class_flip_rate"][1, 2]) and m["count"][1, 2] == 0
    assert all(v.dtype == np.float64 for v in m.values())
    with pytest.raises(PcgError):
        K.metrics_from_sums(np.zeros((2, 7)), 784)


def test_fold_groups_is_the_mean_of_the_batch_means():
    f = K.fold_groups(_sums(), 784)
    # the ragged batch of 3 weighs as much as the full ones (eval_utils.py:97-102), it is NOT the mean over the 11 rows
    np.testing.assert_allclose(f["class_flip_rate"], [(1.0 + 0.5 + 0.0) / 3, (0.25 + 0.75) / 2])
    assert abs(f["class_flip_rate"][0] - 6.0 / 11.0) > 0.04
    np.testing.assert_allclose(f["prediction_gain"], [(0.5 + 0.25 - 0.25) / 3, (0.1 + 0.2) / 2])
    np.testing.assert_allclose(f["actionability"], [(0.25 + 0.5 + 0.1) / 3, (0.0 + 1.0) / 2])
    assert "count" not in f
    with pytest.raises(PcgError):
        K.fold_groups(np.zeros((3, 8)), 784)


def test_fold_groups_float32_sums_are_folded_in_float64():
    s = _sums().astype(np.float32)
    f = K.fold_groups(s, 784)
    assert f["class_flip_rate"].dtype == np.float64
    np.testing.assert_allclose(f["class_flip_rate"], [0.5, 0.5], rtol=1e-15)


# ---- the CSV text (eval_utils.py:104-107) ------------------------------------------------------------------------------------------------
def test_per_class_csv_is_the_references_file_format(ref):
    """The reference's own file, re-written from its parsed numbers, comes back byte for byte (pandas writes floats in their shortest
    repr, an empty first header cell and the class as the index)."""
    text = str(ref["table.csv"])
    rows = [ln.split(",") for ln in text.strip().split("\n")]
    assert rows[0] == ["", "class_flip_rate", "prediction_gain", "actionability"] and len(rows) == 11
    table = {int(r[0]): {k: float(v) for k, v in zip(rows[0][1:], r[1:])} for r in rows[1:]}
    assert K.per_class_csv(table) == text
    np.testing.assert_array_equal(np.array([[table[c][k] for k in K.PER_CLASS_FIELDS] for c in range(10)]), ref["table.metrics"])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_argument_structs_have_the_librarys_sizes():
    lib = pcgan_amd.load()
    for name in ("pcg_patch_mask_bits_args", "pcg_mnist_cf_entry_args", "pcg_mnist_cf_tail_args", "pcg_mnist_cf_score_args"):
        assert lib.pcg_abi_struct_bytes(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0, name
    assert lib.pcg_abi_version() == 7
    for name in ("pcg_patch_mask_bits", "pcg_mnist_cf_entry", "pcg_mnist_cf_tail", "pcg_mnist_cf_score"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The entry points' own checks return PCG_ERR_INVALID with a pcg_last_error text before a launch: no GPU is needed."""
    lib = pcgan_amd.load()
    p = ctypes.c_void_p(64)        # never dereferenced: every call below is refused on its scalars
    cases = [
        (lib.pcg_patch_mask_bits, _lib.PatchMaskBitsArgs(p, p, 1, 28, 28, 3), "exceed the 64 bits"),
        (lib.pcg_patch_mask_bits, _lib.PatchMaskBitsArgs(p, p, 1, 28, 28, 29), "no patch"),
        (lib.pcg_mnist_cf_entry, _lib.MnistCfEntryArgs(p, p, p, None, p, 3, 10, 784, 10, 0, 25, 6), "window"),
        (lib.pcg_mnist_cf_entry, _lib.MnistCfEntryArgs(p, p, p, p, p, 3, 10, 784, 10, 0, 0, 3), "T = 1"),
        (lib.pcg_mnist_cf_entry, _lib.MnistCfEntryArgs(p, p, p, None, p, 3, 10, 784, 10, 3, 0, 3), "mask mode"),
        (lib.pcg_mnist_cf_tail, _lib.MnistCfTailArgs(p, p, p, p, None, None, p, 0.1, 3, 10, 783, 0, 0, 3), "multiple of 4"),
        (lib.pcg_mnist_cf_tail, _lib.MnistCfTailArgs(p, ctypes.c_void_p(68), p, p, None, None, p, 0.1, 3, 10, 784, 0, 0, 3), "16-byte"),
        (lib.pcg_mnist_cf_score, _lib.MnistCfScoreArgs(p, None, None, None, None, p, None, None, None, None, None, None, 3, 10, 17, 20, 2, 0, 30), "K 17"),
        (lib.pcg_mnist_cf_score, _lib.MnistCfScoreArgs(p, p, None, None, None, p, None, None, None, None, None, None, 3, 10, 10, 12, 2, 0, 30), "y_true"),
        (lib.pcg_mnist_cf_score, _lib.MnistCfScoreArgs(p, None, None, None, None, None, None, None, None, None, None, None, 3, 10, 10, 12, 2, 0, 30), "no output"),
    ]
    for fn, args, text in cases:
        assert fn(ctypes.byref(args), None) != 0, text
        assert text in lib.pcg_last_error().decode(), (text, lib.pcg_last_error().decode())
    assert lib.pcg_mnist_cf_tail(None, None) != 0


# ---- the BatchNorm fold and its cache --------------------------------------------------------------------------------------------------
def _gen():
    torch.manual_seed(0)
    G = K.ResidualGenerator(base_ch=8, n_resblocks=2)
    with torch.no_grad():
        for blk in G.resblocks:
            blk.bn1.running_mean.normal_(); blk.bn1.running_var.uniform_(0.5, 2.0)
            blk.bn1.weight.normal_(); blk.bn1.bias.normal_(); blk.conv1.bias.normal_()
    return G.eval()


def test_fold_is_the_float64_affine_rounded_once():
    G = _gen()
    for blk, (w, b) in zip(G.resblocks, G.folded_conv1()):
        bn, conv = blk.bn1, blk.conv1
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (8, 3, 3, 8)          # OHWI
        assert torch.equal(w.permute(0, 3, 1, 2), (conv.weight.double() * s.view(-1, 1, 1, 1)).float())
        assert torch.equal(b, ((conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()).float())
        # and it IS the eval-mode conv1 -> bn1 of the block
        x = torch.randn(2, 8, 5, 5, dtype=torch.float64)
        want = bn.double()(conv.double()(x))
        got = torch.nn.functional.conv2d(x, w.permute(0, 3, 1, 2).double(), b.double(), padding=1)
        bn.float(); conv.float()
        np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-6)


def test_fold_cache_is_kept_and_dropped():
    G = _gen()
    f = G.folded_conv1()
    assert G.folded_conv1() is f                                            # cached
    G.train()
    assert G._fold_cache is None
    with pytest.raises(PcgError, match="eval"):
        G.folded_conv1()                                                    # training-mode BatchNorm has nothing to fold
    G.eval()
    f2 = G.folded_conv1()
    assert f2 is not f and torch.equal(f2[0][0], f[0][0])
    G.load_state_dict(G.state_dict())
    assert G._fold_cache is None
    f3 = G.folded_conv1()
    G.to(torch.float32)                                                     # .to(): storages may move
    assert G._fold_cache is None
    f4 = G.folded_conv1()
    with torch.no_grad():
        G.resblocks[1].bn1.running_var.mul_(4.0)                            # a buffer's version changes
    f5 = G.folded_conv1()
    assert f5 is not f4 and torch.equal(f5[0][0], f4[0][0]) and not torch.equal(f5[1][0], f4[1][0])
    with torch.no_grad():
        G.resblocks[0].conv1.weight.add_(1.0)                               # a parameter's version changes
    assert not torch.equal(G.folded_conv1()[0][0], f5[0][0])
    assert f3 is not None


def test_forward_queries_refuses_training_mode_and_cpu_tensors():
    G = _gen()
    x, m = torch.zeros(2, 1, 28, 28), torch.ones(784)
    with pytest.raises(PcgError, match="no CPU path"):
        G.forward_queries(x, None, m, "shared")
    G.train()
    with pytest.raises(PcgError, match="eval"):
        G.forward_queries(x, None, m, "shared")


def test_prompt_guards_need_no_gpu():
    G, C = _gen(), K.CNNClassifier().eval()
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(PcgError, match="GPU"):
        K.counterfactuals(G, C, x, 3, patches=[1, 5])
    with pytest.raises(PcgError, match="GPU"):
        K.counterfactual_sweep(G, C, x)
    with pytest.raises(PcgError, match="no patch"):
        K.build_patch_mask_for_batch(x, patch_size=29, device="cuda")
    with pytest.raises(PcgError, match="no CPU path"):
        K.make_mask_from_patch_list(x, 7, [1, 5])
