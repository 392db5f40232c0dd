"""CPU: the host side of the max-pool MNIST classifier -- the two pooling entry points are exported and declared,
tests/pool_clf_restate.py reproduces the reference's recorded results (tests/golden/mnist_pool_clf_ref.npz), countergan.Classifier
keeps the reference's state_dict in both directions, and the argument checks of ops.relu_maxpool2_* that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pool_clf_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcg_relu_maxpool2_fwd", "pcg_relu_maxpool2_bwd")


@pytest.fixture(scope="module", autouse=True)
def feature():
    """Every test of this file is about the max-pool classifier: none passes on a tree without it."""
    from pcgan_amd import countergan, ops
    return countergan.Classifier, ops.relu_maxpool2_fwd, ops.relu_maxpool2_bwd


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mnist_pool_clf_ref.npz")))


@pytest.fixture(scope="module")
def sd(ref):
    """The golden file's weights, rebuilt from its seed and checked against its per-tensor sums."""
    sd = R.seeded_state(int(ref["seed"]))
    sums = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    np.testing.assert_allclose(sums, ref["weight_sums"], rtol=1e-12, atol=1e-12,
                               err_msg="torch's default initialisation draws differ from the ones the golden file was made with")
    return sd


def _c_params(name):
    text = open(os.path.join(ROOT, "include", "pcgan_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_new_symbols_exported_and_declared_alike():
    import pcgan_amd
    from pcgan_amd import _lib
    raw = ctypes.CDLL(pcgan_amd.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"{name} is not exported by libpcgan_hip.so"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int
        params = _c_params(name)
        assert len(params) == len(argtypes), (name, params)
        for c_decl, ct in zip(params, argtypes):
            want = ctypes.c_void_p if ("*" in c_decl or "pcg_stream_t" in c_decl) else ctypes.c_int32
            assert ct is want, (name, c_decl, ct)
    assert [p.split()[-1] for p in _c_params(NEW[0])] == ["z", "p", "idx", "B", "H", "W", "C", "stream"]
    assert [p.split()[-1] for p in _c_params(NEW[1])] == ["dp", "p", "idx", "dz", "B", "H", "W", "C", "stream"]
    assert "maxpool.hip" in open(os.path.join(ROOT, "promptable-counterfactual-gan_amd", "csrc", "Makefile")).read()


def test_restatement_reproduces_the_reference(ref, sd):
    x, target = torch.from_numpy(ref["x"]), torch.from_numpy(ref["target"])
    f32 = R.forward(sd, x)
    f64 = R.forward(R.cast(sd, torch.float64), x.double())
    np.testing.assert_allclose(f32["logits"].numpy(), ref["logits32"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(f64["logits"].numpy(), ref["logits64"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(f64["logits"].argmax(1).numpy(), ref["pred"])
    np.testing.assert_allclose(R.input_grad(R.cast(sd, torch.float64), x.double(), target).reshape(16, 784).numpy(), ref["dx64"], rtol=0, atol=1e-12)
    for i in (1, 2):
        np.testing.assert_array_equal(f64[f"idx{i}"].numpy(), ref[f"idx{i}"])
        np.testing.assert_array_equal((f64[f"p{i}"] > 0).numpy(), ref[f"live{i}"])
        near = (f64[f"p{i}"] > 0) & (R.top2_gap(f64[f"z{i}"]) < float(ref[f"bound{i}"]))
        np.testing.assert_array_equal(near.numpy(), ref[f"near{i}"])
        assert ref[f"near{i}"].sum() <= 0.002 * ref[f"live{i}"].sum()
    assert ref["undecided"].sum() <= 1


def test_pinned_forward_with_its_own_routing_is_the_forward(sd):
    """With the routing and masks of the same float64 run, the pinned forward and its input gradient are the plain ones."""
    sd64 = R.cast(sd, torch.float64)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 1, 28, 28, generator=g, dtype=torch.float64)
    y = torch.tensor([1, 7, 3])
    f = R.forward(sd64, x)
    xp = x.clone().requires_grad_(True)
    logits = R.pinned_forward(sd64, xp, f["idx1"], f["p1"] > 0, f["idx2"], f["p2"] > 0, f["h"] > 0)
    np.testing.assert_allclose(logits.detach().numpy(), f["logits"].numpy(), rtol=0, atol=1e-13)
    torch.nn.functional.cross_entropy(logits, y, reduction="sum").backward()
    np.testing.assert_allclose(xp.grad.numpy(), R.input_grad(sd64, x, y).numpy(), rtol=0, atol=1e-13)


def test_state_dict_is_the_references_in_both_directions(ref, sd, tmp_path):
    from pcgan_amd import countergan as K
    assert tuple(ref["keys"]) == R.KEYS and tuple(ref["shapes"]) == tuple(str(s) for s in R.SHAPES)
    if len(ref["shipped_keys"]):                                       # the shipped models/classifier.pt, as the golden script read it
        assert tuple(ref["shipped_keys"]) == R.KEYS and tuple(ref["shipped_shapes"]) == tuple(ref["shapes"])
    net = K.Classifier()
    assert tuple(net.state_dict()) == R.KEYS
    assert tuple(tuple(v.shape) for v in net.state_dict().values()) == R.SHAPES
    net.load_state_dict(sd, strict=True)                               # a checkpoint of the reference's module
    torch_net = R.TorchClassifier()
    torch_net.load_state_dict({k: v.contiguous() for k, v in net.state_dict().items()}, strict=True)      # and back
    for k in R.KEYS:
        assert torch.equal(torch_net.state_dict()[k], sd[k]), k
    path = str(tmp_path / "classifier.pt")
    K.save_classifier(net, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(back) == R.KEYS and all(torch.equal(back[k], sd[k]) for k in R.KEYS)
    loaded = K.load_classifier(path, "cpu")
    assert not loaded.training and all(torch.equal(loaded.state_dict()[k], sd[k]) for k in R.KEYS)
    assert K.get_pool_classifier(path, device="cpu").state_dict()["net.9.bias"].equal(sd["net.9.bias"])     # the file exists: loaded
    with pytest.raises(K.PcgError, match="does not exist"):
        K.get_pool_classifier(str(tmp_path / "missing.pt"), device="cpu")
    torch.manual_seed(int(ref["seed"]))                                # the same draws as the reference's constructor
    assert all(torch.equal(v, sd[k]) for k, v in K.Classifier().state_dict().items())
    assert net._draw_dropout_masks(torch.zeros(2, 1, 28, 28)) == []


def test_argument_checks_that_need_no_device():
    import pcgan_amd
    ops, Err = pcgan_amd.ops, pcgan_amd.PcgError
    z = torch.zeros(2, 4, 4, 8)
    with pytest.raises(Err, match="multiple of 4"):
        ops.relu_maxpool2_fwd(torch.zeros(2, 4, 4, 6))
    with pytest.raises(Err, match="NHWC"):
        ops.relu_maxpool2_fwd(torch.zeros(4, 4, 8))
    with pytest.raises(Err, match="float32"):
        ops.relu_maxpool2_fwd(z.double())
    with pytest.raises(Err, match="contiguous"):
        ops.relu_maxpool2_fwd(torch.zeros(2, 4, 8, 4).permute(0, 1, 3, 2))
    with pytest.raises(Err, match="at least 2"):
        ops.relu_maxpool2_fwd(torch.zeros(2, 1, 4, 8))
    with pytest.raises(Err, match="GPU"):
        ops.relu_maxpool2_fwd(z)
    dp, p, idx = torch.zeros(2, 2, 2, 8), torch.zeros(2, 2, 2, 8), torch.zeros(2, 2, 2, 8, dtype=torch.uint8)
    with pytest.raises(Err, match="does not pool"):
        ops.relu_maxpool2_bwd(dp, p, idx, (6, 4))
    with pytest.raises(Err, match="multiple of 4"):
        ops.relu_maxpool2_bwd(torch.zeros(2, 2, 2, 6), p, idx, (4, 4))
    with pytest.raises(Err, match="p: expected shape"):
        ops.relu_maxpool2_bwd(dp, torch.zeros(2, 2, 3, 8), idx, (4, 4))
    with pytest.raises(Err, match="idx: expected torch.uint8"):
        ops.relu_maxpool2_bwd(dp, p, idx.to(torch.int32), (4, 4))
    with pytest.raises(Err, match="GPU"):
        ops.relu_maxpool2_bwd(dp, p, idx, (5, 5))                      # odd sizes pool to the same 2 x 2


def test_library_refuses_bad_channel_counts_without_a_launch():
    """PCG_REQUIRE in front of the launch: C = 6 comes back as an error (null-safe: the check precedes any use of the pointers)."""
    import pcgan_amd
    lib = pcgan_amd.load()
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    assert lib.pcg_relu_maxpool2_fwd(ptr, ptr, ptr, 1, 4, 4, 6, None) != 0
    assert b"multiple of 4" in lib.pcg_last_error()
    assert lib.pcg_relu_maxpool2_bwd(ptr, ptr, ptr, ptr, 1, 4, 4, 6, None) != 0
    assert b"multiple of 4" in lib.pcg_last_error()
    assert lib.pcg_relu_maxpool2_fwd(ptr, ptr, ptr, 1, 1, 4, 8, None) != 0
