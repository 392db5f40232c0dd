"""CPU: the references the GPU tests of the MNIST classifier fit (tests/test_hip_mnist_clf_fit.py) are measured against, and the
host side of the feature.
(1) tests/mnist_clf_restate.py -- the head and the two flatten entries with a hand-written backward, composed into one step --
against the oracle's autograd step (oracle/countergan_ref.classifier_train_step) on the reference's recorded batches and Dropout
draws, in float64; (2) the batch entry's host model and its span arithmetic; (3) ClassifierFit.unsupported's reasons; (4) the ABI
additions and the entry points' refusals (every call below is refused before anything is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnist_clf_restate as RS  # noqa: E402
from oracle import countergan_ref as CR  # noqa: E402
from oracle import rng_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pcg_mnist_clf_batch", "pcg_mnist_clf_batch_counter", "pcg_drop2d_flatten_fwd", "pcg_drop2d_flatten_bwd", "pcg_mnist_clf_head")
FAKE = 0x10000                                # a non-null, 16-byte aligned address: never dereferenced


def test_restatement_is_the_oracle_step(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "classifier_pretrain_mnist.npz")))
    torch.manual_seed(5)
    clf = CR.CNNClassifier().double()
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3)
    for i in range(2):
        x, y = torch.from_numpy(gold[f"x{i}"]).double(), torch.from_numpy(gold[f"y{i}"])
        masks = (torch.from_numpy(gold[f"mask{2 * i}"]), torch.from_numpy(gold[f"mask{2 * i + 1}"]))
        assert x.shape[0] == 8
        sd = {k: v.clone() for k, v in clf.state_dict().items()}
        loss, grads = RS.train_grads(sd, x, y, masks)
        ref = CR.classifier_train_step(clf, opt, x, y, masks)                    # leaves p.grad of this step, then moves the parameters
        assert abs(loss - ref) <= 1e-12 * max(1.0, abs(ref)), (i, loss, ref)
        assert set(grads) == {n for n, _ in clf.named_parameters()} and len(grads) == 10
        for n, p in clf.named_parameters():
            scale = float(p.grad.abs().max())
            assert scale > 0 and float((grads[n] - p.grad).abs().max()) <= 1e-12 * scale, (i, n)


def test_flatten_restatements_are_the_chain_and_each_others_adjoint():
    rs = np.random.RandomState(2)
    for R, HW, C in ((1, 49, 128), (5, 5, 12)):
        a = torch.from_numpy(rs.normal(0, 1, (R, HW, C)))
        y = torch.relu(torch.from_numpy(rs.normal(0, 1, (R, HW, C))))
        m = torch.from_numpy((rs.random_sample((R, C)) < 0.75).astype(np.float32))
        g = torch.from_numpy(rs.normal(0, 1, (R, C * HW)))
        out = RS.drop2d_flatten_fwd(a, m, 0.25)
        nchw = a.permute(0, 2, 1).reshape(R, C, HW) * (m.double()[:, :, None] / 0.75)          # Dropout2d on the NCHW tensor, then Flatten
        assert torch.equal(out, nchw.reshape(R, C * HW))
        assert out[R - 1, 3 * HW + 2] == a[R - 1, 2, 3] * m[R - 1, 3].double() / 0.75
        ones = torch.ones_like(y)
        assert abs(float((out * g).sum() - (a * RS.drop2d_flatten_bwd(g, m, 0.25, ones)).sum())) <= 1e-10     # <A a, g> == <a, A^T g>
        assert torch.equal(RS.drop2d_flatten_bwd(g, m, 0.25, y), RS.drop2d_flatten_bwd(g, m, 0.25, ones) * (y > 0))


def test_head_restatement_is_autograd():
    rs = np.random.RandomState(3)
    for R, K in ((1, 3), (5, 10), (8, 16)):
        h = torch.relu(torch.from_numpy(rs.normal(0, 1, (R, 256)))).requires_grad_()
        m1 = torch.from_numpy((rs.random_sample((R, 256)) < 0.5).astype(np.float32))
        W2 = torch.from_numpy(rs.uniform(-1, 1, (K, 256)) / 16).requires_grad_()
        b2 = torch.from_numpy(rs.uniform(-0.1, 0.1, K)).requires_grad_()
        y = torch.from_numpy(rs.randint(0, K, R))
        loss = torch.nn.functional.cross_entropy((h * m1.double() / 0.5) @ W2.T + b2, y)
        loss.backward()
        o = RS.head(h.detach(), m1, 0.5, W2.detach(), b2.detach(), y)
        assert abs(float(o["loss"] - loss.detach())) <= 1e-14
        pre = (h.detach() > 0).double()                                            # dh continues through fc1's ReLU
        for got, want in ((o["dW2"], W2.grad), (o["db2"], b2.grad), (o["dh"], h.grad * pre), (o["db1"], (h.grad * pre).sum(0))):
            assert float((got - want).abs().max()) <= 1e-14
    # a tie counts for the lower index
    o = RS.head(torch.ones(2, 256, dtype=torch.float64), torch.ones(2, 256), 0.5, torch.ones(3, 256, dtype=torch.float64) / 256,
                torch.zeros(3, dtype=torch.float64), torch.tensor([0, 1]))
    assert o["hits"] == 1


def test_batch_host_model_and_span_arithmetic():
    from pcgan_amd import ops
    assert RS.batch_span(1) == 32 + 64 and RS.batch_span(5) == 160 + 320 and RS.batch_span(128) == 4096 + 8192
    assert RS.batch_span(3, (5, 3)) == 4 + 3                                     # (15 + 3) / 4 and (9 + 3) / 4: each span rounds up alone
    for B, widths in ((1, RS.WIDTHS), (44, RS.WIDTHS), (3, (5, 3))):
        assert ops.DeviceRNG.mnist_clf_batch_span(B, widths) == RS.batch_span(B, widths)
    rs = np.random.RandomState(4)
    N, D, B, seed, off = 23, 6, 5, 21, 7
    X, Y, perm = rs.random_sample((N, D)).astype(np.float32), rs.randint(0, 10, N), rs.permutation(N)
    x, y, ms, end = RS.batch_host(X, Y, perm, 10, B, seed, off, widths=(5, 3), keeps=(0.75, 0.5))
    assert np.array_equal(x, X[perm[10:15]]) and np.array_equal(y, Y[perm[10:15]])
    assert end == off + 7 + 4                                                # (25 + 3) / 4 and (15 + 3) / 4
    assert np.array_equal(ms[0].ravel(), rng_np.bernoulli(25, 0.75, seed, off)[0])
    assert np.array_equal(ms[1].ravel(), rng_np.bernoulli(15, 0.5, seed, off + 7)[0])   # the second mask starts a whole quad later
    big = RS.batch_host(X, Y, perm, 0, 20, seed, off)[2]
    assert big[0].shape == (20, 128) and big[1].shape == (20, 256) and 0.6 < big[0].mean() < 0.9 and 0.4 < big[1].mean() < 0.6


def test_unsupported_reasons():
    import torch.nn as nn
    from pcgan_amd import countergan as K
    U = K.ClassifierFit.unsupported
    assert U(K.CNNClassifier(), 128) is None and U(K.CNNClassifier(num_classes=16), 1) is None
    assert "classes" in U(K.CNNClassifier(num_classes=17), 128)
    assert "batch size 160" in U(K.CNNClassifier(), 160)
    c = K.CNNClassifier()
    c.conv_precision = "bf16"
    assert "bf16" in U(c, 128)
    c = K.CNNClassifier()
    c.fc[1], c.fc[4] = nn.Linear(6272, 128), nn.Linear(128, 10)
    assert "linear layers" in U(c, 128)
    c = K.CNNClassifier()
    c.conv[2] = nn.Conv2d(32, 64, 3, 1, 1)
    assert "convolutions" in U(c, 128)
    c = K.CNNClassifier()
    c.conv[0] = nn.Conv2d(1, 32, 5, 1, 2)
    assert "convolutions" in U(c, 128)
    with pytest.raises(K.PcgError, match="ClassifierFit: batch size 160"):
        K.ClassifierFit(K.CNNClassifier(), np.zeros((4, 1, 28, 28), np.float32), np.zeros(4, np.int64), 160)


def test_new_symbols_declared_exported_and_refusing():
    from pcgan_amd import _lib
    with open(os.path.join(ROOT, "include", "pcgan_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), f"{name} is not exported by the built library"
        assert name + "(" in header, f"{name} is not declared in include/pcgan_hip.h"
    assert "conditional_counteRGAN/mnist/trainer.py:8-39" in header and "classifier.py:19-21" in header
    lib = _lib.load()
    assert lib.pcg_abi_version() == 7, "the additions are additive"
    p = ctypes.c_void_p(FAKE)
    head = lambda R, I, K: lib.pcg_mnist_clf_head(p, p, 2.0, p, p, p, R, I, K, p, p, p, p, p, p, p, None)      # noqa: E731
    for R, I, K, why in ((129, 256, 10, b"129 rows"), (0, 256, 10, b"0 rows"), (128, 512, 10, b"512 inputs"), (128, 256, 17, b"17 classes")):
        assert head(R, I, K) != 0 and why in lib.pcg_last_error(), (R, I, K, lib.pcg_last_error())
    batch = lambda n_perm, cursor, B: lib.pcg_mnist_clf_batch(p, p, p, n_perm, 300, p, p, B, 784, p, 128, 0.75, p, 256, 0.5, 1, 0, cursor, None)  # noqa: E731
    assert batch(300, 257, 44) != 0 and b"permutation of 300" in lib.pcg_last_error()
    assert batch(300, -1, 44) != 0
    assert lib.pcg_mnist_clf_batch_counter(p, p, p, 300, 300, p, p, 44, 784, p, 128, 0.75, p, 256, 0.5, 1, None, None) != 0
    assert b"null counter" in lib.pcg_last_error()
    assert lib.pcg_drop2d_flatten_fwd(p, p, 1.0, 0, 49, 128, ctypes.c_void_p(FAKE + 64), None) != 0                # no rows
    assert lib.pcg_drop2d_flatten_fwd(p, p, 1.0, 4, 49, 128, p, None) != 0                                        # in place
    assert lib.pcg_drop2d_flatten_bwd(p, p, 1.0, None, 1, 0.0, 4, 49, 128, ctypes.c_void_p(FAKE + 64), None) != 0
