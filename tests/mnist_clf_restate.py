"""Restatement of the launches around the convolutions of the MNIST classifier's training step (conditional_counteRGAN/mnist/
models/classifier.py:7-22 in training mode, trainer.py:16-20) with the backward written out by hand: the reference of
tests/test_hip_mnist_clf_fit.py for pcg_drop2d_flatten_fwd / _bwd, pcg_mnist_clf_head and pcg_mnist_clf_batch.  Plain torch / NumPy on
the CPU, in whatever dtype its inputs have: float64 is the truth, float32 the yardstick of what fp32 arithmetic in another order
gives.  tests/test_mnist_clf_fit_host.py pins it to the oracle's autograd step."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import rng_np

P2D, P1 = 0.25, 0.5
WIDTHS, KEEPS = (128, 256), (1.0 - P2D, 1.0 - P1)
CONVS = ((0, 1), (2, 2), (4, 2))                              # (index in classifier.conv, stride); 3x3, padding 1


def drop2d_flatten_fwd(a, mask, p):
    """a [R, HW, C] (NHWC), mask [R, C] -> [R, C * HW]: Dropout2d then nn.Flatten of the NCHW tensor."""
    R, HW, C = a.shape
    return (a * (mask.to(a.dtype) / (1.0 - p))[:, None, :]).permute(0, 2, 1).reshape(R, C * HW)


def drop2d_flatten_bwd(dflat, mask, p, y):
    """dflat [R, C * HW], y [R, HW, C] the saved ReLU output -> [R, HW, C]: Flatten', Dropout2d', ReLU'."""
    R, HW, C = y.shape
    d = dflat.reshape(R, C, HW).permute(0, 2, 1) * (mask.to(dflat.dtype) / (1.0 - p))[:, None, :]
    return d * (y > 0).to(d.dtype)


def head(h, m1, p, W2, b2, y):
    """Dropout(p), Linear(W2, b2), mean cross-entropy and their backward down to fc1's pre-activation.  h [R, I] is fc1's post-ReLU
    output.  Returns a dict: logits, loss, hits (rows whose FIRST maximum is the label), dW2, db2, dh, db1."""
    R = h.shape[0]
    hd = h * (m1.to(h.dtype) / (1.0 - p))
    logits = hd @ W2.T + b2
    lse = torch.logsumexp(logits, 1)
    loss = (lse - logits.gather(1, y[:, None])[:, 0]).sum() / R
    onehot = torch.zeros_like(logits).scatter_(1, y[:, None], 1.0)
    dl = (torch.exp(logits - lse[:, None]) - onehot) / R
    dh = (dl @ W2) * (m1.to(h.dtype) / (1.0 - p)) * (h > 0).to(h.dtype)
    return dict(logits=logits, loss=loss, hits=int((logits.argmax(1) == y).sum()), dW2=dl.T @ hd, db2=dl.sum(0), dh=dh, db1=dh.sum(0))


def train_grads(sd, x, y, masks):
    """Loss and every parameter gradient of one step from state_dict `sd` (keys of CNNClassifier: conv.0.weight, ..., fc.4.bias),
    Dropout masks (m2d [R, 128], m1 [R, 256]) supplied.  x [R, 1, 28, 28].  Returns (loss, {name: grad})."""
    m2d, m1 = masks
    acts = [x]
    for i, s in CONVS:
        acts.append(torch.relu(F.conv2d(acts[-1], sd[f"conv.{i}.weight"], sd[f"conv.{i}.bias"], stride=s, padding=1)))
    R, C, H, W = acts[-1].shape
    a3 = acts[-1].permute(0, 2, 3, 1).reshape(R, H * W, C)                       # the NHWC activation the kernels hold
    flat = drop2d_flatten_fwd(a3, m2d, P2D)
    h = torch.relu(flat @ sd["fc.1.weight"].T + sd["fc.1.bias"])
    o = head(h, m1, P1, sd["fc.4.weight"], sd["fc.4.bias"], y)
    grads = {"fc.4.weight": o["dW2"], "fc.4.bias": o["db2"], "fc.1.weight": o["dh"].T @ flat, "fc.1.bias": o["db1"]}
    d = drop2d_flatten_bwd(o["dh"] @ sd["fc.1.weight"], m2d, P2D, a3)
    d = d.reshape(R, H, W, C).permute(0, 3, 1, 2)                                  # back to NCHW; ReLU' of conv3 is applied
    for li in (2, 1, 0):
        i, s = CONVS[li]
        below, w = acts[li], sd[f"conv.{i}.weight"]
        grads[f"conv.{i}.weight"] = torch.nn.grad.conv2d_weight(below, w.shape, d, stride=s, padding=1)
        grads[f"conv.{i}.bias"] = d.sum((0, 2, 3))
        if li > 0:
            d = torch.nn.grad.conv2d_input(below.shape, w, d, stride=s, padding=1) * (below > 0).to(d.dtype)
    return float(o["loss"]), grads


def batch_span(B, widths=WIDTHS):
    """Counter values one pcg_mnist_clf_batch call consumes: (n + 3) / 4 per mask."""
    return sum((B * w + 3) // 4 for w in widths)


def batch_host(X, Y, perm, cursor, B, seed, offset, widths=WIDTHS, keeps=KEEPS):
    """pcg_mnist_clf_batch on the host: rows perm[cursor .. cursor + B) and the two masks, the values of two bernoulli draws at
    consecutive offsets.  -> (x [B, D], y [B], [m0 [B, w0], m1 [B, w1]], offset after the call)."""
    x, y, _ = rng_np.gather_batch(np.asarray(X), np.asarray(Y), perm, cursor, B)
    ms = []
    for w, k in zip(widths, keeps):
        m, (lo, hi) = rng_np.bernoulli(B * w, k, seed, offset)
        assert lo == offset
        ms.append(m.reshape(B, w))
        offset = hi
    return x, y, ms, offset
