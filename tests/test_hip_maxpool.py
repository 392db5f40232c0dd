"""GPU: pcg_relu_maxpool2_fwd / _bwd (csrc/maxpool.hip through pcgan_amd.ops) bit for bit against torch on the CPU.

Pooling selects and copies; nothing is rounded.  So the tolerance is zero: p, idx and dz are compared with assert_array_equal against
max_pool2d(relu(z), 2, return_indices=True), its flat indices turned into 0..3 = dh * 2 + dw, and against its autograd backward.
Values lie on a 1/4 grid in [-2, 2], so ties and windows without a positive cell are common (asserted).  Every case runs eagerly and
inside a captured and replayed HIP graph; p, idx and dz are pre-filled with sentinels, which shows that every element is written."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_clf_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
SHAPES = [(1, 2, 2, 4),      # one window per channel quad
          (2, 4, 4, 4),      # smallest multi-window case
          (3, 7, 7, 8),      # odd size: the left-over row and column must come back 0
          (5, 6, 10, 12),    # non-square, C not a power of two
          (2, 28, 28, 32),   # the net's first pooling layer
          (2, 14, 14, 64)]   # the net's second pooling layer


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    return pcgan_amd.ops


def _grid(shape, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-8, 9, shape, generator=g).float() / 4.0                  # NHWC, on a 1/4 grid in [-2, 2]
    B, H, W, C = shape
    dp = torch.randint(-8, 9, (B, H // 2, W // 2, C), generator=g).float() / 4.0
    dp[dp == 0] = 0.25                                                          # a written gradient is never mistaken for a zero
    return z, dp


def _torch_reference(z, dp):
    """(p, idx, dz), NHWC numpy, from torch's own max_pool2d(relu(z)) and its autograd backward on the CPU."""
    zc = R.nchw(z).requires_grad_(True)
    p, flat = F.max_pool2d(torch.relu(zc), 2, return_indices=True)
    p.backward(R.nchw(dp))
    W = z.shape[2]
    idx = ((flat // W) % 2) * 2 + (flat % W) % 2
    return R.nhwc(p.detach()).numpy(), R.nhwc(idx).numpy().astype(np.uint8), R.nhwc(zc.grad).numpy()


def _run(ops, z, dp, graphed):
    """(p, idx, dz) of the two kernels as numpy, eagerly or from one replay of a captured graph; outputs start as sentinels."""
    from pcgan_amd import nn as N
    B, H, W, C = z.shape
    zd, dpd = z.to(DEV), dp.to(DEV)
    p = torch.full((B, H // 2, W // 2, C), SENTINEL, device=DEV)
    idx = torch.full((B, H // 2, W // 2, C), 255, dtype=torch.uint8, device=DEV)
    dz = torch.full((B, H, W, C), SENTINEL, device=DEV)

    def launches():
        ops.relu_maxpool2_fwd(zd, out=p, idx=idx)
        ops.relu_maxpool2_bwd(dpd, p, idx, (H, W), out=dz)

    if graphed:
        cap = N._HipGraphCapture(torch.device(DEV), tick=False)
        cap.warmup(launches, 1, None)
        p.fill_(SENTINEL); idx.fill_(255); dz.fill_(SENTINEL)
        torch.cuda.synchronize()
        cap.begin()
        try:
            launches()
        finally:
            graph = cap.end()
        torch.cuda.synchronize()
        assert float(dz[0, 0, 0, 0]) == SENTINEL                                  # captured, not run
        graph.replay()
    else:
        launches()
    torch.cuda.synchronize()
    return p.cpu().numpy(), idx.cpu().numpy(), dz.cpu().numpy()


def _compare(got, want, what):
    for name, g, w in zip(("p", "idx", "dz"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_is_torch_bit_for_bit(ops, shape, graphed):
    z, dp = _grid(shape, seed=sum(shape))
    want = _torch_reference(z, dp)
    win = R.windows(R.nchw(z))
    top = torch.sort(torch.relu(win), dim=-1).values
    ties, dead = int((top[..., 3] == top[..., 2]).sum()), int((win.max(-1).values <= 0).sum())
    if win[..., 0].numel() >= 64:                                               # (the 4-window case is too small to promise either)
        assert ties > 0 and dead > 0, (ties, dead)
    got = _run(ops, z, dp, graphed)
    _compare(got, want, str(shape))
    B, H, W, C = shape
    assert got[1].max() <= 3 and not (got[2] == SENTINEL).any()
    if H % 2:
        assert (got[2][:, H - 1] == 0).all()
    if W % 2:
        assert (got[2][:, :, W - 1] == 0).all()
    # exactly one cell per window can be non-zero, and it holds dp where the maximum is positive
    assert (np.count_nonzero(R.windows(R.nchw(torch.from_numpy(got[2]))).numpy(), axis=-1) <= 1).all()
    assert np.count_nonzero(got[2]) == np.count_nonzero(want[0] > 0)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_all_zero_and_tied_windows_keep_the_first_cell(ops, graphed):
    z = torch.zeros(1, 4, 4, 4)
    z[0, 0:2, 0:2, :] = -1.0                                                    # a dead patch: relu makes it an all-zero window
    z[0, 0:2, 2:4, :] = 1.5                                                     # a four-way tie above zero
    z[0, 2:4, 0:2, 0] = torch.tensor([[0.5, 2.0], [2.0, 2.0]])                  # a three-way tie: the first of them, cell 1
    z[0, 2, 2, :], z[0, 3, 3, :] = -0.0, 0.0
    dp = torch.full((1, 2, 2, 4), 3.0)
    got = _run(ops, z, dp, graphed)
    _compare(got, _torch_reference(z, dp), "ties")
    assert (got[1][0, 0, 0] == 0).all() and (got[1][0, 0, 1] == 0).all() and got[1][0, 1, 0, 0] == 1
    assert (got[2][0, 0:2, 0:2] == 0).all()                                     # the dead patch passes no gradient
    assert (got[2][0, 0, 2] == 3.0).all() and np.count_nonzero(got[2][0, 0:2, 2:4]) == 4


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_nan_and_inf_survive(ops, graphed):
    shape = (2, 4, 4, 4)
    z, dp = _grid(shape, seed=3)
    z[0, 1, 0, 2] = float("nan")                                                # cell 2 of window (0, 0), channel 2
    z[1, 2, 3, 1] = float("inf")                                                # cell 1 of window (1, 1), channel 1
    want = _torch_reference(z, dp)
    got = _run(ops, z, dp, graphed)
    _compare(got, want, "nan / inf")
    assert np.isnan(got[0][0, 0, 0, 2]) and got[1][0, 0, 0, 2] == 2 and np.isnan(got[0]).sum() == 1
    assert got[0][1, 1, 1, 1] == np.inf and got[1][1, 1, 1, 1] == 1
    assert got[2][0, 1, 0, 2] == dp[0, 0, 0, 2] and got[2][1, 2, 3, 1] == dp[1, 1, 1, 1]
    assert np.isfinite(got[2]).all()


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_input_already_through_relu_gives_the_identical_result(ops, graphed):
    z, dp = _grid((3, 7, 7, 8), seed=5)
    raw = _run(ops, z, dp, graphed)
    _compare(_run(ops, torch.relu(z), dp, graphed), raw, "relu(z) against z")
    _compare(raw, _torch_reference(z, dp), "z")


def test_grid_stride_loop_walks_more_than_once(ops):
    """More work items than the grid's cap of 8192 blocks of 256 threads covers in one pass: 16 * 32 * 33 * 128 = 2 162 688 items
    against 2 097 152 threads, so some threads take a second trip through the loop."""
    shape = (16, 64, 66, 512)
    assert shape[0] * (shape[1] // 2) * (shape[2] // 2) * (shape[3] // 4) > 8192 * 256
    z, dp = _grid(shape, seed=9)
    _compare(_run(ops, z, dp, False), _torch_reference(z, dp), str(shape))


def test_bad_channel_count_is_refused_not_launched(ops):
    import pcgan_amd
    z = torch.zeros(2, 4, 4, 6, device=DEV)
    with pytest.raises(pcgan_amd.PcgError, match="multiple of 4"):
        ops.relu_maxpool2_fwd(z)
    with pytest.raises(pcgan_amd.PcgError, match="multiple of 4"):
        ops.relu_maxpool2_bwd(torch.zeros(2, 2, 2, 6, device=DEV), torch.zeros(2, 2, 2, 6, device=DEV),
                              torch.zeros(2, 2, 2, 6, dtype=torch.uint8, device=DEV), (4, 4))
    # the library's own PCG_REQUIRE, past the Python checks: an error code and a message, the buffers untouched
    lib = pcgan_amd.load()
    p = torch.full((2, 2, 2, 6), SENTINEL, device=DEV)
    idx = torch.full((2, 2, 2, 6), 255, dtype=torch.uint8, device=DEV)
    dz = torch.full((2, 4, 4, 6), SENTINEL, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.pcg_relu_maxpool2_fwd(vp(z), vp(p), vp(idx), 2, 4, 4, 6, None) != 0
    assert b"multiple of 4" in lib.pcg_last_error()
    assert lib.pcg_relu_maxpool2_bwd(vp(p), vp(p), vp(idx), vp(dz), 2, 4, 4, 6, None) != 0
    assert b"multiple of 4" in lib.pcg_last_error()
    torch.cuda.synchronize()
    assert (p == SENTINEL).all() and (idx == 255).all() and (dz == SENTINEL).all()
