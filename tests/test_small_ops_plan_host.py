"""CPU: (1) every case table of tests/test_hip_small_ops.py reaches the route it names, through pcg_launch_plan_describe alone -- host
logic, no device; (2) the float64 references of those GPU tests (tests/small_ops_ref.py), whose backwards are written out by hand,
agree with torch.float64 autograd, so a wrong reference fails here and not on the GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ops_ref as R  # noqa: E402
import test_hip_small_ops as T  # noqa: E402


def test_small_op_cases_reach_their_routes():
    """The case tables of test_hip_small_ops.py against the describe entry, and every route the tables are meant to cover is reached
    by at least one case (GEMM: skinny with and without a second column, rowdot<1..4>, the tile; both forms of the reductions, of the
    cross-entropy block and rows, of the embedding gradient; the second pass of each element-wise grid)."""
    T.check_all_routes()


def test_launch_plan_describe_refuses_what_it_does_not_know():
    import pcgan_amd
    from pcgan_amd import _lib, ops
    for args in ((77, 1), (_lib.PLAN_ELEMENTWISE, 9, 100), (_lib.PLAN_GEMM_ACT, 0, 1, 512, 17), (_lib.PLAN_MEAN, 0),
                 (_lib.PLAN_EMBED_CONCAT_BWD, 64, 0, 0), (_lib.PLAN_BN_COLREDUCE, 0, 8, 1), (_lib.PLAN_BN_APPLY, 3, 5, 8, 1),
                 (_lib.PLAN_BN_FINALIZE, 0), (_lib.PLAN_INSTNORM, 0, 2, 0, 4, 1), (_lib.PLAN_SPECTRAL_NORM, 0, 257, 8), (_lib.PLAN_ADAM, 0, 1, 1), (_lib.PLAN_ADAM, 8, 1)):
        with pytest.raises(pcgan_amd.PcgError, match="pcg_launch_plan_describe"):
            ops.launch_plan(*args)
    # pcg_gemm has no skinny launch: the shape pcg_gemm_act sends there stays on the tile
    assert ops.launch_plan(_lib.PLAN_GEMM_ACT, 0, 1, 512, 17, 38).startswith("skinny")
    assert ops.launch_plan(_lib.PLAN_GEMM, 0, 1, 512, 17, 38) == "64x64 tiles: 1 x 8"


def _f64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_cross_entropy_matches_autograd(weighted):
    B, K = 37, 5
    z = _f64(B, K, seed=1) * 3
    t = torch.arange(B) % (K - 1)
    w = torch.tensor([0.4, 0.0, 1.7, 0.9, 2.3], dtype=torch.float64) if weighted else None
    zr = z.clone().requires_grad_(True)
    loss = F.cross_entropy(zr, t, weight=w)
    (1.9 * 0.7 * loss).backward()
    ref_loss, ref_dz = R.cross_entropy(z, t, w, 1.9, 0.7)
    torch.testing.assert_close(ref_loss, loss.detach(), rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref_dz, zr.grad, rtol=1e-12, atol=1e-15)
    if weighted:
        assert bool((ref_dz[t == 1] == 0).all())


def test_reference_embedding_gradient_matches_autograd():
    B, HW, K, C = 29, 11, 6, 3
    idx = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(2))
    x, mask, cot = _f64(B, HW, seed=3), _f64(B, HW, seed=4), _f64(B, HW, C, seed=5)
    table = _f64(K, HW, seed=6).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    out = R.embed_concat_fwd(xr, idx, table, mask)
    assert out.shape == (B, HW, C)
    out.backward(cot)
    base = _f64(K, HW, seed=7)
    dt, mag = R.embed_table_grad(cot, idx, K, 1)
    torch.testing.assert_close(dt, table.grad, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(R.embed_table_grad(cot, idx, K, 1, base)[0], table.grad + base, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(cot[..., 0], xr.grad, rtol=0, atol=0)                  # dx is channel 0 of the cotangent
    assert bool((mag >= dt.abs() - 1e-12).all())
    dt2, _ = R.embed_table_grad(cot, idx, K, 2)                                        # another channel: the mask's slot
    torch.testing.assert_close(dt2, torch.zeros(K, HW, dtype=torch.float64).index_add_(0, idx, cot[..., 2]), rtol=0, atol=0)


@pytest.mark.parametrize("form", ["plain", "mask", "one_minus"])
def test_reference_abs_mean_matches_autograd(form):
    n = 501
    a = _f64(n, seed=8).requires_grad_(True)
    m = None if form == "plain" else torch.rand(n, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    w = torch.ones(n, dtype=torch.float64) if m is None else (1 - m if form == "one_minus" else m)
    val = (a * w).abs().mean()
    (0.7 * 1.3 * val).backward()
    ref, mag = R.abs_mean(a.detach(), m, form == "one_minus")
    torch.testing.assert_close(ref, val.detach(), rtol=1e-14, atol=0)
    torch.testing.assert_close(mag / n, ref, rtol=1e-14, atol=0)
    torch.testing.assert_close(R.abs_mean_bwd(a.detach(), m, form == "one_minus", 0.7, 1.3), a.grad, rtol=1e-13, atol=1e-18)


def test_reference_average_pooling_matches_autograd():
    B, HW, C = 3, 49, 20
    x = _f64(B, HW, C, seed=10).requires_grad_(True)
    cot = _f64(B, C, seed=11)
    y = F.adaptive_avg_pool2d(x.permute(0, 2, 1).reshape(B, C, 7, 7), 1).reshape(B, C)     # NHWC [B][HW][C] as torch's NCHW
    y.backward(cot)
    torch.testing.assert_close(R.avgpool_fwd(x.detach()), y.detach(), rtol=1e-14, atol=1e-16)
    torch.testing.assert_close(R.avgpool_bwd(cot, HW), x.grad, rtol=1e-14, atol=1e-18)


def test_reference_gemm_and_weight_gradient_match_autograd():
    M, N, K = 9, 5, 7
    A, Bm, bias, C0 = (_f64(M, K, seed=12).requires_grad_(True), _f64(N, K, seed=13).requires_grad_(True), _f64(N, seed=14).requires_grad_(True),
                       _f64(M, N, seed=15))
    out = F.leaky_relu(F.linear(A, Bm, bias) + C0, 0.2)
    ref, mag = R.gemm(A.detach(), Bm.detach(), False, True, bias.detach(), C0, 0.2)
    torch.testing.assert_close(ref, out.detach(), rtol=1e-14, atol=1e-15)
    assert bool((mag >= (F.linear(A, Bm, bias) + C0).abs().detach() - 1e-12).all())
    torch.testing.assert_close(R.gemm(A.detach().T.contiguous(), Bm.detach().T.contiguous(), True, False)[0], (A @ Bm.T).detach(), rtol=1e-14, atol=1e-15)
    lin = F.linear(A, Bm, bias)                                  # the weight gradient of a Linear layer: dW = dy^T x, db = colsum(dy)
    cot = _f64(M, N, seed=16)
    lin.backward(cot)
    dW, db, mW, mb = R.linear_wgrad(cot, A.detach())
    torch.testing.assert_close(dW, Bm.grad, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(db, bias.grad, rtol=1e-13, atol=1e-14)
    assert bool((mW >= dW.abs() - 1e-12).all()) and bool((mb >= db.abs() - 1e-12).all())


def test_cf_metric_rows_and_inputs():
    """cf_metric_rows against the softmax definition; cf_inputs keeps its promise (exact ties, margins, targets on both tied indices)."""
    lcf, lref, t, other = T.cf_inputs(257, 4, 5)
    hit, rows = R.cf_metric_rows(lcf, t, lref)
    rng = torch.arange(257)
    torch.testing.assert_close(rows, torch.softmax(lcf, 1)[rng, t] - torch.softmax(lref, 1)[rng, t], rtol=0, atol=0)
    _, rows_o = R.cf_metric_rows(lcf, t, None, other)
    torch.testing.assert_close(rows_o, torch.softmax(lcf, 1)[rng, t] - torch.softmax(lcf, 1)[rng, other], rtol=0, atol=0)
    ties = [b for b in range(257) if b % 7 == 3]
    first = torch.tensor([int((lcf[b] == lcf[b].max()).nonzero()[0]) for b in ties])
    assert all(int((lcf[b] == lcf[b].max()).sum()) == 2 for b in ties)
    assert torch.equal(hit[ties], t[ties] == first) and 0 < int(hit[ties].sum()) < len(ties)      # the first tied index wins
    gain, bound, dist = T.cf_gain_bound(lcf, lref, t, None)
    assert 0 < dist < 1e-7 and 4 * dist < bound < 1e-6 and abs(gain) < 1
