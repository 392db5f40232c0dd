"""GPU: the five entries of csrc/delta_gan.hip through pcgan_amd.ops, each alone, eagerly and from a captured and
replayed HIP graph, with every output pre-filled with a sentinel.

Batches are B = 1, 3 and 4 (R = 2, 6, 8 rows for the head in mode D): the smallest at which the row halves, odd rows and the partial
last chunk / last 16-byte group can go wrong; the spatial sizes are the nets' own, 784 pixels and F = 12544.  Only the tail forward walks
its data under a capped grid, and its grid is a parameter: grid = 2 on the three chunks of B = 3 is the case beyond one trip.
Copies (entry, x_cf) are compared with zero tolerance; sums and products against a float64 evaluation by the project's rule of §3.18,
rtol 1e-4 and atol 2e-5 * max|reference|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
HW, F, K = 784, 12544, 10
MODES = pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    return pcgan_amd.ops


def _exec(launches, outs, graphed):
    """Run `launches` eagerly or as one replay of a captured graph; `outs` (tensors) are sentinel-filled first."""
    from pcgan_amd import nn as N
    fills = [(t, t.clone()) for t in outs]
    if graphed:
        cap = N._HipGraphCapture(torch.device(DEV), tick=False)
        cap.warmup(launches, 1, None)
        for t, t0 in fills:
            t.copy_(t0)
        torch.cuda.synchronize()
        cap.begin()
        try:
            launches()
        finally:
            graph = cap.end()
        torch.cuda.synchronize()
        assert all(torch.equal(t, t0) for t, t0 in fills), "captured, not run"
        graph.replay()
    else:
        launches()
    torch.cuda.synchronize()


def _close(got, want64, what):
    want64 = np.asarray(want64, np.float64)
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=2e-5 * float(np.abs(want64).max()), err_msg=what)


def _quarter_grid(shape, gen):
    return torch.randint(-8, 9, shape, generator=gen).float() / 4.0              # [-2, 2] on a 1/4 grid: exact zeros and negatives


# ---- entry -----------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("B", [1, 3, 4])
def test_entry_is_embed_concat_bit_for_bit_and_regather_touches_one_channel(ops, B, graphed):
    gen = torch.Generator().manual_seed(B)
    x = (2 * torch.rand(B, HW, generator=gen) - 1).to(DEV)
    y = torch.randint(0, K, (B,), generator=gen)
    t = torch.randint(0, K, (B,), generator=gen)
    if B == 3:
        y = torch.tensor([-3, 12, 4])                                            # device labels out of range: clamped as embed_concat_fwd clamps
    y, t = y.to(DEV), t.to(DEV)
    EG, ED, ED2 = (torch.randn(K, HW, generator=gen).to(DEV) for _ in range(3))
    w = torch.randn(F, generator=gen).to(DEV)
    g_in = torch.full((B, HW, 2), SENTINEL, device=DEV)
    d_in = torch.full((2 * B, HW, 2), SENTINEL, device=DEV)
    lab = torch.full((2 * B,), -7, dtype=torch.int64, device=DEV)
    wp = torch.full((F,), SENTINEL, device=DEV)
    _exec(lambda: ops.delta_gan_entry(x, y, t, EG, ED, g_in=g_in, d_in=d_in, labels_2b=lab, head_w=w, head_w_packed=wp, head_shape=(256, 49)),
          [g_in, d_in, lab, wp], graphed)
    assert torch.equal(g_in, ops.embed_concat_fwd(x, t, EG, None))
    assert torch.equal(d_in[:B], ops.embed_concat_fwd(x, y, ED, None))
    assert torch.equal(d_in[B:, :, 1], ops.embed_concat_fwd(x, t, ED, None)[:, :, 1])
    assert bool((d_in[B:, :, 0] == SENTINEL).all()), "channel 0 of rows B..2B belongs to the tail forward"
    assert torch.equal(lab, torch.cat([y, t]))
    assert torch.equal(wp, w.view(256, 49).t().contiguous().view(-1))
    # the regather after Adam(D): another table, another target; nothing but channel 1 of rows B..2B (and the packed weight) may change
    before_g, before_d, before_lab = g_in.clone(), d_in.clone(), lab.clone()
    t2 = ((t + 1) % K).contiguous()
    w2 = (w * 2).contiguous()
    _exec(lambda: ops.delta_gan_entry(None, None, t2, None, ED2, d_in=d_in, head_w=w2, head_w_packed=wp, head_shape=(256, 49), regather=True),
          [d_in, wp], graphed)
    assert torch.equal(g_in, before_g) and torch.equal(lab, before_lab)
    assert torch.equal(d_in[:B], before_d[:B]) and torch.equal(d_in[B:, :, 0], before_d[B:, :, 0])
    assert torch.equal(d_in[B:, :, 1], ED2[t2])
    assert torch.equal(wp, w2.view(256, 49).t().contiguous().view(-1))


def test_entry_refuses_host_visible_labels_out_of_range(ops):
    from pcgan_amd import PcgError
    x = torch.zeros(2, HW, device=DEV)
    E = torch.zeros(K, HW, device=DEV)
    y, t = torch.tensor([1, 10]), torch.tensor([5, 5])
    with pytest.raises(PcgError, match="label 10"):
        ops.delta_gan_entry(x, y.clamp(0, 9).to(DEV), t.to(DEV), E, E, y_host=y, target_host=t)


# ---- tail forward ------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("B", [1, 3, 4])
def test_tail_forward_copies_exactly_and_sums_in_one_order_for_every_grid(ops, B, graphed):
    gen = torch.Generator().manual_seed(10 + B)
    x = 2 * torch.rand(B, HW, generator=gen) - 1
    delta = _quarter_grid((B, HW), gen) * 0.125
    assert bool((delta == 0).any())
    want = x + delta                                                             # one fp32 add per element: nothing to tolerate
    xd, dd = x.to(DEV), delta.to(DEV)
    tail_ws, _ = ops.delta_gan_workspace(B, HW, torch.device(DEV))
    losses = []
    for grid in (0, 1, 2):                                                       # B = 3 holds 3 chunks: grid 2 takes a second trip, grid 1 three
        x_cf = torch.full((B, HW), SENTINEL, device=DEV)
        d_in = torch.full((2 * B, HW, 2), SENTINEL, device=DEV)
        loss = torch.full((1,), SENTINEL, device=DEV)
        _exec(lambda: ops.delta_gan_tail_fwd(xd, dd, d_in, x_cf=x_cf, loss_reg=loss, ws=tail_ws, grid=grid), [x_cf, d_in, loss], graphed)
        assert torch.equal(x_cf.cpu(), want) and torch.equal(d_in[B:, :, 0].cpu(), want)
        assert bool((d_in[:B] == SENTINEL).all()) and bool((d_in[B:, :, 1] == SENTINEL).all())
        assert not tail_ws[:16].any(), "the arrival counter is left zero"
        losses.append(float(loss.cpu()))
    _close(losses[0], float(delta.double().abs().mean()), "loss_reg")
    assert losses[0] == losses[1] == losses[2], f"loss_reg depends on the grid: {losses}"


# ---- tail backward -----------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_tail_backward_is_the_fp32_expression_in_its_order(ops, B, stride, graphed):
    gen = torch.Generator().manual_seed(20 + B)
    dD_full = torch.randn(B, HW, stride, generator=gen) * 1e-3
    dC = torch.randn(B, HW, generator=gen) * 1e-3
    delta = _quarter_grid((B, HW), gen) * 0.125
    assert bool((delta == 0).any()) and bool((delta < 0).any())
    lam_cls, lam_reg = 3.0, 0.05
    dD = dD_full[:, :, 0]
    c32 = torch.tensor(lam_reg / (B * HW), dtype=torch.float32)
    want32 = (dD + torch.tensor(lam_cls, dtype=torch.float32) * dC) + c32 * torch.sign(delta)
    want64 = dD.double() + lam_cls * dC.double() + (lam_reg / (B * HW)) * torch.sign(delta).double()
    out = torch.full((B, HW), SENTINEL, device=DEV)
    a, b, c = dD_full.contiguous().to(DEV), dC.to(DEV), delta.to(DEV)
    _exec(lambda: ops.delta_gan_tail_bwd(a, b, c, lam_cls, lam_reg, dD_stride=stride, out=out), [out], graphed)
    got = out.cpu()
    assert torch.equal(got, want32), float((got - want32).abs().max())
    _close(got.numpy(), want64.numpy(), "d_delta")
    assert torch.equal(got[delta == 0], (dD + 3.0 * dC)[delta == 0]), "sign(0) = 0"


# ---- head ----------------------------------------------------------------------------------------------------------------------------------------
def _head_reference(a, w, bias, mode_g, slope):
    a64, w64 = a.double(), w.double()
    z = a64 @ w64 + float(bias)
    R = a.shape[0]
    half = R if mode_g else R // 2
    t = (torch.arange(R) < half).double()
    l = torch.nn.functional.softplus(-z) * t + torch.nn.functional.softplus(z) * (1 - t)
    n = torch.where(t > 0, torch.tensor(float(half)), torch.tensor(float(max(R - half, 1))))
    loss = (l / n).sum()
    dl = (torch.sigmoid(z) - t) / n
    da = dl[:, None] * w64[None, :] * torch.where(a64 > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64))
    return z, loss, dl, dl.sum(), da, dl @ a64


@MODES
@pytest.mark.parametrize("R,mode_g", [(2, False), (6, False), (8, False), (1, True), (3, True), (4, True)])
def test_head_forward_and_backward_against_float64(ops, R, mode_g, graphed):
    gen = torch.Generator().manual_seed(30 + R)
    a = _quarter_grid((R, F), gen)
    w = _quarter_grid((F,), gen) / 128.0
    bias = torch.tensor([0.375])
    slope = 0.2
    assert bool((a == 0).any()) and bool((a < 0).any()) and float(a.abs().max()) == 2.0
    z64, loss64, dl64, db64, da64, dw64 = _head_reference(a, w, bias, mode_g, slope)
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    _, head_ws = ops.delta_gan_workspace(1, 4, torch.device(DEV))
    logits, dlogit = torch.full((R,), SENTINEL, device=DEV), torch.full((R,), SENTINEL, device=DEV)
    loss, db = torch.full((1,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
    da = torch.full((R, F), SENTINEL, device=DEV)
    dw = torch.full((F,), SENTINEL, device=DEV)
    dw_chw = torch.full((F,), SENTINEL, device=DEV)

    def launches():
        ops.logit_head_fwd(ad, wd, bd, mode_g=mode_g, logits=logits, loss=loss, dlogit=dlogit, db=db, ws=head_ws)
        ops.logit_head_bwd(ad, wd, dlogit, slope, da=da, dw=None if mode_g else dw)
        if not mode_g:
            ops.logit_head_bwd(ad, wd, dlogit, slope, da=da, dw=dw_chw, dw_shape=(256, 49))

    _exec(launches, [logits, dlogit, loss, db, da, dw, dw_chw], graphed)
    assert not head_ws.any(), "the arrival counter is left zero"
    _close(logits.cpu().numpy(), z64.numpy(), "logits")
    _close(float(loss.cpu()), float(loss64), "loss")
    _close(dlogit.cpu().numpy(), dl64.numpy(), "dlogit")
    np.testing.assert_allclose(float(db.cpu()), float(db64), rtol=1e-4, atol=2e-5 * float(dl64.abs().max()), err_msg="db")
    _close(da.cpu().numpy(), da64.numpy(), "da")
    # the slope branch, and a == 0 -> slope: exact, from the kernel's own dlogit
    got_da, dlg = da.cpu(), dlogit.cpu()
    zero = a == 0
    assert bool(zero.any()) and torch.equal(got_da[zero], ((dlg[:, None] * w[None, :]) * slope)[zero])
    pos = a > 0
    assert torch.equal(got_da[pos], (dlg[:, None] * w[None, :]).expand(R, F)[pos])
    if mode_g:
        assert bool((dw == SENTINEL).all()), "mode G passes dw = NULL: no weight gradient is formed"
    else:
        _close(dw.cpu().numpy(), dw64.numpy(), "dw")
        assert torch.equal(dw_chw.cpu(), dw.cpu().view(49, 256).t().contiguous().view(-1)), "dw in the Linear weight's own (c,h,w) order"


@pytest.mark.parametrize("mode_g", [False, True], ids=["D", "G"])
def test_head_losses_stay_finite_for_large_logits_of_both_signs(ops, mode_g):
    scale = torch.tensor([1.0, -1.0, 2.0, -2.0])                                 # logits 31.36, -31.36, 62.72, -62.72
    a = (scale[:, None] * 0.01).expand(4, F).contiguous()
    w = torch.full((F,), 0.25)
    bias = torch.zeros(1)
    z64, loss64, dl64, _, _, _ = _head_reference(a, w, bias, mode_g, 0.2)
    assert float(z64.abs().min()) >= 30.0
    logits, loss, dlogit, _ = ops.logit_head_fwd(a.to(DEV), w.to(DEV), bias.to(DEV), mode_g=mode_g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dlogit).all())
    _close(logits.cpu().numpy(), z64.numpy(), "logits")
    _close(float(loss.cpu()), float(loss64), "loss")
    _close(dlogit.cpu().numpy(), dl64.numpy(), "dlogit")
