"""GPU: the five entries of csrc/delta_gan.hip through pcgan_amd.ops, each alone, eagerly and from a captured and
replayed HIP graph, with every output pre-filled with a sentinel.

Batches are B = 1, 3 and 4 (R = 2, 6, 8 rows for the head in mode D): the smallest at which the row halves, odd rows and the partial
last chunk / last 16-byte group can go wrong; the spatial sizes are the nets' own, 784 pixels and F = 12544.  Only the tail forward walks
its data under a capped grid, and its grid is a parameter: grid = 2 on the three chunks of B = 3 is the case beyond one trip.
Copies (entry, x_cf) are compared with zero tolerance; sums and products against a float64 evaluation by the project's rule of §3.18,
rtol 1e-4 and atol 2e-5 * max|reference|.

Training runs these kernels at batch 128, where whole parts of them run that B <= 4 never reaches; the cases at the end of each
section reach them with small F and HW (free parameters of the entries) and a sentinel tail behind every output (`_Guard`):
  head backward   R = 16 ... 257 (1 to 17 rows per wave; clipped, short and empty row groups), F = 4, 252, 256, 260 (idle lanes)
  head forward    R up to 600 (second and third trip of the finishing loop), F = 4, 1028, 12544; logits equal to float64
  tail forward    257, 258 and 1025 chunks: beyond the finishing loop's first trip and beyond the grid cap; loss_reg exact
  entry           25088 rows over 12544 head columns, and 32 head columns over 16 rows
Measured (MI355X): dw uses at most 0.111 of its bound (R 17, F 256; 0.019 at training's R 256), db at most 0.089 of its bound
(mode G, R 301, F 1028); the 135 cases of this file take 7 s."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
TAIL = 64
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


class _Guard:
    """Sentinel-filled outputs, each a view into an allocation with TAIL more sentinels behind it (tests/test_hip_house_fused_edges.py's
    _Guarded, for outputs the test allocates itself): an element not written shows as the sentinel, a write past the end in the tail."""

    def __init__(self):
        self.flats = []

    def new(self, *shape):
        n = int(np.prod(shape))
        flat = torch.full((n + TAIL,), SENTINEL, device=DEV)
        self.flats.append((flat, n))
        return flat[:n].view(shape)

    def all(self):
        """The whole allocations, tails included: what _exec fills again before a capture."""
        return [flat for flat, _ in self.flats]

    def check_tails(self, what):
        for flat, n in self.flats:
            assert bool((flat[n:] == SENTINEL).all()), f"{what}: a write past the end of an output of {n} elements"


# ---- entry -----------------------------------------------------------------------------------------------------------------------------------
def _entry_case(ops, B, HW, head_shape, graphed):
    C, P = head_shape
    F = C * P
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
    _exec(lambda: ops.delta_gan_entry(x, y, t, EG, ED, g_in=g_in, d_in=d_in, labels_2b=lab, head_w=w, head_w_packed=wp, head_shape=(C, P)),
          [g_in, d_in, lab, wp], graphed)
    assert torch.equal(g_in, ops.embed_concat_fwd(x, t, EG, None))
    assert torch.equal(d_in[:B], ops.embed_concat_fwd(x, y, ED, None))
    assert torch.equal(d_in[B:, :, 1], ops.embed_concat_fwd(x, t, ED, None)[:, :, 1])
    assert bool((d_in[B:, :, 0] == SENTINEL).all()), "channel 0 of rows B..2B belongs to the tail forward"
    assert torch.equal(lab, torch.cat([y, t]))
    assert torch.equal(wp, w.view(C, P).t().contiguous().view(-1))
    # the regather after Adam(D): another table, another target; nothing but channel 1 of rows B..2B (and the packed weight) may change
    before_g, before_d, before_lab = g_in.clone(), d_in.clone(), lab.clone()
    t2 = ((t + 1) % K).contiguous()
    w2 = (w * 2).contiguous()
    _exec(lambda: ops.delta_gan_entry(None, None, t2, None, ED2, d_in=d_in, head_w=w2, head_w_packed=wp, head_shape=(C, P), regather=True),
          [d_in, wp], graphed)
    assert torch.equal(g_in, before_g) and torch.equal(lab, before_lab)
    assert torch.equal(d_in[:B], before_d[:B]) and torch.equal(d_in[B:, :, 0], before_d[B:, :, 0])
    assert torch.equal(d_in[B:, :, 1], ED2[t2])
    assert torch.equal(wp, w2.view(C, P).t().contiguous().view(-1))


@MODES
@pytest.mark.parametrize("B", [1, 3, 4])
def test_entry_is_embed_concat_bit_for_bit_and_regather_touches_one_channel(ops, B, graphed):
    _entry_case(ops, B, HW, (256, 49), graphed)


@MODES
@pytest.mark.parametrize("B,hw,head_shape", [(32, 784, (256, 49)), (1, 16, (4, 8))], ids=["rows25088_head12544", "rows16_head32"])
def test_entry_with_rows_outnumbering_head_columns_and_the_reverse(ops, B, hw, head_shape, graphed):
    """The grid covers max(B*HW, C*P) threads.  B = 32: 25088 rows of threads over 12544 head columns, the side every training step
    (100352 > 12544) takes and B <= 4 never does; B = 1, HW = 16, head 4 x 8: 32 head columns over 16 rows, within one workgroup."""
    _entry_case(ops, B, hw, head_shape, graphed)


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


@MODES
@pytest.mark.parametrize("B,hw,chunks", [(16385, 16, 257), (65793, 4, 258), (65537, 16, 1025)], ids=["chunks257", "chunks258_last4", "chunks1025"])
def test_tail_forward_beyond_256_chunks_and_beyond_the_grid_cap(ops, B, hw, chunks, graphed):
    """More chunks of 1024 elements than the finishing workgroup has threads (its `c += 256` loop takes a second trip: 257, and 258
    with a last chunk of 4 elements, one live thread) and more than the grid cap of 1024 workgroups (1025: with grid 0 workgroup 0 walks
    two chunks).  Grids 0 (the cap), 1, 7 and 1024.  Deltas on the 1/32 grid: every thread's four-term sum, every chunk sum (at most
    8192 units of 1/32) and the double total are exact, so loss_reg equals the float64 mean rounded once, whatever the grid."""
    n = B * hw
    assert -(-n // 1024) == chunks and (chunks != 258 or n - 257 * 1024 == 4)
    gen = torch.Generator().manual_seed(40 + chunks)
    x = 2 * torch.rand(B, hw, generator=gen) - 1
    delta = _quarter_grid((B, hw), gen) * 0.125
    want = x + delta
    want_loss = float(np.float32(float(delta.double().abs().sum()) / n))
    xd, dd = x.to(DEV), delta.to(DEV)
    tail_ws, _ = ops.delta_gan_workspace(B, hw, torch.device(DEV))
    for grid in (0, 1, 7, 1024):
        g = _Guard()
        x_cf, d_in, loss = g.new(B, hw), g.new(2 * B, hw, 2), g.new(1)
        _exec(lambda: ops.delta_gan_tail_fwd(xd, dd, d_in, x_cf=x_cf, loss_reg=loss, ws=tail_ws, grid=grid), g.all(), graphed)
        g.check_tails(f"grid {grid}")
        assert torch.equal(x_cf.cpu(), want) and torch.equal(d_in[B:, :, 0].cpu(), want)
        assert bool((d_in[:B] == SENTINEL).all()) and bool((d_in[B:, :, 1] == SENTINEL).all())
        assert not tail_ws[:16].any(), "the arrival counter is left zero"
        assert float(loss.cpu()) == want_loss, f"grid {grid}: loss_reg {float(loss.cpu())!r}, float64 mean rounded once {want_loss!r}"


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


# ---- head at the row counts and widths of training and at every edge of its loops ---------------------------------------------------------------
U = 2.0 ** -24
HEAD_BWD_CASES = [(R, 260) for R in (16, 17, 31, 32, 33, 128, 256, 257)] + [(17, F_) for F_ in (4, 252, 256)]


@MODES
@pytest.mark.parametrize("R,F_", HEAD_BWD_CASES, ids=[f"R{R}_F{F_}" for R, F_ in HEAD_BWD_CASES])
def test_head_backward_row_groups_and_column_blocks(ops, R, F_, graphed):
    """logit_head_bwd_kernel: sixteen waves, wave g owns rows g*rpg .. min((g+1)*rpg, R) with rpg = ceil(R / 16); lane = one 16-byte
    column group, 64 to a workgroup.

      R 16 rpg 1                      R 17 rpg 2: group 8 holds one row, groups 9..15 start beyond R      R 31 rpg 2: the last group is short
      R 32 rpg 2, every group full    R 33 rpg 3: eleven full groups, five empty                          R 128, 256: training's rpg 8 and 16
      R 257 rpg 17: fifteen full groups, the last holds two rows
      F 4: one live lane   F 252: 63 lanes   F 256: exactly one workgroup   F 260: a second workgroup with one live lane

    dlogit is a given vector, so the reference sees the kernel's operand.  da is the fp32 expression (dl * w) * (a > 0 ? 1 : slope)
    evaluated in float32 on the CPU, bit for bit on every element (the kernel has contraction off).  dw against float64 within
    (rpg + 15 + 2) * 2^-24 * sum_r |dl_r * a_rf| per column: an fma chain of rpg rows, the fifteen adds of the fold, slack of two; a
    zero bound asks for equality.  dw = None, flat, and both (C, P) orders of F (for F = 260: (65, 4) and (4, 65)); tails intact."""
    gen = torch.Generator().manual_seed(1000 * R + F_)
    a = _quarter_grid((R, F_), gen)
    w = _quarter_grid((F_,), gen) / 128.0
    dl = torch.randn(R, generator=gen) / R
    slope = 0.2
    assert bool((a == 0).any()) and bool((a < 0).any()) and bool((a > 0).any())
    want_da = (dl[:, None] * w[None, :]) * torch.where(a > 0, torch.tensor(1.0), torch.tensor(slope))
    assert want_da.dtype == torch.float32
    dw64 = (dl.double() @ a.double()).numpy()
    bound = (-(-R // 16) + 15 + 2) * U * (dl.double().abs() @ a.double().abs()).numpy()
    orders = [None, (F_ // 4, 4), (4, F_ // 4)]
    ad, wd, dld = a.to(DEV), w.to(DEV), dl.to(DEV)
    g = _Guard()
    da_only = g.new(R, F_)
    das = [g.new(R, F_) for _ in orders]
    dws = [g.new(F_) for _ in orders]

    def launches():
        ops.logit_head_bwd(ad, wd, dld, slope, da=da_only, dw=None)
        for da, dw, order in zip(das, dws, orders):
            ops.logit_head_bwd(ad, wd, dld, slope, da=da, dw=dw, dw_shape=order)

    _exec(launches, g.all(), graphed)
    g.check_tails(f"R {R} F {F_}")
    for da in [da_only] + das:
        got = da.cpu()
        assert torch.equal(got, want_da), f"da: {int((got != want_da).sum())} elements differ, max {float((got - want_da).abs().max()):.3e}"
    share = 0.0
    flat = dws[0].cpu()
    for dw, order in zip(dws, orders):
        got = dw.cpu()
        if order is not None:                                                    # packed column p * C + c is stored at [c * P + p]
            got = got.view(order[0], order[1]).t().contiguous().view(-1)
            assert torch.equal(got, flat), f"dw in order {order} is not the flat dw reordered"
        err = np.abs(got.double().numpy() - dw64)
        assert (err <= bound).all(), f"dw {order}: column {int(np.argmax(err - bound))}: error {err.max():.3e}, bound there {bound[np.argmax(err - bound)]:.3e}"
        share = max(share, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"head bwd R {R} F {F_} rpg {-(-R // 16)}: dw uses {share:.3f} of its bound")


HEAD_FWD_CASES = ([(R, F_, False) for R in (16, 34, 256, 258, 600) for F_ in (4, 1028)] + [(R, F_, True) for R in (17, 255, 257, 301) for F_ in (4, 1028)]
                  + [(256, F, False), (128, F, True)])


@MODES
@pytest.mark.parametrize("R,F_,mode_g", HEAD_FWD_CASES, ids=[f"{'G' if m else 'D'}_R{R}_F{F_}" for R, F_, m in HEAD_FWD_CASES])
def test_head_forward_finishing_loop_and_exact_logits(ops, R, F_, mode_g, graphed):
    """logit_head_fwd_kernel: the finishing workgroup's loop `q += 256` over the rows with threads beyond one wave at work (R >= 65), the
    real / fake split between waves (R 256: row 128), a second trip (R 257, 258, 301) and a third (R 600); the dot product's own loop
    with one 16-byte group (F 4), one full trip plus one group (F 1028: 257 groups) and training's 3136 (F 12544 at training's
    R = 256 in mode D and R = 128 in mode G).

    a and bias on the 1/4 grid, w on the 1/4 grid over 128: every product is a multiple of 2^-11 and every partial sum stays below
    2^24 of them, so fp32 is exact in any order and the logits must EQUAL the float64 dot product plus bias.  dlogit and loss by the
    file's rule; db against the float64 sum of the kernel's own dlogit within (ceil(R / 256) + 8 + 2) * 2^-24 * sum|dlogit| (a thread's
    chain, the eight levels of the tree, slack of two): the real and fake halves cancel, so max|dlogit| is no scale for it."""
    gen = torch.Generator().manual_seed(2000 * R + F_ + int(mode_g))
    a = _quarter_grid((R, F_), gen)
    w = _quarter_grid((F_,), gen) / 128.0
    bias = torch.tensor([0.375])
    z64, loss64, dl64, _, _, _ = _head_reference(a, w, bias, mode_g, 0.2)
    assert float((a.double().abs() @ w.double().abs()).max()) * 2048 + 768 < 2 ** 24, "not exact in fp32: the test proves nothing"
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    _, head_ws = ops.delta_gan_workspace(1, 4, torch.device(DEV))
    g = _Guard()
    logits, dlogit, loss, db = g.new(R), g.new(R), g.new(1), g.new(1)
    _exec(lambda: ops.logit_head_fwd(ad, wd, bd, mode_g=mode_g, logits=logits, loss=loss, dlogit=dlogit, db=db, ws=head_ws), g.all(), graphed)
    g.check_tails(f"R {R} F {F_}")
    assert not head_ws.any(), "the arrival counter is left zero"
    got_z = logits.cpu().double()
    assert torch.equal(got_z, z64), f"logits: {int((got_z != z64).sum())} of {R} differ from the exact value, max {float((got_z - z64).abs().max()):.3e}"
    _close(float(loss.cpu()), float(loss64), "loss")
    got_dl = dlogit.cpu().double()
    _close(got_dl.numpy(), dl64.numpy(), "dlogit")
    db_bound = (-(-R // 256) + 8 + 2) * U * float(got_dl.abs().sum())
    db_err = abs(float(db.cpu()) - float(got_dl.sum()))
    print(f"head fwd {'G' if mode_g else 'D'} R {R} F {F_}: db {float(db.cpu()):.3e}, error {db_err:.3e}, {db_err / db_bound:.3f} of its bound")
    assert db_err <= db_bound
