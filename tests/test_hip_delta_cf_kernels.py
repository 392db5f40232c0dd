"""GPU: the three entries of csrc/delta_cf_eval.hip through pcgan_amd.ops, each alone, eagerly and from a captured
and replayed HIP graph, with every output pre-filled with a sentinel.

Windows (B, T, q0, nq): the whole sweep of 3 rows, a window that starts and ends inside a target, one row, and the per-row form; HW =
784 (the nets' own: 196 16-byte groups over 64 lanes, so lanes hold 4 or 3 groups) and HW = 16 (4 groups: 60 idle lanes).  Copies and
the clamp are compared with zero tolerance against torch; the three sums against a float64 evaluation at rtol 1e-6; the draw bit for
bit against the host Philox model oracle/rng_np.py and against DeviceRNG.randint."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
K = 10
MODES = pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
WINDOWS = [(3, 10, 0, 30, False), (3, 10, 7, 11, False), (1, 10, 0, 10, False), (5, 1, 0, 5, True)]
WINDOW_IDS = ["sweep", "inside-a-target", "one-row", "per-row"]


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    return pcgan_amd.ops


def _capture(launches, before_capture=None):
    """Capture `launches` after one real execution of them on the current stream (they allocate nothing: every output is given)."""
    from pcgan_amd import nn as N
    cap = N._HipGraphCapture(torch.device(DEV), tick=False)
    launches()
    if before_capture is not None:
        before_capture()
    torch.cuda.synchronize()
    cap.begin()
    try:
        launches()
    finally:
        graph = cap.end()
    torch.cuda.synchronize()
    return graph


def _exec(launches, outs, graphed):
    """Run `launches` eagerly or as one replay of a captured graph; `outs` (tensors) are sentinel-filled first."""
    fills = [(t, t.clone()) for t in outs]
    if graphed:
        graph = _capture(launches, lambda: [t.copy_(t0) for t, t0 in fills])
        assert all(torch.equal(t, t0) for t, t0 in fills), "captured, not run"
        graph.replay()
    else:
        launches()
    torch.cuda.synchronize()


def _queries(B, q0, nq):
    q = torch.arange(q0, q0 + nq)
    return q // B, q % B


# ---- entry -----------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("HW", [784, 16])
@pytest.mark.parametrize("B,T,q0,nq,per_row", WINDOWS, ids=WINDOW_IDS)
def test_entry_equals_torch_indexing_bit_for_bit(ops, B, T, q0, nq, per_row, HW, graphed):
    gen = torch.Generator().manual_seed(100 * B + q0)
    x = (2 * torch.rand(B, HW, generator=gen) - 1)
    table = torch.randn(K, HW, generator=gen)
    target = torch.tensor([7, 0, 9, 3, 3]) if per_row else None
    t, b = _queries(B, q0, nq)
    cls = target[b] if per_row else t
    want = torch.stack([x[b], table[cls]], dim=-1)
    out = torch.full((nq, HW, 2), SENTINEL, device=DEV)
    xd, td, tg = x.to(DEV), table.to(DEV), (target.to(DEV) if per_row else None)
    _exec(lambda: ops.delta_cf_entry(xd, tg, td, T, q0, nq, out=out), [out], graphed)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("B", [1, 4])
def test_entry_at_t1_is_the_training_entrys_g_in(ops, B):
    gen = torch.Generator().manual_seed(B)
    x = (2 * torch.rand(B, 784, generator=gen) - 1).to(DEV)
    y, t = (torch.randint(0, K, (B,), generator=gen).to(DEV) for _ in range(2))
    EG, ED = (torch.randn(K, 784, generator=gen).to(DEV) for _ in range(2))
    g_in, _ = ops.delta_gan_entry(x, y, t, EG, ED)
    assert torch.equal(ops.delta_cf_entry(x, t, EG), g_in)


def test_entry_clamps_a_device_label_and_refuses_the_same_label_as_a_host_copy(ops):
    from pcgan_amd import PcgError
    gen = torch.Generator().manual_seed(3)
    x = (2 * torch.rand(3, 16, generator=gen) - 1).to(DEV)
    table = torch.randn(K, 16, generator=gen).to(DEV)
    bad = torch.tensor([-3, 12, 4])
    out = ops.delta_cf_entry(x, bad.to(DEV), table)
    assert torch.equal(out[:, :, 1], table[bad.clamp(0, K - 1).to(DEV)]) and torch.equal(out[:, :, 0], x)
    with pytest.raises(PcgError, match="label -3 of row 0"):
        ops.delta_cf_entry(x, bad.to(DEV), table, target_host=bad)
    ok = torch.tensor([0, 9, 4])
    assert torch.equal(ops.delta_cf_entry(x, ok.to(DEV), table, target_host=ok)[:, :, 1], table[ok.to(DEV)])
    with pytest.raises(PcgError, match="T = 1"):
        ops.delta_cf_entry(x, ok.to(DEV), table, T=2)
    with pytest.raises(PcgError, match="window"):
        ops.delta_cf_entry(x, None, table, T=10, q0=25, nq=6)


# ---- tail --------------------------------------------------------------------------------------------------------------------------------------
def _tail_inputs(B, nq, q0, HW, with_nan):
    """x in [-1, 1] and delta such that the window holds: sums clamped on both sides, sums exactly +1 and -1, delta == 0, and (one
    element, with_nan) a NaN."""
    gen = torch.Generator().manual_seed(7 * B + q0 + HW)
    x = 2 * torch.rand(B, HW, generator=gen) - 1
    delta = 0.8 * torch.randn(nq, HW, generator=gen)
    _, b = _queries(B, q0, nq)
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0.75, -0.75, 0.5, -0.25
    delta[:, 0], delta[:, 1] = 0.25, -0.25                     # x + delta == +1 and -1 exactly
    delta[:, 2], delta[:, 3] = 2.0, -3.0                       # clamped on both sides
    delta[:, 4:8] = 0.0                                        # delta == 0
    if with_nan:
        delta[nq - 1, HW - 1] = float("nan")
    s = x[b] + delta
    assert bool((s > 1).any()) and bool((s < -1).any()) and bool((s == 1).any()) and bool((s == -1).any())
    return x, delta, b


@MODES
@pytest.mark.parametrize("HW", [784, 16])
@pytest.mark.parametrize("B,T,q0,nq,per_row", WINDOWS, ids=WINDOW_IDS)
def test_tail_clamps_as_torch_and_sums_against_float64(ops, B, T, q0, nq, per_row, HW, graphed):
    x, delta, b = _tail_inputs(B, nq, q0, HW, with_nan=True)
    want = (x[b] + delta).clamp(-1, 1)                         # the fp32 sum is rounded, then clamped; torch keeps the NaN
    assert bool(torch.isnan(want[nq - 1, HW - 1]))
    x_cf = torch.full((nq, HW), SENTINEL, device=DEV)
    sums = torch.full((nq, 3), SENTINEL, device=DEV)
    xd, dd = x.to(DEV), delta.to(DEV)
    _exec(lambda: ops.delta_cf_tail(dd, xd, T, q0, nq, out={"x_cf": x_cf, "sums": sums}), [x_cf, sums], graphed)
    got = x_cf.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))
    c64 = want.double() - x[b].double()
    ref = torch.stack([c64.abs().sum(1), delta.double().abs().sum(1), (c64 * c64).sum(1)], dim=1).numpy()
    s = sums.cpu().double().numpy()
    assert np.isnan(s[nq - 1]).all() and np.isnan(ref[nq - 1]).all(), "the NaN row's sums are NaN"
    rel = np.abs(s[:nq - 1] - ref[:nq - 1]) / np.abs(ref[:nq - 1])
    print(f"sums: worst relative error {rel.max() if rel.size else 0.0:.3e} against float64 (rtol 1e-6)")
    np.testing.assert_allclose(s[:nq - 1], ref[:nq - 1], rtol=1e-6, atol=0.0)


def test_tail_eager_equals_a_replayed_graph_and_refuses_mismatched_windows(ops):
    from pcgan_amd import PcgError
    B, T, q0, nq, HW = 3, 10, 7, 11, 784
    x, delta, _ = _tail_inputs(B, nq, q0, HW, with_nan=False)
    xd, dd = x.to(DEV), delta.to(DEV)
    e_cf, e_s = ops.delta_cf_tail(dd, xd, T, q0, nq)
    g_cf, g_s = torch.full_like(e_cf, SENTINEL), torch.full_like(e_s, SENTINEL)
    _exec(lambda: ops.delta_cf_tail(dd, xd, T, q0, nq, out={"x_cf": g_cf, "sums": g_s}), [g_cf, g_s], True)
    assert torch.equal(e_cf, g_cf) and torch.equal(e_s, g_s)
    with pytest.raises(PcgError, match="window"):
        ops.delta_cf_tail(dd, xd, T, 25, nq)
    with pytest.raises(PcgError, match="holds 11 queries"):
        ops.delta_cf_tail(dd, xd, T, q0, 5)


# ---- the class draw ----------------------------------------------------------------------------------------------------------------------------
OFFSETS = (0, 1, 2 ** 32 - 1, 2 ** 32)


def _model(k, seed, offset):
    from oracle import rng_np
    return int(rng_np.randint(1, 0, k, seed, offset)[0][0])


@pytest.mark.parametrize("k", [10, 3])
def test_draw_by_value_is_one_class_for_all_rows_and_the_host_models(ops, k):
    seed = 0x1234_5678_9ABC_DEF0
    seen = set()
    for B in (1, 5, 257, 1000):
        for off in OFFSETS:
            target = torch.full((B,), -7, dtype=torch.int64, device=DEV)
            ops.delta_gan_target_draw(target, k, seed, offset=off)
            rng = ops.DeviceRNG(seed)
            rng.offset = off
            one = rng.randint(0, k, 1, DEV)
            got = target.cpu()
            assert bool((got == got[0]).all()), (B, off)
            assert int(got[0]) == _model(k, seed, off) == int(one.cpu()[0]), (B, off)
            assert rng.offset == off + 1
            seen.add(int(got[0]))
    assert len(seen) > 1


@pytest.mark.parametrize("start", OFFSETS)
def test_draw_counter_form_walks_the_stream_eagerly_and_on_every_replay(ops, start):
    seed, B = 77, 257
    rng = ops.DeviceRNG(seed)
    rng.offset = start
    want = [_model(K, seed, start + i) for i in range(3)]
    # three eager launches
    ctr = rng.device_counter(DEV)
    target = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    got = []
    for _ in range(3):
        rng.delta_gan_target(target, K, counter=ctr)
        got.append(target.cpu().clone())
    assert [int(g[0]) for g in got] == want and all(bool((g == g[0]).all()) for g in got)
    assert ctr.cpu().tolist() == [start + 3, 0] and rng.offset == start, "the counter form leaves the host offset alone"
    # three replays of one captured launch
    ctr2 = rng.device_counter(DEV)
    ctr0 = ctr2.clone()
    graph = _capture(lambda: rng.delta_gan_target(target, K, counter=ctr2), lambda: ctr2.copy_(ctr0))
    assert ctr2.cpu().tolist() == [start, 0], "captured, not run"
    got = []
    for _ in range(3):
        graph.replay()
        got.append(target.cpu().clone())
    assert [int(g[0]) for g in got] == want and all(bool((g == g[0]).all()) for g in got)
    assert ctr2.cpu().tolist() == [start + 3, 0]
    # by value through DeviceRNG: the same classes, and the host offset advances by one counter value per draw
    for i in range(3):
        rng.delta_gan_target(target, K)
        assert int(target.cpu()[0]) == want[i] and rng.offset == start + i + 1
