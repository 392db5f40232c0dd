"""GPU: every draw of csrc/rng.hip (through ops.DeviceRNG) against the host Philox model oracle/rng_np.py.

Integer-valued draws (randint, rand, bernoulli, feature_mask, patch_mask, the one-hot buffers, the gathered batch) are compared
with torch.equal: bit for bit.  The float draws (randn, gumbel) are compared with the model's float64 values computed from the
same bits, under a bound that is derived here and never taken from GPU output.

The unit.  "ulp(x)" below is 2^-23 |x| (floored at the smallest fp32 subnormal): the largest an fp32 ulp can be relative to x.  A
function documented to be within e ulps has a relative error <= e 2^-23, so relative errors of a chain add in this unit without a
factor for the binade.

Assumed bounds of the device functions (HIP's math API documents its maximum ulp errors; that table is not shipped with the
toolchain, the figures are the ones it gives for single precision without fast-math): logf 2, sqrtf 1, sincosf 2 for either
result; a multiply or a fused multiply-add rounds once: 0.5.

gumbel = -logf(-logf(u)), u the exact fp32 u01_open value.  The inner logf has a relative error e1 <= 2 * 2^-23, and
log(L (1 + e1)) = log(L) + e1: an ABSOLUTE error of 2^-22 in the result, which passes through zero at u = 1/e.  The outer logf
adds 2 ulps of the result.  So |gpu - f64| <= K_GUMBEL ulp(f64) + 2^-22 with K_GUMBEL = 2.

randn: v = r * t, r = sqrtf(-2 logf(u1)), t = cos or sin of the fp32 product 6.2831855f * u2 (one IEEE multiply, reproduced by the
model, so the argument is exact).  Relative errors: logf 2 ulps, halved by the square root: 1; sqrtf 1; sincosf 2; the product 0.5:
K_RANDN = 4.5 ulps of v.  (-2 * x is exact.)  The result is fmaf(v, std, mean): the error of v reaches it scaled by |std|, that is
K_RANDN ulp(std v) whatever std v + mean cancels to — this is the absolute term that std and mean make of the argument above —
and the fmaf rounds once: 0.5 ulp of the result.  So |gpu - f64| <= K_RANDN ulp(std v) + 0.5 ulp(f64); with mean = 0, std = 1
the fmaf is exact and this is K_RANDN ulps of the value.

The yardstick: the same chains evaluated in np.float32 on the CPU (oracle randn_f32 / gumbel_f32), measured in the same unit
after the same absolute term.  The asserted bound is max(K, 2 x the yardstick's worst figure); GPU figure, yardstick and bound
are printed before the assertion (pytest -s).

The top of each uniform map: the model was searched for counters whose word is the map's largest (seed 0: counter 9588211 has
x >> 8 == 0xFFFFFF, so u01 == 1.0f and the radius is 0; counter 7566921 has w >> 8 == 0xFFFFFF, the angle 2 pi and u01_open's
top value 1 - 2^-24); test_top_of_the_maps_is_finite draws exactly those quads on the device.  The maps' edges themselves are in
tests/test_rng_model_host.py.
"""
import numpy as np
import pytest
import torch

from oracle import rng_np as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = [0, 0x9E3779B97F4A7C15]                      # the second has a high word
OFFSETS = [0, 2 ** 32 - 2, 2 ** 40 + 7]              # 2^32 - 2: the carry into counter word 1 happens inside the draw
SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025]
BIG = 4 * 256 * 4096 + 5                             # the last two quads come from the second trip of the grid-stride loop
K_GUMBEL, ABS_GUMBEL = 2.0, 2.0 ** -22
K_RANDN = 4.5
TOP_U01_X, TOP_U01_W = 9588211, 7566921              # seed 0: counters whose x / w word is the top of the maps (see above)


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd.ops


@pytest.fixture(scope="module")
def house():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import house
    return house


def _rng(ops, seed, offset):
    rng = ops.DeviceRNG(seed)
    rng.offset = offset
    return rng


def _cases():
    return [(s, o, n) for s in SEEDS for o in OFFSETS for n in SIZES]


def _eq(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = torch.nonzero(got.reshape(-1) != want.reshape(-1)).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} differ, first at {i}: {got.reshape(-1)[i].item()} against {want.reshape(-1)[i].item()}")


def _ulp(x):
    return np.maximum(np.abs(np.asarray(x, np.float64)) * 2.0 ** -23, 2.0 ** -149)


def _figure(got, ref, unit, absterm):
    """Worst error in `unit`s after `absterm` has been taken off."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all(), "non-finite value"
    return float(np.max(np.maximum(err - absterm, 0.0) / unit))


class Worst:
    """Running worst figures of one test: GPU and CPU-fp32 yardstick."""

    def __init__(self, what, K):
        self.what, self.K, self.gpu, self.yard, self.where = what, K, 0.0, 0.0, None

    def add(self, case, got, f32, ref, unit, absterm):
        assert got.dtype == torch.float32
        g = _figure(got.detach().cpu().numpy().reshape(-1), ref, unit, absterm)
        self.yard = max(self.yard, _figure(f32, ref, unit, absterm))
        if g >= self.gpu:
            self.gpu, self.where = g, case

    def check(self):
        bound = max(self.K, 2.0 * self.yard)
        print(f"{self.what}: gpu-vs-f64 {self.gpu:.3f} ulp  fp32cpu-vs-f64 {self.yard:.3f} ulp  bound {bound:.3f} ulp  (worst case {self.where})")
        assert self.gpu <= bound, f"{self.what}: {self.gpu:.3f} ulp > {bound:.3f} ulp at {self.where}"


def _add_gumbel(worst, case, got, n, seed, offset):
    ref, _ = R.gumbel_f64(n, seed, offset)
    worst.add(case, got, R.gumbel_f32(n, seed, offset)[0], ref, _ulp(ref), ABS_GUMBEL)


# ---- integer-valued draws: bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo, hi", [(0, 10), (3, 4), (-5, 5), (0, 2 ** 31 - 1), (0, 2)])     # (0, 2): the labels of moons.run_epochs
def test_randint_exact(ops, lo, hi):
    for seed, off, n in _cases():
        rng = _rng(ops, seed, off)
        out = rng.randint(lo, hi, n, DEV)
        want, _, (c0, c1) = R.randint(n, lo, hi, seed, off)
        _eq(out, want, f"randint[{lo},{hi}) n={n} seed={seed:#x} off={off}")
        assert int(out.min()) >= lo and int(out.max()) < hi
        assert rng.offset == c1 and c0 == off


@pytest.mark.parametrize("span", [2, 4, 10])
def test_randint_exclude_exact(ops, span):
    """The guarantee that the check=False launches rely on: lo <= out < hi and out != exclude, for every element."""
    for lo in (0, -3):
        for seed, off, n in _cases():
            ex = (np.arange(n) * 7 + 1) % span
            ex[n // 2:] = span - 1                                   # the last class: the cyclic +1 wraps to the first
            ex += lo
            out = _rng(ops, seed, off).randint(lo, lo + span, n, DEV, exclude=torch.from_numpy(ex).to(DEV))
            want, _, _ = R.randint(n, lo, lo + span, seed, off, exclude=ex)
            what = f"randint span {span} lo {lo} exclude n={n} seed={seed:#x} off={off}"
            _eq(out, want, what)
            got = out.cpu().numpy()
            assert (got >= lo).all() and (got < lo + span).all() and (got != ex).all(), what
            if span == 2:
                assert np.array_equal(got - lo, 1 - (ex - lo)), what


def test_rand_exact(ops):
    for seed, off, n in _cases():
        out = _rng(ops, seed, off).rand((n,), DEV)
        _eq(out, R.uniform(n, seed, off)[0], f"rand n={n} seed={seed:#x} off={off}")
        assert float(out.min()) >= 0.0 and float(out.max()) < 1.0


@pytest.mark.parametrize("keep", [0.0, 0.25, 0.5, 0.75, 1.0])
def test_bernoulli_exact(ops, keep):
    for seed, off, n in _cases():
        out = _rng(ops, seed, off).bernoulli((n,), DEV, keep)
        _eq(out, R.bernoulli(n, keep, seed, off)[0], f"bernoulli({keep}) n={n} seed={seed:#x} off={off}")
        if keep in (0.0, 1.0):
            assert float(out.min()) == float(out.max()) == keep


def test_grid_stride_tail_exact(ops):
    """More values than 4096 blocks of 256 threads hold: the last two quads (and the n % 4 tail) come from the loop's second trip."""
    seed, off = SEEDS[1], 2 ** 32 - 2
    w, (c0, c1) = R.words(BIG, seed, off)
    assert c1 - c0 == 256 * 4096 + 2
    rng = _rng(ops, seed, off)
    _eq(rng.rand((BIG,), DEV), R.u_half_open(w), "rand, grid-stride size")
    assert rng.offset == c1
    rng.offset = off
    _eq(rng.randint(-5, 5, BIG, DEV), ((w * np.uint64(10)) >> np.uint64(32)).astype(np.int64) - 5, "randint, grid-stride size")
    assert np.array_equal(R.randint(1025, -5, 5, seed, off)[0], (((w[:1025] * np.uint64(10)) >> np.uint64(32)).astype(np.int64) - 5))


def test_feature_mask_exact(ops, house):
    imm = list(house.CONFIG["immutable_idx"])
    assert imm and max(imm) < 17
    for B, D, zc in ((5, 1, None), (257, 17, imm), (64, 2, None)):
        z = None if zc is None else torch.tensor(zc, dtype=torch.int32, device=DEV)
        for seed in SEEDS:
            for off in OFFSETS:
                rng = _rng(ops, seed, off)
                out = rng.feature_mask(B, D, DEV, zero_cols=z)
                want, (_, c1) = R.feature_mask(B, D, zc, seed, off)
                _eq(out, want, f"feature_mask {B}x{D} seed={seed:#x} off={off}")
                assert rng.offset == c1
                if zc:
                    assert float(out[:, zc].abs().sum()) == 0.0


@pytest.mark.parametrize("B, H, W, ps, nsel", [
    (1, 28, 28, 7, 10),
    (257, 28, 28, 7, 10),        # a second block, with idle threads in it
    (300, 8, 8, 1, 64),          # 64 patches: the shifts reach bit 63
    (300, 8, 8, 1, 63),
    (64, 30, 30, 7, 3),          # remainder pixels stay 0
    (64, 28, 28, 7, 0),
    (64, 28, 28, 7, 20),         # nsel > total: all ones
])
def test_patch_mask_exact(ops, B, H, W, ps, nsel):
    total = (H // ps) * (W // ps)
    for seed in SEEDS:
        for off in OFFSETS:
            rng = _rng(ops, seed, off)
            out = rng.patch_mask(B, H, W, ps, nsel, DEV)
            want, (c0, c1) = R.patch_mask(B, H, W, ps, nsel, seed, off)
            _eq(out, want, f"patch_mask B={B} {H}x{W} ps={ps} nsel={nsel} seed={seed:#x} off={off}")
            assert rng.offset == off + 16 * B and c0 == off and c1 <= rng.offset
            per = out.reshape(B, -1).sum(1)
            assert float(per.min()) == float(per.max()) == min(nsel, total) * ps * ps
    if nsel >= total:
        assert float(out[:, :, :(H // ps) * ps, :(W // ps) * ps].min()) == 1.0


# ---- float draws: against float64 from the same bits -------------------------------------------------------------------------
def _add_randn(worst, case, got, n, mean, std, seed, offset):
    ref, _ = R.randn_f64(n, mean, std, seed, offset)
    sv = ref - np.float64(np.float32(mean))                          # std * v, exact to float64 rounding
    worst.add(case, got, R.randn_f32(n, mean, std, seed, offset)[0], ref, _ulp(sv), 0.5 * _ulp(ref))


@pytest.mark.parametrize("mean, std", [(0.0, 1.0), (0.3, 1.5)])
def test_randn_against_float64(ops, mean, std):
    """See the module docstring for the bound: K_RANDN ulp(std v) + 0.5 ulp(value)."""
    worst = Worst(f"randn(mean {mean}, std {std})", K_RANDN)
    for seed, off, n in _cases():
        rng = _rng(ops, seed, off)
        out = rng.randn((n,), DEV, mean=mean, std=std)
        assert out.shape == (n,) and rng.offset == off + (n + 3) // 4
        _add_randn(worst, (hex(seed), off, n), out, n, mean, std, seed, off)
    worst.check()


def test_gumbel_against_float64(ops):
    """See the module docstring for the bound: K_GUMBEL ulp(value) + 2^-22."""
    worst = Worst("gumbel", K_GUMBEL)
    for seed, off, n in _cases():
        rng = _rng(ops, seed, off)
        out = rng.gumbel((n,), DEV)
        assert out.shape == (n,) and rng.offset == off + (n + 3) // 4
        _add_gumbel(worst, (hex(seed), off, n), out, n, seed, off)
    worst.check()


def test_top_of_the_maps_is_finite(ops):
    """The quads whose uniform is the largest value of each map (found with the model, see the module docstring)."""
    x = R.draw(0, TOP_U01_X, [0])[0]
    w = R.draw(0, TOP_U01_W, [0])[0]
    assert int(x[0]) >> 8 == 0xFFFFFF and int(w[3]) >> 8 == 0xFFFFFF and int(w[3]) >> 9 == 0x7FFFFF
    assert R.u01(x[:1])[0] == np.float32(1.0) and R.u01_open(w[3:])[0] == np.float32(1.0) - np.float32(2.0 ** -24)
    wn, wg = Worst("randn at the top of u01", K_RANDN), Worst("gumbel at the top of u01_open", K_GUMBEL)
    for off in (TOP_U01_X, TOP_U01_W):
        out = _rng(ops, 0, off).randn((4,), DEV)
        assert bool(torch.isfinite(out).all())
        _add_randn(wn, off, out, 4, 0.0, 1.0, 0, off)
        g = _rng(ops, 0, off).gumbel((4,), DEV)
        assert bool(torch.isfinite(g).all())
        _add_gumbel(wg, off, g, 4, 0, off)
        if off == TOP_U01_X:
            assert out[:2].abs().tolist() == [0.0, 0.0]              # radius sqrt(-2 log 1) = 0
    wn.check()
    wg.check()


# ---- fused draws ---------------------------------------------------------------------------------------------------------
HOUSE_SHAPES = [(5, 17, 70), (257, 17, 70), (4096, 17, 70)]          # the last: 71 680 quads, above the 256-block cap of the ticketed launches
NC = 4


def _house_bufs(B, D, T):
    out = (torch.full((B,), -1, dtype=torch.int64, device=DEV), torch.full((B, D), -1.0, device=DEV), torch.full((B, T), float("nan"), device=DEV))
    oh = (torch.full((B, NC), -1.0, device=DEV), torch.full((B, NC), -1.0, device=DEV))
    return out, oh


def _check_house(worst, case, want, t, mask, noise, oh, seed, off_n):
    _eq(t, want["target"], f"{case}: target")
    _eq(mask, want["mask"], f"{case}: mask")
    _eq(oh[0], want["onehot_t"], f"{case}: one-hot of the target")
    _eq(oh[1], want["onehot_y"], f"{case}: one-hot of y")
    _add_gumbel(worst, case, noise, noise.numel(), seed, off_n)


def _y(B, salt):
    return (np.arange(B) * 5 + salt) % NC


@pytest.mark.parametrize("B, D, T", HOUSE_SHAPES)
def test_house_draws_host_offsets(ops, house, B, D, T):
    imm = list(house.CONFIG["immutable_idx"])
    z = torch.tensor(imm, dtype=torch.int32, device=DEV)
    worst = Worst(f"house_draws noise B={B}", K_GUMBEL)
    for seed, off in ((SEEDS[0], OFFSETS[2]), (SEEDS[1], OFFSETS[1])):
        y = _y(B, 1)
        rng = _rng(ops, seed, off)
        out, oh = _house_bufs(B, D, T)
        rng.house_draws(torch.from_numpy(y).to(DEV), NC, D, T, z, out, onehots=oh)
        want, (c0, c1) = R.house_draws(y, NC, D, T, imm, seed, off)
        assert rng.offset == c1 == off + ops.DeviceRNG.house_draws_span(B, D, T)
        _check_house(worst, (hex(seed), off), want, out[0], out[1], out[2], oh, seed, c1 - (B * T + 3) // 4)
        got = out[0].cpu().numpy()
        assert (got != y).all() and (got >= 0).all() and (got < NC).all()
    worst.check()


@pytest.mark.parametrize("B, D, T", HOUSE_SHAPES)
def test_house_draws_device_counter(ops, house, B, D, T):
    """Two launches in a row from one device counter that starts at 2^32 - 100: each draws the model's values at the counter's
    offset, advances it by house_draws_span and leaves the ticket at 0."""
    imm = list(house.CONFIG["immutable_idx"])
    z = torch.tensor(imm, dtype=torch.int32, device=DEV)
    seed, start = SEEDS[1], 2 ** 32 - 100
    rng = _rng(ops, seed, start)
    ctr = rng.device_counter(torch.device(DEV))
    span = ops.DeviceRNG.house_draws_span(B, D, T)
    worst = Worst(f"house_draws(counter) noise B={B}", K_GUMBEL)
    first = None
    for it in range(2):
        off = start + it * span
        y = _y(B, it)
        out, oh = _house_bufs(B, D, T)
        rng.house_draws(torch.from_numpy(y).to(DEV), NC, D, T, z, out, onehots=oh, counter=ctr)
        assert ctr.tolist() == [off + span, 0], f"launch {it}: counter {ctr.tolist()}"
        assert rng.offset == start                                   # the host-side offset is not touched
        want, (_, c1) = R.house_draws(y, NC, D, T, imm, seed, off)
        _check_house(worst, f"launch {it}", want, out[0], out[1], out[2], oh, seed, c1 - (B * T + 3) // 4)
        if it == 0:
            first = [o.clone() for o in out]
        else:
            assert not torch.equal(first[1], out[1]) and not torch.equal(first[2], out[2])     # not the first launch's numbers again
    worst.check()


@pytest.mark.parametrize("B, D, T", HOUSE_SHAPES)
def test_house_batch_draws(ops, house, B, D, T):
    """house_batch_draws twice in a row: the gathered x / y / source rows and every draw equal the model's, the counter advances by
    house_draws_span, the cursor by B, the ticket returns to 0."""
    imm = list(house.CONFIG["immutable_idx"])
    z = torch.tensor(imm, dtype=torch.int32, device=DEV)
    seed, start = SEEDS[1], 2 ** 32 - 100
    rs = np.random.RandomState(B)
    N = 2 * B + 3
    X, Y, perm = rs.uniform(-1, 1, (N, D)).astype(np.float32), rs.randint(0, NC, N).astype(np.int64), rs.permutation(N).astype(np.int64)
    dX, dY, dperm = (torch.from_numpy(a).to(DEV) for a in (X, Y, perm))
    rng = _rng(ops, seed, start)
    ctr = rng.device_counter(torch.device(DEV), cursor=True)
    span = ops.DeviceRNG.house_draws_span(B, D, T)
    worst = Worst(f"house_batch_draws noise B={B}", K_GUMBEL)
    first = None
    for it in range(2):
        off = start + it * span
        (o_t, o_m, o_n), oh = _house_bufs(B, D, T)
        o_x, o_y = torch.full((B, D), float("nan"), device=DEV), torch.full((B,), -1, dtype=torch.int64, device=DEV)
        src = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        rng.house_batch_draws(dX, dY, dperm, NC, T, z, (o_x, o_y, o_t, o_m, o_n), oh, ctr, src_out=src)
        assert ctr.tolist() == [off + span, 0, (it + 1) * B, 0], f"launch {it}: counter {ctr.tolist()}"
        want, (_, c1) = R.house_batch_draws(X, Y, perm, it * B, B, NC, T, imm, seed, off)
        assert np.array_equal(want["src"], perm[it * B:(it + 1) * B])
        _eq(src, want["src"], f"launch {it}: source rows")
        _eq(o_x, want["x"], f"launch {it}: x")
        _eq(o_y, want["y"], f"launch {it}: y")
        _check_house(worst, f"launch {it}", want, o_t, o_m, o_n, oh, seed, c1 - (B * T + 3) // 4)
        assert bool((o_t != o_y).all())
        if it == 0:
            first = (o_m.clone(), o_n.clone())
        else:
            assert not torch.equal(first[0], o_m) and not torch.equal(first[1], o_n)
    worst.check()


def test_refusals_come_before_any_launch(ops):
    """PCG_REQUIRE paths of the draws: bad arguments are refused with an error, the stream's buffers untouched."""
    from pcgan_amd import _lib
    rng = ops.DeviceRNG(1)
    with pytest.raises(_lib.PcgError):
        rng.patch_mask(4, 9, 9, 1, 5, DEV)                           # 81 patches: more than the 64-bit set holds
    with pytest.raises(_lib.PcgError):
        rng.randint(3, 3, 8, DEV)                                    # empty range
    with pytest.raises(_lib.PcgError):
        rng.randint(3, 4, 8, DEV, exclude=torch.full((8,), 3, dtype=torch.int64, device=DEV))    # nothing left to draw
    with pytest.raises(_lib.PcgError):
        rng.bernoulli((8,), DEV, 1.5)
