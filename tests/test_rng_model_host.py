"""CPU: the host model of csrc/rng.hip (oracle/rng_np.py) against the Philox-4x32-10 standard, the edges of its uniform maps, and
the stream bookkeeping of ops.DeviceRNG against the counter ranges the model reads.  tests/test_hip_rng_exact.py then pins the
device to this model."""
import numpy as np
import pytest
import torch

from oracle import rng_np as R

EDGE_WORDS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]


# ---- the model is Philox-4x32-10 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    """The known-answer vectors of Random123 (kat_vectors, philox4x32 with 10 rounds)."""
    got = R.philox4x32_10(ctr, key)
    assert " ".join(f"{int(w[0]):08x}" for w in got) == want


def test_philox_is_vectorised_and_draw_lays_out_the_counter():
    """draw(seed, offset, idx) is Philox on {lo32(c), hi32(c), 0x5eed5eed, 0}, c = offset + idx mod 2^64, key (lo32, hi32)(seed)."""
    seed, off = 0x9E3779B97F4A7C15, 2 ** 32 - 2
    q = R.draw(seed, off, np.arange(5))
    assert q.shape == (5, 4) and q.dtype == np.uint64 and int(q.max()) <= 0xFFFFFFFF
    for i in range(5):
        c = off + i
        one = R.philox4x32_10((c & 0xFFFFFFFF, c >> 32, 0x5EED5EED, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(w[0]) for w in one] == q[i].tolist()
    assert (c >> 32) == 1                                            # the carry into counter word 1 happened inside the range
    # counter word 1 and the key's high word matter; the sum wraps mod 2^64
    assert not np.array_equal(R.draw(seed, 2 ** 32, [0]), R.draw(seed, 0, [0]))
    assert not np.array_equal(R.draw(seed, 0, [0]), R.draw(seed & 0xFFFFFFFF, 0, [0]))
    assert np.array_equal(R.draw(seed, 2 ** 64 - 1, [1]), R.draw(seed, 0, [0]))


# ---- uniform-map edges ----------------------------------------------------------------------------------------------------
def test_uniform_map_edges():
    v = np.array(EDGE_WORDS, dtype=np.uint64)
    a, b, c = R.u01(v), R.u01_open(v), R.u_half_open(v)
    assert a.dtype == b.dtype == c.dtype == np.float32
    assert (a > 0).all() and (a <= 1).all() and (b > 0).all() and (b < 1).all() and (c >= 0).all() and (c < 1).all()
    # the rounding of (float)(v >> 8) + 0.5f is the kernel's: the top word gives exactly 1.0f under u01, 1 - 2^-24 under u01_open
    assert a[-1] == np.float32(1.0) and b[-1] == np.float32(1.0) - np.float32(2.0 ** -24)
    assert a[0] == np.float32(2.0 ** -25) and b[0] == np.float32(2.0 ** -24) and c[0] == 0.0
    assert c[-1] == np.float32(1.0) - np.float32(2.0 ** -24) and c[3] == np.float32(0.5)
    # from 2^23 on, k + 0.5 is a tie between k and k + 1 and goes to the even one
    assert a[3] == np.float32(0.5) and R.u01([0x80000100])[0] == np.float32(0.5 + 2.0 ** -23) and a[2] == np.float32(0.5 - 2.0 ** -25)
    # monotone over the whole word range (sampled), so the edges above are the extremes
    w = np.linspace(0, 0xFFFFFFFF, 100001).astype(np.uint64)
    for f in (R.u01, R.u01_open, R.u_half_open):
        assert (np.diff(f(w)) >= 0).all()
    # randn and gumbel are finite at both ends of their maps (log(1) = 0 gives radius 0; u01_open never reaches 1)
    with np.errstate(all="raise"):
        rad = np.sqrt(-2.0 * np.log(a.astype(np.float64)))
        g = -np.log(-np.log(b.astype(np.float64)))
        g32 = -np.log(-np.log(b))
    assert np.isfinite(rad).all() and rad[-1] == 0.0 and np.isfinite(g).all() and np.isfinite(g32).all()


def test_bernoulli_uniform_extremes():
    n = 4099
    u, _ = R.uniform(n, 3, 0)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert R.bernoulli(n, 0.0, 3, 0)[0].sum() == 0 and R.bernoulli(n, 1.0, 3, 0)[0].sum() == n
    half = R.bernoulli(n, 0.5, 3, 0)[0]
    assert np.array_equal(half, (u < np.float32(0.5)).astype(np.float32)) and 0.4 < half.mean() < 0.6


def test_model_draws_are_well_formed():
    """Properties of the model that do not need a GPU: ranges, the exclude rule, exact patch counts, tails are prefixes."""
    seed, off = 11, 2 ** 40 + 7
    for lo, hi in ((0, 10), (3, 4), (-5, 5), (0, 2 ** 31 - 1)):
        out, oh, rng = R.randint(1025, lo, hi, seed, off)
        assert oh is None and out.dtype == np.int64 and (out >= lo).all() and (out < hi).all() and rng == (off, off + 257)
    for span in (2, 4, 10):
        ex = np.arange(1025) % span
        ex[-3:] = span - 1                                           # the cyclic +1 wraps
        out, oh, _ = R.randint(1025, 0, span, seed, off, exclude=ex)
        assert (out != ex).all() and (out >= 0).all() and (out < span).all()
        assert np.array_equal(oh.argmax(1), out) and (oh.sum(1) == 1).all()
        plain = R.randint(1025, 0, span, seed, off)[0]
        assert np.array_equal(out, np.where(plain == ex, (plain + 1) % span, plain))
        if span == 2:
            assert np.array_equal(out, 1 - ex)
    # a shorter draw is a prefix of a longer one at the same offset (the n % 4 tail drops words, never shifts them)
    full = R.uniform(1028, seed, off)[0]
    for n in (1, 2, 3, 5, 1023, 1025):
        assert np.array_equal(R.uniform(n, seed, off)[0], full[:n])
    for total, nsel in ((16, 10), (64, 64), (64, 63), (16, 0), (16, 20), (1, 1)):
        bits, _ = R.patch_bits(300, total, nsel, seed, off)
        assert all(bin(int(b)).count("1") == min(nsel, total) for b in bits) and all(int(b) >> total == 0 for b in bits)
    m, _ = R.patch_mask(64, 30, 30, 7, 3, seed, off)
    assert m.shape == (64, 1, 30, 30) and (m[:, :, 28:, :] == 0).all() and (m[:, :, :, 28:] == 0).all()
    assert (m.reshape(64, -1).sum(1) == 3 * 49).all()
    fm, _ = R.feature_mask(257, 17, [0, 16], seed, off)
    assert (fm[:, [0, 16]] == 0).all() and 0.4 < fm[:, 1:16].mean() < 0.6
    # every patch is selected first about equally often: the partial Fisher-Yates is uniform
    first, _ = R.patch_bits(16000, 16, 1, seed, 0)
    cnt = np.bincount(np.log2(first.astype(np.float64)).astype(int), minlength=16)
    assert np.abs(cnt - 1000).max() < 5 * np.sqrt(1000 * 15 / 16)


# ---- stream bookkeeping of ops.DeviceRNG ------------------------------------------------------------------------------------
OFFSET_ARGS = {"pcg_patch_mask": (7,), "pcg_randint": (6,), "pcg_randn": (5,), "pcg_rand_gumbel": (3,), "pcg_feature_mask": (6,),
               "pcg_rand_uniform": (3,), "pcg_rand_bernoulli": (4,), "pcg_house_draws": (4, 9, 12)}


class RecordingLib:
    """Stands in for the loaded library: every entry point records its arguments and reports success."""

    def __init__(self, prototypes):
        self.calls, self._prototypes = [], prototypes

    def __getattr__(self, name):
        if name not in self._prototypes:
            raise AttributeError(name)

        def fn(*args):
            assert len(args) == len(self._prototypes[name][1]), f"{name}: {len(args)} arguments for the prototype's {len(self._prototypes[name][1])}"
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def recorded(monkeypatch):
    import pcgan_amd
    from pcgan_amd import _lib, ops
    lib = RecordingLib(_lib.PROTOTYPES)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return ops, lib


def test_device_rng_hands_out_the_ranges_the_kernels_read(recorded):
    """One DeviceRNG through every method once, sizes with n % 4 != 0: the offsets handed to the library are the running sum of
    the advances, the counter range the model reads for each call lies inside [offset, offset + advance), consecutive ranges are
    disjoint."""
    ops, lib = recorded
    seed, start = 0x9E3779B97F4A7C15, 2 ** 32 - 100
    rng = ops.DeviceRNG(seed)
    rng.offset = start
    cpu = "cpu"
    B, D, T, n = 5, 17, 7, 1023
    ex = torch.arange(n) % 4
    y = torch.arange(B) % 4
    zc = torch.tensor([0, 16], dtype=torch.int32)
    bufs = (torch.empty(B, dtype=torch.int64), torch.empty(B, D), torch.empty(B, T))
    # (method call, the model's range for a call at `off`)
    plan = [
        (lambda: rng.patch_mask(B, 28, 28, 7, 10, cpu), lambda off: R.patch_mask(B, 28, 28, 7, 10, seed, off)[-1]),
        (lambda: rng.patch_mask(3, 8, 8, 1, 64, cpu), lambda off: R.patch_mask(3, 8, 8, 1, 64, seed, off)[-1]),
        (lambda: rng.randint(0, 10, n, cpu), lambda off: R.randint(n, 0, 10, seed, off)[-1]),
        (lambda: rng.randint(0, 4, n, cpu, exclude=ex), lambda off: R.randint(n, 0, 4, seed, off, exclude=ex.numpy())[-1]),
        (lambda: rng.randn((n,), cpu), lambda off: R.randn_f64(n, 0, 1, seed, off)[-1]),
        (lambda: rng.gumbel((B, T), cpu), lambda off: R.gumbel_f64(B * T, seed, off)[-1]),
        (lambda: rng.feature_mask(B, D, cpu, zero_cols=zc), lambda off: R.feature_mask(B, D, [0, 16], seed, off)[-1]),
        (lambda: rng.rand((n, 1, 1), cpu), lambda off: R.uniform(n, seed, off)[-1]),
        (lambda: rng.bernoulli((3, 7), cpu, 0.5), lambda off: R.bernoulli(21, 0.5, seed, off)[-1]),
        (lambda: rng.house_draws(y, 4, D, T, zc, bufs), lambda off: R.house_draws(y.numpy(), 4, D, T, [0, 16], seed, off)[-1]),
        (lambda: rng.randn((2,), cpu), lambda off: R.randn_f64(2, 0, 1, seed, off)[-1]),
    ]
    expect_off, prev_hi = start, start
    for call, model_range in plan:
        before = rng.offset
        assert before == expect_off
        call()
        name, args = lib.calls[-1]
        offs = [args[i] for i in OFFSET_ARGS[name]]
        assert offs[0] == before, f"{name}: offset {offs[0]}, running sum {before}"
        advance = rng.offset - before
        lo, hi = model_range(before)
        assert before <= lo and hi <= before + advance and lo < hi, f"{name}: reads [{lo}, {hi}), was given [{before}, {before + advance})"
        assert lo >= prev_hi, f"{name}: overlaps the previous draw"
        prev_hi, expect_off = hi, before + advance
        if name == "pcg_house_draws":
            spans = [(B + 3) // 4, (B * D + 3) // 4, (B * T + 3) // 4]
            assert offs == [before, before + spans[0], before + spans[0] + spans[1]]
            assert advance == sum(spans) == ops.DeviceRNG.house_draws_span(B, D, T) == R.house_draws_span(B, D, T)
            # the three sub-draws are the separate calls at those offsets
            assert R.randint(B, 0, 4, seed, offs[0], exclude=y.numpy())[-1] == (offs[0], offs[1])
            assert R.feature_mask(B, D, None, seed, offs[1])[-1] == (offs[1], offs[2])
            assert R.gumbel_f64(B * T, seed, offs[2])[-1] == (offs[2], before + advance)
        assert args[OFFSET_ARGS[name][0] - 1 if name != "pcg_house_draws" else 13] == seed
    assert [c[0] for c in lib.calls] == ["pcg_patch_mask", "pcg_patch_mask", "pcg_randint", "pcg_randint", "pcg_randn", "pcg_rand_gumbel",
                                         "pcg_feature_mask", "pcg_rand_uniform", "pcg_rand_bernoulli", "pcg_house_draws", "pcg_randn"]
    assert start < 2 ** 32 < rng.offset                              # the stream crossed the 32-bit boundary on the way


def test_counter_form_leaves_the_host_offset_alone(recorded):
    ops, lib = recorded
    rng = ops.DeviceRNG(1)
    rng.offset = 40
    B, D, T = 5, 17, 7
    ctr = rng.device_counter("cpu")
    assert ctr.tolist() == [40, 0] and rng.device_counter("cpu", cursor=True).tolist() == [40, 0, 0, 0]
    rng.house_draws(torch.zeros(B, dtype=torch.int64), 4, D, T, None, (torch.empty(B, dtype=torch.int64), torch.empty(B, D), torch.empty(B, T)),
                    counter=ctr)
    assert lib.calls[-1][0] == "pcg_house_draws_counter" and rng.offset == 40


def test_patch_selection_stays_inside_its_sixteen_counters():
    """patch_mask advances by 16 counters per sample; at 64 selections of 64 patches the model reads b * 16 + 0 .. 15, never
    b * 16 + 16 (which is the next sample's first counter)."""
    for B in (1, 3, 300):
        _, (lo, hi) = R.patch_bits(B, 64, 64, 5, 1000)
        assert (lo, hi) == (1000, 1000 + 16 * B)
        _, (lo, hi) = R.patch_bits(B, 64, 63, 5, 1000)
        assert hi == 1000 + 16 * B
        _, (lo, hi) = R.patch_bits(B, 16, 10, 5, 1000)
        assert hi == 1000 + 16 * (B - 1) + 3
        _, (lo, hi) = R.patch_bits(B, 16, 0, 5, 1000)
        assert hi == 1000 + 16 * (B - 1) + 1                         # the first quad is drawn even when nothing is selected
    # a sample's selection depends on its own sixteen counters only: sample b of a batch is sample 0 of a draw at offset + 16 b
    bits, _ = R.patch_bits(7, 64, 64 - 3, 5, 1000)
    for b in range(7):
        assert R.patch_bits(1, 64, 61, 5, 1000 + 16 * b)[0][0] == bits[b]
