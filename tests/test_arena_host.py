"""CPU: tests/arena.py catches what it claims to.  The "kernels" here are torch CPU ops that write through as_strided on the arena's
underlying buffer — one float before the payload, one after it, a 128-row tile past the end, an output element skipped, a guard value
multiplied by zero into the output — and every one of them must fail Arena.check() with the right tensor, side and offset.  Then
exact_scratch (exact sizes, refilled, restored, a non-null zero-byte request) and the arena bytes of every case table that
tests/test_hip_arena.py runs, from the geometry and the library's size queries (the library loads without a device)."""
import pytest
import torch

import arena as A

CPU = torch.device("cpu")


def _raw_f32(ar, t):
    """(float32 view of the whole allocation behind arena tensor t, index of the payload's first float in it)"""
    blk = ar.block_of(t)
    assert blk.start % 4 == 0 and blk.raw.numel() % 4 == 0
    return blk.raw.view(torch.float32), blk.start // 4


def _fake_store(ar, t, first, count, value=1.0):
    """The fake kernel: `count` floats stored from float index `first` relative to the payload (negative: before it)."""
    raw, p0 = _raw_f32(ar, t)
    torch.as_strided(raw, (count,), (1,), p0 + first).fill_(value)


# ---- layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [((3, 11, 7, 20), torch.float32), ((5,), torch.float32), ((2, 1024), torch.float32), ((70001,), torch.float32),
                                         ((7, 3), torch.float64), ((9,), torch.int32), ((1,), torch.int64), ((4, 33), torch.uint8)])
def test_payload_alignment_guard_size_and_fill(shape, dtype):
    ar = A.Arena(CPU)
    t = ar.output(shape, dtype)
    blk = ar.block_of(t)
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 256 == 16                                      # the ABI's 16 bytes and nothing better
    item = t.element_size()
    guard = A.guard_for(shape, item)
    rule = max(64 * 1024, 2 * 128 * shape[-1] * item) if len(shape) > 1 else 64 * 1024     # vectors and scratch: 64 KiB
    assert guard % 256 == 0 and rule <= guard < rule + 256
    assert blk.start >= guard and blk.raw.numel() - blk.start - blk.nbytes >= guard
    assert blk.raw.numel() <= A.arena_bytes(shape, dtype)
    assert bool((blk.raw == 0xFF).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())                                 # 0xFF bytes: float32 NaN, float64 NaN
    elif dtype != torch.uint8:
        assert bool((t == -1).all())                                      # ... and int32 / int64 -1
    src = torch.arange(t.numel(), dtype=torch.float64).reshape(shape).to(dtype)
    x = ar.input(src)
    assert torch.equal(x, src) and x.data_ptr() % 256 == 16
    y = ar.inout(src)
    assert torch.equal(y, src) and y.data_ptr() != x.data_ptr()
    t.copy_(src)
    ar.check()


def test_guard_rule_values():
    assert A.guard_bytes(1, 1) == 64 * 1024                               # scratch and vectors
    assert A.guard_bytes(64, 4) == 64 * 1024                              # 2 x 128 x 256 B = 64 KiB
    assert A.guard_bytes(260, 4) == 2 * 128 * 260 * 4
    assert A.guard_bytes(65, 4) == 66560 and 66560 % 256 == 0
    assert A.guard_bytes(33, 8) == (2 * 128 * 33 * 8 + 255) // 256 * 256


# ---- oversteps -------------------------------------------------------------------------------------------------------------------
ROWS, C = 150, 20          # a [150, 20] float32 output: rows of 80 bytes, a ragged second 128-row tile


def _clean_output(ar, name="y"):
    y = ar.output((ROWS, C), name=name)
    y.copy_(torch.randn(ROWS, C))
    return y


def test_one_float_before_the_payload_is_reported():
    ar = A.Arena(CPU)
    ar.input(torch.randn(8), name="x")
    y = _clean_output(ar)
    ar.check()
    _fake_store(ar, y, -1, 1)
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    assert "y (output): guard BEFORE the payload overwritten: 4 bytes changed, first at payload offset -4, last at -1" in msg, msg
    assert "AFTER" not in msg and "x (input)" not in msg


def test_one_float_after_the_payload_is_reported():
    ar = A.Arena(CPU)
    ar.input(torch.randn(8), name="x")
    y = _clean_output(ar)
    _fake_store(ar, y, ROWS * C, 1)
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    nbytes = ROWS * C * 4
    assert (f"y (output): guard AFTER the payload overwritten: 4 bytes changed, first at payload offset {nbytes}, last at {nbytes + 3} "
            f"(payload is {nbytes} bytes)") in msg, msg
    assert "BEFORE" not in msg and "x (input)" not in msg


def test_one_tile_of_128_rows_past_the_end_is_reported():
    """A ragged tile kernel without its row bound stores rows 128 .. 255 of the second tile: 106 rows beyond the 150 there are."""
    ar = A.Arena(CPU)
    w = ar.inout(torch.randn(4, 4), name="dw")
    y = _clean_output(ar)
    _fake_store(ar, y, 128 * C, 128 * C, value=2.0)
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    nbytes, end = ROWS * C * 4, 256 * C * 4
    assert (f"y (output): guard AFTER the payload overwritten: {end - nbytes} bytes changed, first at payload offset {nbytes}, last at "
            f"{end - 1} ") in msg, msg
    assert "dw (inout)" not in msg and "BEFORE" not in msg
    assert 256 * C * 4 - nbytes <= A.guard_bytes(C, 4)                  # the whole overstep lies inside the guard: the rule's point
    assert torch.isfinite(w).all()


def test_overstep_into_an_input_and_a_scratch_guard_names_them():
    ar = A.Arena(CPU)
    x = ar.input(torch.randn(6, 8), name="x")
    s = ar.scratch(1000, name="ws")
    _fake_store(ar, x, -2, 1)
    blk = ar.block_of(s)
    blk.raw[blk.start + 1000] = 0
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    assert "x (input): guard BEFORE the payload overwritten" in msg and "first at payload offset -8, " in msg
    assert "ws (scratch): guard AFTER the payload overwritten: 1 bytes changed, first at payload offset 1000, last at 1000" in msg


def test_a_skipped_output_element_is_reported():
    ar = A.Arena(CPU)
    y = ar.output((ROWS, C), name="y")
    src = torch.randn(ROWS, C)
    flat = y.view(-1)
    flat[:777].copy_(src.view(-1)[:777])                                 # the fake kernel stores everything but element 777
    flat[778:].copy_(src.view(-1)[778:])
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    assert f"y (output): 1 of {ROWS * C} elements hold the fill pattern (never written, or a NaN that came out of a guard), first at flat index 777, last at 777" in msg
    assert "overwritten" not in msg
    flat[777] = 0.0
    ar.check()


def test_zero_times_a_guard_value_is_flagged():
    """A loader that reads one element past the operand and masks it with a multiplication by zero: 0 x NaN = NaN in the output."""
    ar = A.Arena(CPU)
    n = 96
    x = ar.input(torch.randn(n), name="x")
    y = ar.output((n,), name="y")
    raw, p0 = _raw_f32(ar, x)
    loaded = torch.as_strided(raw, (n + 1,), (1,), p0)                   # one float too many: the last one is guard
    mask = torch.ones(n + 1)
    mask[n] = 0.0
    prod = loaded * mask                                                 # a select would give 0 here
    y.copy_(prod[:n])
    y[n - 1] += prod[n]                                                  # the K-tail sum
    with pytest.raises(AssertionError) as e:
        ar.check()
    # 0 x NaN keeps the guard's NaN payload, so the element may still be the fill pattern bit for bit: either line names element n - 1
    assert (f"y (output): 1 of {n} elements hold the fill pattern (never written, or a NaN that came out of a guard), first at flat index "
            f"{n - 1}, last at {n - 1}") in str(e.value) or f"y (output): 1 of {n} elements are not finite, first at flat index {n - 1}" in str(e.value)
    assert not bool(torch.isfinite(y[n - 1]))
    assert "overwritten" not in str(e.value)                             # nothing was stored outside: only the value gives it away
    y[n - 1] = torch.where(mask[n] != 0, loaded[n], torch.zeros(())) + prod[n - 1]
    ar.check()


def test_non_finite_inout_is_flagged_and_inputs_are_not_judged():
    ar = A.Arena(CPU)
    ar.input(torch.tensor([float("inf"), 1.0]), name="x")                # an input may hold anything
    rv = ar.inout(torch.ones(5), name="running_var")
    ar.check()
    rv[3] = float("nan")
    with pytest.raises(AssertionError, match=r"running_var \(inout\): 1 of 5 elements are not finite, first at flat index 3"):
        ar.check()


# ---- exact scratch ---------------------------------------------------------------------------------------------------------------
def test_exact_scratch_sizes_refill_zero_bytes_and_restore():
    from pcgan_amd import ops
    before = ops._scratch
    ar = A.Arena(CPU)
    with pytest.MonkeyPatch.context() as mp:
        log = A.exact_scratch(mp, ar)
        assert ops._scratch is not before
        a = ops.workspace(4000, CPU)
        assert a.dtype == torch.uint8 and a.numel() == 4000 and a.data_ptr() % 256 == 16 and bool((a == 0xFF).all())
        a.fill_(7)                                                       # a kernel leaves plausible numbers behind
        b = ops.workspace(4000, CPU)                                     # the next request does not see them
        assert b.numel() == 4000 and b.data_ptr() != a.data_ptr() and bool((b == 0xFF).all())
        c = ops.workspace2(12, CPU)
        assert c.numel() == 12
        z = ops.workspace(0, CPU)
        assert z.numel() == 0 and z.data_ptr() != 0 and z.data_ptr() % 256 == 16
        d = ops._scratch(17, 1 << 20, CPU)
        assert d.numel() == 1 << 20
        assert [(r.kind, r.nbytes, r.changed) for r in log] == [(0, 4000, True), (0, 4000, False), (2, 12, False), (0, 0, False),
                                                                (17, 1 << 20, False)]
        ar.check()                                                       # registered: a write past the 12 bytes is found
        blk = ar.blocks[2]
        blk.raw[blk.start + 12] = 1
        with pytest.raises(AssertionError, match=r"scratch request 2 \(kind 2, 12 bytes\) \(scratch\): guard AFTER the payload overwritten: "
                                                 r"1 bytes changed, first at payload offset 12, last at 12"):
            ar.check()
    assert ops._scratch is before


# ---- the arena bytes of the device cases -----------------------------------------------------------------------------------------
def test_every_device_case_fits_in_2_gib():
    import test_hip_arena as T
    rows = list(T.case_arena_bytes())
    families = {f for f, _, _ in rows}
    assert families == set(T.FAMILY_SIZES), families ^ set(T.FAMILY_SIZES)
    for fam, want in T.FAMILY_SIZES.items():
        assert sum(1 for f, _, _ in rows if f == fam) == want(), fam
    worst = max(rows, key=lambda r: r[2])
    print(f"{len(rows)} cases, largest: {worst[0]} {worst[1]}: {worst[2] / 2 ** 20:.1f} MiB; sum {sum(r[2] for r in rows) / 2 ** 30:.2f} GiB")
    for fam, cid, nbytes in rows:
        assert 0 < nbytes <= 2 ** 31, f"{fam} {cid}: {nbytes} bytes"
