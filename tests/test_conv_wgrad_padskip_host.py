"""CPU: the padding skip of the weight gradients (csrc/igemm_core.h PadSkip) without a GPU — which launches
pcg_conv_wgrad_padskip_query says have the skipping consumers and which share of their MFMAs those leave out, and the wgrad_padskip
switch of pcg_tune_set: its name, its range and its place in the unknown-switch error text.

The fractions follow from the geometry alone.  k4 s2 p1, k = output position, MFMA t of a k-group takes positions {q + t, q + 4 + t}:
OW = 4 — both have ow = t, so one MFMA in four is padding for the taps kw = 0 and kw = 3 (half the taps): 1/4 * 1/2 = 0.125; OW = 8 and
16 — a k-group lies in one output row and is padding for kh = 0 at oh = 0 and kh = 3 at oh = OH - 1: 1/OH * 1/2 = 0.0625 and 0.03125."""
import ctypes

import pytest

WGRAD = 2


def _query(lib, g, op=WGRAD):
    applies, frac = ctypes.c_int32(-1), ctypes.c_double(-1.0)
    rc = lib.pcg_conv_wgrad_padskip_query(ctypes.byref(g), op, ctypes.byref(applies), ctypes.byref(frac))
    assert rc == 0, lib.pcg_last_error().decode()
    return applies.value, frac.value


# the three layer classes of the DCGAN step at batch 512 (D4 / G2, D3 / G3, D2 / G4) and the smallest shapes of the GPU test
@pytest.mark.parametrize("B,H,Cin,Cout,want", [
    (512, 8, 256, 512, 0.125), (512, 16, 128, 256, 0.0625), (512, 32, 64, 128, 0.03125),
    (8, 8, 64, 64, 0.125), (12, 16, 128, 96, 0.0625), (8, 32, 64, 96, 0.03125),
])
def test_fraction_of_the_three_layer_classes(B, H, Cin, Cout, want):
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(B, H, H, Cin, H // 2, H // 2, Cout, 4, 4, 2, 1)
    assert _query(lib, g) == (1, want)
    assert _query(lib, g, 0) == (0, 0.0) and _query(lib, g, 1) == (0, 0.0)      # forward and grad-input kernels: not this skip


def test_ineligible_geometries_report_zero():
    from pcgan_amd import _lib
    lib = _lib.load()
    cases = {
        "3x3 stride 1": _lib.ConvGeom(64, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1),
        "k4 s2 p1, OH = 2": _lib.ConvGeom(64, 4, 4, 128, 2, 2, 128, 4, 4, 2, 1),
        "OW = 6: no power of two": _lib.ConvGeom(64, 8, 12, 128, 4, 6, 128, 4, 4, 2, 1),
        "OH = OW = 7 (14 -> 7)": _lib.ConvGeom(64, 14, 14, 64, 7, 7, 128, 4, 4, 2, 1),
        "k4 s2 p0": _lib.ConvGeom(64, 10, 10, 64, 4, 4, 128, 4, 4, 2, 0),
        "Cin = 32: a wave tile spans two taps": _lib.ConvGeom(64, 16, 16, 32, 8, 8, 64, 4, 4, 2, 1),
        "thin: Cin = 1": _lib.ConvGeom(64, 64, 64, 1, 32, 32, 64, 4, 4, 2, 1),
    }
    for name, g in cases.items():
        assert _query(lib, g) == (0, 0.0), name


def test_bf16_mode_reports_zero():
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(512, 16, 16, 128, 8, 8, 256, 4, 4, 2, 1)
    assert _query(lib, g) == (1, 0.0625)
    try:
        assert lib.pcg_conv_precision_set(1) == _lib.PCG_OK
        assert _query(lib, g) == (0, 0.0)
    finally:
        lib.pcg_conv_precision_set(0)
    assert _query(lib, g) == (1, 0.0625)


def test_query_does_not_depend_on_the_switch_and_refuses_a_bad_op():
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(512, 8, 8, 256, 4, 4, 512, 4, 4, 2, 1)
    try:
        for v in (0, 1, 2, 3):
            assert lib.pcg_tune_set(b"wgrad_padskip", v) == _lib.PCG_OK
            assert _query(lib, g) == (1, 0.125)
    finally:
        lib.pcg_tune_set(b"wgrad_padskip", -1)
    assert lib.pcg_conv_wgrad_padskip_query(ctypes.byref(g), 3, None, None) != _lib.PCG_OK
    assert b"pcg_conv_wgrad_padskip_query" in lib.pcg_last_error()
    assert lib.pcg_conv_wgrad_padskip_query(ctypes.byref(g), WGRAD, None, None) == _lib.PCG_OK     # outputs may be NULL


def test_switch_name_range_and_error_text():
    from pcgan_amd import _lib
    lib = _lib.load()
    try:
        for v in (0, 1, 2, 3, -1):
            assert lib.pcg_tune_set(b"wgrad_padskip", v) == _lib.PCG_OK
        for v in (4, -2):                                           # out of range: refused, and the message names the switch
            assert lib.pcg_tune_set(b"wgrad_padskip", v) != _lib.PCG_OK and b"wgrad_padskip" in lib.pcg_last_error()
    finally:
        lib.pcg_tune_set(b"wgrad_padskip", -1)
    assert lib.pcg_tune_set(b"wgrad_padskid", 1) != _lib.PCG_OK
    msg = lib.pcg_last_error().decode()
    assert "unknown switch 'wgrad_padskid'" in msg and "wgrad_padskip" in msg and "pad_clip_dgrad" in msg


def _plan(lib, g, assume_scratch=1):
    mode, bit = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.pcg_conv_wgrad_padskip_plan(ctypes.byref(g), assume_scratch, ctypes.byref(mode), ctypes.byref(bit))
    assert rc == 0, lib.pcg_last_error().decode()
    return mode.value, bit.value


# The bits follow from today's block orders.  D4: 512 stream-K ranges, range g = (b & 7) * 64 + (b >> 3), tile g / 4, two
# tiles per tap: b ^ 64 moves the tile by 2, i.e. kw by 1.  D3: tile-major, tile = (x & 7) * 4 + (x >> 3), four tiles per tap row: b ^ 1
# moves the tile by 4, i.e. kh by 1.  D2: slice-major, tile = (b >> 3) & 7, two tiles per tap row: b ^ 16 moves the tile by 2, i.e. kh by 1.
@pytest.mark.parametrize("B", [512, 1024])
@pytest.mark.parametrize("H,Cin,Cout,default,every", [(8, 256, 512, (2, 64), (2, 64)), (16, 128, 256, (2, 1), (2, 1)),
                                                       (32, 64, 128, (0, 0), (2, 16))])
def test_plan_of_the_three_layer_classes(B, H, Cin, Cout, default, every):
    """Switch 1 (and the built-in default): the paired skip with a non-zero bit for OW = 4 and 8, today's kernel for OW = 16; 2: every
    class paired; 3: every class skipping in today's order; 0: today's kernels."""
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(B, H, H, Cin, H // 2, H // 2, Cout, 4, 4, 2, 1)
    try:
        assert _plan(lib, g) == default
        for v, want in ((0, (0, 0)), (1, default), (2, every), (3, (1, 0))):
            assert lib.pcg_tune_set(b"wgrad_padskip", v) == _lib.PCG_OK
            assert _plan(lib, g) == want, v
        assert lib.pcg_conv_precision_set(1) == _lib.PCG_OK             # the bf16 twins launch what they always did
        assert _plan(lib, g) == (0, 0)
    finally:
        lib.pcg_conv_precision_set(0)
        lib.pcg_tune_set(b"wgrad_padskip", -1)


def test_plan_of_small_and_ineligible_launches():
    from pcgan_amd import _lib
    lib = _lib.load()
    assert _plan(lib, _lib.ConvGeom(8, 16, 16, 64, 8, 8, 64, 4, 4, 2, 1)) == (2, 0)       # fewer than two rounds of 256 blocks: no bit
    assert _plan(lib, _lib.ConvGeom(64, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1)) == (0, 0)
    assert _plan(lib, _lib.ConvGeom(64, 16, 16, 32, 8, 8, 64, 4, 4, 2, 1)) == (0, 0)
    g = _lib.ConvGeom(8, 16, 16, 64, 8, 8, 64, 4, 4, 2, 1)
    assert lib.pcg_conv_wgrad_padskip_plan(ctypes.byref(g), 1, None, None) == _lib.PCG_OK
