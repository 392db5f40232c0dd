"""CPU: the host builder of a geometry's pixel descriptor table (csrc/conv_pixtab.h, pcg_conv_pixtab_register with a host buffer
only) against a brute-force loop over (oh, ow, kh, kw).  Offsets and masks must be exactly equal; the 7 tail entries continue into
the next images (entry r >= OH*OW = entry r % (OH*OW) moved by r // (OH*OW) images)."""
import ctypes

import numpy as np
import pytest

# IH(=IW), k, stride, pad, Cin
GEOMS = [(8, 4, 2, 1, 32), (16, 4, 2, 1, 128), (64, 4, 2, 1, 4), (7, 3, 1, 1, 64), (28, 3, 1, 1, 64), (7, 3, 2, 1, 16), (4, 4, 1, 0, 512)]
TAIL = 7


def _table(lib, g):
    n = lib.pcg_conv_pixtab_bytes(ctypes.byref(g))
    assert n == (g.OH * g.OW + TAIL) * 8
    buf = np.full(n // 4 + 2, 0xDEADBEEF, dtype=np.uint32)          # two guard words behind the table
    rc = lib.pcg_conv_pixtab_register(ctypes.byref(g), ctypes.c_void_p(buf.ctypes.data), n, None)
    assert rc == 0, lib.pcg_last_error().decode()
    assert (buf[-2:] == 0xDEADBEEF).all()
    t = buf[:-2].reshape(-1, 2)
    return t[:, 0].astype(np.uint32).view(np.int32).astype(np.int64), t[:, 1].astype(np.int64)


@pytest.mark.parametrize("H,k,s,p,Cin", GEOMS, ids=[f"k{k}s{s}p{p}@{H}" for H, k, s, p, _ in GEOMS])
def test_table_matches_brute_force(H, k, s, p, Cin):
    from pcgan_amd import _lib
    lib = _lib.load()
    OH = (H + 2 * p - k) // s + 1
    g = _lib.ConvGeom(3, H, H, Cin, OH, OH, 8, k, k, s, p)
    off, mask = _table(lib, g)
    assert {(8, 4): 4, (16, 4): 8, (64, 4): 32, (28, 3): 28, (4, 4): 1}.get((H, k), OH) == OH
    for r in range(OH * OH + TAIL):
        img, rr = divmod(r, OH * OH)
        oh, ow = divmod(rr, OH)
        want_mask = 0
        for kh in range(k):
            for kw in range(k):
                ih, iw = oh * s - p + kh, ow * s - p + kw
                if 0 <= ih < H and 0 <= iw < H:
                    want_mask |= 1 << (kh * k + kw)
        want_off = img * H * H * Cin * 4 + ((oh * s - p) * H + (ow * s - p)) * Cin * 4
        assert off[r] == want_off, (r, oh, ow, off[r], want_off)
        assert mask[r] == want_mask, (r, oh, ow, hex(mask[r]), hex(want_mask))
    if p > 0:
        assert off[0] < 0                        # the padded corner starts in front of the image


def test_short_buffer_and_bad_geometry_are_refused():
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(2, 8, 8, 32, 4, 4, 32, 4, 4, 2, 1)
    n = lib.pcg_conv_pixtab_bytes(ctypes.byref(g))
    buf = np.zeros(n // 4, dtype=np.uint32)
    assert lib.pcg_conv_pixtab_register(ctypes.byref(g), ctypes.c_void_p(buf.ctypes.data), n - 8, None) == -1
    assert not buf.any()
    bad = _lib.ConvGeom(2, 8, 8, 32, 5, 4, 32, 4, 4, 2, 1)          # OH inconsistent
    assert lib.pcg_conv_pixtab_bytes(ctypes.byref(bad)) == 0
    assert lib.pcg_conv_pixtab_register(ctypes.byref(bad), ctypes.c_void_p(buf.ctypes.data), n, None) == -1


def test_switch_is_accepted():
    from pcgan_amd import _lib
    lib = _lib.load()
    try:
        for v in (0, 1):
            assert lib.pcg_tune_set(b"wgrad_pixtab", v) == _lib.PCG_OK
    finally:
        assert lib.pcg_tune_set(b"wgrad_pixtab", -1) == _lib.PCG_OK
