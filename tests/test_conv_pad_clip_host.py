"""CPU: the host side of the clipped forward / grad-input launches (csrc/conv_cliptab.h): the tile descriptor table of a k4 s2 p1
geometry against tap masks derived here from the geometry alone, the schedule model against the table of predicted kernel times it
was specified with, and the launch decision (pcg_conv_pad_clip_query)."""
import ctypes

import numpy as np
import pytest


def _geom(B, IH, Cin, Cout):
    from pcgan_amd import _lib
    return _lib.ConvGeom(B, IH, IH, Cin, IH // 2, IH // 2, Cout, 4, 4, 2, 1)


def _table(lib, g):
    n = lib.pcg_conv_cliptab_bytes(ctypes.byref(g))
    assert n == 5 * g.OH * g.OW * 4
    buf = np.full(n // 4 + 2, 0xDEADBEEF, dtype=np.uint32)
    assert lib.pcg_conv_cliptab_register(ctypes.byref(g), ctypes.c_void_p(buf.ctypes.data), n, None) == 0, lib.pcg_last_error().decode()
    assert (buf[-2:] == 0xDEADBEEF).all()
    return buf[:-2].reshape(5, g.OH * g.OW)


def _fields(d):
    d = int(d)
    return d & 0xFFFF, (d >> 16) & 15, (d >> 20) & 15, (d >> 24) & 15, d >> 28


def _fwd_valid(o, IH):                     # taps k of the 4-wide window whose input coordinate o*2 - 1 + k exists
    return [k for k in range(4) if 0 <= o * 2 - 1 + k < IH]


def _dgrad_valid(a, ph, OH):               # taps of input coordinate i = 2a + ph: k with (i + 1 - k) even, in ascending order -> index j
    ks = [k for k in range(4) if (2 * a + ph + 1 - k) % 2 == 0]
    return [j for j, k in enumerate(ks) if 0 <= (2 * a + ph + 1 - k) // 2 < OH]


@pytest.mark.parametrize("IH", [8, 16])
def test_table_covers_every_pixel_with_its_tap_rectangle(IH):
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _geom(128, IH, 64, 64)
    OH = g.OH
    tab = _table(lib, g)
    for section in range(5):
        seen, sizes = set(), []
        for d in tab[section]:
            pos, h0, nh, w0, nw = _fields(d)
            r, c = divmod(pos, OH)
            assert r < OH and pos not in seen
            seen.add(pos)
            if section == 0:
                vh, vw = _fwd_valid(r, IH), _fwd_valid(c, IH)
            else:
                ph, pw = divmod(section - 1, 2)
                vh, vw = _dgrad_valid(r, ph, OH), _dgrad_valid(c, pw, OH)
            # every row of a tile is this one position, so the intersection of the rows' tap masks is the position's own mask
            assert list(range(h0, h0 + nh)) == vh and list(range(w0, w0 + nw)) == vw, (section, r, c, _fields(d), vh, vw)
            sizes.append(nh * nw)
        assert len(seen) == OH * OH                      # every output (phase) pixel exactly once
        assert sizes == sorted(sizes, reverse=True)      # largest rectangle first
    full = 16 * OH * OH
    assert sum(nh * nw for _, _, nh, _, nw in map(_fields, tab[0])) / full == pytest.approx(((4 * OH - 2) / (4 * OH)) ** 2)


def test_table_is_refused_for_other_geometries():
    from pcgan_amd import _lib
    lib = _lib.load()
    for g in (_lib.ConvGeom(8, 7, 7, 64, 7, 7, 64, 3, 3, 1, 1), _lib.ConvGeom(8, 9, 9, 64, 4, 4, 64, 4, 4, 2, 1)):
        assert lib.pcg_conv_cliptab_bytes(ctypes.byref(g)) == 0
        buf = np.zeros(16, dtype=np.uint32)
        assert lib.pcg_conv_cliptab_register(ctypes.byref(g), ctypes.c_void_p(buf.ctypes.data), 64, None) == -1
        assert not buf.any()


def _classes(P, ntiles):                   # grad-input form: per phase (P-1)^2 full (4 taps), 2(P-1) half (2), 1 quarter (1) positions
    per = ntiles // (P * P)
    return [4] * ((P - 1) ** 2 * per) + [2] * (2 * (P - 1) * per) + [1] * per


def _model(lib, lens):
    a = np.asarray(lens, dtype=np.int32)
    return lib.pcg_conv_sched_model(ctypes.c_void_p(a.ctypes.data), len(a))


# (phase grid P, tiles) -> predicted kernel time clipped / unclipped: long tiles first, short tiles first, work left
MODEL_TABLE = [
    (4, 512, 1.000, 1.000, 0.766), (4, 1024, 1.000, 0.907, 0.766), (4, 2048, 0.812, 0.875, 0.766),
    (8, 1024, 1.000, 1.000, 0.879), (8, 2048, 1.000, 0.954, 0.879), (8, 4096, 0.906, 0.938, 0.879),
    (16, 8192, 0.953, 0.969, 0.938),
]


@pytest.mark.parametrize("P,tiles,long_first,short_first,work", MODEL_TABLE, ids=[f"P{r[0]}x{r[1]}" for r in MODEL_TABLE])
def test_schedule_model_reproduces_the_predicted_times(P, tiles, long_first, short_first, work):
    from pcgan_amd import _lib
    lib = _lib.load()
    c = _classes(P, tiles)
    base = _model(lib, [4] * tiles)
    assert base == pytest.approx(tiles // 512 * 4 * 3.5)          # whole rounds of two workgroups per CU
    assert sum(c) / (4 * tiles) == pytest.approx(work, abs=6e-4)
    assert _model(lib, sorted(c, reverse=True)) / base == pytest.approx(long_first, abs=6e-4)
    assert _model(lib, sorted(c)) / base == pytest.approx(short_first, abs=6e-4)


def test_schedule_model_alone_rate_and_empty():
    from pcgan_amd import _lib
    lib = _lib.load()
    assert _model(lib, [10]) == pytest.approx(22.0)               # one workgroup alone on its CU
    assert _model(lib, [10] * 257) == pytest.approx(35.0)         # CU 0 holds two
    assert lib.pcg_conv_sched_model(None, 0) == 0.0


def _query(lib, g, op, groups=1):
    taken, order, rows, pred = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_double(-1.0)
    rc = lib.pcg_conv_pad_clip_query(ctypes.byref(g), op, groups, 1, ctypes.byref(taken), ctypes.byref(order), ctypes.byref(rows), ctypes.byref(pred))
    assert rc == 0, lib.pcg_last_error().decode()
    return taken.value, order.value, rows.value, pred.value


def test_query_leaves_whole_rounds_of_equal_mix_alone():
    """512 tiles of 128 rows whose class mix is the same in every slot round (the 8<->4 grad-input at batch 512: 4 phases x 16 positions
    x 4 image blocks x 2 N tiles): no order removes a round, the launch stays today's."""
    from pcgan_amd import _lib
    lib = _lib.load()
    try:
        assert lib.pcg_tune_set(b"pad_clip", 1) == 0
        taken, _, _, pred = _query(lib, _geom(512, 8, 256, 512), 1)
        assert taken == 0 and pred > 0.95
        # not a multiple of a tile, another geometry, a thin layer, switch off: not eligible at all
        assert _query(lib, _geom(96, 8, 64, 64), 0)[0] == 0 and _query(lib, _geom(96, 8, 64, 64), 0)[3] == 1.0
        assert _query(lib, _lib.ConvGeom(128, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1), 0)[3] == 1.0
        assert _query(lib, _geom(128, 8, 1, 64), 0)[3] == 1.0
        # the same layer's forward kernel runs 512 tiles of 64 rows: sorted, an interior tile shares its CU with an edge or corner tile
        # and has it alone at the end — the model takes it (no table registered in this process: still not taken)
        d4 = _geom(512, 8, 256, 512)
        taken, order, rows, pred = _query(lib, d4, 0)
        assert (taken, order, rows) == (0, 0, 64) and pred == pytest.approx(0.907, abs=6e-4)
        assert lib.pcg_tune_set(b"pad_clip", 0) == 0
        assert _query(lib, d4, 0)[3] == 1.0
    finally:
        lib.pcg_tune_set(b"pad_clip", -1)


def test_tune_switch_is_known():
    from pcgan_amd import _lib
    lib = _lib.load()
    for v in (0, 1, -1):
        assert lib.pcg_tune_set(b"pad_clip", v) == _lib.PCG_OK
    assert lib.pcg_tune_set(b"pad_clap", 1) != _lib.PCG_OK and b"pad_clip" in lib.pcg_last_error()
