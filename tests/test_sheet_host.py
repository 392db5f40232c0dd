"""CPU: the host half of the image sheets.  The restatement of make_grid / save_image (tests/sheet_restate.py) against a
grid written out by hand and against the reference's own recorded PNGs (tests/golden/sheets_ref.npz, written by
tests/golden/make_golden_sheets.py); _cfeval.write_png_rgb through a PNG decode written here; the header declares the entries of
csrc/image_sheet.hip and the built library exports them."""
import ctypes
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sheet_restate as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcg_image_range_workspace_bytes", "pcg_image_range", "pcg_image_sheet")
# key -> (images, nrow): 122 = 4 * 30 + 2, 152 = 5 * 30 + 2
RECORDED = {"countergan.original": (16, 4), "countergan.counterfactual": (16, 4), "countergan.delta": (16, 4), "mnist_gan.epoch1": (25, 5)}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "sheets_ref.npz")))


def test_literal_layout():
    """Two 1 x 2 images, padding 1, pad_value 0.5: cells of 2 x 3 behind a border of 1 -> [3, 3, 7]."""
    t = torch.tensor([[[[0.0, 1.0]]], [[[0.25, 0.75]]]])
    p = 0.5
    plane = [[p, p, p, p, p, p, p],
             [p, 0.0, 1.0, p, 0.25, 0.75, p],
             [p, p, p, p, p, p, p]]
    g = SR.make_grid(t, padding=1, pad_value=0.5)
    assert g.shape == (3, 3, 7) and g.tolist() == [plane, plane, plane]
    u = SR.to_u8(g)
    assert u.shape == (3, 7, 3) and u[:, :, 0].tolist() == [[128] * 7, [128, 0, 255, 128, 64, 191, 128], [128] * 7]
    # nrow 1: one column, two rows of cells; a single image is its own grid
    g1 = SR.make_grid(t, nrow=1, padding=1, pad_value=0.5)
    assert g1.shape == (3, 5, 4) and g1[0].tolist() == [[p] * 4, [p, 0.0, 1.0, p], [p] * 4, [p, 0.25, 0.75, p], [p] * 4]
    assert SR.make_grid(t[:1], padding=1, pad_value=0.5).tolist() == [[[0.0, 1.0]]] * 3
    # normalize: 2 * x + 0.25 has the global range [0.25, 2.25], d = 2
    n = SR.make_grid(t, padding=0, normalize=True, pre=(2.0, 0.25))
    assert n[0].tolist() == [[0.0, 1.0, 0.25, 0.75]]
    c = SR.make_grid(t, padding=0, normalize=True, value_range=(0.25, 0.75))
    assert c[0].tolist() == [[0.0, 1.0, 0.0, 1.0]]
    assert SR.make_grid(torch.full((2, 1, 1, 1), 3.0), padding=0, normalize=True).tolist() == [[[0.0, 0.0]]] * 3      # d = 1e-5


def test_the_division_is_not_a_reciprocal_product():
    """The restatement divides: it equals NumPy's fp32 division, and a tensor exists on which the reciprocal form differs."""
    g = torch.Generator().manual_seed(5)
    t = torch.randn((4, 1, 6, 6), generator=g)
    lo, hi = float(t.min()), float(t.max())
    d = np.float32(max(hi - lo, 1e-5))
    want = (np.clip(t.numpy(), np.float32(lo), np.float32(hi)) - np.float32(lo)) / d
    got = SR.make_grid(t, padding=0, nrow=4, normalize=True)[0].numpy()
    assert np.array_equal(got.reshape(6, 4, 6).transpose(1, 0, 2).reshape(4, 1, 6, 6), want)
    assert not np.array_equal(want, (t.numpy() - np.float32(lo)) * (np.float32(1.0) / d))


def test_reference_pin(gold):
    """The sixteen cells of the recorded original.png, mapped back to [-1, 1], give the recorded sheet again: lo = -1, hi = 1."""
    rec = gold["countergan.original"]
    cells = SR.cells(rec, 16, 4, 28, 28)
    x = torch.from_numpy((cells.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).view(16, 1, 28, 28)
    assert float(x.min()) == -1.0 and float(x.max()) == 1.0
    got = SR.sheet_u8(x, nrow=4, normalize=True)
    assert got.shape == (122, 122, 3) and np.array_equal(got.numpy(), rec)


@pytest.mark.parametrize("key", sorted(RECORDED))
def test_recorded_sheets(gold, key):
    n, nrow = RECORDED[key]
    rec = gold[key]
    side = nrow * 30 + 2
    assert rec.shape == (side, side, 3) and rec.dtype == np.uint8
    assert np.array_equal(rec[:, :, 0], rec[:, :, 1]) and np.array_equal(rec[:, :, 0], rec[:, :, 2])
    assert not rec[SR.padding_mask(n, nrow, 28, 28)].any()
    assert rec.max() == 255                                                   # normalize=True: the maximum maps to 1


def _decode_png(path):
    """(width, height, bit depth, colour type, the rows without their filter bytes) of a PNG whose rows all use filter 0."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, filt, lace) == (0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, -1)
    assert not raw[:, 0].any()
    return w, h, depth, colour, raw[:, 1:]


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (122, 122, 3)])
def test_write_png_rgb_round_trips(tmp_path, shape):
    from pcgan_amd import _cfeval
    a = np.random.RandomState(shape[1]).randint(0, 256, shape).astype(np.uint8)
    a.flat[0], a.flat[-1] = 255, 0
    path = str(tmp_path / "sub" / "s.png")
    _cfeval.write_png_rgb(path, a)
    w, h, depth, colour, rows = _decode_png(path)
    assert (w, h, depth, colour) == (shape[1], shape[0], 8, 2)
    np.testing.assert_array_equal(rows.reshape(shape), a)
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        np.testing.assert_array_equal(np.asarray(im), a)
    for bad in (a[:, :, 0], a.astype(np.float32), a[:, :, :2]):
        with pytest.raises(_cfeval.PcgError):
            _cfeval.write_png_rgb(path, bad)


def test_header_declares_and_library_exports_the_sheet_entries():
    import pcgan_amd
    from pcgan_amd import _lib, sheets
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcgan_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcg_[a-z0-9_]+)\s*\(", text))
    lib = pcgan_amd.load()
    raw = ctypes.CDLL(pcgan_amd.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in pcgan_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by libpcgan_hip.so"
        assert name in _lib.PROTOTYPES
    assert lib.pcg_abi_version() == 7
    assert lib.pcg_abi_struct_bytes(b"pcg_image_sheet_args") == ctypes.sizeof(_lib.ImageSheetArgs) > 0
    assert lib.pcg_image_range_workspace_bytes() >= 16 + 8
    assert pcgan_amd.sheets is sheets and "sheets" in pcgan_amd.__all__
    assert sheets.grid_shape(64, 64, 64) == (530, 530) and sheets.grid_shape(16, 28, 28, nrow=4) == (122, 122)
    assert sheets.grid_shape(1, 28, 28) == (28, 28) and sheets.grid_shape(5, 28, 28, nrow=4) == (62, 122)


def test_sheets_refuse_the_host():
    from pcgan_amd import PcgError, sheets
    t = torch.zeros(2, 1, 4, 4)
    for call in (lambda: sheets.make_grid(t), lambda: sheets.sheet_u8(t), lambda: sheets.image_range(t), lambda: sheets.save_image(t, "x.png")):
        with pytest.raises(PcgError):
            call()
