"""CPU: the pad_clip_dgrad switch of pcg_tune_set (csrc/conv_igemm.hip) — known by name, named in the error text, and the gate it
puts on the grad-input answer of pcg_conv_pad_clip_query (no table is registered in this process, so nothing is ever `taken`; the
predicted ratio shows which plan was consulted: exactly 1.0 is "not eligible")."""
import ctypes


def _query(lib, g, op):
    taken, order, rows, pred = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_double(-1.0)
    rc = lib.pcg_conv_pad_clip_query(ctypes.byref(g), op, 1, 1, ctypes.byref(taken), ctypes.byref(order), ctypes.byref(rows), ctypes.byref(pred))
    assert rc == 0, lib.pcg_last_error().decode()
    return taken.value, order.value, rows.value, pred.value


def test_switch_is_known_and_named_in_the_error_text():
    from pcgan_amd import _lib
    lib = _lib.load()
    for v in (0, 1, 2, -1):
        assert lib.pcg_tune_set(b"pad_clip_dgrad", v) == _lib.PCG_OK
    for v in (3, -2):                                               # out of range: refused, the setting stays
        assert lib.pcg_tune_set(b"pad_clip_dgrad", v) != _lib.PCG_OK and b"pad_clip_dgrad" in lib.pcg_last_error()
    assert lib.pcg_tune_set(b"pad_clip_dgrid", 1) != _lib.PCG_OK and b"pad_clip_dgrad" in lib.pcg_last_error()


def test_switch_0_gates_the_model_taken_grad_input_only():
    from pcgan_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(2048, 8, 8, 256, 4, 4, 512, 4, 4, 2, 1)       # 2048 tiles of 128 rows: the model's best 8 <-> 4 case (long first 0.812)
    try:
        assert lib.pcg_tune_set(b"pad_clip", 1) == 0
        on_d, on_f = _query(lib, g, 1), _query(lib, g, 0)
        assert on_d[2] == 128                                       # planned: the plan's tile height is reported
        assert lib.pcg_tune_set(b"pad_clip_dgrad", 0) == 0
        assert _query(lib, g, 1) == (0, 0, 0, 1.0)                  # grad-input: not eligible
        assert _query(lib, g, 0) == on_f                            # forward: unchanged
        assert lib.pcg_tune_set(b"pad_clip", 3) == 0                # forced modes measure the kernel itself: not gated
        assert _query(lib, g, 1)[3] != 1.0
    finally:
        lib.pcg_tune_set(b"pad_clip_dgrad", -1)
        lib.pcg_tune_set(b"pad_clip", -1)
