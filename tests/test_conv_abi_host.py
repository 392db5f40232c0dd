"""CPU: the struct-based ABI of the forward and grad-input convolutions (include/pcgan_hip.h: pcg_conv_args, pcg_conv2d).  The layout of
the ctypes class against the library's own sizeof, and every refusal pcg_conv2d makes before any HIP call — no device is touched: every
pointer is a fake address, and a call that got past the checks would launch on it."""
import ctypes

import pytest

FAKE = 0x1000          # a non-null, 16-byte aligned "device pointer"
S_SK = (13, 68, 196, 16, 16, 3, 3, 1, 1)        # tests/test_hip_igemm_branches.py: an MFMA layer with no 1..3-channel side
S_ODD = (13, 68, 198, 16, 16, 3, 3, 1, 1)       # MFMA, but Cout % 4 != 0: no fused statistics / column sums in the forward
S_THIN = (4, 1, 64, 16, 16, 4, 4, 2, 1)         # Cin = 1: the thin path
S_D64E = (3, 36, 68, 14, 10, 4, 4, 2, 1)        # four equal sub-pixel phases of 3 * 7 * 5 rows: no whole 128-row tiles
FWD, DGRAD = 0, 1
PCG_ERR_INVALID, PCG_ERR_WORKSPACE = -1, -2
TANH = 3


def _geom(shape):
    from pcgan_amd import _lib
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    return _lib.ConvGeom(B, H, W, Cin, (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1, Cout, KH, KW, s, p)


def _epi(name):
    from pcgan_amd import _lib
    return _lib.CONV_EPIS.index(name)


def _call(shape, op, **members):
    """pcg_conv2d on `shape` with in / w / out fake and `members` on top; returns (status, message)."""
    from pcgan_amd import _lib
    lib = _lib.load()
    a = _lib.ConvArgs(**dict(dict(op=op, in_=FAKE, w=FAKE, out=FAKE), **members))
    rc = lib.pcg_conv2d(ctypes.byref(_geom(shape)), ctypes.byref(a), None)
    return rc, lib.pcg_last_error().decode()


def _refused(shape, op, words, status=PCG_ERR_INVALID, **members):
    rc, msg = _call(shape, op, **members)
    assert rc == status and msg.startswith("pcg_conv2d:") and words in msg, (rc, msg)


def _stats(**over):
    return dict(dict(stats=1, eps=1e-5, momentum=0.1, save_mean=FAKE, save_invstd=FAKE, workspace=FAKE, workspace_bytes=1 << 30), **over)


def _bnbwd(**over):
    return dict(dict(epi=_epi("bnbwd"), z=FAKE, mean=FAKE, invstd=FAKE, gamma=FAKE, beta=FAKE, partial=FAKE, partial_bytes=1 << 30), **over)


def _bnsum(**over):
    return dict(dict(epi=_epi("add_bnsum"), addend=FAKE, z=FAKE, mean=FAKE, invstd=FAKE, sum_scale=0.1, partial=FAKE, partial_bytes=1 << 30), **over)


def _xf(scale=FAKE, shift=FAKE, act=0):
    from pcgan_amd import _lib
    return _lib.InXform(scale, shift, act, 0.2)


BOTH = pytest.mark.parametrize("op", [FWD, DGRAD], ids=["fwd", "dgrad"])


def test_struct_size_matches_the_library():
    from pcgan_amd import _lib
    assert ctypes.sizeof(_lib.ConvArgs) == _lib.load().pcg_abi_struct_bytes(b"pcg_conv_args") > 0
    assert _lib.STRUCTS["pcg_conv_args"] is _lib.ConvArgs
    assert _lib.CONV_EPIS == ("none", "mask", "add", "add_mask", "add_bnsum", "bnbwd")      # pcg_conv_epi, by value


def test_null_argument_struct_refused():
    from pcgan_amd import _lib
    lib = _lib.load()
    assert lib.pcg_conv2d(ctypes.byref(_geom(S_SK)), None, None) == PCG_ERR_INVALID
    assert lib.pcg_last_error().decode().startswith("pcg_conv2d: null argument struct")
    assert lib.pcg_conv2d(None, None, None) == PCG_ERR_INVALID                                # (the geometry's own refusal)


@BOTH
def test_all_default_struct_refused_for_the_null_operands_only(op):
    """A zero-filled struct is the plain convolution: nothing about its (absent) epilogue, statistics or groups is objected to."""
    rc, msg = _call(S_SK, op, in_=None, w=None, out=None)
    assert rc == PCG_ERR_INVALID and msg == "pcg_conv2d: null pointer (in / w / out)"
    for missing in ("in_", "w", "out"):
        _refused(S_SK, op, "null pointer (in / w / out)", **{missing: None})


def test_the_plain_conveniences_fill_the_same_struct():
    from pcgan_amd import _lib
    lib = _lib.load()
    for fn in (lib.pcg_conv2d_fwd, lib.pcg_conv2d_dgrad):
        assert fn(ctypes.byref(_geom(S_SK)), FAKE, FAKE, None, None, None, 0, None) == PCG_ERR_INVALID
        assert lib.pcg_last_error().decode() == "pcg_conv2d: null pointer (in / w / out)"


@BOTH
def test_unknown_op_activation_and_epilogue_refused(op):
    _refused(S_SK, 2, "unknown op 2")
    _refused(S_SK, op, "unknown activation 5", act=5)
    _refused(S_SK, op, "unknown activation -1", act=-1)
    _refused(S_SK, op, "unknown epilogue 6", epi=6)


@BOTH
def test_epilogue_activation_must_be_none_relu_or_leaky_relu(op):
    for members in (dict(epi=_epi("mask"), a_below=FAKE), dict(epi=_epi("add_mask"), addend=FAKE, a_below=FAKE + 16), _bnbwd()):
        _refused(S_SK, op, "epilogue activation 3 is not none / ReLU / LeakyReLU", epi_act=TANH, **members)
    # the two epilogues that have no activation of their own do not silently ignore one
    _refused(S_SK, op, "add, add_bnsum: none", epi=_epi("add"), addend=FAKE, epi_act=1)
    _refused(S_SK, op, "add, add_bnsum: none", epi_act=2, **_bnsum())


@BOTH
def test_null_and_misaligned_epilogue_tensors_refused(op):
    _refused(S_SK, op, "null pointer (the epilogue's a_below)", epi=_epi("mask"))
    _refused(S_SK, op, "null pointer (the epilogue's addend)", epi=_epi("add"))
    _refused(S_SK, op, "null pointer (the epilogue's addend)", epi=_epi("add_mask"), a_below=FAKE + 16)
    _refused(S_SK, op, "null pointer (the epilogue's z)", **_bnbwd(z=None))
    _refused(S_SK, op, "16-byte aligned", epi=_epi("mask"), a_below=FAKE + 4)
    _refused(S_SK, op, "16-byte aligned", epi=_epi("add"), addend=FAKE + 8)
    _refused(S_SK, op, "16-byte aligned", epi=_epi("add"), addend=FAKE, out=FAKE + 4)
    _refused(S_SK, op, "16-byte aligned", **_bnbwd(z=FAKE + 4))
    _refused(S_SK, op, "a_below must be a 16-byte aligned tensor", epi=_epi("add_mask"), addend=FAKE)
    _refused(S_SK, op, "a_below must be a 16-byte aligned tensor", epi=_epi("add_mask"), addend=FAKE, a_below=FAKE + 20)
    for name in ("mean", "invstd", "gamma", "beta"):
        _refused(S_SK, op, "null BatchNorm parameter", **_bnbwd(**{name: None}))
        _refused(S_SK, op, "must be 16-byte aligned", **_bnbwd(**{name: FAKE + 4}))
    for name in ("z", "mean", "invstd"):
        _refused(S_SK, op, "null BatchNorm parameter", **_bnsum(**{name: None}))
        _refused(S_SK, op, "must be 16-byte aligned", **_bnsum(**{name: FAKE + 4}))


@BOTH
def test_add_mask_refuses_the_output_as_a_below(op):
    _refused(S_SK, op, "other than the output", epi=_epi("add_mask"), addend=FAKE, a_below=FAKE)


@BOTH
def test_epilogue_on_a_thin_layer_refused(op):
    for members in (dict(epi=_epi("add"), addend=FAKE), dict(epi=_epi("add_mask"), addend=FAKE, a_below=FAKE + 16), _bnsum(), _bnbwd(),
                    dict(epi=_epi("mask"), a_below=FAKE + 16)):
        _refused(S_THIN, op, "epilogues only on MFMA layers", **members)


@BOTH
def test_statistics_refusals(op):
    _refused(S_THIN, op, "statistics only on MFMA layers", **_stats())
    _refused(S_SK, op, "null statistics output", **_stats(save_mean=None))
    _refused(S_SK, op, "null statistics output", **_stats(save_invstd=None))
    _refused(S_SK, op, "coef_out needs gamma and beta", **_stats(coef_out=FAKE))
    _refused(S_SK, op, "coef_out needs gamma and beta", **_stats(coef_out=FAKE, gamma=FAKE))


def test_statistics_and_column_sums_need_the_output_channels_in_fours():
    _refused(S_ODD, FWD, "statistics only on MFMA layers", **_stats())
    _refused(S_ODD, FWD, "not eligible for the column sums", **_bnbwd())
    _refused(S_ODD, FWD, "not eligible for the column sums", **_bnsum())
    _refused(S_ODD, DGRAD, "must be a multiple of 4", **_stats())


@BOTH
def test_short_buffers_return_the_workspace_status(op):
    from pcgan_amd import _lib
    lib = _lib.load()
    need = (lib.pcg_conv2d_dgrad_bn_workspace_bytes if op else lib.pcg_conv2d_fwd_bn_workspace_bytes)(ctypes.byref(_geom(S_SK)))
    assert need > 0
    _refused(S_SK, op, f"workspace {need - 1} B < required {need} B", PCG_ERR_WORKSPACE, **_stats(workspace_bytes=need - 1))
    _refused(S_SK, op, f"workspace {need} B < required {need} B", PCG_ERR_WORKSPACE, **_stats(workspace=None, workspace_bytes=need))
    for form in (_bnbwd, _bnsum):
        _refused(S_SK, op, f"partial-sum buffer {need - 1} B < required {need} B", PCG_ERR_WORKSPACE, **form(partial_bytes=need - 1))
        _refused(S_SK, op, "partial-sum buffer", PCG_ERR_WORKSPACE, **form(partial=None))


def test_group_refusals():
    _refused(S_SK, FWD, "13 images do not split into 2 groups of whole 128-row tiles", **_stats(groups=2))
    _refused(S_SK, FWD, "do not split into 9 groups", **_stats(groups=9))
    _refused(S_SK, DGRAD, "split into 2 groups of whole 128-row tiles", **_bnbwd(groups=2))
    _refused(S_SK, DGRAD, "split into 13 groups of whole 128-row tiles", **_bnbwd(groups=13))          # 13 > 8
    _refused(S_D64E, DGRAD, "split into 1 groups of whole 128-row tiles", **_bnbwd(groups=1))         # 105 rows per phase
    _refused(S_SK, FWD, "groups = -1", **_stats(groups=-1))


# what no retired entry offered: (op, members, words of the refusal)
def _unoffered():
    mask = dict(epi=_epi("mask"), a_below=FAKE + 16)
    return [
        ("epilogue + statistics", FWD, dict(_stats(), **mask), "an epilogue goes with no statistics"),
        ("epilogue + statistics, grad-input", DGRAD, dict(_stats(), **_bnbwd()), "an epilogue goes with no statistics"),
        ("epilogue + transform", FWD, dict(mask, xf="xf"), "an epilogue goes with no statistics, input transform"),
        ("epilogue + bias", DGRAD, dict(mask, bias=FAKE), "an epilogue goes with no statistics, input transform, bias"),
        ("epilogue + output activation", FWD, dict(mask, act=1), "bias or output activation"),
        ("statistics + output activation", FWD, _stats(act=2), "statistics go with no output activation"),
        ("groups on the plain forward", FWD, dict(groups=2), "groups = 2 goes with"),
        ("groups on the plain grad-input", DGRAD, dict(groups=1), "groups = 1 goes with"),
        ("grouped statistics of the grad-input", DGRAD, _stats(groups=1), "groups = 1 goes with"),
        ("grouped bnbwd of the forward", FWD, _bnbwd(groups=1), "groups = 1 goes with"),
        ("grouped mask", DGRAD, dict(mask, groups=1), "groups = 1 goes with"),
        ("grouped statistics + transform", FWD, _stats(groups=1, xf="xf"), "groups = 1 goes with"),
        ("grouped statistics + coef_out", FWD, _stats(groups=1, gamma=FAKE, beta=FAKE, coef_out=FAKE), "groups = 1 goes with"),
    ]


@pytest.mark.parametrize("what,op,members,words", _unoffered(), ids=[u[0] for u in _unoffered()])
def test_combinations_no_retired_entry_offered_are_refused(what, op, members, words):
    xf = _xf()                                             # (alive until the call has returned)
    if members.get("xf") == "xf":
        members = dict(members, xf=ctypes.addressof(xf))
    _refused(S_SK, op, words, **members)


@BOTH
def test_input_transform_refusals(op):
    for xf, words in ((_xf(shift=None), "input transform without shift"), (_xf(act=TANH), "input transform activation 3"),
                      (_xf(scale=FAKE + 4), "16-byte aligned scale / shift")):
        _refused(S_SK, op, words, xf=ctypes.addressof(xf))
    xf = _xf()
    _refused(S_THIN, FWD, "input transforms on the MFMA path", xf=ctypes.addressof(xf))
    _refused((4, 1, 32, 16, 16, 4, 4, 2, 1), DGRAD, "input transforms on the MFMA path", xf=ctypes.addressof(xf))     # thin, but not Cout = 64
    none = _xf(scale=None)                                 # scale == NULL: no transform, so nothing to refuse but the operands
    _refused(S_THIN, op, "null pointer (in / w / out)", xf=ctypes.addressof(none), out=None)


def test_mfma_channel_and_stride_refusals():
    _refused((4, 6, 64, 16, 16, 3, 3, 1, 1), FWD, "Cin=6")
    _refused((4, 64, 6, 16, 16, 3, 3, 1, 1), DGRAD, "Cout=6")
    _refused((4, 64, 64, 16, 16, 3, 3, 3, 1), DGRAD, "grad-input stride 3 > 2 unsupported")
