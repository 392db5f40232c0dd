"""GPU parity of the implicit-GEMM convolutions (csrc/conv_igemm.hip, igemm_core.h, conv_loaders.h) against float64, form by form.

The host planners (plan_fwd, fwd_use_t64, plan_sk_shape, plan_skn_shape, dgrad_as_gemm, build_phases, plan_wgrad) and the eleven
pcg_tune_set switches choose among ~20 kernel forms per launch, each with an fp32 and a bf16 twin; one epilogue (igemm_store_tile) applies
the output modes to all of them.  Every case of CASES is picked from those predicates to reach one form (its id names it) and asserts
that form through pcg_conv_plan_describe before it runs, so a planner change that moves a case elsewhere fails the case instead of
quietly testing something else.  The forms the describe string does not name carry a comment citing the predicate that selects them.
CASES is checked on the CPU as well (tests/test_host_logic.py::test_igemm_branch_cases_reach_their_forms).

Inputs are randn rounded to float32 (the reference sees exactly the kernel's operands), biases are nonzero on both sides.
Tolerance: the bound of test_hip_ops.py, |err| <= 2e-6 * sqrt(K) * scale + 1e-6, K the true length of the dot product (taps x Cin for
the forward, taps x Cout for the grad-input, B*OH*OW for the weight gradient), scale 4 for the forward / grad-input and 8 for the
weight gradient.  The bf16 twins (ops.conv_precision("bf16")) use test_hip_conv_bf16.py's bound against float64 of the bf16-rounded
operands and must be at least 10x that bound away from float64 of the unrounded ones.
"""
import contextlib
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
FWD, DGRAD, WGRAD = 0, 1, 2
SWITCHES = ("korder", "edge_prio", "dgrad_swz3", "wgrad_rounds", "wgrad_order", "dgrad_interleave", "fwd_splits", "stream_k",
            "sk_blocks", "dgrad_gemm", "t64")
U = 2.0 ** -24
SK = {"stream_k": 2}      # stream-K wherever the form is valid (sk_mode 2)

# (B, Cin, Cout, H, W, KH, KW, stride, pad)
S_FWD64 = (3, 36, 20, 11, 7, 3, 3, 1, 1)
S_DEEP = (2, 1024, 260, 6, 6, 3, 3, 1, 1)
S_T64 = (15, 36, 256, 32, 32, 3, 3, 1, 1)
S_SK = (13, 68, 196, 16, 16, 3, 3, 1, 1)
S_NSQ = (4, 68, 132, 12, 17, 3, 5, 2, 1)
S_D64 = (3, 36, 68, 13, 11, 4, 4, 2, 1)        # four phases of unequal height / width (13 and 11 are odd)
S_D64E = (3, 36, 68, 14, 10, 4, 4, 2, 1)       # four equal phases: the interleaved launch can take them
S_W192 = (3, 64, 60, 11, 7, 3, 3, 1, 1)
S_WSLAB = (5, 100, 196, 23, 19, 3, 3, 1, 1)    # 128x128 slabs with several K-slices
S_WDEEP = (8, 100, 196, 34, 34, 3, 3, 1, 1)    # 289 k-tiles: wgrad_rounds changes the K-slices (29 of 10 -> 16 of 19)

# (id, shape, op, tune, pcg_conv_plan_describe(op, assume_scratch=1))
CASES = [
    # ---- forward
    ("fwd-128x64-mnk-tails", S_FWD64, FWD, {}, "128x64 tiles: 2"),
    ("fwd-128x64-b1-k5p2", (1, 20, 36, 9, 13, 5, 5, 1, 2), FWD, {}, "128x64 tiles: 1"),
    ("fwd-128x64-cin4", (3, 4, 36, 10, 9, 3, 3, 1, 1), FWD, {}, "128x64 tiles: 3"),
    # plan_fwd cuts this one into 4 K-slices of 8 k-tiles (1 x 2 tiles, 32 k-tiles); the describe string does not name K-slices at N <= 64
    ("fwd-128x64-s2-korder0", (5, 36, 20, 13, 11, 4, 4, 2, 1), FWD, {"korder": 0}, "128x64 tiles: 2"),
    ("fwd-128x64-s2-korder1", (5, 36, 20, 13, 11, 4, 4, 2, 1), FWD, {"korder": 1}, "128x64 tiles: 2"),
    ("fwd-128x128-ntail", S_DEEP, FWD, {"fwd_splits": 1}, "128x128 tiles: 3"),
    ("fwd-128x128-k1", (3, 100, 68, 7, 9, 1, 1, 1, 0), FWD, {}, "128x128 tiles: 2"),
    ("fwd-128x128-cin516", (2, 516, 68, 5, 7, 3, 3, 1, 1), FWD, {}, "128x128 tiles: 1 x 17 K-slices of 9 k-tiles (slabs)"),
    ("fwd-kslices-36x8", S_DEEP, FWD, {}, "128x128 tiles: 3 x 36 K-slices of 8 k-tiles (slabs)"),
    ("fwd-kslices-7x42-uneven", S_DEEP, FWD, {"fwd_splits": 7}, "128x128 tiles: 3 x 7 K-slices of 42 k-tiles (slabs)"),   # 288 = 6 x 42 + 36
    ("fwd-t64", S_T64, FWD, {}, "64x128 tiles: 480"),
    ("fwd-t64-off", S_T64, FWD, {"t64": 0}, "128x128 tiles: 240"),
    ("fwd-sk-256", S_SK, FWD, {}, "stream-K: 0 whole tiles + 52 tiles x 27 k-tiles over 256 ranges"),
    ("fwd-sk-128", S_SK, FWD, {"sk_blocks": 128}, "stream-K: 0 whole tiles + 52 tiles x 27 k-tiles over 128 ranges"),
    ("fwd-sk-64", S_SK, FWD, dict(SK, sk_blocks=64), "stream-K: 0 whole tiles + 52 tiles x 27 k-tiles over 64 ranges"),
    ("fwd-sk-256-forced", S_SK, FWD, dict(SK, sk_blocks=256), "stream-K: 0 whole tiles + 52 tiles x 27 k-tiles over 256 ranges"),
    ("fwd-sk-mode3", S_SK, FWD, {"stream_k": 3}, "stream-K: 52 whole tiles + 0 tiles x 27 k-tiles over 0 ranges"),
    ("fwd-nonsquare-s2-korder0", S_NSQ, FWD, {"korder": 0}, "128x128 tiles: 4 x 5 K-slices of 9 k-tiles (slabs)"),
    ("fwd-nonsquare-s2-korder1", S_NSQ, FWD, {"korder": 1}, "128x128 tiles: 4 x 5 K-slices of 9 k-tiles (slabs)"),
    ("fwd-nonsquare-s2-plain", S_NSQ, FWD, {"fwd_splits": 1}, "128x128 tiles: 4"),
] + [
    (f"fwd-128x128-edge{e}", S_DEEP, FWD, {"fwd_splits": 1, "edge_prio": e}, "128x128 tiles: 3") for e in range(4)
] + [
    # ---- grad-input
    ("dgrad-1ph-128x128", (3, 68, 100, 11, 7, 3, 3, 1, 1), DGRAD, {}, "1 phase: 128x128 tiles: 2 per phase"),
    ("dgrad-1ph-128x64-b1-k5p2", (1, 20, 36, 9, 13, 5, 5, 1, 2), DGRAD, {}, "1 phase: 128x64 tiles: 1 per phase"),
    ("dgrad-1ph-sk", (16, 132, 260, 15, 15, 3, 3, 1, 1), DGRAD, SK, "1 phase: stream-K: 0 whole tiles + 58 tiles over 256 ranges"),
    ("dgrad-4ph-uniform-sk-korder1", (16, 132, 256, 14, 14, 4, 4, 2, 1), DGRAD, dict(SK, korder=1),
     "4 phases: stream-K: 0 whole tiles + 56 tiles over 256 ranges"),
    ("dgrad-4ph-uniform-sk-korder0", (16, 132, 256, 14, 14, 4, 4, 2, 1), DGRAD, dict(SK, korder=0),
     "4 phases: stream-K: 0 whole tiles + 56 tiles over 256 ranges"),
    ("dgrad-4ph-unequal-skn-korder1", (64, 132, 260, 13, 13, 3, 3, 2, 0), DGRAD, dict(SK, dgrad_gemm=0, korder=1),
     "4 phases: stream-K over unequal phases: 170 tiles, 3636 k-tile iterations over 256 ranges"),
    ("dgrad-4ph-unequal-skn-korder0", (64, 132, 260, 13, 13, 3, 3, 2, 0), DGRAD, dict(SK, dgrad_gemm=0, korder=0),
     "4 phases: stream-K over unequal phases: 170 tiles, 3636 k-tile iterations over 256 ranges"),
    ("dgrad-4ph-unequal-sk128", (64, 132, 260, 13, 13, 3, 3, 2, 0), DGRAD, dict(SK, dgrad_gemm=0, sk_blocks=128),
     "4 phases: stream-K over unequal phases: 170 tiles, 3636 k-tile iterations over 128 ranges"),
    ("dgrad-4ph-unequal-plain", (64, 132, 260, 13, 13, 3, 3, 2, 0), DGRAD, {"stream_k": 0}, "4 phases: 128x128 tiles: 50 per phase"),
    ("dgrad-gemm-col2im", (8, 132, 516, 13, 11, 3, 3, 2, 0), DGRAD, {"dgrad_gemm": 1}, "GEMM + col2im: 128x128 tiles: 20"),
    ("dgrad-gemm-col2im-sk", (8, 132, 516, 13, 11, 3, 3, 2, 0), DGRAD, dict(SK, dgrad_gemm=1),
     "GEMM + col2im: stream-K: 0 whole tiles + 20 tiles x 17 k-tiles over 64 ranges"),
    ("dgrad-nonsquare-s2-korder0", S_NSQ, DGRAD, {"korder": 0}, "4 phases: 128x128 tiles: 2 per phase"),
    ("dgrad-nonsquare-s2-korder1", S_NSQ, DGRAD, {"korder": 1}, "4 phases: 128x128 tiles: 2 per phase"),
    # 128x64 grad-input: conv2d_dgrad_impl takes Cfg128x64P when nph > 1 && dgrad_swz3 == 0, else the swizzled Cfg128x64
    ("dgrad-128x64-swz-unequal", S_D64, DGRAD, {}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64P-unequal", S_D64, DGRAD, {"dgrad_swz3": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64-swz-s2-korder0", S_D64, DGRAD, {"korder": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64P-s2-korder0", S_D64, DGRAD, {"korder": 0, "dgrad_swz3": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    # interleaved phases: launch_dgrad_x interleaves when nph > 1, dgrad_interleave != 0, w_bytes <= 1 MiB and every phase has equal Mp
    ("dgrad-128x64-swz-interleave1", S_D64E, DGRAD, {"dgrad_interleave": 1}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64-swz-interleave0", S_D64E, DGRAD, {"dgrad_interleave": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64P-interleave1", S_D64E, DGRAD, {"dgrad_interleave": 1, "dgrad_swz3": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-128x64P-interleave0", S_D64E, DGRAD, {"dgrad_interleave": 0, "dgrad_swz3": 0}, "4 phases: 128x64 tiles: 1 per phase"),
    # k1 s2: build_phases gives three phases no tap (nth = 0, ntw = 1): zero k-tiles, the bias alone
    ("dgrad-k1s2-notaps-128x64", (4, 64, 132, 9, 9, 1, 1, 2, 0), DGRAD, {}, "4 phases: 128x64 tiles: 1 per phase"),
    ("dgrad-k1s2-notaps-128x128", (4, 132, 68, 9, 9, 1, 1, 2, 0), DGRAD, {}, "4 phases: 128x128 tiles: 2 per phase"),
    ("dgrad-k1s2-gemm-col2im", (4, 64, 512, 9, 9, 1, 1, 2, 0), DGRAD, {}, "GEMM + col2im: 128x128 tiles: 1"),
] + [
    (f"dgrad-128x64-edge{e}", S_D64, DGRAD, {"edge_prio": e}, "4 phases: 128x64 tiles: 1 per phase") for e in range(4)
] + [
    # ---- weight gradient (slice order: slice_major = wgrad_order if set, else tiles <= 8)
    ("wgrad-64x128-narrow", S_FWD64, WGRAD, {}, "64x128 tiles: 3 x 1 K-slices of 8 k-tiles (slabs + slab_reduce)"),
    ("wgrad-64x128-b1-k5p2", (1, 20, 36, 9, 13, 5, 5, 1, 2), WGRAD, {}, "64x128 tiles: 4 x 1 K-slices of 4 k-tiles (slabs + slab_reduce)"),
    ("wgrad-64x128-cin4", (3, 4, 36, 10, 9, 3, 3, 1, 1), WGRAD, {}, "64x128 tiles: 1 x 1 K-slices of 9 k-tiles (slabs + slab_reduce)"),
    ("wgrad-w192", S_W192, WGRAD, {}, "64x192 tiles: 3 x 1 K-slices of 8 k-tiles (slabs + slab_reduce)"),
    ("wgrad-w192-slices-order0", (7, 64, 60, 21, 19, 3, 3, 1, 1), WGRAD, {"wgrad_order": 0},
     "64x192 tiles: 3 x 11 K-slices of 8 k-tiles (slabs + slab_reduce)"),
    ("wgrad-w192-slices-order1", (7, 64, 60, 21, 19, 3, 3, 1, 1), WGRAD, {"wgrad_order": 1},
     "64x192 tiles: 3 x 11 K-slices of 8 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-slab", (3, 100, 196, 11, 7, 3, 3, 1, 1), WGRAD, {}, "128x128 tiles: 16 x 1 K-slices of 8 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-nonsquare-s2", S_NSQ, WGRAD, {}, "128x128 tiles: 16 x 1 K-slices of 6 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-slices", S_WSLAB, WGRAD, {}, "128x128 tiles: 16 x 8 K-slices of 9 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-slices-order0", S_WSLAB, WGRAD, {"wgrad_order": 0}, "128x128 tiles: 16 x 8 K-slices of 9 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-slices-order1", S_WSLAB, WGRAD, {"wgrad_order": 1}, "128x128 tiles: 16 x 8 K-slices of 9 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-deep", S_WDEEP, WGRAD, {}, "128x128 tiles: 16 x 29 K-slices of 10 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-deep-rounds2", S_WDEEP, WGRAD, {"wgrad_rounds": 2}, "128x128 tiles: 16 x 16 K-slices of 19 k-tiles (slabs + slab_reduce)"),
    ("wgrad-128x128-deep-rounds3-order1", S_WDEEP, WGRAD, {"wgrad_rounds": 3, "wgrad_order": 1},
     "128x128 tiles: 16 x 16 K-slices of 19 k-tiles (slabs + slab_reduce)"),
    ("wgrad-sk-epilogue", (6, 516, 260, 9, 9, 3, 3, 1, 1), WGRAD, SK,
     "stream-K: 0 whole tiles + 111 tiles x 16 k-tiles over 256 ranges, dw written by the epilogue"),
    ("wgrad-dp-epilogue", (2, 516, 260, 4, 4, 3, 3, 1, 1), WGRAD, {}, "128x128 tiles: 111, dw written by the epilogue"),
]


def _expected_plan(want):
    if os.environ.get("PCG_WGRAD_192") == "0" and want.startswith("64x192 tiles: "):
        # env-only switch (read once per process): the 64x192 tile is off, its N / 192 tiles (M <= 64) become ceil(N / 128) of 64x128
        tiles, rest = want[len("64x192 tiles: "):].split(" ", 1)
        want = f"64x128 tiles: {-(-int(tiles) * 192 // 128)} {rest}"
    return want


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    lib = pcgan_amd.load()
    pcgan_amd.ops._conv_scratch()           # this stream's stream-K scratch before the first workspace query (it plans with it)
    try:
        yield pcgan_amd
    finally:
        for name in SWITCHES:
            lib.pcg_tune_set(name.encode(), -1)
        lib.pcg_conv_precision_set(0)


@contextlib.contextmanager
def _tuned(lib, tune):
    try:
        for k, v in tune.items():
            assert lib.pcg_tune_set(k.encode(), int(v)) == 0, k
        yield
    finally:
        for k in tune:
            lib.pcg_tune_set(k.encode(), -1)


def _geom(shape):
    from pcgan_amd import _lib
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    return _lib.ConvGeom(B, H, W, Cin, (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1, Cout, KH, KW, s, p)


def _describe(lib, shape, op):
    buf = ctypes.create_string_buffer(512)
    assert lib.pcg_conv_plan_describe(ctypes.byref(_geom(shape)), op, 1, buf, 512) == 0
    return buf.value.decode()


def _assert_plan(lib, shape, op, tune, want):
    with _tuned(lib, tune):
        got = _describe(lib, shape, op)
    want = _expected_plan(want)
    assert got == want, f"plan moved: {got!r} (expected {want!r})"


def _check_plans():
    """Every case's form through the planner alone (no device): tests/test_host_logic.py runs this in a fresh process."""
    from pcgan_amd import _lib
    lib = _lib.load()
    for cid, shape, op, tune, want in CASES:
        try:
            _assert_plan(lib, shape, op, tune, want)
        except AssertionError as e:
            raise AssertionError(f"{cid}: {e}") from None
    for name, shape, tune, fwd_want, dgrad_want in EPI_FORMS:
        for op, want in ((FWD, fwd_want), (DGRAD, dgrad_want)):
            if want is not None:
                _assert_plan(lib, shape, op, tune, want)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def _tol(K, scale):
    return 2e-6 * math.sqrt(K) * scale + 1e-6


def _bf16_bound(K, s_term):
    return 16.0 * U * K * s_term / math.sqrt(6.0) + 1e-6


def _randn(*shape, g, scale=1.0):
    """float64 values that are exactly representable in float32 (the kernels' inputs are then the reference's inputs)."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _on_dev(t):
    return t.detach().float().contiguous().to(dev())


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


def _act64(v, act, slope):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def _operands(shape, seed):
    """x [B,Cin,H,W], w [Cout,Cin,KH,KW] (scaled 1/sqrt(taps*Cin)), dy [B,Cout,OH,OW], bias [Cout], bias_x [Cin]: float64, fp32-exact."""
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
    g = torch.Generator().manual_seed(seed)
    x = _randn(B, Cin, H, W, g=g)
    w = _randn(Cout, Cin, KH, KW, g=g, scale=1.0 / math.sqrt(Cin * KH * KW))
    dy = _randn(B, Cout, OH, OW, g=g)
    return x, w, dy, _randn(Cout, g=g), _randn(Cin, g=g)


def _seed(cid):
    return sum(ord(c) * (i + 1) for i, c in enumerate(cid)) % 100003


def _fwd64(x, w, s, p, b=None):
    return _nhwc(F.conv2d(x, w, b, stride=s, padding=p))


def _dgrad64(x_shape, w, dy, s, p, bx=None):
    dx = torch.nn.grad.conv2d_input(x_shape, w, dy, stride=s, padding=p)
    return _nhwc(dx + bx.view(1, -1, 1, 1) if bx is not None else dx)


def _wgrad64(x, w_shape, dy, s, p):
    return _nhwc(torch.nn.grad.conv2d_weight(x, w_shape, dy, stride=s, padding=p))


def _bf(t):
    return t.float().to(torch.bfloat16).double()


# ---- 1 + 3: the form table, fp32 and bf16 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in CASES])
def test_igemm_form_against_float64(pcg, case, precision):
    ops, lib = pcg.ops, pcg.load()
    cid, shape, op, tune, want = case
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    g = ops.conv_geom(B, H, W, Cin, Cout, KH, KW, s, p)
    x, w, dy, b, bx = _operands(shape, _seed(cid))
    xd, wd, dyd, bd, bxd = _on_dev(_nhwc(x)), _on_dev(_nhwc(w)), _on_dev(_nhwc(dy)), _on_dev(b), _on_dev(bx)
    bf16 = precision == "bf16"
    with _tuned(lib, tune):
        got_plan = _describe(lib, shape, op)
        assert got_plan == _expected_plan(want), f"plan moved: {got_plan!r} (expected {want!r})"
        with ops.conv_precision(precision):
            if op == FWD:
                got = ops.conv2d_fwd(g, xd, wd, bd)
            elif op == DGRAD:
                got = ops.conv2d_dgrad(g, dyd, wd, bxd)
            else:
                dwd = torch.full((Cout, KH, KW, Cin), 0.5, dtype=torch.float32, device=dev())
                ops.conv2d_wgrad(g, xd, dyd, dwd, accumulate=False)          # overwrites the 0.5 fill
                got = dwd.clone()
                ops.conv2d_wgrad(g, xd, dyd, dwd, accumulate=True)
                got2 = dwd
    torch.cuda.synchronize()

    def ref(rounded):
        xr, wr, dyr = (_bf(x), _bf(w), _bf(dy)) if rounded else (x, w, dy)
        if op == FWD:
            return _fwd64(xr, wr, s, p, b)
        if op == DGRAD:
            return _dgrad64(x.shape, wr, dyr, s, p, bx)
        return _wgrad64(xr, w.shape, dyr, s, p)

    taps = KH * KW
    if not bf16:
        K, scale = {FWD: (taps * Cin, 4.0), DGRAD: (taps * Cout, 4.0), WGRAD: (B * g.OH * g.OW, 8.0)}[op]
        bound = _tol(K, scale)
    else:
        Kf = taps * Cin
        bound = {FWD: _bf16_bound(Kf, 1 / math.sqrt(Kf)),
                 DGRAD: _bf16_bound(Cout * ((KH + s - 1) // s) * ((KW + s - 1) // s), 1 / math.sqrt(Kf)),
                 WGRAD: _bf16_bound(B * g.OH * g.OW, 1.0)}[op]
    want64 = ref(bf16)
    err = _err(got, want64)
    assert err <= bound, f"{cid} {precision}: max err {err:.3e} > {bound:.3e}"
    if op == WGRAD:
        err = _err(got2, 2 * want64)
        assert err <= 2 * bound, f"{cid} {precision}: accumulate max err {err:.3e} > {2 * bound:.3e}"
    if bf16:
        far = _err(got, ref(False))
        assert far >= 10 * bound, f"{cid}: only {far:.3e} from the unrounded float64 (bound {bound:.3e}): did it run fp32?"


def test_wide192_cases_on_the_64x128_tile_in_a_child_process():
    """PCG_WGRAD_192=0 (env-only, read once per process): a fresh process runs the 64x192 cases of this file on the 64x128 tile (their
    plan assertion expects "64x128" there) against float64."""
    env = dict(os.environ, PCG_WGRAD_192="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "w192 and not child_process"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out after {e.timeout} s\n{e.stdout or ''}\n{e.stderr or ''}")
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"child exit {r.returncode}\n{out[-8000:]}"
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, out[-4000:]


# ---- 2: epilogues and fused statistics ------------------------------------------------------------------------------------------
# (name, shape, tune, forward form, grad-input form; None: not run on that side).  Ragged M everywhere but on the 64x128 forward
# (fwd_use_t64 needs M % 128 == 0).  The fused forward epilogues need a forward without K-slices: the skn geometry's has them.
EPI_FORMS = [
    ("f128x128-d128x128", (3, 68, 132, 11, 7, 3, 3, 1, 1), {}, "128x128 tiles: 4", "1 phase: 128x128 tiles: 2 per phase"),
    ("f128x64-d128x64-4ph", (3, 20, 36, 13, 11, 4, 4, 2, 1), {}, "128x64 tiles: 1", "4 phases: 128x64 tiles: 1 per phase"),
    ("f64x128-d128x64", S_T64, {}, "64x128 tiles: 480", "1 phase: 128x64 tiles: 120 per phase"),
    ("fsk-dsk", (13, 68, 196, 15, 15, 3, 3, 1, 1), SK, "stream-K: 0 whole tiles + 46 tiles x 27 k-tiles over 256 ranges",
     "1 phase: stream-K: 0 whole tiles + 23 tiles over 128 ranges"),
    ("dskn", (48, 132, 260, 13, 13, 3, 3, 2, 0), dict(SK, dgrad_gemm=0), None,
     "4 phases: stream-K over unequal phases: 130 tiles, 2772 k-tile iterations over 256 ranges"),
]
EPI_SIDES = [pytest.param(f, dgrad, id=f"{f[0]}-{'dgrad' if dgrad else 'fwd'}")
             for f in EPI_FORMS for dgrad in (False, True) if f[4 if dgrad else 3] is not None]


class _Epi:
    """One form's operands: a forward conv of x (output [B,OH,OW,Cout]) and a grad-input of dy (output [B,H,W,Cin])."""

    def __init__(self, pcg, form, seed):
        self.name, self.shape, self.tune, fwd_want, dgrad_want = form
        self.want = {False: fwd_want, True: dgrad_want}
        B, Cin, Cout, H, W, KH, KW, s, p = self.shape
        self.ops, self.lib = pcg.ops, pcg.load()
        self.g = self.ops.conv_geom(B, H, W, Cin, Cout, KH, KW, s, p)
        self.x, self.w, self.dy, self.b, self.bx = _operands(self.shape, seed)
        self.xd, self.wd, self.dyd = _on_dev(_nhwc(self.x)), _on_dev(_nhwc(self.w)), _on_dev(_nhwc(self.dy))
        self.bd, self.bxd = _on_dev(self.b), _on_dev(self.bx)
        self.s, self.p = s, p
        self.K = {False: KH * KW * Cin, True: KH * KW * Cout}
        self.gen = torch.Generator().manual_seed(seed + 1)

    def check_plan(self, dgrad):
        """(inside the form's tune switches)"""
        _assert_plan(self.lib, self.shape, DGRAD if dgrad else FWD, {}, self.want[dgrad])

    def conv64(self, dgrad, bias=False):
        """float64 forward (dgrad False) or grad-input (True), NHWC."""
        if dgrad:
            return _dgrad64(self.x.shape, self.w, self.dy, self.s, self.p, self.bx if bias else None)
        return _fwd64(self.x, self.w, self.s, self.p, self.b if bias else None)

    def tol(self, dgrad):
        return _tol(self.K[dgrad], 4.0)

    def out_shape(self, dgrad):
        g = self.g
        return (g.B, g.IH, g.IW, g.Cin) if dgrad else (g.B, g.OH, g.OW, g.Cout)

    def rand(self, dgrad, scale=1.0, shift=0.0):
        return _randn(*self.out_shape(dgrad), g=self.gen, scale=scale) + shift


# the grad-input as GEMM + col2im takes no epilogue (dgrad_as_gemm needs !epi): its activation is col2im_kernel's (ReLU / LeakyReLU) or
# the second pass
COL2IM_SIDES = [pytest.param(("dgemm", (8, 132, 516, 13, 11, 3, 3, 2, 0), {"dgrad_gemm": 1}, None, "GEMM + col2im: 128x128 tiles: 20"),
                             True, id="dgemm-dgrad"),
                pytest.param(("dgemm-sk", (8, 132, 516, 13, 11, 3, 3, 2, 0), dict(SK, dgrad_gemm=1), None,
                              "GEMM + col2im: stream-K: 0 whole tiles + 20 tiles x 17 k-tiles over 64 ranges"), True, id="dgemm-sk-dgrad")]
ACTS = [pytest.param(ACT_RELU, 0.0, id="relu"), pytest.param(ACT_LRELU, 0.2, id="lrelu"), pytest.param(ACT_TANH, 0.0, id="tanh"),
        pytest.param(ACT_SIGMOID, 0.0, id="sigmoid")]


@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("form,dgrad", EPI_SIDES + COL2IM_SIDES)
def test_fused_activation_against_float64(pcg, form, dgrad, act, slope):
    """fwd_act / dgrad_act: ReLU / LeakyReLU in the epilogue, tanh / sigmoid as the second pass, with the bias."""
    e = _Epi(pcg, form, 101 + act)
    with _tuned(e.lib, e.tune):
        e.check_plan(dgrad)
        if dgrad:
            got = e.ops.conv2d_dgrad(e.g, e.dyd, e.wd, e.bxd, act=act, slope=slope)
        else:
            got = e.ops.conv2d_fwd(e.g, e.xd, e.wd, e.bd, act=act, slope=slope)
    err = _err(got, _act64(e.conv64(dgrad, bias=True), act, slope))
    assert err <= e.tol(dgrad), f"max err {err:.3e}"


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("form,dgrad", EPI_SIDES)
def test_mask_add_and_add_mask_epilogues_against_float64(pcg, form, dgrad, act, slope):
    """fwd_mask / dgrad_mask (times act'(a_below)), fwd_add / dgrad_add (into a new tensor and in place: addend = output) and
    fwd_add_mask / dgrad_add_mask.  The masks read a_below > 0 on the given tensor: exact, no band."""
    e = _Epi(pcg, form, 202 + act)
    ops = e.ops
    a_below, addend = e.rand(dgrad), e.rand(dgrad)
    ad, add_d = _on_dev(a_below), _on_dev(addend)
    conv = e.conv64(dgrad)
    m = torch.where(a_below > 0, 1.0, slope)
    d = e.dyd if dgrad else e.xd
    with _tuned(e.lib, e.tune):
        e.check_plan(dgrad)
        res = ops.conv_bwd_data_fused(e.g, d, e.wd, not dgrad, act, slope, a_below=ad)
        assert res is not None
        err = _err(res[0], conv * m)
        assert err <= e.tol(dgrad), f"mask max err {err:.3e}"
        got = ops.conv2d_dgrad_add(e.g, d, e.wd, add_d, transposed=not dgrad)
        err = _err(got, conv + addend)
        assert err <= e.tol(dgrad), f"add max err {err:.3e}"
        inplace = add_d.clone()
        got = ops.conv2d_dgrad_add(e.g, d, e.wd, inplace, out=inplace, transposed=not dgrad)
        assert got.data_ptr() == inplace.data_ptr()
        err = _err(inplace, conv + addend)
        assert err <= e.tol(dgrad), f"in-place add max err {err:.3e}"
        got = ops.conv2d_dgrad_add_mask(e.g, d, e.wd, add_d, ad, act, slope, transposed=not dgrad)
        err = _err(got, (conv + addend) * m)
        assert err <= e.tol(dgrad), f"add_mask max err {err:.3e}"
        inplace = add_d.clone()
        ops.conv2d_dgrad_add_mask(e.g, d, e.wd, inplace, ad, act, slope, out=inplace, transposed=not dgrad)
        err = _err(inplace, (conv + addend) * m)
        assert err <= e.tol(dgrad), f"in-place add_mask max err {err:.3e}"


def _bn_bwd64(dm, z, mean, invstd, gamma):
    """float64 BatchNorm backward from dm (the gradient w.r.t. the BatchNorm output) with the given statistics: dz, dgamma, dbeta."""
    C = z.shape[-1]
    dm, z = dm.reshape(-1, C), z.reshape(-1, C)
    xh = (z - mean) * invstd
    n = z.shape[0]
    db, dg = dm.sum(0), (dm * xh).sum(0)
    return gamma * invstd * (dm - db / n - xh * dg / n), dg, db


def _check_sums(dgd, dbd, dg_ref, db_ref):
    """test_hip_ops.py::test_batchnorm_fwd_bwd's bounds on dgamma / dbeta: rtol 1e-4, atol 2e-5 * scale."""
    scale = max(float(dg_ref.abs().max()), float(db_ref.abs().max()), 1.0)
    for what, got, ref in (("dgamma", dgd, dg_ref), ("dbeta", dbd, db_ref)):
        d = (got.cpu().double() - ref).abs()
        assert bool((d <= 1e-4 * ref.abs() + 2e-5 * scale).all()), f"{what} max err {float(d.max()):.3e}"


def _check_dz(dz, dz_ref):
    """... and on the BatchNorm input gradient: rtol 1e-4, atol 2e-5."""
    d = (dz.cpu().double().reshape(dz_ref.shape) - dz_ref).abs()
    assert bool((d <= 1e-4 * dz_ref.abs() + 2e-5).all()), f"dz max err {float(d.max()):.3e}"


def _check_bn_bwd(dz, dgd, dbd, want):
    dz_ref, dg_ref, db_ref = want
    _check_sums(dgd, dbd, dg_ref, db_ref)
    _check_dz(dz, dz_ref)


def _stats(e, C, dgrad, seed):
    g = torch.Generator().manual_seed(seed)
    z = e.rand(dgrad, scale=1.3, shift=0.25)
    zr = z.reshape(-1, C)
    mean = zr.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(zr.var(0, unbiased=False) + 1e-5)).float().double()
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    beta = _randn(C, g=g, scale=0.1)
    return z, mean, invstd, gamma, beta


@pytest.mark.parametrize("with_addend", [pytest.param(True, id="addend"), pytest.param(False, id="no_addend")])
@pytest.mark.parametrize("form,dgrad", EPI_SIDES)
def test_add_bnsum_against_float64(pcg, form, dgrad, with_addend):
    """fwd_add_bnsum / dgrad_add_bnsum: out = conv + addend (or the plain conv), and the column sums of scale*out for the BatchNorm of
    z_next, consumed by bn_bwd_partial(dm_scale=scale): dz, dgamma, dbeta against float64 of the kernel's own output (the sums are
    what is under test; the output itself against the float64 conv)."""
    e = _Epi(pcg, form, 303 + with_addend)
    ops = e.ops
    C = e.out_shape(dgrad)[3]
    z, mean, invstd, gamma, beta = _stats(e, C, dgrad, 7)
    addend = e.rand(dgrad) if with_addend else None
    scale = 0.1
    dg0, db0 = _randn(C, g=e.gen), _randn(C, g=e.gen)
    dgd, dbd = _on_dev(dg0), _on_dev(db0)
    with _tuned(e.lib, e.tune):
        e.check_plan(dgrad)
        out, partial, nparts = ops.conv2d_dgrad_add(e.g, e.dyd if dgrad else e.xd, e.wd, _on_dev(addend) if with_addend else None,
                                                    bnsum=(_on_dev(z), _on_dev(mean), _on_dev(invstd), scale), transposed=not dgrad)
        dz = ops.bn_bwd_partial(out, _on_dev(z), C, _on_dev(mean), _on_dev(invstd), _on_dev(gamma), partial, nparts, dgd, dbd, True,
                                dm_scale=scale)
    want_out = e.conv64(dgrad) + (addend if with_addend else 0.0)
    err = _err(out, want_out)
    assert err <= e.tol(dgrad), f"output max err {err:.3e}"
    _check_bn_bwd(dz, dgd - _on_dev(dg0), dbd - _on_dev(db0), _bn_bwd64(scale * out.cpu().double(), z, mean, invstd, gamma))


def _fold32(mean, invstd, gamma, beta):
    """bn_fold in fp32: sc = gamma * invstd, sh = fmaf(-mean, sc, beta) (the product is exact in float64, one rounding to fp32)."""
    sc = (gamma.float() * invstd.float()).double()
    sh = (beta - mean * sc).float().double()
    return sc, sh


def _pre32(z, sc, sh):
    """fmaf(z, sc, sh): exact product in float64, one rounding to fp32 (the double rounding of the sum is below the band below)."""
    return (z * sc + sh).float().double()


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("form,dgrad", EPI_SIDES)
def test_bnbwd_epilogue_against_float64(pcg, form, dgrad, act, slope):
    """dgrad_bnbwd / fwd_bnbwd: out = conv * act'(bn(z_below)) and the BatchNorm-backward column sums, consumed by bn_bwd_partial.
    The mask is the kernel's: pre = fmaf(z, sc, sh) from the fp32 bn_fold; elements within 1e-6 of the kink are excluded, and
    there must be few of them."""
    e = _Epi(pcg, form, 404 + act)
    ops = e.ops
    C = e.out_shape(dgrad)[3]
    z, mean, invstd, gamma, beta = _stats(e, C, dgrad, 9)
    dgd, dbd = torch.zeros(C, device=dev()), torch.zeros(C, device=dev())
    with _tuned(e.lib, e.tune):
        e.check_plan(dgrad)
        res = ops.conv_bwd_data_fused(e.g, e.dyd if dgrad else e.xd, e.wd, not dgrad, act, slope, z_below=_on_dev(z),
                                      bn=(_on_dev(mean), _on_dev(invstd), _on_dev(gamma), _on_dev(beta)))
        assert res is not None
        dm, partial, nparts = res
        dz = ops.bn_bwd_partial(dm, _on_dev(z), C, _on_dev(mean), _on_dev(invstd), _on_dev(gamma), partial, nparts, dgd, dbd, False)
    sc, sh = _fold32(mean, invstd, gamma, beta)
    pre = _pre32(z, sc, sh)
    near = pre.abs() <= 1e-6
    assert int(near.sum()) <= max(4, 1e-4 * near.numel()), f"{int(near.sum())} elements at the kink"
    want = e.conv64(dgrad) * torch.where(pre > 0, 1.0, slope)
    d = (dm.cpu().double() - want).abs()
    assert float(d[~near].max()) <= e.tol(dgrad), f"masked output max err {float(d[~near].max()):.3e}"
    _check_bn_bwd(dz, dgd, dbd, _bn_bwd64(dm.cpu().double(), z, mean, invstd, gamma))


@pytest.mark.parametrize("form,dgrad", EPI_SIDES)
def test_conv_bn_statistics_against_float64(pcg, form, dgrad):
    """fwd_bn / dgrad_bn (conv_bn_train): z against the float64 conv with its bias; mean / invstd, the running statistics and
    num_batches_tracked against float64 of the kernel's own z (test_hip_ops.py's bounds: rtol 1e-5, atol 1e-6); the folded
    coefficients against gamma * invstd, beta - mean * gamma * invstd."""
    e = _Epi(pcg, form, 505)
    ops = e.ops
    C = e.out_shape(dgrad)[3]
    rm0, rv0 = _randn(C, g=e.gen, scale=0.1), torch.rand(C, generator=e.gen, dtype=torch.float64).float().double() + 0.5
    rm, rv, nbt = _on_dev(rm0), _on_dev(rv0), torch.full((1,), 3, dtype=torch.int64, device=dev())
    gamma, beta = _randn(C, g=e.gen) + 1.0, _randn(C, g=e.gen, scale=0.1)
    with _tuned(e.lib, e.tune):
        e.check_plan(dgrad)
        z, mean, invstd, coef = ops.conv_bn_train(e.g, e.dyd if dgrad else e.xd, e.wd, e.bxd if dgrad else e.bd, dgrad, 1e-5, 0.1,
                                                  rm, rv, nbt, gamma=_on_dev(gamma), beta=_on_dev(beta))
    err = _err(z, e.conv64(dgrad, bias=True))
    assert err <= e.tol(dgrad), f"z max err {err:.3e}"
    zz = z.cpu().double().reshape(-1, C)
    m64, v64 = zz.mean(0), zz.var(0, unbiased=False)
    torch.testing.assert_close(mean.cpu().double(), m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(invstd.cpu().double(), 1.0 / torch.sqrt(v64 + 1e-5), rtol=1e-5, atol=1e-6)
    n = zz.shape[0]
    torch.testing.assert_close(rm.cpu().double(), 0.9 * rm0 + 0.1 * m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.cpu().double(), 0.9 * rv0 + 0.1 * v64 * n / (n - 1), rtol=1e-5, atol=1e-6)
    assert int(nbt.item()) == 4
    sc = gamma * invstd.cpu().double()
    torch.testing.assert_close(coef.cpu().double()[:C], sc, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(coef.cpu().double()[C:], beta - mean.cpu().double() * sc, rtol=1e-5, atol=1e-6)


XF_FORMS = [pytest.param(f, id=f[0]) for f in EPI_FORMS] + [
    pytest.param(("w192-xf", S_W192, {}, "128x64 tiles: 2", "1 phase: 128x64 tiles: 2 per phase"), id="w192-xf")]


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("form", XF_FORMS)
def test_input_transform_against_float64(pcg, form, act, slope):
    """The XF instantiations: forward with x = act(z*sc + sh), grad-input with dy transformed, and both weight-gradient sides.  At Cout
    <= 64 with 3x3x64 columns (w192-xf) plan_wgrad picks the 64x192 tile, which has no XF form: pcg_conv2d_wgrad_xf re-plans onto
    64x128 (the branch `if (wp.wide192)` under `side != 0`)."""
    e = _Epi(pcg, form, 606 + act)
    ops = e.ops
    B, Cin, Cout, H, W, KH, KW, s, p = e.shape

    def xform(C, like_dgrad_out):
        z = e.rand(like_dgrad_out, scale=1.3, shift=0.2)
        sc = (torch.rand(C, generator=e.gen, dtype=torch.float64) + 0.5).float().double()
        sh = _randn(C, g=e.gen, scale=0.3)
        a = _pre32(z, sc, sh)
        a = torch.where(a > 0, a, (a * slope).float().double()) if act == ACT_LRELU else a.clamp_min(0)
        xf = ops.InputXform(_on_dev(torch.cat([sc, sh])), act, slope)
        return z, a, xf

    zx, ax, xfx = xform(Cin, True)           # an activation of x's shape [B,H,W,Cin]
    zy, ay, xfy = xform(Cout, False)         # an activation of dy's shape [B,OH,OW,Cout]
    a_x, a_y = _nchw(ax), _nchw(ay)
    with _tuned(e.lib, e.tune):
        got_f = ops.conv2d_fwd(e.g, _on_dev(zx), e.wd, e.bd, xf=xfx)
        got_d = ops.conv2d_dgrad(e.g, _on_dev(zy), e.wd, e.bxd, xf=xfy)
        dw_x = torch.full((Cout, KH, KW, Cin), 0.5, device=dev())
        ops.conv2d_wgrad(e.g, _on_dev(zx), e.dyd, dw_x, False, xf_x=xfx)
        dw_y = torch.full((Cout, KH, KW, Cin), 0.5, device=dev())
        ops.conv2d_wgrad(e.g, e.xd, _on_dev(zy), dw_y, False, xf_dy=xfy)
        dw_y2 = dw_y.clone()
        ops.conv2d_wgrad(e.g, e.xd, _on_dev(zy), dw_y2, True, xf_dy=xfy)
    err = _err(got_f, _fwd64(a_x, e.w, s, p, e.b))
    assert err <= e.tol(False), f"fwd xf max err {err:.3e}"
    err = _err(got_d, _dgrad64(e.x.shape, e.w, a_y, s, p, e.bx))
    assert err <= e.tol(True), f"dgrad xf max err {err:.3e}"
    K = B * e.g.OH * e.g.OW
    err = _err(dw_x, _wgrad64(a_x, e.w.shape, e.dy, s, p))
    assert err <= _tol(K, 8.0), f"wgrad xf_x max err {err:.3e}"
    ref = _wgrad64(e.x, e.w.shape, a_y, s, p)
    err = _err(dw_y, ref)
    assert err <= _tol(K, 8.0), f"wgrad xf_dy max err {err:.3e}"
    err = _err(dw_y2, 2 * ref)
    assert err <= 2 * _tol(K, 8.0), f"wgrad xf_dy accumulate max err {err:.3e}"


# ---- grouped BatchNorm forms -----------------------------------------------------------------------------------------------------
# (B over all groups, Cin, Cout, H, groups): k4 s2 p1; every group has whole 128-row tiles
GROUPED_FWD = [(4, 36, 64, 16, 2), (6, 36, 64, 16, 3), (8, 36, 128, 16, 4), (16, 20, 64, 16, 8), (288, 64, 128, 32, 3)]


@pytest.mark.parametrize("B,Cin,Cout,H,groups", GROUPED_FWD)
def test_grouped_conv_bn_against_float64(pcg, B, Cin, Cout, H, groups):
    """fwd_bn_g: each group's statistics against float64 of its own rows of the kernel's z; the running statistics move once per
    group, in group order; num_batches_tracked advances by `groups`.  (288, 64, 128, 32, 3) is test_hip_groups.py's [96-128-16-3]."""
    ops = pcg.ops
    shape = (B, Cin, Cout, H, H, 4, 4, 2, 1)
    g = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    assert ops.group_fwd_ok(g, groups)
    x, w, _, b, _ = _operands(shape, 700 + B + groups)
    per = B // groups
    x = torch.cat([x[k * per:(k + 1) * per] * (1 + 0.5 * k) + 0.2 * k for k in range(groups)]).float().double()   # distinct statistics
    rm0 = _randn(Cout, g=torch.Generator().manual_seed(1), scale=0.1)
    rv0 = rm0.abs() + 0.75
    rm, rv, nbt = _on_dev(rm0), _on_dev(rv0), torch.zeros(1, dtype=torch.int64, device=dev())
    z, mean, invstd = ops.conv_bn_train_g(g, _on_dev(_nhwc(x)), _on_dev(_nhwc(w)), _on_dev(b), 1e-5, 0.1, rm, rv, nbt, groups)
    err = _err(z, _fwd64(x, w, 2, 1, b))
    assert err <= _tol(16 * Cin, 4.0), f"z max err {err:.3e}"
    zz = z.cpu().double()
    rm_want, rv_want = rm0.clone(), rv0.clone()
    for k in range(groups):
        zk = zz[k * per:(k + 1) * per].reshape(-1, Cout)
        m64, v64 = zk.mean(0), zk.var(0, unbiased=False)
        torch.testing.assert_close(mean[k].cpu().double(), m64, rtol=1e-5, atol=1e-6, msg=f"group {k} mean")
        torch.testing.assert_close(invstd[k].cpu().double(), 1.0 / torch.sqrt(v64 + 1e-5), rtol=1e-5, atol=1e-6, msg=f"group {k} invstd")
        n = zk.shape[0]
        rm_want = 0.9 * rm_want + 0.1 * m64
        rv_want = 0.9 * rv_want + 0.1 * v64 * n / (n - 1)
    torch.testing.assert_close(rm.cpu().double(), rm_want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.cpu().double(), rv_want, rtol=1e-5, atol=1e-6)
    assert int(nbt.item()) == groups


# (B over all groups, Cin, Cout, H, groups): the grad-input of a k4 s2 p1 conv with four equal phases of (H/2)^2 pixels
GROUPED_DGRAD = [(4, 64, 36, 16, 2), (6, 64, 68, 16, 3), (8, 128, 36, 16, 4), (16, 128, 68, 16, 8), (4, 256, 132, 16, 2)]


@pytest.mark.parametrize("act,slope", ACTS[:2])
@pytest.mark.parametrize("B,Cin,Cout,H,groups", GROUPED_DGRAD)
def test_grouped_bnbwd_against_float64(pcg, B, Cin, Cout, H, groups, act, slope):
    """dgrad_bnbwd_g + bn_bwd_partial_g: each group masked by and summed against its own statistics (mean / invstd [groups][Cin])."""
    ops = pcg.ops
    shape = (B, Cin, Cout, H, H, 4, 4, 2, 1)
    g = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    assert ops.group_dgrad_ok(g, groups)
    x, w, dy, _, _ = _operands(shape, 800 + B + groups)
    gen = torch.Generator().manual_seed(B + groups)
    per = B // groups
    z = torch.cat([_randn(per, H, H, Cin, g=gen, scale=1.0 + 0.4 * k) + 0.3 * (k - 1) for k in range(groups)])
    mean = torch.stack([z[k * per:(k + 1) * per].reshape(-1, Cin).mean(0) for k in range(groups)]).float().double()
    invstd = torch.stack([1.0 / torch.sqrt(z[k * per:(k + 1) * per].reshape(-1, Cin).var(0, unbiased=False) + 1e-5)
                          for k in range(groups)]).float().double()
    gamma = (torch.rand(Cin, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = _randn(Cin, g=gen, scale=0.1)
    dgd, dbd = torch.zeros(Cin, device=dev()), torch.zeros(Cin, device=dev())
    dm, partial, nparts, nph = ops.conv_bwd_data_fused_g(g, _on_dev(_nhwc(dy)), _on_dev(_nhwc(w)), act, slope, _on_dev(z),
                                                         (_on_dev(mean), _on_dev(invstd), _on_dev(gamma), _on_dev(beta)), groups)
    dz = ops.bn_bwd_partial_g(dm, _on_dev(z), Cin, _on_dev(mean), _on_dev(invstd), _on_dev(gamma), partial, nparts, nph, dgd, dbd, False,
                              groups)
    conv = _dgrad64(x.shape, w, dy, 2, 1)
    dm64 = dm.cpu().double()
    dg_want, db_want = torch.zeros(Cin, dtype=torch.float64), torch.zeros(Cin, dtype=torch.float64)
    for k in range(groups):
        sl = slice(k * per, (k + 1) * per)
        sc, sh = _fold32(mean[k], invstd[k], gamma, beta)
        pre = _pre32(z[sl], sc, sh)
        near = pre.abs() <= 1e-6
        assert int(near.sum()) <= max(4, 1e-4 * near.numel()), f"group {k}: {int(near.sum())} elements at the kink"
        d = (dm64[sl] - conv[sl] * torch.where(pre > 0, 1.0, slope)).abs()
        assert float(d[~near].max()) <= _tol(16 * Cout, 4.0), f"group {k}: masked output max err {float(d[~near].max()):.3e}"
        dz_k, dg_k, db_k = _bn_bwd64(dm64[sl], z[sl], mean[k], invstd[k], gamma)
        _check_dz(dz[sl], dz_k)
        dg_want += dg_k
        db_want += db_k
    _check_sums(dgd, dbd, dg_want, db_want)                 # the parameters are shared: the groups' sums add up


# ---- 4: weight adjoints ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Cout,KH,KW,Cin", [(12, 64, 3, 3, 64), (16, 20, 5, 3, 36), (1, 132, 4, 4, 68), (3, 4, 1, 1, 516)])
def test_weight_adjoint_many_against_flip_transpose(pcg, n, Cout, KH, KW, Cin):
    """conv_weight_adjoint_many: bit-equal to per-tensor conv_weight_adjoint and to w[co][kh][kw][ci] -> [ci][KH-1-kh][KW-1-kw][co]."""
    ops = pcg.ops
    gen = torch.Generator().manual_seed(n * 7 + Cout)
    ws = [torch.randn(Cout, KH, KW, Cin, generator=gen).to(dev()) for _ in range(n)]
    many = ops.conv_weight_adjoint_many(ws)
    assert len(many) == n
    for w, wa in zip(ws, many):
        want = w.cpu().double().flip(1, 2).permute(3, 1, 2, 0)
        assert torch.equal(wa.cpu().double(), want)
        assert torch.equal(wa, ops.conv_weight_adjoint(w))
