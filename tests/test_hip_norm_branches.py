"""GPU parity of the normalisation layer -- csrc/batchnorm.hip, csrc/instnorm.hip and the spectral-norm bodies of
csrc/spectral_norm_body.h (launched from csrc/tabular.hip) -- against float64 (tests/norm_ref.py), at every host-side switch that
chooses a kernel, a template instantiation or a path inside one.

Every case names the route it is meant to take and asserts it through pcg_launch_plan_describe (ops.launch_plan) before it runs;
tests/test_norm_plan_host.py checks the same tables, the references and the mask-gap condition without a device.

Inputs are rounded to float32 before the float64 reference is built.  Output buffers the test owns are pre-filled with a sentinel
and carry a sentinel tail that must survive; inputs are compared with a copy afterwards.  "Misaligned" is a view one float past a
16-byte boundary.

Out of scope here: the grouped `_g` BatchNorm forms (tests/test_hip_groups.py), partial rows produced by the conv epilogues
(tests/test_hip_igemm_branches.py; the partial rows below are synthesised), and the exact global-batch mode, which needs several ranks.

Bounds, per output element, in float64, u = 2^-24 (derivations in the docstrings of tests/norm_ref.py):
  BatchNorm statistics   save_mean / save_invstd: the float32 rounding of the float64 value to within 1 ulp (the sums are fp64 over
                         exact fp32 inputs; this is what the mean-100 / std-0.01 channel checks); running statistics
                         3 u (|(1 - m) r| + |m s|); the folded coef from the saved values: u |sc| and u (2 |mean sc| + |beta|)
  BatchNorm apply        c u (|x sc| + |mean sc| + |beta|) through the activation's slope, c = 3 (6 for the var_eps form, which takes
                         1 / sqrtf itself), + u |a| for the LeakyReLU product, + u (|alpha a| + |residual|) for the residual fma
  BatchNorm backward     dbeta 2 u sum|dz| + u |sum|, dgamma 4 u sum|dz xh| + u |sum| (fp64 sums of fp32 terms; an accumulating add
                         one more rounding); dx u |k0| (6 |dz| + 5 |k1| + 2 mean|dz| + 7 |xh k2| + 4 |xh| mean|dz xh|); dcol the sum
                         of dx's bounds + one rounding; colsum one rounding
  InstanceNorm           reductions (np + lanes + 2) u sum|terms| with both numbers read off the plan, carried to first order through
                         every expression behind them; rsqrtf: RSQRT_U u (measured, see below).  Where the older test of these kernels
                         has a tolerance for the same output (y, dx, ddy, ez and the parameter gradients summed over the batch),
                         the bound is the smaller of the two (norm_ref.in_bound): a worst case over 256 lanes exceeds it
  spectral norm          the tolerances of test_spectral_norm_matches_torch, now against float64: 1e-5 / 1e-6 for u, v, w_bar and
                         sigma, 2e-4 with 1e-5 max|dW| for dW (per pass of an accumulating sequence, + one rounding)

rsqrtf belongs to the toolchain: the measured max |invstd_device / invstd_float64 - 1| over all InstanceNorm table cases on the MI355X is
3.429 u (0.9 to 2.9 u for the other cases; test_instnorm_forward prints it per case); the allowance RSQRT_U is twice that, rounded up
to whole u: 7 u, under the cap of 8 u.
"""
import math
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
SENT = -77.0
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2
MEASURED_RSQRT = 3.429       # max |invstd_device / invstd_float64 - 1| in units of u over IN_CASES on the MI355X (the C = 8, HW = 169 case)
RSQRT_U = 7                  # min(8, ceil(2 * MEASURED_RSQRT))

# =================================================================================================================================
# Case tables.  Host data only -- tests/test_norm_plan_host.py imports them.
# =================================================================================================================================
# (rows, C, misaligned, column-reduce route, apply route, backward-apply route [with column sums where the fast kernel fuses them])
_T = "temporal stores, thread 0: "
BN_CASES = [
    (5, 8, False, "float4: 2 x 128 threads, 1 channel pass, 1 block of 512 rows", f"fast<2>: 1 block, {_T}0 main trips + tail of 1",
     f"fast<2>: 1 block, {_T}0 main trips + tail of 1"),                                              # one ragged row block
    (2, 4, False, "float4: 1 x 256 threads, 1 channel pass, 1 block of 1024 rows", f"fast<2>: 1 block, {_T}0 main trips + tail of 1",
     f"fast<2>: 1 block, {_T}0 main trips + tail of 1"),                                              # the smallest training batch
    (1000, 8, False, "float4: 2 x 128 threads, 1 channel pass, 2 blocks of 512 rows", f"fast<2>: 4 blocks, {_T}1 main trip + tail of 0",
     f"fast<2>: 4 blocks, {_T}1 main trip + tail of 0"),                                              # second row block: 488 rows
    (37, 10, False, "scalar: 8 x 32 threads, 2 channel passes, 1 block of 128 rows", "scalar lanes: 2 blocks of 256: 1 pass",
     "scalar lanes: 2 blocks of 256: 1 pass"),
    (1000, 36, False, "float4: 8 x 32 threads, 2 channel passes, 8 blocks of 128 rows", "float4 lanes: 36 blocks of 256: 1 pass",
     "float4 lanes: 36 blocks of 256: 1 pass"),                                                       # generic float4, CG = 9
    (1000, 1024, False, "float4: 256 x 1 threads, 1 channel pass, 250 blocks of 4 rows", f"fast<2>: 500 blocks, {_T}1 main trip + tail of 0",
     f"fast<2>: 500 blocks, {_T}1 main trip + tail of 0"),                                            # TY = 1; 250 partial rows
    (2051, 1024, False, "float4: 256 x 1 threads, 1 channel pass, 411 blocks of 5 rows", f"fast<2>: 1026 blocks, {_T}1 main trip + tail of 0",
     f"fast<2>: 1024 blocks, {_T}1 main trip + tail of 1"),                                           # last block one row
    (300, 1028, False, "float4: 256 x 1 threads, 2 channel passes, 75 blocks of 4 rows", "float4 lanes: 302 blocks of 256: 1 pass",
     "float4 lanes: 302 blocks of 256: 1 pass"),                                                      # CG = 257 > TX
    (64, 2048, False, "float4: 256 x 1 threads, 2 channel passes, 16 blocks of 4 rows", "float4 lanes: 128 blocks of 256: 1 pass",
     "float4 lanes: 128 blocks of 256: 1 pass"),                                                      # C/4 = 512: a power of two, not fast
    (777, 64, True, "scalar: 64 x 4 threads, 1 channel pass, 49 blocks of 16 rows", "scalar lanes: 195 blocks of 256: 1 pass",
     "scalar lanes: 195 blocks of 256: 1 pass"),                                                      # scalar despite C % 4 == 0
]
BN_COLSUM_ONLY = (8200, 256, "float4: 64 x 4 threads, 1 channel pass, 483 blocks of 17 rows",
                  f"fast<2>: 1024 blocks, {_T}1 main trip + tail of 1")        # 1025 blocks wanted against the cap: main loop plus tail
BN_FINALIZE_OF_CASE = {(1000, 1024): "256 threads, 1 eight-deep trip", (2051, 1024): "256 threads, 1 eight-deep trip",
                       (5, 8): "256 threads, 0 eight-deep trips"}
# nparts -> finalize route of pcg_bn_bwd_partial*
BN_PARTIAL_NPARTS = {1: "256 threads, 0 eight-deep trips", 1025: "1024 threads, 1 eight-deep trip",
                     2048: "presum: 256 chunks of 8 rows, 256 threads, 1 eight-deep trip",
                     2049: "presum: 228 chunks of 9 rows, 256 threads, 1 eight-deep trip"}
BN_PARTIAL_SHAPES = [(300, 8), (300, 36)]
# knob child: (rows, C); env -> text the child's apply route of (1000, 64) must contain
BN_KNOB_SHAPES = [(1000, 8), (1000, 64), (1001, 256)]
BN_KNOB_SETTINGS = [({"PCG_BN_DEPTH": "4", "PCG_BN_NT": "1", "PCG_BN_BLOCKS": "3"}, "fast<4>: 3 blocks, non-temporal stores, thread 0: 5 main trips + tail of 1"),
                    ({"PCG_BN_DEPTH": "2", "PCG_BN_NT": "0", "PCG_BN_BLOCKS": "1"}, "fast<2>: 1 block, temporal stores, thread 0: 31 main trips + tail of 1")]

# (C, HW, misaligned x, forward / backward route, backward-of-backward route); B = 2 throughout
IN_B = 2
IN_CASES = [
    (4, 169, False, "reg<1>: 4 channels x 256 lanes, grid 2 x 1", "reg<1>: 4 channels x 256 lanes, grid 2 x 1"),
    (8, 169, False, "reg<2>: 8 channels x 128 lanes, grid 2 x 1", "reg<2>: 8 channels x 128 lanes, grid 2 x 1"),
    (256, 4, False, "reg<1>: 256 channels x 4 lanes, grid 2 x 1", "reg<1>: 256 channels x 4 lanes, grid 2 x 1"),
    (384, 4, False, "reg<1>: 128 channels x 8 lanes, grid 2 x 3", "reg<1>: 128 channels x 8 lanes, grid 2 x 3"),
    (128, 6, False, "reg<1>: 128 channels x 8 lanes, grid 2 x 1", "reg<1>: 128 channels x 8 lanes, grid 2 x 1"),
    (64, 25, False, "reg<2>: 64 channels x 16 lanes, grid 2 x 1", "reg<2>: 64 channels x 16 lanes, grid 2 x 1"),
    (64, 40, False, "reg<3>: 64 channels x 16 lanes, grid 2 x 1", "reg<3>: 64 channels x 16 lanes, grid 2 x 1"),
    (64, 49, False, "reg<2>: 32 channels x 32 lanes, grid 2 x 2", "reg<6>: 64 channels x 16 lanes, grid 2 x 1"),
    (64, 169, False, "reg<6>: 32 channels x 32 lanes, grid 2 x 2", "reg<12>: 64 channels x 16 lanes, grid 2 x 1"),
    (64, 196, False, "reg<12>: 32 channels x 32 lanes, grid 2 x 2", "stream<4>: 64 channels x 16 lanes, grid 2 x 1"),
    (32, 200, False, "reg<12>: 32 channels x 32 lanes, grid 2 x 1", "reg<12>: 32 channels x 32 lanes, grid 2 x 1"),
    (64, 400, False, "stream<4>: 64 channels x 16 lanes, grid 2 x 1", "stream<4>: 64 channels x 16 lanes, grid 2 x 1"),
    (100, 30, False, "reg<2>: 64 channels x 16 lanes, grid 2 x 2", "reg<2>: 64 channels x 16 lanes, grid 2 x 2"),   # 36 live channels in block 2
    (6, 15, False, "stream<1>: 8 channels x 32 lanes, grid 2 x 1", "stream<1>: 8 channels x 32 lanes, grid 2 x 1"),
    (70, 9, False, "stream<1>: 64 channels x 4 lanes, grid 2 x 2", "stream<1>: 64 channels x 4 lanes, grid 2 x 2"),
    (1, 2, False, "stream<1>: 1 channels x 256 lanes, grid 2 x 1", "stream<1>: 1 channels x 256 lanes, grid 2 x 1"),
    (64, 25, True, "stream<1>: 64 channels x 4 lanes, grid 2 x 1", "stream<1>: 64 channels x 4 lanes, grid 2 x 1"),   # by alignment
]
IN_OPTIONAL_OUTPUT_CASES = [(64, 25, False), (64, 400, False), (6, 15, False)]       # one per kernel form: reg, stream<4>, stream<1>

# (O, I, forward route, backward route)
SN_CASES = [
    (32, 21, "LDS image: 672 of 12288 floats, row stride 21", "one burst: 672 of 8192 elements"),
    (64, 128, "LDS image: 8256 of 12288 floats, row stride 129", "one burst: 8192 of 8192 elements"),
    (128, 65, "LDS image: 8320 of 12288 floats, row stride 65", "loops: 8320 elements exceed 8192"),
    (96, 127, "LDS image: 12192 of 12288 floats, row stride 127", "loops: 12192 elements exceed 8192"),
    (96, 128, "global memory: 12384 floats exceed 12288, row stride 129", "loops: 12288 elements exceed 8192"),
    (256, 256, "global memory: 65792 floats exceed 12288, row stride 257", "loops: 65536 elements exceed 8192"),
    (1, 256, "LDS image: 257 of 12288 floats, row stride 257", "one burst: 256 of 8192 elements"),
    (256, 1, "LDS image: 256 of 12288 floats, row stride 1", "one burst: 256 of 8192 elements"),
]
SN_BATCHED = [(64, 128), (96, 128)]          # an LDS-form and a global-form layer in one launch


def all_routes():
    """[(plan op name, args, expected text)] of every table above."""
    out = []
    for rows, C, mis, cols, apply_, bwd in BN_CASES:
        al = int(not mis)
        out += [("BN_COLREDUCE", (rows, C, al), cols), ("BN_APPLY", (0, rows, C, al), apply_), ("BN_APPLY", (2, rows, C, al), bwd)]
        if not bwd.startswith("fast") or "1024 blocks" not in bwd:
            out.append(("BN_APPLY", (1, rows, C, al), bwd))      # without column sums: the same route unless the 1024 cap bit
    rows, C, cols, bwd = BN_COLSUM_ONLY
    out += [("BN_COLREDUCE", (rows, C, 1), cols), ("BN_APPLY", (2, rows, C, 1), bwd)]
    for (rows, C), want in BN_FINALIZE_OF_CASE.items():
        nblocks = int(re.search(r"(\d+) blocks? of", dict(((c[0], c[1]), c[3]) for c in BN_CASES)[(rows, C)]).group(1))
        out.append(("BN_FINALIZE", (nblocks,), want))
    out += [("BN_FINALIZE", (n,), want) for n, want in BN_PARTIAL_NPARTS.items()]
    for C, HW, mis, fwd, bb in IN_CASES:
        out += [("INSTNORM", (0, IN_B, HW, C, int(not mis)), fwd), ("INSTNORM", (1, IN_B, HW, C, int(not mis)), fwd),
                ("INSTNORM", (2, IN_B, HW, C, int(not mis)), bb)]
    for O, I, fwd, bwd in SN_CASES:
        out += [("SPECTRAL_NORM", (0, O, I), fwd), ("SPECTRAL_NORM", (1, O, I), bwd)]
    return out


# the routes this file is there to cover: (plan op, pattern), each reached by at least one case (checked on the host as well)
REQUIRED_ROUTES = (
    [("BN_COLREDUCE", p) for p in (r"^float4: .* 1 channel pass", r"^float4: 8 x 32 threads, 2 channel passes", r"^scalar: .* 2 channel passes",
                                   r"^float4: 256 x 1 threads, 2 channel passes", r"^float4: 256 x 1 threads, 1 channel pass, 250 blocks",
                                   r"411 blocks of 5 rows", r"^scalar: 64 x 4 threads, 1 channel pass, 49 blocks", r"2 blocks of 512 rows")] +
    [("BN_APPLY", p) for p in (r"^fast<2>: 1 block,", r"^fast<2>: .*1 main trip \+ tail of 1$", r"^fast<2>: 1024 blocks", r"^float4 lanes: ", r"^scalar lanes: ")] +
    [("BN_FINALIZE", p) for p in (r"^256 threads, 0 eight-deep", r"^256 threads, 1 eight-deep", r"^1024 threads, 1 eight-deep",
                                  r"^presum: 256 chunks of 8 rows, 256 threads", r"^presum: 228 chunks of 9 rows, 256 threads")] +
    [("INSTNORM", p) for p in (r"^reg<1>: 4 channels x 256 lanes", r"^reg<2>: 8 channels x 128 lanes", r"^reg<1>: 256 channels x 4 lanes",
                               r"^reg<1>: 128 channels x 8 lanes, grid 2 x 3", r"^reg<2>: 64 channels", r"^reg<3>: ", r"^reg<2>: 32 channels x 32 lanes",
                               r"^reg<6>: 32 channels", r"^reg<6>: 64 channels", r"^reg<12>: 32 channels", r"^reg<12>: 64 channels", r"^stream<4>: ",
                               r"^stream<1>: 8 channels", r"^stream<1>: 64 channels x 4 lanes, grid 2 x 2", r"^stream<1>: 1 channels",
                               r"^stream<1>: 64 channels x 4 lanes, grid 2 x 1")] +
    [("SPECTRAL_NORM", p) for p in (r"^LDS image: ", r"^LDS image: 12192 of 12288", r"^global memory: 12384", r"^global memory: 65792",
                                    r"^one burst: 8192 of 8192", r"^loops: 8320 ")])


def plan(op, *args):
    from pcgan_amd import _lib, ops
    return ops.launch_plan(getattr(_lib, "PLAN_" + op), *[int(a) for a in args])


def assert_route(op, args, want):
    got = plan(op, *args)
    assert got == want, f"route moved: {op}{tuple(args)} takes {got!r}, the case expects {want!r}"


def check_all_routes():
    seen = []
    for op, args, want in all_routes():
        assert_route(op, args, want)
        seen.append((op, want))
    for op, pat in REQUIRED_ROUTES:
        assert any(o == op and re.search(pat, s) for o, s in seen), f"no case reaches a {op} route like {pat!r}"
    # the backward-of-backward differs from the other passes only through `wide13`; Reg<2> and Stream<4> are reached in every pass
    for p in (0, 1, 2):
        texts = [plan("INSTNORM", p, IN_B, HW, C, int(not mis)) for C, HW, mis, _, _ in IN_CASES]
        for form in ("reg<1>", "reg<2>", "reg<3>", "reg<6>", "reg<12>", "stream<4>", "stream<1>"):
            assert any(t.startswith(form) for t in texts), f"pass {p}: no case reaches {form}"


# =================================================================================================================================
# host-side inputs and references (no device): shared by the GPU tests and tests/test_norm_plan_host.py
# =================================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gapped(*shape, g):
    """+-(0.2 + |randn|) / 1.165: about unit variance, nothing within 0.17 of zero."""
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return s * (0.2 + torch.randn(*shape, generator=g, dtype=torch.float64).abs()) / 1.165


def _signed(n, lo, hi, g):
    return (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1) * (lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64))


BN_SEED_SHIFT = {(5, 8): 1}         # shapes whose first seed put a pre-activation of the mean-100 channel inside the mask gap


@lru_cache(maxsize=4)
def bn_inputs(rows, C):
    """x with the two hard channels (0: constant 0.75; 1: mean 100, standard deviation 0.01), gamma of either sign in 0.75..1.25, a small
    beta (+-0.5 on the constant channel, whose output is beta), dy, a residual, running statistics."""
    g = _gen(7 * rows + C + 100000 * BN_SEED_SHIFT.get((rows, C), 0))
    x = (0.3 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)) + (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * _gapped(rows, C, g=g)
    x[:, 0] = 0.75
    x[:, 1] = 100.0 + 0.01 * _gapped(rows, g=g)
    gamma, beta = _signed(C, 0.75, 1.25, g), _signed(C, 0.0, 0.03, g)
    beta[0] = 0.5 if beta[0] > 0 else -0.5
    d = dict(x=x, gamma=gamma, beta=beta, dy=torch.randn(rows, C, generator=g, dtype=torch.float64),
             res=torch.randn(rows, C, generator=g, dtype=torch.float64), rm0=torch.randn(C, generator=g, dtype=torch.float64),
             rv0=1 + torch.rand(C, generator=g, dtype=torch.float64))
    d = {k: R.f32_exact(v) for k, v in d.items()}
    st = R.bn_stats(d["x"], EPS, MOM, d["rm0"], d["rv0"])
    d["stats"] = st
    d["mean32"], d["invstd32"], d["var32"] = R.f32_exact(st["mean"]), R.f32_exact(st["invstd"]), R.f32_exact(st["var"])
    return d


# the forms of pcg_bn_apply_act each case runs: (statistics form, activation, residual with alpha = 0.7, gamma / beta given)
BN_APPLY_FORMS = [("train", ACT_NONE, False, True), ("train", ACT_RELU, True, True), ("train", ACT_LRELU, False, False),
                  ("train", ACT_LRELU, True, True), ("eval", ACT_LRELU, True, True), ("eval", ACT_RELU, False, True), ("eval", ACT_NONE, False, False)]
# of pcg_bn_act_bwd*: (mask source "y" | "premask" | None, activation, dy_scale, accumulate, dcol: None | accumulate_col)
BN_BWD_FORMS = [("y", ACT_LRELU, 1.0, False, None), ("premask", ACT_RELU, 0.5, True, True), (None, ACT_NONE, 0.5, True, False),
                ("y", ACT_RELU, 1.0, True, None), ("premask", ACT_LRELU, 1.0, False, False)]


def bn_apply_ref(d, form):
    stat_form, act, res, affine = form
    return R.bn_apply(d["x"], d["mean32"], d["invstd32"] if stat_form == "train" else d["var32"], d["gamma"] if affine else None,
                      d["beta"] if affine else None, act, SLOPE, d["res"] if res else None, 0.7 if res else 1.0, -1.0 if stat_form == "train" else EPS)


def bn_pre(d, act):
    """The pre-activation (and its bound) the masks of the backward come from: training statistics, gamma and beta given."""
    return R.bn_apply(d["x"], d["mean32"], d["invstd32"], d["gamma"], d["beta"], act, SLOPE)


def bn_mask_gaps(rows, C):
    """[(what, ok, count)] of the mask-gap condition for every pre-activation the case's calls take a mask from."""
    d = bn_inputs(rows, C)
    out = []
    for form in BN_APPLY_FORMS:
        r = bn_apply_ref(d, form)
        out.append((f"bn apply {rows}x{C} {form}",) + R.mask_gap_ok(r["pre"], r["pre_bound"]))
    return out


IN_SEED_SHIFT = {(4, 169): 2, (1, 2): 1}


@lru_cache(maxsize=4)
def in_inputs(C, HW):
    g = _gen(1000 * C + HW + 100000 * IN_SEED_SHIFT.get((C, HW), 0))
    B = IN_B
    x = (0.3 + 0.5 * torch.randn(B, 1, C, generator=g, dtype=torch.float64)) + (0.5 + torch.rand(B, 1, C, generator=g, dtype=torch.float64)) * _gapped(B, HW, C, g=g)
    x[0, :, 0] = 0.75                                                        # one constant map: variance 0
    gamma, beta = _signed(C, 0.75, 1.25, g), _signed(C, 0.02, 0.05, g)
    d = dict(x=x, gamma=gamma, beta=beta)
    for k in ("dy", "r", "add", "cot"):
        d[k] = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    return {k: R.f32_exact(v) for k, v in d.items()}


def in_plan_numbers(text, HW):
    """(positions per lane, lanes) of an InstanceNorm route."""
    lanes = int(re.search(r"x (\d+) lanes", text).group(1))
    return -(-HW // lanes), lanes


def in_refs(C, HW, fwd_route, bb_route, rsqrt_u=RSQRT_U):
    """The by-hand references and bounds of one case, with the reduction constants of its routes."""
    d = in_inputs(C, HW)
    f = R.instnorm_fwd(d["x"], d["gamma"], d["beta"], EPS, *in_plan_numbers(fwd_route, HW), rsqrt_u)
    f2 = R.instnorm_fwd(d["x"], d["gamma"], d["beta"], EPS, *in_plan_numbers(bb_route, HW), rsqrt_u)     # K of the backward-of-backward; xh from the forward's
    f2 = dict(f, K=f2["K"])
    neg = R.f32_scalar(SLOPE)
    mask = torch.where(f["n"] > 0, torch.ones_like(f["n"]), torch.full_like(f["n"], neg))
    return dict(d=d, f=f, f2=f2, mask=mask, bwd=R.instnorm_bwd(f, d["dy"], d["gamma"]),
                fused=R.instnorm_bwd(f, R.f32_exact(d["cot"] * mask), d["gamma"], d_rounded=False, add=d["add"]),
                bare=R.instnorm_bwd(f, d["dy"], d["gamma"]), bb=R.instnorm_bwd_bwd(f2, d["r"], d["dy"], d["gamma"]))


def in_mask_gap(C, HW, fwd_route):
    d = in_inputs(C, HW)
    f = R.instnorm_fwd(d["x"], d["gamma"], d["beta"], EPS, *in_plan_numbers(fwd_route, HW), RSQRT_U)
    return R.mask_gap_ok(f["n"], f["n_bound"])


@lru_cache(maxsize=2)
def sn_inputs(O, I):
    g = _gen(300 * O + I)
    W = (torch.rand(O, I, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(I)
    u, v = torch.randn(O, generator=g, dtype=torch.float64), torch.randn(I, generator=g, dtype=torch.float64)
    d = dict(W=W, u=u / u.norm(), v=v / v.norm(), dwbar=[torch.randn(O, I, generator=g, dtype=torch.float64) for _ in range(2)],
             dW0=torch.randn(O, I, generator=g, dtype=torch.float64))
    return {k: ([R.f32_exact(t) for t in v_] if isinstance(v_, list) else R.f32_exact(v_)) for k, v_ in d.items()}


def sn_reference(O, I):
    """Two training forwards (with the gradient of <dwbar_k, w_bar>) and one evaluation forward of the float64 module."""
    d = sn_inputs(O, I)
    lin = R.sn_module(d["W"], d["u"], d["v"])
    lin.train()
    calls = [R.sn_forward(lin, d["dwbar"][k]) for k in range(2)]
    lin.eval()
    return d, calls, R.sn_forward(lin)


# =================================================================================================================================
# device helpers
# =================================================================================================================================
@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd


def _dev(t):
    return t.float().to(DEV).contiguous()


def _off_by_one_float(t):
    """A contiguous device copy of t whose storage starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t.float())
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _place(t, misaligned):
    return _off_by_one_float(t) if misaligned else _dev(t)


def _out_like(shape, misaligned=False):
    """(buffer, view): a sentinel-filled output view with 8 sentinel floats behind it (and one in front when misaligned)."""
    n = int(np.prod(shape))
    lead = 1 if misaligned else 0
    buf = torch.full((lead + n + 8,), SENT, dtype=torch.float32, device=DEV)
    v = buf[lead:lead + n].view(shape)
    assert v.data_ptr() % 16 == (4 if misaligned else 0)
    return buf, v


def _untouched(buf, view, what):
    n, lead = view.numel(), (view.data_ptr() - buf.data_ptr()) // 4
    assert bool((buf[:lead] == SENT).all()) and bool((buf[lead + n:] == SENT).all()), f"{what}: wrote outside its output"
    assert not bool((view == SENT).any()), f"{what}: left part of its output unwritten"


def _within(got, ref, bound, what):
    """|got - ref| <= bound per element, in float64; prints the worst ratio before it asserts."""
    got = got.detach().double().cpu().reshape(-1)
    bound = (torch.broadcast_to(bound.double(), ref.shape).reshape(-1) if torch.is_tensor(bound) else torch.full((ref.numel(),), float(bound), dtype=torch.float64))
    ref = ref.double().reshape(-1)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    print(f"{what}: worst err/bound {float(ratio[worst]):.3g} (err {float(err[worst]):.3g}, bound {float(bound[worst]):.3g}) at {worst}")
    assert float(ratio[worst]) <= 1.0, f"{what}: |err| {float(err[worst]):.3e} > bound {float(bound[worst]):.3e} at flat index {worst}"


def _one_ulp(got, ref64, what):
    """got equals the float32 rounding of ref64 to within 1 ulp."""
    ref32 = R.f32_exact(ref64)
    _within(got, ref32, R.ulp32(ref32), what)


def _bn_id(c):
    return f"{c[0]}x{c[1]}{'-misaligned' if c[2] else ''}"


# =================================================================================================================================
# BatchNorm
# =================================================================================================================================
@pytest.mark.parametrize("case", BN_CASES, ids=_bn_id)
def test_bn_train_stats(pcg, case):
    """pcg_bn_train_stats(_coef) and pcg_colsum on the case's column-reduce route: save_mean / save_invstd within 1 ulp of the float64
    value (the constant channel exercises the variance clamp, the mean-100 channel the fp64 sums), the running statistics, the
    batch counter, the folded coef."""
    rows, C, mis, cols, _, _ = case
    ops = pcg.ops
    assert_route("BN_COLREDUCE", (rows, C, int(not mis)), cols)
    if (rows, C) in BN_FINALIZE_OF_CASE:
        assert_route("BN_FINALIZE", (int(re.search(r"(\d+) blocks? of", cols).group(1)),), BN_FINALIZE_OF_CASE[(rows, C)])
    d = bn_inputs(rows, C)
    st = d["stats"]
    xd = _place(d["x"], mis)
    x0 = xd.clone()
    rm, rv, nbt = _dev(d["rm0"]), _dev(d["rv0"]), torch.full((1,), 41, dtype=torch.int64, device=DEV)
    gd, bd = _dev(d["gamma"]), _dev(d["beta"])
    mean, invstd, coef = ops.bn_train_stats(xd, C, EPS, MOM, rm, rv, nbt, gamma=gd, beta=bd)
    _one_ulp(mean, st["mean"], f"save_mean {rows}x{C}")
    _one_ulp(invstd, st["invstd"], f"save_invstd {rows}x{C}")
    _within(rm, st["rm"], st["rm_bound"], "running_mean")
    _within(rv, st["rv"], st["rv_bound"], "running_var")
    assert int(nbt) == 42
    m32, i32 = mean.double().cpu(), invstd.double().cpu()              # coef is folded from the saved float32 values
    sc = d["gamma"] * i32
    _within(coef[:C], sc, U * sc.abs(), "coef scale")
    _within(coef[C:], d["beta"] - m32 * sc, U * (2 * (m32 * sc).abs() + d["beta"].abs()), "coef shift")
    mean2, invstd2 = ops.bn_train_stats(xd, C, EPS, MOM)               # no running statistics, no coef: the same statistics
    assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd) and torch.equal(xd, x0)
    # pcg_colsum over the same plan, accumulating and not
    dyd = _place(d["dy"], mis)
    s = d["dy"].sum(0)
    for acc in (False, True):
        db = torch.full((C,), 0.5, dtype=torch.float32, device=DEV)
        ops.colsum(rows, C, dyd, db, acc)
        want = s + 0.5 if acc else s
        _within(db, want, U * s.abs() + (U * want.abs() if acc else 0.0), f"colsum {rows}x{C} acc={acc}")


@pytest.mark.parametrize("case", BN_CASES, ids=_bn_id)
def test_bn_apply_act(pcg, case):
    """pcg_bn_apply_act on the case's apply route: training statistics and the var_eps evaluation form, no activation / ReLU /
    LeakyReLU, with residual and alpha = 0.7 and without, gamma / beta given and absent."""
    rows, C, mis, _, route, _ = case
    ops = pcg.ops
    assert_route("BN_APPLY", (0, rows, C, int(not mis)), route)
    d = bn_inputs(rows, C)
    xd, resd = _place(d["x"], mis), _dev(d["res"])
    x0 = xd.clone()
    md, isd, vd, gd, bd = (_dev(d[k]) for k in ("mean32", "invstd32", "var32", "gamma", "beta"))
    for form in BN_APPLY_FORMS:
        stat_form, act, res, affine = form
        ref = bn_apply_ref(d, form)
        ok, n_bad = R.mask_gap_ok(ref["pre"], ref["pre_bound"])
        assert ok, f"{form}: {n_bad} pre-activations of the reference lie within 8 bounds of zero"
        buf, y = _out_like((rows, C))
        ops.bn_apply_act(xd, C, md, isd if stat_form == "train" else vd, gd if affine else None, bd if affine else None, act, SLOPE,
                         var_eps=-1.0 if stat_form == "train" else EPS, out=y, residual=resd if res else None, alpha=0.7 if res else 1.0)
        _untouched(buf, y, f"bn_apply_act {form}")
        _within(y, ref["out"], ref["bound"], f"bn_apply_act {rows}x{C} {form}")
    assert torch.equal(xd, x0)


def _run_bn_bwd(ops, d, rows, C, mis, form, fused_route=None):
    src, act, dy_scale, acc, col = form
    pre = bn_pre(d, act)
    ok, n_bad = R.mask_gap_ok(pre["pre"], pre["pre_bound"])
    assert ok, f"{n_bad} pre-activations of the reference lie within 8 bounds of zero"
    ref = R.bn_bwd(d["dy"], d["x"], d["mean32"], d["invstd32"], d["gamma"], pre["pre"], act, SLOPE, dy_scale)
    xd, dyd = _place(d["x"], mis), _dev(d["dy"])
    md, isd, gd, bd = (_dev(d[k]) for k in ("mean32", "invstd32", "gamma", "beta"))
    yd = ops.bn_apply_act(xd, C, md, isd, gd, bd, act, SLOPE) if src == "y" else None
    buf, dx = _out_like((rows, C), mis)
    dg, db = torch.full((C,), 0.25, dtype=torch.float32, device=DEV), torch.full((C,), -0.5, dtype=torch.float32, device=DEV)
    dcol = torch.full((C,), 0.125, dtype=torch.float32, device=DEV) if col is not None else None
    x0, dy0 = xd.clone(), dyd.clone()
    ops.bn_act_bwd(dyd, xd, yd, C, md, isd, gd, act, SLOPE, dg, db, acc, out=dx, dy_scale=dy_scale, beta=bd if src == "premask" else None,
                   dcol=dcol, accumulate_col=bool(col))
    tag = f"bn_act_bwd {rows}x{C} {form}"
    _untouched(buf, dx, tag)
    assert torch.equal(xd, x0) and torch.equal(dyd, dy0)
    _within(dx, ref["dx"], ref["dx_bound"], tag + " dx")
    for name, got, old in (("dgamma", dg, 0.25), ("dbeta", db, -0.5)):
        want, bound = R.accumulated(ref[name], ref[name + "_bound"], old) if acc else (ref[name], ref[name + "_bound"])
        _within(got, want, bound, f"{tag} {name}")
    if col is not None:
        want, bound = R.accumulated(ref["dcol"], ref["dcol_bound"], 0.125) if col else (ref["dcol"], ref["dcol_bound"])
        _within(dcol, want, bound, tag + " dcol")
        # the column sums are those of the dx the kernel wrote: fp64 sum, one rounding (and the add's)
        s = dx.double().sum(0).cpu()
        want = s + 0.125 if col else s
        _within(dcol, want, U * s.abs() + (U * want.abs() if col else 0.0) + 1e-300, tag + " dcol of the written dx")


@pytest.mark.parametrize("case", BN_CASES, ids=_bn_id)
def test_bn_act_bwd(pcg, case):
    """pcg_bn_act_bwd / _premask / _db on the case's routes: the mask from y and recomputed, no activation, dy_scale 1 and 0.5,
    accumulate on and off into non-zero buffers, dcol with both accumulate_col."""
    rows, C, mis, cols, _, route = case
    al = int(not mis)
    assert_route("BN_COLREDUCE", (rows, C, al), cols)
    assert_route("BN_APPLY", (2, rows, C, al), route)
    d = bn_inputs(rows, C)
    for form in BN_BWD_FORMS:
        _run_bn_bwd(pcg.ops, d, rows, C, mis, form)


def test_bn_act_bwd_column_sums_at_the_grid_cap(pcg):
    """(8200, 256), backward with column sums only: 1025 blocks wanted against the cap of 1024, so the two-deep main loop runs and
    the first 512 threads take the tail statement; 1024 partial rows of column sums behind it."""
    rows, C, cols, route = BN_COLSUM_ONLY
    assert_route("BN_COLREDUCE", (rows, C, 1), cols)
    assert_route("BN_APPLY", (2, rows, C, 1), route)
    assert_route("BN_FINALIZE", (1024,), "256 threads, 4 eight-deep trips")
    _run_bn_bwd(pcg.ops, bn_inputs(rows, C), rows, C, False, ("premask", ACT_LRELU, 0.5, False, True))


def test_bn_eval_form_one_row(pcg):
    """The evaluation form at rows = 1."""
    C = 8
    d = bn_inputs(5, 8)
    x = d["x"][:1]
    ref = R.bn_apply(x, d["mean32"], d["var32"], d["gamma"], d["beta"], ACT_LRELU, SLOPE, None, 1.0, EPS)
    assert R.mask_gap_ok(ref["pre"], ref["pre_bound"])[0]
    assert_route("BN_APPLY", (0, 1, C, 1), f"fast<2>: 1 block, {_T}0 main trips + tail of 1")
    buf, y = _out_like((1, C))
    pcg.ops.bn_apply_act(_dev(x), C, _dev(d["mean32"]), _dev(d["var32"]), _dev(d["gamma"]), _dev(d["beta"]), ACT_LRELU, SLOPE, var_eps=EPS, out=y)
    _untouched(buf, y, "eval form, one row")
    _within(y, ref["out"], ref["bound"], "bn_apply_act eval form, rows = 1")


def bn_partial_buffer_doubles(nparts, C):
    """What the conv workspace queries size for `nparts` partial rows (bn_partial_buffer_bytes): the rows [nparts][2][C], the chunk
    sums of the two-level finalize, and 4 C doubles of scratch."""
    m = re.match(r"presum: (\d+) chunks", plan("BN_FINALIZE", nparts))
    return nparts * 2 * C + (int(m.group(1)) if m else 0) * 2 * C + 4 * C


@pytest.mark.parametrize("nparts", sorted(BN_PARTIAL_NPARTS))
@pytest.mark.parametrize("rows,C", BN_PARTIAL_SHAPES)
def test_bn_bwd_partial(pcg, rows, C, nparts):
    """pcg_bn_bwd_partial and pcg_bn_bwd_partial_db from partial rows the test synthesises: the float64 column sums of dm_scale dm and
    dm_scale dm xhat split over `nparts` rows (random rows, the last one closes the sum), in a buffer sized as the conv workspace
    query sizes it.  nparts 1, 1025 (1024-thread finalize), 2048 (presum, 256 chunks of 8), 2049 (228 chunks of 9, the last ragged)."""
    ops = pcg.ops
    assert_route("BN_FINALIZE", (nparts,), BN_PARTIAL_NPARTS[nparts])
    g = _gen(nparts + C)
    d = bn_inputs(1000, C) if C in (8, 36) else None
    x, mean, invstd, gamma = d["x"][:rows], d["mean32"], d["invstd32"], d["gamma"]
    dm = R.f32_exact(torch.randn(rows, C, generator=g, dtype=torch.float64))
    for dm_scale, with_col in ((1.0, False), (0.5, True), (0.5, False)):
        ref = R.bn_bwd(dm, x, mean, invstd, gamma, None, ACT_NONE, 0.0, dm_scale)
        sums = torch.stack([ref["dbeta"], ref["dgamma"]])                           # [2][C]: sum dm, sum dm xhat
        part = torch.randn(nparts, 2, C, generator=g, dtype=torch.float64) * sums.abs().clamp_min(1e-3)
        part[-1] = sums - part[:-1].sum(0)
        fin_err = nparts * 2.0 ** -52 * part.abs().sum(0)                           # the fp64 finalize, any order
        buf = torch.full((bn_partial_buffer_doubles(nparts, C) + 4,), float(SENT), dtype=torch.float64, device=DEV)
        buf[:part.numel()] = part.reshape(-1).to(DEV)
        p0 = buf[:part.numel()].clone()
        xd, dmd = _dev(x), _dev(dm)
        obuf, dx = _out_like((rows, C))
        dg, db = torch.full((C,), 0.25, dtype=torch.float32, device=DEV), torch.full((C,), -0.5, dtype=torch.float32, device=DEV)
        dcol = torch.full((C,), 0.125, dtype=torch.float32, device=DEV) if with_col else None
        ops.bn_bwd_partial(dmd, xd, C, _dev(mean), _dev(invstd), _dev(gamma), buf, nparts, dg, db, True, out=dx, dcol=dcol, accumulate_col=True,
                           dm_scale=dm_scale)
        tag = f"bn_bwd_partial {rows}x{C} nparts={nparts} scale={dm_scale} dcol={with_col}"
        _untouched(obuf, dx, tag)
        assert torch.equal(buf[:part.numel()], p0) and bool((buf[-4:] == SENT).all()), tag + ": the partial rows changed"
        k = U * (gamma * invstd).abs() * (fin_err[0] + ref["xh"].abs() * fin_err[1]) / rows
        _within(dx, ref["dx"], ref["dx_bound"] + k, tag + " dx")
        for i, (name, got, old) in enumerate((("dbeta", db, -0.5), ("dgamma", dg, 0.25))):
            want = sums[i] + old
            _within(got, want, U * sums[i].abs() + U * want.abs() + fin_err[i], f"{tag} {name}")
        if with_col:
            s = dx.double().sum(0).cpu()
            _within(dcol, s + 0.125, U * s.abs() + U * (s + 0.125).abs() + 1e-300, tag + " dcol of the written dx")
            _within(dcol, ref["dcol"] + 0.125, ref["dcol_bound"] + k.sum(0) + U * (ref["dcol"] + 0.125).abs(), tag + " dcol")


def test_bn_environment_knobs(pcg, tmp_path):
    """PCG_BN_DEPTH / PCG_BN_NT / PCG_BN_BLOCKS are read once per process: tests/bn_knobs_child.py runs the three shapes in a fresh
    child per setting (one at a time, every exit status checked) and leaves y, dx, dcol in an .npz.  The knobs move no arithmetic:
    y and dx are bit-identical to this process's default-knob outputs (which are held to float64 here); dcol, whose partial rows
    regroup with the grid, stays within the column-sum bound.  The child's describe text names the instantiation it ran."""
    import bn_knobs_child as K
    mine = K.run(BN_KNOB_SHAPES)
    for rows, C in BN_KNOB_SHAPES:
        d = K.inputs(rows, C)
        ref = R.bn_apply(d["x"], d["mean32"], d["invstd32"], d["gamma"], d["beta"], ACT_LRELU, SLOPE)
        assert R.mask_gap_ok(ref["pre"], ref["pre_bound"])[0]
        bw = R.bn_bwd(d["dy"], d["x"], d["mean32"], d["invstd32"], d["gamma"], ref["pre"], ACT_LRELU, SLOPE, 0.5)
        _within(torch.from_numpy(mine[f"y_{rows}_{C}"]), ref["out"], ref["bound"], f"default knobs y {rows}x{C}")
        _within(torch.from_numpy(mine[f"dx_{rows}_{C}"]), bw["dx"], bw["dx_bound"], f"default knobs dx {rows}x{C}")
        _within(torch.from_numpy(mine[f"dcol_{rows}_{C}"]), bw["dcol"], bw["dcol_bound"], f"default knobs dcol {rows}x{C}")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn_knobs_child.py")
    for i, (env, want) in enumerate(BN_KNOB_SETTINGS):
        out = tmp_path / f"knobs{i}.npz"
        r = subprocess.run([sys.executable, child, str(out)], env={**os.environ, **env}, timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f"knob child {env} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        got = np.load(out)
        assert str(got["plan_1000_64"]) == want, f"child {env}: apply route {str(got['plan_1000_64'])!r}, expected {want!r}"
        for rows, C in BN_KNOB_SHAPES:
            for k in ("y", "dx"):
                a, b = got[f"{k}_{rows}_{C}"], mine[f"{k}_{rows}_{C}"]
                assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), f"{env}: {k} {rows}x{C} differs from the default knobs"
            d = K.inputs(rows, C)
            pre = R.bn_apply(d["x"], d["mean32"], d["invstd32"], d["gamma"], d["beta"], ACT_LRELU, SLOPE)["pre"]
            bw = R.bn_bwd(d["dy"], d["x"], d["mean32"], d["invstd32"], d["gamma"], pre, ACT_LRELU, SLOPE, 0.5)
            _within(torch.from_numpy(got[f"dcol_{rows}_{C}"]), bw["dcol"], bw["dcol_bound"], f"{env}: dcol {rows}x{C}")


# =================================================================================================================================
# InstanceNorm
# =================================================================================================================================
def _in_id(c):
    return f"C{c[0]}-HW{c[1]}{'-misaligned' if c[2] else ''}"


def _in_device(c, mis):
    C, HW = c
    d = in_inputs(C, HW)
    dd = {k: _dev(v) for k, v in d.items()}
    if mis:
        dd["x"] = _off_by_one_float(d["x"])
    return d, dd


_rsqrt_seen = []


@pytest.mark.parametrize("case", IN_CASES, ids=_in_id)
def test_instnorm_forward(pcg, case):
    """pcg_instnorm_fwd with LeakyReLU and with no activation against F.instance_norm in float64: y, mean, invstd.  Prints the
    measured |invstd_device / invstd_float64 - 1| in units of u (the rsqrtf allowance of the module docstring comes from it)."""
    C, HW, mis, route, bb = case
    ops = pcg.ops
    assert_route("INSTNORM", (0, IN_B, HW, C, int(not mis)), route)
    ok, n_bad = in_mask_gap(C, HW, route)
    assert ok, f"{n_bad} pre-activations of the reference lie within 8 bounds of zero"
    d, dd = _in_device((C, HW), mis)
    rf = in_refs(C, HW, route, bb)
    f = rf["f"]
    auto = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], EPS, SLOPE, d["dy"])
    x0 = dd["x"].clone()
    for act in (ACT_LRELU, ACT_NONE):
        y, mean, invstd = ops.instnorm_fwd(dd["x"], IN_B, HW, C, dd["gamma"], dd["beta"], EPS, act, SLOPE)
        want, bound = R.act_out(f["n"], f["n_bound"], SLOPE, act)
        want = auto["y"] if act == ACT_LRELU else auto["n"]
        _within(y, want, R.in_bound("y", bound, want), f"instnorm_fwd y {_in_id(case)} act={act}")
        _within(mean.view(IN_B, C), f["mean"], f["mean_bound"], "instnorm_fwd mean")
        _within(invstd.view(IN_B, C), f["invstd"], f["invstd_bound"], "instnorm_fwd invstd")
    rel = float(((invstd.view(IN_B, C).double().cpu() / f["invstd"]) - 1).abs().max()) / U
    _rsqrt_seen.append(rel)
    print(f"rsqrt measurement {_in_id(case)}: max |invstd_device / invstd_float64 - 1| = {rel:.3f} u (running max {max(_rsqrt_seen):.3f} u)")
    assert torch.equal(dd["x"], x0)


@pytest.mark.parametrize("case", IN_CASES, ids=_in_id)
def test_instnorm_backward(pcg, case):
    """pcg_instnorm_bwd, pcg_instnorm_bwd_fused (once with act_y, keep_dn, addend, parameter partials and dxsum, once with none of
    them) and pcg_rowsum3 against float64 autograd of z -> InstanceNorm -> LeakyReLU."""
    C, HW, mis, route, bb = case
    ops = pcg.ops
    assert_route("INSTNORM", (1, IN_B, HW, C, int(not mis)), route)
    assert in_mask_gap(C, HW, route)[0]
    d, dd = _in_device((C, HW), mis)
    rf = in_refs(C, HW, route, bb)
    tag = _in_id(case)
    y, mean, invstd = ops.instnorm_fwd(dd["x"], IN_B, HW, C, dd["gamma"], dd["beta"], EPS, ACT_LRELU, SLOPE)
    auto = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], EPS, SLOPE, d["dy"])
    b = rf["bwd"]
    dx, dgp, dbp = ops.instnorm_bwd(dd["dy"], dd["x"], IN_B, HW, C, mean, invstd, dd["gamma"])
    _within(dx, auto["dx"], R.in_bound("dx", b["dx_bound"], auto["dx"]), f"instnorm_bwd dx {tag}")
    _within(dgp, b["dgamma_part"], b["dgamma_part_bound"], f"instnorm_bwd dgamma partials {tag}")
    _within(dbp, b["dbeta_part"], b["dbeta_part_bound"], f"instnorm_bwd dbeta partials {tag}")
    _within(dgp.double().sum(0), auto["dgamma"], R.in_bound("dgamma", b["dgamma_part_bound"].sum(0), auto["dgamma"]), f"instnorm_bwd dgamma {tag}")
    _within(dbp.double().sum(0), auto["dbeta"], R.in_bound("dbeta", b["dbeta_part_bound"].sum(0), auto["dbeta"]), f"instnorm_bwd dbeta {tag}")
    only_p = ops.instnorm_bwd(dd["dy"], dd["x"], IN_B, HW, C, mean, invstd, dd["gamma"], need_dx=False)
    assert only_p[0] is None and torch.equal(only_p[1], dgp) and torch.equal(only_p[2], dbp)
    # the fused stage backward: cotangent on the activation's output, masked by the forward's LeakyReLU
    fu = rf["fused"]
    auto_f = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], EPS, SLOPE, R.f32_exact(d["cot"] * rf["mask"]))
    dx, dn, dgp, dbp, dsp = ops.instnorm_bwd_fused(dd["cot"], dd["x"], IN_B, HW, C, mean, invstd, dd["gamma"], act_y=y, slope=SLOPE, keep_dn=True,
                                                   addend=dd["add"], need_params=True, need_dxsum=True)
    _within(dn, d["cot"] * rf["mask"], U * (d["cot"] * rf["mask"]).abs(), f"fused dn {tag}")
    _within(dx, auto_f["dx"] + d["add"], R.in_bound("dx", fu["dx_bound"], auto_f["dx"] + d["add"]), f"fused dx + addend {tag}")
    _within(dgp.double().sum(0), auto_f["dgamma"], R.in_bound("dgamma", fu["dgamma_part_bound"].sum(0), auto_f["dgamma"]), f"fused dgamma {tag}")
    _within(dbp.double().sum(0), auto_f["dbeta"], R.in_bound("dbeta", fu["dbeta_part_bound"].sum(0), auto_f["dbeta"]), f"fused dbeta {tag}")
    _within(dsp, fu["dxsum"], fu["dxsum_bound"], f"fused dxsum {tag}")
    dx2, dn2, g2, b2, s2 = ops.instnorm_bwd_fused(dd["dy"], dd["x"], IN_B, HW, C, mean, invstd, dd["gamma"], need_params=False)
    assert dn2 is None and g2 is None and b2 is None and s2 is None
    _within(dx2, auto["dx"], R.in_bound("dx", rf["bare"]["dx_bound"], auto["dx"]), f"bare fused dx {tag}")
    # pcg_rowsum3: fp64 sums of the float32 partials over B, one rounding (and the add's)
    outs = [torch.full((C,), 0.5, dtype=torch.float32, device=DEV), torch.full((C,), SENT, dtype=torch.float32, device=DEV),
            torch.full((C,), SENT, dtype=torch.float32, device=DEV)]
    ops.rowsum3([(dgp, outs[0], True), (dbp, outs[1], False), (dsp, outs[2], False)], IN_B, C)
    for src, out, old in ((dgp, outs[0], 0.5), (dbp, outs[1], None), (dsp, outs[2], None)):
        s = src.double().sum(0).cpu()
        want = s if old is None else s + old
        _within(out, want, U * s.abs() + (U * want.abs() if old is not None else 0.0) + 1e-300, f"rowsum3 {tag}")


def _check_bwd_bwd(ops, case, dd, d, rf, mean, invstd, y, need, masked):
    C, HW, mis, route, bb = case
    auto = R.instnorm_autograd(d["x"], d["gamma"], d["beta"], EPS, SLOPE, d["dy"], d["r"])
    ref = rf["bb"]
    ddy, ez, dgp = ops.instnorm_bwd_bwd(dd["r"], dd["dy"], dd["x"], IN_B, HW, C, mean, invstd, dd["gamma"], need_ddy=need[0], need_ez=need[1],
                                        need_gamma=need[2], act_y=y if masked else None, slope=SLOPE)
    tag = f"instnorm_bwd_bwd {_in_id(case)} need={need} masked={masked}"
    assert (ddy is not None, ez is not None, dgp is not None) == tuple(need)
    if need[0]:
        m = rf["mask"] if masked else torch.ones_like(rf["mask"])
        _within(ddy, auto["ddy"] * m, R.in_bound("ddy", m * ref["ddy_bound"] + (U * (auto["ddy"] * m).abs() if masked else 0.0), auto["ddy"] * m), tag + " ddy")
    if need[1]:
        _within(ez, auto["ez"], R.in_bound("ez", ref["ez_bound"], auto["ez"], ref["ez_floor"]), tag + " ez")
    if need[2]:
        _within(dgp, ref["dgamma_part"], ref["dgamma_part_bound"], tag + " dgamma partials")
        _within(dgp.double().sum(0), auto["dgamma2"], R.in_bound("dgamma2", ref["dgamma_part_bound"].sum(0), auto["dgamma2"]), tag + " dgamma")


@pytest.mark.parametrize("case", IN_CASES, ids=_in_id)
def test_instnorm_backward_of_backward(pcg, case):
    """pcg_instnorm_bwd_bwd plain and with act_y against float64 autograd with create_graph=True; at one case per kernel form
    every combination of the three optional outputs."""
    C, HW, mis, route, bb = case
    ops = pcg.ops
    assert_route("INSTNORM", (2, IN_B, HW, C, int(not mis)), bb)
    assert in_mask_gap(C, HW, route)[0]
    d, dd = _in_device((C, HW), mis)
    rf = in_refs(C, HW, route, bb)
    y, mean, invstd = ops.instnorm_fwd(dd["x"], IN_B, HW, C, dd["gamma"], dd["beta"], EPS, ACT_LRELU, SLOPE)
    _check_bwd_bwd(ops, case, dd, d, rf, mean, invstd, y, (True, True, True), False)
    _check_bwd_bwd(ops, case, dd, d, rf, mean, invstd, y, (True, True, True), True)
    if (C, HW, mis) in IN_OPTIONAL_OUTPUT_CASES:
        for bits in range(1, 7):
            _check_bwd_bwd(ops, case, dd, d, rf, mean, invstd, y, (bool(bits & 1), bool(bits & 2), bool(bits & 4)), bool(bits & 1))


# =================================================================================================================================
# spectral norm
# =================================================================================================================================
@pytest.mark.parametrize("case", SN_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_spectral_norm_routes(pcg, case):
    """pcg_spectral_norm_fwd / _bwd against torch.nn.utils.spectral_norm in float64: two training forwards (u and v keep moving), each
    with the backward accumulate off and on, then one evaluation forward."""
    O, I, fwd, bwd = case
    ops = pcg.ops
    assert_route("SPECTRAL_NORM", (0, O, I), fwd)
    assert_route("SPECTRAL_NORM", (1, O, I), bwd)
    d, calls, ev = sn_reference(O, I)
    Wd, u, v = _dev(d["W"]), _dev(d["u"]), _dev(d["v"])
    W0 = Wd.clone()
    tag = f"{O}x{I}"
    for k, ref in enumerate(calls):
        w_bar, sigma, uu, vu = ops.spectral_norm_fwd(Wd, u, v, 1e-12, True)
        _within(u, ref["u"], R.sn_bound("u", ref["u"]), f"u {tag} call {k}")
        _within(v, ref["v"], R.sn_bound("v", ref["v"]), f"v {tag} call {k}")
        assert torch.equal(uu, u) and torch.equal(vu, v)
        _within(w_bar, ref["w_bar"], R.sn_bound("w_bar", ref["w_bar"]), f"w_bar {tag} call {k}")
        sig = ref["u"] @ (d["W"] @ ref["v"])
        _within(sigma, sig.reshape(1), 1e-5 * sig.abs().reshape(1), f"sigma {tag} call {k}")
        for acc in (False, True):
            buf, gw = _out_like((O, I))
            if acc:
                gw.copy_(_dev(d["dW0"]))
            ops.spectral_norm_bwd(_dev(d["dwbar"][k]), w_bar, uu, vu, sigma, gw, acc)
            _untouched(buf, gw, f"dW {tag}")
            want = ref["dW"] + d["dW0"] if acc else ref["dW"]
            _within(gw, want, R.sn_bound("dW", ref["dW"]) + (U * want.abs() if acc else 0.0), f"dW {tag} call {k} acc={acc}")
    ub, vb = u.clone(), v.clone()
    w_bar, _, _, _ = ops.spectral_norm_fwd(Wd, u, v, 1e-12, False)
    assert torch.equal(ub, u) and torch.equal(vb, v) and torch.equal(Wd, W0)
    _within(w_bar, ev["w_bar"], R.sn_bound("w_bar", ev["w_bar"]), f"w_bar {tag} eval")


def test_spectral_norm_batched(pcg):
    """The batched entries with an LDS-form and a global-form layer in one launch: reps = 2 forward (each call's outputs land in its
    own set: the `rp * rstride` indexing), then passes = 2 backward into one dW per layer with a db_dst / db_src pair."""
    ops = pcg.ops
    refs = [sn_reference(O, I) for O, I in SN_BATCHED]
    assert plan("SPECTRAL_NORM", 0, *SN_BATCHED[0]).startswith("LDS image") and plan("SPECTRAL_NORM", 0, *SN_BATCHED[1]).startswith("global memory")
    Ws, us, vs = ([_dev(r[0][k]) for r in refs] for k in ("W", "u", "v"))
    outs = ops.spectral_norm_fwd_batched(Ws, us, vs, 1e-12, True, reps=2)
    for call in range(2):
        for l, (d, calls, _) in enumerate(refs):
            w_bar, sigma, uu, vu = outs[call][l]
            ref = calls[call]
            tag = f"batched layer {l} call {call}"
            _within(w_bar, ref["w_bar"], R.sn_bound("w_bar", ref["w_bar"]), "w_bar " + tag)
            _within(uu, ref["u"], R.sn_bound("u", ref["u"]), "u_used " + tag)
            _within(vu, ref["v"], R.sn_bound("v", ref["v"]), "v_used " + tag)
            sig = ref["u"] @ (d["W"] @ ref["v"])
            _within(sigma, sig.reshape(1), 1e-5 * sig.abs().reshape(1), "sigma " + tag)
    for l in range(2):
        assert torch.equal(us[l], outs[1][l][2]) and torch.equal(vs[l], outs[1][l][3])          # the state is the last call's
    passes = [[(_dev(refs[l][0]["dwbar"][q]),) + tuple(outs[q][l][i] for i in (0, 2, 3, 1)) for l in range(2)] for q in range(2)]
    gws = [_dev(r[0]["dW0"]) for r in refs]
    O1 = SN_BATCHED[1][0]
    db_dst, db_src = torch.full((O1,), 0.5, dtype=torch.float32, device=DEV), _dev(torch.arange(O1, dtype=torch.float64) / 8)
    ops.spectral_norm_bwd_batched(passes, gws, [False, True], bias_adds=[None, (db_dst, db_src)])
    for l, (d, calls, _) in enumerate(refs):
        want = calls[0]["dW"] + calls[1]["dW"] + (d["dW0"] if l == 1 else 0.0)
        bound = R.sn_bound("dW", calls[0]["dW"]) + R.sn_bound("dW", calls[1]["dW"]) + 2 * U * want.abs()
        _within(gws[l], want, bound, f"batched dW layer {l}")
    assert torch.equal(db_dst.cpu(), (0.5 + torch.arange(O1, dtype=torch.float64) / 8).float())


def test_spectral_norm_refuses_257(pcg):
    """O or I of 257 is refused before any launch, by every entry."""
    ops = pcg.ops
    for O, I in ((257, 4), (4, 257)):
        W, u, v = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((O, I), (O,), (I,)))
        sigma = torch.ones(1, dtype=torch.float32, device=DEV)
        with pytest.raises(pcg.PcgError, match="pcg_spectral_norm_fwd"):
            ops.spectral_norm_fwd(W, u, v, 1e-12, True)
        with pytest.raises(pcg.PcgError, match="pcg_spectral_norm_bwd"):
            ops.spectral_norm_bwd(W, W, u, v, sigma, W.clone(), False)
        with pytest.raises(pcg.PcgError, match="pcg_spectral_norm_fwd_batched"):
            ops.spectral_norm_fwd_batched([W], [u], [v], 1e-12, True)
        with pytest.raises(pcg.PcgError, match="pcg_spectral_norm_bwd_batched"):
            ops.spectral_norm_bwd_batched([[(W, W, u, v, sigma)]], [W.clone()], [False])
        with pytest.raises(pcg.PcgError, match="pcg_launch_plan_describe"):
            plan("SPECTRAL_NORM", 0, O, I)
