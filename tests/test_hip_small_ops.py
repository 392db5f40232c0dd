"""GPU parity of the layer everything tabular is built from -- csrc/tabular.hip (GEMM routes, weight gradients, mean), csrc/cf_ops.hip
(embedding gradient, losses, metrics, |.| mean, pooling, element-wise ops) and the small kernels at the end of csrc/pointwise.hip --
against float64 (tests/small_ops_ref.py), at every host-side switch that chooses a kernel or a path inside one.

Every case names the route it is meant to take and asserts it through pcg_launch_plan_describe (ops.launch_plan) before it runs: a
later threshold change fails the case instead of silently moving it to the other side.  The same tables are checked without a device
by tests/test_small_ops_plan_host.py.

Inputs are randn rounded to float32 before the float64 reference is built (the reference sees exactly the kernel's operands); biases
and addends are nonzero; outputs that a call must not touch are pre-filled with a sentinel.  Bounds are per output element, in float64,
and scale with the magnitude sum of the terms (u = 2^-24):
  GEMM                 (K + 3) u (|A| |B| + |bias| + |C0|): an fp32 FMA chain in any order plus the epilogue adds; LeakyReLU is 1-Lipschitz
  weight gradients     (rows per chain + slabs + 3) u sum|terms|, both read off the plan
  reductions           (L + T + 2) u sum|terms|, L the longest per-thread fp32 chain and T the depth of the fp32 tree (per op, below)
  embedding gradient   (B + 17) u sum|terms|
  expf / logf values   the tolerances of the existing tests of the same kernels (test_small_ops, test_hip_house_clf_fit.py)
  element-wise ops     bit-exact against the same fp32 expression on the CPU (see _contractable for the multiply-adds)
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
SENT = -77.0
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
EW_PASS = 256        # work items one block of an element-wise launch covers per pass


# =================================================================================================================================
# Case tables: (…, route).  Host data only -- tests/test_small_ops_plan_host.py imports them.
# =================================================================================================================================
def _skinny(M, N, K):
    return f"skinny: {-(-M // 16)} blocks, {'two columns' if N > 16 else 'one column'} per thread, {(K * 33 + 16 * (K + 1)) * 4} bytes of LDS"


def _tile(M, N):
    return f"64x64 tiles: {-(-N // 64)} x {-(-M // 64)}"


def _rowdot(M, N):
    return f"rowdot<{N}>: {-(-M // 4)} blocks"


# (M, N, K, transA, transB, (extra columns in the row strides of A, B, C), route of pcg_gemm_act, path inside rowdot_kernel).
# rowdot_kernel picks its float4 loop itself: A and B 16-byte aligned and lda % 4 == ldb % 4 == 0; with K % 4 != 0 the last 1..3
# products of a row go to the scalar tail loop ("float4+tail").  Any other stride or alignment walks the scalar loop alone.
DENSE, WIDE = (0, 0, 0), (3, 0, 5)
GEMM_CASES = [
    (512, 17, 38, False, True, DENSE, _skinny(512, 17, 38), None),        # a second column for c = 0 only
    (512, 17, 38, False, False, WIDE, _skinny(512, 17, 38), None),        # transB off
    (523, 32, 320, False, True, WIDE, _skinny(523, 32, 320), None),       # largest N and K (62 784 bytes of LDS), ragged M
    (523, 2, 21, False, True, DENSE, _skinny(523, 2, 21), None),          # smallest N
    (600, 16, 255, False, False, WIDE, _skinny(600, 16, 255), None),      # no second column
    (515, 4, 300, False, False, DENSE, _skinny(515, 4, 300), None),       # rowdot refuses: not transB
    (515, 4, 300, False, True, (4, 0, 5), _rowdot(515, 4), "float4"),     # rowdot precedence
    (515, 4, 255, False, True, DENSE, _skinny(515, 4, 255), None),        # K below 256
    (511, 17, 38, False, True, WIDE, _tile(511, 17), None),               # M below 512
    (512, 33, 38, False, True, DENSE, _tile(512, 33), None),              # N above 32
    (512, 1, 38, False, True, WIDE, _tile(512, 1), None),                 # N below 2
    (512, 17, 321, False, True, DENSE, _tile(512, 17), None),             # K above 320
    (512, 17, 38, True, True, WIDE, _tile(512, 17), None),                # transA
    (37, 1, 256, False, True, DENSE, _rowdot(37, 1), "float4"),           # K at the threshold: one float4 per lane, no tail
    (37, 1, 257, False, True, (3, 3, 2), _rowdot(37, 1), "float4+tail"),  # a tail of one product, on lane 0 alone
    (37, 2, 257, False, True, (3, 3, 5), _rowdot(37, 2), "float4+tail"),
    (37, 2, 258, False, True, (3, 0, 5), _rowdot(37, 2), "scalar"),       # lda = 261: the scalar loop by stride
    (37, 3, 260, False, True, DENSE, _rowdot(37, 3), "float4"),           # 65 float4 per row: lane 0 walks the loop twice
    (37, 3, 259, False, True, (1, 1, 0), _rowdot(37, 3), "float4+tail"),  # a tail of three
    (37, 3, 259, False, True, DENSE, _rowdot(37, 3), "scalar"),           # the same shape with lda = ldb = 259
    (37, 4, 259, False, True, (1, 1, 5), _rowdot(37, 4), "float4+tail"),
    (37, 4, 519, False, True, (1, 1, 3), _rowdot(37, 4), "float4+tail"),  # a ragged second trip of the float4 loop, then the tail
    (37, 5, 300, False, True, WIDE, _tile(37, 5), None),                  # N above rowdot's 4, M below skinny's 512
]
assert 2 * sum(c[5][0] > 0 and c[5][2] > 0 for c in GEMM_CASES) >= len(GEMM_CASES)      # A and C wide in at least half the cases
for _n in (1, 2, 3, 4):                                        # every rowdot<N> on the float4 loop; 3 and 4 with and without a tail
    assert any(c[6].startswith(f"rowdot<{_n}>") and c[7] in ("float4", "float4+tail") for c in GEMM_CASES)
for _n in (3, 4):
    assert {c[7] for c in GEMM_CASES if c[6].startswith(f"rowdot<{_n}>")} >= {"float4", "float4+tail"}
GEMM_MISALIGNED = (130, 3, 301, _rowdot(130, 3))                    # A starts 4 bytes off a 16-byte boundary, K % 4 != 0: scalar path
# pcg_gemm itself (no activation, no skinny launch): (M, N, K, transA, transB, route)
GEMM_PLAIN_CASES = [(512, 17, 38, False, True, _tile(512, 17)), (131, 2, 300, False, True, _rowdot(131, 2))]     # the latter: float4, no tail

# B -> route of pcg_linear_wgrad_grouped
WGRAD_GROUPED_CASES = {1: "blocks per tile: 1, rows per wave: 32", 2: "blocks per tile: 1, rows per wave: 32",
                       63: "blocks per tile: 1, rows per wave: 32", 257: "blocks per tile: 2, rows per wave: 64",
                       777: "blocks per tile: 4, rows per wave: 64", 4097: "blocks per tile: 16, rows per wave: 96"}
# (B, O, I) -> route of pcg_linear_wgrad
LINEAR_WGRAD_CASES = {(127, 33, 33): "64x64 tiles: 1, slabs: 1 of 128 rows", (128, 33, 33): "64x64 tiles: 1, slabs: 1 of 128 rows",
                      (129, 33, 33): "64x64 tiles: 1, slabs: 2 of 80 rows", (129, 70, 64): "64x64 tiles: 4, slabs: 2 of 80 rows"}

# (B, K, logits misaligned by one float) -> route of pcg_cross_entropy_fwd_bwd (dlogits absent or aligned)
CE_CASES = {(1, 1, False): "256 threads, no float4 rows", (1, 10, False): "256 threads, no float4 rows",
            (769, 4, False): "256 threads, float4 rows", (769, 4, True): "256 threads, no float4 rows",
            (1024, 4, False): "256 threads, float4 rows", (1025, 4, False): "1024 threads, float4 rows",
            (3073, 4, False): "1024 threads, float4 rows", (4096, 4, False): "1024 threads, float4 rows",
            (1025, 10, False): "1024 threads, no float4 rows"}

REDUCE_NS = [1, 1023, 1024, 7169, 8192, 8193, 16384, 16385, 70001, 4096 * 256 + 257]


def _reduce_route(n, partials):
    return "one block of 1024" if n <= 16384 else f"{partials} partials + finish"


# (B, has_dtable, has_dx) -> route of pcg_embed_concat_bwd
def _embed_route(B, has_dtable, has_dx):
    return ("batch-split table gradient" + (" + copy" if has_dx else "")) if has_dtable and B >= 64 else "one pass"


EMBED_BS = [7, 63, 64, 65, 133]


def _ew_route(n, cap):
    blocks = max(1, min(cap, -(-n // EW_PASS)))
    passes = -(-n // (blocks * EW_PASS))
    return f"{blocks} block{'s' if blocks != 1 else ''} of 256: {passes} pass{'es' if passes != 1 else ''}"


def _act_route(n, aligned):
    v4 = aligned and n % 4 == 0
    return ("float4 lanes: " if v4 else "scalar lanes: ") + _ew_route(n // 4 if v4 else n, 8192)


# (n, misaligned by one float): act_bwd.  The last one is the first size whose float4 launch walks its grid-stride loop twice
# (8192 blocks of 256 lanes of four floats)
ACT_CASES = [(1001, False), (4096 * 64, False), (1000, True), (4 * (4096 * 256) + 4, False), (4 * (8192 * 256) + 4, False)]
# element-wise launches of cf_ops.hip: at most 8192 blocks, so the stride loop loops from 8192 * 256 + 1 work items
CF_BIG_NS = [4096 * 256 + 257, 8192 * 256 + 257]
GATHER_ROWS = [1, 257, 262144 + 300]
TABULAR_BIG = (61697, 9, 8)          # rows, ca, cb of concat / split / FiLM: 17 columns, 4096 * 256 + 273 elements: two passes


def all_routes():
    """[(plan op name, args, expected text)] of every table above."""
    out = []
    for M, N, K, tA, tB, _, want, _ in GEMM_CASES:
        out.append(("GEMM_ACT", (tA, tB, M, N, K), want))
    M, N, K, want = GEMM_MISALIGNED
    out.append(("GEMM_ACT", (0, 1, M, N, K), want))
    for M, N, K, tA, tB, want in GEMM_PLAIN_CASES:
        out.append(("GEMM", (tA, tB, M, N, K), want))
    out += [("LINEAR_WGRAD_GROUPED", (B,), want) for B, want in WGRAD_GROUPED_CASES.items()]
    out += [("LINEAR_WGRAD", k, want) for k, want in LINEAR_WGRAD_CASES.items()]
    out += [("CROSS_ENTROPY", (B, K, not mis, 1), want) for (B, K, mis), want in CE_CASES.items()]
    for n in REDUCE_NS:
        out += [("MEAN", (n,), _reduce_route(n, 64)), ("ABS_MEAN", (n,), _reduce_route(n, 256))]
    for B in EMBED_BS:
        out += [("EMBED_CONCAT_BWD", (B, dt, dx), _embed_route(B, dt, dx)) for dt, dx in ((1, 1), (1, 0), (0, 1))]
    out += [("ACT", (n, not mis), _act_route(n, not mis)) for n, mis in ACT_CASES]
    out += [("ELEMENTWISE", ("EW_CF_OPS", n), _ew_route(n, 8192)) for n in CF_BIG_NS]
    out += [("ELEMENTWISE", ("EW_GATHER_CHANNEL", n), _ew_route(n, 1024)) for n in GATHER_ROWS]
    out += [("ELEMENTWISE", ("EW_POINTWISE", r * c), _ew_route(r * c, 8192)) for r, c in ((77, 17), (70000, 16))]
    out.append(("ELEMENTWISE", ("EW_TABULAR", TABULAR_BIG[0] * (TABULAR_BIG[1] + TABULAR_BIG[2])), "4096 blocks of 256: 2 passes"))
    return out


# the routes this file is there to cover, each reached by at least one case (checked on the host as well)
REQUIRED_ROUTE_PATTERNS = [r"^skinny: .*two columns", r"^skinny: .*one column", r"^rowdot<1>", r"^rowdot<2>", r"^rowdot<3>", r"^rowdot<4>",
                           r"^64x64 tiles: \d+ x \d+$", r"^one block of 1024$", r"^64 partials \+ finish$", r"^256 partials \+ finish$",
                           r"^256 threads, float4 rows$", r"^256 threads, no float4 rows$", r"^1024 threads, float4 rows$",
                           r"^1024 threads, no float4 rows$", r"^batch-split table gradient \+ copy$", r"^batch-split table gradient$",
                           r"^one pass$", r"^float4 lanes: .* 2 passes$", r"^scalar lanes: ", r"^4096 blocks of 256: 2 passes$",
                           r"^8192 blocks of 256: 2 passes$", r"^1024 blocks of 256: 2 passes$"]


def plan(op, *args):
    """pcg_launch_plan_describe by name: plan("GEMM_ACT", tA, tB, M, N, K); host logic, no device."""
    from pcgan_amd import _lib, ops
    args = [getattr(_lib, "PLAN_" + a) if isinstance(a, str) else int(a) for a in args]
    return ops.launch_plan(getattr(_lib, "PLAN_" + op), *args)


def assert_route(op, args, want):
    got = plan(op, *args)
    assert got == want, f"route moved: {op}{tuple(args)} takes {got!r}, the case expects {want!r}"


def check_all_routes():
    seen = []
    for op, args, want in all_routes():
        assert_route(op, args, want)
        seen.append(want)
    for pat in REQUIRED_ROUTE_PATTERNS:
        assert any(re.search(pat, s) for s in seen), f"no case reaches a route like {pat!r}"


# =================================================================================================================================
# helpers
# =================================================================================================================================
@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, g, scale=1.0):
    """float64 values that are exactly representable in float32."""
    return R.f32_exact(torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def _dyadic(*shape, g, bits=6, span=4):
    """Multiples of 2^-bits in [-span, span): products and sums of a few of them are exact in fp32 in ANY evaluation order."""
    return torch.randint(-span * 2 ** bits, span * 2 ** bits, shape, generator=g).double() / 2 ** bits


def _dev(t):
    return t.float().to(DEV).contiguous()


def _off_by_one_float(t):
    """A contiguous device copy of t whose storage starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t.float())
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _wide(t, ld, left=0):
    """t as a column slice (starting at column `left`) of a sentinel-filled [rows][ld] device buffer: (buffer, view)."""
    buf = torch.full((t.shape[0], ld), SENT, dtype=torch.float32, device=DEV)
    buf[:, left:left + t.shape[1]] = t.float().to(DEV)
    return buf, buf[:, left:left + t.shape[1]]


def _within(got, ref, bound, what):
    """|got - ref| <= bound per element, in float64; prints the worst ratio before it asserts."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.double().reshape(-1)
    bound = (bound.double().reshape(-1) if torch.is_tensor(bound) else torch.full_like(ref, float(bound)))
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    print(f"{what}: worst err/bound {float(ratio[worst]):.3g} (err {float(err[worst]):.3g}, bound {float(bound[worst]):.3g}) at {worst}")
    assert float(ratio[worst]) <= 1.0, f"{what}: |err| {float(err[worst]):.3e} > bound {float(bound[worst]):.3e} at flat index {worst}"


def _bit_equal(got, ref, what):
    got = got.detach().cpu()
    ref = ref.float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    same = got.view(torch.int32) == ref.contiguous().view(torch.int32)
    both_zero = (got == 0) & (ref == 0)                     # +0 and -0 are the same value
    bad = ~(same | both_zero)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {int(bad.reshape(-1).nonzero()[0])}"


def _contractable(got, exact, n_roundings, mag, what):
    """For an expression with a multiply-add that hipcc may contract to an FMA: the bit pattern depends on that choice, so random
    inputs are held to float64 instead: one rounding, u * sum|terms|, for each rounding of the uncontracted expression (a bound on
    the difference to the fp32 CPU value cannot hold -- one ulp of a result near a power of two is already 2 u * |result|).  The
    bit-exact comparison of these ops uses dyadic inputs, where no evaluation order rounds at all."""
    _within(got, exact, n_roundings * U * mag, what)


# =================================================================================================================================
# GEMM routes
# =================================================================================================================================
def _rowdot_path(Ad, lda, Bd, ldb, K):
    """The path rowdot_kernel takes inside (csrc/tabular.hip: `vec`), from the operands a call really passes."""
    vec = Ad.data_ptr() % 16 == 0 and Bd.data_ptr() % 16 == 0 and lda % 4 == 0 and ldb % 4 == 0
    return ("float4+tail" if K % 4 else "float4") if vec else "scalar"


def _gemm_operands(M, N, K, tA, tB, pads, g):
    A = _randn(*((K, M) if tA else (M, K)), g=g)
    B = _randn(*((N, K) if tB else (K, N)), g=g)
    bias, C0 = _randn(N, g=g), _randn(M, N, g=g)
    lda, ldb, ldc = A.shape[1] + pads[0], B.shape[1] + pads[1], N + pads[2]
    _, Ad = _wide(A, lda)
    _, Bd = _wide(B, ldb)
    return A, B, bias, C0, Ad, Bd, lda, ldb, ldc


def _run_gemm_four_ways(ops, M, N, K, tA, tB, A, B, bias, C0, Ad, Bd, lda, ldb, ldc, tag):
    biasd = _dev(bias)
    bound_scale = (K + 3) * U
    for mode in ("plain", "bias", "accumulate", "accumulate+bias+lrelu"):
        use_bias, acc, act = mode != "plain" and mode != "accumulate", mode.startswith("accumulate"), mode.endswith("lrelu")
        ref, mag = R.gemm(A, B, tA, tB, bias if use_bias else None, C0 if acc else None, 0.2 if act else None)
        cbuf = torch.full((M, ldc), SENT, dtype=torch.float32, device=DEV)
        if acc:
            cbuf[:, :N] = _dev(C0)
        ops.gemm(Ad, Bd, M, N, K, transA=tA, transB=tB, lda=lda, ldb=ldb, out=cbuf, ldc=ldc, bias=biasd if use_bias else None,
                 accumulate=acc, act=ACT_LRELU if act else ACT_NONE, slope=0.2)
        _within(cbuf[:, :N], ref, bound_scale * mag, f"gemm {tag} {mode}")
        assert bool((cbuf[:, N:] == SENT).all()), f"gemm {tag} {mode}: wrote past column N of a wider C"


def _gemm_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}{'-tA' if c[3] else ''}{'-tB' if c[4] else ''}-ld+{c[5][0]}+{c[5][1]}+{c[5][2]}{'-' + c[7] if c[7] else ''}"


@pytest.mark.parametrize("case", GEMM_CASES, ids=_gemm_id)
def test_gemm_routes(pcg, case):
    """pcg_gemm_act on each side of every switch of launch_rowdot / launch_skinny, four ways each (plain; bias; accumulate on a random
    C0; accumulate + bias + LeakyReLU 0.2), half the cases with row strides of A and C wider than K and N.  The rowdot cases also pin
    the path the kernel picks inside -- the float4 loop with and without a scalar tail, or the scalar loop -- from the pointers and
    strides the call passes (the describe entry cannot: that choice is the kernel's)."""
    M, N, K, tA, tB, pads, want, rowpath = case
    assert_route("GEMM_ACT", (tA, tB, M, N, K), want)
    g = _gen(1000 * M + 10 * N + K + 2 * tA + tB + 7 * sum(pads))
    A, B, bias, C0, Ad, Bd, lda, ldb, ldc = _gemm_operands(M, N, K, tA, tB, pads, g)
    assert (rowpath is not None) == want.startswith("rowdot")
    if rowpath is not None:
        got = _rowdot_path(Ad, lda, Bd, ldb, K)
        assert got == rowpath, f"rowdot path moved: lda {lda}, ldb {ldb}, K {K} walk {got!r}, the case expects {rowpath!r}"
    _run_gemm_four_ways(pcg.ops, M, N, K, tA, tB, A, B, bias, C0, Ad, Bd, lda, ldb, ldc, f"{M}x{N}x{K} ld+{pads}")


def test_gemm_rowdot_misaligned_rows(pcg):
    """rowdot with an A that starts 4 bytes off a 16-byte boundary and K % 4 != 0: the scalar path of every lane."""
    M, N, K, want = GEMM_MISALIGNED
    assert_route("GEMM_ACT", (0, 1, M, N, K), want)
    g = _gen(77)
    A, B, bias, C0 = _randn(M, K, g=g), _randn(N, K, g=g), _randn(N, g=g), _randn(M, N, g=g)
    Ad, Bd = _off_by_one_float(A), _dev(B)
    assert _rowdot_path(Ad, K, Bd, K, K) == "scalar" and Ad.data_ptr() % 16 == 4
    _run_gemm_four_ways(pcg.ops, M, N, K, False, True, A, B, bias, C0, Ad, Bd, K, K, N, "rowdot misaligned")


@pytest.mark.parametrize("case", GEMM_PLAIN_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_pcg_gemm_entry(pcg, case):
    """pcg_gemm, the exported entry without an activation (ops.gemm goes through pcg_gemm_act): one tile case, one rowdot case,
    with bias, then accumulating on top."""
    M, N, K, tA, tB, want = case
    assert_route("GEMM", (tA, tB, M, N, K), want)
    ops, lib = pcg.ops, pcg.load()
    g = _gen(5 + M)
    A, B, bias, C0 = _randn(M, K, g=g), _randn(N, K, g=g), _randn(N, g=g), _randn(M, N, g=g)
    Ad, Bd, biasd = _dev(A), _dev(B), _dev(bias)
    if want.startswith("rowdot"):
        assert _rowdot_path(Ad, K, Bd, K, K) == "float4"
    for acc in (False, True):
        C = _dev(C0) if acc else torch.full((M, N), SENT, dtype=torch.float32, device=DEV)
        rc = lib.pcg_gemm(int(tA), int(tB), M, N, K, ops._p(Ad), K, ops._p(Bd), K, ops._p(C), N, ops._p(biasd), int(acc), ops._stream())
        assert rc == 0, lib.pcg_last_error()
        ref, mag = R.gemm(A, B, tA, tB, bias, C0 if acc else None)
        _within(C, ref, (K + 3) * U * mag, f"pcg_gemm {M}x{N}x{K} accumulate={acc}")


# =================================================================================================================================
# weight gradients
# =================================================================================================================================
def _grouped_operands(B, g):
    """A 1x1 layer; a 33x33 layer (four 32x32 tiles, three of them one element wide or high) accumulating on nonzero values; a 9x21
    layer without bias gradient whose x is a column slice; a 13x32 layer whose dy is a column slice of a wider buffer."""
    dy0, x0 = _randn(B, 1, g=g), _randn(B, 1, g=g)
    dy1, x1 = _randn(B, 33, g=g), _randn(B, 33, g=g)
    dy2, xw = _randn(B, 9, g=g), _randn(B, 38, g=g)
    dyw, x3 = _randn(B, 40, g=g), _randn(B, 32, g=g)
    W1, b1 = _randn(33, 33, g=g), _randn(33, g=g)
    host = [(dy0, x0, None, None, True), (dy1, x1, W1, b1, True), (dy2, xw[:, 17:], None, None, False), (dyw[:, 5:18], x3, None, None, True)]
    d = {k: _dev(v) for k, v in dict(dy0=dy0, x0=x0, dy1=dy1, x1=x1, dy2=dy2, xw=xw, dyw=dyw, x3=x3).items()}
    views = [(d["dy0"], d["x0"], 1, 1, 1, 1), (d["dy1"], d["x1"], 33, 33, 33, 33), (d["dy2"], d["xw"][:, 17:], 9, 21, 9, 38),
             (d["dyw"][:, 5:], d["x3"], 13, 32, 40, 32)]
    return host, views


@pytest.mark.parametrize("B", sorted(WGRAD_GROUPED_CASES))
def test_linear_wgrad_grouped_batches(pcg, B):
    """pcg_linear_wgrad_grouped at the batches its MFMA step (two rows), its wave slabs and its 64-slab cap can get wrong: B = 1, even
    and odd, the first batch with two blocks per tile, a ragged one, and one above the cap.  Bound: (rows per wave + wave slabs + 3) u
    sum|terms| -- a wave's chain is at most its rows long, the 4 * Sb wave tiles are added one by one."""
    assert_route("LINEAR_WGRAD_GROUPED", (B,), WGRAD_GROUPED_CASES[B])
    Sb, rows = (int(v) for v in re.fullmatch(r"blocks per tile: (\d+), rows per wave: (\d+)", WGRAD_GROUPED_CASES[B]).groups())
    factor = (rows + 4 * Sb + 3) * U
    ops, dev = pcg.ops, torch.device(DEV)
    host, views = _grouped_operands(B, _gen(B))

    def run():
        items, outs = [], []
        for (dyh, xh, W0, b0, has_db), (dy, x, O, I, ldy, ldx) in zip(host, views):
            dW = _dev(W0) if W0 is not None else torch.full((O, I), SENT, dtype=torch.float32, device=dev)
            db = (_dev(b0) if b0 is not None else torch.full((O,), SENT, dtype=torch.float32, device=dev)) if has_db else None
            items.append((dy, x, O, I, dW, db, ldy, ldx, W0 is not None, b0 is not None))
            outs.append((dW, db))
        ops.linear_wgrad_grouped(items, B, dev)
        return outs
    a, b = run(), run()
    for k, ((dyh, xh, W0, b0, has_db), (dW, db), (dW2, db2)) in enumerate(zip(host, a, b)):
        rW, rb, mW, mb = R.linear_wgrad(dyh, xh, W0, b0)
        _within(dW, rW, factor * mW, f"grouped B={B} layer {k} dW")
        if has_db:
            _within(db, rb, factor * mb, f"grouped B={B} layer {k} db")
            assert torch.equal(db, db2)
        assert torch.equal(dW, dW2), f"grouped B={B} layer {k}: two runs differ"


def test_linear_wgrad_grouped_refuses_oversized_groups(pcg):
    """41 layers, or more than 64 output tiles of 32x32, are refused with an error code before anything is launched."""
    ops, dev = pcg.ops, torch.device(DEV)
    B = 8
    dy, x = _dev(torch.ones(B, 288)), _dev(torch.ones(B, 256))
    outs = [torch.full((1, 1), SENT, dtype=torch.float32, device=dev) for _ in range(41)]
    with pytest.raises(pcg.PcgError, match="at most 40 layers"):
        ops.linear_wgrad_grouped([(dy, x, 1, 1, o, None, 288, 256, False, False) for o in outs], B, dev)
    big = torch.full((288, 256), SENT, dtype=torch.float32, device=dev)            # 9 x 8 = 72 tiles
    with pytest.raises(pcg.PcgError, match="more than 64 32x32 output tiles"):
        ops.linear_wgrad_grouped([(dy, x, 288, 256, big, None, 288, 256, False, False)], B, dev)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs) and bool((big == SENT).all())
    ok = torch.full((1, 1), SENT, dtype=torch.float32, device=dev)                 # the entry still works afterwards
    ops.linear_wgrad_grouped([(dy, x, 1, 1, ok, None, 288, 256, False, False)], B, dev)
    assert float(ok) == float(B)


@pytest.mark.parametrize("case", sorted(LINEAR_WGRAD_CASES), ids=lambda c: "x".join(map(str, c)))
def test_linear_wgrad_first_slab_split(pcg, case):
    """pcg_linear_wgrad at B = 127, 128 (one slab) and 129 (the first batch with two), strided dy, accumulating on nonzero values.
    Bound: (rows per slab + slabs + 3) u sum|terms|."""
    B, O, I = case
    want = LINEAR_WGRAD_CASES[case]
    assert_route("LINEAR_WGRAD", case, want)
    S, chunk = (int(v) for v in re.search(r"slabs: (\d+) of (\d+) rows", want).groups())
    factor = (chunk + S + 3) * U
    ops = pcg.ops
    g = _gen(B * O)
    dyw, x, W0, b0 = _randn(B, O + 5, g=g), _randn(B, I, g=g), _randn(O, I, g=g), _randn(O, g=g)
    dyd, xd = _dev(dyw), _dev(x)
    runs = []
    for _ in range(2):
        dW, db = torch.full((O, I), SENT, dtype=torch.float32, device=DEV), torch.full((O,), SENT, dtype=torch.float32, device=DEV)
        ops.linear_wgrad(dyd[:, 2:], xd, B, O, I, dW, db, ldy=O + 5)
        runs.append((dW, db))
    rW, rb, mW, mb = R.linear_wgrad(dyw[:, 2:2 + O], x)
    _within(runs[0][0], rW, factor * mW, f"linear_wgrad {case} dW")
    _within(runs[0][1], rb, factor * mb, f"linear_wgrad {case} db")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    dW, db = _dev(W0), _dev(b0)
    ops.linear_wgrad(dyd[:, 2:], xd, B, O, I, dW, db, ldy=O + 5, accumulate_w=True, accumulate_b=True)
    rW, rb, mW, mb = R.linear_wgrad(dyw[:, 2:2 + O], x, W0, b0)
    _within(dW, rW, factor * mW, f"linear_wgrad {case} dW accumulate")
    _within(db, rb, factor * mb, f"linear_wgrad {case} db accumulate")


# =================================================================================================================================
# losses and metrics
# =================================================================================================================================
CE_LOSS_RTOL = 2e-6                  # test_small_ops (tests/test_hip_countergan.py)
CE_GRAD_RTOL, CE_GRAD_ATOL = 2e-5, 1e-8      # "
CEW_LOSS_RTOL = 1e-6                 # test_tally_segments_count_and_ties (tests/test_hip_house_clf_fit.py)


def _ce_inputs(B, K, seed):
    g = _gen(seed)
    z = _randn(B, K, g=g, scale=3.0)
    t = (torch.arange(B) % K)[torch.randperm(B, generator=g)]           # every class appears once B >= K
    return z, t


def _ce_grad_check(dz, ref_dz, what):
    _within(dz, ref_dz, CE_GRAD_RTOL * ref_dz.abs() + CE_GRAD_ATOL, what)


@pytest.mark.parametrize("case", sorted(CE_CASES), ids=lambda c: f"{c[0]}x{c[1]}{'-misaligned' if c[2] else ''}")
def test_cross_entropy_routes(pcg, case):
    """pcg_cross_entropy_fwd_bwd on both block sizes (B = 1024 / 1025) and with float4 rows on and off; at B = 769 (and B = 3073 with
    1024 threads) exactly one thread enters the float4 rows, at B = 1025 none does although the rows qualify (a thread needs four rows
    of its own).  Loss and gradient together, the loss alone, the gradient alone; a
    device grad_out and grad_scale != 1.  Tolerances: those of test_small_ops."""
    B, K, mis = case
    ops = pcg.ops
    z, t = _ce_inputs(B, K, 31 * B + K)
    if B >= K:
        assert set(t.tolist()) == set(range(K))
    zd = _off_by_one_float(z) if mis else _dev(z)
    td = t.to(DEV)
    assert_route("CROSS_ENTROPY", (B, K, zd.data_ptr() % 16 == 0, 1), CE_CASES[case])
    go, scale = 0.7, 1.9
    god = torch.tensor([go], dtype=torch.float32, device=DEV)
    go = float(god.item())                                               # the rounded cotangent the kernel reads
    ref_loss, ref_dz = R.cross_entropy(z, t, None, scale, go)
    loss, dz = ops.cross_entropy_fwd_bwd(zd, td, grad_out=god, grad_scale=scale)
    assert dz.data_ptr() % 16 == 0
    _within(loss, ref_loss.reshape(1), CE_LOSS_RTOL * abs(float(ref_loss)), f"ce {case} loss")
    _ce_grad_check(dz, ref_dz, f"ce {case} dlogits")
    loss2, none = ops.cross_entropy_fwd_bwd(zd, td, need_grad=False)
    assert none is None and torch.equal(loss2, loss)
    none, dz2 = ops.cross_entropy_fwd_bwd(zd, td, need_loss=False, grad_out=god, grad_scale=scale)
    assert none is None and torch.equal(dz2, dz)


@pytest.mark.parametrize("B", [1, 255, 257, 1000])
def test_cross_entropy_weighted(pcg, B):
    """pcg_cross_entropy_weighted_fwd_bwd with one class weight zero and one class absent from the targets, on either side of one row
    per thread.  Loss tolerance: that of the tally test of the same arithmetic (test_hip_house_clf_fit.py); gradient: test_small_ops'."""
    ops = pcg.ops
    K = 5
    w = torch.tensor([0.4, 0.0, 1.7, 0.9, 2.3], dtype=torch.float64).float().double()
    g = _gen(B)
    z = _randn(B, K, g=g, scale=3.0)
    t = (torch.arange(B) % (K - 1))[torch.randperm(B, generator=g)]      # class 4 never appears
    if B == 1:
        t = torch.tensor([2])
    go, scale = 0.7, 1.9
    god = torch.tensor([go], dtype=torch.float32, device=DEV)
    go = float(god.item())
    ref_loss, ref_dz = R.cross_entropy(z, t, w, scale, go)
    zd, td, wd = _dev(z), t.to(DEV), _dev(w)
    loss, dz = ops.cross_entropy_weighted_fwd_bwd(zd, td, wd, grad_out=god, grad_scale=scale)
    _within(loss, ref_loss.reshape(1), CEW_LOSS_RTOL * abs(float(ref_loss)), f"weighted ce B={B} loss")
    _ce_grad_check(dz, ref_dz, f"weighted ce B={B} dlogits")
    assert bool((dz[td == 1] == 0).all()), "a row whose class has weight zero must have a zero gradient"
    loss2, none = ops.cross_entropy_weighted_fwd_bwd(zd, td, wd, need_grad=False)
    none2, dz2 = ops.cross_entropy_weighted_fwd_bwd(zd, td, wd, need_loss=False, grad_out=god, grad_scale=scale)
    assert none is None and none2 is None and torch.equal(loss2, loss) and torch.equal(dz2, dz)


def cf_inputs(B, K, seed):
    """Logits for pcg_cf_metrics: every row either has an exact tie for its maximum (rows b % 7 == 3; the targets alternate between
    the first and the second tied index) or a top-two margin of at least 1e-3.  float64 values exactly representable in float32."""
    g = _gen(seed)
    lcf = _randn(B, K, g=g, scale=2.0)
    lref = _randn(B, K, g=g, scale=2.0)
    t = torch.randint(0, K, (B,), generator=g)
    top = lcf.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 1e-3
    lcf[close, top.indices[close, 0]] += 1.0
    lcf = R.f32_exact(lcf)
    ties = [b for b in range(B) if b % 7 == 3]
    for n_, b in enumerate(ties):
        j1, j2 = sorted(torch.randperm(K, generator=g)[:2].tolist())
        v = R.f32_exact(lcf[b].max() + 0.5)
        lcf[b, j1] = v
        lcf[b, j2] = v
        t[b] = j1 if n_ % 2 == 0 else j2
    other = (t + 1 + torch.randint(0, K - 1, (B,), generator=g)) % K
    assert bool((other != t).all())
    top = lcf.topk(2, dim=1).values
    margin = top[:, 0] - top[:, 1]
    tie_rows = torch.zeros(B, dtype=torch.bool)
    if ties:
        tie_rows[ties] = True
    assert bool((margin[tie_rows] == 0).all()) and bool((margin[~tie_rows] >= 1e-3).all())
    return lcf, lref, t, other


def cf_gain_bound(lcf, lref, t, other):
    """(float64 gain, bound, measured fp32-vs-float64 distance of the row terms).  Bound = 4 x the mean distance between the row
    terms evaluated in float32 on the CPU and in float64 (device expf is a few ulp off libm's) + the reduction of cf_metrics_kernel:
    (L + T + 2) u mean|terms| with L = ceil(B / 256) fp32 adds per thread, T = 8 levels of the fp32 tree, 2 for the division by B."""
    B = lcf.shape[0]
    _, rows64 = R.cf_metric_rows(lcf, t, lref, other)
    _, rows32 = R.cf_metric_rows(lcf.float(), t, None if lref is None else lref.float(), other)
    dist = float((rows32.double() - rows64).abs().mean())
    red = (math.ceil(B / 256) + 8 + 2) * U * float(rows64.abs().mean())
    return float(rows64.mean()), 4.0 * dist + red, dist


@pytest.mark.parametrize("K", [3, 4, 10])
@pytest.mark.parametrize("B", [1, 255, 257, 1000])
def test_cf_metrics(pcg, B, K):
    """pcg_cf_metrics with logits_ref and with `other`.  Rows with an exact tie for the maximum: the first index wins, as in
    torch.argmax; every other row has a top-two margin >= 1e-3, so the flip rate is float32(count) / float32(B) exactly.
    Gain: no earlier test of this kernel exists, so the bound is measured (cf_gain_bound): 4 x the mean distance between the row terms
    in float32 on the CPU and in float64 -- measured 8.5e-9 .. 2.4e-8 at B >= 255 over these shapes and both forms (7e-11 .. 3.2e-8
    for the single rows of B = 1), so the margin allows 3.4e-8 .. 9.8e-8, up to one and a half float32 ulp of a probability -- plus
    the (L + T + 2) u mean|terms| of the block's fp32 reduction; the bounds come to 1.3e-7 .. 4.2e-7 at B >= 255."""
    ops = pcg.ops
    lcf, lref, t, other = cf_inputs(B, K, 100 * B + K)
    hit64, _ = R.cf_metric_rows(lcf, t, lref)
    assert torch.equal(hit64, torch.argmax(lcf.float(), 1) == t)
    count = int(hit64.sum())
    flip_want = np.float32(count) / np.float32(B)
    lcfd, lrefd, td, od = _dev(lcf), _dev(lref), t.to(DEV), other.to(DEV)
    for form, (ref_arg, oth_arg, dref, doth) in {"logits_ref": (lref, None, lrefd, None), "other": (None, other, None, od)}.items():
        gain64, bound, dist = cf_gain_bound(lcf, ref_arg, t, oth_arg)
        out = ops.cf_metrics(lcfd, td, logits_ref=dref, other=doth).cpu()
        print(f"cf_metrics B={B} K={K} {form}: flips {count}, fp32-vs-float64 row distance {dist:.3g}, bound {bound:.3g}")
        assert np.float32(out[0].item()) == flip_want, f"flip rate {out[0].item()!r} != {count}/{B}"
        _within(out[1:2], torch.tensor([gain64]), bound, f"cf_metrics B={B} K={K} {form} gain")


# =================================================================================================================================
# reductions
# =================================================================================================================================
def _mean_bound_factor(n):
    """pcg_mean_fwd.  One block (n <= 16384): a thread adds ceil(n / 1024) elements in fp32 (L), the tree is fp64 (T = 0).  Otherwise
    64 blocks of 256 threads: L = ceil(n / 16384), an fp32 tree of 256 (T = 8), the 64 partials in fp64.  + 2: the fp64 stages' one
    final fp32 rounding and the rounding of the first term."""
    return (math.ceil(n / 1024) + 0 + 2) if n <= 16384 else (math.ceil(n / 16384) + 8 + 2)


def _abs_mean_bound_factor(n):
    """pcg_abs_mean_fwd.  One block: L = ceil(n / 1024) fp32 adds per thread (eight at a time, in order, then the tail), fp64 tree
    (T = 0).  Otherwise 256 blocks of 256 threads: L = ceil(n / 65536), fp32 tree of 256 (T = 8), fp64 finish.  + 2: the rounding of
    each product a * w and the final fp32 rounding."""
    return (math.ceil(n / 1024) + 0 + 2) if n <= 16384 else (math.ceil(n / 65536) + 8 + 2)


@pytest.mark.parametrize("n", REDUCE_NS)
def test_mean_and_abs_mean(pcg, n):
    """pcg_mean_fwd and pcg_abs_mean_fwd (no mask, mask, 1 - mask) on both forms, at the one-block limit 16384 / 16385, at the
    boundaries of abs_mean_small_kernel's 8-deep loop (n = 7 * 1024 + 1, 8 * 1024, 8 * 1024 + 1) and past the 4096-block grid."""
    ops = pcg.ops
    assert_route("MEAN", (n,), _reduce_route(n, 64))
    assert_route("ABS_MEAN", (n,), _reduce_route(n, 256))
    g = _gen(n)
    a = _randn(n, g=g) + 0.25
    a = R.f32_exact(a)
    m = torch.tensor([0.0, 0.25, 0.75, 1.0], dtype=torch.float64)[torch.randint(0, 4, (n,), generator=g)]      # 1 - m is exact
    ad, md = _dev(a), _dev(m)
    _within(ops.mean_fwd(ad), a.mean().reshape(1), _mean_bound_factor(n) * U * float(a.abs().sum()) / n, f"mean n={n}")
    for mask, om in ((None, False), (m, False), (m, True)):
        ref, mag = R.abs_mean(a, mask, om)
        got = ops.abs_mean_fwd(ad, md if mask is not None else None, om)
        _within(got, ref.reshape(1), _abs_mean_bound_factor(n) * U * float(mag) / n, f"abs_mean n={n} mask={mask is not None} one_minus={om}")


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_sumsq(pcg, n):
    """pcg_sumsq with and without accumulate.  L = ceil(n / 256) FMAs per thread, T = 9: six butterfly levels in the wave, three adds
    of the four wave sums; + 2: the add onto the old value and slack for the last rounding."""
    ops = pcg.ops
    g = _gen(n)
    p = _randn(n, g=g)
    old = _randn(1, g=g) * 3
    pd = _dev(p)
    factor = (math.ceil(n / 256) + 9 + 2) * U
    ssq = p.square().sum()
    out = torch.full((1,), SENT, dtype=torch.float32, device=DEV)
    ops.sumsq(pd, out)
    _within(out, ssq.reshape(1), factor * float(ssq), f"sumsq n={n}")
    out = _dev(old)
    ops.sumsq(pd, out, accumulate=True)
    _within(out, (ssq + old).reshape(1), factor * float(ssq + old.abs()), f"sumsq n={n} accumulate")


@pytest.mark.parametrize("nseg", [1, 16, 17, 45])
def test_norm_sum(pcg, nseg):
    """pcg_norm_sum over 1 (length 65), 16 (one per wave), 17 and 45 segments of lengths 0, 1, 63, 64, 65, ...: everything is fp64 until the one
    final fp32 rounding (L = T = 0), so the bound is 2 u * the sum of the norms."""
    ops = pcg.ops
    lengths = [[65, 0, 1, 63, 64, 130, 257][(k + nseg - 1) % 7] for k in range(nseg)]       # one segment: 65; more: zero lengths among them
    assert lengths[0] > 0 or nseg > 1
    gap = 3
    offs, pos = [], 5
    for ln in lengths:
        offs.append(pos)
        pos += ln + gap
    g = _gen(nseg)
    flat = _randn(pos + 7, g=g)
    seg = torch.tensor(list(zip(offs, lengths)), dtype=torch.int64)
    ref = R.norm_sum(flat, seg.tolist())
    got = ops.norm_sum(_dev(flat), seg.to(DEV))
    _within(got, ref.reshape(1), 2 * U * float(ref), f"norm_sum {nseg} segments")


# =================================================================================================================================
# embedding gradient
# =================================================================================================================================
def _embed_inputs(B, HW, K, C, absent, seed):
    g = _gen(seed)
    present = [k for k in range(K) if k not in absent]
    idx = torch.tensor(present)[torch.randint(0, len(present), (B,), generator=g)]
    dinp = _randn(B, HW, C, g=g)
    base = _randn(K, HW, g=g)
    return idx, dinp, base


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("B", EMBED_BS)
def test_embed_concat_bwd(pcg, B, C):
    """pcg_embed_concat_bwd on both forms (the batch split over 16 thread groups from B = 64, one pass below), with and without dx,
    without the table, and accumulating.  Classes 3 and 8 never appear: their rows stay zero, or untouched under accumulate.  Table
    gradient against float64 index_add_, (B + 17) u sum|terms|; dx is a copy, bit-exact."""
    ops = pcg.ops
    HW, K, absent = 49, 10, (3, 8)
    idx, dinp, base = _embed_inputs(B, HW, K, C, absent, 17 * B + C)
    dd, idxd = _dev(dinp), idx.to(DEV)
    factor = (B + 17) * U
    # fresh table + dx
    assert_route("EMBED_CONCAT_BWD", (B, 1, 1), _embed_route(B, 1, 1))
    dt = torch.full((K, HW), SENT, dtype=torch.float32, device=DEV)
    dx = ops.embed_concat_bwd(dd, idxd, C, K, dtable=dt, accumulate=False, need_dx=True)
    ref, mag = R.embed_table_grad(dinp, idx, K, 1)
    _within(dt, ref, factor * mag, f"embed B={B} C={C} dtable")
    assert bool((dt[list(absent)] == 0).all()), "rows of absent classes must be zero"
    _bit_equal(dx, dinp[..., 0], f"embed B={B} C={C} dx")
    # accumulate, no dx
    assert_route("EMBED_CONCAT_BWD", (B, 1, 0), _embed_route(B, 1, 0))
    dt = _dev(base)
    assert ops.embed_concat_bwd(dd, idxd, C, K, dtable=dt, accumulate=True, need_dx=False) is None
    ref, mag = R.embed_table_grad(dinp, idx, K, 1, base)
    _within(dt, ref, factor * mag, f"embed B={B} C={C} dtable accumulate")
    _bit_equal(dt[list(absent)], base[list(absent)], f"embed B={B} C={C} absent rows under accumulate")
    # dx alone
    assert_route("EMBED_CONCAT_BWD", (B, 0, 1), _embed_route(B, 0, 1))
    dx = ops.embed_concat_bwd(dd, idxd, C, K, dtable=None, need_dx=True)
    _bit_equal(dx, dinp[..., 0], f"embed B={B} C={C} dx alone")


@pytest.mark.parametrize("C,ch", [(1, 0), (5, 3)])
@pytest.mark.parametrize("B", [7, 133])
def test_embed_table_grad(pcg, B, C, ch):
    """pcg_embed_table_grad (always the batch-split kernel) from any channel of any channel count, fresh and accumulating."""
    ops = pcg.ops
    HW, K, absent = 49, 10, (3, 8)
    idx, dinp, base = _embed_inputs(B, HW, K, C, absent, 23 * B + C)
    dd, idxd = _dev(dinp), idx.to(DEV)
    factor = (B + 17) * U
    dt = torch.full((K, HW), SENT, dtype=torch.float32, device=DEV)
    ops.embed_table_grad(dd, idxd, C, ch, K, dt)
    ref, mag = R.embed_table_grad(dinp, idx, K, ch)
    _within(dt, ref, factor * mag, f"embed_table_grad B={B} C={C} ch={ch}")
    assert bool((dt[list(absent)] == 0).all())
    dt = _dev(base)
    ops.embed_table_grad(dd, idxd, C, ch, K, dt, accumulate=True)
    ref, mag = R.embed_table_grad(dinp, idx, K, ch, base)
    _within(dt, ref, factor * mag, f"embed_table_grad B={B} C={C} ch={ch} accumulate")
    _bit_equal(dt[list(absent)], base[list(absent)], "absent rows under accumulate")


# =================================================================================================================================
# element-wise ops: bit-exact against the same fp32 expression on the CPU
# =================================================================================================================================
def _act_grad_cpu(dy, y, act, slope):
    one, s = torch.ones_like(y), torch.full_like(y, slope)
    if act == ACT_RELU:
        return dy * torch.where(y > 0, one, torch.zeros_like(y))
    if act == ACT_LRELU:
        return dy * torch.where(y > 0, one, s)
    if act == ACT_TANH:
        return dy * (1.0 - y * y)
    return dy * (y * (1.0 - y))


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: f"n{c[0]}{'-misaligned' if c[1] else ''}")
def test_act_bwd(pcg, case):
    """pcg_act_bwd: float4 lanes and scalar lanes (n % 4 != 0, or a view one float off alignment), and the float4 grid-stride loop
    walked twice.  The four activations at the small sizes, LeakyReLU at the large ones.  tanh's 1 - y * y may be contracted to an
    FMA: its y are multiples of 2^-8, whose squares and 1 - y^2 are exact, so the bit comparison holds either way."""
    n, mis = case
    ops = pcg.ops
    assert_route("ACT", (n, not mis), _act_route(n, not mis))
    g = _gen(n)
    dy = torch.randn(n, generator=g)
    acts = (ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID) if n < 10 ** 6 else (ACT_LRELU,)
    put = _off_by_one_float if mis else _dev
    dyd = put(dy)
    for act in acts:
        if act == ACT_TANH:
            y = torch.randint(-255, 256, (n,), generator=g).float() / 256
        elif act == ACT_SIGMOID:
            y = torch.rand(n, generator=g)
        else:
            y = torch.randn(n, generator=g)
        slope = 0.2
        want = _act_grad_cpu(dy, y, act, np.float32(slope).item())
        out = put(torch.full((n,), SENT))
        assert out.data_ptr() % 16 == (4 if mis else 0)
        ops.act_bwd(dyd, put(y), act, slope, out=out)
        _bit_equal(out, want, f"act_bwd act={act} n={n}")


@pytest.mark.parametrize("shape", [(6, 4, 256), (3, 49, 20)])
def test_avgpool(pcg, shape):
    """pcg_avgpool_fwd (positions added in order, one division) and pcg_avgpool_bwd (dy times the rounded 1 / HW)."""
    ops = pcg.ops
    B, HW, C = shape
    g = _gen(HW)
    x, dy = torch.randn(B, HW, C, generator=g), torch.randn(B, C, generator=g)
    s = torch.zeros(B, C)
    for p in range(HW):
        s = s + x[:, p, :]
    _bit_equal(ops.avgpool_fwd(_dev(x), B, HW, C), s / float(HW), f"avgpool_fwd {shape}")
    _within(ops.avgpool_fwd(_dev(x), B, HW, C), R.avgpool_fwd(x.double()), (HW + 1) * U * x.double().abs().mean(1), f"avgpool_fwd {shape} vs float64")
    inv = torch.tensor(1.0) / torch.tensor(float(HW))
    _bit_equal(ops.avgpool_bwd(_dev(dy), B, HW, C), (dy * inv)[:, None, :].expand(B, HW, C), f"avgpool_bwd {shape}")
    _within(ops.avgpool_bwd(_dev(dy), B, HW, C), R.avgpool_bwd(dy.double(), HW), 2 * U * R.avgpool_bwd(dy.double().abs(), HW), f"avgpool_bwd {shape} vs float64")


@pytest.mark.parametrize("rows", GATHER_ROWS)
def test_gather_channel(pcg, rows):
    """pcg_gather_channel: each channel of three; one row, two blocks, and more rows than its 1024-block grid covers in one pass."""
    ops = pcg.ops
    assert_route("ELEMENTWISE", ("EW_GATHER_CHANNEL", rows), _ew_route(rows, 1024))
    t = torch.randn(rows, 3, generator=_gen(rows))
    td = _dev(t)
    for ch in range(3):
        _bit_equal(ops.gather_channel(td, ch), t[:, ch:ch + 1], f"gather_channel rows={rows} ch={ch}")


def test_dropout_apply(pcg):
    """pcg_dropout_apply, one mask entry per element (inner = 1) and per (sample, channel) of an NHWC activation (inner = HW)."""
    ops = pcg.ops
    g = _gen(3)
    p = 0.3
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    x, m = torch.randn(5001, generator=g), (torch.rand(5001, generator=g) > p).float()
    _bit_equal(ops.dropout_apply(_dev(x), _dev(m), p, inner=1, C=1), x * m * scale, "dropout inner=1")
    B, HW, C = 3, 49, 20
    x, m = torch.randn(B, HW, C, generator=g), (torch.rand(B, C, generator=g) > p).float()
    assert 0 < int(m.sum()) < B * C
    _bit_equal(ops.dropout_apply(_dev(x), _dev(m), p, inner=HW, C=C), x * m[:, None, :] * scale, "dropout inner=HW")


@pytest.mark.parametrize("form", ["d_raw", "d_masked", "both", "no mask"])
def test_scale_mask_bwd(pcg, form):
    """pcg_scale_mask_bwd, dc = s (d_raw + d_masked * mask), in its three null-pointer forms and with both gradients.  With one
    gradient, or without a mask, no product meets a sum: bit-exact on random inputs.  With both gradients and a mask the multiply-add
    may be contracted: bit-exact on dyadic inputs, float64 within three roundings on random ones (_contractable)."""
    ops = pcg.ops
    n, s = 5003, 0.75
    g = _gen(len(form))
    for exact in (True, False):
        mk = _dyadic if exact else _randn
        d_raw, d_masked = mk(n, g=g), mk(n, g=g)
        mask = (torch.rand(n, generator=g) > 0.4).double() if exact else torch.rand(n, generator=g, dtype=torch.float64).float().double()
        use_raw, use_masked, use_mask = form in ("d_raw", "both", "no mask"), form != "d_raw", form != "no mask"
        mk_ = mask if use_mask else torch.ones(n, dtype=torch.float64)
        exact64 = s * ((d_raw if use_raw else 0) + (d_masked * mk_ if use_masked else 0))
        mag = abs(s) * ((d_raw.abs() if use_raw else 0) + ((d_masked * mk_).abs() if use_masked else 0))
        f = lambda t: t.float()
        cpu32 = torch.tensor(s) * ((f(d_raw) if use_raw else torch.zeros(n)) + (f(d_masked) * f(mk_) if use_masked else torch.zeros(n)))
        like = torch.empty(n, dtype=torch.float32, device=DEV)
        got = ops.scale_mask_bwd(_dev(d_raw) if use_raw else None, _dev(d_masked) if use_masked else None, _dev(mask) if use_mask else None, s, like)
        if exact or form != "both":
            _bit_equal(got, cpu32, f"scale_mask_bwd {form} {'dyadic' if exact else 'random'}")
        else:
            _contractable(got, exact64, 3, mag, f"scale_mask_bwd {form} random")


@pytest.mark.parametrize("shape", [(77, 17), (70000, 16)])
def test_add_bias_rows(pcg, shape):
    ops = pcg.ops
    rows, C = shape
    assert_route("ELEMENTWISE", ("EW_POINTWISE", rows * C), _ew_route(rows * C, 8192))
    g = _gen(rows)
    x, b = torch.randn(rows, C, generator=g), torch.randn(C, generator=g)
    xd = _dev(x)
    assert ops.add_bias_rows(xd, C, _dev(b)) is xd
    _bit_equal(xd, x + b, f"add_bias_rows {shape}")


def test_axpby(pcg):
    """pcg_axpby, out = a x (+ b y): without y a product (bit-exact); with y the multiply-add may be contracted (bit-exact on dyadic
    inputs, float64 within three roundings on random ones); out aliasing x."""
    ops = pcg.ops
    n, a, b = 5003, 0.75, -1.5
    g = _gen(9)
    x, y = _randn(n, g=g), _randn(n, g=g)
    _bit_equal(ops.axpby(a, _dev(x)), torch.tensor(a) * x.float(), "axpby without y")
    _contractable(ops.axpby(a, _dev(x), b, _dev(y)), a * x + b * y, 3, (a * x).abs() + (b * y).abs(), "axpby random")
    xq, yq = _dyadic(n, g=g), _dyadic(n, g=g)
    want = torch.tensor(a) * xq.float() + torch.tensor(b) * yq.float()
    assert torch.equal(want.double(), a * xq + b * yq)                           # nothing rounds
    _bit_equal(ops.axpby(a, _dev(xq), b, _dev(yq)), want, "axpby dyadic")
    xd = _dev(xq)
    assert ops.axpby(a, xd, b, _dev(yq), out=xd) is xd
    _bit_equal(xd, want, "axpby out aliasing x")


@pytest.mark.parametrize("n", [1, 3, 8])
def test_weighted_sum(pcg, n):
    """pcg_weighted_sum_fwd (an explicit FMA chain in term order: bit-exact on dyadic inputs, float64 within n roundings on random
    ones) and pcg_weighted_sum_bwd (a product per term, bit-exact) with holes in the needs list; nine terms are refused."""
    ops = pcg.ops
    g = _gen(n)
    for exact in (True, False):
        vals = (_dyadic if exact else _randn)(n, g=g)
        ws = (_dyadic if exact else _randn)(n, g=g)
        terms = [_dev(vals[i:i + 1]) for i in range(n)]
        got = ops.weighted_sum_fwd(terms, ws.tolist())
        if exact:
            _bit_equal(got, (ws * vals).sum().reshape(1), f"weighted_sum_fwd n={n} dyadic")
        else:
            _contractable(got, (ws * vals).sum().reshape(1), n, float((ws * vals).abs().sum()), f"weighted_sum_fwd n={n} random")
    go = torch.randn(1, generator=g)
    needs = [i % 3 != 1 for i in range(n)]
    outs = ops.weighted_sum_bwd(ws.tolist(), _dev(go), needs)
    assert [o is not None for o in outs] == needs
    for i, o in enumerate(outs):
        if o is not None:
            _bit_equal(o, ws[i:i + 1].float() * go, f"weighted_sum_bwd term {i}")
    if n == 8:
        nine = [_dev(torch.ones(1)) for _ in range(9)]
        with pytest.raises(pcg.PcgError, match="at most 8 terms"):
            ops.weighted_sum_fwd(nine, [1.0] * 9)
        with pytest.raises(pcg.PcgError):
            ops.weighted_sum_bwd([1.0] * 9, _dev(go), [True] * 9)


@pytest.mark.parametrize("n", CF_BIG_NS)
def test_cf_ops_grid_stride(pcg, n):
    """clamp_add_fwd / _bwd and scale_mask_fwd past 4096 blocks and past the 8192-block grid of cf_ops.hip, where the stride loop of
    an element-wise kernel walks a second pass with a ragged tail."""
    ops = pcg.ops
    assert_route("ELEMENTWISE", ("EW_CF_OPS", n), _ew_route(n, 8192))
    g = _gen(n % 1000)
    x, r, dy = torch.rand(n, generator=g) * 2 - 1, torch.randn(n, generator=g) * 0.5, torch.randn(n, generator=g)
    m = (torch.rand(n, generator=g) > 0.4).float()
    xd, rd = _dev(x), _dev(r)
    _bit_equal(ops.clamp_add_fwd(xd, rd, -1.0, 1.0), torch.clamp(x + r, -1.0, 1.0), f"clamp_add_fwd n={n}")
    inside = ((x + r) >= -1) & ((x + r) <= 1)
    _bit_equal(ops.clamp_add_bwd(_dev(dy), xd, rd, -1.0, 1.0), dy * inside, f"clamp_add_bwd n={n}")
    raw, masked = ops.scale_mask_fwd(rd, _dev(m), 0.1)
    s = torch.tensor(0.1)
    _bit_equal(raw, s * r, f"scale_mask_fwd raw n={n}")
    _bit_equal(masked, s * r * m, f"scale_mask_fwd masked n={n}")
    raw, masked = ops.scale_mask_fwd(rd[:5001], None, 0.1)
    _bit_equal(masked, s * r[:5001], "scale_mask_fwd without mask")


def test_tabular_grid_stride(pcg):
    """concat_cols / split_cols / film_bwd of tabular.hip past its 4096-block grid: the second pass of the stride loop."""
    ops = pcg.ops
    rows, ca, cb = TABULAR_BIG
    n = rows * (ca + cb)
    assert_route("ELEMENTWISE", ("EW_TABULAR", n), "4096 blocks of 256: 2 passes")
    g = _gen(4)
    a, b = torch.randn(rows, ca, generator=g), torch.randn(rows, cb, generator=g)
    cat = ops.concat_cols(_dev(a), _dev(b))
    _bit_equal(cat, torch.cat([a, b], 1), "concat_cols")
    da, db = ops.split_cols(cat, ca, cb)
    _bit_equal(da, a, "split_cols a")
    _bit_equal(db, b, "split_cols b")
    dy, gm, h = (torch.randn(n, generator=g) for _ in range(3))
    dg, dh = ops.film_bwd(_dev(dy), _dev(gm), _dev(h))
    _bit_equal(dg, dy * h, "film_bwd dg")
    _bit_equal(dh, dy * gm, "film_bwd dh")
