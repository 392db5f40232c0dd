"""GPU: the convolutions and the other users of the shared scratch inside NaN-guarded, exact-size, 16-byte-aligned buffers
(tests/arena.py; DESIGN.md "Guarded buffers").

No new shapes and no new tolerances: the case tables, float64 references and bounds are imported from the files that own them.  What is
new is where the tensors live.  Every operand, output and caller-supplied buffer of a call sits in its own [guard | payload | guard]
allocation whose payload is aligned to 16 bytes and no better and whose guards read as NaN; ops._scratch is replaced so that every
workspace request returns exactly the bytes the library's size query asked for, filled with NaN.  After the call

  * no guard byte has changed (stores stay inside the tensor, scratch use stays inside the advertised bytes),
  * every output element was written and is finite (a load that strays into a guard and is masked by a multiplication gives NaN;
    a slab or partial row nobody wrote in this call is NaN, not a plausible stale number),
  * the result is within the source file's bound of its float64 reference,

and the plan string is asserted first, as in the source table, so no case drifts to another kernel.  Not guarded: the 64 MiB stream-K
parts buffer (the library's, held for the life of the process) and outputs a wrapper allocates itself.

test_every_family_ran_its_whole_table (last) compares the number of cases that ran per family with the length of the imported table,
so it needs the whole module to have run."""
import collections
import contextlib
import ctypes
import functools
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arena as A
import test_hip_benchshape as BS
import test_hip_dgrad_clip_iter as DC
import test_hip_groups as TG
import test_hip_igemm_branches as IG
import test_hip_norm_branches as NB
import test_hip_ops as HO
import test_hip_pad_clip as PC
import test_hip_small_ops as SO
import test_hip_thin_conv as TH
import test_hip_wgrad_padskip as PS
import test_hip_wgrad_pixtab as PT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, DGRAD, WGRAD = 0, 1, 2
F32 = torch.float32

RAN = collections.defaultdict(set)         # family -> ids of the cases that ran (not: passed)


def _marks(fn):
    """The parametrize lists of an imported test function, by argument names (tables some source files keep in their decorators)."""
    return {m.args[0]: list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"}


CLIP_ITER = _marks(DC.test_tap_walk_both_orders_and_k_tail)
CLIP_ITER_CASES = [(ih, co, ko) for ih in CLIP_ITER["IH"] for co in CLIP_ITER["Cout"] for ko in CLIP_ITER["korder"]]
PADSKIP_DP = _marks(PS.test_data_parallel_kernels)
PADSKIP_DP_CASES = [(h,) + tuple(c) for h in PADSKIP_DP["H"] for c in PADSKIP_DP["Cin,Cout,B"]]          # (H, Cin, Cout, B)
PADSKIP_SK_CASES = [tuple(c) for c in _marks(PS.test_stream_k_kernel)["H,B"]]                             # (H, B) at 448 -> 160
PADSKIP_PAIRED_CASES = [tuple(c) for c in _marks(PS.test_paired_block_order_at_512_workgroups)["H,B,Cin,Cout"]]
PIXTAB_CASES = list(PT.CASES) + [PT.SK_CASE]
_FULL = _marks(HO.test_full_window_grad_input_through_batchnorm_backward)
FULL_BNBWD_CASES = [tuple(bg) + tuple(a) for bg in _FULL["B,groups"] for a in _FULL["act,slope"]]                 # (B, groups, act, slope)

FAMILY_SIZES = {
    "igemm": lambda: 2 * len(IG.CASES),
    "thin": lambda: len(TH.CASES),
    "thin-mask": lambda: 2 * len(TH.MASK_CASES),
    "thin-bnbwd": lambda: 2 * len(TH.BNBWD_CASES),
    "full-bnbwd": lambda: len(_FULL["B,groups"]) * len(_FULL["act,slope"]),
    "pad-clip": lambda: len(PC.CASES),
    "dgrad-clip-iter": lambda: len(CLIP_ITER["IH"]) * len(CLIP_ITER["Cout"]) * len(CLIP_ITER["korder"]),
    "wgrad-padskip": lambda: (len(PADSKIP_DP["H"]) * len(PADSKIP_DP["Cin,Cout,B"]) + len(_marks(PS.test_stream_k_kernel)["H,B"])
                              + len(_marks(PS.test_paired_block_order_at_512_workgroups)["H,B,Cin,Cout"])),
    "wgrad-pixtab": lambda: len(PT.CASES) + 1,
    "epilogue": lambda: sum(1 for f in IG.EPI_FORMS for k in (3, 4) if f[k] is not None),
    "xform": lambda: len(IG.XF_FORMS),
    "grouped-fwd": lambda: len(IG.GROUPED_FWD),
    "grouped-dgrad": lambda: len(IG.GROUPED_DGRAD),
    "bn-stats": lambda: len(NB.BN_CASES),
    "bn-bwd": lambda: len(NB.BN_CASES),
    "bn-partial": lambda: len(NB.BN_PARTIAL_SHAPES) * len(NB.BN_PARTIAL_NPARTS),
    "linear-wgrad": lambda: len(SO.LINEAR_WGRAD_CASES),
    "linear-wgrad-grouped": lambda: len(SO.WGRAD_GROUPED_CASES),
    "reduce": lambda: len(SO.REDUCE_NS),
}


# ---- arena bytes per case, from the geometry and the size queries (host only: tests/test_arena_host.py) --------------------------
def _conv_case_bytes(lib, shape, extra=()):
    """Upper bound of one conv case: x, w, dy, the biases, a forward output, a grad-input output, two weight gradients, and one exact
    scratch request per size query of the geometry; `extra`: further (shape, dtype) tensors."""
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    g = IG._geom(shape)
    t = [(B, H, W, Cin)] * 2 + [(B, g.OH, g.OW, Cout)] * 2 + [(Cout, KH, KW, Cin)] * 3 + [(Cout,), (Cin,)]
    n = sum(A.arena_bytes(s_) for s_ in t) + sum(A.arena_bytes(s_, d) for s_, d in extra)
    for q in ("pcg_conv2d_fwd_workspace_bytes", "pcg_conv2d_dgrad_workspace_bytes", "pcg_conv2d_wgrad_workspace_bytes",
              "pcg_conv2d_fwd_bn_workspace_bytes", "pcg_conv2d_dgrad_bn_workspace_bytes"):
        n += 2 * A.scratch_bytes(getattr(lib, q)(ctypes.byref(g)))
    return n


def _thin9(shape):
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = TH._k2(k)
    return (B, Cin, Cout, H, W, kh, kw, s, p)


def _k4(B, Cin, Cout, H):
    return (B, Cin, Cout, H, H, 4, 4, 2, 1)


def case_arena_bytes():
    """(family, case id, bytes of all arena allocations of the case) for every case this module runs."""
    from pcgan_amd import _lib
    lib = _lib.load()
    for cid, shape, op, tune, want in IG.CASES:
        with IG._tuned(lib, tune):
            n = _conv_case_bytes(lib, shape)
        for prec in ("fp32", "bf16"):
            yield "igemm", f"{cid}-{prec}", n
    for name, shape in TH.CASES:
        yield "thin", name, _conv_case_bytes(lib, _thin9(shape))
    for name, shape in TH.MASK_CASES:
        for act in (1, 2):
            yield "thin-mask", f"{name}-{act}", _conv_case_bytes(lib, _thin9(shape))
    for name, shape in TH.BNBWD_CASES:
        s9 = _thin9(shape)
        g = IG._geom(s9)
        out = (g.B, g.OH, g.OW, g.Cout)
        n = _conv_case_bytes(lib, s9, [(out, F32)] * 2) + 2 * A.scratch_bytes(lib.pcg_conv2d_fwd_bnbwd_thin_workspace_bytes(ctypes.byref(g)))
        for act in (1, 2):
            yield "thin-bnbwd", f"{name}-{act}", n
    for B, groups, act, slope in FULL_BNBWD_CASES:
        g = IG._geom((B, 512, 1, 4, 4, 4, 4, 1, 0))
        yield "full-bnbwd", f"{B}-{groups}-{act}", (3 * A.arena_bytes((B, 4, 4, 512)) + 12 * A.arena_bytes((groups, 512))
                                                   + (2 + 2 * groups) * A.scratch_bytes(max(lib.pcg_conv2d_dgrad_bnbwd_full_workspace_bytes(ctypes.byref(g), groups),
                                                                                            lib.pcg_bn_workspace_bytes(B * 16, 512))))
    for (form, IH, Cin, Cout, B, modes), cid in zip(PC.CASES, PC.IDS):
        yield "pad-clip", cid, (1 + len(modes)) * _conv_case_bytes(lib, _k4(B, Cin, Cout, IH))
    for IH, Cout, korder in CLIP_ITER_CASES:
        yield "dgrad-clip-iter", f"{IH}-{Cout}-{korder}", (1 + len(PC.ORDERS)) * _conv_case_bytes(lib, _k4(DC.B, DC.CIN, Cout, IH))
    for H, Cin, Cout, B in PADSKIP_DP_CASES:
        yield "wgrad-padskip", f"dp-{H}-{Cin}-{Cout}-{B}", _wgrad_case_bytes(lib, _k4(B, Cin, Cout, H), 2 * 2 * 4 * 2)
    for H, B in PADSKIP_SK_CASES:
        yield "wgrad-padskip", f"sk-{H}-{B}", _wgrad_case_bytes(lib, _k4(B, 448, 160, H), 2 * 4 * 2 + 4)
    for H, B, Cin, Cout in PADSKIP_PAIRED_CASES:
        yield "wgrad-padskip", f"paired-{H}-{B}", _wgrad_case_bytes(lib, _k4(B, Cin, Cout, H), 4)
    for name, B, Cin, Cout, H, k, s, p in PIXTAB_CASES:
        yield "wgrad-pixtab", name, _wgrad_case_bytes(lib, (B, Cin, Cout, H, H, k, k, s, p), 4)
    for form in IG.EPI_FORMS:
        with IG._tuned(lib, form[2]):
            g = IG._geom(form[1])
            for k, oshape in ((3, (g.B, g.OH, g.OW, g.Cout)), (4, (g.B, g.IH, g.IW, g.Cin))):
                if form[k] is not None:       # 16 tensors of the output's shape (outputs, aux, dz) and the per-channel vectors
                    yield "epilogue", f"{form[0]}-{'dgrad' if k == 4 else 'fwd'}", _conv_case_bytes(lib, form[1], [(oshape, F32)] * 16 + [((2 * oshape[3],), F32)] * 24)
    for prm in IG.XF_FORMS:
        form = prm.values[0]
        g = IG._geom(form[1])
        yield "xform", form[0], _conv_case_bytes(lib, form[1], [((g.B, g.IH, g.IW, g.Cin), F32), ((g.B, g.OH, g.OW, g.Cout), F32)] + [((g.Cout, g.KH, g.KW, g.Cin), F32)] * 2)
    for B, Cin, Cout, H, groups in IG.GROUPED_FWD:
        yield "grouped-fwd", f"{B}-{Cin}-{Cout}-{H}-{groups}", _conv_case_bytes(lib, _k4(B, Cin, Cout, H), [((groups, Cout), F32)] * 4)
    for rows, C, *_ in NB.BN_CASES:
        n = 4 * A.arena_bytes((rows, C)) + 12 * A.arena_bytes((2 * C,)) + 2 * A.scratch_bytes(lib.pcg_bn_workspace_bytes(rows, C))
        yield "bn-stats", f"{rows}x{C}", n + 2 * A.scratch_bytes(lib.pcg_colsum_workspace_bytes(rows, C))
        yield "bn-bwd", f"{rows}x{C}", n + 2 * A.arena_bytes((rows, C)) + 2 * A.scratch_bytes(lib.pcg_bn_db_workspace_bytes(rows, C))
    for rows, C in NB.BN_PARTIAL_SHAPES:
        for nparts in sorted(NB.BN_PARTIAL_NPARTS):
            yield "bn-partial", f"{rows}x{C}-{nparts}", (4 * A.arena_bytes((rows, C)) + 12 * A.arena_bytes((C,))
                                                        + 2 * A.arena_bytes((nparts * 2 * C + 257 * 2 * C + 4 * C,), torch.float64)
                                                        + A.scratch_bytes(lib.pcg_bn_bwd_partial_workspace_bytes(C))
                                                        + A.scratch_bytes(lib.pcg_bn_bwd_partial_db_workspace_bytes(C)))
    for B, O, I in sorted(SO.LINEAR_WGRAD_CASES):
        yield "linear-wgrad", f"{B}x{O}x{I}", (A.arena_bytes((B, O + 5)) + A.arena_bytes((B, I)) + 2 * A.arena_bytes((O, I)) + 2 * A.arena_bytes((O,))
                                               + 4 * A.scratch_bytes(lib.pcg_linear_wgrad_workspace_bytes(B, O, I)))
    for B in sorted(SO.WGRAD_GROUPED_CASES):
        yield "linear-wgrad-grouped", str(B), 8 * A.arena_bytes((B, 40)) + 8 * A.arena_bytes((33, 33)) + 2 * A.scratch_bytes(1 << 22)
    for n in SO.REDUCE_NS:
        yield "reduce", str(n), 2 * A.arena_bytes((n,)) + A.scratch_bytes(lib.pcg_mean_workspace_bytes()) + 3 * A.scratch_bytes(lib.pcg_abs_mean_workspace_bytes())
    for B, Cin, Cout, H, groups in IG.GROUPED_DGRAD:
        yield "grouped-dgrad", f"{B}-{Cin}-{Cout}-{H}-{groups}", _conv_case_bytes(lib, _k4(B, Cin, Cout, H), [((B, H, H, Cin), F32)] * 3 + [((groups, Cin), F32)] * 6)


def _wgrad_case_bytes(lib, shape, launches):
    """x, dy and per launch one weight gradient and one exact scratch request."""
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    g = IG._geom(shape)
    ws = lib.pcg_conv2d_wgrad_workspace_bytes(ctypes.byref(g))
    return (A.arena_bytes((B, H, W, Cin)) + A.arena_bytes((B, g.OH, g.OW, Cout))
            + launches * (A.arena_bytes((Cout, KH, KW, Cin)) + A.scratch_bytes(ws)))


# ---- fixtures and helpers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import dcgan  # noqa: F401
    lib = pcgan_amd.load()
    pcgan_amd.ops._conv_scratch()           # this stream's stream-K scratch before the first workspace query (it plans with it)
    try:
        yield pcgan_amd
    finally:
        for name in IG.SWITCHES + ("pad_clip", "pad_clip_dgrad", "wgrad_padskip", "wgrad_pixtab"):
            lib.pcg_tune_set(name.encode(), -1)
        lib.pcg_conv_precision_set(0)


@pytest.fixture()
def guarded(pcg, monkeypatch):
    """(arena on the device, log of the exact scratch requests): ops._scratch is replaced until the test ends."""
    ar = A.Arena(DEV)
    return ar, A.exact_scratch(monkeypatch, ar)


def _f32(t):
    return t.detach().float().contiguous()


def _settle(ar):
    """Steps 4 - 6 of every case: synchronize, no guard byte changed, every output element written and finite."""
    torch.cuda.synchronize()
    ar.check()


def _arrivals_are_zero(ops):
    st = torch.cuda.current_stream()
    parts, arrivals = ops._sk_streams[(st.device_index, st.cuda_stream)]
    assert int(arrivals.view(torch.int32).abs().sum()) == 0, "stream-K arrival counters are not back to zero"


@contextlib.contextmanager
def _tune(ops, **switches):
    try:
        for k, v in switches.items():
            ops.tune(k, v)
        yield
    finally:
        for k in switches:
            ops.tune(k, -1)


# forward cases that plan_fwd cuts into K-slices although pcg_conv_plan_describe does not say so at N <= 64 (the source table's comment:
# "4 K-slices of 8 k-tiles (1 x 2 tiles, 32 k-tiles)"): case id -> K-slices
UNNAMED_K_SLICES = {"fwd-128x64-s2-korder0": 4, "fwd-128x64-s2-korder1": 4}


@functools.lru_cache(maxsize=None)
def _ig_operands(cid, shape):
    return IG._operands(shape, IG._seed(cid))


# ---- implicit-GEMM forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in IG.CASES])
def test_igemm_form_in_guarded_buffers(pcg, guarded, case, precision):
    """Every entry of test_hip_igemm_branches.CASES, fp32 and bf16.  Weight gradient: accumulate=False into an output, accumulate=True
    into an inout that starts from that result (the source test's 2 x reference).  The exact scratch was stored into if and only if the
    plan says `slabs` or `GEMM + col2im`: an under-reporting size query would drop the launch to one K-slice with the result still right."""
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    cid, shape, op, tune, want = case
    RAN["igemm"].add((cid, precision))
    B, Cin, Cout, H, W, KH, KW, s, p = shape
    g = ops.conv_geom(B, H, W, Cin, Cout, KH, KW, s, p)
    x, w, dy, b, bx = _ig_operands(cid, shape)
    bf16 = precision == "bf16"
    got2 = None
    with IG._tuned(lib, tune):
        plan = IG._describe(lib, shape, op)
        assert plan == IG._expected_plan(want), f"plan moved: {plan!r} (expected {want!r})"
        wd = ar.input(_f32(IG._nhwc(w)), "w")
        with ops.conv_precision(precision):
            if op == FWD:
                got = ops.conv2d_fwd(g, ar.input(_f32(IG._nhwc(x)), "x"), wd, ar.input(_f32(b), "bias"),
                                     out=ar.output((B, g.OH, g.OW, Cout), name="y"))
            elif op == DGRAD:
                got = ops.conv2d_dgrad(g, ar.input(_f32(IG._nhwc(dy)), "dy"), wd, ar.input(_f32(bx), "bias_x"),
                                       out=ar.output((B, H, W, Cin), name="dx"))
            else:
                xd, dyd = ar.input(_f32(IG._nhwc(x)), "x"), ar.input(_f32(IG._nhwc(dy)), "dy")
                got = ar.output((Cout, KH, KW, Cin), name="dw")
                ops.conv2d_wgrad(g, xd, dyd, got, accumulate=False)
                got2 = ar.inout(got, "dw (accumulate)")
                ops.conv2d_wgrad(g, xd, dyd, got2, accumulate=True)
    _settle(ar)
    uses_scratch = "slabs" in plan or "GEMM + col2im" in plan
    if cid in UNNAMED_K_SLICES:
        # the one form whose K-slices the plan string does not name (N <= 64; see the comment at the case in the source table): the
        # scratch must be exactly the table's number of [M][Cout] fp32 slabs, and it must have been used
        assert "slabs" not in plan and [r.nbytes for r in log] == [UNNAMED_K_SLICES[cid] * B * g.OH * g.OW * Cout * 4]
        uses_scratch = True
    for r in log:
        assert r.changed == uses_scratch, f"scratch of {r.nbytes} bytes {'was' if r.changed else 'was not'} stored into; plan {plan!r}"
    if uses_scratch:
        assert len(log) == (2 if op == WGRAD else 1) and all(r.nbytes > 0 for r in log), f"{log} for plan {plan!r}"
    if "stream-K" in plan:
        _arrivals_are_zero(ops)

    xr, wr, dyr = (IG._bf(x), IG._bf(w), IG._bf(dy)) if bf16 else (x, w, dy)
    if op == FWD:
        want64 = IG._fwd64(xr, wr, s, p, b)
    elif op == DGRAD:
        want64 = IG._dgrad64(x.shape, wr, dyr, s, p, bx)
    else:
        want64 = IG._wgrad64(xr, w.shape, dyr, s, p)
    taps = KH * KW
    if not bf16:
        K, scale = {FWD: (taps * Cin, 4.0), DGRAD: (taps * Cout, 4.0), WGRAD: (B * g.OH * g.OW, 8.0)}[op]
        bound = IG._tol(K, scale)
    else:
        Kf = taps * Cin
        bound = {FWD: IG._bf16_bound(Kf, 1 / math.sqrt(Kf)),
                 DGRAD: IG._bf16_bound(Cout * ((KH + s - 1) // s) * ((KW + s - 1) // s), 1 / math.sqrt(Kf)),
                 WGRAD: IG._bf16_bound(B * g.OH * g.OW, 1.0)}[op]
    err = IG._err(got, want64)
    assert err <= bound, f"{cid} {precision}: max err {err:.3e} > {bound:.3e}"
    if got2 is not None:
        err = IG._err(got2, 2 * want64)
        assert err <= 2 * bound, f"{cid} {precision}: accumulate max err {err:.3e} > {2 * bound:.3e}"


# ---- thin convolutions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TH._params(TH.CASES))
def test_thin_conv_in_guarded_buffers(pcg, guarded, shape):
    """Every entry of test_hip_thin_conv.CASES: forward, grad-input and both weight-gradient forms, as the source test runs them."""
    ar, log = guarded
    ops = pcg.ops
    RAN["thin"].add(shape)
    B, Cin, Cout, H, W, k, s, p = shape
    kh, kw = TH._k2(k)
    x, w, b, bx, y, dy = TH._ref(shape, seed=B * 1009 + Cin * 31 + Cout * 7 + H)
    g = TH._geom(ops, shape)
    xd, wd, dyd = ar.input(_f32(TH.nhwc(x)), "x"), ar.input(_f32(TH.nhwc(w)), "w"), ar.input(_f32(TH.nhwc(dy)), "dy")
    bd, bxd = ar.input(_f32(b), "bias"), ar.input(_f32(bx), "bias_x")
    got_y = ops.conv2d_fwd(g, xd, wd, bd, out=ar.output((B, g.OH, g.OW, Cout), name="y"))
    got_dx = ops.conv2d_dgrad(g, dyd, wd, bxd, out=ar.output((B, H, W, Cin), name="dx"))
    dw = ar.output((Cout, kh, kw, Cin), name="dw")
    ops.conv2d_wgrad(g, xd, dyd, dw, accumulate=False)
    dw2 = ar.inout(dw, "dw (accumulate)")
    ops.conv2d_wgrad(g, xd, dyd, dw2, accumulate=True)
    _settle(ar)
    err = TH._err(got_y, TH.nhwc(y.detach()))
    assert err <= TH._tol(Cin * kh * kw, 4.0), f"fwd max err {err}"
    err = TH._err(got_dx, TH.nhwc(x.grad) + bx)
    assert err <= TH._tol(Cout * kh * kw, 4.0), f"dgrad max err {err}"
    ref, K = TH.nhwc(w.grad), B * g.OH * g.OW
    err = TH._err(dw, ref)
    assert err <= TH._tol(K, 8.0), f"wgrad max err {err}"
    err = TH._err(dw2, 2 * ref)
    assert err <= 2 * TH._tol(K, 8.0), f"wgrad accumulate max err {err}"


@pytest.mark.parametrize("act,slope", TH.ACTS[:2])
@pytest.mark.parametrize("shape", TH._params(TH.MASK_CASES))
def test_thin_grad_input_with_mask_in_guarded_buffers(pcg, guarded, shape, act, slope):
    """MASK_CASES: the launch conv_bwd_data_fused makes for a thin layer, with the arena's output (a_below is a separate allocation:
    the kernel reaches it as a byte distance from the output)."""
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    RAN["thin-mask"].add((shape, act))
    B, Cin, Cout, H, W, k, s, p = shape
    x, w, b, bx, y, dy = TH._ref(shape, seed=B * 13 + Cout + act)
    g = TH._geom(ops, shape)
    assert lib.pcg_conv2d_dgrad_mask_thin_ok(ctypes.byref(g)) == 1
    a_below = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(5))
    out = ar.output((B, H, W, Cin), name="dx")
    ops._conv2d_call(g, DGRAD, in_=ar.input(_f32(TH.nhwc(dy)), "dy"), w=ar.input(_f32(TH.nhwc(w)), "w"), out=out, epi="mask",
                     a_below=ar.input(a_below, "a_below"), epi_act=int(act), epi_slope=float(slope))
    _settle(ar)
    want = TH.nhwc(x.grad) * torch.where(a_below.double() > 0, 1.0, slope)
    err = TH._err(out, want)
    assert err <= TH._tol(Cout * k * k, 4.0), f"masked dgrad max err {err}"


@pytest.mark.parametrize("act,slope", TH.ACTS[:2])
@pytest.mark.parametrize("shape", TH._params(TH.BNBWD_CASES))
def test_thin_forward_through_batchnorm_backward_in_guarded_buffers(pcg, guarded, shape, act, slope):
    """BNBWD_CASES through thin_fwd_bn_bwd: exactly pcg_conv2d_fwd_bnbwd_thin_workspace_bytes of NaN scratch; dgamma / dbeta are inout
    (accumulate False overwrites what they hold, True adds to it).  Reference and bounds: the source test's float64 chain."""
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    RAN["thin-bnbwd"].add((shape, act))
    B, Cin, C, H, W, k, s, p = shape
    g = TH._geom(ops, shape)
    assert ops.thin_fwd_bn_bwd_ok(g)
    gen = torch.Generator().manual_seed(B * 3 + C)
    x = TH._randn(B, H, W, 1, g=gen)
    w = TH._randn(C, k, k, 1, g=gen, scale=0.25)
    z = TH._randn(B, g.OH, g.OW, C, g=gen, scale=1.3) + 0.25
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = TH._randn(C, g=gen, scale=0.1)
    zr = z.reshape(-1, C)
    mean = zr.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(zr.var(0, unbiased=False) + 1e-5)).float().double()
    d = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1).reshape(-1, C)
    sc = gamma * invstd
    pre = zr * sc + (beta - mean * sc)
    neg = slope if act == TH.ACT_LRELU else 0.0
    dm = d * torch.where(pre > 0, 1.0, neg)
    xh = (zr - mean) * invstd
    n = zr.shape[0]
    db_ref, dg_ref = dm.sum(0), (dm * xh).sum(0)
    dz_ref = sc * (dm - db_ref / n - xh * dg_ref / n)
    amb = pre.abs() < 1e-5
    slack_b = (d.abs() * amb).sum(0) * (1 - neg)
    slack_g = (d.abs() * xh.abs() * amb).sum(0) * (1 - neg)
    e_d = TH._tol(k * k, 4.0)
    tol_b = e_d * n ** 0.5 + TH._tol(n, 8.0) * float(dm.abs().max()) + slack_b
    tol_g = e_d * float(xh.abs().max()) * n ** 0.5 + TH._tol(n, 8.0) * float((dm * xh).abs().max()) + slack_g
    tol_z = sc * (e_d * (2 + xh.abs().max()) + (slack_b + xh.abs().max() * slack_g) / n)
    need = lib.pcg_conv2d_fwd_bnbwd_thin_workspace_bytes(ctypes.byref(g))
    assert need > 0
    args = [ar.input(_f32(t), nm) for t, nm in ((x, "x"), (w, "w"), (z, "z"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma"),
                                                (beta, "beta"))]
    for accumulate in (False, True):
        dg0, db0 = TH._randn(C, g=gen), TH._randn(C, g=gen)
        dgd, dbd = ar.inout(_f32(dg0), "dgamma"), ar.inout(_f32(db0), "dbeta")
        log.clear()
        dz = ops.thin_fwd_bn_bwd(g, *args, act, slope, dgd, dbd, accumulate)
        _settle(ar)
        assert [r.nbytes for r in log] == [need]
        assert bool(torch.isfinite(dz).all())
        base_g, base_b = (dg0, db0) if accumulate else (torch.zeros(C, dtype=torch.float64),) * 2
        diff_b = (dbd.cpu().double() - (base_b + db_ref)).abs()
        diff_g = (dgd.cpu().double() - (base_g + dg_ref)).abs()
        assert bool((diff_b <= tol_b + 1e-6).all()), f"dbeta max err {float(diff_b.max())} (accumulate={accumulate})"
        assert bool((diff_g <= tol_g + 1e-6).all()), f"dgamma max err {float(diff_g.max())} (accumulate={accumulate})"
        diff_z = (dz.cpu().double().reshape(-1, C) - dz_ref).abs()
        bad = ~amb & (diff_z > tol_z + 1e-6)
        assert not bool(bad.any()), f"dz max err {float((diff_z * ~amb).max())} (accumulate={accumulate})"


@pytest.mark.parametrize("B,groups,act,slope", FULL_BNBWD_CASES)
def test_full_window_grad_input_through_batchnorm_backward_in_guarded_buffers(pcg, guarded, B, groups, act, slope):
    """full_dgrad_bn_bwd on exactly pcg_conv2d_dgrad_bnbwd_full_workspace_bytes of NaN scratch, dgamma / dbeta inout (overwritten, then
    accumulated into).  Cases, reference (the unfused launches, group by group, here on exact scratch as well) and bounds:
    test_hip_ops.test_full_window_grad_input_through_batchnorm_backward."""
    ar, log = guarded
    RAN["full-bnbwd"].add((B, groups, act))
    ops, lib = pcg.ops, pcg.load()
    C, Bg = 512, B // groups
    g = ops.conv_geom(B, 4, 4, C, 1, 4, 4, 1, 0)
    assert ops.full_dgrad_bn_bwd_ok(g, groups)
    gen = torch.Generator().manual_seed(5 + B)
    z = ar.input(torch.randn(B, 4, 4, C, generator=gen) * 1.3 + 0.2, "z")
    w = ar.input(torch.randn(1, 4, 4, C, generator=gen) * 0.1, "w")
    dy = ar.input(torch.randn(B, 1, 1, 1, generator=gen), "dy")
    gamma, beta = ar.input(1 + 0.1 * torch.randn(C, generator=gen), "gamma"), ar.input(0.1 * torch.randn(C, generator=gen), "beta")
    zg = z.reshape(groups, Bg * 16, C)
    mean, invstd = ar.input(zg.mean(1), "mean"), ar.input(1.0 / torch.sqrt(zg.var(1, unbiased=False) + 1e-5), "invstd")
    dg_ref, db_ref = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ref = []
    for k in range(groups):
        gk = ops.conv_geom(Bg, 4, 4, C, 1, 4, 4, 1, 0)
        d = ops.conv2d_dgrad(gk, dy[k * Bg:(k + 1) * Bg].contiguous(), w)
        ref.append(ops.bn_act_bwd(d, z[k * Bg:(k + 1) * Bg].contiguous(), None, C, mean[k].contiguous(), invstd[k].contiguous(), gamma, act, slope,
                                  dg_ref, db_ref, k > 0, beta=beta))
    ref = torch.cat(ref)
    dg, db = ar.inout(torch.full((C,), 7.0), "dgamma"), ar.inout(torch.full((C,), -7.0), "dbeta")
    log.clear()
    out = ops.full_dgrad_bn_bwd(g, dy, w, z, mean, invstd, gamma, beta, act, slope, dg, db, False, groups=groups)
    dg1 = dg.clone()
    ops.full_dgrad_bn_bwd(g, dy, w, z, mean, invstd, gamma, beta, act, slope, dg, db, True, groups=groups)
    _settle(ar)
    assert [r.nbytes for r in log] == [lib.pcg_conv2d_dgrad_bnbwd_full_workspace_bytes(ctypes.byref(g), groups)] * 2
    assert bool(torch.isfinite(out).all())
    scale = ref.abs().max().item()
    assert (out - ref).abs().max().item() <= 2e-6 * scale
    np.testing.assert_allclose(dg1.cpu().numpy(), dg_ref.cpu().numpy(), rtol=2e-5, atol=2e-6 * dg_ref.abs().max().item())
    np.testing.assert_allclose(dg.cpu().numpy(), 2 * dg_ref.cpu().numpy(), rtol=2e-5, atol=4e-6 * dg_ref.abs().max().item())
    np.testing.assert_allclose(db.cpu().numpy(), 2 * db_ref.cpu().numpy(), rtol=2e-5, atol=4e-6 * db_ref.abs().max().item())


# ---- table-driven loaders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,IH,Cin,Cout,B,modes", PC.CASES, ids=PC.IDS)
def test_clipped_tiles_in_guarded_buffers(pcg, guarded, form, IH, Cin, Cout, B, modes):
    """test_hip_pad_clip.CASES with the switch off (0) and at every forced value of the case: the clip tables hold negative offsets
    and run-on entries, so these loaders are the likeliest to read before x[0] or past the last image."""
    ar, log = guarded
    ops = pcg.ops
    RAN["pad-clip"].add((form, IH, Cin, Cout, B))
    shape = _k4(B, Cin, Cout, IH)
    g = ops.conv_geom(B, IH, IH, Cin, Cout, 4, 4, 2, 1)
    x, w, dy, b, bx = IG._operands(shape, 1000 * IH + Cout + B + form)
    wd = ar.input(_f32(IG._nhwc(w)), "w")
    if form == PC.FWD:
        a, bias, oshape = ar.input(_f32(IG._nhwc(x)), "x"), ar.input(_f32(b), "bias"), (B, g.OH, g.OW, Cout)
        run = lambda name: ops.conv2d_fwd(g, a, wd, bias, out=ar.output(oshape, name=name))                     # noqa: E731
    else:
        a, bias, oshape = ar.input(_f32(IG._nhwc(dy)), "dy"), ar.input(_f32(bx), "bias_x"), (B, IH, IH, Cin)
        run = lambda name: ops.conv2d_dgrad(g, a, wd, bias, out=ar.output(oshape, name=name))                   # noqa: E731
    assert not PC._taken(ops, g, form, 0)
    with PC._switch(ops, 0):
        base = run("out (pad_clip 0)")
    outs = []
    for mode in modes:
        assert PC._taken(ops, g, form, mode), f"mode {mode}: the launch did not take the clipped path"
        with PC._switch(ops, mode):
            outs.append(run(f"out (pad_clip {mode})"))
    _settle(ar)
    want = IG._fwd64(x, w, 2, 1, b) if form == PC.FWD else IG._dgrad64(x.shape, w, dy, 2, 1, bx)
    bound = IG._tol(16 * (Cin if form == PC.FWD else Cout), 4.0)
    assert IG._err(base, want) <= bound
    for mode, got in zip(modes, outs):
        assert torch.equal(got, base), f"mode {mode}: clipped output differs from today's kernel"
        assert IG._err(got, want) <= bound


@pytest.mark.parametrize("IH,Cout,korder", CLIP_ITER_CASES)
def test_clipped_grad_input_tap_walk_in_guarded_buffers(pcg, guarded, IH, Cout, korder):
    """test_hip_dgrad_clip_iter's walk cases (both k-tile orders, the ragged last channel chunk at Cout 48), switch off and forced."""
    ar, log = guarded
    ops = pcg.ops
    RAN["dgrad-clip-iter"].add((IH, Cout, korder))
    B, CIN = DC.B, DC.CIN
    g = ops.conv_geom(B, IH, IH, CIN, Cout, 4, 4, 2, 1)
    wsrc, dysrc, bxsrc, want = DC._case(IH, Cout)
    wd, dyd, bxd = ar.input(wsrc, "w"), ar.input(dysrc, "dy"), ar.input(bxsrc, "bias_x")
    bound = IG._tol(16 * Cout, 4.0)
    with _tune(ops, korder=korder, pad_clip_dgrad=1):
        assert not PC._taken(ops, g, DGRAD, 0)
        with PC._switch(ops, 0):
            base = ops.conv2d_dgrad(g, dyd, wd, bxd, out=ar.output((B, IH, IH, CIN), name="dx (pad_clip 0)"))
        outs = []
        for mode in PC.ORDERS:
            assert PC._taken(ops, g, DGRAD, mode), f"mode {mode}: the launch did not take the clipped path"
            with PC._switch(ops, mode):
                outs.append(ops.conv2d_dgrad(g, dyd, wd, bxd, out=ar.output((B, IH, IH, CIN), name=f"dx (pad_clip {mode})")))
    _settle(ar)
    assert IG._err(base, want) <= bound
    for mode, got in zip(PC.ORDERS, outs):
        assert torch.equal(got, base), f"korder {korder} mode {mode}: clipped output differs from today's kernel"
        assert IG._err(got, want) <= bound


def _wgrad_both_forms(ar, ops, geom, xd, dyd, g0, tag):
    """accumulate=False into an output and accumulate=True into an inout holding g0: (dw, dw_accumulated)."""
    dw = ar.output(tuple(g0.shape), name=f"dw ({tag})")
    ops.conv2d_wgrad(geom, xd, dyd, dw, False)
    acc = ar.inout(g0, f"dw accumulate ({tag})")
    ops.conv2d_wgrad(geom, xd, dyd, acc, True)
    return dw, acc


def _check_wgrad_runs(runs, ref, g0, K):
    """Every (tag, dw, acc) bit-equal to the first and within test_hip_benchshape._bound of float64 (the source files' bound)."""
    _, dw0, acc0 = runs[0]
    for tag, dw, acc in runs:
        assert torch.equal(dw, dw0), f"{tag}: differs from {runs[0][0]}"
        assert torch.equal(acc, acc0), f"{tag}: accumulate differs from {runs[0][0]}"
    err = (dw0.cpu().double() - ref).abs().max().item()
    assert err <= BS._bound(K, 1.0), f"max err {err:.3e} > {BS._bound(K, 1.0):.3e}"
    err = (acc0.cpu().double() - (ref + g0.cpu().double())).abs().max().item()
    assert err <= BS._bound(K + 1, 1.0), f"accumulate max err {err:.3e}"


def _padskip_sweep(ar, ops, geom, xd, dyd, g0, tag, tabs=(1, 0), modes=(0, 2, 3, 1)):
    """One list of (tag, dw, acc) per pixel-table setting: the source file claims bit-equality across the switch within each."""
    groups = []
    for tab in tabs:
        runs = []
        for v in modes:
            with _tune(ops, wgrad_pixtab=tab, wgrad_padskip=v):
                t = f"{tag} pixtab {tab} padskip {v}"
                runs.append((t,) + _wgrad_both_forms(ar, ops, geom, xd, dyd, g0, t))
        groups.append(runs)
    return groups


@pytest.mark.parametrize("H,Cin,Cout,B", PADSKIP_DP_CASES)
def test_padskip_weight_gradient_in_guarded_buffers(pcg, guarded, H, Cin, Cout, B):
    """test_hip_wgrad_padskip.test_data_parallel_kernels' cases: switch 0 .. 3, with and without the pixel table, stream_k 0 and 2."""
    ar, log = guarded
    ops = pcg.ops
    RAN["wgrad-padskip"].add(("dp", H, Cin, Cout, B))
    x, dy, g0 = PS._inputs(B, Cin, Cout, H, seed=H + Cin + Cout + B)
    geom = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    assert ops.conv_wgrad_padskip_query(geom)[0]
    xd, dyd = ar.input(x, "x"), ar.input(dy, "dy")
    groups = []
    for sk in (0, 2):
        with _tune(ops, stream_k=sk):
            groups += _padskip_sweep(ar, ops, geom, xd, dyd, g0, f"stream_k {sk}")
    _settle(ar)
    ref = PS._ref64(x, dy)
    for runs in groups:
        _check_wgrad_runs(runs, ref, g0, B * (H // 2) ** 2)


@pytest.mark.parametrize("H,B", PADSKIP_SK_CASES)
def test_padskip_stream_k_weight_gradient_in_guarded_buffers(pcg, guarded, H, B):
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    RAN["wgrad-padskip"].add(("sk", H, B))
    Cin, Cout = 448, 160
    x, dy, g0 = PS._inputs(B, Cin, Cout, H, seed=H)
    geom = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    desc = ctypes.create_string_buffer(256)
    xd, dyd = ar.input(x, "x"), ar.input(dy, "dy")
    with _tune(ops, stream_k=2, sk_blocks=512):
        ops._conv_scratch()
        assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
        assert desc.value.decode().startswith("stream-K") and "over 512 ranges" in desc.value.decode(), desc.value
        runs = _padskip_sweep(ar, ops, geom, xd, dyd, g0, "stream-K")
        _settle(ar)
        _arrivals_are_zero(ops)
    with _tune(ops, stream_k=0):                # the same gradient as 112 tiles x K-slices (slabs)
        assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
        assert desc.value.decode().startswith("128x128 tiles"), desc.value
        log.clear()
        slabs = _padskip_sweep(ar, ops, geom, xd, dyd, g0, "slabs", tabs=(1,))
        _settle(ar)
        assert log and all(r.changed for r in log)
    K = B * (H // 2) ** 2
    ref = PS._ref64(x, dy)
    for group in runs + slabs:
        _check_wgrad_runs(group, ref, g0, K)


@pytest.mark.parametrize("H,B,Cin,Cout", PADSKIP_PAIRED_CASES)
def test_padskip_paired_block_order_in_guarded_buffers(pcg, guarded, H, B, Cin, Cout):
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    RAN["wgrad-padskip"].add(("paired", H, B, Cin, Cout))
    x, dy, g0 = PS._inputs(B, Cin, Cout, H, seed=3)
    geom = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    desc = ctypes.create_string_buffer(256)
    assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
    tiles = (Cout // 128) * (16 * Cin // 128)
    assert desc.value.decode().startswith(f"128x128 tiles: {tiles} x {512 // tiles} K-slices"), desc.value
    (runs,) = _padskip_sweep(ar, ops, geom, ar.input(x, "x"), ar.input(dy, "dy"), g0, "paired", tabs=(1,))
    _settle(ar)
    assert log and all(r.changed for r in log)
    _check_wgrad_runs(runs, PS._ref64(x, dy), g0, B * (H // 2) ** 2)


@pytest.mark.parametrize("name,B,Cin,Cout,H,k,s,p", PIXTAB_CASES, ids=[c[0] for c in PIXTAB_CASES])
def test_pixel_table_weight_gradient_in_guarded_buffers(pcg, guarded, name, B, Cin, Cout, H, k, s, p):
    """test_hip_wgrad_pixtab.CASES and its stream-K case with the table loader off and on: the table's tail entries run on past the
    last image (up to 7 image strides at OH*OW = 1)."""
    ar, log = guarded
    ops, lib = pcg.ops, pcg.load()
    RAN["wgrad-pixtab"].add(name)
    sk = name == PT.SK_CASE[0]
    x, dy, g0, OH = PT._inputs(B, Cin, Cout, H, k, s, p, seed=5 if sk else len(name))
    geom = ops.conv_geom(B, H, H, Cin, Cout, k, k, s, p)
    xd, dyd = ar.input(x, "x"), ar.input(dy, "dy")
    runs = []
    with _tune(ops, **({"stream_k": 2} if sk else {})):
        if sk:
            ops._conv_scratch()
            desc = ctypes.create_string_buffer(256)
            assert lib.pcg_conv_plan_describe(ctypes.byref(geom), 2, 0, desc, 256) == 0
            assert desc.value.decode().startswith("stream-K"), desc.value
        for v in (0, 1):
            with _tune(ops, wgrad_pixtab=v):
                runs.append((f"pixtab {v}",) + _wgrad_both_forms(ar, ops, geom, xd, dyd, g0, f"pixtab {v}"))
        _settle(ar)
        if sk:
            _arrivals_are_zero(ops)
    assert PT._registered(ops, geom)
    _check_wgrad_runs(runs, PT._ref64(x, dy, k, s, p), g0, B * OH * OH)


# ---- epilogues, statistics, transforms and groups ---------------------------------------------------------------------------
def _bn_queries(lib, g, dgrad):
    """(exact bytes of the partial rows / statistics workspace, number of partial rows) of the fused BatchNorm forms of this side."""
    if dgrad:
        return lib.pcg_conv2d_dgrad_bn_workspace_bytes(ctypes.byref(g)), lib.pcg_conv2d_dgrad_bn_partial_rows(ctypes.byref(g))
    return lib.pcg_conv2d_fwd_bn_workspace_bytes(ctypes.byref(g)), lib.pcg_conv2d_fwd_bn_partial_rows(ctypes.byref(g))


@pytest.mark.parametrize("form,dgrad", IG.EPI_SIDES)
def test_epilogues_and_statistics_in_guarded_buffers(pcg, guarded, form, dgrad):
    """Every side of EPI_FORMS through ops._conv2d_call with the arena's out, partial (exactly pcg_conv2d_{fwd,dgrad}_bn_workspace_bytes,
    NaN before the launch) and workspace: mask, add (into a new tensor and in place), add_mask, add_bnsum with and without an addend,
    bnbwd, and the fused statistics.  The aux tensors are separate allocations, so the byte distances the kernels reach them by are
    large and of either sign.  The sums are consumed by bn_bwd_partial on exact scratch, as in the source tests."""
    ar, log = guarded
    RAN["epilogue"].add((form[0], dgrad))
    e = IG._Epi(pcg, form, 909)
    ops, lib, g = e.ops, e.lib, e.g
    act, slope, scale = IG.ACT_LRELU, 0.2, 0.1
    op = DGRAD if dgrad else FWD
    oshape = e.out_shape(dgrad)
    C = oshape[3]
    d, wd = ar.input(e.dyd if dgrad else e.xd, "in"), ar.input(e.wd, "w")
    bias64 = e.bx if dgrad else e.b
    a_below, addend = e.rand(dgrad), e.rand(dgrad)
    ad, add_d = ar.input(_f32(a_below), "a_below"), ar.input(_f32(addend), "addend")
    z, mean, invstd, gamma, beta = IG._stats(e, C, dgrad, 7)
    zd, md, isd, gd, bd = (ar.input(_f32(t), n) for t, n in ((z, "z"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (beta, "beta")))
    need, nparts = _bn_queries(lib, g, dgrad)
    assert need > 0 and nparts > 0
    dg0, db0 = IG._randn(C, g=e.gen), IG._randn(C, g=e.gen)
    rm0, rv0 = IG._randn(C, g=e.gen, scale=0.1), torch.rand(C, generator=e.gen, dtype=torch.float64).float().double() + 0.5

    def call(name, out=None, **kw):
        out = ar.output(oshape, name=name) if out is None else out
        ops._conv2d_call(g, op, in_=d, w=wd, out=out, **kw)
        return out

    with IG._tuned(lib, e.tune):
        e.check_plan(dgrad)
        o_mask = call("out (mask)", epi="mask", a_below=ad, epi_act=act, epi_slope=slope)
        o_add = call("out (add)", epi="add", addend=add_d)
        o_inplace = ar.inout(add_d, "out = addend (add in place)")
        call(None, out=o_inplace, epi="add", addend=o_inplace)
        o_add_mask = call("out (add_mask)", epi="add_mask", addend=add_d, a_below=ad, epi_act=act, epi_slope=slope)
        sums = []
        for with_addend in (True, False):
            partial = ar.scratch(need, name=f"partial rows (add_bnsum, addend {with_addend})")
            o = call(f"out (add_bnsum, addend {with_addend})", epi="add_bnsum", addend=add_d if with_addend else None, z=zd, mean=md, invstd=isd,
                     sum_scale=scale, partial=partial, partial_bytes=need)
            dgd, dbd = ar.inout(_f32(dg0), "dgamma"), ar.inout(_f32(db0), "dbeta")
            dz = ops.bn_bwd_partial(o, zd, C, md, isd, gd, partial, nparts, dgd, dbd, True, out=ar.output(oshape, name="dz (add_bnsum)"),
                                    dm_scale=scale)
            sums.append((with_addend, o, dz, dgd, dbd))
        partial = ar.scratch(need, name="partial rows (bnbwd)")
        o_bnbwd = call("out (bnbwd)", epi="bnbwd", z=zd, mean=md, invstd=isd, gamma=gd, beta=bd, epi_act=act, epi_slope=slope, partial=partial,
                       partial_bytes=need)
        dg_b, db_b = ar.output((C,), name="dgamma (bnbwd)"), ar.output((C,), name="dbeta (bnbwd)")
        dz_b = ops.bn_bwd_partial(o_bnbwd, zd, C, md, isd, gd, partial, nparts, dg_b, db_b, False, out=ar.output(oshape, name="dz (bnbwd)"))
        # fused statistics
        ws = ar.scratch(need, name="statistics workspace")
        s_mean, s_invstd, coef = ar.output((C,), name="save_mean"), ar.output((C,), name="save_invstd"), ar.output((2 * C,), name="coef")
        rm, rv = ar.inout(_f32(rm0), "running_mean"), ar.inout(_f32(rv0), "running_var")
        nbt = ar.inout(torch.full((1,), 3, dtype=torch.int64), "num_batches_tracked")
        g2, b2 = IG._randn(C, g=e.gen) + 1.0, IG._randn(C, g=e.gen, scale=0.1)
        o_stats = call("z (statistics)", bias=ar.input(_f32(bias64), "bias"), stats=1, eps=1e-5, momentum=0.1, save_mean=s_mean, save_invstd=s_invstd,
                       running_mean=rm, running_var=rv, num_batches_tracked=nbt, gamma=ar.input(_f32(g2), "gamma (fold)"),
                       beta=ar.input(_f32(b2), "beta (fold)"), coef_out=coef, workspace=ws, workspace_bytes=need)
    _settle(ar)
    if "stream-K" in e.want[dgrad]:
        _arrivals_are_zero(ops)

    conv, tol = e.conv64(dgrad), e.tol(dgrad)
    m = torch.where(a_below > 0, 1.0, slope)
    for name, got, want in (("mask", o_mask, conv * m), ("add", o_add, conv + addend), ("add in place", o_inplace, conv + addend),
                            ("add_mask", o_add_mask, (conv + addend) * m)):
        err = IG._err(got, want)
        assert err <= tol, f"{name} max err {err:.3e}"
    for with_addend, o, dz, dgd, dbd in sums:
        err = IG._err(o, conv + (addend if with_addend else 0.0))
        assert err <= tol, f"add_bnsum (addend {with_addend}) output max err {err:.3e}"
        IG._check_bn_bwd(dz, dgd - dg0.float().to(DEV), dbd - db0.float().to(DEV),
                         IG._bn_bwd64(scale * o.cpu().double(), z, mean, invstd, gamma))
    sc, sh = IG._fold32(mean, invstd, gamma, beta)
    pre = IG._pre32(z, sc, sh)
    near = pre.abs() <= 1e-6
    assert int(near.sum()) <= max(4, 1e-4 * near.numel()), f"{int(near.sum())} elements at the kink"
    dd = (o_bnbwd.cpu().double() - conv * torch.where(pre > 0, 1.0, slope)).abs()
    assert float(dd[~near].max()) <= tol, f"bnbwd masked output max err {float(dd[~near].max()):.3e}"
    IG._check_bn_bwd(dz_b, dg_b, db_b, IG._bn_bwd64(o_bnbwd.cpu().double(), z, mean, invstd, gamma))
    # statistics: test_conv_bn_statistics_against_float64's bounds
    err = IG._err(o_stats, e.conv64(dgrad, bias=True))
    assert err <= tol, f"z max err {err:.3e}"
    zz = o_stats.cpu().double().reshape(-1, C)
    m64, v64, n = zz.mean(0), zz.var(0, unbiased=False), zz.shape[0]
    torch.testing.assert_close(s_mean.cpu().double(), m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s_invstd.cpu().double(), 1.0 / torch.sqrt(v64 + 1e-5), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rm.cpu().double(), 0.9 * rm0 + 0.1 * m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.cpu().double(), 0.9 * rv0 + 0.1 * v64 * n / (n - 1), rtol=1e-5, atol=1e-6)
    assert int(nbt.item()) == 4
    scf = g2 * s_invstd.cpu().double()
    torch.testing.assert_close(coef.cpu().double()[:C], scf, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(coef.cpu().double()[C:], b2 - s_mean.cpu().double() * scf, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("form", IG.XF_FORMS)
def test_input_transform_in_guarded_buffers(pcg, guarded, form):
    """XF_FORMS: forward with x = act(z * sc + sh), grad-input with dy transformed, both weight-gradient sides (accumulate into an inout)."""
    ar, log = guarded
    RAN["xform"].add(form[0])
    act, slope = IG.ACT_LRELU, 0.2
    e = IG._Epi(pcg, form, 606 + act)
    ops = e.ops
    B, Cin, Cout, H, W, KH, KW, s, p = e.shape

    def xform(C, like_dgrad_out, name):
        z = e.rand(like_dgrad_out, scale=1.3, shift=0.2)
        sc = (torch.rand(C, generator=e.gen, dtype=torch.float64) + 0.5).float().double()
        sh = IG._randn(C, g=e.gen, scale=0.3)
        a = IG._pre32(z, sc, sh)
        a = torch.where(a > 0, a, (a * slope).float().double())
        return ar.input(_f32(z), f"z ({name})"), a, ops.InputXform(ar.input(_f32(torch.cat([sc, sh])), f"coef ({name})"), act, slope)

    zx, ax, xfx = xform(Cin, True, "x side")
    zy, ay, xfy = xform(Cout, False, "dy side")
    a_x, a_y = IG._nchw(ax), IG._nchw(ay)
    xd, dyd, wd = ar.input(e.xd, "x"), ar.input(e.dyd, "dy"), ar.input(e.wd, "w")
    wshape = (Cout, KH, KW, Cin)
    with IG._tuned(e.lib, e.tune):
        for dgrad in (False, True):
            if e.want[dgrad] is not None:
                e.check_plan(dgrad)
        got_f = ops.conv2d_fwd(e.g, zx, wd, ar.input(e.bd, "bias"), out=ar.output(e.out_shape(False), name="y"), xf=xfx)
        got_d = ops.conv2d_dgrad(e.g, zy, wd, ar.input(e.bxd, "bias_x"), out=ar.output(e.out_shape(True), name="dx"), xf=xfy)
        dw_x = ops.conv2d_wgrad(e.g, zx, dyd, ar.output(wshape, name="dw (xf_x)"), False, xf_x=xfx)
        dw_y = ops.conv2d_wgrad(e.g, xd, zy, ar.output(wshape, name="dw (xf_dy)"), False, xf_dy=xfy)
        dw_y2 = ops.conv2d_wgrad(e.g, xd, zy, ar.inout(dw_y, "dw (xf_dy, accumulate)"), True, xf_dy=xfy)
    _settle(ar)
    err = IG._err(got_f, IG._fwd64(a_x, e.w, s, p, e.b))
    assert err <= e.tol(False), f"fwd xf max err {err:.3e}"
    err = IG._err(got_d, IG._dgrad64(e.x.shape, e.w, a_y, s, p, e.bx))
    assert err <= e.tol(True), f"dgrad xf max err {err:.3e}"
    K = B * e.g.OH * e.g.OW
    err = IG._err(dw_x, IG._wgrad64(a_x, e.w.shape, e.dy, s, p))
    assert err <= IG._tol(K, 8.0), f"wgrad xf_x max err {err:.3e}"
    ref = IG._wgrad64(e.x, e.w.shape, a_y, s, p)
    err = IG._err(dw_y, ref)
    assert err <= IG._tol(K, 8.0), f"wgrad xf_dy max err {err:.3e}"
    err = IG._err(dw_y2, 2 * ref)
    assert err <= 2 * IG._tol(K, 8.0), f"wgrad xf_dy accumulate max err {err:.3e}"


@pytest.mark.parametrize("B,Cin,Cout,H,groups", IG.GROUPED_FWD)
def test_grouped_conv_bn_in_guarded_buffers(pcg, guarded, B, Cin, Cout, H, groups):
    """GROUPED_FWD: conv_bn_train_g's launch with the arena's z, statistics [groups, C], running statistics (inout) and exactly
    pcg_conv2d_fwd_bn_workspace_bytes of workspace."""
    ar, log = guarded
    RAN["grouped-fwd"].add((B, Cin, Cout, H, groups))
    ops, lib = pcg.ops, pcg.load()
    shape = (B, Cin, Cout, H, H, 4, 4, 2, 1)
    g = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    assert ops.group_fwd_ok(g, groups)
    x, w, _, b, _ = IG._operands(shape, 700 + B + groups)
    per = B // groups
    x = torch.cat([x[k * per:(k + 1) * per] * (1 + 0.5 * k) + 0.2 * k for k in range(groups)]).float().double()
    rm0 = IG._randn(Cout, g=torch.Generator().manual_seed(1), scale=0.1)
    rv0 = rm0.abs() + 0.75
    rm, rv = ar.inout(_f32(rm0), "running_mean"), ar.inout(_f32(rv0), "running_var")
    nbt = ar.inout(torch.zeros(1, dtype=torch.int64), "num_batches_tracked")
    need = lib.pcg_conv2d_fwd_bn_workspace_bytes(ctypes.byref(g))
    z = ar.output((B, g.OH, g.OW, Cout), name="z")
    mean, invstd = ar.output((groups, Cout), name="save_mean"), ar.output((groups, Cout), name="save_invstd")
    ops._conv2d_call(g, FWD, in_=ar.input(_f32(IG._nhwc(x)), "x"), w=ar.input(_f32(IG._nhwc(w)), "w"), bias=ar.input(_f32(b), "bias"), out=z, stats=1,
                     eps=1e-5, momentum=0.1, save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv, num_batches_tracked=nbt,
                     groups=int(groups), workspace=ar.scratch(need, name="statistics workspace"), workspace_bytes=need)
    _settle(ar)
    err = IG._err(z, IG._fwd64(x, w, 2, 1, b))
    assert err <= IG._tol(16 * Cin, 4.0), f"z max err {err:.3e}"
    zz = z.cpu().double()
    rm_want, rv_want = rm0.clone(), rv0.clone()
    for k in range(groups):
        zk = zz[k * per:(k + 1) * per].reshape(-1, Cout)
        m64, v64, n = zk.mean(0), zk.var(0, unbiased=False), zk.shape[0]
        torch.testing.assert_close(mean[k].cpu().double(), m64, rtol=1e-5, atol=1e-6, msg=f"group {k} mean")
        torch.testing.assert_close(invstd[k].cpu().double(), 1.0 / torch.sqrt(v64 + 1e-5), rtol=1e-5, atol=1e-6, msg=f"group {k} invstd")
        rm_want = 0.9 * rm_want + 0.1 * m64
        rv_want = 0.9 * rv_want + 0.1 * v64 * n / (n - 1)
    torch.testing.assert_close(rm.cpu().double(), rm_want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.cpu().double(), rv_want, rtol=1e-5, atol=1e-6)
    assert int(nbt.item()) == groups


@pytest.mark.parametrize("B,Cin,Cout,H,groups", IG.GROUPED_DGRAD)
def test_grouped_bnbwd_in_guarded_buffers(pcg, guarded, B, Cin, Cout, H, groups):
    """GROUPED_DGRAD: the grouped bnbwd grad-input with the arena's output and partial rows, consumed by bn_bwd_partial_g on exact
    scratch with dgamma / dbeta in the arena."""
    ar, log = guarded
    RAN["grouped-dgrad"].add((B, Cin, Cout, H, groups))
    ops, lib = pcg.ops, pcg.load()
    act, slope = IG.ACT_LRELU, 0.2
    shape = (B, Cin, Cout, H, H, 4, 4, 2, 1)
    g = ops.conv_geom(B, H, H, Cin, Cout, 4, 4, 2, 1)
    assert ops.group_dgrad_ok(g, groups)
    x, w, dy, _, _ = IG._operands(shape, 800 + B + groups)
    gen = torch.Generator().manual_seed(B + groups)
    per = B // groups
    z = torch.cat([IG._randn(per, H, H, Cin, g=gen, scale=1.0 + 0.4 * k) + 0.3 * (k - 1) for k in range(groups)])
    mean = torch.stack([z[k * per:(k + 1) * per].reshape(-1, Cin).mean(0) for k in range(groups)]).float().double()
    invstd = torch.stack([1.0 / torch.sqrt(z[k * per:(k + 1) * per].reshape(-1, Cin).var(0, unbiased=False) + 1e-5)
                          for k in range(groups)]).float().double()
    gamma = (torch.rand(Cin, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = IG._randn(Cin, g=gen, scale=0.1)
    zd, md, isd, gd, bd = (ar.input(_f32(t), n) for t, n in ((z, "z"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (beta, "beta")))
    need = lib.pcg_conv2d_dgrad_bn_workspace_bytes(ctypes.byref(g))
    nparts, nph = lib.pcg_conv2d_dgrad_bn_partial_rows(ctypes.byref(g)), lib.pcg_conv2d_dgrad_bn_phases(ctypes.byref(g))
    partial = ar.scratch(need, name="partial rows")
    dm = ar.output((B, H, H, Cin), name="dm")
    ops._conv2d_call(g, DGRAD, in_=ar.input(_f32(IG._nhwc(dy)), "dy"), w=ar.input(_f32(IG._nhwc(w)), "w"), out=dm, epi="bnbwd", z=zd, mean=md,
                     invstd=isd, gamma=gd, beta=bd, epi_act=act, epi_slope=slope, partial=partial, partial_bytes=need, groups=int(groups))
    dgd, dbd = ar.output((Cin,), name="dgamma"), ar.output((Cin,), name="dbeta")
    dz = ops.bn_bwd_partial_g(dm, zd, Cin, md, isd, gd, partial, nparts, nph, dgd, dbd, False, groups, out=ar.output((B, H, H, Cin), name="dz"))
    # the unfused grouped form on the same statistics: bn_act_bwd_g against the ungrouped premask call per group (test_hip_groups.py)
    dd = ar.input(torch.randn(B, H, H, Cin, generator=gen), "d")
    dg_u, db_u = ar.output((Cin,), name="dgamma (bn_act_bwd_g)"), ar.output((Cin,), name="dbeta (bn_act_bwd_g)")
    dz_u = ops.bn_act_bwd_g(dd, zd, Cin, md, isd, gd, bd, act, slope, dg_u, db_u, False, groups, out=ar.output((B, H, H, Cin), name="dz (bn_act_bwd_g)"))
    _settle(ar)
    assert [r.nbytes for r in log] == [lib.pcg_bn_bwd_partial_g_workspace_bytes(Cin, int(groups)),
                                       lib.pcg_bn_act_bwd_g_workspace_bytes(B * H * H, Cin, int(groups))]
    dg_r, db_r = torch.zeros(Cin, device=DEV), torch.zeros(Cin, device=DEV)
    for k in range(groups):
        sl = slice(k * per, (k + 1) * per)
        want = ops.bn_act_bwd(dd[sl].contiguous(), zd[sl].contiguous(), None, Cin, md[k].contiguous(), isd[k].contiguous(), gd, act, slope, dg_r, db_r,
                              k > 0, beta=bd)
        assert TG._rel_l2(dz_u[sl], want) <= 1e-6, f"group {k}: unfused grouped BatchNorm backward differs"
    assert TG._rel_l2(dg_u, dg_r) <= 1e-6 and TG._rel_l2(db_u, db_r) <= 1e-6
    conv = IG._dgrad64(x.shape, w, dy, 2, 1)
    dm64 = dm.cpu().double()
    dg_want, db_want = torch.zeros(Cin, dtype=torch.float64), torch.zeros(Cin, dtype=torch.float64)
    for k in range(groups):
        sl = slice(k * per, (k + 1) * per)
        sc, sh = IG._fold32(mean[k], invstd[k], gamma, beta)
        pre = IG._pre32(z[sl], sc, sh)
        near = pre.abs() <= 1e-6
        assert int(near.sum()) <= max(4, 1e-4 * near.numel()), f"group {k}: {int(near.sum())} elements at the kink"
        d = (dm64[sl] - conv[sl] * torch.where(pre > 0, 1.0, slope)).abs()
        assert float(d[~near].max()) <= IG._tol(16 * Cout, 4.0), f"group {k}: masked output max err {float(d[~near].max()):.3e}"
        dz_k, dg_k, db_k = IG._bn_bwd64(dm64[sl], z[sl], mean[k], invstd[k], gamma)
        IG._check_dz(dz[sl], dz_k)
        dg_want += dg_k
        db_want += db_k
    IG._check_sums(dgd, dbd, dg_want, db_want)


# ---- the other users of the shared scratch -------------------------------------------------------------------------------------
def _aligned_route(op, args, want, mis):
    """The source case's route; a case the source runs misaligned sits at 16 bytes here, so its float4 twin is what runs (not pinned)."""
    if mis:
        assert NB.plan(op, *args) != want
    else:
        NB.assert_route(op, args, want)


@pytest.mark.parametrize("case", NB.BN_CASES, ids=NB._bn_id)
def test_bn_statistics_and_colsum_on_exact_scratch(pcg, guarded, case):
    """bn_train_stats and colsum on every column-reduce plan of BN_CASES: x guarded, the running statistics and db inout, exactly
    pcg_bn_workspace_bytes / pcg_colsum_workspace_bytes of NaN scratch.  test_hip_norm_branches.test_bn_train_stats' bounds."""
    ar, log = guarded
    RAN["bn-stats"].add(case[:2])
    rows, C, mis, cols, _, _ = case
    ops, lib = pcg.ops, pcg.load()
    _aligned_route("BN_COLREDUCE", (rows, C, 1), cols, mis)
    d = NB.bn_inputs(rows, C)
    st = d["stats"]
    xd = ar.input(_f32(d["x"]), "x")
    rm, rv = ar.inout(_f32(d["rm0"]), "running_mean"), ar.inout(_f32(d["rv0"]), "running_var")
    nbt = ar.inout(torch.full((1,), 41, dtype=torch.int64), "num_batches_tracked")
    mean, invstd, coef = ops.bn_train_stats(xd, C, NB.EPS, NB.MOM, rm, rv, nbt, gamma=ar.input(_f32(d["gamma"]), "gamma"),
                                            beta=ar.input(_f32(d["beta"]), "beta"))
    assert [(r.kind, r.nbytes) for r in log] == [(0, lib.pcg_bn_workspace_bytes(rows, C))]
    dyd = ar.input(_f32(d["dy"]), "dy")
    dbs = []
    for acc in (False, True):
        db = ar.inout(torch.full((C,), 0.5), f"db (accumulate {acc})")
        ops.colsum(rows, C, dyd, db, acc)
        dbs.append(db)
    assert [r.nbytes for r in log[1:]] == [lib.pcg_colsum_workspace_bytes(rows, C)] * 2
    _settle(ar)
    for t in (mean, invstd, coef):
        assert bool(torch.isfinite(t).all())
    NB._one_ulp(mean, st["mean"], f"save_mean {rows}x{C}")
    NB._one_ulp(invstd, st["invstd"], f"save_invstd {rows}x{C}")
    NB._within(rm, st["rm"], st["rm_bound"], "running_mean")
    NB._within(rv, st["rv"], st["rv_bound"], "running_var")
    assert int(nbt) == 42
    m32, i32 = mean.double().cpu(), invstd.double().cpu()
    sc = d["gamma"] * i32
    NB._within(coef[:C], sc, NB.U * sc.abs(), "coef scale")
    NB._within(coef[C:], d["beta"] - m32 * sc, NB.U * (2 * (m32 * sc).abs() + d["beta"].abs()), "coef shift")
    ssum = d["dy"].sum(0)
    for acc, db in zip((False, True), dbs):
        want = ssum + 0.5 if acc else ssum
        NB._within(db, want, NB.U * ssum.abs() + (NB.U * want.abs() if acc else 0.0), f"colsum {rows}x{C} acc={acc}")


BN_BWD_ARENA_FORMS = [f for f in NB.BN_BWD_FORMS if f[:2] in (("y", NB.ACT_LRELU), ("premask", NB.ACT_RELU))][:2]      # without / with dcol


@pytest.mark.parametrize("case", NB.BN_CASES, ids=NB._bn_id)
def test_bn_act_bwd_on_exact_scratch(pcg, guarded, case):
    """bn_act_bwd without dcol (mask from y) and with it (premask, accumulating) on every plan of BN_CASES: dx an output, dgamma /
    dbeta / dcol inout.  Reference and bounds: test_hip_norm_branches._run_bn_bwd's."""
    ar, log = guarded
    RAN["bn-bwd"].add(case[:2])
    rows, C, mis, cols, _, route = case
    ops, lib = pcg.ops, pcg.load()
    _aligned_route("BN_COLREDUCE", (rows, C, 1), cols, mis)
    _aligned_route("BN_APPLY", (2, rows, C, 1), route, mis)
    assert len(BN_BWD_ARENA_FORMS) == 2 and BN_BWD_ARENA_FORMS[0][4] is None and BN_BWD_ARENA_FORMS[1][4] is not None
    d = NB.bn_inputs(rows, C)
    xd, dyd = ar.input(_f32(d["x"]), "x"), ar.input(_f32(d["dy"]), "dy")
    md, isd, gd, bd = (ar.input(_f32(d[k]), k) for k in ("mean32", "invstd32", "gamma", "beta"))
    done = []
    for form in BN_BWD_ARENA_FORMS:
        src, act, dy_scale, acc, col = form
        pre = NB.bn_pre(d, act)
        ok, n_bad = NB.R.mask_gap_ok(pre["pre"], pre["pre_bound"])
        assert ok, f"{n_bad} pre-activations of the reference lie within 8 bounds of zero"
        yd = ar.input(ops.bn_apply_act(xd, C, md, isd, gd, bd, act, NB.SLOPE), "y") if src == "y" else None
        dx = ar.output((rows, C), name=f"dx {form}")
        dg, db = ar.inout(torch.full((C,), 0.25), "dgamma"), ar.inout(torch.full((C,), -0.5), "dbeta")
        dcol = ar.inout(torch.full((C,), 0.125), "dcol") if col is not None else None
        log.clear()
        ops.bn_act_bwd(dyd, xd, yd, C, md, isd, gd, act, NB.SLOPE, dg, db, acc, out=dx, dy_scale=dy_scale, beta=bd if src == "premask" else None,
                       dcol=dcol, accumulate_col=bool(col))
        want = lib.pcg_bn_db_workspace_bytes(rows, C) if col is not None else lib.pcg_bn_workspace_bytes(rows, C)
        assert [r.nbytes for r in log] == [want]
        done.append((form, dx, dg, db, dcol))
    _settle(ar)
    for form, dx, dg, db, dcol in done:
        src, act, dy_scale, acc, col = form
        pre = NB.bn_pre(d, act)
        ref = NB.R.bn_bwd(d["dy"], d["x"], d["mean32"], d["invstd32"], d["gamma"], pre["pre"], act, NB.SLOPE, dy_scale)
        tag = f"bn_act_bwd {rows}x{C} {form}"
        NB._within(dx, ref["dx"], ref["dx_bound"], tag + " dx")
        for name, got, old in (("dgamma", dg, 0.25), ("dbeta", db, -0.5)):
            want, bound = NB.R.accumulated(ref[name], ref[name + "_bound"], old) if acc else (ref[name], ref[name + "_bound"])
            NB._within(got, want, bound, f"{tag} {name}")
        if col is not None:
            want, bound = NB.R.accumulated(ref["dcol"], ref["dcol_bound"], 0.125) if col else (ref["dcol"], ref["dcol_bound"])
            NB._within(dcol, want, bound, tag + " dcol")


BN_PARTIAL_ARENA_CASES = [(rows, C, nparts) for rows, C in NB.BN_PARTIAL_SHAPES for nparts in sorted(NB.BN_PARTIAL_NPARTS)]


@pytest.mark.parametrize("rows,C,nparts", BN_PARTIAL_ARENA_CASES)
def test_bn_bwd_partial_on_exact_scratch(pcg, guarded, rows, C, nparts):
    """bn_bwd_partial (dm_scale 1, no dcol) and bn_bwd_partial_db (dm_scale 0.5 with dcol) on every finalize plan, from synthesised
    partial rows in a guarded buffer of exactly the size the conv workspace queries give it.  Source: test_bn_bwd_partial."""
    ar, log = guarded
    RAN["bn-partial"].add((rows, C, nparts))
    ops, lib = pcg.ops, pcg.load()
    NB.assert_route("BN_FINALIZE", (nparts,), NB.BN_PARTIAL_NPARTS[nparts])
    gen = NB._gen(nparts + C)
    d = NB.bn_inputs(1000, C)
    x, mean, invstd, gamma = d["x"][:rows], d["mean32"], d["invstd32"], d["gamma"]
    dm = NB.R.f32_exact(torch.randn(rows, C, generator=gen, dtype=torch.float64))
    xd, dmd = ar.input(_f32(x), "x"), ar.input(_f32(dm), "dm")
    md, isd, gd = ar.input(_f32(mean), "mean"), ar.input(_f32(invstd), "invstd"), ar.input(_f32(gamma), "gamma")
    done = []
    for dm_scale, with_col in ((1.0, False), (0.5, True)):
        ref = NB.R.bn_bwd(dm, x, mean, invstd, gamma, None, NB.ACT_NONE, 0.0, dm_scale)
        sums = torch.stack([ref["dbeta"], ref["dgamma"]])
        part = torch.randn(nparts, 2, C, generator=gen, dtype=torch.float64) * sums.abs().clamp_min(1e-3)
        part[-1] = sums - part[:-1].sum(0)
        fin_err = nparts * 2.0 ** -52 * part.abs().sum(0)
        host = torch.full((NB.bn_partial_buffer_doubles(nparts, C),), float(NB.SENT), dtype=torch.float64)
        host[:part.numel()] = part.reshape(-1)
        buf = ar.inout(host, f"partial rows (scale {dm_scale})")
        dx = ar.output((rows, C), name=f"dx (scale {dm_scale})")
        dg, db = ar.inout(torch.full((C,), 0.25), "dgamma"), ar.inout(torch.full((C,), -0.5), "dbeta")
        dcol = ar.inout(torch.full((C,), 0.125), "dcol") if with_col else None
        log.clear()
        ops.bn_bwd_partial(dmd, xd, C, md, isd, gd, buf, nparts, dg, db, True, out=dx, dcol=dcol, accumulate_col=True, dm_scale=dm_scale)
        assert [r.nbytes for r in log] == [(lib.pcg_bn_bwd_partial_db_workspace_bytes if with_col else lib.pcg_bn_bwd_partial_workspace_bytes)(C)]
        done.append((dm_scale, with_col, ref, sums, part, fin_err, buf, dx, dg, db, dcol))
    _settle(ar)
    for dm_scale, with_col, ref, sums, part, fin_err, buf, dx, dg, db, dcol in done:
        tag = f"bn_bwd_partial {rows}x{C} nparts={nparts} scale={dm_scale} dcol={with_col}"
        assert torch.equal(buf[:part.numel()].cpu(), part.reshape(-1)), tag + ": the partial rows changed"
        k = NB.U * (gamma * invstd).abs() * (fin_err[0] + ref["xh"].abs() * fin_err[1]) / rows
        NB._within(dx, ref["dx"], ref["dx_bound"] + k, tag + " dx")
        for i, (name, got, old) in enumerate((("dbeta", db, -0.5), ("dgamma", dg, 0.25))):
            want = sums[i] + old
            NB._within(got, want, NB.U * sums[i].abs() + NB.U * want.abs() + fin_err[i], f"{tag} {name}")
        if with_col:
            NB._within(dcol, ref["dcol"] + 0.125, ref["dcol_bound"] + k.sum(0) + NB.U * (ref["dcol"] + 0.125).abs(), tag + " dcol")


@pytest.mark.parametrize("case", sorted(SO.LINEAR_WGRAD_CASES), ids=lambda c: "x".join(map(str, c)))
def test_linear_wgrad_on_exact_scratch(pcg, guarded, case):
    """linear_wgrad on every plan of LINEAR_WGRAD_CASES: strided dy, dW / db as outputs and, accumulating, as inout; the slab partials
    come from workspace2 (exactly pcg_linear_wgrad_workspace_bytes).  Source: test_linear_wgrad_first_slab_split."""
    ar, log = guarded
    RAN["linear-wgrad"].add(case)
    B, O, I = case
    want = SO.LINEAR_WGRAD_CASES[case]
    SO.assert_route("LINEAR_WGRAD", case, want)
    S, chunk = (int(v) for v in re.search(r"slabs: (\d+) of (\d+) rows", want).groups())
    factor = (chunk + S + 3) * SO.U
    ops, lib = pcg.ops, pcg.load()
    gen = SO._gen(B * O)
    dyw, x, W0, b0 = SO._randn(B, O + 5, g=gen), SO._randn(B, I, g=gen), SO._randn(O, I, g=gen), SO._randn(O, g=gen)
    dyd, xd = ar.input(_f32(dyw), "dy (wide)"), ar.input(_f32(x), "x")
    dW, db = ar.output((O, I), name="dW"), ar.output((O,), name="db")
    ops.linear_wgrad(dyd[:, 2:], xd, B, O, I, dW, db, ldy=O + 5)
    dW2, db2 = ar.inout(_f32(W0), "dW (accumulate)"), ar.inout(_f32(b0), "db (accumulate)")
    ops.linear_wgrad(dyd[:, 2:], xd, B, O, I, dW2, db2, ldy=O + 5, accumulate_w=True, accumulate_b=True)
    _settle(ar)
    need = lib.pcg_linear_wgrad_workspace_bytes(B, O, I)
    assert (need > 0) == (S > 1), f"{need} bytes of slab partials for {S} slab(s)"          # one slab goes straight to dW: no scratch asked for
    assert [(r.kind, r.nbytes) for r in log] == ([(2, need)] * 2 if need else [])
    assert all(r.changed for r in log)
    rW, rb, mW, mb = SO.R.linear_wgrad(dyw[:, 2:2 + O], x)
    SO._within(dW, rW, factor * mW, f"linear_wgrad {case} dW")
    SO._within(db, rb, factor * mb, f"linear_wgrad {case} db")
    rW, rb, mW, mb = SO.R.linear_wgrad(dyw[:, 2:2 + O], x, W0, b0)
    SO._within(dW2, rW, factor * mW, f"linear_wgrad {case} dW accumulate")
    SO._within(db2, rb, factor * mb, f"linear_wgrad {case} db accumulate")


@pytest.mark.parametrize("B", sorted(SO.WGRAD_GROUPED_CASES))
def test_linear_wgrad_grouped_on_exact_scratch(pcg, guarded, B):
    """linear_wgrad_grouped on every plan of WGRAD_GROUPED_CASES: the four layers of _grouped_operands with every operand and
    gradient in the arena (x and dy column slices stay slices of a guarded buffer).  Source: test_linear_wgrad_grouped_batches."""
    ar, log = guarded
    RAN["linear-wgrad-grouped"].add(B)
    SO.assert_route("LINEAR_WGRAD_GROUPED", (B,), SO.WGRAD_GROUPED_CASES[B])
    Sb, rows = (int(v) for v in re.fullmatch(r"blocks per tile: (\d+), rows per wave: (\d+)", SO.WGRAD_GROUPED_CASES[B]).groups())
    factor = (rows + 4 * Sb + 3) * SO.U
    ops = pcg.ops
    gen = SO._gen(B)
    dy0, x0 = SO._randn(B, 1, g=gen), SO._randn(B, 1, g=gen)
    dy1, x1 = SO._randn(B, 33, g=gen), SO._randn(B, 33, g=gen)
    dy2, xw = SO._randn(B, 9, g=gen), SO._randn(B, 38, g=gen)
    dyw, x3 = SO._randn(B, 40, g=gen), SO._randn(B, 32, g=gen)
    W1, b1 = SO._randn(33, 33, g=gen), SO._randn(33, g=gen)
    host = [(dy0, x0, None, None, True), (dy1, x1, W1, b1, True), (dy2, xw[:, 17:], None, None, False), (dyw[:, 5:18], x3, None, None, True)]
    dv = {k: ar.input(_f32(v), k) for k, v in dict(dy0=dy0, x0=x0, dy1=dy1, x1=x1, dy2=dy2, xw=xw, dyw=dyw, x3=x3).items()}
    views = [(dv["dy0"], dv["x0"], 1, 1, 1, 1), (dv["dy1"], dv["x1"], 33, 33, 33, 33), (dv["dy2"], dv["xw"][:, 17:], 9, 21, 9, 38),
             (dv["dyw"][:, 5:], dv["x3"], 13, 32, 40, 32)]
    items, outs = [], []
    for k, ((dyh, xh, W0, b0, has_db), (dy, x, O, I, ldy, ldx)) in enumerate(zip(host, views)):
        dW = ar.inout(_f32(W0), f"dW{k}") if W0 is not None else ar.output((O, I), name=f"dW{k}")
        db = (ar.inout(_f32(b0), f"db{k}") if b0 is not None else ar.output((O,), name=f"db{k}")) if has_db else None
        items.append((dy, x, O, I, dW, db, ldy, ldx, W0 is not None, b0 is not None))
        outs.append((dW, db))
    ops.linear_wgrad_grouped(items, B, torch.device(DEV))
    _settle(ar)
    assert len(log) >= 1
    for k, ((dyh, xh, W0, b0, has_db), (dW, db)) in enumerate(zip(host, outs)):
        rW, rb, mW, mb = SO.R.linear_wgrad(dyh, xh, W0, b0)
        SO._within(dW, rW, factor * mW, f"grouped B={B} layer {k} dW")
        if has_db:
            SO._within(db, rb, factor * mb, f"grouped B={B} layer {k} db")


@pytest.mark.parametrize("n", SO.REDUCE_NS)
def test_mean_and_abs_mean_on_exact_scratch(pcg, guarded, n):
    """mean_fwd and abs_mean_fwd (no mask, mask, 1 - mask) on both plans of REDUCE_NS with the input in the arena and exactly
    pcg_mean_workspace_bytes / pcg_abs_mean_workspace_bytes of NaN scratch.  Source: test_mean_and_abs_mean."""
    ar, log = guarded
    RAN["reduce"].add(n)
    ops, lib = pcg.ops, pcg.load()
    SO.assert_route("MEAN", (n,), SO._reduce_route(n, 64))
    SO.assert_route("ABS_MEAN", (n,), SO._reduce_route(n, 256))
    gen = SO._gen(n)
    a = SO.R.f32_exact(SO._randn(n, g=gen) + 0.25)
    m = torch.tensor([0.0, 0.25, 0.75, 1.0], dtype=torch.float64)[torch.randint(0, 4, (n,), generator=gen)]
    ad, md = ar.input(_f32(a), "a"), ar.input(_f32(m), "mask")
    got_mean = ops.mean_fwd(ad)
    got_abs = [ops.abs_mean_fwd(ad, md if mask is not None else None, om) for mask, om in ((None, False), (m, False), (m, True))]
    _settle(ar)
    assert [r.nbytes for r in log] == [lib.pcg_mean_workspace_bytes()] + [lib.pcg_abs_mean_workspace_bytes()] * 3
    SO._within(got_mean, a.mean().reshape(1), SO._mean_bound_factor(n) * SO.U * float(a.abs().sum()) / n, f"mean n={n}")
    for got, (mask, om) in zip(got_abs, ((None, False), (m, False), (m, True))):
        ref, mag = SO.R.abs_mean(a, mask, om)
        SO._within(got, ref.reshape(1), SO._abs_mean_bound_factor(n) * SO.U * float(mag) / n, f"abs_mean n={n} mask={mask is not None} one_minus={om}")


# ---- the count ---------------------------------------------------------------------------------------------------------------
def test_every_family_ran_its_whole_table():
    """Per family, the number of cases that ran equals the length of the imported table: a table that grows is picked up by the
    parametrize lists above, and a family that loses cases on the way fails here."""
    got = {fam: len(RAN[fam]) for fam in FAMILY_SIZES}
    want = {fam: n() for fam, n in FAMILY_SIZES.items()}
    assert got == want
