"""GPU parity of the front half of csrc/pointwise.hip -- the fused Adam step (pcg_adam_step, pcg_adam_step_capturable) and the three
BCE kernels (pcg_bce_fwd_bwd, pcg_bce_pair, pcg_bce_logits_fwd_bwd) -- against float64 (tests/optim_ref.py), at every host-side
switch of the Adam launch and every trip boundary of the one-block loss kernels.

Every Adam case names the route it is meant to take and asserts it through pcg_launch_plan_describe (ops.launch_plan, PLAN_ADAM)
before it launches; tests/test_optim_plan_host.py checks the same tables, the references and the bounds without a device.

Every device buffer a kernel sees lies between two runs of at least eight sentinel floats that are compared bit for bit afterwards
("misaligned" is a view one float past a 16-byte boundary: nine sentinels in front); the gradient is compared with its upload; an
output that is not asked for is not passed.  One Adam step is checked on its own against the float64 step from the device's own
state before it (teacher forced): the bounds (derived in tests/optim_ref.py, u = 2^-24) do not compound.

Each check prints `ratio[<kernel>]`, its largest error / bound ratio, before it asserts.  The largest over all cases on the MI355X:
Adam p 0.997, m 0.997 (a half-ulp rounding of a result just above a power of two, where the bound is that one rounding), v 0.845, the
three-step segments run 0.801; bce loss 0.196, dp 0.967 (the smallest normal p times 1 / n: a subnormal product, held to half the
subnormal spacing); bce_pair loss 0.083, dp 0.451; bce_logits loss 0.210, dz 0.705.
"""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
SENT = -77.0
PAD = 8                       # sentinel floats on either side of every device buffer
LR, BETA2, EPS = 1e-3, 0.999, 1e-8
T_LARGE = 20000               # 0.999^20000 = 2e-9 < 2^-25: 1 - beta2^t has rounded to 1 in fp32, sqrt(1 - beta2^t) in double has not


# =================================================================================================================================
# Case tables.  Host data only -- tests/test_optim_plan_host.py imports them.
# =================================================================================================================================
def _grid(items, blocks):
    passes = -(-items // (blocks * 256))
    return f"{blocks} {'block' if blocks == 1 else 'blocks'} of 256: {passes} {'pass' if passes == 1 else 'passes'}"


def _f4(n, blocks):
    return f"float4 lanes: {_grid(n // 4, blocks)}" + (f", tail of {n % 4}" if n % 4 else "")


def _sc(n, blocks):
    return f"scalar lanes: {_grid(n, blocks)}"


N_ONE_PASS = 262144           # 256 blocks x 256 threads x 4 floats: exactly one pass of the capped capturable grid
N_SECOND_PASS = 262148 + 3    # one float4 more (a second pass with one working thread) and the tail
N_SCALAR_CAP = 65537          # 256 x 256 scalar lanes and one element
N_EAGER_CAP = 8388608 + 4 + 1  # 8192 x 256 x 4, one float4 more, a tail of one

# (n, misaligned, route of pcg_adam_step, route of pcg_adam_step_capturable)
ADAM_ROUTE_CASES = [
    (1, False, _sc(1, 1), _sc(1, 1)),                                  # scalar by size
    (3, False, _sc(3, 1), _sc(3, 1)),
    (4, False, _f4(4, 1), _f4(4, 1)),                                  # one float4
    (7, False, _f4(7, 1), _f4(7, 1)),                                  # one float4 plus a tail of 3
    (1003, False, _f4(1003, 1), _f4(1003, 1)),                         # bulk plus tail
    (N_ONE_PASS, False, _f4(N_ONE_PASS, 256), _f4(N_ONE_PASS, 256)),
    (N_SECOND_PASS, False, _f4(N_SECOND_PASS, 257), "float4 lanes: 256 blocks of 256: 2 passes, tail of 3"),
    (N_SCALAR_CAP, True, _sc(N_SCALAR_CAP, 257), "scalar lanes: 256 blocks of 256: 2 passes"),
    (N_EAGER_CAP, False, "float4 lanes: 8192 blocks of 256: 2 passes, tail of 1", "float4 lanes: 256 blocks of 256: 33 passes, tail of 1"),
]
N_MISALIGNED = 1003
MISALIGNED_ROUTE = _sc(N_MISALIGNED, 4)                                  # any one pointer 4 bytes off: both entries
BUFFERS = ("param", "grad", "exp_avg", "exp_avg_sq")

DECAYS = {"none": dict(wd=0.0, decoupled=False), "l2": dict(wd=0.01, decoupled=False), "decoupled": dict(wd=0.01, decoupled=True)}
BETA1S = (0.0, 0.5, R.beta1_just_above_half(), 0.9)                     # lerp: second form, second, first (just), first
HYPER_SIZES = (1003, N_SECOND_PASS)
HYPER_STEPS = (1, 2, T_LARGE)

# instantiation agreement: (n, misaligned) of the launches one data set goes through; element i of the data is element i of each
AGREE_N = 1003
AGREE_LAUNCHES = [(1003, False), (1003, True), (1004, False), (999, False)]   # 1000..1002 tail | all scalar | all bulk | 996..998 tail
AGREE_HYPERS = [("none", 0.9), ("l2", 0.5), ("decoupled", 0.0)]

KNOB_N = N_SECOND_PASS
# PCG_ADAM_TICK_BLOCKS -> the capturable route of KNOB_N ("0" is clamped to one block)
KNOB_SETTINGS = [("1", "float4 lanes: 1 block of 256: 257 passes, tail of 3"), ("7", "float4 lanes: 7 blocks of 256: 37 passes, tail of 3"),
                 ("0", "float4 lanes: 1 block of 256: 257 passes, tail of 3")]

BCE_N = (1, 7, 255, 256, 257, 1000, 1024, 2049)
BCE_TARGETS = (0.0, 1.0, 0.9, "tensor")
LOGIT_TARGETS = (0.0, 1.0, 0.9)
PAIR_N_HALF = (1, 255, 257, 1024)
PAIR_COTANGENTS = (0.7, -1.3, 2.1)


def all_routes():
    """[(args of PLAN_ADAM, expected text)] of every table above."""
    out = []
    for n, mis, eager, capt in ADAM_ROUTE_CASES:
        out += [((n, int(not mis), 0), eager), ((n, int(not mis), 1), capt)]
    out += [((N_MISALIGNED, 0, c), MISALIGNED_ROUTE) for c in (0, 1)]
    out += [((n, 1, 1), _f4(n, min(256, -(-(n // 4) // 256)))) for n in HYPER_SIZES]
    for n, mis in AGREE_LAUNCHES:
        out.append(((n, int(not mis), 1), _sc(n, 4) if mis else _f4(n, 1)))
    return out


# the routes this file is there to cover, each reached by at least one case
REQUIRED_ROUTES = (r"^scalar lanes: 1 block of 256: 1 pass$", r"^float4 lanes: 1 block of 256: 1 pass$", r"^float4 lanes: 1 block of 256: 1 pass, tail of 3$",
                   r"^float4 lanes: 256 blocks of 256: 1 pass$", r"^float4 lanes: 256 blocks of 256: 2 passes, tail of 3$",
                   r"^scalar lanes: 256 blocks of 256: 2 passes$", r"^float4 lanes: 8192 blocks of 256: 2 passes, tail of 1$",
                   r"^scalar lanes: 4 blocks of 256: 1 pass$", r"^float4 lanes: 257 blocks of 256: 1 pass, tail of 3$")


def plan(n, aligned, capturable):
    from pcgan_amd import _lib, ops
    return ops.launch_plan(_lib.PLAN_ADAM, int(n), int(aligned), int(capturable))


def assert_route(args, want):
    got = plan(*args)
    assert got == want, f"route moved: PLAN_ADAM{tuple(args)} takes {got!r}, the case expects {want!r}"


def check_all_routes():
    import re
    seen = []
    for args, want in all_routes():
        assert_route(args, want)
        seen.append(want)
    for pat in REQUIRED_ROUTES:
        assert any(re.search(pat, s) for s in seen), f"no case reaches an Adam route like {pat!r}"


# =================================================================================================================================
# host-side inputs (no device): shared by the GPU tests, tests/adam_knob_child.py and tests/test_optim_plan_host.py
# =================================================================================================================================
@lru_cache(maxsize=3)
def adam_state(n, seed=0):
    """fp32 (p, grad, m, v) of a net in mid-training: unit parameters and gradients, moments of the matching size, v >= 0.  With
    n >= 8: element 0 has grad = m = v = 0 (the update is 0 / eps), 1 a zero parameter, 2 fresh moments under a unit gradient."""
    g = torch.Generator().manual_seed(1000003 * seed + n)
    p, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g) + 1e-4
    if n >= 8:
        grad[0] = m[0] = v[0] = 0.0
        p[1] = 0.0
        m[2] = v[2] = 0.0
        grad[2] = 1.0
    return p, grad, m, v


def hyper(decay="none", beta1=0.9, beta2=BETA2, lr=LR):
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=EPS, **DECAYS[decay])


def adam_ref(state, t, hp):
    p, g, m, v = (x.double() for x in state)
    return R.adam_step(p, g, m, v, t, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], hp["decoupled"])


_BCE_P_EDGES = (0.0, 1.0, float(np.finfo(np.float32).tiny), 1.0 - 2.0 ** -24, 1e-40)     # 0, 1, smallest normal, 1 - 2^-24, a denormal
_LOGIT_EDGES = (100.0, -100.0, 1e4, -1e4, 0.0)


def _with_edges(body, edges):
    """The edge values over the first elements (all of them from n = 7 on; n = 1 keeps its interior value)."""
    n = body.numel()
    if n > 1:
        k = min(n - 1, len(edges))
        body[:k] = torch.tensor(edges[:k], dtype=torch.float32)
    return body


@lru_cache(maxsize=None)
def bce_inputs(n, seed=0):
    """fp32 (p, soft targets, logits): probabilities in 0.02 .. 0.98 with the edge values in front, targets in 0 .. 1 with an exact 0 and
    1, logits 5 randn with +-100, +-1e4 and 0 in front."""
    g = torch.Generator().manual_seed(7919 * seed + n)
    p = _with_edges(0.02 + 0.96 * torch.rand(n, generator=g), _BCE_P_EDGES)
    t = torch.rand(n, generator=g)
    if n > 2:
        t[-1], t[-2] = 0.0, 1.0
    z = _with_edges(5.0 * torch.randn(n, generator=g), _LOGIT_EDGES)
    assert n < 6 or (float(p[4]) > 0 and float(p[3]) < 1)          # the denormal and 1 - 2^-24 survived the fp32 tensor
    return p, t, z


# =================================================================================================================================
# device helpers
# =================================================================================================================================
@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd


class Guarded:
    """A device copy of `host` between `lead` (>= 8; 9: one float past a 16-byte boundary) and 8 sentinel floats."""

    def __init__(self, host, misaligned=False):
        self.lead, self.n = PAD + int(misaligned), host.numel()
        self.buf = torch.full((self.lead + self.n + PAD,), SENT, dtype=torch.float32, device=DEV)
        self.view = self.buf[self.lead:self.lead + self.n]
        self.view.copy_(host)
        assert self.view.data_ptr() % 16 == (4 if misaligned else 0)

    def host(self):
        return self.view.cpu()

    def assert_intact(self, what):
        b = self.buf.cpu().view(torch.int32)
        s = torch.tensor([SENT]).view(torch.int32)
        assert bool((b[:self.lead] == s).all()), f"{what}: wrote in front of the buffer"
        assert bool((b[self.lead + self.n:] == s).all()), f"{what}: wrote past the end of the buffer"


class Counter:
    """The int64 device step counter between sentinels, and the 48-byte scratch block (struct AdamCache: ticket at byte 0, t_for at 32)."""

    def __init__(self, step=0):
        self.buf = torch.full((2 * 4 + 1,), -77, dtype=torch.int64, device=DEV)
        self.step = self.buf[4:5]
        self.step.fill_(step)
        self.scratch = Guarded(torch.zeros(12))
        assert self.scratch.view.data_ptr() % 8 == 0

    def read(self):
        """(counter, ticket, t_for)"""
        h = self.scratch.host()
        return int(self.step.item()), int(h.view(torch.int32)[0]), int(h.view(torch.int64)[4])

    def assert_intact(self, what):
        b = self.buf.cpu()
        assert bool((b[:4] == -77).all()) and bool((b[5:] == -77).all()), f"{what}: wrote around the step counter"
        self.scratch.assert_intact(what + " scratch")
        assert bool((self.scratch.host()[10:] == 0).all()), f"{what}: wrote behind the 40 bytes of AdamCache"


class AdamBuffers:
    """Guarded device copies of one (p, grad, m, v); step() launches either entry on them."""

    def __init__(self, state, misaligned=(False, False, False, False)):
        self.state = state
        self.bufs = [Guarded(x, mis) for x, mis in zip(state, misaligned)]

    def step(self, ops, hp, t=None, counter=None):
        a = [b.view for b in self.bufs]
        args = (hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], hp["decoupled"])
        if counter is None:
            ops.adam_step(*a, *args, t)
        else:
            ops.adam_step_capturable(*a, *args, counter.step, counter.scratch.view)

    def read(self):
        """(p, m, v) on the host"""
        torch.cuda.synchronize()
        return self.bufs[0].host(), self.bufs[2].host(), self.bufs[3].host()

    def assert_clean(self, what):
        for b, name in zip(self.bufs, BUFFERS):
            b.assert_intact(f"{what} {name}")
        assert torch.equal(self.bufs[1].host().view(torch.int32), self.state[1].view(torch.int32)), f"{what}: the gradient was written"


def _within(got, ref, bound, what, kernel):
    """|got - ref| <= bound per element, in float64; prints the worst ratio before it asserts."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.double().reshape(-1)
    bound = bound.double().reshape(-1) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.argmax())
    print(f"ratio[{kernel}] {what}: {float(ratio[i]):.3f} (element {i}: got {float(got[i]):.9g}, float64 {float(ref[i]):.9g}, bound {float(bound[i]):.3g})")
    assert float(ratio[i]) <= 1.0, f"{what}: element {i} is {float(ratio[i]):.2f} bounds off ({float(got[i])!r} vs {float(ref[i])!r}, bound {float(bound[i]):.3g})"


def _check_step(out, ref, what):
    p, m, v = out
    _within(p, ref["p"], ref["p_bound"], what + " p", "adam p")
    _within(m, ref["m"], ref["m_bound"], what + " m", "adam m")
    _within(v, ref["v"], ref["v_bound"], what + " v", "adam v")


def _bits_equal(a, b, what):
    for x, y, name in zip(a, b, ("p", "m", "v")):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {name} differs in its bits"


def _one_step(ops, state, mis, capturable, hp, t, what):
    """One launch of either entry at step t on fresh guarded buffers: (p, m, v), with every guard, the gradient and -- capturable --
    the counter, the ticket and the tag checked."""
    bufs = AdamBuffers(state, mis)
    counter = Counter(t - 1) if capturable else None
    bufs.step(ops, hp, t, counter)
    out = bufs.read()
    bufs.assert_clean(what)
    if capturable:
        counter.assert_intact(what)
        assert counter.read() == (t, 0, t + 1), f"{what}: (counter, ticket, tag) = {counter.read()}, expected {(t, 0, t + 1)}"
    return out


# =================================================================================================================================
# Adam
# =================================================================================================================================
@pytest.mark.parametrize("case", ADAM_ROUTE_CASES, ids=lambda c: f"n{c[0]}{'-misaligned' if c[1] else ''}")
def test_adam_routes(pcg, case):
    """Both entries at every grid the launch can take: scalar by size, one float4, the tail lanes, one and two passes of the capped
    capturable grid, the capped scalar grid, the 8192-block cap of the eager entry.  AdamW with beta1 = 0.9 at step 3."""
    n, mis, eager, capt = case
    state, hp, t = adam_state(n), hyper("decoupled"), 3
    ref = adam_ref(state, t, hp)
    outs = []
    for capturable, want in ((False, eager), (True, capt)):
        assert_route((n, int(not mis), int(capturable)), want)
        what = f"adam n={n} {'capturable' if capturable else 'eager'}"
        outs.append(_one_step(pcg.ops, state, (mis,) * 4, capturable, hp, t, what))
        _check_step(outs[-1], ref, what)
    _bits_equal(outs[0], outs[1], f"adam n={n}: eager against capturable")          # step 3 at the betas test_adam asserts it for


@pytest.mark.parametrize("which", range(4), ids=BUFFERS)
def test_adam_one_misaligned_pointer(pcg, which):
    """Each pointer alone 4 bytes off a 16-byte boundary sends the launch down adam_kernel<1>."""
    mis = tuple(i == which for i in range(4))
    state, hp, t = adam_state(N_MISALIGNED), hyper("l2"), 2
    ref = adam_ref(state, t, hp)
    for capturable in (False, True):
        assert_route((N_MISALIGNED, 0, int(capturable)), MISALIGNED_ROUTE)
        what = f"adam misaligned {BUFFERS[which]} {'capturable' if capturable else 'eager'}"
        _check_step(_one_step(pcg.ops, state, mis, capturable, hp, t, what), ref, what)


@pytest.mark.parametrize("decay", sorted(DECAYS))
@pytest.mark.parametrize("n", HYPER_SIZES)
def test_adam_hyper_parameters(pcg, n, decay):
    """No decay, L2 decay (g + wd p: the branch AdamW never takes) and decoupled decay, with beta1 on either side of the lerp switch
    (0.5 takes the second form, the next beta1 whose fp32 weight falls below 0.5f the first), at steps 1, 2 and one where 1 - beta2^t
    has rounded to 1.  The capturable entry, the step set through the device counter; the eager entry as well at the small size."""
    state = adam_state(n)
    assert [R.lerp_takes_first_form(b) for b in BETA1S] == [False, False, True, True]
    for beta1 in BETA1S:
        hp = hyper(decay, beta1)
        for t in HYPER_STEPS:
            ref = adam_ref(state, t, hp)
            for capturable in ((True, False) if n == HYPER_SIZES[0] else (True,)):
                assert_route((n, 1, int(capturable)), _f4(n, min(256, -(-(n // 4) // 256)) if capturable else -(-(n // 4) // 256)))
                what = f"adam n={n} {decay} beta1={beta1!r} t={t} {'capturable' if capturable else 'eager'}"
                _check_step(_one_step(pcg.ops, state, (False,) * 4, capturable, hp, t, what), ref, what)


@pytest.mark.parametrize("decay,beta1", AGREE_HYPERS)
def test_adam_instantiations_agree(pcg, decay, beta1):
    """csrc/epoch_wg.h promises ONE Adam element update everywhere: the same (p, g, m, v) through the float4 lanes of adam_kernel<4>,
    the tail lanes of its block 0 and adam_kernel<1> come out bit-identical.  n = 1003 aligned (elements 1000..1002 on the tail
    lanes), misaligned (all scalar), n = 1004 (all float4), n = 999 (996..998 on the tail lanes)."""
    full = adam_state(AGREE_N + 1, seed=3)
    hp, t = hyper(decay, beta1), 2
    outs = {}
    for n, mis in AGREE_LAUNCHES:
        assert_route((n, int(not mis), 1), _sc(n, 4) if mis else _f4(n, 1))
        what = f"adam agreement n={n}{' misaligned' if mis else ''}"
        outs[(n, mis)] = _one_step(pcg.ops, tuple(x[:n].clone() for x in full), (mis,) * 4, True, hp, t, what)
    base = outs[(1003, False)]
    _check_step(base, adam_ref(tuple(x[:1003] for x in full), t, hp), "adam agreement n=1003")
    for (n, mis), out in outs.items():
        k = min(n, 1003)
        _bits_equal([x[:k] for x in out], [x[:k] for x in base], f"adam {decay} beta1={beta1}: n={n}{' misaligned' if mis else ''} against n=1003")


def _teacher_forced(ops, bufs, counter, hp, what):
    """One capturable launch checked against the float64 step from the state before it, at the step the counter names."""
    p, m, v = bufs.read()
    t = counter.read()[0] + 1
    bufs.step(ops, hp, None, counter)
    out = bufs.read()
    _check_step(out, adam_ref((p, bufs.state[1], m, v), t, hp), f"{what} t={t}")
    assert counter.read() == (t, 0, t + 1), f"{what}: (counter, ticket, tag) = {counter.read()} after step {t}"
    return out


@pytest.mark.parametrize("n", [1003, N_SECOND_PASS])
def test_adam_cache_hit_equals_miss(pcg, n):
    """Five capturable steps twice: one replica has its scratch zeroed before every launch (every launch computes its corrections),
    the other misses once and then loads what the launch before left.  Bit-identical after every step; after k launches the
    counter is k, the ticket 0, the tag k + 1."""
    hp = hyper("decoupled", 0.5)
    a, b = AdamBuffers(adam_state(n)), AdamBuffers(adam_state(n))
    ca, cb = Counter(), Counter()
    for k in range(1, 6):
        ca.scratch.view.zero_()
        assert ca.read()[2] == 0 and cb.read()[2] == (k if k > 1 else 0)
        a.step(pcg.ops, hp, None, ca)
        b.step(pcg.ops, hp, None, cb)
        _bits_equal(a.read(), b.read(), f"adam n={n} step {k}: every launch missing against one miss, then hits")
        assert ca.read() == (k, 0, k + 1) and cb.read() == (k, 0, k + 1), f"step {k}: {ca.read()} / {cb.read()}"
    for x, c in ((a, ca), (b, cb)):
        x.assert_clean(f"adam cache n={n}")
        c.assert_intact(f"adam cache n={n}")


def test_adam_cache_misses(pcg):
    """The three ways a cached correction goes stale, each step against float64 at the step the counter names: beta2 changed after step
    2; the counter set back to 1 after step 3 (what restore() / load_state_dict() do); the counter set to the very value the tag
    holds (the tag names the NEXT step: t = counter + 1 is one past it)."""
    ops, n = pcg.ops, 1003
    hp = hyper("none", 0.9)
    bufs, c = AdamBuffers(adam_state(n, seed=1)), Counter()
    for _ in range(2):
        _teacher_forced(ops, bufs, c, hp, "adam changed beta2")
    _teacher_forced(ops, bufs, c, hyper("none", 0.9, beta2=0.99), "adam changed beta2")
    _teacher_forced(ops, bufs, c, hyper("none", 0.5, beta2=0.99), "adam changed beta1")
    bufs.assert_clean("adam changed betas")

    bufs, c = AdamBuffers(adam_state(n, seed=2)), Counter()
    for _ in range(3):
        _teacher_forced(ops, bufs, c, hp, "adam restored counter")
    c.step.fill_(1)
    assert c.read() == (1, 0, 4)
    _teacher_forced(ops, bufs, c, hp, "adam restored counter")
    assert c.read() == (2, 0, 3)
    _teacher_forced(ops, bufs, c, hp, "adam restored counter")              # a hit again

    bufs, c = AdamBuffers(adam_state(n, seed=4)), Counter()
    for _ in range(3):
        _teacher_forced(ops, bufs, c, hp, "adam counter at the tag")
    c.step.fill_(c.read()[2])
    assert c.read() == (4, 0, 4)
    _teacher_forced(ops, bufs, c, hp, "adam counter at the tag")
    assert c.read() == (5, 0, 6)
    bufs.assert_clean("adam counter at the tag")
    c.assert_intact("adam counter at the tag")


def test_adam_graph_replay(pcg):
    """One capturable step alone in a captured graph (a linear graph): three replays equal three direct launches bit for bit, counter,
    ticket and tag included."""
    ops, n, hp = pcg.ops, N_SECOND_PASS, hyper("l2", 0.9)
    assert_route((n, 1, 1), "float4 lanes: 256 blocks of 256: 2 passes, tail of 3")
    direct, cd = AdamBuffers(adam_state(n)), Counter()
    for _ in range(3):
        direct.step(ops, hp, None, cd)
    want = direct.read()
    replayed, cr = AdamBuffers(adam_state(n)), Counter()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step(ops, hp, None, cr)
    torch.cuda.synchronize()
    assert cr.read() == (0, 0, 0), "captured, not run"
    _bits_equal(replayed.read(), (replayed.state[0], replayed.state[2], replayed.state[3]), "adam graph: captured, not run")
    for _ in range(3):
        graph.replay()
    _bits_equal(replayed.read(), want, "adam graph: three replays against three direct launches")
    assert cr.read() == cd.read() == (3, 0, 4)
    replayed.assert_clean("adam graph")
    cr.assert_intact("adam graph")


def knob_run(ops):
    """Two capturable steps at KNOB_N under whatever PCG_ADAM_TICK_BLOCKS this process started with: {"p", "m", "v", "plan", and the
    state after the first step}.  tests/adam_knob_child.py runs it in a fresh process per setting."""
    hp = hyper("decoupled", 0.5)
    bufs, c = AdamBuffers(adam_state(KNOB_N)), Counter()
    bufs.step(ops, hp, None, c)
    p1, m1, v1 = bufs.read()
    bufs.step(ops, hp, None, c)
    p, m, v = bufs.read()
    bufs.assert_clean("adam knob run")
    c.assert_intact("adam knob run")
    assert c.read() == (2, 0, 3)
    return {"p": p.numpy(), "m": m.numpy(), "v": v.numpy(), "p1": p1.numpy(), "m1": m1.numpy(), "v1": v1.numpy(), "plan": np.array(plan(KNOB_N, 1, 1))}


@pytest.fixture(scope="module")
def knob_default(pcg):
    """This process's default-knob run, held to float64 step by step; shared by the knob cases and never written."""
    hp = hyper("decoupled", 0.5)
    assert os.environ.get("PCG_ADAM_TICK_BLOCKS") is None
    mine = knob_run(pcg.ops)
    assert str(mine["plan"]) == "float4 lanes: 256 blocks of 256: 2 passes, tail of 3"
    state = adam_state(KNOB_N)
    first = tuple(torch.from_numpy(mine[k]) for k in ("p1", "m1", "v1"))
    _check_step(first, adam_ref(state, 1, hp), "adam default knob t=1")
    _check_step(tuple(torch.from_numpy(mine[k]) for k in ("p", "m", "v")), adam_ref((first[0], state[1], first[1], first[2]), 2, hp), "adam default knob t=2")
    return mine


@pytest.mark.parametrize("value,want", KNOB_SETTINGS, ids=[v for v, _ in KNOB_SETTINGS])
def test_adam_tick_blocks_knob(knob_default, tmp_path, value, want):
    """PCG_ADAM_TICK_BLOCKS is read once per process: tests/adam_knob_child.py runs two capturable steps in a fresh child per setting
    (one at a time, its exit status checked).  The knob moves no arithmetic: p, m, v are bit-identical to this process's
    default-knob run, which is held to float64; "0" is clamped to one block."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adam_knob_child.py")
    out = tmp_path / "knob.npz"
    r = subprocess.run([sys.executable, child, str(out)], env={**os.environ, "PCG_ADAM_TICK_BLOCKS": value}, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, f"knob child PCG_ADAM_TICK_BLOCKS={value} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = np.load(out)
    assert str(got["plan"]) == want, f"PCG_ADAM_TICK_BLOCKS={value}: the child took {str(got['plan'])!r}, expected {want!r}"
    for k in ("p", "m", "v"):
        assert got[k].shape == knob_default[k].shape and np.array_equal(got[k].view(np.int32), knob_default[k].view(np.int32)), \
            f"PCG_ADAM_TICK_BLOCKS={value}: {k} differs from the default knob"


# =================================================================================================================================
# optim.Adam / AdamW: segments
# =================================================================================================================================
SEG_GROUPS = (dict(lr=2e-3, betas=(0.5, 0.999)), dict(lr=5e-4, betas=(0.9, 0.99), weight_decay=0.05))


def _seg_layers(m):
    import torch.nn as nn
    m.conv, m.l1, m.l2 = nn.Conv2d(3, 5, 3), nn.Linear(7, 3), nn.Linear(3, 1)


def _seg_groups(net):
    """Group 0: the conv layer and the last Linear -- two runs of memory with the other group's layer between them; group 1: the
    middle Linear with its own lr, betas and weight decay."""
    return [dict(params=list(net.conv.parameters()) + list(net.l2.parameters()), **SEG_GROUPS[0]),
            dict(params=list(net.l1.parameters()), **SEG_GROUPS[1])]


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_adam_segments_two_groups(pcg, name):
    """A FlatModule under two param groups: three launches per step (group 0 has two runs of adjacent parameters, group 1 one), each
    with its group's hyper-parameters and its own counter.  Three steps against torch.optim.Adam / AdamW in float64 on the CPU,
    within the one-step bound compounded over the three steps (tests/optim_ref.py, "Compounding")."""
    import torch.nn as nn
    from pcgan_amd import optim
    from pcgan_amd.nn import FlatModule

    class Net(FlatModule):
        def __init__(self):
            super().__init__()
            _seg_layers(self)

    class TorchNet(nn.Module):
        def __init__(self):
            super().__init__()
            _seg_layers(self)

    torch.manual_seed(21)
    ref = TorchNet()
    values = {k: v.clone() for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(22)
    grads = [[torch.randn(p.shape, generator=g) for p in ref.parameters()] for _ in range(3)]
    ref.double()
    ropt = getattr(torch.optim, name)(_seg_groups(ref), foreach=False)
    net = Net()
    net.load_state_dict(values)
    net.to(DEV)
    net.zero_grad()
    opt = getattr(optim, name)(_seg_groups(net))
    assert opt.num_segments() == 3
    # the compounded bound, per parameter, along the float64 trajectory
    group_of = {id(p): gi for gi, grp in enumerate(ropt.param_groups) for p in grp["params"]}
    chain = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), err=None) for p in ref.parameters()]
    for s in range(3):
        for p, q, gr in zip(net.parameters(), ref.parameters(), grads[s]):
            p.grad.copy_(gr)
            q.grad = gr.double()
        opt.step()
        ropt.step()
        for c, q, gr in zip(chain, ref.parameters(), grads[s]):
            grp = ropt.param_groups[group_of[id(q)]]
            r = R.adam_step(c["p"], gr.double(), c["m"], c["v"], s + 1, grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"],
                            grp["weight_decay"], name == "AdamW", c["err"])
            c.update(p=r["p"], m=r["m"], v=r["v"], err=(r["p_bound"], r["m_bound"], r["v_bound"]))
            torch.testing.assert_close(r["p"], q.detach(), rtol=1e-12, atol=1e-14)      # the chained reference IS torch's float64 run
    torch.cuda.synchronize()
    for (pname, p), q, c in zip(net.named_parameters(), ref.parameters(), chain):
        _within(p.detach().cpu().contiguous(), q.detach().contiguous(), c["err"][0].contiguous(), f"{name} segments {pname} after 3 steps", "adam segments p")
    assert opt.num_segments() == 3
    steps = sorted(int(st["step"].item()) for b in opt._segments for st in b)
    assert steps == [3, 3, 3]


# =================================================================================================================================
# BCE
# =================================================================================================================================
def _bce_launch(pcg, entry, x, target, tconst, grad_scale, grad_out, need_loss, need_grad):
    """pcg_bce_fwd_bwd / pcg_bce_logits_fwd_bwd on guarded buffers; an output that is not needed is not passed.  Returns (loss, grad)
    on the host (None where absent) after checking every guard and that the inputs were not written."""
    from pcgan_amd import _lib
    ops, lib = pcg.ops, _lib.load()
    n = x.numel()
    xb = Guarded(x)
    tb = Guarded(target) if target is not None else None
    gob = Guarded(torch.tensor([grad_out])) if grad_out is not None else None
    lossb = Guarded(torch.full((1,), SENT)) if need_loss else None
    gradb = Guarded(torch.full((n,), SENT)) if need_grad else None
    ptr = lambda b: ops._p(b.view if b is not None else None)         # noqa: E731
    if entry == "bce":
        rc = lib.pcg_bce_fwd_bwd(ptr(xb), ptr(tb), float(tconst), n, float(grad_scale), ptr(gob), ptr(lossb), ptr(gradb), ops._stream())
    else:
        rc = lib.pcg_bce_logits_fwd_bwd(ptr(xb), float(tconst), n, float(grad_scale), ptr(gob), ptr(lossb), ptr(gradb), ops._stream())
    assert rc == 0, lib.pcg_last_error()
    torch.cuda.synchronize()
    for b, name in ((xb, "input"), (tb, "target"), (gob, "grad_out"), (lossb, "loss"), (gradb, "gradient")):
        if b is not None:
            b.assert_intact(f"{entry} n={n} {name}")
    assert torch.equal(xb.host().view(torch.int32), x.view(torch.int32)), f"{entry} n={n}: the input was written"
    if tb is not None:
        assert torch.equal(tb.host().view(torch.int32), target.view(torch.int32)), f"{entry} n={n}: the target was written"
    return (lossb.host() if need_loss else None), (gradb.host() if need_grad else None)


GRAD_SCALE, GRAD_OUT = 0.5, -1.7


def _three_forms(pcg, entry, x, target, tconst, ref_of, what, kernel):
    """Loss and gradient together (grad_scale 1, no grad_out); the loss alone: the same bits; the gradient alone under grad_scale
    0.5 and a device grad_out of -1.7."""
    gkey = "dp" if entry == "bce" else "dz"
    ref = ref_of(1.0)
    loss, grad = _bce_launch(pcg, entry, x, target, tconst, 1.0, None, True, True)
    _within(loss, ref["loss"], ref["loss_bound"], f"{what} loss", f"{kernel} loss")
    _within(grad, ref[gkey], ref[gkey + "_bound"], f"{what} gradient", f"{kernel} {gkey}")
    only, none = _bce_launch(pcg, entry, x, target, tconst, 1.0, None, True, False)
    assert none is None and torch.equal(only.view(torch.int32), loss.view(torch.int32)), f"{what}: the loss alone differs from the loss with the gradient"
    gs = R.f32_scalar(GRAD_SCALE) * R.f32_scalar(GRAD_OUT)
    ref = ref_of(gs)
    none, grad = _bce_launch(pcg, entry, x, target, tconst, GRAD_SCALE, GRAD_OUT, False, True)
    assert none is None
    _within(grad, ref[gkey], ref[gkey + "_bound"], f"{what} gradient alone, scaled", f"{kernel} {gkey}")


@pytest.mark.parametrize("n", BCE_N)
def test_bce_trip_boundaries(pcg, n):
    """bce_kernel around the 256-thread trip boundary with constant targets 0, 1, 0.9 and a tensor of soft targets; p holds 0, 1, the
    smallest normal, 1 - 2^-24 and a denormal (both clamps)."""
    p, soft, _ = bce_inputs(n)
    for t in BCE_TARGETS:
        tens = soft if t == "tensor" else None
        tc = 0.0 if t == "tensor" else t
        tref = soft.double() if t == "tensor" else R.f32_scalar(t)
        _three_forms(pcg, "bce", p, tens, tc, lambda gs: R.bce(p.double(), tref, gs), f"bce n={n} target {t}", "bce")


@pytest.mark.parametrize("n", BCE_N)
def test_bce_logits_trip_boundaries(pcg, n):
    """bce_logits_kernel at the same sizes; the logits hold +-100 and +-1e4 (expf overflows to inf in 1 / (1 + expf(-x))) and 0."""
    _, _, z = bce_inputs(n)
    for t in LOGIT_TARGETS:
        _three_forms(pcg, "bce_logits", z, None, t, lambda gs: R.bce_with_logits(z.double(), R.f32_scalar(t), gs), f"bce_logits n={n} target {t}", "bce_logits")


@pytest.mark.parametrize("n_half", PAIR_N_HALF)
def test_bce_pair_cotangents(pcg, n_half):
    """bce_pair_kernel: all eight present / absent combinations of the three cotangents (all missing counts as 1, otherwise a missing
    one as 0); loss[0] and loss[1] carry the bits of two pcg_bce_fwd_bwd launches on the halves, loss[2] is their fp32 sum; the loss
    alone and the gradient alone, the absent output not passed."""
    from pcgan_amd import _lib
    ops, lib = pcg.ops, _lib.load()
    p = bce_inputs(2 * n_half, seed=5)[0]
    t0, t1 = 0.9, 0.0
    halves = [_bce_launch(pcg, "bce", h.clone(), None, t, 1.0, None, True, False)[0] for h, t in ((p[:n_half], t0), (p[n_half:], t1))]
    for mask in range(8):
        cot = [PAIR_COTANGENTS[i] if mask >> i & 1 else None for i in range(3)]
        for need_loss, need_grad in ((True, True), (True, False), (False, True)) if mask in (0, 5) else ((True, True),):
            what = f"bce_pair n_half={n_half} cotangents {cot} loss={need_loss} grad={need_grad}"
            pb = Guarded(p)
            cb = [Guarded(torch.tensor([c])) if c is not None else None for c in cot]
            lossb = Guarded(torch.full((3,), SENT)) if need_loss else None
            gradb = Guarded(torch.full((2 * n_half,), SENT)) if need_grad else None
            ptr = lambda b: ops._p(b.view if b is not None else None)         # noqa: E731
            rc = lib.pcg_bce_pair(ptr(pb), n_half, t0, t1, ptr(cb[0]), ptr(cb[1]), ptr(cb[2]), ptr(lossb), ptr(gradb), ops._stream())
            assert rc == 0, lib.pcg_last_error()
            torch.cuda.synchronize()
            for b in [pb, lossb, gradb] + cb:
                if b is not None:
                    b.assert_intact(what)
            assert torch.equal(pb.host().view(torch.int32), p.view(torch.int32)), f"{what}: the input was written"
            ref = R.bce_pair(p.double(), n_half, R.f32_scalar(t0), R.f32_scalar(t1), *[None if c is None else R.f32_scalar(c) for c in cot])
            if need_loss:
                loss = lossb.host()
                _within(loss, ref["loss"], ref["loss_bound"], f"{what} loss", "bce_pair loss")
                for h in (0, 1):
                    assert torch.equal(loss[h:h + 1].view(torch.int32), halves[h].view(torch.int32)), f"{what}: loss[{h}] differs from a launch on the half alone"
                assert torch.equal((loss[0:1] + loss[1:2]).view(torch.int32), loss[2:3].view(torch.int32)), f"{what}: loss[2] is not the fp32 sum"
            if need_grad:
                _within(gradb.host(), ref["dp"], ref["dp_bound"], f"{what} gradient", "bce_pair dp")
