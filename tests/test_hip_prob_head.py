"""GPU: the two entries of csrc/prob_head.hip through pcgan_amd.ops, each alone, eagerly and from one captured and
replayed HIP graph, with every output pre-filled with a sentinel before every run.

Rows are R = 2, 6, 8 in mode D and 1, 3, 4 in mode G (the row halves, odd rows), plus 600 / 301 rows of 8 columns, the smallest at
which the finishing workgroup and the loss op walk their row loops (t, t + 256, ...).  Columns: F = 50176, the net's own (49 groups
per thread: the four-deep main loop and its remainder), F = 12544 against pcg_logit_head_fwd, F = 2052 (513 groups: one full trip and
one group) and F = 4 in two slabs (the empty slab).  Slab counts 1, 2, 3 (a shorter last slab), 4, 16 and 0.

Tolerances.  Logits on a 1/4 grid: every product is a multiple of 1/16 and every partial sum is below 2^18, so each is exact in fp32 and
the logit must EQUAL the float64 dot product.  prob: within 2^-22 of the float64 sigmoid (three roundings of a value <= 1 at expf's
documented accuracy, doubled).  loss, dlogit, db: against the float64 formulas evaluated on the kernel's OWN published prob -- the
reference's fp32 loss is itself that function of the rounded d; near d -> 1 the rounding of d moves log(1 - d + eps) by percents, which
is the reference's behaviour, not an error -- rtol 1e-5 (atol 1e-30) elementwise for dlogit and 1e-5 * mean|term| + 2^-23 for the two
sums (about ten fp32 roundings and logf, times ten).  Realistic rows against float64 all the way by the project's rule of §3.18: rtol
1e-4, atol 2e-5 * max|reference|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
EPS = 1e-6
F_NET, F_TWIN, F_ODD = 50176, 12544, 2052
MODES = pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
ROWS = pytest.mark.parametrize("R,mode_g", [(2, False), (6, False), (8, False), (1, True), (3, True), (4, True)])
Z_VALUES = (0.0, 0.5, -0.5, 2.0, -2.0, 6.0, -6.0, 10.0, -10.0, 14.0, -14.0, 17.0, -17.0, 20.0, -20.0, 40.0, -40.0, 100.0, -100.0)


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    return pcgan_amd.ops


class _Runner:
    """`launches` run eagerly, or captured once and replayed; every call refills `outs` with the sentinel first.  The inputs are device
    tensors the caller may rewrite in place between calls."""

    def __init__(self, launches, outs, graphed):
        from pcgan_amd import nn as N
        self.launches, self.outs, self.graph = launches, outs, None
        if graphed:
            cap = N._HipGraphCapture(torch.device(DEV), tick=False)
            cap.warmup(launches, 1, None)
            self._fill()
            torch.cuda.synchronize()
            cap.begin()
            try:
                launches()
            finally:
                self.graph = cap.end()
            torch.cuda.synchronize()
            assert all(bool((t == SENTINEL).all()) for t in outs), "captured, not run"

    def _fill(self):
        for t in self.outs:
            t.fill_(SENTINEL)

    def __call__(self):
        self._fill()
        if self.graph is not None:
            self.graph.replay()
        else:
            self.launches()
        torch.cuda.synchronize()


class _Head:
    """One head configuration on device buffers: a [R, F], w [F], bias [1] are rewritten in place by the tests."""

    def __init__(self, ops, R, F, mode_g, slabs, graphed, ws=None):
        self.R, self.F, self.mode_g = R, F, mode_g
        self.a, self.w, self.bias = torch.zeros(R, F, device=DEV), torch.zeros(F, device=DEV), torch.zeros(1, device=DEV)
        self.ws = ws if ws is not None else ops.prob_head_workspace(R, torch.device(DEV), slabs)
        self.logits, self.prob, self.dlogit = (torch.empty(R, device=DEV) for _ in range(3))
        self.loss, self.db = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
        self.run = _Runner(lambda: ops.prob_head_fwd(self.a, self.w, self.bias, mode_g=mode_g, eps=EPS, slabs=slabs, logits=self.logits,
                                                     prob=self.prob, loss=self.loss, dlogit=self.dlogit, db=self.db, ws=self.ws),
                           [self.logits, self.prob, self.dlogit, self.loss, self.db], graphed)

    def __call__(self, a, w, bias):
        self.a.copy_(a); self.w.copy_(w); self.bias.copy_(bias)
        self.run()
        assert not self.ws.any(), "the workspace is left zero"
        return {k: getattr(self, k).cpu().double().numpy() for k in ("logits", "prob", "loss", "dlogit", "db")}


def _quarter_grid(shape, gen):
    return torch.randint(-8, 9, shape, generator=gen).float() / 4.0              # [-2, 2] on a 1/4 grid: exact zeros and negatives


def _from_prob(d, mode_g):
    """float64: (loss, its terms, dlogit, db) as functions of the probabilities d."""
    d = np.asarray(d, np.float64)
    R = d.shape[0]
    half = R if mode_g else R // 2
    fake = np.arange(R) >= half
    u = np.where(fake, (1.0 - d) + EPS, d + EPS)
    logs = np.log(u)
    terms = logs if mode_g else logs[:half] + logs[half:]
    dlogit = np.where(fake, 1.0, -1.0) / half * d * (1.0 - d) / u
    return -terms.sum() / half, terms, dlogit, dlogit.sum()


def _check_from_own_prob(got, mode_g, what):
    loss, terms, dlogit, db = _from_prob(got["prob"], mode_g)
    tol_l, tol_b = 1e-5 * np.abs(terms).mean() + 2.0 ** -23, 1e-5 * np.abs(dlogit).mean() + 2.0 ** -23
    print(f"{what}: loss {got['loss'][0]:.9g} (float64 of own prob {loss:.9g}, tol {tol_l:.2e}), db error {abs(got['db'][0] - db):.2e} "
          f"(tol {tol_b:.2e}), dlogit worst rel {np.max(np.abs(got['dlogit'] - dlogit) / np.maximum(np.abs(dlogit), 1e-300)):.2e}")
    np.testing.assert_allclose(got["dlogit"], dlogit, rtol=1e-5, atol=1e-30, err_msg=what + " dlogit")
    assert abs(got["loss"][0] - loss) <= tol_l, (what, "loss", got["loss"][0], loss, tol_l)
    assert abs(got["db"][0] - db) <= tol_b, (what, "db", got["db"][0], db, tol_b)


def _close(got, want64, what):
    want64 = np.asarray(want64, np.float64)
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=2e-5 * float(np.abs(want64).max()), err_msg=what)


# ---- logits, exact -------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("F", [F_NET, F_TWIN])
@ROWS
def test_logits_on_a_quarter_grid_equal_the_float64_dot_product_for_every_slab_count(ops, R, mode_g, F, graphed):
    gen = torch.Generator().manual_seed(40 + R)
    a, w, bias = _quarter_grid((R, F), gen), _quarter_grid((F,), gen), torch.tensor([-1.25])
    want = (a.double() @ w.double() + float(bias)).numpy()
    assert np.abs(want).max() < 2.0 ** 18
    for slabs in (1, 2, 3, 4, 0):
        got = _Head(ops, R, F, mode_g, slabs, graphed)(a, w, bias)
        assert np.array_equal(got["logits"], want), (F, slabs, np.abs(got["logits"] - want).max())
        assert np.isfinite(got["loss"]).all() and np.isfinite(got["dlogit"]).all()
    if F == F_TWIN:
        twin = ops.logit_head_fwd(a.to(DEV), w.to(DEV), bias.to(DEV), mode_g=mode_g)[0]
        assert np.array_equal(twin.cpu().double().numpy(), want)


@MODES
def test_an_empty_slab_contributes_plus_zero(ops, graphed):
    a, w, bias = torch.tensor([[0.5, -1.0, 2.0, 0.25], [-2.0, 1.0, 0.0, 1.5]]), torch.tensor([1.0, 0.5, -0.25, 2.0]), torch.tensor([0.75])
    want = (a.double() @ w.double() + 0.75).numpy()
    for slabs in (1, 2, 16):                                                      # F = 4 is one group: every slab but the first is empty
        got = _Head(ops, 2, 4, False, slabs, graphed)(a, w, bias)
        assert np.array_equal(got["logits"], want), slabs
        assert not np.signbit(_Head(ops, 2, 4, False, slabs, graphed)(a * 0, w, bias * 0)["logits"]).any(), "+0, not -0"


# ---- loss and gradient on steered logits ---------------------------------------------------------------------------------------------------
@MODES
@ROWS
def test_loss_and_gradient_on_steered_logits_follow_the_kernels_own_probabilities(ops, R, mode_g, graphed):
    """w is one-hot at column 0 and a[r][0] = z_r, so the logit is exactly z_r.  Call j gives the real rows the values j * half + b and
    the fake rows (mode D) the same walk shifted by 9: every value of Z_VALUES is met as a real and as a fake row."""
    F = F_ODD
    head = _Head(ops, R, F, mode_g, 2, graphed)
    gen = torch.Generator().manual_seed(50 + R)
    w = torch.zeros(F); w[0] = 1.0
    half = R if mode_g else R // 2
    n = len(Z_VALUES)
    for j in range((n + half - 1) // half):
        z = [Z_VALUES[(j * half + b) % n] for b in range(half)] + [Z_VALUES[(j * half + b + 9) % n] for b in range(R - half)]
        a = torch.randn(R, F, generator=gen)
        a[:, 0] = torch.tensor(z)
        got = head(a, w, torch.zeros(1))
        z64 = np.asarray(z, np.float64)
        assert np.array_equal(got["logits"], z64), (got["logits"], z)
        with np.errstate(over="ignore"):
            sig = 1.0 / (1.0 + np.exp(-z64))
        assert np.abs(got["prob"] - sig).max() <= 2.0 ** -22, (z, got["prob"] - sig)
        for k in ("prob", "loss", "dlogit", "db"):
            assert np.isfinite(got[k]).all(), (k, z, got[k])
        _check_from_own_prob(got, mode_g, f"R {R} call {j}")
        for i, zi in enumerate(z):
            if abs(zi) == 100.0:
                assert got["prob"][i] == (1.0 if zi > 0 else 0.0) and got["dlogit"][i] == 0.0, (zi, got["prob"][i], got["dlogit"][i])


# ---- realistic rows ------------------------------------------------------------------------------------------------------------------------------
def _realistic(R, F, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(R, F, generator=gen)
    a = torch.where(a > 0, a, 0.2 * a)                                           # through a LeakyReLU, as D's last activation is
    w = torch.randn(F, generator=gen) / F ** 0.5
    bias = torch.tensor([0.125])
    z = a.double() @ w.double() + 0.125
    assert float(z.abs().max()) < 4.0
    return a, w, bias, z.numpy()


@MODES
@ROWS
def test_realistic_rows_against_float64_and_the_logit_head_bit_for_bit(ops, R, mode_g, graphed):
    a, w, bias, z = _realistic(R, F_NET, 60 + R)
    d = 1.0 / (1.0 + np.exp(-z))
    loss, _, dlogit, db = _from_prob(d, mode_g)
    first = None
    for slabs in (1, 3, 16, 0):
        got = _Head(ops, R, F_NET, mode_g, slabs, graphed)(a, w, bias)
        _close(got["logits"], z, "logits"); _close(got["prob"], d, "prob"); _close(got["loss"][0], loss, "loss")
        _close(got["dlogit"], dlogit, "dlogit")
        np.testing.assert_allclose(got["db"][0], db, rtol=1e-4, atol=2e-5 * np.abs(dlogit).max(), err_msg="db")
        _check_from_own_prob(got, mode_g, f"slabs {slabs}")
        if slabs == 1:
            first = got
            twin = ops.logit_head_fwd(a.to(DEV), w.to(DEV), bias.to(DEV), mode_g=mode_g)[0].cpu().double().numpy()
            assert np.array_equal(got["logits"], twin), "slabs = 1 is pcg_logit_head_fwd's sum order"
            sig = ops.act_fwd(torch.tensor(got["logits"], dtype=torch.float32, device=DEV), ops.ACT_SIGMOID).cpu().double().numpy()
            assert np.array_equal(got["prob"], sig), "the head and pcg_act_fwd publish the same probability for the same logit"
    again = _Head(ops, R, F_NET, mode_g, 1, graphed)(a, w, bias)
    assert all(np.array_equal(first[k], again[k]) for k in first), "deterministic"


# ---- the loss op ---------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("R,mode_g,F", [(2, False, F_ODD), (6, False, F_ODD), (8, False, F_ODD), (1, True, F_ODD), (3, True, F_ODD),
                                        (4, True, F_ODD), (600, False, 8), (301, True, 8)])
def test_loss_op_returns_the_heads_loss_bit_for_bit_and_its_gradient_through_the_sigmoid(ops, R, mode_g, F, graphed):
    a, w, bias, _ = _realistic(R, F, 70 + R)
    head = _Head(ops, R, F, mode_g, 2, graphed)
    got = head(a, w, bias)
    _check_from_own_prob(got, mode_g, f"R {R}")
    loss, dp, dl = torch.empty(1, device=DEV), [None], torch.empty(R, device=DEV)

    def launches():
        _, dp[0] = ops.log_eps_loss_fwd_bwd(head.prob, mode_g, EPS, loss_out=loss)
        ops.act_bwd(dp[0], head.prob, ops.ACT_SIGMOID, out=dl)

    run = _Runner(launches, [loss, dl], graphed)
    run()
    assert float(loss.cpu()) == got["loss"][0], (float(loss.cpu()), got["loss"][0])
    _close(dl.cpu().numpy(), got["dlogit"], "dp through act_bwd")
    # the cotangent, and the loss alone / the gradient alone
    g = torch.tensor([-2.5], device=DEV)
    only_loss, none = ops.log_eps_loss_fwd_bwd(head.prob, mode_g, EPS, need_grad=False)
    nol, scaled = ops.log_eps_loss_fwd_bwd(head.prob, mode_g, EPS, need_loss=False, grad_out=g)
    torch.cuda.synchronize()
    assert none is None and nol is None and float(only_loss.cpu()) == got["loss"][0]
    assert torch.equal(scaled, dp[0] * -2.5)


# ---- the workspace -------------------------------------------------------------------------------------------------------------------------------
@MODES
def test_two_calls_back_to_back_on_one_workspace(ops, graphed):
    ws = ops.prob_head_workspace(8, torch.device(DEV), 4)
    a1, w1, b1, _ = _realistic(8, F_ODD, 81)
    a2, w2, b2, _ = _realistic(6, F_ODD, 82)
    first, second = _Head(ops, 8, F_ODD, False, 4, graphed, ws=ws), _Head(ops, 6, F_ODD, True, 3, graphed, ws=ws)
    r1, r2 = first(a1, w1, b1), second(a2, w2, b2)                                # each asserts that ws is all zero afterwards
    r1b = first(a1, w1, b1)
    assert all(np.array_equal(r1[k], r1b[k]) for k in r1)
    fresh1, fresh2 = _Head(ops, 8, F_ODD, False, 4, graphed)(a1, w1, b1), _Head(ops, 6, F_ODD, True, 3, graphed)(a2, w2, b2)
    assert all(np.array_equal(r1[k], fresh1[k]) for k in r1) and all(np.array_equal(r2[k], fresh2[k]) for k in r2)
    from pcgan_amd import PcgError
    with pytest.raises(PcgError, match="workspace"):
        ops.prob_head_fwd(first.a, first.w, first.bias, slabs=8, ws=ws)           # 8 rows x 8 slabs do not fit a workspace made for 4
