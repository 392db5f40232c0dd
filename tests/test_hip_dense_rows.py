"""GPU: the three whole-batch dense forms of csrc/dense_rows.hip (pcg_dense_rows_fwd / _dgrad / _wgrad) against float64 numpy, over
R in {2, 32, 64, 128} and every Linear shape of simple_gan/mnist/mnist_gan.py (the two nets hold eight Linear layers; the ninth
Linear call of an iteration, D's first layer on the second of its two batches, has the shape of the eighth); refusals; bitwise
repeatability.

Bound of every comparison: relative L2 error against float64 <= max(FLOOR, 3 x the relative L2 error of the same quantity computed
by torch in fp32 on the CPU).  The factor 3: another summation order may land anywhere in the same noise.  FLOOR = 4e-6: the fp32
matrix instruction is a k-ordered fmaf chain whose error is about 1.5e-7 * sum|a b|, and for zero-mean operands
sum|a b| / |sum a b| is about 0.64 sqrt(K) <= 20.5 at K = 1024, so an output column carries up to 3.1e-6 of relative error where a
blocked CPU summation carries less; BatchNorm divides by the column's own scale, so the relative error passes through it.  The
bound never looks at the HIP result.  Figures are printed before they are asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 4e-6
SHAPES = [(100, 128), (128, 256), (256, 512), (512, 1024), (1024, 784), (784, 512), (512, 256), (256, 1)]   # (in, out): G's five, D's three
ROWS = [2, 32, 64, 128]
ACTS = {"none": 0, "lrelu": 2, "tanh": 3, "sigmoid": 4}
SLOPE = 0.2


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd.ops


def _act(v, act):
    if act == "lrelu":
        return np.where(v > 0, v, SLOPE * v)
    if act == "tanh":
        return np.tanh(v)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    return v


def _act_t(v, act):
    if act == "lrelu":
        return torch.nn.functional.leaky_relu(v, SLOPE)
    if act == "tanh":
        return torch.tanh(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    return v


def _dact_from_out(y, act):
    if act == "lrelu":
        return np.where(y > 0, 1.0, SLOPE)
    if act == "tanh":
        return 1.0 - y * y
    if act == "sigmoid":
        return y * (1.0 - y)
    return np.ones_like(y)


def _rel(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _check(what, hip, ref64, ref32):
    got, yard = _rel(hip.detach().cpu().double().numpy(), ref64), _rel(ref32.double().numpy(), ref64)
    bound = max(FLOOR, 3.0 * yard)
    print(f"{what}: hip-vs-f64 {got:.2e}  fp32cpu-vs-f64 {yard:.2e}  bound {bound:.2e}")
    assert np.isfinite(got) and got <= bound, f"{what}: {got:.3e} > {bound:.3e}"


def _data(R, I, O, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (R, I)).astype(np.float32)
    w = (rs.uniform(-1, 1, (O, I)) / np.sqrt(I)).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, O).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_against_float64(ops, R, shape):
    I, O = shape
    x, w, b = _data(R, I, O, 7 * R + I + O)
    rs = np.random.RandomState(R + O)
    gamma, beta = rs.uniform(0.5, 1.5, O).astype(np.float32), rs.uniform(-0.5, 0.5, O).astype(np.float32)
    rm0, rv0 = rs.normal(0, 0.3, O).astype(np.float32), rs.uniform(0.5, 2.0, O).astype(np.float32)
    z64 = x.astype(np.float64) @ w.astype(np.float64).T + b
    tx, tw, tb = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)
    z32 = torch.nn.functional.linear(tx, tw, tb)
    dx, dw, db = tx.to(DEV), tw.to(DEV), tb.to(DEV)
    for an, act in ACTS.items():
        y = ops.dense_rows_fwd(dx, dw, db, act, SLOPE)
        _check(f"fwd R{R} {I}->{O} {an}", y, _act(z64, an), _act_t(z32, an))
        for eps in (0.8, 1e-5):
            # training mode
            mean, var = z64.mean(0), z64.var(0)
            xh = (z64 - mean) / np.sqrt(var + eps)
            m32, v32 = z32.mean(0), z32.var(0, unbiased=False)
            xh32 = (z32 - m32) / torch.sqrt(v32 + eps)
            g_rm, g_rv = torch.from_numpy(rm0).to(DEV), torch.from_numpy(rv0).to(DEV)
            nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
            bn = ops.DenseBN(torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV), g_rm, g_rv, nbt, eps, 0.1, True)
            y = ops.dense_rows_fwd(dx, dw, db, act, SLOPE, bn)
            tag = f"fwd+bn(train,{eps:g}) R{R} {I}->{O} {an}"
            _check(tag + " y", y, _act(xh * gamma + beta, an), _act_t(xh32 * torch.from_numpy(gamma) + torch.from_numpy(beta), an))
            _check(tag + " xhat", bn.xhat, xh, xh32)
            _check(tag + " mean", bn.save_mean, mean, m32)
            _check(tag + " invstd", bn.save_invstd, 1 / np.sqrt(var + eps), 1 / torch.sqrt(v32 + eps))
            _check(tag + " running_mean", g_rm, 0.9 * rm0 + 0.1 * mean, 0.9 * torch.from_numpy(rm0) + 0.1 * m32)
            _check(tag + " running_var", g_rv, 0.9 * rv0 + 0.1 * z64.var(0, ddof=1), 0.9 * torch.from_numpy(rv0) + 0.1 * z32.var(0, unbiased=True))
            assert int(nbt.item()) == 6, "num_batches_tracked"
            # evaluation mode: the running statistics, buffers untouched
            g_rm, g_rv = torch.from_numpy(rm0).to(DEV), torch.from_numpy(rv0).to(DEV)
            nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
            bn = ops.DenseBN(torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV), g_rm, g_rv, nbt, eps, 0.1, False)
            y = ops.dense_rows_fwd(dx, dw, db, act, SLOPE, bn)
            e64 = (z64 - rm0) / np.sqrt(rv0.astype(np.float64) + eps) * gamma + beta
            e32 = (z32 - torch.from_numpy(rm0)) / torch.sqrt(torch.from_numpy(rv0) + eps) * torch.from_numpy(gamma) + torch.from_numpy(beta)
            _check(f"fwd+bn(eval,{eps:g}) R{R} {I}->{O} {an}", y, _act(e64, an), _act_t(e32, an))
            assert int(nbt.item()) == 5 and np.array_equal(g_rm.cpu().numpy(), rm0) and np.array_equal(g_rv.cpu().numpy(), rv0)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grad_input_against_float64(ops, R, shape):
    """dx = dz W with the activation derivative and BatchNorm backward of the layer below (whose width is this layer's `in`)."""
    I, O = shape
    rs = np.random.RandomState(11 * R + I + 3 * O)
    dz = rs.normal(0, 1, (R, O)).astype(np.float32)
    w = (rs.uniform(-1, 1, (O, I)) / np.sqrt(O)).astype(np.float32)
    pre = rs.normal(0, 1, (R, I))
    gamma = rs.uniform(0.5, 1.5, I).astype(np.float32)
    invstd = rs.uniform(0.5, 1.5, I).astype(np.float32)
    # x-hat as the reference's BatchNorm1d(., 0.8) leaves it: zero-mean columns (at eps 1e-5 and R = 2 it is +-1 and dz is exactly 0)
    xh = ((pre - pre.mean(0)) / np.sqrt(pre.var(0) + 0.8)).astype(np.float32)
    g64 = dz.astype(np.float64) @ w.astype(np.float64)
    g32 = torch.from_numpy(dz) @ torch.from_numpy(w)
    ddz, dw = torch.from_numpy(dz).to(DEV), torch.from_numpy(w).to(DEV)
    _check(f"dgrad plain R{R} {O}->{I}", ops.dense_rows_dgrad(ddz, dw), g64, g32)
    for an, act in ACTS.items():
        yb = _act(pre, an).astype(np.float32)
        d64 = g64 * _dact_from_out(yb.astype(np.float64), an)
        d32 = g32 * torch.from_numpy(_dact_from_out(yb, an).astype(np.float32))
        dyb = torch.from_numpy(yb).to(DEV)
        if act:
            _check(f"dgrad act R{R} {O}->{I} {an}", ops.dense_rows_dgrad(ddz, dw, act, SLOPE, dyb), d64, d32)
        # BatchNorm backward below
        x64 = xh.astype(np.float64)
        dbeta, dgamma = d64.sum(0), (d64 * x64).sum(0)
        dzb = gamma * invstd.astype(np.float64) * (d64 - dbeta / R - x64 * dgamma / R)
        txh = torch.from_numpy(xh)
        dbeta32, dgamma32 = d32.sum(0), (d32 * txh).sum(0)
        dzb32 = torch.from_numpy(gamma * invstd) * (d32 - dbeta32 / R - txh * dgamma32 / R)
        gg = torch.full((I,), 7.0, device=DEV); gb = torch.full((I,), -3.0, device=DEV)
        out = ops.dense_rows_dgrad(ddz, dw, act, SLOPE, dyb if act else None,
                                   (torch.from_numpy(xh).to(DEV), torch.from_numpy(gamma).to(DEV), torch.from_numpy(invstd).to(DEV), gg, gb, False))
        tag = f"dgrad+bnbwd R{R} {O}->{I} {an}"
        _check(tag + " dz", out, dzb, dzb32)
        _check(tag + " dgamma", gg, dgamma, dgamma32)
        _check(tag + " dbeta", gb, dbeta, dbeta32)
    # accumulate into dgamma / dbeta
    gg = torch.full((I,), 7.0, device=DEV); gb = torch.full((I,), -3.0, device=DEV)
    ops.dense_rows_dgrad(ddz, dw, 0, 0.0, None, (torch.from_numpy(xh).to(DEV), torch.from_numpy(gamma).to(DEV), torch.from_numpy(invstd).to(DEV), gg, gb, True))
    x64 = xh.astype(np.float64)
    _check(f"dgrad+bnbwd accumulate R{R} dgamma", gg, 7.0 + (g64 * x64).sum(0), 7.0 + (g32 * torch.from_numpy(xh)).sum(0))
    _check(f"dgrad+bnbwd accumulate R{R} dbeta", gb, -3.0 + g64.sum(0), -3.0 + g32.sum(0))


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weight_gradient_against_float64(ops, R, shape):
    I, O = shape
    rs = np.random.RandomState(13 * R + 5 * I + O)
    dz, x = rs.normal(0, 1, (R, O)).astype(np.float32), rs.normal(0, 1, (R, I)).astype(np.float32)
    w64, b64 = dz.astype(np.float64).T @ x.astype(np.float64), dz.astype(np.float64).sum(0)
    w32, b32 = torch.from_numpy(dz).T @ torch.from_numpy(x), torch.from_numpy(dz).sum(0)
    ddz, dx = torch.from_numpy(dz).to(DEV), torch.from_numpy(x).to(DEV)
    dW = torch.full((O, I), 9.0, device=DEV); db = torch.full((O,), 9.0, device=DEV)
    ops.dense_rows_wgrad(ddz, dx, dW, db, accumulate=False)
    _check(f"wgrad R{R} {I}->{O} dW", dW, w64, w32)
    _check(f"wgrad R{R} {I}->{O} db", db, b64, b32)
    dW = torch.full((O, I), 0.5, device=DEV); db = torch.full((O,), 0.5, device=DEV)
    ops.dense_rows_wgrad(ddz, dx, dW, db, accumulate=True)
    _check(f"wgrad accumulate R{R} {I}->{O} dW", dW, 0.5 + w64, 0.5 + w32)
    _check(f"wgrad accumulate R{R} {I}->{O} db", db, 0.5 + b64, 0.5 + b32)
    dW = torch.full((O, I), 9.0, device=DEV)
    ops.dense_rows_wgrad(ddz, dx, dW, None)
    _check(f"wgrad no-bias R{R} {I}->{O} dW", dW, w64, w32)


def test_unsupported_shapes_are_refused_not_run(ops):
    import pcgan_amd
    E = pcgan_amd.PcgError
    t = lambda *s: torch.ones(s, device=DEV)
    sentinel = lambda *s: torch.full(s, -77.0, device=DEV)

    def bn(O, training=True):
        return ops.DenseBN(t(O), t(O), t(O), t(O), torch.zeros((), dtype=torch.int64, device=DEV), 0.8, 0.1, training)

    out = sentinel(129, 16)
    with pytest.raises(E, match="129 rows"):
        ops.dense_rows_fwd(t(129, 16), t(16, 16), t(16), out=out)
    assert bool((out == -77.0).all())
    out = sentinel(1, 16)
    b1 = bn(16)
    with pytest.raises(E, match="more than 1 row"):
        ops.dense_rows_fwd(t(1, 16), t(16, 16), t(16), bn=b1, out=out)
    assert bool((out == -77.0).all()) and int(b1.num_batches_tracked.item()) == 0 and bool((b1.running_mean == 1).all())
    ops.dense_rows_fwd(t(1, 16), t(16, 16), t(16), bn=bn(16, training=False), out=out)      # evaluation mode takes one row, like torch
    assert bool((out != -77.0).all())
    out = sentinel(8, 16)
    with pytest.raises(E, match="multiple of 4"):
        ops.dense_rows_fwd(t(8, 102), t(16, 102), t(16), out=out)
    with pytest.raises(E, match="unknown activation"):
        ops.dense_rows_fwd(t(8, 16), t(16, 16), t(16), act=7, out=out)
    with pytest.raises(E, match="16-byte aligned"):
        ops.dense_rows_fwd(t(8 * 16 + 1)[1:].view(8, 16), t(16, 16), t(16), out=out)
    assert bool((out == -77.0).all())
    out = sentinel(129, 16)
    with pytest.raises(E, match="129 rows"):
        ops.dense_rows_dgrad(t(129, 16), t(16, 16), out=out)
    with pytest.raises(E, match="needs the layer's output"):
        ops.dense_rows_dgrad(t(8, 16), t(16, 16), 2, 0.2, None, out=sentinel(8, 16))
    o1 = sentinel(1, 16)
    with pytest.raises(E, match="more than 1 row"):
        ops.dense_rows_dgrad(t(1, 16), t(16, 16), 0, 0.0, None, (t(1, 16), t(16), t(16), t(16), t(16), False), out=o1)
    assert bool((out == -77.0).all()) and bool((o1 == -77.0).all())
    dW = sentinel(16, 16)
    with pytest.raises(E, match="129 rows"):
        ops.dense_rows_wgrad(t(129, 16), t(129, 16), dW)
    assert bool((dW == -77.0).all())
    with pytest.raises(E, match="no CPU path"):
        ops.dense_rows_fwd(torch.ones(8, 16), torch.ones(16, 16))


@pytest.mark.parametrize("R", [32, 64, 128])
def test_every_form_is_bitwise_repeatable(ops, R):
    for I, O in ((100, 128), (1024, 784), (256, 1)):
        x, w, b = _data(R, I, O, R + I)
        dx, dw, db = (torch.from_numpy(a).to(DEV) for a in (x, w, b))
        dz = torch.from_numpy(np.random.RandomState(R).normal(0, 1, (R, O)).astype(np.float32)).to(DEV)
        runs = []
        for _ in range(2):
            bn = ops.DenseBN(torch.ones(O, device=DEV), torch.zeros(O, device=DEV), torch.zeros(O, device=DEV), torch.ones(O, device=DEV),
                             torch.zeros((), dtype=torch.int64, device=DEV), 0.8, 0.1, True)
            y = ops.dense_rows_fwd(dx, dw, db, 2, 0.2, bn)
            gg, gb = torch.empty(I, device=DEV), torch.empty(I, device=DEV)
            xh_below = torch.tanh(dx)
            d = ops.dense_rows_dgrad(dz, dw, 3, 0.0, xh_below, (xh_below, torch.ones(I, device=DEV), torch.ones(I, device=DEV), gg, gb, False))
            dW, dB = torch.empty(O, I, device=DEV), torch.empty(O, device=DEV)
            ops.dense_rows_wgrad(dz, dx, dW, dB)
            runs.append((y, bn.xhat, bn.save_mean, bn.save_invstd, bn.running_mean, bn.running_var, d, gg, gb, dW, dB))
        for a, c in zip(*runs):
            assert torch.equal(a, c)
