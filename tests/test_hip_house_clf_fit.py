"""GPU: the house-sales classifier fit on whole-batch dense launches -- pcg_dense_rows_fwd_post / _dgrad_post,
pcg_ce_weighted_tally, pcg_house_clf_batch(_counter), house.ClassifierFit and house.train_classifier(fused=True).

Bounds.  Kernel forms against float64 (tests/house_clf_restate.py): relative L2 error <= max(4e-6, 3 x the relative L2 error of the
same quantity computed by torch in fp32 on the CPU) -- the bound and its reasoning are those of tests/test_hip_dense_rows.py (K <= 1024
there, K <= 256 here) and never look at the HIP result.  At R = 2 the stage is run with eps = 0.8 instead of the classifier's 1e-5:
with two rows x-hat is +-1/sqrt(1 + eps/var) and the BatchNorm backward is the difference dn_1 - dn_2 times eps/(var + eps) / 2, a
quantity that fp32 cancels away at eps 1e-5 in ANY summation order (tests/test_hip_dense_rows.py makes the same choice for its
x-hat).  Reference steps: the pass conditions of tests/test_hip_house.py::test_classifier_pretraining_steps_match_reference.
Figures are printed before they are asserted (pytest -s shows them)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import house_clf_restate as RS  # noqa: E402
from oracle import house_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 4e-6
STAGES = [(17, 256), (256, 256), (256, 128), (128, 64)]      # (in, out) of the four Linear -> LeakyReLU -> BatchNorm1d (-> Dropout) stages
ROWS = [2, 48, 73, 128]                                       # BatchNorm's minimum; the golden batch; the reference split's tail; the full batch
SENT = -77.0


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import house  # noqa: F401
    pcgan_amd.load()
    return pcgan_amd


@pytest.fixture(scope="module")
def ops(pcg):
    return pcg.ops


def _dev(t):
    return t.to(DEV).contiguous()


def _rel(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _check(what, hip, ref64, ref32):
    got, yard = _rel(hip.detach().cpu().double().numpy(), ref64.numpy()), _rel(ref32.double().numpy(), ref64.numpy())
    bound = max(FLOOR, 3.0 * yard)
    print(f"{what}: hip-vs-f64 {got:.2e}  fp32cpu-vs-f64 {yard:.2e}  bound {bound:.2e}")
    assert np.isfinite(got) and got <= bound, f"{what}: {got:.3e} > {bound:.3e}"


def _padded(rows, cols, extra=3):
    """A [rows, cols] view at the head of a sentinel-filled buffer with `extra` more rows: (view, the rows behind it)."""
    buf = torch.full((rows + extra, cols), SENT, device=DEV)
    return buf[:rows], buf[rows:]


def _stage_data(R, I, O, seed):
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32))      # noqa: E731
    return dict(x=t(rs.normal(0, 1, (R, I))), W=t(rs.uniform(-1, 1, (O, I)) / np.sqrt(I)), b=t(rs.uniform(-0.5, 0.5, O)),
                gamma=t(rs.uniform(0.5, 1.5, O)), beta=t(rs.uniform(-0.5, 0.5, O)), rm=t(rs.normal(0, 0.3, O)), rv=t(rs.uniform(0.5, 2.0, O)),
                mask=t(rs.random_sample((R, O)) < 0.7))


# ---- 1. kernel forms against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("shape", STAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_post_against_float64(ops, R, shape):
    I, O = shape
    d = _stage_data(R, I, O, 7 * R + I + O)
    eps = 0.8 if R == 2 else RS.EPS
    for mask, p in ((None, 0.0), (d["mask"], 0.3)):
        r64 = RS.stage_fwd(*(d[k].double() for k in ("x", "W", "b", "gamma", "beta")), mask, p, eps=eps)
        r32 = RS.stage_fwd(*(d[k] for k in ("x", "W", "b", "gamma", "beta")), mask, p, eps=eps)
        runs = []
        for _ in range(2):
            y, y_tail = _padded(R, O)
            a, a_tail = _padded(R, O)
            vec = torch.full((4, O + 8), SENT, device=DEV)                       # save_mean, save_invstd, running_mean, running_var (+ 8 behind)
            vec[2, :O], vec[3, :O] = _dev(d["rm"]), _dev(d["rv"])
            nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
            bn = ops.DenseBN(_dev(d["gamma"]), _dev(d["beta"]), vec[2, :O], vec[3, :O], nbt, eps, RS.MOMENTUM, True, vec[0, :O], vec[1, :O])
            ops.dense_rows_fwd_post(_dev(d["x"]), _dev(d["W"]), _dev(d["b"]), bn, ops.ACT_LRELU, RS.SLOPE, mask=None if mask is None else _dev(mask),
                                    p=p, a=a, out=y)
            assert bool((y_tail == SENT).all()) and bool((a_tail == SENT).all()) and bool((vec[:, O:] == SENT).all()), "wrote outside its outputs"
            assert int(nbt.item()) == 6, "num_batches_tracked"
            runs.append((y.clone(), a.clone(), vec.clone()))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), "two runs differ"
        y, a, vec = runs[0]
        tag = f"fwd_post R{R} {I}->{O} {'mask' if mask is not None else 'no mask'}"
        _check(tag + " y", y, r64[0], r32[0])
        _check(tag + " a", a, r64[1], r32[1])
        _check(tag + " mean", vec[0, :O], r64[2], r32[2])
        _check(tag + " invstd", vec[1, :O], r64[3], r32[3])
        _check(tag + " running_mean", vec[2, :O], 0.9 * d["rm"].double() + 0.1 * r64[2], 0.9 * d["rm"] + 0.1 * r32[2])
        _check(tag + " running_var", vec[3, :O], 0.9 * d["rv"].double() + 0.1 * r64[4], 0.9 * d["rv"] + 0.1 * r32[4])


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("shape", STAGES + [(64, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_grad_input_post_against_float64(ops, R, shape):
    """dz [R][O] through W [O][I] and the whole backward of a stage of width I below it ((64, 4): the step's first, below the logits)."""
    I, O = shape
    rs = np.random.RandomState(11 * R + I + 3 * O)
    t = lambda a: torch.from_numpy(a.astype(np.float32))      # noqa: E731
    dz, W = t(rs.normal(0, 1, (R, O))), t(rs.uniform(-1, 1, (O, I)) / np.sqrt(O))
    pre = rs.normal(0, 1, (R, I))
    a = t(np.where(pre > 0, pre, RS.SLOPE * pre))
    eps = 0.8 if R == 2 else RS.EPS
    mean = a.double().mean(0).float()
    invstd = (1.0 / torch.sqrt(a.double().var(0, unbiased=False) + eps)).float()          # as a forward would have left them
    gamma, mask = t(rs.uniform(0.5, 1.5, I)), t(rs.random_sample((R, I)) < 0.8)
    for m, p in ((None, 0.0), (mask, 0.2)):
        r64 = RS.stage_bwd(dz.double() @ W.double(), a.double(), mean.double(), invstd.double(), gamma.double(), m, p)
        r32 = RS.stage_bwd(dz @ W, a, mean, invstd, gamma, m, p)
        runs = []
        for _ in range(2):
            dx, dx_tail = _padded(R, I)
            gg = torch.full((3, I + 8), SENT, device=DEV)                        # dgamma, dbeta, db (+ 8 behind)
            ops.dense_rows_dgrad_post(_dev(dz), _dev(W), _dev(a), _dev(mean), _dev(invstd), _dev(gamma), gg[0, :I], gg[1, :I], ops.ACT_LRELU,
                                      RS.SLOPE, mask=None if m is None else _dev(m), p=p, out=dx, db=gg[2, :I])
            assert bool((dx_tail == SENT).all()) and bool((gg[:, I:] == SENT).all()), "wrote outside its outputs"
            runs.append((dx.clone(), gg.clone()))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), "two runs differ"
        dx, gg = runs[0]
        tag = f"dgrad_post R{R} {O}->{I} {'mask' if m is not None else 'no mask'}"
        _check(tag + " dx", dx, r64[0], r32[0])
        _check(tag + " dgamma", gg[0, :I], r64[1], r32[1])
        _check(tag + " dbeta", gg[1, :I], r64[2], r32[2])
        _check(tag + " db", gg[2, :I], r64[0].sum(0), r32[0].sum(0))             # the Linear's bias gradient: column sums of dx
        dx0 = torch.full((R, I), SENT, device=DEV)                               # without db: the same dx, dgamma, dbeta
        g0 = torch.full((2, I), SENT, device=DEV)
        ops.dense_rows_dgrad_post(_dev(dz), _dev(W), _dev(a), _dev(mean), _dev(invstd), _dev(gamma), g0[0], g0[1], ops.ACT_LRELU, RS.SLOPE,
                                  mask=None if m is None else _dev(m), p=p, out=dx0)
        assert torch.equal(dx0, dx) and torch.equal(g0, gg[:2, :I])
        # accumulate adds to what dgamma / dbeta hold, and leaves dx as it was
        acc = torch.stack([torch.full((I,), 7.0, device=DEV), torch.full((I,), -3.0, device=DEV), torch.full((I,), 5.0, device=DEV)])
        dx2 = ops.dense_rows_dgrad_post(_dev(dz), _dev(W), _dev(a), _dev(mean), _dev(invstd), _dev(gamma), acc[0], acc[1], ops.ACT_LRELU, RS.SLOPE,
                                        mask=None if m is None else _dev(m), p=p, accumulate=True, db=acc[2])
        assert torch.equal(dx2, dx)
        _check(tag + " dgamma accumulate", acc[0], 7.0 + r64[1], 7.0 + r32[1])
        _check(tag + " dbeta accumulate", acc[1], -3.0 + r64[2], -3.0 + r32[2])
        _check(tag + " db accumulate", acc[2], 5.0 + r64[0].sum(0), 5.0 + r32[0].sum(0))


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(pcg, ops):
    E = pcg.PcgError
    t = lambda *s: torch.ones(s, device=DEV)                  # noqa: E731
    sentinel = lambda *s: torch.full(s, SENT, device=DEV)     # noqa: E731

    def bn(O):
        return ops.DenseBN(t(O), t(O), t(O), t(O), torch.zeros((), dtype=torch.int64, device=DEV), 1e-5, 0.1, True)

    for R, text in ((1, "1 rows"), (129, "129 rows")):
        out, b = sentinel(R, 16), bn(16)
        with pytest.raises(E, match=text):
            ops.dense_rows_fwd_post(t(R, 16), t(16, 16), t(16), b, out=out)
        assert bool((out == SENT).all()) and int(b.num_batches_tracked.item()) == 0 and bool((b.running_mean == 1).all())
        out = sentinel(R, 16)
        with pytest.raises(E, match=text):
            ops.dense_rows_dgrad_post(t(R, 16), t(16, 16), t(R, 16), t(16), t(16), t(16), t(16), t(16), out=out)
        assert bool((out == SENT).all())
    out = sentinel(8, 16)
    with pytest.raises(E, match="unknown activation"):
        ops.dense_rows_fwd_post(t(8, 16), t(16, 16), t(16), bn(16), act=7, out=out)
    with pytest.raises(E, match="unknown activation"):
        ops.dense_rows_dgrad_post(t(8, 16), t(16, 16), t(8, 16), t(16), t(16), t(16), t(16), t(16), act=7, out=out)
    with pytest.raises(E, match="needs a, mean, invstd"):
        ops.dense_rows_dgrad_post(t(8, 16), t(16, 16), None, t(16), t(16), t(16), t(16), t(16), out=out)
    with pytest.raises(E, match="needs a, mean, invstd"):
        ops.dense_rows_dgrad_post(t(8, 16), t(16, 16), t(8, 16), t(16), None, t(16), t(16), t(16), out=out)
    assert bool((out == SENT).all())
    # null saved buffers of the forward: the wrapper allocates them, so straight through the C ABI
    lib = pcg.load()
    P = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)      # noqa: E731
    x, W, v, y, a = t(8, 16), t(16, 16), t(16), sentinel(8, 16), t(8, 16)
    for a_, m_, s_ in ((None, v, v), (a, None, v), (a, v, None)):
        rc = lib.pcg_dense_rows_fwd_post(P(x), P(W), P(v), 8, 16, 16, 2, 0.1, P(v), P(v), None, None, None, 1e-5, 0.1, None, 1.0, P(a_), P(m_), P(s_),
                                         P(y), None)
        assert rc != 0 and b"a, save_mean and save_invstd" in lib.pcg_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
    # the pre-activation forward keeps refusing the first layer's width
    with pytest.raises(E, match="multiple of 4"):
        ops.dense_rows_fwd(t(8, 17), t(16, 17), t(16), out=out)
    assert bool((out == SENT).all())
    with pytest.raises(E, match="dbias is the column sum"):
        ops.ce_weighted_tally(t(8, 4), torch.zeros(8, dtype=torch.int64, device=DEV), t(4), torch.zeros(3, dtype=torch.float64, device=DEV), dbias=t(4))
    with pytest.raises(E, match="ONE mean"):
        ops.ce_weighted_tally(t(8, 4), torch.zeros(8, dtype=torch.int64, device=DEV), t(4), torch.zeros(3, dtype=torch.float64, device=DEV), seg=4,
                              dlogits=sentinel(8, 4))


# ---- 3. tally -----------------------------------------------------------------------------------------------------------------
def test_tally_equals_the_loss_entry_bit_for_bit(ops):
    rs = np.random.RandomState(3)
    B, K = 48, 4
    z = _dev(torch.from_numpy(rs.normal(0, 2, (B, K)).astype(np.float32)))
    y = _dev(torch.from_numpy(rs.randint(0, K, B)))
    w = _dev(torch.tensor([0.4, 1.7, 0.9, 2.3]))
    loss, dz = ops.cross_entropy_weighted_fwd_bwd(z, y, w)
    tally = torch.zeros(3, dtype=torch.float64, device=DEV)
    dl, sl = torch.full((B, K), SENT, device=DEV), torch.full((1,), SENT, device=DEV)
    db = torch.full((K + 4,), SENT, device=DEV)
    ops.ce_weighted_tally(z, y, w, tally, dlogits=dl, seg_loss=sl, dbias=db[:K])
    assert torch.equal(sl, loss) and torch.equal(dl, dz) and bool((db[K:] == SENT).all())
    # the logits layer's bias gradient: column sums of dlogits, against float64 of the same fp32 entries; the 48 terms of a column
    # are summed as 48 partial sums folded in halves, so 6 roundings of at most 2^-24 each on terms that cancel: absolute bound on sum|.|
    want = dz.double().sum(0).cpu()
    err = (db[:K].double().cpu() - want).abs().max().item()
    bound = 6 * 2.0 ** -24 * dz.double().abs().sum(0).max().item()
    print(f"dbias {db[:K].tolist()}  float64 {want.tolist()}  err {err:.2e}  bound {bound:.2e}")
    assert err <= bound
    hits = int((z.argmax(1) == y).sum())
    assert tally.tolist() == [float(loss.item()) * B, float(hits), float(B)]
    ops.ce_weighted_tally(z, y, w, tally, seg=1000)                                          # a second call accumulates
    assert tally.tolist() == [2 * float(loss.item()) * B, 2.0 * hits, 2.0 * B]


def test_tally_segments_count_and_ties(ops):
    rs = np.random.RandomState(4)
    B, K, seg = 300, 4, 128
    z = torch.from_numpy(rs.normal(0, 2, (B, K)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, K, B))
    z[5] = torch.tensor([1.5, 0.25, 1.5, -1.0]); y[5] = 0          # two bit-identical top logits: the lower index is the prediction
    z[6] = torch.tensor([1.5, 0.25, 1.5, -1.0]); y[6] = 2          # ... so this row is wrong
    z[7] = torch.tensor([0.0, 3.0, -1.0, 3.0]); y[7] = 1
    z[8] = torch.tensor([0.0, 3.0, -1.0, 3.0]); y[8] = 3
    w = torch.tensor([0.4, 1.7, 0.9, 2.3])
    (tot, hits, n), losses = RS.ce_tally(z.double(), y, w.double(), seg)
    assert hits == int((z.argmax(1) == y).sum())               # torch.argmax: first maximum
    base = int((torch.cat([z[:5], z[9:]]).argmax(1) == torch.cat([y[:5], y[9:]])).sum())
    assert hits == base + 2
    tally = torch.zeros(3, dtype=torch.float64, device=DEV)
    sl = torch.zeros(3, device=DEV)
    ops.ce_weighted_tally(_dev(z), _dev(y), _dev(w), tally, seg=seg, seg_loss=sl)
    got = tally.tolist()
    print(f"tally {got}  float64 {(tot, hits, n)}  segment losses {sl.tolist()} vs {losses}")
    assert abs(got[0] - tot) <= 1e-6 * abs(tot) and got[1] == hits and got[2] == n
    np.testing.assert_allclose(sl.cpu().numpy(), losses, rtol=1e-6)


# ---- 4. batch counter -----------------------------------------------------------------------------------------------------------
def test_batch_launch_rows_masks_and_counter(ops):
    rs = np.random.RandomState(5)
    N, D, B = 301, 17, 73
    X = _dev(torch.from_numpy(rs.random_sample((N, D)).astype(np.float32)))
    Y = _dev(torch.from_numpy(rs.randint(0, 4, N)))
    perm = _dev(torch.from_numpy(rs.permutation(N)))
    widths, keeps = (256, 256, 128), (0.7, 0.8, 0.9)
    bufs = lambda: ((torch.empty((B, D), device=DEV), torch.empty((B,), dtype=torch.int64, device=DEV)),      # noqa: E731
                    [torch.empty((B, w), device=DEV) for w in widths])
    seed = 21
    a, b, ref = ops.DeviceRNG(seed), ops.DeviceRNG(seed), ops.DeviceRNG(seed)
    for r in (a, b, ref):
        r.rand((7,), DEV)                                      # the stream does not start at offset 0
    ctr = a.device_counter(DEV, cursor=True)
    for it in range(2):
        (x1, y1), m1 = bufs()
        a.house_clf_batch(X, Y, perm, (x1, y1), m1, keeps, counter=ctr)
        (x2, y2), m2 = bufs()
        b.house_clf_batch(X, Y, perm, (x2, y2), m2, keeps, cursor=it * B)
        rows = perm[it * B:(it + 1) * B]
        assert torch.equal(x1, X[rows]) and torch.equal(y1, Y[rows]) and torch.equal(x2, X[rows]) and torch.equal(y2, Y[rows])
        for u, v, w, k in zip(m1, m2, widths, keeps):
            assert torch.equal(u, v) and torch.equal(u, ref.bernoulli((B, w), DEV, k))
        assert ctr.tolist() == [b.offset, 0, (it + 1) * B, 0] and b.offset == ref.offset
        assert 0.0 < float(m1[0].mean()) < 1.0
    assert a.offset == 2                                       # the counter form leaves the host offset alone (rand((7,)) took 2)
    with pytest.raises(Exception, match="permutation of"):
        b.house_clf_batch(X, Y, perm, bufs()[0], bufs()[1], keeps, cursor=N - B + 1)


# ---- 5. the reference's own steps ---------------------------------------------------------------------------------------------------
def _gold(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "classifier_pretrain_house.npz")))
    rows = np.concatenate([gold[f"step{i}.rows"] for i in range(int(gold["meta.steps"]))])
    cw = torch.tensor(HR.balanced_class_weights(gold["y"][rows], 4), dtype=torch.float32)     # weights from the training split (trainer.py:53)
    return gold, cw, rows


def test_reference_steps_teacher_forced_and_free_run(pcg, golden_dir):
    H = pcg.house
    gold, cw, rows = _gold(golden_dir)
    init = {k[5:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.")}
    X, y = torch.from_numpy(gold["X"]), torch.from_numpy(gold["y"])
    steps = int(gold["meta.steps"])
    o64, o32 = HR.NNClassifier(17, 4), HR.NNClassifier(17, 4)
    o64.load_state_dict(init); o32.load_state_dict(init)
    o64 = o64.double()
    opt64 = torch.optim.AdamW(o64.parameters(), lr=1e-3, weight_decay=1e-4)
    mine = H.NNClassifier(17, 4)
    mine.load_state_dict(init)
    mine = mine.to(DEV)
    fit = H.ClassifierFit(mine, gold["X"][rows], gold["y"][rows], _dev(cw), 48, lr=1e-3, weight_decay=1e-4, graph=False)
    for i in range(steps):
        r = torch.from_numpy(gold[f"step{i}.rows"])
        masks = [torch.from_numpy(gold[f"step{i}.mask{j}"]) for j in range(3)]
        sd = {k: v.float() if v.is_floating_point() else v.clone() for k, v in o64.state_dict().items()}
        o32.load_state_dict(sd); mine.load_state_dict(sd)                       # teacher forcing: same starting point
        o32.train(); o32.zero_grad()
        l32 = F.cross_entropy(HR.classifier_forward_train(o32, X[r], masks), y[r], weight=cw)
        l32.backward()
        l64 = HR.classifier_train_step(o64, opt64, cw.double(), X[r].double(), y[r], masks)   # advances the teacher
        lm = fit.run_batch(_dev(X[r]), _dev(y[r]), [_dev(t) for t in masks]).item()
        print(f"step {i}: loss {lm:.7f}  float64 {l64:.7f}  fp32 oracle {l32.item():.7f}")
        assert abs(lm - l64) <= max(2e-5, 3 * abs(l32.item() - l64)), (i, lm, l64)
        for (n, p), (_, q32), (_, q64) in zip(mine.named_parameters(), o32.named_parameters(), o64.named_parameters()):
            truth = q64.grad
            tol = max(1e-4 * float(truth.abs().max()), 3 * float((q32.grad.double() - truth).abs().max()), 1e-8)
            err = float((p.grad.cpu().double() - truth).abs().max())
            assert err <= tol, (f"step {i} grad {n}", err, tol)
    assert fit.read_tally()[2] == 48.0 * steps
    # free run from the initial state, AdamW included
    mine.load_state_dict(init)
    for b_ in mine.modules():
        if isinstance(b_, torch.nn.BatchNorm1d):
            b_.num_batches_tracked.zero_()
    for i in range(steps):
        r = torch.from_numpy(gold[f"step{i}.rows"])
        fit.run_batch(_dev(X[r]), _dev(y[r]), [_dev(torch.from_numpy(gold[f"step{i}.mask{j}"])) for j in range(3)])
        fit.optimizer.step()
    for k, v in mine.state_dict().items():
        ref = gold[f"final.{k}"]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref)
        elif "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=2e-3, atol=2e-3, err_msg=k)
        else:
            assert float(np.abs(v.cpu().numpy() - ref).max()) <= 2.2 * 1e-3 * 3 + 1e-5, k


# ---- 6. replay equals eager -----------------------------------------------------------------------------------------------------------
def test_replays_equal_the_eager_entries(pcg):
    H, ops = pcg.house, pcg.ops
    rs = np.random.RandomState(6)
    N = 300                                                     # 128 + 128 + 44: both graphs within three steps
    X, y = rs.random_sample((N, 17)).astype(np.float32), rs.randint(0, 4, N)
    perm = torch.from_numpy(rs.permutation(N))
    cw = _dev(torch.tensor([0.5, 1.0, 1.5, 2.0]))
    torch.manual_seed(3)
    init = {k: v.clone() for k, v in H.NNClassifier(17, 4).state_dict().items()}
    states = []
    for graph in (True, False):
        model = H.NNClassifier(17, 4)
        model.load_state_dict(init)
        model = model.to(DEV)
        rng = ops.DeviceRNG(9)
        rng.rand((5,), DEV)
        fit = H.ClassifierFit(model, X, y, cw, 128, rng=rng, graph=graph)
        assert fit.steps_per_epoch == 3 and rng.offset == 2, "building the fit must not advance the stream"
        assert all(int(m.num_batches_tracked) == 0 for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d))
        fit.new_epoch(perm)
        recs = []
        for _ in range(3):
            rec = {}
            fit.step(record=rec)
            recs.append(rec)
        with pytest.raises(pcg.PcgError, match="used up"):
            fit.step()
        states.append(({k: v.clone() for k, v in model.state_dict().items()}, recs, fit.read_tally(), rng.offset))
    (sa, ra, ta, oa), (sb, rb, tb, ob) = states
    assert ta == tb and ta[2] == float(N) and oa == ob
    for u, v in zip(ra, rb):
        assert torch.equal(u["x"], v["x"]) and torch.equal(u["y"], v["y"]) and torch.equal(u["loss"], v["loss"])
        assert all(torch.equal(p, q) for p, q in zip(u["masks"], v["masks"]))
    assert torch.equal(ra[0]["x"].cpu(), torch.from_numpy(X)[perm[:128]]) and ra[2]["x"].shape[0] == 44
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        assert k.endswith("num_batches_tracked") or not torch.equal(sa[k].cpu(), init[k]), f"{k} did not move"


def test_tail_of_one_row_is_refused(pcg):
    H = pcg.house
    model = H.NNClassifier(17, 4).to(DEV)
    with pytest.raises(pcg.PcgError, match="one row"):
        H.ClassifierFit(model, np.zeros((129, 17), np.float32), np.zeros(129, np.int64), torch.ones(4, device=DEV), 128, graph=False)


# ---- 7. - 9. house.train_classifier(fused=True) -------------------------------------------------------------------------------------
def _separable(n, seed=0):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 4, size=n)
    centers = rs.random_sample((4, 17))
    return np.clip(centers[y] + 0.05 * rs.standard_normal((n, 17)), 0, 1), y


def test_same_batches_and_masks_as_the_chain(pcg):
    H = pcg.house
    X, y = _separable(150)
    hist = {}
    for fused in (True, False):
        cfg = dict(H.CONFIG, clf_epochs=1, batch_size=128, seed=5)
        model = H.train_classifier(X[:120], X[120:], y[:120], y[120:], None, cfg, device=DEV, verbose=False, fused=fused)
        hist[fused] = model.history
    print(f"fused {hist[True]}  chain {hist[False]}")
    assert len(hist[True]) == len(hist[False]) == 1
    assert abs(hist[True][0][0] - hist[False][0][0]) <= 2e-5
    assert abs(hist[True][0][1] - hist[False][0][1]) <= 1.0 / 120 + 1e-9


def test_train_classifier_fused_learns(pcg):
    H = pcg.house
    X, y = _separable(1200)
    cfg = dict(H.CONFIG, clf_epochs=6, batch_size=128, seed=1)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*op chain.*")  # the reference widths at batch 128 must not fall back
        model = H.train_classifier(X[:1000], X[1000:], y[:1000], y[1000:], None, cfg, device=DEV, verbose=False, fused=True)   # 900 = 7 * 128 + 4
    assert len(model.history) == 6 and all(len(h) == 4 for h in model.history)
    assert model.history[-1][3] > 0.9, model.history
    model.eval()
    with torch.no_grad():
        yt = _dev(torch.tensor(y[1000:]))
        acc = pcg.ops.cf_metrics(model(_dev(torch.tensor(X[1000:], dtype=torch.float32))).contiguous(), yt, other=yt)[0].item()
    assert acc > 0.9
    ref = HR.NNClassifier(17, 4)
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        assert float((ref(torch.tensor(X[1000:], dtype=torch.float32)).argmax(1) == torch.tensor(y[1000:])).float().mean()) > 0.9


def test_fallback_warns_and_runs_the_chain(pcg):
    H = pcg.house
    X, y = _separable(400)
    H._fused_fallback_warned = False
    with pytest.warns(RuntimeWarning, match="op chain"):
        model = H.train_classifier(X[:300], X[300:], y[:300], y[300:], None, dict(H.CONFIG, clf_epochs=1, batch_size=160, seed=1), device=DEV,
                                   verbose=False, fused=True)
    assert len(model.history) == 1


def test_launch_count(pcg, monkeypatch):
    H, ops = pcg.house, pcg.ops
    calls = []
    real_check = ops.check
    monkeypatch.setattr(ops, "check", lambda rc, what="": (calls.append(what), real_check(rc, what))[1])
    new = {"pcg_dense_rows_fwd_post", "pcg_dense_rows_dgrad_post", "pcg_ce_weighted_tally", "pcg_house_clf_batch", "pcg_house_clf_batch_counter"}
    per_step_chain_ops = ("pcg_dropout_apply", "pcg_rand_bernoulli", "pcg_bn_train_stats", "pcg_bn_apply_act", "pcg_bn_act_bwd", "pcg_act_fwd")
    X, y = _separable(330)
    seen = {}
    for fused in (True, False):
        del calls[:]
        H.train_classifier(X[:300], X[300:], y[:300], y[300:], None, dict(H.CONFIG, clf_epochs=2, batch_size=128, seed=1), device=DEV,
                           verbose=False, fused=fused)                       # 270 training rows: 128 + 128 + 14
        seen[fused] = list(calls)
    print(f"fused: {len(seen[True])} library calls {sorted(set(seen[True]))}; chain: {len(seen[False])}")
    assert not new & set(seen[False]) and all(seen[False].count(w) >= 6 for w in per_step_chain_ops)
    assert not [w for w in seen[True] if w in per_step_chain_ops or w.startswith("pcg_bn_")]
    # two graphs, each run once and captured once, and one validation launch per epoch; the replays are not library calls
    assert seen[True].count("pcg_ce_weighted_tally") == 2 * 2 + 2 and seen[True].count("pcg_adam_step_capturable") == 2 * 3
    # the same entries called eagerly: per batch one gather, one tally, 4 + 1 forwards, 4 stage backwards, 5 weight gradients, AdamW
    model = H.NNClassifier(17, 4).to(DEV)
    fit = H.ClassifierFit(model, X[:270].astype(np.float32), y[:270], torch.ones(4, device=DEV), 128, graph=False)
    del calls[:]
    fit.epoch(torch.arange(270))
    want = {"pcg_house_clf_batch": 1, "pcg_dense_rows_fwd_post": 4, "pcg_dense_rows_fwd": 1, "pcg_ce_weighted_tally": 1, "pcg_dense_rows_dgrad_post": 4,
            "pcg_dense_rows_wgrad": 5, "pcg_adam_step_capturable": 1}
    got = {w: calls.count(w) for w in set(calls) - {"pcg_fill"}}          # (pcg_fill: the fresh Adam moments, once)
    print(f"eager epoch of 3 batches: {got}")
    assert got == {w: 3 * n for w, n in want.items()}
