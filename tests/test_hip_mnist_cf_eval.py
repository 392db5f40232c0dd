"""GPU: the MNIST CounteRGAN's prompted queries and per-target evaluation (csrc/mnist_cf_eval.hip through pcgan_amd.ops and
pcgan_amd.countergan) against torch indexing, float64 numpy, the float64 generator built from the oracle module, and
the reference's own recorded results (tests/golden/mnist_cf_eval_ref.npz, made by make_golden_mnist_cf_eval.py).

Tolerances.  Elementwise results of the tail kernel: 1 ulp of fp32 per step (each step against float64 fed with the step before).
Sums of 784 fp32 terms: rtol 1e-5.  Residuals and counterfactuals of the whole generator: test_trained_checkpoint_eval_forward's
rtol 1e-4, atol 2e-5 * max|raw|, or 3x the CPU fp32 module's own distance from float64 where that is larger; probabilities: the same
with scale 1.  Metrics: rtol 2e-4, atol 2e-6 (test_evaluate_counterfactuals_matches_reference's).
Undecided queries.  The golden file marks the queries whose float64 top-two probability gap is under max(1e-5, 100 x the reference's
own fp32-to-float64 distance): they are left out of the pred / flip equalities and widen the flip-rate tolerance by
undecided / count.  The bound comes from the reference's two CPU runs, never from the GPU result; at most 5 % may be undecided."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import countergan_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW = 784
USER = [1, 5, 10, 12, 13, 14]


@pytest.fixture(scope="module")
def K():
    import pcgan_amd  # noqa: F401
    from pcgan_amd import countergan
    return countergan


@pytest.fixture(scope="module")
def ops():
    import pcgan_amd
    return pcgan_amd.ops


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mnist_cf_eval_ref.npz")))


@pytest.fixture(scope="module")
def state(golden_dir):
    return torch.load(os.path.join(golden_dir, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def nets(K, state):
    """The shipped generator checkpoint and the seeded classifier of the golden files, in eval mode on the GPU."""
    G = K.ResidualGenerator()
    G.load_state_dict(state)
    torch.manual_seed(3)
    C = K.CNNClassifier()
    return G.to(DEV).eval(), C.to(DEV).eval()


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _query_rows(B, T, q0, nq):
    q = np.arange(q0, q0 + nq)
    return q, q // B, q % B


# ---- 1. the entry kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sweep", "per_row"])
def test_entry_is_torch_indexing(ops, form):
    g = torch.Generator().manual_seed(0)
    B, T, Kc = (3, 10, 10) if form == "sweep" else (5, 1, 10)
    x = torch.randn(B, HW, generator=g)
    table = torch.randn(Kc, HW, generator=g)
    target = None if form == "sweep" else torch.randint(0, Kc, (B,), generator=g)
    masks = {"shared": torch.rand(HW, generator=g), "row": torch.rand(B, HW, generator=g), "query": torch.rand(T * B, HW, generator=g)}
    windows = [(0, T * B), (4, 7)] if form == "sweep" else [(0, B), (1, 3)]
    for mode, m in masks.items():
        for q0, nq in windows:
            q, t, b = _query_rows(B, T, q0, nq)
            tgt = torch.from_numpy(t) if target is None else target[b]
            mrow = m.expand(nq, HW) if mode == "shared" else m[b] if mode == "row" else m[q]
            want = torch.stack([x[b], table[tgt], mrow], dim=-1)
            got = ops.mnist_cf_entry(x.to(DEV), target.to(DEV) if target is not None else None, table.to(DEV), m.to(DEV), mode, T, q0, nq)
            assert tuple(got.shape) == (nq, HW, 3)
            assert torch.equal(got.cpu(), want), (form, mode, q0, nq)


# ---- 2. patch masks -----------------------------------------------------------------------------------------------------------------------
def test_patch_masks_are_the_references(K, ops, ref):
    cases = json.loads(str(ref["sel.cases"]))
    x = torch.zeros(4, 1, 28, 28, device=DEV)
    for name, case in cases.items():
        np.random.seed(case["seed"])
        bm, sm = K.build_patch_mask_for_batch(x[:case["bs"]], patch_size=case["patch_size"], **case["kwargs"])
        want = ref[f"sel.{name}.mask"].astype(np.float32)
        assert tuple(bm.shape) == (case["bs"], 1, 28, 28) and tuple(sm.shape) == (1, 1, 28, 28)
        np.testing.assert_array_equal(bm.cpu().numpy()[:, 0], want, err_msg=name)
        np.testing.assert_array_equal(sm.cpu().numpy()[0, 0], want[0], err_msg=name)
    # the prompt's own entry point (gradio_app.py:234-240): 16 patches; 25 with the 3-pixel border; 49 with bits above 31 and indices
    # outside [0, 49) ignored; the empty list
    for name in ("user7", "user5", "user4", "empty7"):
        case = cases[name]
        m = K.make_mask_from_patch_list(x[:1], case["patch_size"], case["kwargs"]["modifiable_patches"]).cpu().numpy()[0, 0]
        np.testing.assert_array_equal(m, ref[f"sel.{name}.mask"][0].astype(np.float32), err_msg=name)
    assert ref["sel.user5.mask"][0][25:, :].sum() == 0 and ref["sel.user5.mask"][0][:, 25:].sum() == 0 and ref["sel.user5.mask"][0].sum() == 5 * 25
    assert ref["sel.user4.mask"][0].sum() == 5 * 16 and ref["sel.empty7.mask"].sum() == 0
    # raw words: every bit of a 7 x 7 grid on its own, and all 64 bits of an 8 x 8 grid (ps = 3 on 24 x 24)
    bits = torch.tensor([1 << p for p in range(49)], dtype=torch.int64, device=DEV)
    m = ops.patch_mask_bits(bits, 28, 28, 4).cpu().numpy()[:, 0]
    for p in range(49):
        want = np.zeros((28, 28), np.float32)
        want[4 * (p // 7):4 * (p // 7) + 4, 4 * (p % 7):4 * (p % 7) + 4] = 1
        np.testing.assert_array_equal(m[p], want, err_msg=str(p))
    full = ops.patch_mask_bits(torch.tensor([-1, K.patch_bits([63], 64)], dtype=torch.int64, device=DEV), 24, 24, 3).cpu().numpy()[:, 0]
    assert full[0].sum() == 576 and full[1].sum() == 9 and full[1][21:, 21:].sum() == 9


# ---- 3. the tail kernel ---------------------------------------------------------------------------------------------------------------------
def test_tail_against_float64(ops):
    g = torch.Generator().manual_seed(2)
    B, T, q0, nq, scale = 3, 10, 4, 7, 0.1
    q, t, b = _query_rows(B, T, q0, nq)
    x = torch.rand(B, HW, generator=g) * 2 - 1
    edge = torch.tensor([1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), -np.nextafter(np.float32(1), np.float32(0)), 0.0])
    x[:, :200] = edge[torch.randint(0, 5, (B, 200), generator=g)]           # at and next to +-1
    c = torch.randn(nq, HW, generator=g) * 3
    c[:, :100] = torch.where(torch.rand(nq, 100, generator=g) > 0.5, 50.0, -50.0)   # |raw| = 5: both clamps fire
    m = torch.tensor([0.0, 1.0, 0.37])[torch.randint(0, 3, (B, HW), generator=g)]
    xd, cd, md = x.to(DEV), c.to(DEV), m.to(DEV)
    x_cf, raw, masked, sums = (v.cpu().numpy().astype(np.float64) for v in ops.mnist_cf_tail(cd, xd, md, "row", scale, T, q0, nq))
    x64, c64, m64 = x.numpy().astype(np.float64)[b], c.numpy().astype(np.float64), m.numpy().astype(np.float64)[b]
    s32 = float(np.float32(scale))
    # every step within 1 ulp of the float64 result of that step (the compiler may contract x + raw * m)
    assert (np.abs(raw - c64 * s32) <= _ulp(c64 * s32)).all()
    assert (np.abs(masked - raw * m64) <= _ulp(raw * m64)).all()
    want_cf = np.clip(x64 + masked, -1.0, 1.0)
    assert (np.abs(x_cf - want_cf) <= _ulp(want_cf)).all()
    assert (x_cf == 1.0).sum() > 50 and (x_cf == -1.0).sum() > 50 and np.abs(x_cf).max() <= 1.0
    r64 = c64 * s32
    cf64 = np.clip(x64 + r64 * m64, -1.0, 1.0)
    want = np.stack([np.abs(cf64 - x64).sum(1), np.abs(r64 * m64).sum(1), np.abs(r64 * (1.0 - m64)).sum(1)], axis=1)
    np.testing.assert_allclose(sums, want, rtol=1e-5)
    # the optional outputs off; the same bits from a second call
    x_cf2, raw2, masked2, sums2 = ops.mnist_cf_tail(cd, xd, md, "row", scale, T, q0, nq, want_residuals=False)
    assert raw2 is None and masked2 is None
    assert np.array_equal(x_cf2.cpu().numpy(), x_cf.astype(np.float32)) and np.array_equal(sums2.cpu().numpy(), sums.astype(np.float32))
    # the other two mask modes read the rows they should
    mq = torch.rand(T * B, HW, generator=g)
    s_q = ops.mnist_cf_tail(cd, xd, mq.to(DEV), "query", scale, T, q0, nq)[3].cpu().numpy()
    np.testing.assert_allclose(s_q[:, 1], np.abs(r64 * mq.numpy().astype(np.float64)[q]).sum(1), rtol=1e-5)
    s_s = ops.mnist_cf_tail(cd, xd, mq[5].contiguous().to(DEV), "shared", scale, T, q0, nq)[3].cpu().numpy()
    np.testing.assert_allclose(s_s[:, 2], np.abs(r64 * (1.0 - mq[5].numpy().astype(np.float64))).sum(1), rtol=1e-5)


# ---- 4. the score kernel -------------------------------------------------------------------------------------------------------------------
def _softmax64(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@pytest.mark.parametrize("with_orig", [False, True])
def test_score_against_float64(ops, with_orig):
    g = torch.Generator().manual_seed(4)
    B, T, Kc, ld, gr = 3, 10, 10, 12, 2
    TB = T * B
    lg = torch.randn(TB, ld, generator=g) * 3
    lg[:, Kc:] = 1e30                                        # the padding columns are never read
    lg[2, 3], lg[2, 8] = 80.0, -80.0
    lg[7, 0], lg[7, 9] = -80.0, 80.0
    lg[11, 2] = lg[11, 6] = 9.0                              # an exact tie at the top: the lower index wins
    lo = torch.randn(B, ld, generator=g) * 3
    lo[:, Kc:] = 1e30
    lo[1, 4] = 80.0
    y = torch.tensor([4, 4, 7])
    tail = torch.rand(TB, 3, generator=g) * 100
    p = _softmax64(lg[:, :Kc].numpy().astype(np.float64))
    top = np.sort(p, -1)
    assert ((top[:, -1] - top[:, -2])[np.arange(TB) != 11] > 1e-4).all()       # every other argmax is decided
    po = _softmax64(lo[:, :Kc].numpy().astype(np.float64))
    q, t, b = _query_rows(B, T, 0, TB)
    yb = y.numpy()[b]
    want = {"pred": p.argmax(-1), "conf": p.max(-1), "p_target": p[q, t], "p_true": p[q, yb],
            "p_orig_true": po[b, yb] if with_orig else np.zeros(TB)}
    want["flip"] = (want["pred"] == t).astype(np.float64)
    assert want["pred"][11] == 2

    def run(q0=0, nq=TB):
        return ops.mnist_cf_score(lg[q0:q0 + nq].contiguous().to(DEV), Kc, B, T, y_true=y.to(DEV), logits_orig=lo.to(DEV) if with_orig else None,
                                  tail_sums=tail[q0:q0 + nq].contiguous().to(DEV), group_rows=gr, q0=q0, nq=nq)
    res = run()
    assert torch.equal(res["pred"].cpu(), torch.from_numpy(want["pred"]))
    assert np.array_equal(res["flip"].cpu().numpy(), want["flip"])
    for k in ("conf", "p_target", "p_true", "p_orig_true"):                    # expf and a ten-term sum in fp32
        np.testing.assert_allclose(res[k].cpu().numpy(), want[k], rtol=1e-5, atol=1e-7, err_msg=k)
    per = np.stack([want["flip"], want["flip"], want["p_target"] - want["p_true"],
                    (want["p_target"] - want["p_orig_true"]) if with_orig else np.zeros(TB)] + [tail.numpy().astype(np.float64)[:, i] for i in range(3)]
                   + [np.ones(TB)], axis=1).reshape(T, B, 8)
    gs = np.zeros((T, 2, 8))
    for j, (b0, b1) in enumerate(((0, 2), (2, 3))):                            # a group of 2 rows and the ragged one of 1
        gs[:, j] = per[:, b0:b1].sum(1)
        gs[:, j, 1] = per[:, b0:b1, 1].max(1)
    got = res["group_sums"].cpu().numpy()
    assert got.shape == (T, 2, 8)
    np.testing.assert_array_equal(got[..., 7], [[2, 1]] * T)
    np.testing.assert_array_equal(got[..., :2], gs[..., :2])
    np.testing.assert_allclose(got, gs, rtol=1e-5, atol=1e-6)
    res2 = run()
    for k in res:
        assert torch.equal(res[k], res2[k]), k                                  # fixed order: the same bits
    # a window that cuts groups: per-query values are the same bits, the groups count only their rows inside it
    w = run(4, 7)
    for k in ("pred", "conf", "p_target", "p_true", "p_orig_true", "flip"):
        assert torch.equal(w[k], res[k][4:11]), k
    cnt = np.zeros((T, 2))
    for qq in range(4, 11):
        cnt[qq // B, (qq % B) // gr] += 1
    np.testing.assert_array_equal(w["group_sums"].cpu().numpy()[..., 7], cnt)


# ---- 5. the BatchNorm fold -----------------------------------------------------------------------------------------------------------------
def _tol(got, ref64, cpu32, scale):
    """rtol 1e-4, atol 2e-5 * scale — or 3x the CPU fp32 module's own distance from float64 where that is larger."""
    floor = 3.0 * float(np.abs(cpu32.astype(np.float64) - ref64).max())
    np.testing.assert_allclose(got, ref64, rtol=1e-4, atol=max(2e-5 * scale, floor))


def test_forward_queries_folded_and_unfolded_against_float64(K, nets, state, ref):
    G, _ = nets
    B = 4
    x = torch.from_numpy(ref["x"][:B])
    t = torch.tensor([7, 1, 0, 9])
    np.random.seed(5)
    mask = K.build_patch_mask_for_batch(x.to(DEV), patch_size=7, min_patches=6, max_patches=15)[0].contiguous()
    R32 = CR.ResidualGenerator()
    R32.load_state_dict(state)
    R32.eval()
    R64 = CR.ResidualGenerator().double()
    R64.load_state_dict(state)
    R64.eval()
    with torch.no_grad():
        raw32, masked32 = (v.numpy().reshape(B, HW) for v in R32(x, t, mask.cpu()))
        raw64, masked64 = (v.numpy().reshape(B, HW) for v in R64(x.double(), t, mask.cpu().double()))
    cf64 = np.clip(x.numpy().astype(np.float64).reshape(B, HW) + masked64, -1, 1)
    cf32 = np.clip(x.numpy().reshape(B, HW) + masked32, -1, 1)
    scale = float(np.abs(raw64).max())
    outs = {}
    for fold in (True, False):
        r = G.forward_queries(x.to(DEV), t.to(DEV), mask, "row", fold_eval_bn=fold)
        outs[fold] = r
        _tol(r["raw"].cpu().numpy(), raw64, raw32, scale)
        _tol(r["masked"].cpu().numpy(), masked64, masked32, scale)
        _tol(r["x_cf"].cpu().numpy(), cf64, cf32, scale)
        m64 = mask.cpu().numpy().astype(np.float64).reshape(B, HW)
        want = np.stack([np.abs(cf64 - x.numpy().reshape(B, HW)).sum(1), np.abs(raw64 * m64).sum(1), np.abs(raw64 * (1 - m64)).sum(1)], 1)
        np.testing.assert_allclose(r["sums"].cpu().numpy(), want, rtol=1e-4, atol=2e-5 * scale * HW)
    assert not torch.equal(outs[True]["raw"], outs[False]["raw"])               # two different roundings: the switch does switch
    assert G._fold_cache is not None and len(G.folded_conv1()) == 6
    # the unfolded chain IS the module's eval forward
    with torch.no_grad():
        raw_m, masked_m = G(x.to(DEV), t.to(DEV), mask)
    assert torch.equal(raw_m.view(B, HW), outs[False]["raw"]) and torch.equal(masked_m.view(B, HW), outs[False]["masked"])


# ---- 6. the golden sweep --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(K, nets, ref):
    G, C = nets
    x, y = torch.from_numpy(ref["x"][:6]).to(DEV), torch.from_numpy(ref["y"][:6]).to(DEV)
    return x, y, K.counterfactual_sweep(G, C, x, y_true=y, patches=USER, patch_size=7)


def test_sweep_matches_the_reference(K, ref, sweep):
    x, y, s = sweep
    T, B = 10, 6
    scale = float(np.abs(ref["sweep.raw"]).max())
    np.testing.assert_array_equal(s["mask"].cpu().numpy()[0, 0], ref["sweep.mask"])
    for k, g in (("raw_residual", "raw"), ("masked_residual", "masked"), ("x_cf", "x_cf")):
        assert tuple(s[k].shape) == (T, B, 1, 28, 28)
        np.testing.assert_allclose(s[k].cpu().numpy().reshape(T, B, HW), ref[f"sweep.{g}"], rtol=1e-4, atol=2e-5 * scale, err_msg=k)
    p, yb = ref["sweep.probs_cf"], ref["y"][:6]
    tt, bb = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    np.testing.assert_allclose(s["conf"].cpu().numpy(), p.max(-1), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(s["p_target"].cpu().numpy(), p[tt, bb, tt], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(s["p_true"].cpu().numpy(), p[tt, bb, yb[bb]], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(s["p_orig_true"].cpu().numpy(), np.broadcast_to(ref["sweep.probs_orig"][np.arange(B), yb], (T, B)), rtol=1e-4, atol=2e-5)
    und = ref["sweep.undecided"]
    assert und.mean() <= 0.05
    print(f"sweep: {int(und.sum())} of {und.size} queries undecided (bound {float(ref['sweep.undecided_bound']):.1e})")
    np.testing.assert_array_equal(s["pred"].cpu().numpy()[~und], ref["sweep.pred"][~und])
    np.testing.assert_array_equal(s["flip"].cpu().numpy()[~und], (ref["sweep.pred"] == tt)[~und].astype(np.float32))
    assert (ref["sweep.pred"] == tt).any() and not (ref["sweep.pred"] == tt).all()      # the data has flips and misses


def test_masked_metrics_match_the_reference(K, nets, ref, sweep):
    """compute_masked_metrics' six values per target class: from the sweep's own group sums, and through the function with the
    reference's signature for three of the targets (one that flips, two that do not)."""
    _, C = nets
    x, y, s = sweep
    gold, und = ref["sweep.masked_metrics"], ref["sweep.undecided"]
    m = K.metrics_from_sums(s["group_sums"].cpu().numpy()[:, 0], HW)
    got = np.stack([m["class_flip_rate"], m["class_flip_max"], m["allowed_l1"], m["prediction_gain_orig"], m["actionability"], m["mask_penalty_pre"]], 1)
    slack = und.sum(1) / 6.0
    for t in range(10):
        print(f"target {t}: sums {got[t]} reference {gold[t]}")
        if und[t].any():
            assert abs(got[t, 0] - gold[t, 0]) <= slack[t] + 2e-6
        else:
            np.testing.assert_allclose(got[t, :2], gold[t, :2], rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(got[t, 2:], gold[t, 2:], rtol=2e-4, atol=2e-6, err_msg=str(t))
    for t in (7, 1, 4):
        d = K.compute_masked_metrics(s["raw_residual"][t], s["masked_residual"][t], x, s["x_cf"][t], s["mask"].expand(6, 1, 28, 28), C, y,
                                     torch.full_like(y, t), DEV)
        assert tuple(d) == K.MASKED_METRIC_KEYS
        v = np.array(list(d.values()))
        np.testing.assert_allclose(v[2:], gold[t, 2:], rtol=2e-4, atol=2e-6, err_msg=str(t))
        np.testing.assert_allclose(v[:2], gold[t, :2], rtol=2e-4, atol=2e-6 + slack[t], err_msg=str(t))


def test_prompted_query_is_the_sweeps_row(K, nets, ref, sweep):
    """counterfactuals(): one target per row, patch lists per row and a dense mask; equal to the sweep's entries where they ask the same."""
    G, C = nets
    x, y, s = sweep
    tgt = torch.tensor([7, 1, 4, 7, 0, 9], device=DEV)
    r = K.counterfactuals(G, C, x, tgt, patches=USER, y_true=y)
    idx = tgt.cpu().numpy(), np.arange(6)
    scale = float(np.abs(ref["sweep.raw"]).max())
    np.testing.assert_allclose(r["raw_residual"].cpu().numpy().reshape(6, HW), ref["sweep.raw"][idx], rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(r["x_cf"].cpu().numpy().reshape(6, HW), ref["sweep.x_cf"][idx], rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(r["p_target"].cpu().numpy(), ref["sweep.probs_cf"][idx][np.arange(6), idx[0]], rtol=1e-4, atol=2e-5)
    ok = ~ref["sweep.undecided"][idx]
    np.testing.assert_array_equal(r["pred"].cpu().numpy()[ok], ref["sweep.pred"][idx][ok])
    assert tuple(r["sums"].shape) == (6, 3) and tuple(r["mask"].shape) == (1, 1, 28, 28)
    # the same prompt as a dense mask and as one list per row; an int target
    r2 = K.counterfactuals(G, C, x, tgt, mask=r["mask"])
    r3 = K.counterfactuals(G, C, x, tgt, patches=[USER] * 6)
    for k in ("x_cf", "raw_residual", "masked_residual", "sums", "pred", "p_target"):
        assert torch.equal(r2[k], r[k]) and torch.equal(r3[k], r[k]), k
    one = K.counterfactuals(G, C, x[:1], 7, patches=USER)                       # "turn this image into a 7, touching only these patches"
    np.testing.assert_allclose(one["x_cf"].cpu().numpy().reshape(1, HW), ref["sweep.x_cf"][7, :1], rtol=1e-4, atol=2e-5 * scale)
    outside = ref["sweep.mask"].reshape(HW) == 0
    assert torch.equal(one["x_cf"].view(HW)[torch.from_numpy(outside).to(DEV)], x[0].view(HW)[torch.from_numpy(outside).to(DEV)])


# ---- 7. the per-target table -----------------------------------------------------------------------------------------------------------------
class _Cfg:
    device, num_classes = DEV, 10

    def __init__(self, save_dir):
        self.save_dir = str(save_dir)


def test_per_target_table(K, nets, ref, tmp_path):
    G, C = nets
    x, y = torch.from_numpy(ref["x"]), torch.from_numpy(ref["y"])
    loader = [(x[i:i + 4], y[i:i + 4]) for i in range(0, 11, 4)]
    gold = ref["table.metrics"]
    und, counts = ref["table.undecided"], ref["table.counts"]
    assert und.sum() <= 0.05 * 110
    print(f"table: {int(und.sum())} of 110 queries undecided (bound {float(ref['table.undecided_bound']):.1e})")
    slack = (und / counts[None, :]).mean(1)

    def table(sub, **kw):
        res = K.evaluate_generator_per_target(G, C, loader, _Cfg(tmp_path / sub), verbose=False, **kw)
        return np.array([[res[c][k] for k in K.PER_CLASS_FIELDS] for c in range(10)])

    def close(a, b, what):
        np.testing.assert_allclose(a[:, 1:], b[:, 1:], rtol=2e-4, atol=2e-6, err_msg=what)
        assert (np.abs(a[:, 0] - b[:, 0]) <= 2e-4 * np.abs(b[:, 0]) + 2e-6 + slack).all(), what
    one = table("one")
    print("one pass\n", one, "\nreference\n", gold)
    close(one, gold, "one pass against the reference")
    close(table("loop", one_pass=False), gold, "evaluate_counterfactuals loop against the reference")
    close(one, table("loop2", one_pass=False), "one pass against the loop")
    close(table("chunk", query_chunk=7), one, "query_chunk = 7 against the unchunked pass")
    close(table("unfolded", fold_eval_bn=False), one, "unfolded against folded")
    assert gold[:, 0].max() > 0                                                  # some target does flip
    text = open(tmp_path / "one" / "countergan_metrics_per_class.csv").read()
    assert text.split("\n")[0] == ",class_flip_rate,prediction_gain,actionability" and len(text.strip().split("\n")) == 11
    assert text == K.per_class_csv({c: dict(zip(K.PER_CLASS_FIELDS, one[c])) for c in range(10)})


def test_evaluate_classifier_counts(K, nets, ref):
    _, C = nets
    x, y = torch.from_numpy(ref["x"]), torch.from_numpy(ref["y"])
    loader = [(x[i:i + 4], y[i:i + 4]) for i in range(0, 11, 4)]
    acc, cm = K.evaluate_classifier(C, loader, DEV, verbose=False)
    with torch.no_grad():
        pred = C(x.to(DEV)).argmax(1).cpu().numpy()
    want = np.zeros((10, 10), np.int64)
    np.add.at(want, (y.numpy(), pred), 1)
    np.testing.assert_array_equal(cm, want)
    assert cm.sum() == 11 and acc == float((pred == y.numpy()).mean())


# ---- 8. argument checks -------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(K, ops, nets, ref):
    import pcgan_amd
    E = pcgan_amd.PcgError
    G, C = nets
    x = torch.from_numpy(ref["x"][:3]).to(DEV)
    with pytest.raises(E, match="GPU"):
        K.counterfactuals(G, C, x.cpu(), 3)
    with pytest.raises(E, match="GPU"):
        K.counterfactuals(G, C, x, 3, mask=torch.ones(1, 1, 28, 28))
    with pytest.raises(E, match="not both"):
        K.counterfactuals(G, C, x, 3, patches=USER, mask=torch.ones(1, 1, 28, 28, device=DEV))
    with pytest.raises(E, match="no patch"):
        K.counterfactuals(G, C, x, 3, patches=USER, patch_size=29)
    with pytest.raises(E, match="no patch"):
        K.make_mask_from_patch_list(x, 0, USER)
    with pytest.raises(E, match="mask"):
        K.counterfactuals(G, C, x, 3, mask=torch.ones(2, 1, 28, 28, device=DEV))          # neither 1 nor B rows
    with pytest.raises(E, match="mask"):
        K.counterfactual_sweep(G, C, x, mask=torch.ones(10, 2, 1, 28, 28, device=DEV))
    with pytest.raises(E, match="mask"):
        G.forward_queries(x, None, torch.ones(3, HW, device=DEV), "shared")
    with pytest.raises(E, match="mask_mode"):
        G.forward_queries(x, None, torch.ones(HW, device=DEV), "all")
    with pytest.raises(E, match="window"):
        G.forward_queries(x, None, torch.ones(HW, device=DEV), "shared", q0=28, nq=3)
    with pytest.raises(E, match="target"):
        K.counterfactuals(G, C, x, torch.tensor([1, 2], device=DEV))
    with pytest.raises(E, match="lists"):
        K.counterfactuals(G, C, x, 3, patches=[USER, USER])
    G.train()
    try:
        with pytest.raises(E, match="eval"):
            K.counterfactuals(G, C, x, 3, patches=USER)
    finally:
        G.eval()
    # more than 64 patches: the dense host path gives the same kind of mask
    m = K.make_mask_from_patch_list(x, 2, [0, 14, 195, 196]).cpu().numpy()[0, 0]
    assert m.sum() == 12 and m[0:2, 0:2].all() and m[2:4, 0:2].all() and m[26:28, 26:28].all()
