"""GPU: the evaluation reports (csrc/cf_report.hip through pcgan_amd.ops, countergan, gan_train and house) against
the restatement (tests/cf_report_restate.py) and the reference's own recorded runs (tests/golden/cf_report_ref.npz, written by
tests/golden/make_golden_cf_report.py).

Tolerances, none of them new.  The pick alone, on given logits: the picks equal the float64 restatement exactly (the data keeps the
top two confidences of a class >= 1e-4 apart) and the confidences hold test_hip_mnist_cf_eval.py's score-kernel tolerance, rtol 1e-5,
atol 1e-7.  Pixels: bit-identical.  The grid against the golden: cells at that file's query tolerance for x_cf, rtol 1e-4, atol
2e-5 * max|raw| (halved, as (x_cf + 1) / 2 halves a distance), conf at its probability tolerance rtol 1e-4, atol 2e-5, pred on the
decided cells.  The additive-delta grids: test_hip_delta_cf.py's rule (rtol 1e-4 with atol 2e-5 * max|reference|, or 3x the
restatement's own fp32-to-float64 distance).  The case studies: test_hip_house_cf_eval.py's classifier-probability tolerance, rtol
2e-4, atol 2e-5, for prediction_gain; everything else as tests/test_cf_report_host.py."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cf_report_restate as RR  # noqa: E402
import test_cf_report_host as HT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW = 784


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
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cf_report_ref.npz")))


@pytest.fixture(scope="module")
def nets(K, golden_dir):
    """The shipped generator checkpoint and the seeded classifier of the golden file, in eval mode on the GPU."""
    G = K.ResidualGenerator()
    G.load_state_dict(torch.load(os.path.join(golden_dir, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    torch.manual_seed(3)
    C = K.CNNClassifier()
    return G.to(DEV).eval(), C.to(DEV).eval()


def _words(state):
    return state.cpu().numpy().view(np.uint64)


# ---- 1. pcg_class_pick alone ----------------------------------------------------------------------------------------------------------
def _pick_case(Kc, kp):
    """700 rows of logits on the 1/8 grid; planted: a class without a row (Kc - 1), labels -1 and Kc, a NaN row that would win, and the
    best row of class 0 repeated bit for bit in the last chunk."""
    g = np.random.RandomState(10 + Kc)
    n = 700
    logits = (g.randint(-24, 25, (n, kp)) / 8.0).astype(np.float32)
    labels = g.randint(0, Kc - 1, n).astype(np.int64)
    labels[[5, 300]], labels[[6, 699]] = -1, Kc
    logits[40] = np.nan
    logits[41, :Kc] = -3.0
    logits[41, labels[41]] = np.nan
    conf64 = RR.confidences(logits[:, :Kc].astype(np.float64), labels)
    rows, _ = RR.pick(labels, Kc, conf64)
    dup = 600 + Kc
    logits[dup], labels[dup] = logits[rows[0]], 0
    assert rows[0] < 512 < dup
    conf64 = RR.confidences(logits[:, :Kc].astype(np.float64), labels)
    rows, conf = RR.pick(labels, Kc, conf64)
    assert rows[Kc - 1] == RR.ABSENT and (rows[:-1] >= 0).all() and conf64[dup] == conf64[rows[0]]
    for k in range(Kc - 1):                       # the winner is decided: the next distinct confidence of the class is >= 1e-4 below
        c = conf64[(labels == k) & np.isfinite(conf64)]
        below = c[c < conf[k]]
        assert len(below) and conf[k] - below.max() >= 1e-4, (k, conf[k], below.max())
    return logits, labels, rows, conf


@pytest.mark.parametrize("Kc,kp", [(10, 12), (3, 4)])
def test_class_pick_alone(ops, Kc, kp):
    logits, labels, rows, conf = _pick_case(Kc, kp)
    ld, yd = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    chunks = [(r0, min(256, 700 - r0)) for r0 in range(0, 700, 256)]
    assert [c[1] for c in chunks] == [256, 256, 188]

    def run(order, mode):
        state = ops.class_pick_state(Kc, DEV)
        for r0, n in order:
            ops.class_pick(state, yd[r0:r0 + n], Kc, row0=r0, logits=ld[r0:r0 + n] if mode == "best" else None, mode=mode)
        return state
    best = run(chunks, "best")
    got_rows, got_conf, src = ops.class_pick_gather(best, Kc, "best")
    assert src is None
    np.testing.assert_array_equal(got_rows.cpu().numpy(), rows)
    np.testing.assert_allclose(got_conf.cpu().numpy(), conf, rtol=1e-5, atol=1e-7)
    assert _words(best)[Kc - 1] == 0 and float(got_conf[Kc - 1]) == 0.0
    np.testing.assert_array_equal(_words(run(chunks[::-1], "best")), _words(best))          # any order of the chunks: the same words
    np.testing.assert_array_equal(_words(run([chunks[1], chunks[2], chunks[0]], "best")), _words(best))
    first = run(chunks, "first")
    f_rows, f_conf, _ = ops.class_pick_gather(first, Kc, "first", X=None)
    np.testing.assert_array_equal(f_rows.cpu().numpy(), RR.pick(labels, Kc)[0])
    assert not f_conf.cpu().numpy().any()
    np.testing.assert_array_equal(_words(run(chunks[::-1], "first")), _words(first))
    # the resident gather: X[rows], zeros for the absent class
    X = torch.from_numpy(np.random.RandomState(1).rand(700, 20).astype(np.float32)).to(DEV)
    _, _, src = ops.class_pick_gather(best, Kc, "best", X=X)
    want = X.cpu().numpy()[np.maximum(rows, 0)]
    want[rows < 0] = 0.0
    np.testing.assert_array_equal(src.cpu().numpy(), want)


def test_class_pick_argument_checks(ops):
    import pcgan_amd
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    lg = torch.zeros((4, 12), device=DEV)
    st = ops.class_pick_state(10, DEV)
    for bad in (dict(row0=(1 << 32) - 4), dict(row0=-1), dict(mode="best"), dict(mode="best", logits=lg[:, :10].contiguous()),
                dict(mode="best", logits=lg[:3]), dict(mode="nearest")):
        with pytest.raises(pcgan_amd.PcgError):
            ops.class_pick(st, y, 10, **bad)
    with pytest.raises(pcgan_amd.PcgError):
        ops.class_pick_state(65, DEV)
    with pytest.raises(pcgan_amd.PcgError):
        ops.class_pick(st, y.cpu(), 10)
    ops.class_pick(st, y, 10, row0=(1 << 32) - 5)                                          # the last rows a key can hold
    assert int(ops.class_pick_gather(st, 10, "first")[0][0]) == (1 << 32) - 5


# ---- 2. pick_sources end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth():
    g = torch.Generator().manual_seed(5)
    X = torch.randint(-8, 9, (300, 1, 28, 28), generator=g).float() / 8.0
    Y = torch.randint(0, 10, (300,), generator=g)
    Y[:40] = torch.randint(0, 9, (40,), generator=g)        # class 9 first shows up late: the reference's scan goes on past row 40
    return X, Y


@pytest.mark.parametrize("which", ["cnn", "pool"])
def test_pick_sources_is_the_first_maximum_of_p_true(K, ops, synth, which):
    X, Y = synth
    torch.manual_seed(3)
    C = (K.CNNClassifier() if which == "cnn" else K.Classifier()).to(DEV).eval()
    Xd, Yd = X.to(DEV), Y.to(DEV)

    def p_true(n):
        """The score kernel's own-label probabilities of rows [0, n), from the chunks pick_sources walks: the same launches, the same bits."""
        out = []
        for r0 in range(0, n, 128):
            xr = Xd[r0:min(n, r0 + 128)].reshape(-1, HW).contiguous()
            out.append(ops.mnist_cf_score(K._padded_logits(C, xr), 10, xr.shape[0], 1, y_true=Yd[r0:min(n, r0 + 128)].contiguous(),
                                          outputs=("p_true",), group_sums=False)["p_true"].cpu().numpy())
        return np.concatenate(out)
    y = Y.numpy()
    end = RR.scan_end(y, 10)
    assert 40 < end < 300
    for full, n in ((True, 300), (False, end)):
        src, rows, conf = K.pick_sources(C, (Xd, Yd), pick_best_source=True, chunk=128, full_scan=full)
        rows, conf, p = rows.cpu().numpy(), conf.cpu().numpy(), p_true(n)
        for k in range(10):
            cand = np.flatnonzero(y[:n] == k)
            want = cand[np.argmax(p[cand])]                 # argmax: the first maximum
            assert rows[k] == want and conf[k] == p[want], (full, k, rows[k], want, conf[k], p[want])
        assert torch.equal(src.cpu(), X[torch.from_numpy(rows)])
    full_rows = K.pick_sources(C, (Xd, Yd), True, 128, True)[1].cpu().numpy()
    assert (full_rows != rows).any(), "the data must tell the whole-data-set scan from the reference's"
    # "first" mode; a host pair and a map-style data set give the same picks as the resident one
    first = RR.pick(y, 10)[0]
    for ds in ((Xd, Yd), (X, Y), [(X[i], int(Y[i])) for i in range(300)]):
        src, rows, conf = K.pick_sources(C, ds, chunk=128)
        np.testing.assert_array_equal(rows.cpu().numpy(), first)
        assert not conf.cpu().numpy().any() and torch.equal(src.cpu(), X[torch.from_numpy(first)])
    src2, rows2, _ = K.pick_sources(C, [(X[i], int(Y[i])) for i in range(300)], True, 128, True)
    np.testing.assert_array_equal(rows2.cpu().numpy(), full_rows)
    with pytest.raises(K.PcgError, match="no row of class"):
        K.pick_sources(C, (Xd[:30], Yd[:30]))


# ---- 3. the pixels ------------------------------------------------------------------------------------------------------------------------
def _unit_edge(g, shape):
    """Values in [-1, 1] with the ends and arbitrary fp32 values in between."""
    v = torch.rand(shape, generator=g) * 2 - 1
    flat = v.view(-1)
    flat[:6] = torch.tensor([1.0, -1.0, 0.0, -0.0, 0.999999, -0.999999])
    return v


@pytest.mark.parametrize("n,shared", [(3, False), (1, True)])
def test_panels_are_bit_identical(ops, n, shared):
    g = torch.Generator().manual_seed(n)
    H, W = 28, 28
    x, x_cf = _unit_edge(g, (n, H * W)), _unit_edge(g, (n, H * W))
    mask = (torch.rand((1 if shared else n, H * W), generator=g) > 0.5).float()
    panels, vmax = ops.cf_panels(x.to(DEV), x_cf.to(DEV), H, W, mask=mask.to(DEV), mode="panels")
    want, wmax = RR.panels(x.numpy().reshape(n, H, W), x_cf.numpy().reshape(n, H, W), mask.numpy().reshape(-1, H, W))
    assert panels.shape == (n, 4, H, W) and panels.dtype == torch.float32
    np.testing.assert_array_equal(panels.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert vmax.cpu().numpy().view(np.uint32)[0] == np.float32(wmax).view(np.uint32) and wmax > 0


def test_panels_larger_than_one_grid_pass_and_a_zero_difference(ops):
    """More elements than 8192 blocks x 256 threads visit once (the grid-stride loop), an odd image size, and x_cf == x: vmax stays 0."""
    g = torch.Generator().manual_seed(9)
    n, H, W = 41, 231, 227
    assert n * H * W > 8192 * 256
    x, x_cf = torch.rand((n, H * W), generator=g) * 2 - 1, torch.rand((n, H * W), generator=g) * 2 - 1
    mask = torch.rand((H * W,), generator=g)
    panels, vmax = ops.cf_panels(x.to(DEV), x_cf.to(DEV), H, W, mask=mask.to(DEV), mode="panels")
    want, wmax = RR.panels(x.numpy().reshape(n, H, W), x_cf.numpy().reshape(n, H, W), mask.numpy().reshape(H, W))
    assert np.array_equal(panels.cpu().numpy().view(np.uint32), want.view(np.uint32)) and float(vmax) == float(wmax)
    same, v0 = ops.cf_panels(x[:2].to(DEV), x[:2].clone().to(DEV), H, W, mask=mask.to(DEV), mode="panels")
    assert float(v0) == 0.0 and not same[:, 2].cpu().numpy().any()


@pytest.mark.parametrize("Kc,H,W", [(3, 5, 7), (10, 28, 28)])
def test_grid_image_is_bit_identical(ops, Kc, H, W):
    g = torch.Generator().manual_seed(Kc)
    src, x_cf = _unit_edge(g, (Kc, H * W)), _unit_edge(g, (Kc, Kc, H * W))
    lv = min(256, H * W)
    x_cf[0, 1, :lv] = torch.arange(256)[:lv] / 255.0 * 2 - 1          # the 8-bit levels themselves
    image, u8 = ops.cf_panels(src.to(DEV), x_cf.to(DEV), H, W, mode="grid")
    want, want8 = RR.grid_image(src.numpy().reshape(Kc, H, W), x_cf.numpy().reshape(Kc, Kc, H, W))
    assert image.shape == (Kc * H, Kc * W) and u8.dtype == torch.uint8
    np.testing.assert_array_equal(image.cpu().numpy().view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(u8.cpu().numpy(), want8)


# ---- 4. countergan.counterfactual_grid against the golden ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["first", "best", "late"])
def test_counterfactual_grid_matches_the_reference(K, nets, gold, mode):
    """ "late": pick_best_source on the labels that hold class 9 back to the last row, so the reference's scan covers all 40 rows and
    its picks differ from the first rows; "best" with labels i % 10 ends after 10 rows and can only repeat "first"."""
    G, C = nets
    X, Y = torch.from_numpy(gold["grid.x"]), torch.from_numpy(gold["grid.y_late" if mode == "late" else "grid.y"])
    res = K.counterfactual_grid(G, C, (X.to(DEV), Y.to(DEV)), pick_best_source=(mode != "first"), chunk=16)
    rows = gold[f"grid.{mode}.rows"]
    np.testing.assert_array_equal(res["source_rows"].cpu().numpy(), rows)
    assert torch.equal(res["sources"].cpu(), X[torch.from_numpy(rows)])
    if mode != "first":
        np.testing.assert_allclose(res["source_conf"].cpu().numpy(), gold[f"grid.{mode}.row_conf"][rows], rtol=1e-4, atol=2e-5)
        assert not gold[f"grid.{mode}.pick_undecided"].any()
    if mode == "late":
        assert (rows != RR.pick(Y.numpy(), 10)[0]).sum() >= 5 and len(gold["grid.late.row_conf"]) == 40
    cells, und = gold[f"grid.{mode}.cells"], gold[f"grid.{mode}.undecided"]
    assert und.sum() <= 0.05 * 90
    image = res["image"].cpu().numpy()
    got = image.reshape(10, 28, 10, 28).transpose(0, 2, 1, 3)
    atol = 0.5 * 2e-5 * float(gold[f"grid.{mode}.raw_scale"])
    print(f"{mode}: max cell error {np.abs(got - cells).max():.3e}, atol {atol:.3e}")
    np.testing.assert_allclose(got, cells, rtol=1e-4, atol=atol)
    d = np.arange(10)
    np.testing.assert_array_equal(got[d, d], cells[d, d])                                  # the sources, bit for bit
    np.testing.assert_array_equal(res["image_u8"].cpu().numpy(), RR.to_u8(image))
    off = ~np.eye(10, dtype=bool)
    np.testing.assert_array_equal(res["pred"][off & ~und], gold[f"grid.{mode}.pred"][off & ~und])
    np.testing.assert_allclose(res["conf"][off], gold[f"grid.{mode}.conf"][off], rtol=1e-4, atol=2e-5)
    assert res["pred"][d, d].tolist() == d.tolist() and (res["conf"][d, d] == 1.0).all() and res["hit"][d, d].all()   # :176-178
    np.testing.assert_array_equal(res["hit"][off], (res["pred"] == d[None, :])[off])
    # the same launches as one sweep over the sources: the same bits, [source][target]
    sw = K.counterfactual_sweep(G, C, res["sources"])
    assert tuple(res["x_cf"].shape) == (10, 10, 1, 28, 28) and torch.equal(res["x_cf"], sw["x_cf"].transpose(0, 1))
    want_img, _ = RR.grid_image(res["sources"].cpu().numpy()[:, 0], sw["x_cf"].cpu().numpy()[:, :, 0])
    np.testing.assert_array_equal(image, want_img)
    text = K.grid_csv(res).splitlines()
    assert text[0] == "source,target,pred,conf,hit" and len(text) == 101 and text[1] == "0,0,0,1.0,1"


# ---- 5. the additive-delta grids ------------------------------------------------------------------------------------------------------------
def _rule(got, want64, dist, what):
    want64 = np.asarray(want64, np.float64)
    atol = max(2e-5 * float(np.abs(want64).max()), 3.0 * float(np.max(dist)))
    print(f"{what}: max error {float(np.abs(np.asarray(got, np.float64) - want64).max()):.3e}, atol {atol:.3e}")
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=atol, err_msg=what)


@pytest.mark.parametrize("which", ["gan_train", "countergan2"])
def test_delta_grid_against_the_restatement(K, synth, which):
    import countergan2_restate as C2
    import delta_gan_restate as RS
    import pool_clf_restate as PR
    from pcgan_amd import countergan2, gan_train
    mod, rs = (gan_train, RS) if which == "gan_train" else (countergan2, C2)
    X, Y = synth[0][:60], synth[1][:60].clone()
    Y[50:] = torch.arange(10)                                                       # every class has a row
    torch.manual_seed(RS.SEED_GAN)
    G = mod.Generator().to(DEV)
    C = K.Classifier()
    C.load_state_dict(PR.seeded_state(PR.SEED), strict=True)
    C = C.to(DEV).eval()
    for best in (False, True):
        res = gan_train.counterfactual_grid(G, C, (X.to(DEV), Y.to(DEV)), pick_best_source=best, chunk=32)
        ref = {}
        for dt in (torch.float64, torch.float32):
            G_ref, _ = rs.seeded_nets(dt)
            ref[dt] = RR.delta_grid(G_ref, RS.classifier_state(dt), X, Y.numpy(), best, dt)
        r64, r32 = ref[torch.float64], ref[torch.float32]
        if best:                                                                    # the pick is decided in the restatement itself
            assert np.array_equal(r64["rows"], r32["rows"])
        np.testing.assert_array_equal(res["source_rows"].cpu().numpy(), r64["rows"])
        x_cf = res["x_cf"].cpu().numpy().transpose(1, 0, 2, 3, 4)                   # back to [target][row]
        _rule(x_cf, r64["x_cf"], np.abs(r32["x_cf"] - r64["x_cf"]), f"{which} x_cf")
        off = ~np.eye(10, dtype=bool)
        _rule(res["conf"].T[off], r64["confs"][off], np.abs(r32["confs"] - r64["confs"]), f"{which} conf")
        top = np.sort(r64["probs"], -1)
        near = (top[..., -1] - top[..., -2]) < max(1e-6, 100.0 * float(np.abs(r32["probs"] - r64["probs"]).max()))
        assert near.mean() <= 0.05
        np.testing.assert_array_equal(res["pred"].T[off & ~near], r64["preds"][off & ~near])
        want_img, want_u8 = RR.grid_image(res["sources"].cpu().numpy()[:, 0], x_cf[:, :, 0])
        np.testing.assert_array_equal(res["image"].cpu().numpy(), want_img)
        np.testing.assert_array_equal(res["image_u8"].cpu().numpy(), want_u8)
        d = np.arange(10)
        assert res["pred"][d, d].tolist() == d.tolist() and (res["conf"][d, d] == 1.0).all() and res["hit"][d, d].all()


# ---- 6. heat-map panels ----------------------------------------------------------------------------------------------------------------------
def test_heatmap_batch_and_user_modification_example(K, nets, gold):
    G, C = nets
    x = torch.from_numpy(gold["grid.x"][:3]).to(DEV)
    patches = [1, 5, 10, 12, 13, 14]
    q = K.counterfactuals(G, C, x, 4, patches=patches, patch_size=7)
    hb = K.heatmap_batch(x, q["x_cf"], q["mask"], classifier=C)
    want, wmax = RR.panels(x.cpu().numpy()[:, 0], q["x_cf"].cpu().numpy()[:, 0], q["mask"].cpu().numpy()[0, 0])
    np.testing.assert_array_equal(hb["panels"].cpu().numpy(), want)
    assert float(hb["vmax"]) == float(wmax) > 0
    assert torch.equal(hb["pred"], q["pred"]) and torch.equal(hb["conf"], q["conf"])
    assert K.heatmap_batch(x, q["x_cf"], q["mask"], max_samples=2)["panels"].shape == (2, 4, 28, 28)
    rowmask = q["mask"].expand(3, 1, 28, 28).contiguous()
    rowmask[1] = 0.0
    hr = K.heatmap_batch(x, q["x_cf"], rowmask)
    np.testing.assert_array_equal(hr["panels"].cpu().numpy(), RR.panels(x.cpu().numpy()[:, 0], q["x_cf"].cpu().numpy()[:, 0], rowmask.cpu().numpy()[:, 0])[0])
    um = K.user_modification_example(x, patches, G, C, 4, patch_size=7)
    one = K.counterfactuals(G, C, x[:1].contiguous(), 4, patches=patches, patch_size=7)
    w1, m1 = RR.panels(x.cpu().numpy()[:1, 0], one["x_cf"].cpu().numpy()[:, 0], one["mask"].cpu().numpy()[0, 0])
    np.testing.assert_array_equal(um["panels"].cpu().numpy(), w1)
    assert float(um["vmax"]) == float(m1) and torch.equal(um["pred"], one["pred"]) and torch.equal(um["conf"], one["conf"])
    assert torch.equal(um["mask"], one["mask"]) and um["panels"].shape == (1, 4, 28, 28)
    with pytest.raises(K.PcgError):
        K.heatmap_batch(x, q["x_cf"][:2], q["mask"])


# ---- 7. house.case_studies -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def house(golden_dir):
    from pcgan_amd import house as H
    C = H.NNClassifier(17, 4)
    C.load_state_dict(torch.load(os.path.join(golden_dir, "house_classifier_trained.pt"), map_location="cpu", weights_only=True))
    return H, C.to(DEV).eval()


def test_case_studies_against_the_reference(house, gold, tmp_path):
    H, C = house
    names = json.loads(str(gold["case.feature_names"]))
    und = gold["case.undecided"]
    out = str(tmp_path / "case_studies")
    tables = H.case_studies(C, gold["case.originals"], gold["case.cfs"], {"feature_names": names},
                            scaler=HT._Scaler(gold["case.data_min"], gold["case.data_max"]), n_samples=20, save_dir=out)
    HT.check_case_tables(gold, names, tables, skip_rows=set(np.flatnonzero(und).tolist()), gain_tol=(2e-4, 2e-5))
    assert not und.any()                                                                # so every row's decisions were compared
    written = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert written == HT.expected_files(gold)
    with open(os.path.join(out, "case_study_sample_summary.csv")) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 20 and list(rows[0]) == list(H.SAMPLE_FIELDS) and rows[0]["topk_features"] == tables[0][0]["topk_features"]
    with open(os.path.join(out, "case_study_aggregate_summary.csv")) as f:
        agg = list(csv.DictReader(f))
    assert len(agg) == 1 and agg[0]["topk_features_global"] == tables[2]["topk_features_global"] and list(agg[0]) == list(H.AGGREGATE_FIELDS)


# ---- 8. the pipelines ------------------------------------------------------------------------------------------------------------------------
def test_mnist_pipeline_with_and_without_the_grid(K, nets, gold, tmp_path):
    from PIL import Image
    G, C = nets
    X, Y = torch.from_numpy(gold["grid.x"]), torch.from_numpy(gold["grid.y"])
    loader = [(X[i:i + 8], Y[i:i + 8]) for i in range(0, 16, 8)]
    out = {}
    for grid in (False, True):
        cfg = type("Cfg", (K.Config,), {"device": DEV, "save_dir": str(tmp_path / f"grid{int(grid)}")})
        np.random.seed(4); torch.manual_seed(4)
        out[grid] = (K.evaluate_pipeline(G, C, (X, Y), loader, cfg, verbose=False, grid=True) if grid else
                     K.evaluate_pipeline(G, C, (X, Y), loader, cfg, verbose=False))
    base = {"countergan_metrics.csv", "countergan_metrics_per_class.csv"}
    assert set(os.listdir(tmp_path / "grid0")) == base
    assert set(os.listdir(tmp_path / "grid1")) == base | {"cf_grid.npy", "cf_grid.png", "cf_grid.csv"}
    assert out[False] == out[True]
    for name in base:
        assert open(tmp_path / "grid0" / name).read() == open(tmp_path / "grid1" / name).read()
    img = np.load(tmp_path / "grid1" / "cf_grid.npy")
    assert img.shape == (280, 280) and img.dtype == np.float32 and 0.0 <= img.min() and img.max() <= 1.0
    with Image.open(tmp_path / "grid1" / "cf_grid.png") as im:
        np.testing.assert_array_equal(np.asarray(im), RR.to_u8(img))
    with open(tmp_path / "grid1" / "cf_grid.csv") as f:
        cells = list(csv.DictReader(f))
    assert len(cells) == 100 and list(cells[0]) == ["source", "target", "pred", "conf", "hit"]
    assert all(c["pred"] == c["source"] and c["hit"] == "1" and float(c["conf"]) == 1.0 for c in cells if c["source"] == c["target"])


def test_house_pipeline_with_and_without_case_studies(house, golden_dir, tmp_path):
    H, C = house
    g = dict(np.load(os.path.join(golden_dir, "house_eval.npz")))
    cfg0 = dict(H.CONFIG)
    cfg0["categorical_info"] = {f: {"n": len(g[f"raw_values.{f}"]), "raw_values": g[f"raw_values.{f}"].tolist()} for f in H.CONFIG["categorical_info"]}
    cfg0["scaler"] = HT._Scaler(g["scaler.data_min"], g["scaler.data_max"])
    G = H.ResidualGenerator(17, 32, 4, cfg0["continuous_idx"], cfg0["categorical_info"], tau=0.5)
    G.load_state_dict(torch.load(os.path.join(golden_dir, "house_generator_trained.pt"), map_location="cpu", weights_only=True))
    e = {"H": H, "gold": g, "cfg": cfg0, "G": G.to(DEV).eval(), "C": C}
    X, y = e["gold"]["X_test"][:120], e["gold"]["y_test"][:120]
    rows = {}
    for on in (False, True):
        e["G"].rng = None
        cfg = dict(e["cfg"], out_dir=str(tmp_path / f"cs{int(on)}"), batch_size=64, feature_names=H.FEATURES, case_study_n=6)
        torch.manual_seed(8)
        rows[on] = H.evaluate_pipeline(e["G"], e["C"], X, y, cfg, case_studies=True) if on else H.evaluate_pipeline(e["G"], e["C"], X, y, cfg)
    e["G"].rng = None
    base = {"countergan_metrics.csv", "feature_shift_importance.csv", "class_pair_sensitivity"}
    assert set(os.listdir(tmp_path / "cs0")) == base and set(os.listdir(tmp_path / "cs1")) == base | {"case_studies"}
    assert rows[False] == rows[True]
    cs = tmp_path / "cs1" / "case_studies"
    assert {"case_study_sample_summary.csv", "case_study_feature_summary.csv", "case_study_aggregate_summary.csv", "samples"} == set(os.listdir(cs))
    with open(cs / "case_study_sample_summary.csv") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 6 and list(got[0]) == list(H.SAMPLE_FIELDS)
    per = [os.path.join(d, f) for d, _, fs in os.walk(cs / "samples") for f in fs]
    assert len(per) == 6 and all(os.path.basename(os.path.dirname(p)) == f"src{r['source_pred']}_tgt{r['intended_target']}"
                                 for r in got for p in per if os.path.basename(p) == f"sample_{r['sample_idx_in_vis']}_features.csv")
    with open(per[0]) as f:
        assert len(list(csv.DictReader(f))) == 17
