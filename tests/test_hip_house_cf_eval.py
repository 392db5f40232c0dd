"""GPU: the tabular CounteRGAN's prompted queries and evaluation in one launch (csrc/house_cf_eval.hip through pcgan_amd.house,
DESIGN.md §3.12) against a float64 oracle — oracle/house_ref.py's modules in .double() on the CPU, eval mode, with the shipped
checkpoints of tests/golden — and against the reference's own recorded results (house_eval.npz, house_cf_eval_ref.npz).

Tolerances.  Per-row values: test_hip_moons_cf_eval.py's, rtol 1e-5, atol 1e-6 + 1e-5 max|ref|.  A sum: the sum of its rows'
tolerances.  Chosen categories and predicted classes are compared exactly wherever the float64 top-2 margin (of logit + noise for a
head, of the logits for a class) is >= 1e-4; the inputs leave no row under that, which every test asserts.  Against the reference's
recorded fp32 results: the existing evaluation test's, rtol 2e-4 / atol 2e-5 for metrics and rtol 1e-4 / atol 2e-5 for rows.

Input A: the first 83 rows of the test split (groups of 32, 32, 19 rows at group 32: a partial last tile), seeded noise and prompt
masks.  Input B: the exact case of house_eval.npz (512 rows, the reference's recorded draws)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-4
NA = 83
FLOAT_OUTS = ("cont", "logits", "masked_residual", "x_cf", "x_cf_raw", "logits_cf", "logits_x", "gain")
ROW_OUTS = FLOAT_OUTS + ("chosen", "pred_cf", "pred_x")


class _Scaler:
    def __init__(self, lo, hi):
        self.data_min_, self.data_max_ = lo, hi


@pytest.fixture(scope="module")
def env():
    import pcgan_amd
    from oracle import house_ref as R
    from pcgan_amd import house as H
    pcgan_amd.load()
    gold = dict(np.load(os.path.join(GOLD, "house_eval.npz")))
    cfg = dict(H.CONFIG)
    cfg["categorical_info"] = {f: {"n": len(gold[f"raw_values.{f}"]), "raw_values": gold[f"raw_values.{f}"].tolist()} for f in H.CONFIG["categorical_info"]}
    cfg["scaler"] = _Scaler(gold["scaler.data_min"], gold["scaler.data_max"])
    sd_g = torch.load(os.path.join(GOLD, "house_generator_trained.pt"), map_location="cpu", weights_only=True)
    sd_c = torch.load(os.path.join(GOLD, "house_classifier_trained.pt"), map_location="cpu", weights_only=True)
    G = H.ResidualGenerator(17, 32, 4, cfg["continuous_idx"], cfg["categorical_info"], tau=0.5)
    C = H.NNClassifier(17, 4)
    G.load_state_dict(sd_g); C.load_state_dict(sd_c)
    oG = R.ResidualGenerator(17, 32, 4, R.CONFIG["continuous_idx"], R.CONFIG["categorical_info"], tau=0.5)
    oC = R.NNClassifier(17, 4)
    oG.load_state_dict(sd_g); oC.load_state_dict(sd_c)
    norm = H.cat_norm_maps(G, cfg, "cpu").double()                            # the float32 values the kernel reads
    e = {"pcg": pcgan_amd, "H": H, "gold": gold, "cfg": cfg, "G": G.to(DEV).eval(), "C": C.to(DEV).eval(), "oG": oG.double().eval(),
         "oC": oC.double().eval(), "norm": norm, "seg": G.seg, "cat_idx": G.cat_idx, "cont_idx": G.continuous_idx}
    g = torch.Generator().manual_seed(11)
    e["noiseA"] = -torch.empty(4, NA, 70).exponential_(generator=g).log()
    pm = torch.randint(0, 2, (NA, 17), generator=g).float()
    pm[:, cfg["immutable_idx"]] = 0.0
    e["pmaskA"] = pm
    e["XA"], e["yA"] = gold["X_test"][:NA], gold["y_test"][:NA]
    assert np.bincount(e["yA"]).tolist() == [17, 20, 17, 29]
    e["ref_cache"] = {}
    return e


def margin(v):
    top = torch.topk(v, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).numpy()


def oracle(e, x, t, mk, noise):
    """x [N][17] float32, t [N] int64, mk [N][17] float32, noise [N][70] float32 (numpy / tensors) -> per-row values in float64."""
    with torch.no_grad():
        xd, m, tt, nz = (v.clone() if torch.is_tensor(v) else torch.tensor(np.asarray(v)) for v in (x, mk, t, noise))
        xd, m, tt, nz = xd.double(), m.double(), tt.long(), nz.double()
        seg, cat_idx = e["seg"], e["cat_idx"]
        gd = {f: nz[:, seg[s]:seg[s + 1]] for s, f in enumerate(cat_idx)}
        cont, lg, smp = e["oG"](xd, F.one_hot(tt, 4).double(), m, gd, temperature=e["cfg"]["gumbel_tau"], hard=True)
        logits = torch.cat([lg[f] for f in cat_idx], 1)
        chosen = torch.stack([smp[f].argmax(1) for f in cat_idx], 1)
        head_margin = np.stack([margin(lg[f] + gd[f]) for f in cat_idx], 1)
        res = torch.zeros_like(xd)
        for i, f in enumerate(e["cont_idx"]):
            res[:, f] = cont[:, i]
        for s, f in enumerate(cat_idx):
            res[:, f] = e["norm"][seg[s]:seg[s + 1]][chosen[:, s]] - xd[:, f]
        masked = res * m
        raw = xd + masked
        cf = raw.clamp(0.0, 1.0)
        lx, lraw, lcl = e["oC"](xd), e["oC"](raw), e["oC"](cf)
        ar = torch.arange(len(tt))
        px = F.softmax(lx, 1)[ar, tt]
        return {"cont": cont.numpy(), "logits": logits.numpy(), "chosen": chosen.numpy(), "head_margin": head_margin,
                "masked_residual": masked.numpy(), "x_cf_raw": raw.numpy(), "x_cf": cf.numpy(), "logits_x": lx.numpy(),
                "pred_x": lx.argmax(1).numpy(), "margin_x": margin(lx),
                0: {"logits_cf": lraw.numpy(), "pred_cf": lraw.argmax(1).numpy(), "margin_cf": margin(lraw), "gain": (F.softmax(lraw, 1)[ar, tt] - px).numpy()},
                1: {"logits_cf": lcl.numpy(), "pred_cf": lcl.argmax(1).numpy(), "margin_cf": margin(lcl), "gain": (F.softmax(lcl, 1)[ar, tt] - px).numpy()}}


def oracle_A(e, t, which):
    """The oracle of input A, slot t, mask 'plain' (the config's) or 'prompt' (per row): computed once, shared, never changed."""
    key = (t, which)
    if key not in e["ref_cache"]:
        mk = e["pmaskA"].numpy() if which == "prompt" else np.broadcast_to(e["H"].prompt_mask(e["cfg"]), (NA, 17))
        e["ref_cache"][key] = oracle(e, e["XA"], np.full(NA, t), mk, e["noiseA"][t])
    return e["ref_cache"][key]


def row_tol(ref):
    return 1e-5 * np.abs(ref) + 1e-6 + 1e-5 * np.abs(ref).max()


def assert_rows(ours, ref, clamp, what):
    """Every per-row output of one slot against the oracle; nothing may be left out of the exact comparisons."""
    rc = dict(ref, **ref[int(clamp)])
    for k in FLOAT_OUTS:
        got = ours[k].cpu().numpy()
        err = np.abs(got - rc[k])
        print(f"{what} {k}: max error / tolerance = {(err / row_tol(rc[k])).max():.3f}")
        assert (err <= row_tol(rc[k])).all(), f"{what} {k}: max error {err.max():.3e}"
    for k, mg in (("chosen", "head_margin"), ("pred_cf", "margin_cf"), ("pred_x", "margin_x")):
        print(f"{what} {k}: smallest float64 margin {rc[mg].min():.2e}")
        assert (rc[mg] >= MARGIN).all(), f"{what} {k}: {int((rc[mg] < MARGIN).sum())} entries under the margin would be left out"
        assert np.array_equal(ours[k].cpu().numpy(), rc[k]), f"{what} {k}"


def slot(out, t):
    return {k: (out[k] if k in ("logits_x", "pred_x") else out[k][t]) for k in ROW_OUTS}


def sweep_A(e, which, group=32, clamp=False, **kw):
    H = e["H"]
    mask = e["pmaskA"] if which == "prompt" else None
    return H.counterfactual_sweep(e["G"], e["C"], e["XA"], e["yA"], e["cfg"], mask=mask, batch_size=group, gumbel=e["noiseA"],
                                  outputs=H.CF_ROW_OUTPUTS, clamp_cls=clamp, **kw)


def bitwise_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---- case 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "prompt"])
def test_sweep_rows_match_the_float64_oracle(env, which):
    e = env
    out = sweep_A(e, which)
    mk = e["pmaskA"].numpy() if which == "prompt" else np.broadcast_to(e["H"].prompt_mask(e["cfg"]), (NA, 17))
    x, off = torch.from_numpy(e["XA"]), torch.from_numpy(mk == 0)
    for t in range(4):
        assert_rows(slot(out, t), oracle_A(e, t, which), False, f"{which} t={t}")
        md, raw = out["masked_residual"][t].cpu(), out["x_cf_raw"][t].cpu()
        assert (md[off] == 0).all(), "a masked-out column moved"
        assert torch.equal(raw[off].view(torch.int32), x[off].view(torch.int32)), "x_cf_raw differs from x in a masked-out column"
    assert off.any() and (~off).any()


# ---- case 2 --------------------------------------------------------------------------------------------------------------------------
def test_per_row_form_and_second_run_are_bitwise_the_sweep(env):
    e = env
    H = e["H"]
    a = sweep_A(e, "prompt", clamp=True)
    b = sweep_A(e, "prompt", clamp=True)
    for k in a:
        assert bitwise_equal(a[k], b[k]), f"second run differs in {k}"
    for t in range(4):
        q = H.counterfactuals(e["G"], e["C"], e["XA"], t, e["cfg"], mask=e["pmaskA"], gumbel=e["noiseA"][t])
        assert sorted(q) == sorted(H.CF_ROW_OUTPUTS) == sorted(ROW_OUTS)
        for k, v in slot(a, t).items():
            assert bitwise_equal(q[k], v), f"per-row form differs from the sweep in {k}, target {t}"
    # mixed per-row targets: row i asks for class i % 4 and gets slot (i % 4)'s row
    tt = torch.arange(NA) % 4
    noise = torch.stack([e["noiseA"][int(tt[i]), i] for i in range(NA)])
    q = H.counterfactuals(e["G"], e["C"], e["XA"], tt, e["cfg"], mask=e["pmaskA"], gumbel=noise)
    for k in ("masked_residual", "x_cf", "logits_cf", "gain", "chosen", "pred_cf"):
        want = torch.stack([a[k][int(tt[i]), i] for i in range(NA)])
        assert bitwise_equal(q[k], want), f"mixed targets: {k}"


@pytest.mark.parametrize("group", [1, 32, 83])
def test_group_does_not_change_the_rows(env, group):
    e = env
    base = env.setdefault("group_base", sweep_A(e, "plain", group=16))
    out = sweep_A(e, "plain", group=group)
    for k in e["H"].CF_ROW_OUTPUTS:
        assert bitwise_equal(out[k], base[k]), f"group {group}: {k} differs"
    n_tiles = {1: 83, 32: 6, 83: 6}[group]
    assert out["tile_sums"].shape == (4, n_tiles, 4)


@pytest.mark.parametrize("group", [32, 83, 20])
def test_sums_equal_a_host_recomputation(env, group):
    e = env
    out = sweep_A(e, "prompt", group=group, class_sums=True)
    y = e["yA"]
    tpg = -(-min(group, NA) // 16)
    n_groups = -(-NA // group)
    assert out["tile_sums"].shape == (4, n_groups * tpg, 4) and out["class_sums"].shape == (4, n_groups * tpg, 4, 17)
    ts, cs, cc = out["tile_sums"].cpu().numpy(), out["class_sums"].cpu().numpy(), out["class_counts"].cpu().numpy()
    for t in range(4):
        gain = out["gain"][t].cpu().numpy().astype(np.float64)
        am = np.abs(out["masked_residual"][t].cpu().numpy().astype(np.float64))
        flip = out["pred_cf"][t].cpu().numpy() == t
        tol_g, tol_m = row_tol(gain), row_tol(am)
        for q in range(n_groups * tpg):
            g, j = divmod(q, tpg)
            lo = g * group + 16 * j
            hi = max(lo, min(lo + 16, (g + 1) * group, NA))
            rows = np.arange(lo, hi)
            inc = rows[y[rows] != t]
            assert ts[t, q, 0] == len(inc) and ts[t, q, 1] == flip[inc].sum(), (t, q)
            assert abs(ts[t, q, 2] - gain[inc].sum()) <= tol_g[inc].sum() + 1e-30, (t, q)
            assert abs(ts[t, q, 3] - am[inc].sum()) <= tol_m[inc].sum() + 1e-30, (t, q)
            for c in range(4):
                rc = rows[y[rows] == c]
                assert cc[t, q, c] == len(rc)
                assert (np.abs(cs[t, q, c] - am[rc].sum(0)) <= tol_m[rc].sum(0) + 1e-30).all(), (t, q, c)
    # and the fold: the metrics of the reference's loop over these groups, from the per-row outputs
    got = e["H"].metrics_from_sums(ts, group)
    for t in range(4):
        per = []
        for g in range(n_groups):
            rows = np.arange(g * group, min((g + 1) * group, NA))
            inc = rows[y[rows] != t]
            if len(inc):
                per.append(((out["pred_cf"][t].cpu().numpy()[inc] == t).mean(), out["gain"][t].cpu().numpy().astype(np.float64)[inc].mean(),
                            np.abs(out["masked_residual"][t].cpu().numpy().astype(np.float64))[inc].mean()))
        np.testing.assert_allclose(got[t], np.mean(per, 0), rtol=1e-5, atol=1e-7)


# ---- case 3 --------------------------------------------------------------------------------------------------------------------------
def test_clamp_cls_changes_only_rows_that_leave_the_unit_box(env):
    e = env
    raw = sweep_A(e, "plain", clamp=False)
    cl = sweep_A(e, "plain", clamp=True)
    for k in ("cont", "logits", "chosen", "masked_residual", "x_cf", "x_cf_raw", "logits_x", "pred_x"):
        assert bitwise_equal(raw[k], cl[k]), k
    inside = ((raw["x_cf_raw"] >= 0) & (raw["x_cf_raw"] <= 1)).all(-1)
    assert inside.any() and (~inside).any(), "the input must have rows on both sides"
    for k in ("logits_cf", "gain", "pred_cf"):
        assert torch.equal(raw[k][inside], cl[k][inside]), f"{k} changed in a row that stays inside [0, 1]"
    assert not torch.equal(raw["logits_cf"][~inside], cl["logits_cf"][~inside])
    for t in range(4):
        assert_rows(slot(raw, t), oracle_A(e, t, "plain"), False, f"unclamped t={t}")
        assert_rows(slot(cl, t), oracle_A(e, t, "plain"), True, f"clamped t={t}")


# ---- case 4 --------------------------------------------------------------------------------------------------------------------------
def test_one_launch_metrics_exact_case(env):
    e = env
    H, gold, G, C = e["H"], e["gold"], e["G"], e["C"]
    n = int(gold["meta.exact_rows"])
    noise = [G.pack_noise({f: torch.from_numpy(gold[f"exact.gumbel.{t}.{f}"]).to(DEV) for f in G.cat_idx}) for t in range(4)]
    cfg = dict(e["cfg"], batch_size=n)
    X, y = gold["X_test"][:n], gold["y_test"][:n]
    # nothing under the margin in the rows the metrics count (float64 oracle on the recorded draws)
    for t in range(4):
        sel = y != t
        ref = oracle(e, X[sel], np.full(int(sel.sum()), t), np.broadcast_to(H.prompt_mask(cfg), (int(sel.sum()), 17)), noise[t].cpu())
        assert ref["head_margin"].min() >= MARGIN and ref[0]["margin_cf"].min() >= MARGIN
    res, orig, cfs = H.compute_metrics_per_target(G, C, X, y, cfg, gumbel_per_call=noise, max_vis=10 ** 9, one_launch=True)
    got = np.array([[r["class_flip"], r["prediction_gain"], r["avg_actionability"]] for r in res])
    assert [r["target_class"] for r in res] == [0, 1, 2, 3]
    np.testing.assert_allclose(got, gold["exact.metrics"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(cfs, gold["exact.x_cf"], rtol=1e-4, atol=2e-5)
    res2, orig2, cfs2 = H.compute_metrics_per_target(G, C, X, y, cfg, gumbel_per_call=noise, max_vis=10 ** 9)      # the chain
    got2 = np.array([[r["class_flip"], r["prediction_gain"], r["avg_actionability"]] for r in res2])
    np.testing.assert_allclose(got, got2, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(cfs, cfs2, rtol=1e-4, atol=2e-5)
    np.testing.assert_array_equal(orig, orig2)
    # max_vis cuts at whole calls, as the chain does
    _, o3, c3 = H.compute_metrics_per_target(G, C, X, y, cfg, gumbel_per_call=noise, max_vis=500, one_launch=True)
    _, o4, c4 = H.compute_metrics_per_target(G, C, X, y, cfg, gumbel_per_call=noise, max_vis=500)
    assert o3.shape == o4.shape == c3.shape == c4.shape
    np.testing.assert_array_equal(o3, o4)


def test_one_launch_metrics_many_batches_same_draws_as_the_chain(env):
    """Batches of 32 over input A (the last one short, targets with different row counts per batch): the rng path lays the chain's
    own per-call draws, so both paths see the same noise."""
    e = env
    H = e["H"]
    cfg = dict(e["cfg"], batch_size=32)
    one = H.compute_metrics_per_target(e["G"], e["C"], e["XA"], e["yA"], cfg, rng=e["pcg"].ops.DeviceRNG(5), one_launch=True)
    e["G"].rng = None
    chain = H.compute_metrics_per_target(e["G"], e["C"], e["XA"], e["yA"], cfg, rng=e["pcg"].ops.DeviceRNG(5))
    e["G"].rng = None
    a = np.array([[r[k] for k in H.METRIC_FIELDS] for r in one[0]])
    b = np.array([[r[k] for k in H.METRIC_FIELDS] for r in chain[0]])
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5)
    np.testing.assert_array_equal(one[1], chain[1])
    np.testing.assert_allclose(one[2], chain[2], rtol=1e-4, atol=2e-5)


# ---- case 5 --------------------------------------------------------------------------------------------------------------------------
def test_one_launch_full_run_agrees_with_shipped_metrics(env):
    e = env
    H, gold = e["H"], e["gold"]
    e["G"].rng = None
    res, _, _ = H.compute_metrics_per_target(e["G"], e["C"], gold["X_test"], gold["y_test"], dict(e["cfg"], batch_size=int(gold["meta.batch_size"])),
                                             rng=e["pcg"].ops.DeviceRNG(7), one_launch=True)
    e["G"].rng = None
    got = np.array([[r["class_flip"], r["prediction_gain"], r["avg_actionability"]] for r in res])
    print(got)
    assert np.abs(got - gold["shipped.metrics"]).max() < 0.01, got
    assert np.abs(got - gold["full.metrics"]).max() < 0.01, got


# ---- case 6 --------------------------------------------------------------------------------------------------------------------------
def test_queries_and_sensitivity_match_the_reference(env):
    e = env
    H, gold = e["H"], e["gold"]
    ref = dict(np.load(os.path.join(GOLD, "house_cf_eval_ref.npz")))
    X = gold["X_test"]
    for r in range(ref["gradio.target"].shape[0]):
        allowed = [a for a in str(ref["gradio.allowed"][r]).split(",") if a] or None
        np.testing.assert_array_equal(H.prompt_mask(e["cfg"], allowed), ref["gradio.immutable_mask"][r])
        o = oracle(e, X[:NA], ref["gradio.target"][r], np.broadcast_to(ref["gradio.immutable_mask"][r], (NA, 17)), ref["gradio.gumbel"][r])
        assert o["head_margin"].min() >= MARGIN and o[1]["margin_cf"].min() >= MARGIN
        q = H.counterfactuals(e["G"], e["C"], X[:NA], ref["gradio.target"][r], e["cfg"], mask=H.prompt_mask(e["cfg"], allowed),
                              gumbel=torch.from_numpy(ref["gradio.gumbel"][r]))
        np.testing.assert_allclose(q["masked_residual"].cpu().numpy(), ref["gradio.masked_residual"][r], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(q["x_cf"].cpu().numpy(), ref["gradio.x_cf"][r], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(F.softmax(q["logits_x"], 1).cpu().numpy(), ref["gradio.probs_x"], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(F.softmax(q["logits_cf"], 1).cpu().numpy(), ref["gradio.probs_cf"][r], rtol=2e-4, atol=2e-5)
    S = ref["sens.gumbel"].shape[1]
    deltas = H.analyze_class_pair_sensitivity(e["G"], e["C"], X[:S], gold["y_test"][:S], e["cfg"], gumbel=torch.from_numpy(ref["sens.gumbel"]))
    assert deltas.shape == (4, 4, 17) and (deltas[np.arange(4), np.arange(4)] == 0).all()
    np.testing.assert_allclose(deltas, ref["sens.deltas"], rtol=2e-4, atol=2e-5)


# ---- the wrappers around the launch ---------------------------------------------------------------------------------------------------
def test_evaluate_classifier_and_pipeline(env, tmp_path):
    e = env
    H, gold = e["H"], e["gold"]
    X, y = gold["X_test"][:200], gold["y_test"][:200]
    r = H.evaluate_classifier(e["C"], X, y, class_names=["q1", "q2", "q3", "q4"])
    with torch.no_grad():
        pred = e["oC"](torch.from_numpy(X).double()).argmax(1).numpy()
    sure = margin(e["oC"](torch.from_numpy(X).double()).detach()) >= MARGIN
    assert sure.all()
    np.testing.assert_array_equal(r["confusion_matrix"], H.confusion_matrix(y, pred))
    assert r["accuracy"] == pytest.approx((pred == y).mean()) and "weighted avg" in r["report"]
    e["G"].rng = None
    cfg = dict(e["cfg"], out_dir=str(tmp_path / "out"), batch_size=64, feature_names=H.FEATURES)
    rows = H.evaluate_pipeline(e["G"], e["C"], X, y, cfg)
    e["G"].rng = None
    lines = open(tmp_path / "out" / "countergan_metrics.csv").read().splitlines()
    assert lines[0] == "target_class,class_flip,prediction_gain,avg_actionability" and len(lines) == 5
    assert [float(v) for v in lines[1].split(",")[1:]] == [rows[0][k] for k in H.METRIC_FIELDS]
    shift = open(tmp_path / "out" / "feature_shift_importance.csv").read().splitlines()
    assert shift[0] == "feature,mean_abs_change_norm,mean_pct_of_range,mean_abs_change_denorm" and len(shift) == 18
    assert np.load(tmp_path / "out" / "class_pair_sensitivity" / "deltas.npy").shape == (4, 4, 17)
