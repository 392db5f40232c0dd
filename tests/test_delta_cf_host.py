"""Host-side checks (no GPU) of the additive-delta CounteRGAN's prompted half (pcgan_amd.gan_train, csrc/delta_cf_eval.hip; DESIGN.md
§3.20): the restatement (tests/delta_cf_restate.py) pinned to the reference's own recorded runs (tests/golden/delta_cf_ref.npz), the
host model of the class draw, the fold, the ABI additions, every entry's refusals before any HIP call and every refusal of the front
ends."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_cf_restate as CR  # noqa: E402
import delta_gan_restate as RS  # noqa: E402

NEW_SYMBOLS = ("pcg_delta_cf_entry", "pcg_delta_cf_tail", "pcg_delta_gan_target_draw")
NEW_STRUCTS = ("pcg_delta_cf_entry_args", "pcg_delta_cf_tail_args", "pcg_delta_gan_target_draw_args")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "delta_cf_ref.npz")))


def _pinned(got64, got32, want, dist, what):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(np.asarray(got64, np.float64), want, rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(want).max())), err_msg=what)
    assert np.abs(np.asarray(got32, np.float64) - want).max() <= 3.0 * float(np.max(dist)) + 1e-12, what     # rule (b), as the GPU tests apply it


# ---- the restatement against the reference's recorded runs --------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 3])
def test_random_target_iterations_reproduce_the_recording(gold, B):
    classes = CR.drawn_classes(int(gold["meta.steps"]))
    assert classes == gold[f"B{B}.classes"].tolist() and len(set(classes)) > 1
    _, r64, _, _ = CR.run_random_target(B, torch.float64)
    _, r32, _, _ = CR.run_random_target(B, torch.float32)
    for name in CR.LOSSES:
        _pinned([s[name] for s in r64], [s[name] for s in r32], gold[f"B{B}.{name}.f64"], gold[f"B{B}.{name}.dist"], name)


@pytest.mark.parametrize("B", [4, 3])
def test_queries_sweep_and_metrics_reproduce_the_recording(gold, B):
    x, y, q64, s64 = CR.recorded_queries(B, torch.float64)
    _, _, q32, s32 = CR.recorded_queries(B, torch.float32)
    assert np.array_equal(x.numpy(), gold[f"B{B}.x"].astype(np.float64)) and np.array_equal(y.numpy(), gold[f"B{B}.y"])
    assert np.array_equal(CR.query_targets(B).numpy(), gold[f"B{B}.query.targets"])
    for k in ("x_cf", "delta", "probs", "confs"):
        _pinned(q64[k].numpy(), q32[k].numpy(), gold[f"B{B}.query.{k}.f64"], gold[f"B{B}.query.{k}.dist"], "query " + k)
    assert np.array_equal(q64["preds"].numpy(), gold[f"B{B}.query.preds.f64"])
    for k in ("probs", "confs"):
        _pinned(s64[k].numpy(), s32[k].numpy(), gold[f"B{B}.sweep.{k}.f64"], gold[f"B{B}.sweep.{k}.dist"], "sweep " + k)
    if B == 4:
        _pinned(s64["delta"].numpy(), s32["delta"].numpy(), gold["B4.sweep.delta.f64"], gold["B4.sweep.delta.dist"], "sweep delta")
    near = gold[f"B{B}.sweep.near"]
    assert np.array_equal(s64["preds"].numpy(), gold[f"B{B}.sweep.preds.f64"])
    assert np.array_equal(s32["preds"].numpy()[~near], gold[f"B{B}.sweep.preds.f64"][~near])
    _pinned(CR.query_sums(x, s64["x_cf"], s64["delta"]).numpy(), CR.query_sums(x.float(), s32["x_cf"], s32["delta"]).numpy(),
            gold[f"B{B}.sweep.sums.f64"], gold[f"B{B}.sweep.sums.dist"], "sums")
    m64, m32 = CR.per_target_metrics(x, y, s64), CR.per_target_metrics(x.float(), y, s32)
    for k in CR.METRICS:
        dist = gold[f"B{B}.sweep.{k}.dist"] + (near.sum(1) / B if k == "class_flip_rate" else 0.0)
        _pinned(m64[k], m32[k], gold[f"B{B}.sweep.{k}.f64"], dist, k)


@pytest.mark.parametrize("B", [4, 3])
def test_the_condition_on_discrete_outputs_holds_in_the_recording(gold, B):
    near, gap, bound = gold[f"B{B}.sweep.near"], gold[f"B{B}.sweep.gap"], float(gold[f"B{B}.sweep.bound"])
    assert bound >= 1e-6 and np.array_equal(near, gap < bound)
    n = near.sum() + gold[f"B{B}.query.near"].sum()
    assert n <= CR.NEAR_CAP * (near.size + gold[f"B{B}.query.near"].size)
    p32, p64 = gold[f"B{B}.sweep.preds.f32"], gold[f"B{B}.sweep.preds.f64"]
    assert np.array_equal(p32[~near], p64[~near])
    hits = p64 == np.arange(CR.K)[:, None]
    assert hits.any() and not hits.all(), "the per-row query test needs a hit and a miss"
    for layer in (1, 2):                                                        # DESIGN.md §3.18's routing precondition on the query rows
        assert gold[f"B{B}.sweep.routing.near{layer}"] <= 0.002 * gold[f"B{B}.sweep.routing.live{layer}"]


def test_fold_is_the_mean_over_batches_of_per_batch_means(gold):
    """gan_train._fold_eval on group sums built from the recorded float64 sweep equals the restated fold: a ragged batch weighs as
    much as a full one."""
    from pcgan_amd import countergan as CG, gan_train as T
    per, groups = [], []
    for B in (4, 3):
        x, y, _, s64 = CR.recorded_queries(B, torch.float64)
        per.append(CR.per_target_metrics(x, y, s64))
        rows = torch.arange(B)
        g = np.zeros((CR.K, 1, 8))
        for t in range(CR.K):
            p = s64["probs"][t]
            flip = (s64["preds"][t] == t).double()
            g[t, 0] = [flip.sum(), flip.max(), (p[rows, t] - p[rows, y]).sum(), 0.0, *gold[f"B{B}.sweep.sums.f64"][t].sum(0), B]
        groups.append(g)
    want = CR.fold(per)
    got = T._fold_eval(np.concatenate(groups, axis=1))
    assert sorted(got) == list(range(CR.K)) and tuple(got[0]) == T.EVAL_FIELDS == CR.METRICS
    for k in CR.METRICS:
        np.testing.assert_allclose([got[t][k] for t in range(CR.K)], want[k], rtol=1e-12, atol=1e-15, err_msg=k)
    not_pooled = (4 * per[0]["actionability"] + 3 * per[1]["actionability"]) / 7
    assert np.abs(want["actionability"] - not_pooled).max() > 0
    text = CG.per_class_csv(got, fields=T.EVAL_FIELDS)                          # usable with countergan.per_class_csv, default fields too
    assert text.splitlines()[0] == "," + ",".join(T.EVAL_FIELDS) and len(text.splitlines()) == 1 + CR.K
    assert CG.per_class_csv(got).splitlines()[0] == "," + ",".join(CG.PER_CLASS_FIELDS)
    with pytest.raises(T.PcgError, match="no batch"):
        T._fold_eval(np.zeros((CR.K, 1, 8)))


def test_host_model_of_the_class_draw():
    """The draw's host model is oracle.rng_np.randint(1, 0, K, seed, offset)[0]: one counter value per draw, the first word of it."""
    from oracle import rng_np
    from pcgan_amd import ops
    for seed, off in ((0, 0), (3, 1), (3, 2 ** 32 - 1), (2 ** 63 + 5, 2 ** 32)):
        out, _, rng = rng_np.randint(1, 0, CR.K, seed, off)
        quad = rng_np.draw(seed, off, np.arange(1, dtype=np.uint64))
        assert int(out[0]) == (int(quad[0, 0]) * CR.K) >> 32 and 0 <= int(out[0]) < CR.K
        assert tuple(int(v) for v in rng) == (off, off + 1)
    r = ops.DeviceRNG(5)
    assert r._advance(1) == 0 and r.offset == 1                                 # randint(.., n = 1)'s span: (1 + 3) // 4
    seen = {int(rng_np.randint(1, 0, CR.K, 5, o)[0][0]) for o in range(64)}
    assert len(seen) == CR.K


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_structs_and_version():
    from pcgan_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pcgan_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and hasattr(raw, name) and name + "(" in header, name
    for name in NEW_STRUCTS:
        assert name in _lib.STRUCTS and "} " + name + ";" in header, name
        assert lib.pcg_abi_struct_bytes(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0, name
    assert lib.pcg_abi_version() == 7
    assert [ctypes.sizeof(_lib.STRUCTS[n]) for n in NEW_STRUCTS] == [5 * 8 + 6 * 4, 4 * 8 + 5 * 4 + 4, 4 * 8 + 2 * 4]


def _fake(n=64):
    """A host buffer standing in for device memory: 16-byte aligned, never touched (the entries refuse before any HIP call)."""
    raw = ctypes.create_string_buffer(n + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, addr


def test_every_new_entry_refuses_bad_arguments_before_any_hip_call():
    from pcgan_amd import _lib
    lib = _lib.load()
    keep, p = _fake()
    err = lambda: lib.pcg_last_error().decode()      # noqa: E731
    INV = -1                                          # PCG_ERR_INVALID: a launch attempt on this machine would give PCG_ERR_LAUNCH instead

    def entry(**kw):
        base = dict(x=p, table=p, target=None, target_host=None, out=p, B=3, T=10, HW=784, K=10, q0=0, nq=30)
        base.update(kw)
        return _lib.DeltaCfEntryArgs(**base)

    def tail(**kw):
        base = dict(delta=p, x=p, x_cf=p, sums=p, B=3, T=10, HW=784, q0=0, nq=30)
        base.update(kw)
        return _lib.DeltaCfTailArgs(**base)

    def draw(**kw):
        base = dict(target=p, counter=None, seed=1, offset=0, B=4, K=10)
        base.update(kw)
        return _lib.DeltaGanTargetDrawArgs(**base)

    bad = (ctypes.c_int64 * 3)(3, 10, 0)
    neg = (ctypes.c_int64 * 3)(0, -1, 0)
    cases = [
        (lib.pcg_delta_cf_entry, None, "null"), (lib.pcg_delta_cf_entry, entry(x=None), "null"), (lib.pcg_delta_cf_entry, entry(out=None), "null"),
        (lib.pcg_delta_cf_entry, entry(HW=783), "multiple of 4"), (lib.pcg_delta_cf_entry, entry(K=0), "K 0"),
        (lib.pcg_delta_cf_entry, entry(q0=7, nq=24), "window"), (lib.pcg_delta_cf_entry, entry(nq=0), "window"),
        (lib.pcg_delta_cf_entry, entry(q0=-1), "window"), (lib.pcg_delta_cf_entry, entry(B=0), "window"),
        (lib.pcg_delta_cf_entry, entry(T=11, nq=33), "sweep T <= K"), (lib.pcg_delta_cf_entry, entry(target=p), "T = 1"),
        (lib.pcg_delta_cf_entry, entry(T=1, nq=3, target_host=ctypes.addressof(bad)), "target is null"),
        (lib.pcg_delta_cf_entry, entry(T=1, nq=3, target=p, target_host=ctypes.addressof(bad)), "label 10 of row 1"),
        (lib.pcg_delta_cf_entry, entry(T=1, nq=3, target=p, target_host=ctypes.addressof(neg)), "label -1 of row 1"),
        (lib.pcg_delta_cf_entry, entry(out=p + 4), "aligned"),
        (lib.pcg_delta_cf_tail, None, "null"), (lib.pcg_delta_cf_tail, tail(delta=None), "null"), (lib.pcg_delta_cf_tail, tail(sums=None), "null"),
        (lib.pcg_delta_cf_tail, tail(HW=786), "multiple of 4"), (lib.pcg_delta_cf_tail, tail(q0=25, nq=6), "window"),
        (lib.pcg_delta_cf_tail, tail(x=p + 8), "aligned"), (lib.pcg_delta_cf_tail, tail(x_cf=p + 4), "aligned"),
        (lib.pcg_delta_gan_target_draw, None, "null"), (lib.pcg_delta_gan_target_draw, draw(target=None), "null target"),
        (lib.pcg_delta_gan_target_draw, draw(B=0), "batch of 0"), (lib.pcg_delta_gan_target_draw, draw(K=0), "0 classes"),
        (lib.pcg_delta_gan_target_draw, draw(counter=p + 4), "aligned"),
    ]
    for fn, args, what in cases:
        rc = fn(ctypes.byref(args) if args is not None else None, None)
        assert rc == INV and what in err(), (fn.__name__, what, rc, err())
    del keep                                          # (no accepted call is made here: the buffers are not device memory)


# ---- the front ends' refusals, all on the host -------------------------------------------------------------------------------------------------
def test_params_random_target():
    from pcgan_amd import gan_train as T
    assert T.params_random_target == {"batch_size": 128, "epochs_clf": 10, "epochs_gan": 50, "lr_G": 5e-5, "lr_D": 1e-5, "lr_C": 1e-3,
                                      "lambda_cls": 2.0, "lambda_reg": 0.01, "device": "cuda"}
    assert "target_class" not in T.params_random_target and T.params["target_class"] == 5


def test_refusals_that_need_no_gpu():
    from pcgan_amd import PcgError, countergan as K, gan_train as T, ops
    G, D, C = T.Generator(), T.Discriminator(), K.Classifier().eval()
    x, y = torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64)
    for call in (lambda: T.counterfactuals(G, C, x, 3), lambda: T.counterfactual_sweep(G, C, x), lambda: T.evaluate_examples(G, C, x, y),
                 lambda: T.evaluate_per_target(G, C, [(x, y)], verbose=False), lambda: G.forward_queries(x.view(2, 784), None)):
        with pytest.raises(PcgError, match="no CPU path"):
            call()
    with pytest.raises(PcgError, match="query_chunk 0"):
        T.counterfactuals(G, C, x, 3, query_chunk=0)
    with pytest.raises(PcgError, match="query_chunk -2"):
        T.counterfactual_sweep(G, C, x, query_chunk=-2)
    with pytest.raises(PcgError, match="query_chunk 0"):
        T.evaluate_per_target(G, C, [(x, y)], query_chunk=0, verbose=False)
    rp = dict(T.params_random_target, epochs_gan=1)
    with pytest.raises(PcgError, match="eval mode"):
        T.train_gan(G, D, K.Classifier().train(), [(x, y)], rp, rng=ops.DeviceRNG(1), verbose=False)
    with pytest.raises(PcgError, match="no CPU path"):
        T.train_gan(G, D, C, [(x, y)], rp, rng=ops.DeviceRNG(1), verbose=False)
    with pytest.raises(PcgError, match="no CPU path"):
        T.GraphedTrainStep(G, D, C, 4, rp, rng=ops.DeviceRNG(1))


class _OnGpu:
    """Stands in for the device check alone: the refusals below are host logic that comes after it."""

    def __init__(self, monkeypatch, T):
        monkeypatch.setattr(T, "_check_query_nets", lambda G, C, imgs, who, query_chunk=1: None)


def test_label_refusals_are_host_side(monkeypatch):
    from pcgan_amd import PcgError, gan_train as T
    dev = torch.device("cpu")
    assert T._query_labels(3, 4, 10, dev, "target").tolist() == [3, 3, 3, 3]
    assert T._query_labels([1, 2, 9, 0], 4, 10, dev, "target").tolist() == [1, 2, 9, 0]
    assert T._query_labels(None, 4, 10, dev, "y_true") is None
    for bad, what in ((10, "outside 0..9"), (-1, "outside 0..9"), ([0, 1, 2], "expected 4 labels, got 3"), (torch.tensor([0, 1, 2, 10]), "outside 0..9"),
                      (torch.zeros(5, dtype=torch.int64), "expected 4 labels, got 5")):
        with pytest.raises(PcgError, match=what):
            T._query_labels(bad, 4, 10, dev, "target")
    G, C = T.Generator(), __import__("pcgan_amd").countergan.Classifier().eval()
    _OnGpu(monkeypatch, T)
    x = torch.zeros(4, 1, 28, 28)
    with pytest.raises(PcgError, match="outside 0..9"):
        T.counterfactuals(G, C, x, 10)
    with pytest.raises(PcgError, match="expected 4 labels, got 2"):
        T.counterfactuals(G, C, x, [1, 2])
    with pytest.raises(PcgError, match="expected 4 labels, got 3"):
        T.evaluate_examples(G, C, x, targets=[1, 2, 3])
    with pytest.raises(PcgError, match="no rng"):
        T.evaluate_examples(G, C, x)


def test_real_query_check_refuses_training_classifier_and_class_mismatch():
    from pcgan_amd import PcgError, countergan as K, gan_train as T

    class OnGpu:                                        # what the check reads of a tensor and of a net, without a GPU
        is_cuda, shape = True, (2, 1, 28, 28)

        def dim(self):
            return 4

        def numel(self):
            return 2 * 784

    class Net(T.Generator):
        def parameters(self):
            return iter([type("P", (), {"device": torch.device("cuda:0")})()])

    class Clf:
        training, num_classes = True, 10

        def parameters(self):
            return iter([type("P", (), {"device": torch.device("cuda:0")})()])

    real = torch.is_tensor
    try:
        torch.is_tensor = lambda t: isinstance(t, OnGpu) or real(t)
        with pytest.raises(PcgError, match="training mode"):
            T._check_query_nets(Net(), Clf(), OnGpu(), "counterfactuals")
        Clf.training, Clf.num_classes = False, 7
        with pytest.raises(PcgError, match="embeds 10 classes, the classifier has 7"):
            T._check_query_nets(Net(), Clf(), OnGpu(), "counterfactuals")
        Clf.num_classes = 10
        T._check_query_nets(Net(), Clf(), OnGpu(), "counterfactuals")
        with pytest.raises(PcgError, match="not gan_train.Generator"):
            T._check_query_nets(Clf(), Clf(), OnGpu(), "counterfactuals")
    finally:
        torch.is_tensor = real
    assert K.Classifier().eval().num_classes == 10


def test_target_source_fixed_class_never_draws_and_the_other_refusals(monkeypatch):
    """train_gan's target source: with target_class set it fills once per batch size and never calls the draw (today's path); an
    iterable that runs out, a class outside the table, targets next to a fixed class, and a missing rng are refused on the host."""
    from pcgan_amd import PcgError, gan_train as T, ops
    calls = []
    monkeypatch.setattr(ops, "delta_gan_target_draw", lambda *a, **k: calls.append((a, k)) or a[0])
    dev = torch.device("cpu")
    rng = ops.DeviceRNG(3)
    src = T._TargetSource(T.params, 10, dev, rng=rng)
    a, b, c = src.next(4), src.next(3), src.next(4)
    assert a.tolist() == [5] * 4 and b.tolist() == [5] * 3 and c is a and not calls and rng.offset == 0
    src = T._TargetSource(T.params_random_target, 10, dev, targets=[1, 9, 0])
    assert [src.next(4).tolist()[0] for _ in range(3)] == [1, 9, 0] and not calls
    with pytest.raises(PcgError, match="ran out at iteration 4"):
        src.next(4)
    with pytest.raises(PcgError, match="class 10 of iteration 1 is outside 0..9"):
        T._TargetSource(T.params_random_target, 10, dev, targets=[10]).next(2)
    with pytest.raises(PcgError, match="target_class"):
        T._TargetSource(T.params, 10, dev, targets=[1])
    with pytest.raises(PcgError, match="rng"):
        T._TargetSource(T.params_random_target, 10, dev)
    assert T._TargetSource(T.params_random_target, 10, dev, rng=rng, in_step=True).next(4) is None and not calls and rng.offset == 0
    src = T._TargetSource(T.params_random_target, 10, dev, rng=rng)              # the op chain: offset by value, rng.offset advances
    src.next(4); src.next(4)
    assert [k["offset"] for _, k in calls] == [0, 1] and rng.offset == 2 and all(k.get("counter") is None for _, k in calls)
    import inspect
    sig = inspect.signature(T.train_gan)
    assert list(sig.parameters) == ["G", "D", "C", "train_loader", "params", "fused", "rng", "targets", "verbose"]
    assert "_TargetSource(" in inspect.getsource(T.train_gan)


def test_restated_sums_match_their_definition():
    x = torch.tensor([[[[0.5, -0.5], [1.0, 0.0]]]], dtype=torch.float64)
    d = torch.tensor([[[[0.75, -0.25], [0.5, 0.0]]]], dtype=torch.float64)
    cf = torch.clamp(x + d, -1, 1)
    np.testing.assert_allclose(CR.query_sums(x, cf, d).numpy(), [[0.5 + 0.25 + 0.0 + 0.0, 1.5, 0.25 + 0.0625]], rtol=1e-15)
    assert RS.TARGET_CLASS == 5
