"""Host-side checks (no GPU) of the full-resolution MNIST CounteRGAN port (pcgan_amd.countergan2, csrc/prob_head.hip): the restatement
(tests/countergan2_restate.py) pinned to the reference's own recorded runs (tests/golden/countergan2_ref.npz), the ABI additions, the
refusals of both new entries before any HIP call, the modules' state_dict contract and the "no CPU path" errors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countergan2_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

NEW_SYMBOLS = ("pcg_prob_head_workspace_bytes", "pcg_prob_head_fwd", "pcg_log_eps_loss_fwd_bwd")
NEW_STRUCTS = ("pcg_prob_head_fwd_args", "pcg_log_eps_loss_args")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "countergan2_ref.npz")))


@pytest.fixture(scope="module")
def runs():
    return {(B, dt): RS.run(B, dt) for B in (4, 3) for dt in (torch.float32, torch.float64)}


def _stored(gold, key):
    return (gold[key + ".full"], False) if key + ".full" in gold else (gold[key + ".digest"], True)


def _same_form(t, digest):
    return RS.digest(t) if digest else t.detach().double().numpy()


# ---- the restatement against the reference's recorded runs --------------------------------------------------------------------------------
def test_seeds_rebuild_the_recorded_weights(gold):
    G, D = RS.seeded_nets()
    for net, sd in (("G", G.state_dict()), ("D", D.state_dict()), ("C", PR.seeded_state(PR.SEED))):
        for k, v in sd.items():
            np.testing.assert_allclose([float(v.double().sum()), float(v.double().abs().sum())],
                                       [float(gold[f"init.{net}.{k}.sum"]), float(gold[f"init.{net}.{k}.abssum"])], rtol=1e-12, atol=1e-12,
                                       err_msg=f"{net} {k}")
    assert tuple(G.state_dict()) == RS.G_KEYS and tuple(D.state_dict()) == RS.D_KEYS
    assert tuple(tuple(v.shape) for v in G.state_dict().values()) == RS.G_SHAPES
    assert tuple(tuple(v.shape) for v in D.state_dict().values()) == RS.D_SHAPES


@pytest.mark.parametrize("B", [4, 3])
def test_restatement_reproduces_the_recording(gold, runs, B):
    for i, (x, y) in enumerate(RS.batches(B)):
        assert np.array_equal(x.numpy(), gold[f"B{B}.step{i}.x"]) and np.array_equal(y.numpy(), gold[f"B{B}.step{i}.y"])
    (s64, G64, D64), (s32, G32, D32) = runs[(B, torch.float64)], runs[(B, torch.float32)]
    for name in RS.LOSSES:
        l64, l32 = np.asarray([s[name] for s in s64]), np.asarray([s[name] for s in s32])
        np.testing.assert_allclose(l64, gold[f"B{B}.{name}.f64"], rtol=1e-9, err_msg=name)
        assert (np.abs(l32 - gold[f"B{B}.{name}.f64"]) <= 3.0 * gold[f"B{B}.{name}.dist"] + 1e-12).all(), (name, l32, gold[f"B{B}.{name}.f64"])
    for name in RS.FORWARD:
        want = gold[f"B{B}.{name}.f64"]
        np.testing.assert_allclose(s64[0][name].numpy(), want, rtol=1e-9, atol=1e-12 * np.abs(want).max(), err_msg=name)
        assert np.abs(s32[0][name].double().numpy() - want).max() <= 3.0 * float(gold[f"B{B}.{name}.dist"]), name
    for net, keys, m64, m32 in (("G", RS.G_KEYS, G64, G32), ("D", RS.D_KEYS, D64, D32)):
        sd64, sd32 = m64.state_dict(), m32.state_dict()
        for k in keys:
            for what, t64, t32 in (("grad", s64[0][f"grad_{net}"][k], s32[0][f"grad_{net}"][k]), ("final", sd64[k], sd32[k])):
                want, dig = _stored(gold, f"B{B}.{what}.{net}.{k}")
                scale = np.abs(want[2:] if dig else want).max()
                np.testing.assert_allclose(_same_form(t64, dig), want, rtol=1e-9, atol=1e-11 * max(scale, abs(want[1]) if dig else scale),
                                           err_msg=f"{what} {net} {k}")
                if not dig:
                    assert np.abs(_same_form(t32, False) - want).max() <= 3.0 * float(gold[f"B{B}.{what}.{net}.{k}.dist"]), (what, net, k)
                else:
                    assert np.abs(_same_form(t32, True)[2:] - want[2:]).max() <= 3.0 * float(gold[f"B{B}.{what}.{net}.{k}.dist"]), (what, net, k)


def test_recorded_distances_are_inside_the_makers_bounds(gold):
    """The fixture's own statement of the reference's fp32 error: every loss within 2e-6 relative, every parameter gradient within
    2.5e-5 * max|gradient| of float64; at most 0.2 % of the live pooling windows under the gap bound."""
    worst = max(float(gold[k]) / float(gold[k[:-5] + ".max"]) for k in gold if ".grad." in k and k.endswith(".dist"))
    assert 0 < worst <= 2.5e-5
    for B in (4, 3):
        for name in RS.LOSSES:
            assert (gold[f"B{B}.{name}.dist"] <= 2e-6 * np.abs(gold[f"B{B}.{name}.f64"])).all(), name
        for layer in (1, 2):
            assert gold[f"B{B}.near{layer}"].sum() <= 0.002 * gold[f"B{B}.live{layer}"].sum()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_structs_and_version():
    from pcgan_amd import _lib, ops
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
    assert _lib.PROTOTYPES["pcg_prob_head_fwd"] == (ctypes.c_int, [ctypes.POINTER(_lib.ProbHeadFwdArgs), ctypes.c_void_p])
    assert _lib.PROTOTYPES["pcg_log_eps_loss_fwd_bwd"] == (ctypes.c_int, [ctypes.POINTER(_lib.LogEpsLossArgs), ctypes.c_void_p])
    assert _lib.PROTOTYPES["pcg_prob_head_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32])
    assert lib.pcg_abi_version() == 7
    assert lib.pcg_prob_head_workspace_bytes(256, 4) == 16 + 4 * 256 * 4
    assert lib.pcg_prob_head_workspace_bytes(256, 1) == 16 + 4 * 256
    assert lib.pcg_prob_head_workspace_bytes(256, 0) == 16 + 4 * 256 and lib.pcg_prob_head_workspace_bytes(129, 0) == 16 + 4 * 129
    assert lib.pcg_prob_head_workspace_bytes(128, 0) == 16 + 4 * 128 * 2                           # the header's rule: 2 slabs up to 128 rows
    assert lib.pcg_prob_head_workspace_bytes(0, 1) == 0 and lib.pcg_prob_head_workspace_bytes(4, 17) == 0
    assert lib.pcg_prob_head_workspace_bytes(4, -1) == 0 and lib.pcg_prob_head_workspace_bytes(65536, 1) == 0
    assert (_lib.PROB_HEAD_D, _lib.PROB_HEAD_G, _lib.PROB_HEAD_MAX_SLABS) == (0, 1, 16) and ops.LOG_EPS == 1e-6
    for const in ("PCG_PROB_HEAD_D 0", "PCG_PROB_HEAD_G 1", "PCG_PROB_HEAD_MAX_SLABS 16"):
        assert "#define " + const in header, const


def _fake(n=64):
    """A host buffer standing in for device memory: 16-byte aligned, never touched (the entries refuse before any HIP call)."""
    raw = ctypes.create_string_buffer(n + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, addr


def test_both_entries_refuse_bad_arguments_before_any_hip_call():
    from pcgan_amd import _lib
    lib = _lib.load()
    keep, p = _fake()
    err = lambda: lib.pcg_last_error().decode()      # noqa: E731
    INV, WS = -1, -2                                  # PCG_ERR_INVALID / PCG_ERR_WORKSPACE: a launch attempt here would give PCG_ERR_LAUNCH instead

    def head(**kw):
        base = dict(a=p, w=p, bias=p, logits=p, prob=p, loss=p, dlogit=p, db=p, workspace=p, workspace_bytes=1 << 20, eps=1e-6, R=4, F=50176,
                    mode=0, slabs=0)
        base.update(kw)
        return _lib.ProbHeadFwdArgs(**base)

    def loss(**kw):
        base = dict(p=p, grad_out=None, loss=p, dp=p + 16, eps=1e-6, R=4, mode=0)
        base.update(kw)
        return _lib.LogEpsLossArgs(**base)

    H, L = lib.pcg_prob_head_fwd, lib.pcg_log_eps_loss_fwd_bwd
    cases = [
        (H, None, "null"), (H, head(R=0), "rows"), (H, head(R=65536), "rows"), (H, head(R=3), "odd"), (H, head(mode=2), "mode"),
        (H, head(F=50178), "multiple of 4"), (H, head(F=0), "multiple of 4"), (H, head(a=p + 4), "aligned"), (H, head(w=p + 8), "aligned"),
        (H, head(slabs=17), "slabs"), (H, head(slabs=-1), "slabs"), (H, head(eps=0.0), "eps"), (H, head(eps=-1e-6), "eps"),
        (H, head(eps=float("nan")), "eps"),
    ] + [(H, head(**{k: None}), "null") for k in ("a", "w", "bias", "logits", "prob", "loss", "dlogit", "db", "workspace")] + [
        (L, None, "null"), (L, loss(R=0), "rows"), (L, loss(R=5), "odd"), (L, loss(mode=-1), "mode"), (L, loss(p=None), "null"),
        (L, loss(loss=None, dp=None), "neither"), (L, loss(eps=0.0), "eps"), (L, loss(dp=p), "out of place"),
    ]
    for fn, args, what in cases:
        rc = fn(ctypes.byref(args) if args is not None else None, None)
        assert rc == INV and what in err(), (fn.__name__, what, rc, err())
    for kw in (dict(workspace_bytes=16 + 4 * 4 * 2 - 1, slabs=2), dict(workspace_bytes=8, slabs=0), dict(workspace_bytes=16 + 4 * 3, slabs=1)):
        rc = H(ctypes.byref(head(**kw)), None)
        assert rc == WS and "workspace" in err(), (kw, rc, err())
    del keep                                          # (no accepted call is made here: the buffers are not device memory)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_the_reference_layer_lists():
    from pcgan_amd import countergan2 as T
    for mine, theirs, keys, shapes in ((T.Generator(), RS.TorchGenerator(), RS.G_KEYS, RS.G_SHAPES),
                                       (T.Discriminator(), RS.TorchDiscriminator(), RS.D_KEYS, RS.D_SHAPES)):
        assert tuple(mine.state_dict()) == keys
        assert tuple(tuple(v.shape) for v in mine.state_dict().values()) == shapes
        theirs.load_state_dict(mine.state_dict(), strict=True)
        torch.manual_seed(11)
        fresh = type(theirs)()
        mine.load_state_dict(fresh.state_dict(), strict=True)
        assert all(torch.equal(mine.state_dict()[k], fresh.state_dict()[k]) for k in keys)
        assert [type(m).__name__ for m in mine.net] == [type(m).__name__ for m in theirs.net]
    assert type(T.Discriminator().net[6]).__name__ == "Sigmoid"
    torch.manual_seed(RS.SEED_GAN)                      # same constructor draws in the same order as the reference's classes
    G, D = T.Generator(), T.Discriminator()
    G0, D0 = RS.seeded_nets()
    assert all(torch.equal(G.state_dict()[k], G0.state_dict()[k]) for k in RS.G_KEYS)
    assert all(torch.equal(D.state_dict()[k], D0.state_dict()[k]) for k in RS.D_KEYS)


def test_params_and_refusals_that_need_no_gpu():
    from pcgan_amd import PcgError, countergan as K, countergan2 as T, gan_train
    assert T.params(5) == {"batch_size": 128, "epochs": 50, "lr_G": 1e-3, "lr_D": 1e-3, "lambda_cls": 3.0, "lambda_reg": 0.05, "device": "cuda",
                           "target": 5}
    with pytest.raises(PcgError, match="outside 0..9"):
        T.params(10)
    G, D, C = T.Generator(), T.Discriminator(), K.Classifier().eval()
    x, y = torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64)
    P = T.params(5)
    with pytest.raises(PcgError, match="no CPU path"):
        G(x, y)
    with pytest.raises(PcgError, match="no CPU path"):
        D(x, y)
    with pytest.raises(PcgError, match="no CPU path"):
        T.counterfactual_batch(G, x, 5)
    with pytest.raises(PcgError, match="no CPU path"):
        T.delta_image(x)
    with pytest.raises(PcgError, match="no CPU path"):
        T.train_step(G, D, C, None, None, x, y, y, P)
    with pytest.raises(PcgError, match="no CPU path"):
        T.GraphedTrainStep(G, D, C, 4, P)
    with pytest.raises(PcgError, match="no CPU path"):
        T.train_gan(G, D, C, [(x, y)], dict(P, epochs=1), verbose=False)
    with pytest.raises(PcgError, match="GPU"):
        T.ops.prob_head_fwd(torch.zeros(2, 8), torch.zeros(8), torch.zeros(1))
    with pytest.raises(PcgError, match="GPU"):
        T.ops.log_eps_loss_fwd_bwd(torch.full((2,), 0.5))
    with pytest.raises(PcgError, match="eval mode"):
        T.GraphedTrainStep(G, D, K.Classifier().train(), 4, P)
    assert "not countergan2.Generator" in T.GraphedTrainStep.unsupported(gan_train.Generator(), D, C)
    assert "not countergan2.Generator" in T.GraphedTrainStep.unsupported(G, gan_train.Discriminator(), C)
    assert "not gan_train.Generator" in gan_train.GraphedTrainStep.unsupported(G, gan_train.Discriminator(), C)     # the twin does not take these nets
    C.conv_precision = "bf16"
    assert "fp32 only" in T.GraphedTrainStep.unsupported(G, D, C)
    with pytest.raises(NotImplementedError):
        D.conv_precision = "bf16"                       # bf16 operands are out of scope for these nets
