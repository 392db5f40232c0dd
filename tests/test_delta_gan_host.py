"""Host-side checks (no GPU) of the additive-delta MNIST CounteRGAN port (pcgan_amd.gan_train, csrc/delta_gan.hip): the restatement
(tests/delta_gan_restate.py) pinned to the reference's own recorded runs (tests/golden/delta_gan_ref.npz), the ABI additions, the
refusals of every new entry before any HIP call, the modules' state_dict contract and the "no CPU path" errors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_gan_restate as RS  # noqa: E402
import pool_clf_restate as PR  # noqa: E402

NEW_SYMBOLS = ("pcg_delta_gan_entry", "pcg_delta_gan_tail_workspace_bytes", "pcg_delta_gan_tail_fwd", "pcg_logit_head_fwd", "pcg_logit_head_bwd",
               "pcg_delta_gan_tail_bwd")
NEW_STRUCTS = ("pcg_delta_gan_entry_args", "pcg_delta_gan_tail_fwd_args", "pcg_logit_head_fwd_args", "pcg_logit_head_bwd_args",
               "pcg_delta_gan_tail_bwd_args")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "delta_gan_ref.npz")))


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
    for name in ("delta", "x_cf", "d_real", "d_fake", "d_fake_g", "cls_logits"):
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


def test_recorded_gradients_pass_rule_b_where_they_miss_rule_a(gold):
    """The fixture's own statement of the reference's fp32 error: every parameter gradient within 2.5e-5 * max|gradient| of float64."""
    worst = max(float(gold[k]) / float(gold[k[:-5] + ".max"]) for k in gold if ".grad." in k and k.endswith(".dist"))
    assert 0 < worst <= 2.5e-5


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
    assert lib.pcg_delta_gan_tail_workspace_bytes(128, 784) == 16 + 4 * 98
    assert lib.pcg_delta_gan_tail_workspace_bytes(0, 784) == 0


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
        base = dict(x=p, y=p, target=p, table_g=p, table_d=p, g_in=p, d_in=p, B=2, HW=784, K=10, mode=0)
        base.update(kw)
        return _lib.DeltaGanEntryArgs(**base)

    def tail_fwd(**kw):
        base = dict(x=p, delta=p, x_cf=p, d_in=p, loss_reg=p, workspace=p, workspace_bytes=1 << 20, B=2, HW=784, grid=0)
        base.update(kw)
        return _lib.DeltaGanTailFwdArgs(**base)

    def head_fwd(**kw):
        base = dict(a=p, w=p, bias=p, logits=p, loss=p, dlogit=p, db=p, workspace=p, R=4, F=12544, mode=0)
        base.update(kw)
        return _lib.LogitHeadFwdArgs(**base)

    def head_bwd(**kw):
        base = dict(a=p, w=p, dlogit=p, da=p, dw=p, slope=0.2, R=4, F=12544, dw_C=0, dw_P=0)
        base.update(kw)
        return _lib.LogitHeadBwdArgs(**base)

    def tail_bwd(**kw):
        base = dict(dD=p, dC=p, delta=p, d_delta=p, lambda_cls=3.0, reg_scale=1e-5, B=2, HW=784, dD_stride=1)
        base.update(kw)
        return _lib.DeltaGanTailBwdArgs(**base)

    bad_y = (ctypes.c_int64 * 2)(3, 10)
    neg_t = (ctypes.c_int64 * 2)(-1, 5)
    ok_y = (ctypes.c_int64 * 2)(0, 9)
    cases = [
        (lib.pcg_delta_gan_entry, None, "null"), (lib.pcg_delta_gan_entry, entry(B=0), "batch"), (lib.pcg_delta_gan_entry, entry(x=None), "null"),
        (lib.pcg_delta_gan_entry, entry(d_in=None), "null"), (lib.pcg_delta_gan_entry, entry(mode=2), "mode"),
        (lib.pcg_delta_gan_entry, entry(y_host=ctypes.addressof(bad_y)), "label 10"),
        (lib.pcg_delta_gan_entry, entry(y_host=ctypes.addressof(ok_y), target_host=ctypes.addressof(neg_t)), "label -1"),
        (lib.pcg_delta_gan_entry, entry(mode=1, x=None, y=None, table_g=None, g_in=None, target_host=ctypes.addressof(bad_y)), "label 10"),
        (lib.pcg_delta_gan_entry, entry(head_w=p), "go together"),
        (lib.pcg_delta_gan_tail_fwd, None, "null"), (lib.pcg_delta_gan_tail_fwd, tail_fwd(B=0), "batch"),
        (lib.pcg_delta_gan_tail_fwd, tail_fwd(delta=None), "null"), (lib.pcg_delta_gan_tail_fwd, tail_fwd(HW=783), "multiple of 4"),
        (lib.pcg_delta_gan_tail_fwd, tail_fwd(x=p + 4), "aligned"), (lib.pcg_delta_gan_tail_fwd, tail_fwd(grid=5000), "grid"),
        (lib.pcg_logit_head_fwd, None, "null"), (lib.pcg_logit_head_fwd, head_fwd(R=0), "rows"), (lib.pcg_logit_head_fwd, head_fwd(R=3), "odd"),
        (lib.pcg_logit_head_fwd, head_fwd(w=None), "null"), (lib.pcg_logit_head_fwd, head_fwd(F=12543), "multiple of 4"),
        (lib.pcg_logit_head_fwd, head_fwd(mode=7), "mode"),
        (lib.pcg_logit_head_bwd, None, "null"), (lib.pcg_logit_head_bwd, head_bwd(R=0), "rows"), (lib.pcg_logit_head_bwd, head_bwd(da=None), "null"),
        (lib.pcg_logit_head_bwd, head_bwd(dw_C=256, dw_P=48), "does not cover"),
        (lib.pcg_delta_gan_tail_bwd, None, "null"), (lib.pcg_delta_gan_tail_bwd, tail_bwd(B=0), "batch"),
        (lib.pcg_delta_gan_tail_bwd, tail_bwd(dC=None), "null"), (lib.pcg_delta_gan_tail_bwd, tail_bwd(dD_stride=3), "dD_stride"),
    ]
    for fn, args, what in cases:
        rc = fn(ctypes.byref(args) if args is not None else None, None)
        assert rc == INV and what in err(), (fn.__name__, what, rc, err())
    rc = lib.pcg_delta_gan_tail_fwd(ctypes.byref(tail_fwd(workspace_bytes=8)), None)
    assert rc == -2 and "workspace" in err()                                   # PCG_ERR_WORKSPACE
    del keep                                          # (no accepted call is made here: the buffers are not device memory)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_the_reference_layer_lists():
    from pcgan_amd import gan_train as T
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
    torch.manual_seed(RS.SEED_GAN)                      # same constructor draws in the same order as the reference's modules
    G, D = T.Generator(), T.Discriminator()
    G0, D0 = RS.seeded_nets()
    assert all(torch.equal(G.state_dict()[k], G0.state_dict()[k]) for k in RS.G_KEYS)
    assert all(torch.equal(D.state_dict()[k], D0.state_dict()[k]) for k in RS.D_KEYS)


def test_params_and_refusals_that_need_no_gpu():
    from pcgan_amd import PcgError, countergan as K, gan_train as T
    assert T.params == {"batch_size": 128, "epochs_clf": 10, "epochs_gan": 40, "lr_G": 1e-3, "lr_D": 1e-3, "lr_C": 1e-3, "lambda_cls": 3.0,
                        "lambda_reg": 0.05, "target_class": 5, "device": "cuda"}
    G, D, C = T.Generator(), T.Discriminator(), K.Classifier().eval()
    x, y = torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(PcgError, match="no CPU path"):
        G(x, y)
    with pytest.raises(PcgError, match="no CPU path"):
        D(x, y)
    with pytest.raises(PcgError, match="no CPU path"):
        T.counterfactual_batch(G, x, y)
    with pytest.raises(PcgError, match="no CPU path"):
        T.train_step(G, D, C, None, None, x, y, y)
    with pytest.raises(PcgError, match="no CPU path"):
        T.GraphedTrainStep(G, D, C, 4)
    with pytest.raises(PcgError, match="no CPU path"):
        T.train_gan(G, D, C, [(x, y)], dict(T.params, epochs_gan=1), verbose=False)
    with pytest.raises(PcgError, match="eval mode"):
        T.GraphedTrainStep(G, D, K.Classifier().train(), 4)
    assert "not gan_train.Generator" in T.GraphedTrainStep.unsupported(K.ResidualGenerator(), D, C)
    C.conv_precision = "bf16"
    assert "fp32 only" in T.GraphedTrainStep.unsupported(G, D, C)
    with pytest.raises(NotImplementedError):
        G.conv_precision = "bf16"                       # bf16 operands are out of scope for these nets
