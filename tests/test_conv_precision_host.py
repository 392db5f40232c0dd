"""CPU: the bf16-operand mode's switch without a GPU — the thread-local library setting (pcg_conv_precision_set /
_get), the ops.conv_precision context manager, and which nets accept FlatModule.conv_precision = "bf16".  No compute call is made."""
import threading

import pytest

import pcgan_amd
from pcgan_amd import _lib, ops

PCG_ERR_INVALID = -1          # include/pcgan_hip.h


@pytest.fixture()
def lib():
    lib = pcgan_amd.load()
    assert lib.pcg_conv_precision_get() == 0
    yield lib
    lib.pcg_conv_precision_set(0)


def test_set_get_round_trip_and_invalid_values(lib):
    assert lib.pcg_conv_precision_set(1) == _lib.PCG_OK
    assert lib.pcg_conv_precision_get() == 1
    assert lib.pcg_conv_precision_set(0) == _lib.PCG_OK
    assert lib.pcg_conv_precision_get() == 0
    for bad in (2, -1, 7, 1 << 20):
        assert lib.pcg_conv_precision_set(bad) == PCG_ERR_INVALID
        assert b"pcg_conv_precision_set" in lib.pcg_last_error()
        assert lib.pcg_conv_precision_get() == 0          # a rejected value leaves the setting alone


def test_setting_is_thread_local(lib):
    assert lib.pcg_conv_precision_set(1) == _lib.PCG_OK
    seen = {}

    def other():
        seen["before"] = lib.pcg_conv_precision_get()
        lib.pcg_conv_precision_set(1)
        lib.pcg_conv_precision_set(0)
        seen["after"] = lib.pcg_conv_precision_get()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": 0, "after": 0}
    assert lib.pcg_conv_precision_get() == 1              # the other thread's set did not reach this one


def test_context_manager_restores_on_exit_and_on_exception(lib):
    assert ops.current_conv_precision() == "fp32"
    with ops.conv_precision("bf16"):
        assert lib.pcg_conv_precision_get() == 1
        with ops.conv_precision("fp32"):
            assert ops.current_conv_precision() == "fp32"
        assert ops.current_conv_precision() == "bf16"
    assert lib.pcg_conv_precision_get() == 0
    with pytest.raises(RuntimeError, match="inside"):
        with ops.conv_precision("bf16"):
            raise RuntimeError("inside")
    assert lib.pcg_conv_precision_get() == 0
    lib.pcg_conv_precision_set(1)
    with ops.conv_precision("fp32"):
        assert lib.pcg_conv_precision_get() == 0
    assert lib.pcg_conv_precision_get() == 1              # restores the previous mode, not the default
    scope = ops.conv_precision("bf16")         # one object entered again while active (nested use) restores each level
    lib.pcg_conv_precision_set(0)
    with scope:
        with ops.conv_precision("fp32"):
            with scope:
                assert lib.pcg_conv_precision_get() == 1
            assert lib.pcg_conv_precision_get() == 0
        assert lib.pcg_conv_precision_get() == 1
    assert lib.pcg_conv_precision_get() == 0
    for bad in ("bf32", "BF16", "fp16", None, 1):
        with pytest.raises(ValueError):
            ops.conv_precision(bad)


def test_nets_that_honour_the_mode_accept_it():
    from pcgan_amd import countergan as C
    from pcgan_amd import dcgan as D
    cfg = {"g_hidden": 16, "d_hidden": 16, "z_dim": 32}
    for net in (D.Generator(cfg), D.Discriminator(cfg), C.ResidualGenerator(), C.Discriminator(), C.CNNClassifier()):
        assert net.conv_precision == "fp32"
        net.conv_precision = "bf16"
        assert net.conv_precision == "bf16"
        net.conv_precision = "fp32"
        assert net.conv_precision == "fp32"
        with pytest.raises(ValueError):
            net.conv_precision = "fp16"
    a, b = D.Generator(cfg), D.Generator(cfg)
    a.conv_precision = "bf16"
    assert b.conv_precision == "fp32"                     # per net, not per class


def test_nets_that_do_not_honour_the_mode_refuse_it():
    from pcgan_amd import house as H
    from pcgan_amd import moons as M
    from pcgan_amd import wgan as W
    nets = [W.Generator(), W.Critic(), H.Discriminator(17, 32, 4), H.NNClassifier(17, 4),
            M.build_generator(2, 16), M.build_discriminator(16)]
    for net in nets:
        with pytest.raises(NotImplementedError):
            net.conv_precision = "bf16"
        assert net.conv_precision == "fp32"
        net.conv_precision = "fp32"                       # the default stays settable
