"""Host-side preconditions (no GPU) of tests/test_hip_delta_steps_train_batch.py, for both MNIST CounteRGAN ports at batch 128: on the
rows G hands the classifier, §3.18's gap bound leaves at most 0.2 % of a pool layer's live windows undecided, and the float32
restatement of G's and the classifier's forward sits inside rule (a) (rtol 1e-4, atol 2e-5 * max|float64|) of the float64 one -- so a
GPU step that misses the rule there is wrong, not unlucky.  G's and the classifier's forward only: a few seconds.

Measured (CPU, these seeds): under the bound
  gan_train    pool 1  74 of 713727 live windows (bound 3.0e-05)    pool 2  135 of 249143 (bound 5.7e-05)
  countergan2  pool 1  81 of 711228 (bound 2.9e-05)                 pool 2  124 of 250160 (bound 5.4e-05)
all under 0.06 % (the bounds, and with them the counts, follow the host's fp32 convolutions); float32 against float64 uses at most
0.027 of rule (a)'s atol (gan_train's delta; the cls_logits of both ports 0.023).  Of G's ReLU units 611 of 6422528, 817 of 6422528
and (gan_train's third) 481 of 3211264 have a float64 pre-activation under the activation bound (5.7e-5, 3.2e-5, 1.6e-5), the
precondition of the mask pins of delta_train_batch_ref; the host's float32 run takes the other side of zero on none of them.  4 s for
both ports on 8 threads."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countergan2_restate as CR  # noqa: E402
import delta_gan_restate as RS  # noqa: E402
import delta_train_batch_ref as TB  # noqa: E402

PORTS = {"gan_train": RS, "countergan2": CR}


@pytest.fixture(scope="module", params=sorted(PORTS))
def pair(request):
    with TB.cpu_threads():
        return request.param, TB.g_and_classifier_forward(PORTS[request.param], torch.float32), \
            TB.g_and_classifier_forward(PORTS[request.param], torch.float64)


def test_training_batch_is_the_ports_own(pair):
    from pcgan_amd import countergan2, gan_train
    assert gan_train.params["batch_size"] == countergan2.params(5)["batch_size"] == TB.B_TRAIN and 60000 % TB.B_TRAIN == TB.B_TAIL
    assert pair[1]["x_cf"].shape == (TB.B_TRAIN, 1, 28, 28)


def test_near_share_of_the_live_windows_is_under_the_cap(pair):
    port, f32, f64 = pair
    route = TB.routing(f32["clf"], f64["clf"])
    for layer in (1, 2):
        r = route[layer]
        near, live = int(r["near"].sum()), int(r["live"].sum())
        print(f"{port} pool {layer}: {near} of {live} live windows under the bound {r['bound']:.1e}")
        assert live > 0 and near / live <= TB.NEAR_CAP


def test_float32_restatement_is_inside_rule_a(pair):
    port, f32, f64 = pair
    for name in ("loss_cls", "loss_reg", "delta", "x_cf", "cls_logits"):
        share = TB.rule_a(f32[name], f64[name], f"{port} {name}")
        print(f"{port} {name}: float32 uses {share:.3f} of rule (a)'s atol")


def test_near_share_of_gs_relu_units_is_under_the_cap(pair):
    """The same precondition for the ReLU masks the float64 iteration is pinned to (delta_train_batch_ref.mask_report), on G's layers."""
    port, f32, f64 = pair
    for i, (z32, z64) in enumerate(zip(f32["z"], f64["z"])):
        rep = TB.mask_report(z64, z32, z64 > 0)
        print(f"{port} G ReLU {i}: {rep['near']} of {rep['units']} units under the bound {rep['bound']:.1e}; float32 takes the other side on "
              f"{int(((z32 > 0) != (z64 > 0)).sum())}")
        assert rep["near"] / rep["units"] <= TB.NEAR_CAP
        assert TB.mask_report(z64, z32, z32 > 0)["wrong"] == 0
