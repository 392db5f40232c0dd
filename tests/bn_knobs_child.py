"""Child process of test_bn_environment_knobs (tests/test_hip_norm_branches.py); not collected by pytest.

PCG_BN_DEPTH / PCG_BN_NT / PCG_BN_BLOCKS are read once per process, so each setting runs here, in a fresh process started with the
knobs in its environment:  python bn_knobs_child.py OUT.npz  runs BatchNorm + LeakyReLU forward (pcg_bn_apply_act) and backward with
column sums (pcg_bn_act_bwd_db, dy_scale 0.5) at the knob shapes and writes y, dx, dcol and the describe text of every apply launch.
The parent calls run() in its own process for the default-knob outputs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
ACT_LRELU, SLOPE = 2, 0.2


def inputs(rows, C):
    import test_hip_norm_branches as T
    return T.bn_inputs(rows, C)


def run(shapes):
    import pcgan_amd
    import test_hip_norm_branches as T
    pcgan_amd.load()
    ops = pcgan_amd.ops
    out = {}
    for rows, C in shapes:
        d = inputs(rows, C)
        x, dy, mean, invstd, gamma, beta = (d[k].float().to(DEV).contiguous() for k in ("x", "dy", "mean32", "invstd32", "gamma", "beta"))
        y = ops.bn_apply_act(x, C, mean, invstd, gamma, beta, ACT_LRELU, SLOPE)
        dg, db, dcol = (torch.zeros(C, dtype=torch.float32, device=DEV) for _ in range(3))
        dx = ops.bn_act_bwd(dy, x, y, C, mean, invstd, gamma, ACT_LRELU, SLOPE, dg, db, False, dy_scale=0.5, dcol=dcol, accumulate_col=False)
        torch.cuda.synchronize()
        out[f"y_{rows}_{C}"], out[f"dx_{rows}_{C}"], out[f"dcol_{rows}_{C}"] = y.cpu().numpy(), dx.cpu().numpy(), dcol.cpu().numpy()
        out[f"plan_{rows}_{C}"] = np.array(T.plan("BN_APPLY", 0, rows, C, 1))
    return out


if __name__ == "__main__":
    import test_hip_norm_branches as T
    np.savez(sys.argv[1], **run(T.BN_KNOB_SHAPES))
