"""Child process of test_adam_tick_blocks_knob (tests/test_hip_optim_branches.py) and of the host test of the knob
(tests/test_optim_plan_host.py); not collected by pytest.

PCG_ADAM_TICK_BLOCKS is read once per process, so each setting runs here, in a fresh process started with the knob in its
environment:
  python adam_knob_child.py OUT.npz   runs two capturable Adam steps at the knob size (T.knob_run) and writes p, m, v and the describe
                                      text of the launch;
  python adam_knob_child.py --plan    prints the describe text alone: host logic, no device.
The parent calls T.knob_run() in its own process for the default-knob outputs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == "__main__":
    import pcgan_amd
    import test_hip_optim_branches as T
    pcgan_amd.load()
    if sys.argv[1] == "--plan":
        print(T.plan(T.KNOB_N, 1, 1))
    else:
        np.savez(sys.argv[1], **T.knob_run(pcgan_amd.ops))
