"""CPU: the references the GPU tests of the house-sales classifier fit (tests/test_hip_house_clf_fit.py) are measured against.
(1) tests/house_clf_restate.py -- the step written stage by stage with a hand-written backward -- against the oracle's autograd step
(oracle/house_ref.classifier_train_step) on the reference's recorded batches and Dropout draws, in float64;
(2) the tally's bookkeeping (sum of loss * rows, correct rows, rows; one segment per loader batch) against the sums the reference's
loops keep (trainer.py:89-91, :110-115) over a recorded three-batch split."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import house_clf_restate as RS  # noqa: E402
from oracle import house_ref as HR  # noqa: E402


def _gold(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "classifier_pretrain_house.npz")))
    rows = np.concatenate([gold[f"step{i}.rows"] for i in range(int(gold["meta.steps"]))])
    return gold, torch.tensor(HR.balanced_class_weights(gold["y"][rows], 4), dtype=torch.float64), rows


def test_restatement_is_the_oracle_step(golden_dir):
    gold, cw, _ = _gold(golden_dir)
    clf = HR.NNClassifier(17, 4)
    clf.load_state_dict({k[5:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.")})
    clf = clf.double()
    opt = torch.optim.AdamW(clf.parameters(), lr=1e-3, weight_decay=1e-4)
    X, y = torch.from_numpy(gold["X"]).double(), torch.from_numpy(gold["y"])
    for i in range(int(gold["meta.steps"])):
        r = torch.from_numpy(gold[f"step{i}.rows"])
        masks = [torch.from_numpy(gold[f"step{i}.mask{j}"]) for j in range(3)]
        sd = {k: v.clone() for k, v in clf.state_dict().items()}
        loss, grads, run = RS.train_grads(sd, X[r], y[r], masks, cw)
        ref = HR.classifier_train_step(clf, opt, cw, X[r], y[r], masks)          # leaves p.grad of this step, then moves the parameters
        assert abs(loss - ref) <= 1e-12 * max(1.0, abs(ref)), (i, loss, ref)
        for n, p in clf.named_parameters():
            scale = float(p.grad.abs().max())
            assert float((grads[n] - p.grad).abs().max()) <= 1e-10 * max(scale, 1e-3), (i, n)
        after = clf.state_dict()
        for k, v in run.items():
            assert float((v - after[k]).abs().max()) <= 1e-12, (i, k)


def test_tally_bookkeeping_is_the_loops_sums(golden_dir):
    gold, cw, rows = _gold(golden_dir)
    clf = HR.NNClassifier(17, 4)
    clf.load_state_dict({k[5:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.")})
    clf.eval()
    X, y, w = torch.from_numpy(gold["X"]), torch.from_numpy(gold["y"]), cw.float()
    with torch.no_grad():
        logits = clf(X[rows])                                                   # the three recorded batches, 48 rows each, in loader order
    run_loss, correct, total = 0.0, 0, 0
    for i in range(int(gold["meta.steps"])):                                    # trainer.py:104-115
        lb, yb = logits[48 * i:48 * (i + 1)], y[rows][48 * i:48 * (i + 1)]
        run_loss += F.cross_entropy(lb, yb, weight=w).item() * lb.size(0)
        correct += int((lb.argmax(1) == yb).sum())
        total += lb.size(0)
    (tot, hits, n), losses = RS.ce_tally(logits.double(), y[rows], w.double(), 48)
    assert len(losses) == 3 and hits == correct and n == total == 144
    assert abs(tot - run_loss) <= 1e-6 * abs(run_loss)                          # fp32 losses against float64 ones
    # a ragged last segment: 144 rows in runs of 64 are 64 + 64 + 16
    (tot2, hits2, n2), losses2 = RS.ce_tally(logits.double(), y[rows], w.double(), 64)
    want = sum(F.cross_entropy(logits[s:s + 64].double(), y[rows][s:s + 64], weight=w.double()).item() * min(64, 144 - s) for s in (0, 64, 128))
    assert len(losses2) == 3 and hits2 == correct and n2 == 144 and abs(tot2 - want) <= 1e-12 * abs(want)
    # the gradient of one segment is autograd's
    lg = logits[:48].double().requires_grad_()
    F.cross_entropy(lg, y[rows][:48], weight=w.double()).backward()
    assert float((RS.ce_segment(logits[:48].double(), y[rows][:48], w.double())[1] - lg.grad).abs().max()) <= 1e-14
