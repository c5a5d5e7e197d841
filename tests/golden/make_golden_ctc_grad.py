#!/usr/bin/env python3
"""Golden vectors for the CTC loss's gradient with respect to the logits: tests/golden/g11_ctc_grad.npz.

Runs the REAL reference criterion (`SetCriterion.loss_CTC`, models/dino/dino.py:457-551, through tests/golden/ref_harness.py) on the
seeded head outputs of tests/util.ctc_case -- g5's five cases plus one with a line whose transcription does not fit 2 nq frames -- and
takes torch.autograd.grad of its loss with respect to pred_logits.  Stores data only: the case parameters, the label sequences of the
extra case, the loss values, the full gradients of the small cases, and for the 2 x 900 x 166 case every 16th query row plus the sum and
the sum of absolute values.
Authoring container only:  python tests/golden/make_golden_ctc_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from dtlr_amd.config import DTLRConfig                      # noqa: E402
from dtlr_amd.weights import synthetic_state_dict           # noqa: E402
from tests.golden import ref_harness as rh                  # noqa: E402
from tests.golden.make_golden_ctc import CASES              # noqa: E402
from tests.util import ctc_case                             # noqa: E402

ROW_STRIDE = 16
# the extra case: ctc_case(11, 4, 12, 7, -2.0, 5) with these labels; the last line has 28 labels > 24 frames -> infeasible
INFEASIBLE = (11, 4, 12, 7, -2.0, 5)
INFEASIBLE_LABELS = [[1, 1, 1, 1], [], [0, 6, 3], list(range(7)) * 4]


def reference_grad(crit, outputs, labels):
    x = outputs["pred_logits"].clone().requires_grad_(True)
    targets = [{"labels": torch.tensor(l, dtype=torch.int64)} for l in labels]
    loss = crit.loss_CTC({"pred_logits": x, "pred_boxes": outputs["pred_boxes"]}, targets, None, None)["loss_CTC"]
    (g,) = torch.autograd.grad(loss, x)
    return float(loss), g


def main():
    cfg = DTLRConfig.tiny()
    _, _, crit = rh.build_reference_model(cfg, synthetic_state_dict(cfg, 0))
    out = {"cases": np.array(list(CASES) + [INFEASIBLE], dtype=np.float64), "row_stride": np.int64(ROW_STRIDE),
           "infeasible_labels": np.array([l + [-1] * (28 - len(l)) for l in INFEASIBLE_LABELS], dtype=np.int64)}
    for k, case in enumerate(list(CASES) + [INFEASIBLE]):
        outputs, labels = ctc_case(*case)
        if case == INFEASIBLE:
            labels = INFEASIBLE_LABELS
        loss, g = reference_grad(crit, outputs, labels)
        g = g.numpy()
        out[f"loss_{k}"] = np.float64(loss)
        if g.size > 100000:
            out[f"grad_rows_{k}"] = g[:, ::ROW_STRIDE].astype(np.float32)
            out[f"grad_sum_{k}"] = np.float64(g.astype(np.float64).sum())
            out[f"grad_abssum_{k}"] = np.float64(np.abs(g.astype(np.float64)).sum())
        else:
            out[f"grad_{k}"] = g.astype(np.float32)
        print(k, case, loss, float(np.abs(g).max()))
    np.savez_compressed(os.path.join(HERE, "g11_ctc_grad.npz"), **out)


if __name__ == "__main__":
    main()
