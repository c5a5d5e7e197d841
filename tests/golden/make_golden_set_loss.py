#!/usr/bin/env python3
"""Golden vectors for the set criterion: tests/golden/g12_set_loss.npz.

Runs the REAL reference `HungarianMatcher` (models/dino/matcher.py) and `SetCriterion.forward_standard` (models/dino/dino.py:780-964,
imported through tests/golden/ref_harness.py's stubs) on the CPU, in the reference's own fp32, on the two seeded cases
tests/set_loss_ref.GOLDEN_CASES (main + five auxiliary + the intermediate output), with the reference's matcher costs and weight_dict
(config/Latin_CTC.py:78-89).  One more shim than ref_harness lists: forward_standard moves its zero-valued `*_dn` entries `.to("cuda")`,
which is made a no-op here.  Stores data only: the case parameters, every output's assignment as match_q rows, the loss dict's keys and
values, and the full dlogits / dboxes of torch.autograd.grad of the weighted sum.
Authoring container only:  python tests/golden/make_golden_set_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests import set_loss_ref as R                         # noqa: E402
from tests.golden import ref_harness as rh                  # noqa: E402


def main():
    rh._install_stubs()
    from models.dino.dino import SetCriterion
    from models.dino.matcher import HungarianMatcher
    to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if a and a[0] == "cuda" else to(self, *a, **k)
    out = {"names": np.array(list(R.GOLDEN_CASES)), "cases": np.array(list(R.GOLDEN_CASES.values()), dtype=np.int64)}
    for k, name in enumerate(R.GOLDEN_CASES):
        logits, boxes, targets = R.case(name)
        L, B, nq, C = logits.shape
        wd = R.weight_dict(n_aux=L - 2)
        crit = SetCriterion(C, HungarianMatcher(focal_alpha=R.ALPHA, **R.COSTS), wd, R.ALPHA, ["labels", "boxes", "cardinality"])
        x, bx = logits.clone().requires_grad_(True), boxes.clone().requires_grad_(True)
        outputs = R.outputs_dict(x, bx)
        outputs["dn_meta"] = None
        losses, indices = crit.forward_standard(outputs, targets, return_indices=True)
        indices = indices[-1:] + indices[:-1]                       # the main output first, as the outputs are stacked
        Tmax = max(max(len(t["labels"]) for t in targets), 1)
        match = np.full((L * B, Tmax), -1, dtype=np.int32)
        for l in range(L):
            for b, (i, j) in enumerate(indices[l]):
                match[l * B + b, j.numpy()] = i.numpy()
        total = sum(losses[key] * wd[key] for key in losses if key in wd)
        gl, gb = torch.autograd.grad(total, (x, bx))
        keys = sorted(key for key in losses if not key.split("_")[-1] == "dn" and "_dn_" not in key)
        out[f"match_{k}"] = match
        out[f"keys_{k}"] = np.array(keys)
        out[f"values_{k}"] = np.array([float(losses[key]) for key in keys], dtype=np.float64)
        out[f"total_{k}"] = np.float64(float(total))
        out[f"dlogits_{k}"] = gl.numpy().astype(np.float32)
        out[f"dboxes_{k}"] = gb.numpy().astype(np.float32)
        print(name, [len(t["labels"]) for t in targets], float(total), len(keys))
    np.savez_compressed(os.path.join(HERE, "g12_set_loss.npz"), **out)


if __name__ == "__main__":
    main()
