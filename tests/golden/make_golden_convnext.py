"""Golden fixture for the ConvNeXt backbone, from the REAL reference (authoring container only).

    python -m tests.golden.make_golden_convnext          # writes tests/golden/g18_convnext.npz

G18 backbone level: the reference's ConvNeXt class (models/dino/convnext.py:55) instantiated DIRECTLY -- never through build_backbone /
    build_convnext, which are hard-wired to pretrained=True and fetch a checkpoint -- with a test-sized network (dims 32/64/96/160,
    depths 2/1/2/1, out_indices 1/2/3) and the name-seeded weights of dtlr_amd.weights (cfg.backbone = "convnext_custom"), on an
    odd-sized pair (2 x 3 x 37 x 90: floor sizes 9x22, 4x11, 2x5, 1x2) and on a 64 x 256 pair.  The three maps of each, NCHW fp32.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from dtlr_amd.synth import noise_lines                      # noqa: E402
from dtlr_amd.weights import GENERATOR_VERSION, synthetic_state_dict   # noqa: E402
from tests.convnext_ref import TEST_DEPTHS, TEST_DIMS, test_cfg   # noqa: E402
from tests.golden import ref_harness as rh                   # noqa: E402

warnings.filterwarnings("ignore")

INPUTS = {"a": (37, 90, 71), "b": (64, 256, 72)}             # name -> (H, W, seed of dtlr_amd.synth.noise_lines)


def golden_input(name):
    h, w, seed = INPUTS[name]
    return torch.stack(noise_lines(2, h, w, seed=seed))


def main():
    rh._install_stubs()
    from models.dino.convnext import ConvNeXt
    out = {"generator_version": np.int64(GENERATOR_VERSION)}
    sd = synthetic_state_dict(test_cfg(), seed=0)
    m = ConvNeXt(depths=list(TEST_DEPTHS), dims=list(TEST_DIMS), out_indices=(1, 2, 3))
    m.eval()
    m.load_state_dict({k[len("backbone.0."):]: v for k, v in sd.items() if k.startswith("backbone.0.")}, strict=True)
    for name in INPUTS:
        with torch.no_grad():
            feats = m.forward_features(golden_input(name))
        for i, f in enumerate(feats):
            out[f"{name}_feat{i}"] = f.detach().cpu().numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "g18_convnext.npz"), **out)
    print("g18 written")


if __name__ == "__main__":
    assert rh.reference_available(), "needs the reference checkout"
    torch.set_num_threads(8)
    main()
