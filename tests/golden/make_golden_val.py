#!/usr/bin/env python3
"""Generate tests/golden/val_small.json by importing the REFERENCE itself (build container only, like make_golden.py; data only):

    python tests/golden/make_golden_val.py

Five samples at 64 x 96 through the reference's validation pass (train_hdf5_ddp.py:423-512: net.eval(), forward at batch 1, fp_loss,
compute_score, mean over the samples) on the state and inputs tests/util_val.py defines by formula: per-sample loss, IoU and tp/fp/fn,
the two means and logit samples.  The smallest relative top-two logit gap over the sampled pixels is checked (>= util_val.MIN_REL_GAP,
so no argmax flip can hide behind a tolerance) and stored."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = ["/root/reference/src/deepCam", ROOT, os.path.join(ROOT, "tests")]

from architecture import deeplab_xception as ref_arch      # noqa: E402
from utils import losses as ref_losses                      # noqa: E402
from utils import utils as ref_utils                        # noqa: E402

import util_val                                             # noqa: E402
from util_inputs import sample_index                        # noqa: E402

CLASS_W = [0.986267818390377 ** -0.125, 0.0004578708870701058 ** -0.125, 0.01327431072255291 ** -0.125]
FPW = (2.61461122397522257612, 1.71641974795896018744)


def main():
    torch.manual_seed(333)
    net = ref_arch.DeepLabv3_plus(n_input=16, n_classes=3, os=16, pretrained=False, rank=1)
    net.load_state_dict(util_val.perturbed_state())
    net.eval()
    x, y = util_val.val_inputs()
    samples, min_gap, below_all = [], float("inf"), 0
    with torch.no_grad():
        for i in range(util_val.N_SAMPLES):
            o = net(x[i:i + 1])
            loss = ref_losses.fp_loss(o, y[i:i + 1], CLASS_W, fpw_1=FPW[0], fpw_2=FPW[1])
            pred = torch.max(o, 1)[1]
            iou = ref_utils.compute_score(pred, y[i:i + 1], num_classes=3, device_id=0)
            gt = y[i:i + 1]
            eq, ne = pred == gt, pred != gt
            idx = sample_index(o.numel())
            gap = util_val.rel_gap(o).flatten()
            pix = idx % (util_val.H * util_val.W)          # flat index into [1,3,H,W] -> its pixel
            min_gap = min(min_gap, float(gap[pix].min()))
            below_all += int((gap < util_val.MIN_REL_GAP).sum())
            samples.append({"loss": float(loss), "iou": float(iou),
                            "tp": [int(torch.sum(eq[gt == j])) for j in range(3)],
                            "fp": [int(torch.sum(ne[pred == j])) for j in range(3)],
                            "fn": [int(torch.sum(ne[gt == j])) for j in range(3)],
                            "logit_samples": [float(v) for v in o.flatten()[idx]],
                            "logit_absmax": float(o.abs().max())})
    assert min_gap >= util_val.MIN_REL_GAP, f"a sampled pixel's top-two gap is {min_gap:.2e}: choose other seeds in tests/util_val.py"
    out = {"recipe": "state util_val.perturbed_state(), inputs util_val.val_inputs(), reference eval forward at batch 1 per sample",
           "H": util_val.H, "W": util_val.W, "state_seed": util_val.STATE_SEED, "input_seed": util_val.INPUT_SEED,
           "samples": samples, "mean_loss": float(np.mean([s["loss"] for s in samples])),
           "mean_iou": float(np.mean([s["iou"] for s in samples])),
           "min_rel_gap_sampled": min_gap, "pixels_below_gap_all": below_all}
    json.dump(out, open(os.path.join(HERE, "val_small.json"), "w"), indent=0)
    print("val_small.json:", {k: v for k, v in out.items() if k != "samples"})
    for s in samples:
        print({k: v for k, v in s.items() if k != "logit_samples"})


if __name__ == "__main__":
    main()
