#!/usr/bin/env python3
"""Generate tests/golden/virtual_ranks_small.json by importing the REFERENCE itself (build container only, like make_golden.py; data only):

    python tests/golden/make_golden_virtual_ranks.py

The reference net at seed 333 on 64 x 96, two micro-batches of 2 samples (util_inputs.make_inputs(4, 64, 96), samples 0-1 and 2-3) standing
for two data-parallel ranks, two torch.optim.Adam steps (lr 1e-3, eps 1e-8, weight decay 1e-6, as model_small.json).  Each step is
zero_grad, then twice (forward, fp_loss / 2, backward) -- autograd sums the two gradients, the division by 2 is the average over the
ranks (train_hdf5_ddp.py:227,359-363) --, then step.  The BatchNorm running buffers are put back to what the first micro-batch's forward
left (rank 0's buffers).  Stored: the two micro-batch losses, 64 sampled weights (flat, parameter order) and sampled buffers per step."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = ["/root/reference/src/deepCam", ROOT, os.path.join(ROOT, "tests")]

from architecture import deeplab_xception as ref_arch      # noqa: E402
from utils import losses as ref_losses                      # noqa: E402

from util_inputs import make_inputs, sample_index           # noqa: E402

CLASS_W = [0.986267818390377 ** -0.125, 0.0004578708870701058 ** -0.125, 0.01327431072255291 ** -0.125]
FPW = (2.61461122397522257612, 1.71641974795896018744)
H, W, B, K, STEPS = 64, 96, 2, 2, 2
BUFFER_EVERY = 12          # every 12th BatchNorm, first 4 channels of its running mean and variance


def main():
    torch.manual_seed(333)
    net = ref_arch.DeepLabv3_plus(n_input=16, n_classes=3, os=16, pretrained=False, rank=1)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-8, weight_decay=1e-6)
    x, y = make_inputs(K * B, H, W)
    n_params = sum(p.numel() for p in net.parameters())
    idx = sample_index(n_params)
    bn_names = [k[:-len(".running_mean")] for k in net.state_dict() if k.endswith(".running_mean")][::BUFFER_EVERY]
    steps = []
    for _ in range(STEPS):
        opt.zero_grad()
        losses, aside = [], None
        for v in range(K):
            out = net(x[v * B:(v + 1) * B])
            loss = ref_losses.fp_loss(out, y[v * B:(v + 1) * B], CLASS_W, fpw_1=FPW[0], fpw_2=FPW[1])
            (loss / K).backward()
            losses.append(float(loss))
            if v == 0:
                aside = {k: t.clone() for k, t in net.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
        with torch.no_grad():
            sd = net.state_dict()
            for k, t in aside.items():
                sd[k].copy_(t)
        opt.step()
        flat = torch.cat([p.detach().flatten() for p in net.parameters()])
        sd = net.state_dict()
        steps.append({"losses": losses, "weight_samples": [float(v) for v in flat[idx]],
                      "buffers": {n: {"running_mean": [float(v) for v in sd[n + ".running_mean"][:4]],
                                      "running_var": [float(v) for v in sd[n + ".running_var"][:4]],
                                      "num_batches_tracked": int(sd[n + ".num_batches_tracked"])} for n in bn_names}})
    out = {"recipe": "reference net seed 333, make_inputs(4, 64, 96) as two micro-batches of 2, Adam lr 1e-3 eps 1e-8 wd 1e-6; per step: "
                     "zero_grad, 2 x (forward, fp_loss / 2, backward), running buffers back to micro-batch 0's, step",
           "H": H, "W": W, "B": B, "K": K, "sample_index": [int(i) for i in idx], "steps": steps}
    json.dump(out, open(os.path.join(HERE, "virtual_ranks_small.json"), "w"), indent=0)
    for s in steps:
        print(s["losses"], s["weight_samples"][:3])


if __name__ == "__main__":
    main()
