#!/usr/bin/env python3
"""Times the scale-separation verification (dc_scale_score; nn.ScaleSkill) at batch 8, 768 x 1152, uint8 masks, the full band, L = 7
(T = 128), for one origin and for four, and two kinds of input -- sparse frames of about 97 % background (ellipses, the prediction a
displaced copy of the labels with some objects of its own) and uniform-random frames (every pixel 0, 1 or 2 with equal probability,
independently on both sides) -- and prints beside each figure

  dc_fss_score (nn.FractionsSkill, the default windows) on the same masks, and the forward pass of the same batch (nn.Predictor, bf16),
      the thing both run behind, in the same process;
  the same integers through plain PyTorch operators on the same GPU: per origin a torch.roll, per level a view(...).sum((2, 4)) of the
      int64 indicator fields and the three sums of squares.  It is checked for equality with the HIP rows before it is timed.

Every call is timed with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks.  Only standard
output belongs in the profile:

    python scripts/scale_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/scale_skill.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from distance_bench import sparse_masks  # noqa: E402
from event_match_bench import B, H, W, time_block  # noqa: E402

LEVELS = 7
ORIGINS = {1: (0,), 4: (0, 1, 37, 64)}


def torch_rows(pred: torch.Tensor, truth: torch.Tensor, levels: int, origins) -> torch.Tensor:
    """int64 [B, 2, O, levels + 1, 3] by plain PyTorch operators, the full band"""
    n, h, w = pred.shape
    out = torch.zeros((n, 2, len(origins), levels + 1, 3), dtype=torch.int64, device=pred.device)
    for k in (1, 2):
        f, o = (pred == k).to(torch.int64), (truth == k).to(torch.int64)
        for i, c in enumerate(origins):
            fr, tr = torch.roll(f, -c, dims=2), torch.roll(o, -c, dims=2)
            for j in range(levels + 1):
                s = 1 << j
                sf = fr.view(n, h // s, s, w // s, s).sum((2, 4))
                so = tr.view(n, h // s, s, w // s, s).sum((2, 4))
                out[:, k - 1, i, j, 0] = ((sf - so) ** 2).sum((1, 2))
                out[:, k - 1, i, j, 1] = (sf ** 2).sum((1, 2))
                out[:, k - 1, i, j, 2] = (so ** 2).sum((1, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--torch_calls", type=int, default=2, help="calls per block of the PyTorch evaluation")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, uint8 masks, L = {LEVELS} (T = {1 << LEVELS}), origins "
          f"{[list(o) for o in ORIGINS.values()]}, the full band; {a.blocks} blocks of {a.calls} calls per figure ({a.torch_calls} for PyTorch), "
          "HIP events, medians")
    assert dnn.scale_levels(H, W) == LEVELS
    rs = np.random.RandomState(11)
    kinds = {"sparse": sparse_masks(rs), "uniform-random": tuple(rs.randint(0, 3, size=(B, H, W)).astype(np.uint8) for _ in range(2))}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    predictor = dnn.Predictor(net, B, H, W)
    fs = dnn.FractionsSkill(B, H, W, device=dev)
    med = lambda v: statistics.median(v)  # noqa: E731
    fmt = lambda v: "none" if v is None else f"{v:.4f}"  # noqa: E731
    for kind, (pred_h, truth_h) in kinds.items():
        pred, truth = torch.from_numpy(pred_h).to(dev), torch.from_numpy(truth_h).to(dev)
        background = 1.0 - float(((truth_h == 1) | (truth_h == 2)).mean())
        print(f"{kind}: {100 * background:.1f} % of the labels and {100 * (1.0 - float(((pred_h == 1) | (pred_h == 2)).mean())):.1f} % of the "
              f"prediction are background")
        for O, origins in ORIGINS.items():
            ss = dnn.ScaleSkill(B, H, W, levels=LEVELS, origins=origins, device=dev)
            rows, pixels = (t.clone() for t in ss(pred, truth).frame_rows())
            ref = torch_rows(pred, truth, LEVELS, origins)
            print(f"  O = {O}: HIP rows against the PyTorch rows: {'equal' if torch.equal(ref, rows) else 'DIFFERENT'}")
            del ref
            c = ss.result()["class_1"]
            print(f"    class 1, pooled: mse per scale {' '.join(fmt(v) for v in c['mse'])}")
            print(f"    skill {' '.join(fmt(v) for v in c['skill'])}; skilful from scale {c['skilful_scale']}")
            print(f"    energy (pred - truth) / (pred + truth) {' '.join(fmt(v) for v in c['energy_rel_diff'])}")
            print(f"    spread of mse over the origins {' '.join('none' if v is None else f'{v:.2e}' for v in c['origin_spread'])}")
            routes = {"dc_scale_score (nn.ScaleSkill)": (lambda: ss(pred, truth), a.calls),
                      "dc_fss_score (nn.FractionsSkill, 7 windows)": (lambda: fs(pred, truth), a.calls),
                      "forward pass (nn.Predictor, bf16)": (lambda: predictor(x), a.calls),
                      "the rows by plain PyTorch, roll / view / sum": (lambda: torch_rows(pred, truth, LEVELS, origins), a.torch_calls)}
            for fn, _ in routes.values():             # warm-up: code objects, weight repack, allocator
                fn()
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            for _ in range(a.blocks):                 # alternating blocks
                for name, (fn, calls) in routes.items():
                    times[name].append(time_block(fn, calls))
            for name, v in times.items():
                print(f"    {name:46s} {med(v):9.3f} ms/batch   blocks {' '.join(f'{t:.3f}' for t in v)}")
            ms = med(times["dc_scale_score (nn.ScaleSkill)"])
            print(f"    PyTorch / HIP = {med(times['the rows by plain PyTorch, roll / view / sum']) / ms:.0f} x; HIP / dc_fss_score = "
                  f"{ms / med(times['dc_fss_score (nn.FractionsSkill, 7 windows)']):.2f}; HIP / forward pass = "
                  f"{100 * ms / med(times['forward pass (nn.Predictor, bf16)']):.2f} %")
            print(f"    workspace {L.load().dc_scale_workspace(B, H, W, LEVELS, O) / 1e3:.1f} kB, rows {B * 2 * O * (LEVELS + 1) * 3 * 8 / 1e3:.1f} kB; "
                  f"the masks read: {2 * B * H * W / 1e6:.1f} MB, once per origin")
            del ss
    print("launches per call: 3 (scale_sums, scale_coarse, scale_total) and two memsets")
    predictor.close()


if __name__ == "__main__":
    main()
