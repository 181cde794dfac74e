#!/usr/bin/env python3
"""Times the displacement verification (dc_displacement_score; nn.DisplacementSkill) at batch 8, 768 x 1152, uint8 masks, the full band,
for the radii R = 8, 16 and 32 and two kinds of input -- sparse frames of about 97 % background (ellipses, the prediction a displaced copy
of the labels with some objects of its own) and uniform-random frames (every pixel 0, 1 or 2 with equal probability, independently on both
sides: no label word is zero, nothing is skipped) -- and prints beside each figure

  dc_distance_score (nn.DistanceSkill, R = 16) and dc_fss_score (nn.FractionsSkill, the default windows) on the same masks, and the
      forward pass of the same batch (nn.Predictor, bf16), the thing all three run behind, in the same process;
  the same tables through plain PyTorch operators on the same GPU: per dy one torch.roll along the rows (what rolls in from the other pole
      is cleared) and a sum for kept, per (dy, dx) a torch.roll along the columns, `&` and sum -- (2 R + 1)^2 passes.  It is checked for
      equality with the HIP tables before it is timed, and timed at the radii of --torch_radii only (8 and 16 by default: at R = 32 it
      makes 4225 passes).  At a radius where it is not run, the centre of the HIP table is compared with the HIP table of the next
      smaller radius instead.

Every call is timed with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks.  Only standard
output belongs in the profile:

    python scripts/displacement_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/displacement.txt"""
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

RADII = (8, 16, 32)


def torch_tables(pred: torch.Tensor, truth: torch.Tensor, R: int) -> torch.Tensor:
    """int64 [B, 2, 2 R + 1, 2 R + 2] by plain PyTorch operators, the full band"""
    P = torch.stack([pred == 1, pred == 2], dim=1)                                # [B, 2, H, W]
    T = torch.stack([truth == 1, truth == 2], dim=1)
    S = 2 * R + 1
    out = torch.zeros((pred.shape[0], 2, S, S + 1), dtype=torch.int64, device=pred.device)
    for dy in range(-R, R + 1):
        moved = torch.roll(P, dy, dims=2)
        if dy > 0:
            moved[:, :, :dy] = False
        elif dy < 0:
            moved[:, :, dy:] = False
        out[:, :, dy + R, S] = moved.sum(dim=(2, 3))
        for dx in range(-R, R + 1):
            out[:, :, dy + R, dx + R] = (torch.roll(moved, dx, dims=3) & T).sum(dim=(2, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--torch_calls", type=int, default=1, help="calls per block of the PyTorch evaluation (it takes a thousand times longer)")
    ap.add_argument("--torch_radii", type=int, nargs="*", default=[8, 16], help="the radii at which the PyTorch evaluation is run and timed")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, uint8 masks, radii {list(RADII)}, the full band; {a.blocks} blocks of "
          f"{a.calls} calls per figure ({a.torch_calls} for PyTorch, at R in {a.torch_radii}), HIP events, medians")
    rs = np.random.RandomState(11)
    kinds = {"sparse": sparse_masks(rs), "uniform-random": tuple(rs.randint(0, 3, size=(B, H, W)).astype(np.uint8) for _ in range(2))}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    predictor = dnn.Predictor(net, B, H, W)
    fs = dnn.FractionsSkill(B, H, W, device=dev)
    dist = dnn.DistanceSkill(B, H, W, radius=16, device=dev)
    med = lambda v: statistics.median(v)  # noqa: E731
    for kind, (pred_h, truth_h) in kinds.items():
        pred, truth = torch.from_numpy(pred_h).to(dev), torch.from_numpy(truth_h).to(dev)
        background = 1.0 - float(((truth_h == 1) | (truth_h == 2)).mean())
        print(f"{kind}: {100 * background:.1f} % of the labels and {100 * (1.0 - float(((pred_h == 1) | (pred_h == 2)).mean())):.1f} % of the "
              f"prediction are background")
        smaller = None                                # (R, rows) of the radius before
        for R in RADII:
            S = 2 * R + 1
            ds = dnn.DisplacementSkill(B, H, W, radius=R, device=dev)
            rows, pixels, best = (t.clone() for t in ds(pred, truth).frame_rows())
            with_torch = R in a.torch_radii
            if with_torch:
                ref = torch_tables(pred, truth, R)
                print(f"  R = {R}: HIP tables against the PyTorch tables: {'equal' if torch.equal(ref, rows) else 'DIFFERENT'}")
                del ref
            elif smaller is not None:
                r, small = smaller
                centre = rows[:, :, R - r:R + r + 1]
                same = torch.equal(centre[..., R - r:R + r + 1], small[..., :2 * r + 1]) and torch.equal(centre[..., S], small[..., 2 * r + 1])
                print(f"  R = {R}: the centre of the HIP tables against the HIP tables at R = {r}: {'equal' if same else 'DIFFERENT'}")
            smaller = (R, rows)
            host_best = [[list(dnn.displacement_best(rows[b, k].tolist(), R)) for k in range(2)] for b in range(B)]
            print(f"    best shifts on the device against the host's order: {'equal' if host_best == best.tolist() else 'DIFFERENT'}")
            c = ds.result()["class_1"]
            fmt = lambda v: "none" if v is None else f"{v:.3f}"  # noqa: E731
            print(f"    class 1, pooled: shift ({c['shift']['rows']}, {c['shift']['cols']}), CSI {fmt(c['csi']['unshifted'])} -> "
                  f"{fmt(c['csi']['shifted'])}, shares displacement / volume / pattern {fmt(c['share']['displacement'])} / "
                  f"{fmt(c['share']['volume'])} / {fmt(c['share']['pattern'])}; per-frame shifts {[b[0][:2] for b in best.tolist()]}")
            routes = {"dc_displacement_score (nn.DisplacementSkill)": (lambda: ds(pred, truth), a.calls),
                      "dc_distance_score (nn.DistanceSkill, R = 16)": (lambda: dist(pred, truth), a.calls),
                      "dc_fss_score (nn.FractionsSkill, 7 windows)": (lambda: fs(pred, truth), a.calls),
                      "forward pass (nn.Predictor, bf16)": (lambda: predictor(x), a.calls)}
            if with_torch:
                routes["the tables by plain PyTorch, roll / & / sum"] = (lambda: torch_tables(pred, truth, R), a.torch_calls)
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
            ms = med(times["dc_displacement_score (nn.DisplacementSkill)"])
            ratio = f"{med(times['the tables by plain PyTorch, roll / & / sum']) / ms:.0f} x" if with_torch else "not run"
            print(f"    PyTorch / HIP = {ratio}; HIP / dc_distance_score = {ms / med(times['dc_distance_score (nn.DistanceSkill, R = 16)']):.2f}; "
                  f"HIP / dc_fss_score = {ms / med(times['dc_fss_score (nn.FractionsSkill, 7 windows)']):.2f}; HIP / forward pass = "
                  f"{100 * ms / med(times['forward pass (nn.Predictor, bf16)']):.2f} %")
            print(f"    workspace {L.load().dc_displacement_workspace(B, H, W, R) / 1e6:.2f} MB, tables {B * 2 * S * (S + 1) * 8 / 1e6:.2f} MB")
            del ds
    print("launches per call: 4 (and three memsets)")
    predictor.close()


if __name__ == "__main__":
    main()
