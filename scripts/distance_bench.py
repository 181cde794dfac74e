#!/usr/bin/env python3
"""Times the distance-map verification (dc_distance_score; nn.DistanceSkill) at batch 8, 768 x 1152, periodic columns, for the caps R = 16,
32 and 64 and two kinds of input -- sparse frames of about 97 % background (ellipses, the prediction a displaced copy of the labels with
some objects of its own) and uniform-random frames (every pixel 0, 1 or 2 with equal probability, independently on both sides: every
distance is 0 to 2 and the walk over the columns ends at once) -- and prints beside each figure

  the same call with keep_maps (the four uint16 maps are stored as well);
  dc_fss_score (nn.FractionsSkill, the default windows) on the same masks, and the forward pass of the same batch (nn.Predictor, bf16),
      the thing both scores run behind, in the same process;
  the same maps through plain PyTorch operators on the same GPU: two passes of 2 R + 1 torch.roll / torch.minimum steps on int32 (the row
      distances, then dx^2 + g^2), checked for equality with the HIP maps before it is timed.  It makes the maps only, not the scores.

The HIP maps of the full-size batch are compared with the PyTorch maps, and the HIP rows of its first frame with the rows the numpy checker
of tests/util_distance.py derives from those maps (its own non-separable transform would need hours at this size).  Every call is timed
with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks.  Only standard output belongs in
the profile:

    python scripts/distance_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/distance.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, time_block  # noqa: E402

RADII = (16, 32, 64)


def sparse_masks(rs, objects: int = 40, own: int = 4):
    """two uint8 [B, H, W] of about 97 % background: `objects` ellipses per sample in the labels, copied into the prediction displaced by
    up to 12 pixels, except `own` of them that only one side has"""
    rr, cc = np.mgrid[0:H, 0:W]

    def draw(m, r0, c0, a, bb, cl):
        dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
        m[((rr - r0) / a) ** 2 + (dc / bb) ** 2 <= 1.0] = cl

    pred, truth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    for s in range(B):
        for k in range(objects + own):
            r0, c0, a, bb, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(3, 16), rs.randint(6, 40), rs.randint(1, 3)
            if k < objects:
                draw(truth[s], r0, c0, a, bb, cl)
            if k >= own:
                draw(pred[s], r0 + rs.randint(-12, 13), (c0 + rs.randint(-12, 13)) % W, a, bb, cl)
    return pred, truth


def torch_maps(pred: torch.Tensor, truth: torch.Tensor, R: int) -> torch.Tensor:
    """int32 [B, 2, 2, H, W] by plain PyTorch operators: the row distances by 2 R + 1 rolls along the rows (what rolls in from the other
    pole is cleared), then min over dx of dx^2 + g^2 by 2 R + 1 periodic rolls along the columns"""
    ind = torch.stack([pred == 1, pred == 2, truth == 1, truth == 2], dim=1)                           # [B, 4, H, W]
    far = torch.full(ind.shape, R + 1, dtype=torch.int32, device=ind.device)
    g = far.clone()
    for dy in range(-R, R + 1):
        shifted = torch.roll(ind, dy, dims=2)
        if dy > 0:
            shifted[:, :, :dy] = False
        elif dy < 0:
            shifted[:, :, dy:] = False
        g = torch.minimum(g, torch.where(shifted, abs(dy), far))
    g2 = g * g
    cap = R * R + 1
    d2 = torch.full(ind.shape, cap, dtype=torch.int32, device=ind.device)
    for dx in range(-R, R + 1):
        d2 = torch.minimum(d2, torch.roll(g2, dx, dims=3) + dx * dx)
    return d2.view(pred.shape[0], 2, 2, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--torch_calls", type=int, default=3, help="calls per block of the PyTorch evaluation (it takes a thousand times longer)")
    a = ap.parse_args()
    import util_distance as ud
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, caps {list(RADII)}, periodic columns; {a.blocks} blocks of {a.calls} calls "
          f"per figure ({a.torch_calls} for PyTorch), HIP events, medians")
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
    for kind, (pred_h, truth_h) in kinds.items():
        pred, truth = torch.from_numpy(pred_h).to(dev), torch.from_numpy(truth_h).to(dev)
        background = 1.0 - float(((truth_h == 1) | (truth_h == 2)).mean())
        print(f"{kind}: {100 * background:.1f} % of the labels and {100 * (1.0 - float(((pred_h == 1) | (pred_h == 2)).mean())):.1f} % of the "
              f"prediction are background")
        for R in RADII:
            ds, dm = dnn.DistanceSkill(B, H, W, radius=R, device=dev), dnn.DistanceSkill(B, H, W, radius=R, keep_maps=True, device=dev)
            ds(pred, truth), dm(pred, truth)
            ref = torch_maps(pred, truth, R)
            maps_equal = torch.equal(ref, dm.maps().view(torch.int16).to(torch.int32))    # values below 2^15
            rows, bad = (t.cpu().numpy() for t in ds.frame_rows())
            rows_m, bad_m = (t.cpu().numpy() for t in dm.frame_rows())
            want_rows, want_bad = ud.rows_from_maps(ref[0].cpu().numpy().astype(np.int64), R)
            rows_equal = np.array_equal(rows[0], want_rows) and np.array_equal(bad[0], want_bad) and np.array_equal(rows, rows_m) \
                and np.array_equal(bad, bad_m)
            print(f"  R = {R}: HIP maps against the PyTorch maps: {'equal' if maps_equal else 'DIFFERENT'}; HIP rows of frame 0 against the "
                  f"checker's rows of those maps, and with against without keep_maps: {'equal' if rows_equal else 'DIFFERENT'}")
            c = ds.result()["class_1"]
            fmt = lambda v: "none" if v is None else f"{v:.3f}"  # noqa: E731
            print(f"    class 1: MED miss {fmt(c['med_miss'])} false alarm {fmt(c['med_false_alarm'])} px, beyond {fmt(c['beyond_miss'])} / "
                  f"{fmt(c['beyond_false_alarm'])}, POD within 0 / 4 / R {fmt(c['pod_within'][0])} / {fmt(c['pod_within'][4])} / "
                  f"{fmt(c['pod_within'][R])}, Hausdorff q90 {c['hausdorff_q90']}, Baddeley {fmt(c['baddeley'])}")
            del ref
            routes = {"dc_distance_score (nn.DistanceSkill)": (lambda: ds(pred, truth), a.calls),
                      "dc_distance_score with keep_maps": (lambda: dm(pred, truth), a.calls),
                      "dc_fss_score (nn.FractionsSkill, 7 windows)": (lambda: fs(pred, truth), a.calls),
                      "forward pass (nn.Predictor, bf16)": (lambda: predictor(x), a.calls),
                      "the maps by plain PyTorch, roll / minimum": (lambda: torch_maps(pred, truth, R), a.torch_calls)}
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
            ms = med(times["dc_distance_score (nn.DistanceSkill)"])
            print(f"    PyTorch maps / HIP with keep_maps = {med(times['the maps by plain PyTorch, roll / minimum']) / med(times['dc_distance_score with keep_maps']):.0f} x; "
                  f"HIP / dc_fss_score = {ms / med(times['dc_fss_score (nn.FractionsSkill, 7 windows)']):.2f}; HIP / forward pass = "
                  f"{100 * ms / med(times['forward pass (nn.Predictor, bf16)']):.2f} %")
            del ds, dm
    print(f"workspace {B * H * W * 4 / 1e6:.1f} MB (one packed word per pixel), with keep_maps {B * 4 * H * W * 2 / 1e6:.1f} MB of maps; launches per call: 3")
    predictor.close()


if __name__ == "__main__":
    main()
