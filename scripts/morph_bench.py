#!/usr/bin/env python3
"""Times the mask morphology (nn.MaskMorphology: dc_mask_morph, csrc/morph.hip) at batch 8, 768 x 1152, wrap on:

  closing(2), fill, opening(3)   one program for both classes each: morph_planes (one workgroup per class and frame, the plane in LDS)
                                 and morph_compose (one streaming pass) together, as a call issues them
  the driver's chain             closing(2) + fill + opening by reconstruction(3), what predict.py --morph_close 2 2 --morph_fill
                                 --morph_open 3 3 --morph_open_reconstruct runs
  rounds per FILL                the relaxation rounds of the fill program, per frame and class (the final empty round counted)
against three yardsticks from the same job: dc_mask_thin on the same masks, nn.Predictor's forward pass of the batch, and the same steps
with torch.roll and Boolean operators on the same GPU (both classes as one [16, H, W] bool tensor; its fill grows one pixel a round for
the rounds a host loop found necessary, without a convergence test on the device), whose mask is compared with the kernel's.

Measurement: two untimed calls, then --blocks blocks of --calls consecutive calls; a block is timed with HIP events, a block's figure is
the median of its calls, a call's figure the median of its blocks.  There is no time to meet.  A program is serial in its steps and 16
workgroups run at batch 8: where FILL takes longer than the forward pass the script says so.

    python scripts/morph_bench.py [--blocks 5] [--calls 10] > profiles/morph.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from events_bench import B, H, W, blob_mask, time_block  # noqa: E402
from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402

N4 = [(-1, 0), (1, 0), (0, -1), (0, 1)]
N8 = N4 + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def moved(x, dr, dc, pad):
    """x[r + dr, c + dc]: columns periodic, rows outside the frame `pad`"""
    y = torch.roll(x, shifts=(-dr, -dc), dims=(1, 2))
    if dr:
        y[:, -1 if dr > 0 else 0] = pad
    return y


def torch_steps(x, steps, rounds):
    """the header's operators on a bool tensor [N, H, W]; a propagation runs `rounds` rounds of one pixel each"""
    orig = x
    for step in steps:
        if step[0] in ("dilate", "erode"):
            for j in range(1, step[1] + 1):
                near = [moved(x, *d, step[0] == "erode") for d in (N4 if j % 2 else N8)]
                for y in near:
                    x = (x | y) if step[0] == "dilate" else (x & y)
        else:
            inside = ~x if step[0] == "fill" else orig
            seed = torch.zeros_like(x)
            if step[0] == "fill":
                seed[:, 0], seed[:, -1] = inside[:, 0], inside[:, -1]
            else:
                seed = x & orig
            for _ in range(rounds):
                grown = seed
                for d in (N4 if step[0] == "fill" else N8):
                    grown = grown | moved(seed, *d, False)
                seed = grown & inside
            x = ~seed if step[0] == "fill" else seed
    return x


def torch_rounds(x, steps):
    """the rounds the slowest propagation of `steps` needs on x, found with a convergence test on the host"""
    hi = 2
    while not torch.equal(torch_steps(x, steps, hi), torch_steps(x, steps, hi + 1)):
        hi *= 2
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    med = lambda fn, calls=a.calls: statistics.median(time_block(fn, calls) for _ in range(a.blocks))  # noqa: E731
    x = torch.rand(B, 16, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    plain = dnn.Predictor(net, B, H, W)
    plain(x)
    plain(x)
    torch.cuda.synchronize()
    fwd = med(lambda: plain(x))
    plain.close()
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls, HIP events, medians")
    print(f"nn.Predictor (bf16 forward pass and mask): {fwd:8.3f} ms/batch")
    print(f"LDS per workgroup: {L.load().dc_thin_lds_bytes(H, W)} bytes; {2 * B} workgroups of morph_planes")
    MM = dnn.MaskMorphology
    programs = {"closing(2)": MM.closing(2), "fill": [("fill",)], "opening(3)": MM.opening(3),
                "chain: closing(2), fill, opening by reconstruction(3)": MM.closing(2) + [("fill",)] + MM.opening_by_reconstruction(3)}
    rs = np.random.RandomState(7)
    cases = {"blobs (8 ellipses per sample)": blob_mask(rs, 8),
             "uniform random: a third each of background, class 1 and class 2": rs.randint(0, 3, (B, H, W)).astype(np.uint8)}
    for name, mask in cases.items():
        m = torch.from_numpy(mask).to(dev)
        planes = torch.cat([m == 1, m == 2])
        skel, iters = torch.empty_like(m), torch.zeros((B, 2, 2), dtype=torch.int32, device=dev)
        st = L.stream_ptr()
        thin = lambda: L.call("dc_mask_thin", B, B, H, W, L.dptr(m), 1, 1, max(H, W), L.dptr(skel), L.dptr(iters), st)  # noqa: E731
        thin()
        thin()
        t_thin = med(thin)
        print(f"{name}: {100 * float((mask == 0).mean()):.1f} % background")
        print(f"    {'dc_mask_thin':58s} {t_thin:8.3f} ms/batch = {100 * t_thin / fwd:6.2f} % of the forward pass")
        for label, steps in programs.items():
            mm = MM(B, H, W, steps)
            mm(m)
            mm(m)
            torch.cuda.synchronize()
            t = med(lambda: mm(m))
            rounds, out = mm.rounds(), mm.mask_buffer
            need = torch_rounds(planes, steps) if any(s[0] in ("fill", "reconstruct") for s in steps) else 0
            x1, x2 = torch_steps(planes, steps, need).chunk(2)
            ref = torch.where((m == 1) & x1, 1, torch.where((m == 2) & x2, 2, torch.where(x1, 1, torch.where(x2, 2, 0)))).to(torch.uint8)
            same = bool(torch.equal(ref, out))
            t_torch = med(lambda: torch_steps(planes, steps, need), max(a.calls // 5, 1))
            moved_px = [[sum(f[j][k] for f in mm.counts()) for k in ("added", "removed")] for j in range(2)]
            print(f"    {label:58s} {t:8.3f} ms/batch = {100 * t / fwd:6.2f} % of the forward pass, {100 * t / t_thin:6.1f} % of dc_mask_thin; "
                  f"torch {t_torch:8.3f} ms = {t_torch / t:.1f} x ({need} rounds a propagation); mask equals torch's: {same}; "
                  f"converged {bool((mm.converged() == 1).all())}; pixels added, removed per class {moved_px}")
            if label == "fill":
                print(f"        rounds per FILL, per frame (class 1, class 2): {rounds[:, :, 0].tolist()}")
                if t > fwd:
                    print("        FILL takes LONGER than the batch's forward pass: the rounds are serial and only 16 of the CUs work")


if __name__ == "__main__":
    main()
