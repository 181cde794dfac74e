#!/usr/bin/env python3
"""Times the frame renderer (dc_render_frames, nn.FrameRenderer) at batch 8, 768 x 1152 x 16, two panels, Gall rows (885 per panel), on
the blob masks of scripts/event_match_bench.py, and puts the figure beside the forward pass of the same process:

  dc_render_frames       HIP-event time per batch, median of blocks of calls after warm-up, and its two launches apart (the outline pass
                         alone is the call at Ho = 1: its gather then touches one output row)
  bytes per second       against the traffic estimate: per sample the field rows that are shown, one 64-byte segment per pixel at
                         ldc = 16 (H * W * 64 B when every source row is shown), the masks (1 B per pixel and panel, read with their
                         halo), the paint bytes written and read (2 B per pixel and panel) and the RGB bytes (3 B per output pixel and
                         panel)
  nn.Predictor           samples/s of the bf16 forward pass at batch 8 as scripts/predict_bench.py times it, alone and with the renderer
                         called on every batch and its RGB bytes copied to a pinned host buffer (no PNG), in alternating blocks

Only standard output belongs in the profile:

    python scripts/render_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/render.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, blob_masks, time_block  # noqa: E402

CH = 16


def traffic_bytes(r: "dnn.FrameRenderer", rows_shown: int) -> dict:
    """bytes per batch the algorithm needs, from the shapes (the field term counts a whole 64-byte segment per pixel of a shown row)"""
    px, opx = H * W, r.Ho * W
    return {"fields": B * rows_shown * W * 4 * r.ldc, "masks": B * r.P * px, "paint": B * r.P * (px + opx), "rgb": B * r.P * opx * 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no_forward", action="store_true", help="leave the forward-pass comparison out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W} x {CH}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    rs = np.random.RandomState(7)
    ma, mb = (torch.from_numpy(m).to(dev) for m in blob_masks(rs))
    lo = np.linspace(-50.0, 200.0, CH).astype(np.float32)
    span = np.linspace(1.0, 300.0, CH).astype(np.float32)
    fields = torch.from_numpy(lo + rs.random_sample((B, H, W, CH)).astype(np.float32) * span).to(dev)
    r = dnn.FrameRenderer(B, H, W, channel=0, ldc=CH, lo=float(lo[0]), hi=float(lo[0] + span[0]), panels=2, device=dev)
    one_row = dnn.FrameRenderer(B, H, W, channel=0, ldc=CH, lo=float(lo[0]), hi=float(lo[0] + span[0]), panels=2, device=dev,
                                projection=np.zeros(1, np.int32))
    lb = mb.long()                                                  # labels arrive as int64
    med = lambda fn: statistics.median(time_block(fn, a.calls) for _ in range(a.blocks))  # noqa: E731
    for _ in range(3):                                                # warm-up: code objects
        r(fields, ma, mb)
        one_row(fields, ma, mb)
        r(fields, ma, lb)
    torch.cuda.synchronize()
    t_full = med(lambda: r(fields, ma, mb))
    t_paint = med(lambda: one_row(fields, ma, mb))
    t_i64 = med(lambda: r(fields, ma, lb))
    shown = len(np.unique(np.clip(r.rows, 0, H - 1)))
    tb = traffic_bytes(r, shown)
    total = sum(tb.values())
    print(f"two panels, Gall rows: Ho = {r.Ho} output rows per panel showing {shown} of {H} source rows, outline width {r.outline}")
    print(f"    dc_render_frames (uint8 masks)            {t_full:8.3f} ms/batch  {t_full / B:7.3f} ms/sample")
    print(f"    dc_render_frames (labels as int64)        {t_i64:8.3f} ms/batch  {t_i64 / B:7.3f} ms/sample")
    print(f"    at Ho = 1: render_paint + one output row  {t_paint:8.3f} ms/batch   -> render_gather about {t_full - t_paint:.3f} ms/batch")
    print("    traffic estimate per batch: " + ", ".join(f"{k} {v / 1e6:.1f} MB" for k, v in tb.items()) + f"; total {total / 1e6:.1f} MB "
          f"({total / B / 1e6:.1f} MB per sample)")
    print(f"    {total / (t_full * 1e-3) / 1e9:8.1f} GB/s of the estimate over the call's time")
    if a.no_forward:
        return
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    pred = dnn.Predictor(net, B, H, W)
    host = torch.empty((B, r.P * r.Ho, W, 3), dtype=torch.uint8).pin_memory()

    def forward():
        pred(x)

    def forward_render():
        pred(x)
        host.copy_(r(fields, pred.mask_buffer, lb), non_blocking=True)

    for fn in (forward, forward_render):
        fn()
        fn()
    torch.cuda.synchronize()
    ta, tr = [], []
    for _ in range(a.blocks):
        ta.append(time_block(forward, a.calls))
        tr.append(time_block(forward_render, a.calls))
    fa, fr = statistics.median(ta), statistics.median(tr)
    sa, sr = (max(ta) - min(ta)) / fa, (max(tr) - min(tr)) / fr
    print(f"nn.Predictor({B}), bf16, alternating blocks:")
    print(f"    forward alone                             {fa:8.3f} ms/batch  {fa / B:7.3f} ms/sample  {B / fa * 1e3:8.1f} samples/s  block spread "
          f"{100 * sa:5.2f} %")
    print(f"    forward + render + copy to pinned memory  {fr:8.3f} ms/batch  {fr / B:7.3f} ms/sample  {B / fr * 1e3:8.1f} samples/s  block spread "
          f"{100 * sr:5.2f} %")
    print(f"    render and copy add {fr - fa:.3f} ms/batch = {(fr - fa) / B:.3f} ms/sample, {100 * (fr - fa) / fa:.1f} % of the forward pass "
          f"(render alone above: {t_i64 / B:.3f} ms/sample; the copy is {host.numel() / 1e6:.1f} MB per batch)")
    pred.close()


if __name__ == "__main__":
    main()
