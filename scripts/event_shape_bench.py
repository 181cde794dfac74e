#!/usr/bin/env python3
"""Times the event shapes and the shape filter at batch 8, 768 x 1152, in one process, beside the Predictor's forward pass (bf16):

  dc_component_stats   (the yardstick: the parent commit has it, and it reads the same label map)
  dc_component_shape   (nn.EventShape: faces and spherical moments per event)
  dc_event_select      (one thread per event row)
  dc_mask_select       (the filtered mask, one streaming pass)
  nn.EventFilter       (catalogue + shape + select + mask-select)

on the two masks of scripts/events_bench.py: 40 blobs per sample and 45 % random foreground.  Every call is timed with HIP events, a
block's figure is the median of its calls, a call's figure the median of its blocks.  There is no time to meet; the ratio
dc_component_shape / dc_component_stats is printed, and above about 3 a kernel trace of its own has to say why.

    python scripts/event_shape_bench.py [--blocks 5] [--calls 10] > profiles/event_shape.txt"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    med = lambda fn: statistics.median(time_block(fn, a.calls) for _ in range(a.blocks))  # noqa: E731
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
    rs = np.random.RandomState(7)
    cases = {"blobs (40 ellipses per sample)": blob_mask(rs),
             "random 45 % foreground": ((rs.rand(B, H, W) < 0.45) * rs.randint(1, 3, (B, H, W))).astype(np.uint8)}
    for name, mask in cases.items():
        cat = dnn.EventCatalog(B, H, W)                 # the default cap, as in events_bench.py: events beyond it have no row
        filt = dnn.EventFilter(cat, min_pixels=(3, 10), min_length_km=(0, 2000), min_aspect=(0, 2))
        sh = filt.shape
        m = torch.from_numpy(mask).to(dev)
        filt(m)
        filt(m)
        torch.cuda.synchronize()
        st = L.stream_ptr()
        stats = lambda: L.call("dc_component_stats", B, B, H, W, L.dptr(m), L.dptr(cat._labels), L.dptr(cat._wy), L.dptr(cat._cx),  # noqa: E731
                               L.dptr(cat._sx), cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(cat._ws), st)
        select = lambda: L.call("dc_event_select", B, B, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(sh._shape),  # noqa: E731
                                L.dptr(filt._criteria), L.dptr(filt._keep), L.dptr(filt._counts), st)
        pick = lambda: L.call("dc_mask_select", B, B, H, W, L.dptr(m), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(filt._keep),  # noqa: E731
                              L.dptr(filt._out), L.dptr(filt._counts), st)
        t = {"dc_component_stats": med(stats), "dc_component_shape": med(lambda: sh()), "dc_event_select": med(select),
             "dc_mask_select": med(pick), "nn.EventFilter": med(lambda: filt(m))}
        filt(m)
        torch.cuda.synchronize()
        counts = filt.counts().sum(0).cpu().tolist()
        print(f"{name}: events per sample {cat.counts()[:, 0].cpu().tolist()} (cap {cat.cap}); kept / dropped events and pixels per class {counts}")
        for k, v in t.items():
            print(f"    {k:20s} {v:8.3f} ms/batch = {100 * v / fwd:5.2f} % of the forward pass")
        print(f"    dc_component_shape / dc_component_stats = {t['dc_component_shape'] / t['dc_component_stats']:.2f}")


if __name__ == "__main__":
    main()
