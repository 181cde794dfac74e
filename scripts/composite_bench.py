#!/usr/bin/env python3
"""Times the storm-centred composites at batch 8, 768 x 1152, 16 channels, R = 32, 40 radial bins, one group, in one process, beside the
Predictor's forward pass (bf16) and dc_component_fields on the same batch:

  dc_composite_centers      (one thread per catalogue row)
  dc_composite_accumulate   (the gather: events * S^2 * 64 bytes of field values)
  nn.StormComposite         (both)

on the blob masks of scripts/events_bench.py (40 ellipses per sample, about 33 events) and on 45 % random foreground, where every
sample fills the catalogue's cap.  Both classes are composited so that every event takes part.  Every call is timed with HIP events, a
block's figure is the median of its calls, a call's figure the median of its blocks.  There is no time to meet; the ratios to
dc_component_fields and to the forward pass and the gather's bytes per second are printed.

    python scripts/composite_bench.py [--blocks 5] [--calls 10] > profiles/composite.txt"""
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

CH, R, BINS = 16, 32, 40


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
    del plain, net, x
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W} x {CH}, R = {R}, {BINS} bins, one group; {a.blocks} blocks of {a.calls} "
          f"calls, HIP events, medians")
    print(f"nn.Predictor (bf16 forward pass and mask): {fwd:8.3f} ms/batch")
    rs = np.random.RandomState(7)
    fields = (torch.rand(B, H, W, CH, generator=torch.Generator().manual_seed(9)) * 1000.0).to(dev)
    cases = {"blobs (40 ellipses per sample)": blob_mask(rs),
             "random 45 % foreground": ((rs.rand(B, H, W) < 0.45) * rs.randint(1, 3, (B, H, W))).astype(np.uint8)}
    S = 2 * R + 1
    for name, mask in cases.items():
        cat = dnn.EventCatalog(B, H, W)                 # the default cap: events beyond it have no row
        ef = dnn.EventFields(cat, CH, dnn.event_field_bits([0.0] * CH, [1000.0] * CH))
        comp = dnn.StormComposite(ef, 0, radius=R, bits=dnn.composite_bits([0.0] * CH, [1000.0] * CH), classes=(1, 2), bins=BINS)
        m = torch.from_numpy(mask).to(dev)
        for _ in range(2):
            cat(m)
            ef(fields)
            comp(fields)
        torch.cuda.synchronize()
        st = L.stream_ptr()
        table = comp._tables[(0,) * B]
        centers = lambda: L.call("dc_composite_centers", B, B, H, W, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(ef._ftable),  # noqa: E731
                                 ef.C, 0, 0, comp.class_mask, 0, L.dptr(table), 1, None, 0, L.dptr(comp._centers), L.dptr(comp._egroup),
                                 L.dptr(comp._counts), st)
        gather = lambda: L.call("dc_composite_accumulate", B, B, H, W, cat.cap, R, 1, L.dptr(comp._centers), L.dptr(comp._egroup),  # noqa: E731
                                L.dptr(cat._table), L.dptr(cat._labels), L.dptr(fields), CH, CH, None, L.dptr(comp._bits), 0, 1,
                                L.dptr(comp._rbin), BINS, L.dptr(comp._events), L.dptr(comp._sum), L.dptr(comp._n), L.dptr(comp._inside),
                                L.dptr(comp._rsum), L.dptr(comp._rn), st)
        t = {"dc_component_fields": med(lambda: ef(fields)), "dc_composite_centers": med(centers), "dc_composite_accumulate": med(gather),
             "nn.StormComposite": med(lambda: comp(fields))}
        comp.reset()
        comp(fields)
        torch.cuda.synchronize()
        state = comp.state()
        events = int(state["events"].sum())
        moved = events * S * S * CH * 4
        print(f"{name}: events per sample {cat.counts()[:, 0].cpu().tolist()} (cap {cat.cap}); one call: {state['counts']}")
        for k, v in t.items():
            print(f"    {k:24s} {v:9.3f} ms/batch = {100 * v / fwd:7.2f} % of the forward pass")
        acc = t["dc_composite_accumulate"]
        print(f"    dc_composite_accumulate / dc_component_fields = {acc / t['dc_component_fields']:.2f}; the gather moves {events} events x "
              f"{S} x {S} x {CH * 4} B = {moved / 1e6:.1f} MB: {moved / acc / 1e9:.3f} TB/s")


if __name__ == "__main__":
    main()
