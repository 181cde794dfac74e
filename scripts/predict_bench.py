#!/usr/bin/env python3
"""Times inference at batch 8, 768 x 1152, bf16 through two routes in one process:

  (a) what existed before nn.Predictor: the train-capable Engine(8, ...).forward(train=False), then torch.max(logits, 1)[1]
      (fp32 NCHW logits written and read back, an int64 mask);
  (b) nn.Predictor at batch 8: forward-only engine, the uint8 mask written by the classifier's kernel.

The routes alternate in blocks (a b a b ...); every call is timed with HIP events, a block's figure is the median of its calls, a
route's figure the median of its blocks, and the block-to-block spread (max - min of a route's block medians, relative to its median) is
printed beside it.  Also: library launches per call and the device memory each route's engine holds.

    python scripts/predict_bench.py [--blocks 5] [--calls 10] > profiles/predict.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from mlperf_deepcam_amd.engine import Engine  # noqa: E402

H, W, B = 768, 1152, 8


def count_launches(fn) -> int:
    real, n = L.call, [0]

    def spy(name, *args):
        n[0] += 1
        return real(name, *args)
    L.call = spy
    try:
        fn()
    finally:
        L.call = real
    return n[0]


def time_block(fn, calls: int) -> float:
    """median milliseconds of `calls` calls, each between two HIP events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    m0 = torch.cuda.memory_allocated()
    eng = Engine(B, H, W, torch.bfloat16, share_from=net.engine)
    m1 = torch.cuda.memory_allocated()
    pred = dnn.Predictor(net, B, H, W)
    m2 = torch.cuda.memory_allocated()
    keep = {}

    def route_a():
        keep["a"] = torch.max(eng.forward(x, train=False), 1)[1]

    def route_b():
        keep["b"] = pred(x)

    for fn in (route_a, route_b):            # warm-up: weight repack, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    same = float((keep["a"] == keep["b"].long()).float().mean())
    la, lb = count_launches(route_a), count_launches(route_b)
    ta, tb = [], []
    for _ in range(a.blocks):
        ta.append(time_block(route_a, a.calls))
        tb.append(time_block(route_b, a.calls))
    ma, mb = statistics.median(ta), statistics.median(tb)
    sa, sb = (max(ta) - min(ta)) / ma, (max(tb) - min(tb)) / mb
    print(f"batch {B}, {H} x {W}, bf16; {a.blocks} alternating blocks of {a.calls} calls, HIP events, medians")
    print(f"(a) Engine({B}).forward(train=False) + torch.max: {ma:8.3f} ms/batch  {B / ma * 1e3:8.1f} samples/s  block spread {100 * sa:5.2f} %  "
          f"{la:4d} launches  engine {(m1 - m0) / 2 ** 30:6.2f} GiB   blocks " + " ".join(f"{t:.3f}" for t in ta))
    print(f"(b) nn.Predictor({B}):                              {mb:8.3f} ms/batch  {B / mb * 1e3:8.1f} samples/s  block spread {100 * sb:5.2f} %  "
          f"{lb:4d} launches  engine {(m2 - m1) / 2 ** 30:6.2f} GiB   blocks " + " ".join(f"{t:.3f}" for t in tb))
    spread = max(sa, sb)
    verdict = "faster beyond the block spread" if mb < ma * (1 - spread) else \
        ("SLOWER beyond the block spread" if mb > ma * (1 + spread) else "equal within the block spread")
    print(f"(a) / (b) = {ma / mb:.3f}x  -> Predictor is {verdict} ({100 * spread:.2f} %)")
    print(f"masks of the two routes agree on {100 * same:.4f} % of the pixels (the routes pick tiles of their own: other summation orders)")
    pred.close()


if __name__ == "__main__":
    main()
