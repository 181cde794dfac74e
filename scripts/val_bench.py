#!/usr/bin/env python3
"""Times the validation pass at 768 x 1152 in bf16 through two paths in one process:

  (a) the loop of train.py at --validation_batch_size 1: batch-1 engine, wce_fused, counts.cpu() per sample;
  (b) nn.ValStep at batch 8: forward-only engine, per-sample score behind the classifier, sums kept on the device.

For both: samples/s, library launches per sample and peak device memory (torch.cuda.max_memory_allocated; each path is built, timed and
freed before the other is built).  --deviation also prints the largest per-sample deviation of path (a) from the fp32 CPU oracle on the
two full-size samples tests/test_val_gpu.py uses (minutes of CPU).

    python scripts/val_bench.py [--samples 64] [--deviation] > profiles/val_step.txt"""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402

H, W, VB = 768, 1152, 8


class Counter:
    def __init__(self):
        self.n, self.real = 0, L.call

    def __enter__(self):
        def spy(name, *args):
            self.n += 1
            return self.real(name, *args)
        L.call = spy
        return self

    def __exit__(self, *exc):
        L.call = self.real


def path_a(net, cw, x, y, n):
    eng = net.engine_for(shape=(1, 16, H, W))
    sums = torch.zeros(3, dtype=torch.float64, device=x.device)
    for i in range(n):
        j = i % x.shape[0]
        out = eng.forward(x[j:j + 1], train=False)
        counts = torch.zeros(9, dtype=torch.int64, device=x.device)
        ls = dnn.wce_fused(out, y[j:j + 1], cw, counts=counts)
        sums[0] += 1.0
        sums[1] += ls[0] / y[j].numel()
        sums[2] += dnn.iou_from_counts(counts.cpu().tolist())
    return sums.cpu().tolist()


def path_b(vs, x, y, n):
    vs.reset()
    for _ in range(n // VB):
        vs(x, y)
    return list(vs.result())


def timed(fn, n):
    fn(VB)                                   # warm-up: weight repack, allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with Counter() as c:
        t0 = time.perf_counter()
        res = fn(n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return res, n / dt, c.n / n, torch.cuda.max_memory_allocated() / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--deviation", action="store_true")
    a = ap.parse_args()
    n = a.samples // VB * VB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cw = dnn.class_weights(-0.125)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(VB, 16, H, W, generator=g).to(dev)
    y = torch.randint(0, 3, (VB, H, W), generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)                 # the batch-1 engine is the primary one: path (a) as train.py runs it
    net.eval()
    base = torch.cuda.memory_allocated() / 2 ** 30
    ra, sa, la, ma = timed(lambda k: path_a(net, cw, x, y, k), n)
    print(f"(a) batch-1 engine + wce_fused + counts.cpu(): {sa:8.1f} samples/s  {la:6.1f} launches/sample  peak {ma:6.2f} GiB "
          f"(engine and weights resident: {base:.2f} GiB)   mean loss {ra[1] / ra[0]:.6f} iou {ra[2] / ra[0]:.6f}")
    vs = dnn.ValStep(net, cw, VB, H, W)
    rb, sb, lb, mb = timed(lambda k: path_b(vs, x, y, k), n)
    print(f"(b) ValStep batch {VB}:                           {sb:8.1f} samples/s  {lb:6.1f} launches/sample  peak {mb:6.2f} GiB "
          f"(of which the batch-1 engine of (a): {base:.2f} GiB)   mean loss {rb[1] / rb[0]:.6f} iou {rb[2] / rb[0]:.6f}")
    print(f"    forward-only engine activations: {vs.eng.act_bytes / 2 ** 30:.2f} GiB pooled, {vs.eng.act_bytes_unpooled / 2 ** 30:.2f} GiB one buffer each")
    print(f"(b) / (a) = {sb / sa:.2f}x  -> " + ("faster by more than the +-3 % run spread" if sb > 1.03 * sa else "NOT faster beyond the +-3 % run spread"))
    vs.close()
    del vs
    gc.collect()
    if a.deviation:
        import util_val
        import test_val_gpu as T
        state = util_val.perturbed_state()
        xs, ys = util_val.val_inputs(n=2, h=H, w=W, seed=util_val.INPUT_SEED + 70)
        net.load_state_dict(state)
        old = T._existing_path(net, xs, ys)
        torch.set_num_threads(16)
        ora = T._oracle_per_sample(state, xs, ys)
        print("existing batch-1 bf16 path vs fp32 oracle, 768 x 1152, max per-sample rel (loss, iou):", T._max_rel(old, ora))


if __name__ == "__main__":
    main()
