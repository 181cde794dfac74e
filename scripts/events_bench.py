#!/usr/bin/env python3
"""Times the event catalogue at batch 8, 768 x 1152, bf16, in one process:

  (a) nn.Predictor alone (the forward pass and the mask, as before);
  (b) nn.Predictor(events=True): the same plus the connected components of every mask on the device;
  (c) the catalogue alone (nn.EventCatalog) on two synthetic masks: a few dozen blobs per sample (what a detector's output looks like) and
      a 45 % random mask (the worst case for merges), with the time of each of its two library calls;
  (d) the host alternative on those masks: copy them to the host and label them on one CPU core with scipy.ndimage.label, per class and
      sample (no periodic columns, no statistics: less than the catalogue does); "not available" without scipy.

(a) and (b) alternate in blocks; every call is timed with HIP events, a block's figure is the median of its calls, a route's figure the
median of its blocks.  The model is untrained, so the masks of (b) are whatever its random weights give; (c) is the figure to read for a
given kind of mask.

    python scripts/events_bench.py [--blocks 5] [--calls 10] > profiles/events.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import nn as dnn  # noqa: E402

H, W, B = 768, 1152, 8


def time_block(fn, calls: int) -> float:
    """median milliseconds of `calls` calls, each between two HIP events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def blob_mask(rs, blobs: int = 40) -> np.ndarray:
    """uint8 [B, H, W]: `blobs` ellipses per sample, classes mixed, some across the seam"""
    m = np.zeros((B, H, W), np.uint8)
    rr, cc = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(blobs):
            r0, c0, a, bb = rs.randint(0, H), rs.randint(0, W), rs.randint(4, 40), rs.randint(8, 120)
            dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
            m[b][((rr - r0) / a) ** 2 + (dc / bb) ** 2 <= 1.0] = rs.randint(1, 3)
    return m


def host_label(mask_dev, connectivity: int = 8):
    """copy to the host, scipy.ndimage.label per class and sample on one core; seconds per batch, or None without scipy"""
    try:
        from scipy import ndimage
    except ImportError:
        return None, 0
    st = np.ones((3, 3), int) if connectivity == 8 else None
    best, n = None, 0
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = mask_dev.cpu().numpy()
        n = 0
        for b in range(host.shape[0]):
            for cl in (1, 2):
                n += ndimage.label(host[b] == cl, structure=st)[1]
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    plain = dnn.Predictor(net, B, H, W)
    events = dnn.Predictor(net, B, H, W, events=True)
    for fn in (plain, events):
        fn(x)
        fn(x)
    torch.cuda.synchronize()
    assert torch.equal(plain(x), events(x))
    ta, tb = [], []
    for _ in range(a.blocks):
        ta.append(time_block(lambda: plain(x), a.calls))
        tb.append(time_block(lambda: events(x), a.calls))
    ma, mb = statistics.median(ta), statistics.median(tb)
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (ta, tb))
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, bf16; {a.blocks} alternating blocks of {a.calls} calls, HIP events, medians")
    print(f"(a) nn.Predictor:               {ma:8.3f} ms/batch  {B / ma * 1e3:8.1f} samples/s   blocks " + " ".join(f"{t:.3f}" for t in ta))
    print(f"(b) nn.Predictor(events=True):  {mb:8.3f} ms/batch  {B / mb * 1e3:8.1f} samples/s   blocks " + " ".join(f"{t:.3f}" for t in tb))
    print(f"    (b) - (a) = {mb - ma:.3f} ms = {100 * (mb - ma) / ma:.2f} % of the forward pass (block spread {100 * spread:.2f} %); "
          f"components of the untrained model's masks: {events.catalog.counts().sum(0).tolist()}")
    events.close()
    plain.close()

    rs = np.random.RandomState(7)
    cases = {"blobs (40 ellipses per sample)": blob_mask(rs),
             "random 45 % foreground": ((rs.rand(B, H, W) < 0.45) * rs.randint(1, 3, (B, H, W))).astype(np.uint8)}
    cat = dnn.EventCatalog(B, H, W)
    from mlperf_deepcam_amd import lib as L
    for name, mask in cases.items():
        m = torch.from_numpy(mask).to(dev)
        cat(m)
        cat(m)
        torch.cuda.synchronize()
        total = statistics.median(time_block(lambda: cat(m), a.calls) for _ in range(a.blocks))
        st = L.stream_ptr()
        label = lambda: L.call("dc_mask_components", B, B, H, W, L.dptr(m), 8, 1, L.dptr(cat._labels), L.dptr(cat._ws), st)  # noqa: E731
        stats = lambda: L.call("dc_component_stats", B, B, H, W, L.dptr(m), L.dptr(cat._labels), L.dptr(cat._wy), L.dptr(cat._cx),  # noqa: E731
                               L.dptr(cat._sx), cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(cat._ws), st)
        t_label = statistics.median(time_block(label, a.calls) for _ in range(a.blocks))
        t_stats = statistics.median(time_block(stats, a.calls) for _ in range(a.blocks))
        t0 = time.perf_counter()
        ev = cat.events()
        t_read = time.perf_counter() - t0
        ncomp = cat.counts().cpu()
        host, nhost = host_label(m)
        print(f"(c) EventCatalog, {name}: {total:7.3f} ms/batch = {100 * total / ma:5.2f} % of (a)   dc_mask_components {t_label:.3f} ms, "
              f"dc_component_stats {t_stats:.3f} ms; components {ncomp[:, 0].tolist()} (largest table fill {max(len(e) for e in ev)} of {cat.cap}); "
              f"events() read-back and decoding {1e3 * t_read:.2f} ms")
        if host is None:
            print("(d) host alternative: not available (no scipy on this machine)")
        else:
            print(f"(d) host alternative, {name}: {1e3 * host:8.2f} ms/batch (device-to-host copy + scipy.ndimage.label per class and sample, one core, "
                  f"best of 3; {nhost} components without periodic columns) = {host * 1e3 / total:.1f} x (c)")


if __name__ == "__main__":
    main()
