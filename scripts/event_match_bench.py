#!/usr/bin/env python3
"""Times the event matching at batch 8, 768 x 1152, on blob masks with event counts like the data's (a few dozen per sample): side a and
side b share most blobs, shifted by a few pixels, and each has some of its own.  Per library call, in one process:

  dc_mask_components, dc_component_stats   (one catalogue; the matcher runs two)
  dc_component_overlap, dc_event_scores    (the new calls)
  nn.EventMatcher                          (both catalogues, the overlap and the scores: one call)

The yardstick is dc_component_stats on the same masks: the overlap pass reads two label maps and two masks once (about 10 B per pixel),
the statistics call reads mask and labels in three passes (about 14 B per pixel), so the overlap should cost no more.  Every call is timed
with HIP events; a block's figure is the median of its calls, a call's figure the median of its blocks.

Where the overlap call's time goes is taken apart by calling it three more times on inputs that switch parts of its work off:

  pair_cap 64             the same masks and the same pairs (they fit), but 30 KiB of pair rows and table to clear instead of 3.5 MiB
  no foreground           all-zero masks and label maps: the pixel pass streams its 10 B per pixel and meets no pair at all
  ranks beyond the caps   the blob masks and label maps with rank maps that hold `cap` everywhere: the runs go through the workgroup's LDS
                          table and every flushed slot does its two rank lookups, but the coverage adds and the global pair table's
                          atomics are skipped

Only standard output belongs in the profile:

    python scripts/event_match_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/event_match.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
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


def blob_masks(rs, shared: int = 32, own: int = 8):
    """two uint8 [B, H, W]: `shared` ellipses per sample in both (shifted by up to 6 pixels and a little resized in b), `own` more in each"""
    rr, cc = np.mgrid[0:H, 0:W]

    def draw(m, r0, c0, a, bb, cl):
        dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
        m[((rr - r0) / a) ** 2 + (dc / bb) ** 2 <= 1.0] = cl

    ma, mb = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    for s in range(B):
        for k in range(shared + 2 * own):
            r0, c0, a, bb, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(4, 40), rs.randint(8, 120), rs.randint(1, 3)
            if k < shared or k < shared + own:
                draw(ma[s], r0, c0, a, bb, cl)
            if k < shared:
                draw(mb[s], (r0 + rs.randint(-6, 7)) % H, (c0 + rs.randint(-6, 7)) % W, max(a + rs.randint(-2, 3), 2), max(bb + rs.randint(-4, 5), 2), cl)
            elif k >= shared + own:
                draw(mb[s], r0, c0, a, bb, cl)
    return ma, mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--plain", action="store_true", help="leave the taking apart out (for a kernel trace: every launch is then of the real call)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rs = np.random.RandomState(7)
    cases = {"blobs (32 shared + 8 own ellipses per sample and side)": blob_masks(rs)}
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    m = dnn.EventMatcher(B, H, W)
    med = lambda fn: statistics.median(time_block(fn, a.calls) for _ in range(a.blocks))  # noqa: E731
    for name, (ha, hb) in cases.items():
        ta, tb = torch.from_numpy(ha).to(dev), torch.from_numpy(hb).to(dev)
        m(ta, tb)
        m(ta, tb)
        torch.cuda.synchronize()
        st, ca, cb = L.stream_ptr(), m.a, m.b
        label = lambda: L.call("dc_mask_components", B, B, H, W, L.dptr(ta), 8, 1, L.dptr(ca._labels), L.dptr(ca._ws), st)  # noqa: E731
        stats = lambda: L.call("dc_component_stats", B, B, H, W, L.dptr(ta), L.dptr(ca._labels), L.dptr(ca._wy), L.dptr(ca._cx),  # noqa: E731
                               L.dptr(ca._sx), ca.cap, L.dptr(ca._table), L.dptr(ca._ncomp), L.dptr(ca._ws), st)

        def overlap_call(mask_a, labels_a, rank_a, mask_b, labels_b, rank_b, pair_cap):
            return lambda: L.call("dc_component_overlap", B, B, H, W, L.dptr(mask_a), L.dptr(labels_a), L.dptr(rank_a), ca.cap, L.dptr(mask_b),
                                  L.dptr(labels_b), L.dptr(rank_b), cb.cap, pair_cap, L.dptr(m._pairs), L.dptr(m._npairs),
                                  L.dptr(m._cover_a), L.dptr(m._cover_b), L.dptr(m._ws), st)

        overlap = overlap_call(ta, ca._labels, ca._ws, tb, cb._labels, cb._ws, m.pair_cap)
        scores = lambda: L.call("dc_event_scores", B, B, ca.cap, L.dptr(ca._table), L.dptr(ca._ncomp), L.dptr(m._cover_a), cb.cap,  # noqa: E731
                                L.dptr(cb._table), L.dptr(cb._ncomp), L.dptr(m._cover_b), L.dptr(m._npairs), 0, m.cover_q,
                                L.dptr(m._scores), L.dptr(m.acc), st)
        t = {"dc_mask_components": med(label), "dc_component_stats": med(stats), "dc_component_overlap": med(overlap),
             "dc_event_scores": med(scores), "nn.EventMatcher": med(lambda: m(ta, tb))}
        # the overlap call taken apart (the catalogues' buffers still hold what the matcher's last call left)
        small = 64
        zero_mask, zero_labels = torch.zeros_like(ta), torch.zeros_like(ca._labels)
        far_a, far_b = torch.full_like(ca._labels, ca.cap), torch.full_like(cb._labels, cb.cap)
        parts = {f"pair_cap {small}": overlap_call(ta, ca._labels, ca._ws, tb, cb._labels, cb._ws, small),
                 "no foreground": overlap_call(zero_mask, zero_labels, ca._ws, zero_mask, zero_labels, cb._ws, m.pair_cap),
                 "ranks beyond the caps": overlap_call(ta, ca._labels, far_a, tb, cb._labels, far_b, m.pair_cap)}
        tp = {}
        for k, fn in ({} if a.plain else parts).items():
            tp[k] = med(fn)
            n = m._npairs.cpu().numpy()
            tp[k] = (tp[k], n[:, 0].tolist(), n[:, 1].tolist())
        m(ta, tb)
        pairs, flags = m.pairs()
        print(f"{name}: events per sample a {m.a.counts()[:, 0].tolist()}, b {m.b.counts()[:, 0].tolist()}; pairs stored {[len(p) for p in pairs]}, "
              f"overflow flags {flags}")
        for k, v in t.items():
            print(f"    {k:22s} {v:8.3f} ms/batch")
        print(f"    dc_component_overlap / dc_component_stats = {t['dc_component_overlap'] / t['dc_component_stats']:.2f}")
        if a.plain:
            continue
        print("  dc_component_overlap taken apart (the same call on inputs that switch parts of its work off):")
        for k, (v, stored, flag) in tp.items():
            print(f"    {k:22s} {v:8.3f} ms/batch   pairs stored {stored}, overflow flags {flag}")
        full, none, far = t["dc_component_overlap"], tp["no foreground"][0], tp["ranks beyond the caps"][0]
        print(f"    clearing 3.5 MiB instead of 30 KiB          {full - tp[f'pair_cap {small}'][0]:+8.3f} ms")
        print(f"    LDS table and rank lookups                  {far - none:+8.3f} ms   (ranks beyond the caps - no foreground)")
        print(f"    coverage adds and global pair table         {full - far:+8.3f} ms   (full call - ranks beyond the caps)")


if __name__ == "__main__":
    main()
