#!/usr/bin/env python3
"""Times the track verification (nn.TrackMatcher: dc_track_match_append per batch, dc_track_match_resolve when results are read) at
batch 8, 768 x 1152, on the moving blobs of scripts/track_bench.py on both sides: the prediction is --blobs ellipses (default 96) that
are born, drift and die inside a series of 64 frames; the labels are the same scene moved by 2 rows and 5 columns plus --extra blobs of
their own (default 24), so that most storms have a partner and some have none.  In one process:

  per batch     nn.EventMatcher (both catalogues, dc_component_overlap, dc_event_scores), dc_component_overlap alone (issued again on the
                matcher's buffers), the two nn.EventTracker calls and nn.TrackMatcher.__call__, each between two HIP events, the median
                over the batches of a series and then over the series
  a year        --year frames (default 2920 = 365 batches: 3-hourly for a year), the 64-frame series repeated, then
                nn.TrackMatcher.resolve() (both dc_track_resolve calls + dc_track_match_resolve), dc_track_match_resolve alone and
                nn.TrackMatcher.rows() (the same plus the synchronising reads, wall clock)
  memory        the device bytes of the link store, the outputs and the workspace at the default capacities

Only standard output belongs in the profile:

    python scripts/track_match_bench.py [--series 5] [--year 2920] 2>/dev/null > profiles/track_match.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from track_bench import B, H, W, moving_blobs  # noqa: E402

FRAMES = 64


def overlap_again(m, mask_a):
    """dc_component_overlap as nn.EventMatcher.__call__ issues it, on the buffers of the matcher's last call (mask_a: its first argument)"""
    a, b = m.a, m.b
    L.call("dc_component_overlap", m.B, m._last_valid, m.H, m.W, L.dptr(mask_a), L.dptr(a._labels), L.dptr(a._ws), a.cap, L.dptr(m._mask_b),
           L.dptr(b._labels), L.dptr(b._ws), b.cap, m.pair_cap, L.dptr(m._pairs), L.dptr(m._npairs), L.dptr(m._cover_a), L.dptr(m._cover_b),
           L.dptr(m._ws), L.stream_ptr())


def match_resolve_again(tm):
    """dc_track_match_resolve as nn.TrackMatcher.resolve() issues it, behind trackers that are resolved already"""
    ta, tb = tm.tracker_a, tm.tracker_b
    L.call("dc_track_match_resolve", ta.event_cap, tb.event_cap, ta.track_cap, tb.track_cap, tm.link_cap, tm.pair_cap, tm.min_frames, tm.cover_q,
           L.dptr(tm._state), L.dptr(tm._links), L.dptr(ta._store), L.dptr(ta._track_of), L.dptr(ta._tracks), L.dptr(ta._ntracks),
           L.dptr(tb._track_of), L.dptr(tb._tracks), L.dptr(tb._ntracks), L.dptr(tm._tpairs), L.dptr(tm._cover_a), L.dptr(tm._cover_b),
           L.dptr(tm._scores), L.dptr(tm._counts), L.dptr(tm._ws), L.stream_ptr())


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--blobs", type=int, default=96)
    ap.add_argument("--extra", type=int, default=24)
    ap.add_argument("--year", type=int, default=2920)
    a = ap.parse_args()
    assert a.year % B == 0
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pred = moving_blobs(np.random.RandomState(7), FRAMES, a.blobs)
    own = moving_blobs(np.random.RandomState(11), FRAMES, a.extra)
    truth = np.roll(pred, (2, 5), axis=(1, 2))
    truth = np.where(truth == 0, own, truth).astype(np.uint8)
    masks_a, masks_b = torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev)
    m = dnn.EventMatcher(B, H, W)
    ta, tb = dnn.EventTracker(m.a), dnn.EventTracker(m.b)
    tm = dnn.TrackMatcher(m, ta, tb)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {FRAMES} frames per series, {a.series} series, HIP events, medians")

    calls = (("nn.EventMatcher (2 catalogues, overlap, scores)", lambda k: m(masks_a[k:k + B], masks_b[k:k + B])),
             ("dc_component_overlap alone", lambda k: overlap_again(m, masks_a[k:k + B])),
             ("nn.EventTracker, prediction", lambda k: ta(masks_a[k:k + B])), ("nn.EventTracker, labels", lambda k: tb(m.mask_b)),
             ("nn.TrackMatcher.__call__ (append)", lambda k: tm()))

    def reset():
        for obj in (tm, ta, tb):
            obj.reset()

    per_call = {name: [] for name, _ in calls}
    for _ in range(a.series + 1):                        # the first series warms up and is dropped
        reset()
        marks = []
        for k in range(0, FRAMES, B):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
            ev[0].record()
            for i, (_, fn) in enumerate(calls):
                fn(k)
                ev[i + 1].record()
            marks.append(ev)
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(calls):
            per_call[name].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in marks))
    rows = tm.rows()
    st = tm.state()
    print(f"moving blobs, {FRAMES} frames: {ta.state()['events']} predicted and {tb.state()['events']} labelled events, {len(rows['tracks_a'])} and "
          f"{len(rows['tracks_b'])} tracks, {st['links']} links, {len(rows['pairs'])} track pairs, scores {rows['scores'].tolist()}")
    for name, _ in calls:
        print(f"    {name:52s} {statistics.median(per_call[name][1:]):8.3f} ms per batch")

    resolve_ms, alone_ms, rows_ms = [], [], []
    for _ in range(3):                                   # the first year warms up and is dropped
        reset()
        for k in range(0, a.year, B):
            j = k % FRAMES
            m(masks_a[j:j + B], masks_b[j:j + B])
            ta(masks_a[j:j + B])
            tb(m.mask_b)
            tm()
        torch.cuda.synchronize()
        resolve_ms.append(timed(tm.resolve))
        alone_ms.append(timed(lambda: match_resolve_again(tm)))
        t0 = time.perf_counter()
        rows = tm.rows()
        rows_ms.append(1e3 * (time.perf_counter() - t0))
    st = tm.state()
    frames_b = rows["tracks_b"][:, 4] - rows["tracks_b"][:, 3] + 1
    print(f"a year, {a.year} frames ({a.year // B} batches): {ta.state()['events']} predicted and {tb.state()['events']} labelled events, "
          f"{len(rows['tracks_a'])} and {len(rows['tracks_b'])} tracks (longest labelled {int(frames_b.max())} frames), {st['links']} links "
          f"({st['links_dropped']} dropped), {len(rows['pairs'])} track pairs, scores {rows['scores'].tolist()}")
    print(f"    {'nn.TrackMatcher.resolve() (2 x dc_track_resolve + match)':52s} {statistics.median(resolve_ms[1:]):8.3f} ms, once per read")
    print(f"    {'dc_track_match_resolve alone':52s} {statistics.median(alone_ms[1:]):8.3f} ms, once per read")
    print(f"    {'nn.TrackMatcher.rows() (wall clock, with reads)':52s} {statistics.median(rows_ms[1:]):8.3f} ms, once per read")
    out = sum(t.nbytes for t in (tm._tpairs, tm._cover_a, tm._cover_b, tm._scores, tm._counts, tm._state))
    print(f"    device memory at link_cap = {tm.link_cap}, pair_cap = {tm.pair_cap}, event_cap = track_cap = {ta.event_cap}: link store "
          f"{tm._links.nbytes / 2 ** 20:.1f} MiB, outputs {out / 2 ** 20:.1f} MiB, workspace {tm._ws.nbytes / 2 ** 20:.1f} MiB; the second "
          f"tracker {sum(t.nbytes for t in (tb._parent, tb._store, tb._track_of, tb._tracks, tb._ws)) / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
