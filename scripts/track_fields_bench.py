#!/usr/bin/env python3
"""Times the storm life cycles (nn.TrackFields: dc_track_fields_append per batch, dc_track_cycles when they are read) at batch 8,
768 x 1152, 16 channels, on the moving blobs of scripts/track_bench.py: --blobs ellipses (default 96) that are born, drift a few pixels
per frame and die inside the series, so that a frame holds between ten and thirty events -- the order of what a CAM5 snapshot holds, a
handful of cyclones and a dozen or two rivers; the first line of the output states the count that was met.  --frames frames (default
64 = 8 batches) are one series.  In one process:

  per batch     nn.EventCatalog, nn.EventTracker, nn.EventFields and nn.TrackFields.__call__, each between two HIP events, the median over
                the batches of a series and then over the series
  at the end    nn.TrackFields.launch() (dc_track_resolve + dc_track_cycles, HIP events) and nn.TrackFields.rows() (the same plus the
                synchronising reads of the counters and of the filled parts, wall clock)
  bytes         what rows() reads back, for every track and for the tracks of at least --min_frames frames (default 8), against what a
                host join needs whatever it selects: the event_fields rows of every file (48 bytes per event and channel) on top of the
                tracker's own tables

Only standard output belongs in the profile:

    python scripts/track_fields_bench.py [--frames 64] [--series 5] [--blobs 96] 2>/dev/null > profiles/track_fields.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from track_bench import B, H, W, moving_blobs  # noqa: E402

CH = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--blobs", type=int, default=96)
    ap.add_argument("--min_frames", type=int, default=8)
    a = ap.parse_args()
    assert a.frames % B == 0 and a.frames >= B
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rs = np.random.RandomState(7)
    masks = torch.from_numpy(moving_blobs(rs, a.frames, a.blobs)).to(dev)
    lo, hi = np.linspace(-50.0, 200.0, CH), np.linspace(-50.0, 200.0, CH) + np.linspace(1.0, 300.0, CH)
    raw = torch.from_numpy((lo + (hi - lo) * rs.rand(B, H, W, CH)).astype(np.float32)).to(dev)       # one batch of fields serves every batch
    cat = dnn.EventCatalog(B, H, W)
    trk = dnn.EventTracker(cat)
    fld = dnn.EventFields(cat, CH, dnn.event_field_bits(lo, hi))
    tf = dnn.TrackFields(trk, fld)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W} x {CH}; {a.frames} frames per series, {a.series} series, HIP events, medians")
    calls = (("nn.EventCatalog", lambda m: cat(m)), ("nn.EventTracker", lambda m: trk(m)), ("nn.EventFields", lambda m: fld(raw)),
             ("nn.TrackFields.__call__", lambda m: tf()))
    per_call = {name: [] for name, _ in calls}
    launch_ms, rows_ms = [], []
    for _ in range(a.series + 1):                        # the first series warms up and is dropped
        trk.reset()
        marks = []
        for k in range(0, a.frames, B):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
            ev[0].record()
            for i, (_, fn) in enumerate(calls):
                fn(masks[k:k + B])
                ev[i + 1].record()
            marks.append(ev)
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(calls):
            per_call[name].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in marks))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tf.launch()
        e1.record()
        torch.cuda.synchronize()
        launch_ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        rows = tf.rows()
        rows_ms.append(1e3 * (time.perf_counter() - t0))
    state = trk.state()
    counts = [int(v) for v in rows["counts"]]
    frames = rows["tracks"][:, 4] - rows["tracks"][:, 3] + 1
    print(f"moving blobs, {a.frames} frames: {state['events']} events ({state['events'] / a.frames:.1f} per frame), {len(rows['tracks'])} tracks, "
          f"longest {int(frames.max())} frames, {counts[2]} step rows of {counts[1]} needed, "
          f"{int((rows['steps'][:, 2] > 1).sum())} steps of more than one event")
    for name, _ in calls:
        print(f"    {name:44s} {statistics.median(per_call[name][1:]):8.3f} ms per batch")
    print(f"    {'nn.TrackFields.launch() (resolve + cycles)':44s} {statistics.median(launch_ms[1:]):8.3f} ms, once per read")
    print(f"    {'nn.TrackFields.rows() (wall clock, with reads)':44s} {statistics.median(rows_ms[1:]):8.3f} ms, once per read")
    back = sum(v.nbytes for v in rows.values())
    join = state["events"] * CH * 48 + state["events"] * (12 * 8 + 4) + rows["tracks"].nbytes
    print(f"    read back by rows(): {back} bytes; a host join reads {join} bytes ({state['events'] * CH * 48} of them event_fields rows): "
          f"{join / back:.2f} x")
    some = tf.rows(min_frames=a.min_frames)
    print(f"    rows(min_frames={a.min_frames}): {int(some['counts'][0])} tracks, {int(some['counts'][2])} step rows, "
          f"{sum(v.nbytes for v in some.values())} bytes: {join / sum(v.nbytes for v in some.values()):.2f} x")
    print(f"    device memory of the tables at event_cap = step_cap = {trk.event_cap}: field store {tf._fstore.nbytes >> 20} MiB, step_fields "
          f"{tf._step_fields.nbytes >> 20} MiB, steps {tf._steps.nbytes >> 20} MiB, track_fields {tf._track_fields.nbytes >> 20} MiB")


if __name__ == "__main__":
    main()
