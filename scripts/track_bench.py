#!/usr/bin/env python3
"""Times the event tracks at batch 8, 768 x 1152, on moving blobs: 32 ellipses per frame that drift a few pixels from frame to frame (some
across the seam), 16 frames = two batches.  Per library call, in one process:

  dc_mask_components, dc_component_stats   (the catalogue the tracker runs behind)
  dc_track_append                          (the batch's event numbers, store rows and forest entries)
  dc_track_link                            (the 7 frame pairs inside a batch; the one pair to the carried frame)
  the carry copies                         (mask, labels, rank map and first event number of the last frame: four dc_memcpy_async)
  dc_track_resolve                         (once, when tracks are read)
  nn.EventTracker                          (append, both links and the copies: one call per batch)

The yardstick of the link pass is dc_component_overlap on the SAME 7 consecutive-frame pairs, in the same job: it is the pass over two
label maps that existed before, and it does strictly more (the pair table, the coverage counts).  Every call is timed with HIP events; a
block's figure is the median of its calls, a call's figure the median of its blocks.  Before every timed link call the forest is put
back to "every event its own root" (outside the timed interval), so that every call does the unions and not just the finds of a repeat;
"repeat" is the same call on the forest the call before left.

--driver N also times predict.py on N synthetic files (--events against --events --tracks, three alternating runs each, the driver's own
loop time per file).  Only standard output belongs in the profile:

    python scripts/track_bench.py [--blocks 5] [--calls 10] [--driver 24] 2>/dev/null > profiles/tracks.txt"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402

H, W, B = 768, 1152, 8


def time_block(fn, calls: int, before=None) -> float:
    """median milliseconds of `calls` calls, each between two HIP events; `before` runs ahead of every call, outside its interval"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        if before is not None:
            before()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def moving_blobs(rs, frames: int, blobs: int = 32):
    """uint8 [frames, H, W]: ellipses of class 1 or 2 that move by up to 6 pixels per frame and breathe a little; columns are periodic"""
    rr, cc = np.mgrid[0:H, 0:W]
    m = np.zeros((frames, H, W), np.uint8)
    for _ in range(blobs):
        r0, c0, a, bb, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(4, 40), rs.randint(8, 120), rs.randint(1, 3)
        vr, vc = rs.randint(-3, 4), rs.randint(-6, 7)
        born, dies = rs.randint(-4, frames - 2), rs.randint(4, frames + 6)
        for t in range(max(born, 0), min(dies, frames)):
            rt, ct = r0 + vr * t, (c0 + vc * t) % W
            at, bt = max(a + rs.randint(-1, 2), 2), max(bb + rs.randint(-2, 3), 2)
            lo, hi = max(rt - at, 0), min(rt + at + 1, H)
            if lo >= hi:
                continue
            dc = np.minimum(np.abs(cc[lo:hi] - ct), W - np.abs(cc[lo:hi] - ct))
            m[t, lo:hi][((rr[lo:hi] - rt) / at) ** 2 + (dc / bt) ** 2 <= 1.0] = cl
    return m


def driver_runs(n_files: int, masks: np.ndarray):
    """predict.py on n_files synthetic files, --events against --events --tracks, three alternating runs: ms per file of each run"""
    from mlperf_deepcam_amd import h5lite
    tmp = tempfile.mkdtemp(prefix="track_bench_")
    try:
        rs = np.random.RandomState(3)
        data = os.path.join(tmp, "data")
        os.makedirs(data)
        base = (rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32)
        for i in range(n_files):
            d = base.copy()
            d[..., 0] += 40.0 * masks[i % len(masks)]            # the scene changes slowly from file to file
            with h5lite.File(os.path.join(data, f"data-{i:03d}.h5"), "w") as f:
                f.write("climate/data", d)
        stats = os.path.join(tmp, "stats.h5")
        with h5lite.File(stats, "w") as f:
            f.write("climate/minval", (base.min(axis=(0, 1)) - 1.0).astype(np.float32))
            f.write("climate/maxval", (base.max(axis=(0, 1)) + 41.0).astype(np.float32))
        net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
        net.materialize(1, H, W)
        ckpt = os.path.join(tmp, "model.cpt")
        torch.save({"step": 0, "epoch": 0, "model": net.state_dict()}, ckpt)
        del net
        torch.cuda.empty_cache()
        out = {"--events": [], "--events --tracks": []}
        lines = {}
        for _ in range(3):
            for flags in out:
                cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", data, "--stats_file", stats,
                       "--output_dir", os.path.join(tmp, "out"), "--batch_size", str(B), "--dtype", "bf16"] + flags.split()
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                out[flags].append(1e3 * line["seconds"] / line["samples"])
                lines[flags] = line
        summary = json.load(open(os.path.join(tmp, "out", "summary.json")))
        return out, lines, summary.get("tracks")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--driver", type=int, default=0, help="also time predict.py on this many synthetic files")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    masks = moving_blobs(np.random.RandomState(7), 2 * B)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    med = lambda fn, before=None: statistics.median(time_block(fn, a.calls, before) for _ in range(a.blocks))  # noqa: E731
    m0, m1 = torch.from_numpy(masks[:B]).to(dev), torch.from_numpy(masks[B:]).to(dev)
    cat = dnn.EventCatalog(B, H, W)
    trk = dnn.EventTracker(cat)
    for m in (m0, m1):                                   # the state the timed calls run on: batch 0 carried, batch 1 current
        cat(m)
        trk(m)
    torch.cuda.synchronize()
    st, HW, cap, ecap = L.stream_ptr(), H * W, cat.cap, trk.event_cap
    n_events = trk.state()["events"]
    at = lambda t, k: L.C.c_void_p(t.data_ptr() + k * t.element_size())  # noqa: E731
    side = lambda k: (at(m1, k * HW), at(cat._labels, k * HW), at(cat._ws, 4 * k * HW), at(trk._first, k))  # noqa: E731
    carry = (L.dptr(trk._c_mask), L.dptr(trk._c_labels), L.dptr(trk._c_rank), L.dptr(trk._c_first))
    state0, fresh = trk._state.clone(), torch.arange(ecap, dtype=torch.int32, device=dev)

    def unlinked():
        trk._parent.copy_(fresh)

    def rewind():                                        # the counters of before batch 1, so that append writes the same rows every time
        trk._state.copy_(state_before)

    label = lambda: L.call("dc_mask_components", B, B, H, W, L.dptr(m1), 8, 1, L.dptr(cat._labels), L.dptr(cat._ws), st)  # noqa: E731
    stats = lambda: L.call("dc_component_stats", B, B, H, W, L.dptr(m1), L.dptr(cat._labels), L.dptr(cat._wy), L.dptr(cat._cx),  # noqa: E731
                           L.dptr(cat._sx), cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(cat._ws), st)
    append = lambda: L.call("dc_track_append", B, B, cap, L.dptr(cat._table), L.dptr(cat._ncomp), B, ecap, L.dptr(trk._state),  # noqa: E731
                            L.dptr(trk._first), L.dptr(trk._parent), L.dptr(trk._store), st)
    link = lambda n, x, y: L.call("dc_track_link", n, H, W, *x, *y, cap, ecap, 0, L.dptr(trk._store), L.dptr(trk._parent), st)  # noqa: E731
    copies = lambda: [L.call("dc_memcpy_async", L.dptr(d), s, d.numel() * d.element_size(), st)  # noqa: E731
                      for d, s in zip((trk._c_mask, trk._c_labels, trk._c_rank, trk._c_first), side(B - 1))]
    resolve = lambda: trk.resolve()  # noqa: E731
    # the yardstick: the overlap pass of the parent commit on the same 7 frame pairs (frames 0..6 against frames 1..7 of batch 1)
    pair_cap = 8192
    z = lambda *shape, dtype=torch.int64: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    pairs, npairs, ca, cb = z(B, pair_cap, 3), z(B, 2, dtype=torch.int32), z(B, cap), z(B, cap)
    ows = torch.empty(L.load().dc_component_overlap_workspace(B, pair_cap), dtype=torch.uint8, device=dev)
    a3, b3 = side(0)[:3], side(1)[:3]
    overlap = lambda: L.call("dc_component_overlap", B, B - 1, H, W, *a3, cap, *b3, cap, pair_cap, L.dptr(pairs), L.dptr(npairs),  # noqa: E731
                             L.dptr(ca), L.dptr(cb), L.dptr(ows), st)
    # the counters of before batch 1: two frames' worth of bookkeeping undone on the host
    first1 = int(trk._first[0].item())
    state_before = torch.tensor([first1, B, 0, 0], dtype=torch.int64, device=dev)
    t = {"dc_mask_components": med(label), "dc_component_stats": med(stats), "dc_track_append": med(append, rewind),
         "dc_track_link (7 pairs)": med(lambda: link(B - 1, side(0), side(1)), unlinked),
         "dc_track_link (7 pairs, repeat)": med(lambda: link(B - 1, side(0), side(1))),
         "dc_track_link (carry, 1 pair)": med(lambda: link(1, carry, side(0)), unlinked),
         "dc_component_overlap (7 pairs)": med(overlap), "carry copies (4)": med(copies)}
    trk._state.copy_(state0)
    unlinked()
    link(B - 1, side(0), side(1))
    t["dc_track_resolve"] = med(resolve)
    # the whole call per batch, the series restarted before every block
    def series():
        cat(m1)
        trk(m1)
    trk.reset()
    cat(m0)
    trk(m0)
    t["nn.EventCatalog + nn.EventTracker"] = med(series)
    t["nn.EventCatalog"] = med(lambda: cat(m1))
    cat(m1)
    t["nn.EventTracker"] = med(lambda: trk(m1))
    trk.reset()
    for m in (m0, m1):
        cat(m)
        trk(m)
    tracks = trk.tracks()
    counts = trk.track_counts().tolist()
    print(f"moving blobs, {2 * B} frames: {n_events} events ({n_events / (2 * B):.1f} per frame), tracks {counts[:3]} (all, class 1, class 2), "
          f"longest {max(x['frames'] for x in tracks)} frames, {sum(1 for x in tracks if x['events'] > x['frames'])} tracks with merges or splits; "
          f"pairs of the yardstick per frame pair {npairs[:B - 1, 0].tolist()}")
    for k, v in t.items():
        print(f"    {k:36s} {v:8.3f} ms")
    ratio = t["dc_track_link (7 pairs)"] / t["dc_component_overlap (7 pairs)"]
    print(f"    dc_track_link / dc_component_overlap on the same 7 frame pairs = {ratio:.2f}")
    print(f"    tracker per batch over the catalogue per batch = {t['nn.EventTracker'] / t['nn.EventCatalog']:.2f}")
    if a.driver > 0:
        runs, lines, summary = driver_runs(a.driver, masks)
        print(f"predict.py on {a.driver} synthetic files ({H} x {W} x 16 fp32; untrained weights), bf16, batch {B}, the driver's own loop time, "
              f"three alternating runs each:")
        for k, v in runs.items():
            print(f"    {k:18s} " + "  ".join(f"{x:.2f}" for x in v) + f" ms/file   (median {statistics.median(v):.2f})")
        d = statistics.median(runs["--events --tracks"]) - statistics.median(runs["--events"])
        print(f"    --tracks adds {d:+.2f} ms per file ({100 * d / statistics.median(runs['--events']):+.1f} %); events {lines['--events --tracks'].get('events')}, "
              f"tracks {json.dumps(summary)[:400]}")


if __name__ == "__main__":
    main()
