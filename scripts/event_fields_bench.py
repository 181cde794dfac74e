#!/usr/bin/env python3
"""Times the per-event field statistics (dc_component_fields, nn.EventFields) at batch 8, 768 x 1152 x 16 on the blob masks of
scripts/event_match_bench.py, beside the catalogue's two calls in the same process:

  dc_mask_components, dc_component_stats   (the catalogue)
  dc_component_fields                      (the new call: the init of the table and the pixel pass)

The expectation is a byte count: the call reads the label map (4 B per pixel), writes the empty rows (cap * C * 48 B per sample) and loads
field values at foreground pixels only (64 B each), which puts it near dc_component_stats.  Two more calls switch parts of its work off:

  no foreground           an all-zero label map: the init and the label stream alone
  ranks beyond the cap    the blob label map with a rank map that holds `cap` everywhere: the fields are loaded and reduced through
                          registers and LDS, but no slot reaches a global row

Every call is timed with HIP events; a block's figure is the median of its calls, a call's figure the median of its blocks.

--driver N: also writes N synthetic files (768 x 1152 x 16) and a checkpoint of an untrained network into a temporary directory and
runs predict.py --events with and without --event_fields on them, in alternating runs of fresh processes; the figure is the driver's
own seconds per file over its batch loop.  An untrained network's masks are not blobs: the driver figure measures the path (the extra
launches, the 25 MB table per batch of 8 that crosses to the host, the decoding in the writer thread), the kernel figure above the pass.

Only standard output belongs in the profile:

    python scripts/event_fields_bench.py [--blocks 5] [--calls 10] [--driver 16] 2>/dev/null > profiles/event_fields.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, blob_masks, time_block  # noqa: E402

CH = 16


def synthetic_fields(rs, n):
    """float32 [n, H, W, 16] with per-channel offsets and ranges like the dataset's (data.SyntheticHWC)"""
    lo = np.linspace(-50.0, 200.0, CH).astype(np.float32)
    span = np.linspace(1.0, 300.0, CH).astype(np.float32)
    return lo + rs.random_sample((n, H, W, CH)).astype(np.float32) * span, lo, lo + span


def kernels(a):
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(7)
    mask = torch.from_numpy(blob_masks(rs)[0]).to(dev)
    f, lo, hi = synthetic_fields(rs, B)
    fields = torch.from_numpy(f).to(dev)
    bits = dnn.event_field_bits(lo, hi)
    cat = dnn.EventCatalog(B, H, W)
    ef = dnn.EventFields(cat, CH, bits)
    cat(mask)
    ef(fields)
    torch.cuda.synchronize()
    st = L.stream_ptr()
    med = lambda fn: statistics.median(time_block(fn, a.calls) for _ in range(a.blocks))  # noqa: E731
    label = lambda: L.call("dc_mask_components", B, B, H, W, L.dptr(mask), 8, 1, L.dptr(cat._labels), L.dptr(cat._ws), st)  # noqa: E731
    stats = lambda: L.call("dc_component_stats", B, B, H, W, L.dptr(mask), L.dptr(cat._labels), L.dptr(cat._wy), L.dptr(cat._cx),  # noqa: E731
                           L.dptr(cat._sx), cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(cat._ws), st)

    def fields_call(labels, ranks):
        return lambda: L.call("dc_component_fields", B, B, H, W, L.dptr(labels), L.dptr(ranks), cat.cap, L.dptr(fields), CH, CH,
                              L.dptr(ef._bits), L.dptr(cat._wy), L.dptr(ef._ftable), st)

    t = {"dc_mask_components": med(label), "dc_component_stats": med(stats), "dc_component_fields": med(fields_call(cat._labels, cat._ws)),
         "catalogue + nn.EventFields": med(lambda: ef(fields, n_valid=cat(mask)._last_valid))}
    parts = {"no foreground": med(fields_call(torch.zeros_like(cat._labels), cat._ws)),
             "ranks beyond the cap": med(fields_call(cat._labels, torch.full_like(cat._labels, cat.cap)))}
    cat(mask)
    ef(fields)
    fg = float((cat._labels > 0).float().mean())
    rows = ef.rows()
    print(f"blobs (40 ellipses per sample): events per sample {cat.counts()[:, 0].tolist()}, foreground {100 * fg:.1f} % of the pixels; "
          f"table {ef._ftable.numel() * 8 / 2 ** 20:.1f} MiB, field bytes at foreground {fg * B * H * W * CH * 4 / 2 ** 20:.1f} MiB of "
          f"{B * H * W * CH * 4 / 2 ** 20:.0f} MiB")
    assert all(int((r[:, :, 0] == -1).sum()) == 0 for r in rows)             # every event met finite values in every channel
    for k, v in t.items():
        print(f"    {k:28s} {v:8.3f} ms/batch")
    print(f"    dc_component_fields / dc_component_stats = {t['dc_component_fields'] / t['dc_component_stats']:.2f}, "
          f"/ dc_mask_components = {t['dc_component_fields'] / t['dc_mask_components']:.2f}")
    print("  dc_component_fields taken apart (the same call on inputs that switch parts of its work off):")
    for k, v in parts.items():
        print(f"    {k:28s} {v:8.3f} ms/batch")
    full, none, far = t["dc_component_fields"], parts["no foreground"], parts["ranks beyond the cap"]
    print(f"    field loads, registers and LDS table      {far - none:+8.3f} ms   (ranks beyond the cap - no foreground)")
    print(f"    global atomics of the filled slots        {full - far:+8.3f} ms   (full call - ranks beyond the cap)")


def driver(a):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        print("driver: no HDF5 C library here, not measured")
        return
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "files")
        os.makedirs(root)
        rs = np.random.RandomState(11)
        lo = hi = None
        for i in range(a.driver):
            f, lo, hi = synthetic_fields(rs, 1)
            with h5lite.File(os.path.join(root, f"data-{i:03d}.h5"), "w") as out:
                out.write("climate/data", f[0])
        stats = os.path.join(tmp, "stats.h5")
        with h5lite.File(stats, "w") as out:
            out.write("climate/minval", lo)
            out.write("climate/maxval", hi)
        net = dnn.DeepLabv3_plus(CH, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
        net.materialize(1, H, W)
        ckpt = os.path.join(tmp, "model.cpt")
        torch.save({"step": 0, "epoch": 0, "model": net.state_dict()}, ckpt)
        del net
        torch.cuda.empty_cache()
        ms = {"--events": [], "--events --event_fields": []}
        events = None
        for run in range(a.driver_runs):
            for flags in ms:
                out = os.path.join(tmp, f"out-{run}-{len(flags)}")
                cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats,
                       "--output_dir", out, "--batch_size", str(B), "--dtype", "bf16", *flags.split()]
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                ms[flags].append(1000.0 * line["seconds"] / line["samples"])
                events = line["events"]
        print(f"predict.py, {a.driver} files in batches of {B}, bf16, an untrained network (events of class 1, 2 over all files: {events}); "
              f"{a.driver_runs} alternating runs each, ms per file over the batch loop:")
        for flags, v in ms.items():
            print(f"    {flags:26s} median {statistics.median(v):8.2f}   runs {' '.join(f'{x:.2f}' for x in v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--driver", type=int, default=0, help="files for the predict.py comparison (0: leave it out)")
    ap.add_argument("--driver_runs", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W} x {CH}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    kernels(a)
    if a.driver > 0:
        driver(a)


if __name__ == "__main__":
    main()
