#!/usr/bin/env python3
"""Times the climatology (dc_climatology_accumulate, dc_climatology_maps; nn.Climatology) at batch 8, 768 x 1152 x 16, one group, on the
blob masks of scripts/event_match_bench.py:

  accumulate, 16 channels          the vector form: 16-byte loads, four lanes per pixel
  the same through a channel table the scalar form on the same data (what a subset of the channels takes)
  accumulate, no channel           the counts alone
  accumulate, no foreground        an all-zero mask: the field stream and the "all" row alone, no class row is touched
  maps, two frequencies            what the driver's pictures read

The expectation is a byte count, printed beside every figure with the time the same bytes take at the rate this project has recorded
for a streaming kernel (5.8 TB/s): a call reads 4 C + 1 bytes per pixel and frame and read-modify-writes the "all" row
(2 * 12 C bytes per pixel), the class rows where the class occurred and the counts there.  Every call is timed with HIP events; a
block's figure is the median of its calls, a call's figure the median of its blocks.  One full-size accumulate (two calls, so that the
second adds to what the first left) is compared with the numpy checker of tests/util_climatology.py: this is where the offsets are large.

--driver N: also writes N synthetic files (768 x 1152 x 16) and a checkpoint of an untrained network into a temporary directory and
runs predict.py with and without --climatology --climatology_channels 0 .. 15 on them, in alternating runs of fresh processes of this
tree; the figure is the driver's own milliseconds per file over its batch loop (the flag's own cost).

Only standard output belongs in the profile:

    python scripts/climatology_bench.py [--blocks 5] [--calls 10] [--driver 16] 2>/dev/null > profiles/climatology.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_fields_bench import CH, synthetic_fields  # noqa: E402
from event_match_bench import B, H, W, blob_masks, time_block  # noqa: E402

RATE = 5.8e12                                       # bytes per second: dc_bn_bwd_frozen, DESIGN section 7


def call_bytes(mask: np.ndarray, C: int) -> int:
    """the bytes one call over `mask` (one run of one group) moves under the kernel's rules"""
    hw = H * W
    touched = int((mask == 1).any(axis=0).sum() + (mask == 2).any(axis=0).sum())      # class rows and count words that are written
    return len(mask) * hw * (4 * C + 1) + 2 * 12 * C * hw + touched * (2 * 12 * C + 2 * 4)


def kernels(a):
    import util_climatology as uc
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(7)
    mask_h = blob_masks(rs)[0]
    f, lo, hi = synthetic_fields(rs, B)
    mask, fields = torch.from_numpy(mask_h).to(dev), torch.from_numpy(f).to(dev)
    empty = torch.zeros_like(mask)
    bits = [int(b) for b in dnn.event_field_bits(lo, hi)]
    clim = dnn.Climatology(B, H, W, channels=range(CH), bits=bits, ldc=CH, device=dev)
    counts = dnn.Climatology(B, H, W, device=dev)
    table = torch.arange(CH, dtype=torch.int32, device=dev)
    group = torch.zeros(B, dtype=torch.int32, device=dev)
    st = L.stream_ptr()

    def raw(m, chan):
        return lambda: L.call("dc_climatology_accumulate", B, H, W, 1, L.dptr(m), 1, L.dptr(fields), CH, CH, L.dptr(chan), L.dptr(clim._bits),
                              L.dptr(group), L.dptr(clim._frames), L.dptr(clim._count), L.dptr(clim._sum), L.dptr(clim._n), st)

    # correctness at full size first: two calls against the checker
    clim(mask, fields)
    clim(mask, fields)
    got = clim.state()
    ref = uc.reference([(mask_h, f, [0] * B)] * 2, 1, H, W, list(range(CH)), bits)
    equal = all(np.array_equal(got[k], ref[k]) for k in uc.KEYS)
    print(f"full size, two calls against the numpy checker: {'equal' if equal else 'DIFFERENT'} (frames {got['frames'].tolist()}, "
          f"sum / n of {got['sum'].nbytes / 2 ** 20:.0f} / {got['n'].nbytes / 2 ** 20:.0f} MiB, largest offset {got['sum'].size - 1})")
    del ref
    med = lambda fn: statistics.median(time_block(fn, a.calls) for _ in range(a.blocks))  # noqa: E731
    fg = float((mask_h == 1).mean() + (mask_h == 2).mean())
    print(f"blobs (40 ellipses per sample): foreground {100 * fg:.1f} % of the pixels and frames; accumulators "
          f"{(clim._sum.numel() * 8 + clim._n.numel() * 4 + clim._count.numel() * 4) / 2 ** 20:.0f} MiB")
    products = [("frequency", 1), ("frequency", 2)]
    rows = [("accumulate, 16 channels", med(raw(mask, None)), call_bytes(mask_h, CH)),
            ("the same through a channel table", med(raw(mask, table)), call_bytes(mask_h, CH)),
            ("accumulate, no channel", med(lambda: counts(mask)), call_bytes(mask_h, 0)),
            ("accumulate, no foreground", med(raw(empty, None)), call_bytes(np.zeros_like(mask_h), CH)),
            ("nn.Climatology.__call__, 16 ch.", med(lambda: clim(mask, fields)), call_bytes(mask_h, CH)),
            ("maps, two frequencies", med(lambda: clim.fields(products)), H * W * (2 * 4 + 2 * 4 + 1))]
    for name, ms, nbytes in rows:
        at_rate = 1000.0 * nbytes / RATE
        print(f"    {name:34s} {ms:8.3f} ms/batch   {nbytes / 1e6:8.1f} MB   {at_rate:6.3f} ms at 5.8 TB/s   x {ms / at_rate:5.2f}   "
              f"{nbytes / ms / 1e9:7.2f} TB/s")


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
            with h5lite.File(os.path.join(root, f"data-2005-{1 + i % 12:02d}-{1 + i // 12:02d}-00-1.h5"), "w") as out:
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
        every = " ".join(str(c) for c in range(CH))
        ms = {"": [], "--climatology": [], f"--climatology --climatology_channels {every}": []}
        for run in range(a.driver_runs):
            for k, flags in enumerate(ms):
                out = os.path.join(tmp, f"out-{run}-{k}")
                cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats,
                       "--output_dir", out, "--batch_size", str(B), "--dtype", "bf16", *flags.split()]
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                ms[flags].append(1000.0 * line["seconds"] / line["samples"])
        print(f"predict.py, {a.driver} files in batches of {B}, bf16, an untrained network; {a.driver_runs} alternating runs each of fresh "
              f"processes of one tree, ms per file over the batch loop (the read-back of the state at the end included):")
        for flags, v in ms.items():
            name = (flags or "(no flag)").replace(every, "0 .. 15")
            print(f"    {name:48s} median {statistics.median(v):8.2f}   runs {' '.join(f'{x:.2f}' for x in v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--driver", type=int, default=0, help="files for the predict.py comparison (0: leave it out)")
    ap.add_argument("--driver_runs", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W} x {CH}, one group; {a.blocks} blocks of {a.calls} calls per figure, HIP events, "
          f"medians")
    kernels(a)
    if a.driver > 0:
        driver(a)


if __name__ == "__main__":
    main()
