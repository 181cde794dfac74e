#!/usr/bin/env python3
"""Times the train-time augmentation (dc_augment_view_hwc; data.Augment, data.InputPipeline(augment=...), train.py --augment_*) at
768 x 1152 x 16, and what it costs a training step.

  1. the staging pass, batch 8 and 64 (a step of --virtual_ranks 8 stages 64 samples), bf16 and fp32 output, alternating in this process:
       dc_augment_view_hwc      every sample in a view of its own (rolls over the whole width, every other sample mirrored with two
                                channels negated), the int64 label map moved with it: one launch
       normalise + label copy   dc_input_normalize_hwc and a device-side copy of the label map: what the pass replaces, byte for byte
       B calls of dc_input_view_hwc   the same views from the kernel the tree had, one launch per sample (and no labels)
     Every call is timed with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks.
  2. the step, local batch 8, bf16, LAMB: nn.TrainStep fed by data.InputPipeline from a source that copies a sample from memory (what a
     page-cached file read costs the host, scripts/pipeline_rate.py), with and without Augment(roll, flip_lat, negate): fresh processes
     of this script, alternating, milliseconds per step over the steps behind the fourth.
  3. the driver itself: python -m mlperf_deepcam_amd.train on --synthetic_samples at local batch 8, with and without --augment_roll
     --augment_flip_lat, fresh processes, alternating; milliseconds per step between the first and the last train_loss event.  The
     synthetic source draws 14 million random numbers per sample on the host, so this loop measures the host, with and without the flags.

Only standard output belongs in the profile:

    python scripts/augment_bench.py [--blocks 5] [--calls 20] [--runs 3] 2>/dev/null > profiles/augment.txt"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import data as ddata  # noqa: E402
from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import H, W, time_block  # noqa: E402

CFILE = 16
NEGATE = (2, 4)
STEP_BATCH, STEP_BATCHES, STEP_SKIP = 8, 28, 4


# ---------------------------------------------------------------------------------------------------------------- 1. the staging pass
def staging(blocks: int, calls: int) -> None:
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    shift = (torch.rand(CFILE, generator=g) * 50 - 40).to(dev)
    scale = (1.0 / (torch.rand(CFILE, generator=g) * 300 + 1)).to(dev)
    sign = torch.tensor([-1.0 if c in NEGATE else 1.0 for c in range(CFILE)], dtype=torch.float32, device=dev)
    stream = L.stream_ptr()
    for B in (8, 64):
        raw = torch.empty((B, H, W, CFILE), dtype=torch.float32, device=dev)
        for n in range(B):                            # (one sample at a time: the host side of a 3.6 GB batch stays small)
            raw[n] = (torch.rand(H, W, CFILE, generator=g) * torch.linspace(1, 300, CFILE) - 40.0).to(dev)
        lab = torch.randint(0, 3, (B, H, W), generator=g, dtype=torch.int64).to(dev)
        lab_out = torch.empty_like(lab)
        views = np.asarray([(((n * W) // B + 3 * n) % W, n % 2) for n in range(B)], np.int32)
        px = B * H * W
        for dtype, name, ob in ((torch.bfloat16, "bf16", 2), (torch.float32, "fp32", 4)):
            out = torch.empty((B, H, W, CFILE), dtype=dtype, device=dev)
            dt = L.dtype_code(dtype)

            def augment():
                L.call("dc_augment_view_hwc", dt, B, H, W, CFILE, CFILE, None, L.dptr(sign), L.dptr(raw), L.dptr(shift), L.dptr(scale),
                       C.c_void_p(views.ctypes.data), L.dptr(lab), L.dptr(lab_out), L.dptr(out), CFILE, stream)

            def plain():
                L.call("dc_input_normalize_hwc", dt, px, CFILE, CFILE, None, L.dptr(raw), L.dptr(shift), L.dptr(scale), L.dptr(out), CFILE, stream)
                L.call("dc_memcpy_async", L.dptr(lab_out), L.dptr(lab), lab.numel() * 8, stream)

            def per_sample():
                for n in range(B):
                    dnn.view_input(raw[n:n + 1], None, shift, scale, int(views[n, 0]), bool(views[n, 1]), sign if views[n, 1] else None, out[n:n + 1])

            routes = {"dc_augment_view_hwc (data + labels, one launch)": (augment, px * (64 + CFILE * ob + 16)),
                      "dc_input_normalize_hwc + label copy": (plain, px * (64 + CFILE * ob + 16)),
                      f"{B} calls of dc_input_view_hwc (no labels)": (per_sample, px * (64 + CFILE * ob))}
            # the augmented batch against the per-sample calls, once, for the record
            augment()
            got = out.clone()
            per_sample()
            same = bool(torch.equal(got, out))
            for fn, _ in routes.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in routes}
            for _ in range(blocks):                   # alternating blocks
                for k, (fn, _) in routes.items():
                    times[k].append(time_block(fn, calls))
            print(f"batch {B}, {name} out (equal to the per-sample views: {same})")
            for k, v in times.items():
                med, nbytes = statistics.median(v), routes[k][1]
                print(f"    {k:52s} {med:9.3f} ms/batch  {nbytes / 1e6:9.1f} MB  {nbytes / med / 1e9:5.2f} TB/s   blocks {' '.join(f'{t:.3f}' for t in v)}")
            del out
        del raw, lab, lab_out


# ---------------------------------------------------------------------------------------------------------------- 2. the step
class MemcpySource(ddata.SyntheticHWC):
    """a sample is a copy from memory: what a page-cached file read costs the host"""

    def __init__(self, n):
        super().__init__(n, H, W)
        rs = np.random.RandomState(0)
        self._d = rs.random_sample((H, W, CFILE)).astype(np.float32) * 100.0
        self._l = rs.randint(0, 3, size=(H, W)).astype(np.int64)

    def read_into(self, i, data_out, label_out):
        np.copyto(data_out, self._d)
        np.copyto(label_out, self._l)
        return self.files[i]


def step_worker(kind: str) -> None:
    """one fresh process: milliseconds per step of nn.TrainStep behind data.InputPipeline, on standard output"""
    torch.manual_seed(333)
    dev = torch.device("cuda", 0)
    net = dnn.DeepLabv3_plus(n_input=CFILE, n_classes=3, os=16, pretrained=False, rank=0, dtype=torch.bfloat16, _print=False)
    net.to(dev)
    net.materialize(STEP_BATCH, H, W)
    opt = dnn.make_optimizer("LAMB", net, 1e-3, 1e-6, 1e-2)
    step = dnn.TrainStep(net, opt, dnn.class_weights(-0.125), STEP_BATCH, H, W, with_metrics=False)
    net.train()
    augment = ddata.Augment(roll=True, flip_lat=True, negate=NEGATE, seed=0) if kind == "augment" else None
    pipe = ddata.InputPipeline(MemcpySource(STEP_BATCHES * STEP_BATCH), STEP_BATCH, dtype=torch.bfloat16, device=dev, workers=8, augment=augment)
    t0 = None
    for i, (x, y, _) in enumerate(pipe):
        if i == STEP_SKIP:
            torch.cuda.synchronize()
            t0 = time.time()
        step(x, y)
    torch.cuda.synchronize()
    print(f"STEP_MS {(time.time() - t0) / (STEP_BATCHES - STEP_SKIP) * 1e3:.3f}")


def run_worker(kind: str) -> float:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step_worker", kind], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"step worker ({kind}) failed: {r.stderr[-2000:]}")
    return float([line for line in r.stdout.splitlines() if line.startswith("STEP_MS ")][-1].split()[1])


# ---------------------------------------------------------------------------------------------------------------- 3. the driver
def run_driver(flags, samples: int) -> float:
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.train", "--wireup_method", "single", "--run_tag", "bench", "--output_dir", out,
               "--synthetic_samples", str(samples), "--local_batch_size", str(STEP_BATCH), "--max_epochs", "1", "--dtype", "bf16",
               "--optimizer", "LAMB", "--logging_frequency", "2", "--validation_frequency", "1000000", "--save_frequency", "0"] + list(flags)
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"driver {flags} failed: {r.stdout[-1000:]} {r.stderr[-2000:]}")
    ev = [json.loads(line[len(":::MLLOG "):]) for line in r.stdout.splitlines() if line.startswith(":::MLLOG ")]
    loss = [(e["metadata"]["step_num"], e["time_ms"]) for e in ev if e["key"] == "train_loss"]
    (s0, t0), (s1, t1) = loss[1], loss[-1]            # behind the first logged steps: code objects, allocator, the pipeline's start
    return (t1 - t0) / (s1 - s0)


def spread_line(name, plain, aug):
    lo, hi = min(plain), max(plain)
    m = statistics.median(aug)
    inside = "inside" if lo <= m <= hi else ("below" if m < lo else "ABOVE")
    print(f"    {name}: without {' '.join(f'{v:.2f}' for v in plain)} (median {statistics.median(plain):.2f}, spread {lo:.2f} .. {hi:.2f}) ms/step; "
          f"with {' '.join(f'{v:.2f}' for v in aug)} (median {m:.2f}) ms/step: the median with the flags lies {inside} the spread without")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per side of the step and driver comparisons (0: leave them out)")
    ap.add_argument("--driver_samples", type=int, default=96, help="synthetic samples of a driver run (a step takes 8)")
    ap.add_argument("--step_worker", choices=["plain", "augment"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py needs an MI355X: there is nothing to time without one")
    torch.cuda.set_device(0)
    if a.step_worker:
        return step_worker(a.step_worker)
    print(f"{torch.cuda.get_device_name(0)}; {H} x {W} x {CFILE}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    staging(a.blocks, a.calls)
    torch.cuda.empty_cache()
    if a.runs > 0:
        print(f"the step at local batch {STEP_BATCH} (bf16, LAMB), {a.runs} fresh processes per side, alternating:")
        plain, aug = [], []
        for _ in range(a.runs):
            plain.append(run_worker("plain"))
            aug.append(run_worker("augment"))
        spread_line(f"nn.TrainStep behind data.InputPipeline, samples copied from memory, steps {STEP_SKIP + 1} .. {STEP_BATCHES}", plain, aug)
        plain, aug = [], []
        for _ in range(a.runs):
            plain.append(run_driver([], a.driver_samples))
            aug.append(run_driver(["--augment_roll", "--augment_flip_lat"], a.driver_samples))
        spread_line(f"train.py --synthetic_samples {a.driver_samples} (the host draws every sample: this loop measures the host)", plain, aug)


if __name__ == "__main__":
    main()
