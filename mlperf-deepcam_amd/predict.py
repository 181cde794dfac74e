"""Inference driver: a checkpoint and a directory of unlabelled CAM5 files in, one mask file per input file out.

    python -m mlperf_deepcam_amd.predict --checkpoint model_step_1000.cpt --data_dir /data/unlabelled --stats_file /data/stats.h5 \
        --output_dir /data/masks --batch_size 8 --dtype bf16 --confidence

What the reference offers for this is its validation loop's ``net.eval(); torch.max(net(x), 1)[1]`` (train_hdf5_ddp.py:452-458), which
needs labelled files.  Here the files need no ``climate/labels_0`` (data.CamDataset(labels=False)); the batches run through nn.Predictor
(forward-only engine, the class map written by the classifier's kernel as one byte per pixel); the masks leave the device through two
pinned host buffers, and a writer thread stores them while the device works on the next batch.  Every output file carries the base name
of its input file and holds ``prediction`` (uint8 [H, W]: 0 background, 1 tropical cyclone, 2 atmospheric river) and, with --confidence,
``confidence`` (float32 [H, W]: the predicted class's softmax probability).  ``summary.json`` lists the class pixel counts and the mean
confidence per file.  With --events every output file also carries ``events`` (int64 [n, 10], the raw rows of nn.EventCatalog: root,
class, pixels, area, sum of rows, sum of cx, sum of sx, first row, last row, seam flag -- connected components of the mask, found on the
device; the table, not a label map, is what crosses to the host), and ``summary.json`` the number of class-1 and class-2 events per file
and in total and the number of files whose table overflowed.  Single process, single device."""
from __future__ import annotations

import argparse
import json
import os
import queue
import threading
import time

import numpy as np
import torch

from . import data as ddata
from . import nn as dnn


def build_parser():
    AP = argparse.ArgumentParser(description="DeepCAM inference: masks for unlabelled CAM5 files")
    AP.add_argument("--checkpoint", type=str, required=True, help="a checkpoint written by train.py or by the reference (its 'model' entry), "
                    "or a bare state dict")
    AP.add_argument("--data_dir", type=str, required=True, help="directory with the input .h5 files (climate/data, no labels needed)")
    AP.add_argument("--stats_file", type=str, required=True, help="the stats.h5 of the dataset (climate/minval, climate/maxval)")
    AP.add_argument("--output_dir", type=str, required=True, help="where the mask files and summary.json go")
    AP.add_argument("--batch_size", type=int, default=8, help="samples per forward pass")
    AP.add_argument("--channels", type=int, nargs="+", default=list(range(16)), help="Channels used in input")
    AP.add_argument("--amp_opt_level", type=str, default="O1", help="O0 = fp32 activations, O1/O2 = bf16 activations")
    AP.add_argument("--dtype", type=str, default=None, choices=["fp32", "bf16"], help="overrides --amp_opt_level")
    AP.add_argument("--confidence", action="store_true", help="also store the predicted class's softmax probability")
    AP.add_argument("--events", action="store_true", help="also catalogue the connected components of every mask (dataset 'events')")
    AP.add_argument("--min_event_pixels", type=int, default=0, help="with --events: leave out components of fewer pixels")
    AP.add_argument("--event_connectivity", type=int, default=8, choices=[4, 8], help="with --events: pixel connectivity")
    AP.add_argument("--height", type=int, default=768)
    AP.add_argument("--width", type=int, default=1152)
    AP.add_argument("--max_inter_threads", type=int, default=4, help="Maximum number of concurrent readers")
    return AP


def write_mask_file(path: str, prediction: np.ndarray, confidence, events=None) -> None:
    """`prediction` (and `confidence`, `events`) as datasets of one HDF5 file, through the backend data.CamDataset reads with."""
    backend, h5 = ddata._h5_backend()
    if backend == "h5py":
        with h5.File(path, "w") as f:
            f.create_dataset("prediction", data=prediction)
            if confidence is not None:
                f.create_dataset("confidence", data=confidence)
            if events is not None:
                f.create_dataset("events", data=events)
        return
    with h5.File(path, "w") as f:
        f.write("prediction", prediction)
        if confidence is not None:
            f.write("confidence", confidence)
        if events is not None:
            f.write("events", events)


class _HostSlot:
    def __init__(self, B: int, H: int, W: int, confidence: bool, event_cap: int = 0):
        # --events: the whole table of a batch (cap rows of 80 bytes per sample) and the counts that say how many rows are filled
        self.events = torch.empty((B, event_cap, len(dnn.EVENT_FIELDS)), dtype=torch.int64).pin_memory() if event_cap else None
        self.ncomp = torch.empty((B, 3), dtype=torch.int32).pin_memory() if event_cap else None
        self.mask = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
        self.conf = torch.empty((B, H, W), dtype=torch.float32).pin_memory() if confidence else None
        self.counts = torch.empty((B, 3), dtype=torch.int64).pin_memory()
        self.done = torch.cuda.Event()


def _writer(work_q: "queue.Queue", free_q: "queue.Queue", out_dir: str, records: list, errors: list, min_event_pixels: int = 0) -> None:
    while True:
        item = work_q.get()
        if item is None:
            return
        slot, names = item
        try:
            if not errors:
                slot.done.synchronize()                      # host wait of THIS thread: the copies of the batch have landed
                for j, name in enumerate(names):
                    conf = slot.conf[j].numpy() if slot.conf is not None else None
                    base = os.path.basename(name)
                    rows = None
                    if slot.events is not None:
                        total = int(slot.ncomp[j, 0])
                        rows = slot.events[j, :min(total, slot.events.shape[1])].numpy()
                        rows = np.ascontiguousarray(rows[rows[:, 2] >= min_event_pixels])
                    write_mask_file(os.path.join(out_dir, base), slot.mask[j].numpy(), conf, rows)
                    rec = {"file": base, "class_counts": [int(v) for v in slot.counts[j].tolist()],
                           "mean_confidence": float(conf.mean(dtype=np.float64)) if conf is not None else None}
                    if rows is not None:
                        rec["events"] = [int((rows[:, 1] == 1).sum()), int((rows[:, 1] == 2).sum())]
                        rec["events_overflowed"] = total > slot.events.shape[1]
                    records.append(rec)
        except BaseException as e:      # surfaces in the main thread; the slots keep circulating so that it cannot block
            errors.append(e)
        finally:
            free_q.put(slot)


def main(pargs) -> dict:
    if not torch.cuda.is_available():
        raise RuntimeError("mlperf_deepcam_amd.predict needs an MI355X: there is no CPU path")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = pargs.batch_size, pargs.height, pargs.width
    if B < 1:
        raise ValueError("--batch_size must be at least 1")
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[pargs.dtype] if pargs.dtype else \
        (torch.float32 if pargs.amp_opt_level == "O0" else torch.bfloat16)
    os.makedirs(pargs.output_dir, exist_ok=True)

    dataset = ddata.CamDataset(pargs.data_dir, pargs.stats_file, pargs.channels, allow_uneven_distribution=True, shuffle=False,
                               preprocess=True, labels=False)
    assert tuple(dataset.data_shape[:2]) == (H, W), "pass --height/--width matching the files"

    net = dnn.DeepLabv3_plus(n_input=len(pargs.channels), n_classes=3, os=16, pretrained=False, rank=0, dtype=dtype, _print=False)
    net.materialize(1, H, W)                      # the arena's owner; the batches run on the Predictor's forward-only engine
    checkpoint = torch.load(pargs.checkpoint, map_location=device, weights_only=False)
    net.load_state_dict(checkpoint["model"] if "model" in checkpoint else checkpoint)
    net.eval()
    layout = "nhwc" if net.engine.x0 is not None else "nchw"
    loader = ddata.InputPipeline(dataset, B, dtype=dtype, device=device, layout=layout, drop_last=False, workers=pargs.max_inter_threads)
    predictor = dnn.Predictor(net, B, H, W, confidence=pargs.confidence, events=pargs.events, event_connectivity=pargs.event_connectivity)
    event_cap = predictor.catalog.cap if pargs.events else 0

    free_q: "queue.Queue" = queue.Queue()
    work_q: "queue.Queue" = queue.Queue()
    for _ in range(2):
        free_q.put(_HostSlot(B, H, W, pargs.confidence, event_cap))
    records: list = []
    errors: list = []
    writer = threading.Thread(target=_writer, args=(work_q, free_q, pargs.output_dir, records, errors, pargs.min_event_pixels),
                              daemon=True)
    writer.start()
    t0 = time.perf_counter()
    try:
        for x, _, names in loader:
            nv = len(names)
            slot = free_q.get()                    # blocks only while the writer still holds BOTH host buffers
            if errors:
                free_q.put(slot)
                break
            mask = predictor(x, n_valid=nv)
            slot.mask[:nv].copy_(mask, non_blocking=True)
            if slot.conf is not None:
                slot.conf[:nv].copy_(predictor.confidence, non_blocking=True)
            slot.counts[:nv].copy_(predictor.class_counts, non_blocking=True)
            if slot.events is not None:
                slot.events[:nv].copy_(predictor.catalog.table, non_blocking=True)
                slot.ncomp[:nv].copy_(predictor.catalog.counts(), non_blocking=True)
            slot.done.record(torch.cuda.current_stream())
            work_q.put((slot, names))
    finally:
        work_q.put(None)
        writer.join()
        predictor.close()
    if errors:
        raise errors[0]
    elapsed = time.perf_counter() - t0

    records.sort(key=lambda r: r["file"])
    totals = [sum(r["class_counts"][j] for r in records) for j in range(3)]
    summary = {"files": records, "class_counts": totals}
    if pargs.events:
        summary["events"] = [sum(r["events"][j] for r in records) for j in range(2)]
        summary["events_overflowed_files"] = sum(1 for r in records if r["events_overflowed"])
    with open(os.path.join(pargs.output_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    line = {"samples": len(records), "class_counts": totals, "seconds": round(elapsed, 4),
            "samples_per_second": round(len(records) / elapsed, 3) if elapsed > 0 else None}
    if pargs.events:
        line["events"] = summary["events"]
    if pargs.confidence and records:
        line["mean_confidence"] = float(np.mean([r["mean_confidence"] for r in records]))
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    main(build_parser().parse_args())
