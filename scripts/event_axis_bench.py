#!/usr/bin/env python3
"""Times the event skeletons at batch 8, 768 x 1152, in one process, beside the Predictor's forward pass (bf16):

  dc_mask_thin         (nn.EventAxis: one workgroup per class and frame thins the bit plane in LDS, to convergence)
  dc_skeleton_stats    (the rows: pixels, endpoints, junctions, links, length)
  dc_component_shape   (the yardstick: the parent commit has it, and it reads the same label map)
  torch thinning       (the same rule with torch.roll and Boolean operators on the same GPU, both classes, the passes dc_mask_thin ran)
  dc_skeleton_prune    (nn.EventAxis(prune=N): spurs of at most N = 8, 16, 32 pixels removed from the thinned map, one workgroup per class
                        and frame; dc_mask_thin above, unchanged code, is its yardstick), the pixels it removes, and what it does to the
                        events' mean axis_km and their branches
  dc_event_select_axis (the filter's axis criterion on the catalogue's rows)
  dc_skeleton_course   (nn.EventAxis(course=True): the main course of every event on the thinned map, one workgroup per class and frame;
                        dc_mask_thin is its yardstick too), the nodes per frame, the relaxation rounds per sweep, the class planes over the
                        node cap, and the events' mean course_km beside their mean axis_km

on the masks of scripts/events_bench.py: 8 blobs per sample (about 97 % background), 40 blobs per sample and 45 % uniform-random
foreground; the background share of each is printed.  Every call
is timed with HIP events, a block's figure is the median of its calls, a call's figure the median of its blocks.  There is no time to
meet.  Thinning is serial in its passes and 16 workgroups run at batch 8: where it takes longer than the forward pass the script says so.

    python scripts/event_axis_bench.py [--blocks 5] [--calls 10] > profiles/event_axis.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from events_bench import B, H, W, blob_mask, time_block  # noqa: E402
from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402


def torch_thin(f: torch.Tensor, passes: int) -> torch.Tensor:
    """Guo and Hall's rule on a bool tensor [N, H, W], columns periodic, rows not, `passes` passes without a convergence test"""
    def nb(x, dr, dc):
        y = torch.roll(x, shifts=(-dr, -dc), dims=(1, 2))
        if dr:
            y[:, -1 if dr > 0 else 0] = False
        return y
    for _ in range(passes):
        for sub in (0, 1):
            p2, p3, p4, p5 = nb(f, -1, 0), nb(f, -1, 1), nb(f, 0, 1), nb(f, 1, 1)
            p6, p7, p8, p9 = nb(f, 1, 0), nb(f, 1, -1), nb(f, 0, -1), nb(f, -1, -1)
            i = lambda x: x.to(torch.int8)  # noqa: E731
            C = i(~p2 & (p3 | p4)) + i(~p4 & (p5 | p6)) + i(~p6 & (p7 | p8)) + i(~p8 & (p9 | p2))
            N = torch.minimum(i(p9 | p2) + i(p3 | p4) + i(p5 | p6) + i(p7 | p8), i(p2 | p3) + i(p4 | p5) + i(p6 | p7) + i(p8 | p9))
            m = ((p6 | p7 | ~p9) & p8) if sub == 0 else ((p2 | p3 | ~p5) & p4)
            f = f & ~((C == 1) & (N >= 2) & (N <= 3) & ~m)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    med = lambda fn, calls=a.calls: statistics.median(time_block(fn, calls) for _ in range(a.blocks))  # noqa: E731
    x = torch.rand(B, 16, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    plain = dnn.Predictor(net, B, H, W)
    plain(x)
    plain(x)
    torch.cuda.synchronize()
    fwd = med(lambda: plain(x))
    plain.close()
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls, HIP events, medians")
    print(f"nn.Predictor (bf16 forward pass and mask): {fwd:8.3f} ms/batch")
    print(f"LDS per workgroup: {L.load().dc_thin_lds_bytes(H, W)} bytes; {2 * B} workgroups")
    rs = np.random.RandomState(7)
    cases = {"blobs (8 ellipses per sample)": blob_mask(rs, 8), "blobs (40 ellipses per sample)": blob_mask(rs),
             "random 45 % foreground": ((rs.rand(B, H, W) < 0.45) * rs.randint(1, 3, (B, H, W))).astype(np.uint8)}
    for name, mask in cases.items():
        cat = dnn.EventCatalog(B, H, W)
        shape, axis = dnn.EventShape(cat), dnn.EventAxis(cat)
        m = torch.from_numpy(mask).to(dev)
        cat(m)
        shape()
        axis(m)
        torch.cuda.synchronize()
        iters = axis.iterations()
        ref = axis.skeleton_buffer.clone()
        st = L.stream_ptr()
        thin = lambda: L.call("dc_mask_thin", B, B, H, W, L.dptr(m), 1, int(cat.wrap), axis.max_iters, L.dptr(axis._skel),  # noqa: E731
                              L.dptr(axis._iters), st)
        stats = lambda: L.call("dc_skeleton_stats", B, B, H, W, L.dptr(axis._skel), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap,  # noqa: E731
                               int(cat.wrap), L.dptr(axis._link), L.dptr(axis._rows), st)
        passes = int(iters[:, :, 0].max())
        planes = torch.cat([m == 1, m == 2])
        same = bool(torch.equal(torch_thin(planes, passes), torch.cat([ref == 1, ref == 2])))
        t = {"dc_mask_thin": med(thin), "dc_skeleton_stats": med(stats), "dc_component_shape": med(lambda: shape()),
             "torch thinning": med(lambda: torch_thin(planes, passes), max(a.calls // 5, 1))}
        print(f"{name}: {100 * float((mask == 0).mean()):.1f} % background; events per sample {cat.counts()[:, 0].cpu().tolist()}")
        print(f"    passes per frame and class {iters[:, :, 0].tolist()}; frames stopped at max_iters {int((iters[:, :, 1] == 0).sum())}; "
              f"torch thinning gives the same skeleton: {same}")
        for k, v in t.items():
            print(f"    {k:20s} {v:8.3f} ms/batch = {100 * v / fwd:6.2f} % of the forward pass")
        print(f"    dc_mask_thin per pass {1000 * t['dc_mask_thin'] / passes:.1f} us; torch thinning / dc_mask_thin = "
              f"{t['torch thinning'] / t['dc_mask_thin']:.1f}")
        if t["dc_mask_thin"] > fwd:
            print("    dc_mask_thin takes LONGER than the batch's forward pass: the passes are serial and only 16 of the CUs work")
        # spur pruning of the thinned map `ref`, and the statistics of the pruned map
        pruned, removed = torch.empty_like(ref), torch.zeros((B, 2), dtype=torch.int32, device=dev)
        keep = torch.ones((B, cat.cap), dtype=torch.uint8, device=dev)
        counts = torch.zeros((B, 2, 4), dtype=torch.int64, device=dev)
        stats_pruned = lambda: L.call("dc_skeleton_stats", B, B, H, W, L.dptr(pruned), L.dptr(cat._labels), L.dptr(cat._ws),  # noqa: E731
                                      cat.cap, int(cat.wrap), L.dptr(axis._link), L.dptr(axis._rows), st)
        stats()
        torch.cuda.synchronize()
        before = [dnn.EventAxis.values(r) for r in axis.rows()]
        for spur in (8, 16, 32):
            prune = lambda: L.call("dc_skeleton_prune", B, B, H, W, L.dptr(ref), int(cat.wrap), spur, L.dptr(pruned), L.dptr(removed), st)  # noqa: E731
            tp = med(prune)
            stats_pruned()
            torch.cuda.synchronize()
            after = [dnn.EventAxis.values(r) for r in axis.rows()]
            km = [float(np.concatenate([v[:, 4] for v in side]).mean()) for side in (before, after)]
            br = [int(np.concatenate([v[:, 3] for v in side]).sum()) for side in (before, after)]
            print(f"    dc_skeleton_prune spur {spur:2d} {tp:8.3f} ms/batch = {100 * tp / t['dc_mask_thin']:6.1f} % of dc_mask_thin, "
                  f"{1000 * tp / (2 * spur):.1f} us per round if all {2 * spur} rounds ran; removed {int(removed.sum())} of "
                  f"{int((ref != 0).sum())} skeleton pixels; mean axis_km {km[0]:.1f} -> {km[1]:.1f}, branches {br[0]} -> {br[1]}")
        sel = lambda: L.call("dc_event_select_axis", B, B, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(axis._rows), 0,  # noqa: E731
                             2000000, L.dptr(keep), L.dptr(counts), st)
        print(f"    dc_skeleton_stats (pruned map, spur 32) {med(stats_pruned):8.3f} ms/batch; dc_event_select_axis {med(sel):8.3f} ms/batch")
        # the main course on the thinned map `ref`
        co = dnn.EventAxis(cat, course=True)
        course = lambda: L.call("dc_skeleton_course", B, B, H, W, L.dptr(ref), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap,  # noqa: E731
                                int(cat.wrap), L.dptr(co._link), L.dptr(co._course_rows), L.dptr(co._course), L.dptr(co._course_status),
                                L.dptr(co._node_ws), st)
        tc = med(course)
        torch.cuda.synchronize()
        status = co._course_status.cpu().numpy()
        swept = status[:, :, 2] == 0
        rows = np.concatenate([r for r in dnn._filled_rows(co._course_rows, cat._fill(B))])
        has = rows[:, 6] > 0
        km, axis_km = rows[has, 6] / 1000.0, np.concatenate([v[:, 4] for v in before])[has]
        print(f"    dc_skeleton_course {tc:8.3f} ms/batch = {100 * tc / t['dc_mask_thin']:6.1f} % of dc_mask_thin; nodes per frame (both "
              f"classes) {status[:, :, 0].sum(axis=1).tolist()}; class planes over the node cap {int((~swept).sum())} of {2 * B}; rounds "
              f"per sweep, mean over the swept planes {float(status[:, :, 1][swept].mean()) / 3 if swept.any() else 0:.0f}, largest "
              f"{int(status[:, :, 1][swept].max()) // 3 if swept.any() else 0}; events with a course {len(km)}, mean course_km "
              f"{float(km.mean()) if len(km) else 0:.1f} of their mean axis_km {float(axis_km.mean()) if len(km) else 0:.1f}")


if __name__ == "__main__":
    main()
