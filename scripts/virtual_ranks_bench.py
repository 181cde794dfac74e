#!/usr/bin/env python3
"""Cost of virtual ranks at the benched shape (B = 8, bf16, LAMB, 768 x 1152) on one MI355X.

Interleaves, one fresh process per measurement and `--rounds` times over, (p) the plain TrainStep of ANOTHER checkout (--parent DIR: the
parent commit, built), (1) this tree's TrainStep(virtual_ranks=1) and (K) this tree's TrainStep(virtual_ranks=K), and prints per
process the time per micro-batch (total time of `--steps` steps behind `--warmup`, between two events, divided by steps * K) and the peak
device memory, then the medians and their ratios.  It also times dc_grad_accumulate alone over the whole gradient arena and over the last
bucket of the plan (the only add that nothing in backward hides: an upper bound of the exposed part).

    python scripts/virtual_ranks_bench.py --parent ../parent_checkout [--K 4] [--rounds 3] > profiles/virtual_ranks.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, B = 768, 1152, 8


def child(root: str, K: int, steps: int, warmup: int, kernel: bool) -> None:
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch
    from mlperf_deepcam_amd import lib as L
    from mlperf_deepcam_amd import nn as dnn
    from util_inputs import make_inputs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(B, H, W)
    net.train()
    opt = dnn.make_optimizer("LAMB", net, 1e-3, 1e-8, 1e-2)
    kw = {"virtual_ranks": K} if K > 1 or kernel else {}          # (the parent's TrainStep has no such argument)
    step = dnn.TrainStep(net, opt, dnn.class_weights(), B, H, W, with_metrics=True, **kw)
    x1, y1 = make_inputs(B, H, W)
    x, y = x1.repeat(K, 1, 1, 1).to(dev), y1.repeat(K, 1, 1).to(dev)
    for _ in range(warmup):
        step(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step(x, y)
    e1.record()
    torch.cuda.synchronize()
    out = {"K": K, "ms_per_micro_batch": e0.elapsed_time(e1) / (steps * K), "peak_mb": torch.cuda.max_memory_allocated() / 2 ** 20,
           "loss": step.loss()}
    if kernel:
        # dc_grad_accumulate alone: the whole arena, and the bucket that completes last (nothing of backward is left to hide it)
        from mlperf_deepcam_amd.dist import GradReducer
        eng = net.engine
        acc = torch.empty_like(eng.grads)
        last = GradReducer(eng, 1).buckets[-1]
        eng.on_grad_ready = None
        for name, lo, hi in (("arena", 0, eng.grads.numel()), ("last_bucket", last.lo, last.hi)):
            ts = []
            for first in (1, 0, 0, 0, 0, 0):
                e0.record()
                L.call("dc_grad_accumulate", hi - lo, L.dptr(eng.grads[lo:hi]), L.dptr(acc[lo:hi]), first, L.stream_ptr())
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            out[name] = {"elements": hi - lo, "ms_first": ts[0], "ms_add_median": statistics.median(ts[1:]),
                         "GBps_add": 12.0 * (hi - lo) / statistics.median(ts[1:]) / 1e6}
    print("VRB " + json.dumps(out), flush=True)


def run_child(root: str, K: int, args, kernel: bool = False) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--K", str(K), "--steps", str(args.steps), "--warmup",
           str(args.warmup)] + (["--kernel"] if kernel else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"measurement process failed ({root}, K={K}): exit {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("VRB ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", type=str, default=None, help="a built checkout of the parent commit (its plain TrainStep is the baseline)")
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--root", type=str, default=os.path.dirname(HERE))
    args = ap.parse_args()
    if args.child:
        child(args.root, args.K, args.steps, args.warmup, args.kernel)
        return
    here = os.path.dirname(HERE)
    print(f"# B={B} bf16 LAMB {H}x{W}, {args.steps} steps behind {args.warmup} warm-up steps per process, {args.rounds} rounds, interleaved")
    res = {"parent": [], "k1": [], "kK": []}
    for rnd in range(args.rounds):
        order = [("parent", args.parent, 1), ("k1", here, 1), ("kK", here, args.K)]
        for key, root, K in order:
            if root is None:
                continue
            r = run_child(root, K, args, kernel=(key == "k1" and rnd == 0))
            res[key].append(r)
            print(f"round {rnd} {key:6s} K={K}: {r['ms_per_micro_batch']:.3f} ms per micro-batch, peak {r['peak_mb']:.0f} MB, loss {r['loss']:.6f}")
            for name in ("arena", "last_bucket"):
                if name in r:
                    k = r[name]
                    print(f"  dc_grad_accumulate {name}: {k['elements']} floats, first (copy) {k['ms_first']:.4f} ms, add {k['ms_add_median']:.4f} ms "
                          f"({k['GBps_add']:.0f} GB/s over 12 bytes per element)")
    med = {k: statistics.median(r["ms_per_micro_batch"] for r in v) for k, v in res.items() if v}
    spread = {k: (min(r["ms_per_micro_batch"] for r in v), max(r["ms_per_micro_batch"] for r in v)) for k, v in res.items() if v}
    for k in med:
        print(f"median {k:6s}: {med[k]:.3f} ms per micro-batch (min {spread[k][0]:.3f}, max {spread[k][1]:.3f}), peak {res[k][0]['peak_mb']:.0f} MB")
    base = med.get("parent", med["k1"])
    print(f"K=1 over {'parent' if 'parent' in med else 'itself'}: {med['k1'] / base:.4f}")
    print(f"K={args.K} per micro-batch over {'parent' if 'parent' in med else 'K=1'}'s step: {med['kK'] / base:.4f} "
          f"({med['kK'] - base:+.3f} ms per micro-batch)")
    print(f"peak memory K={args.K} over K=1: {res['kK'][0]['peak_mb'] - res['k1'][0]['peak_mb']:+.0f} MB")


if __name__ == "__main__":
    main()
