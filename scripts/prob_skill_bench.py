#!/usr/bin/env python3
"""Times the probabilistic verification (dc_prob_score; nn.ProbabilitySkill) at batch 8, 768 x 1152, K = 20 and K = 256 bins, on two kinds
of frames, and prints beside it

  the bytes the pass reads (12 bytes of logits and the label per pixel) and the rate that makes of the time, beside the rate
      profiles/climatology.txt records for this project's other streaming pass;
  the same integers by plain PyTorch operators on the same GPU: softmax, q = round(p * 65536), bins, and per class two bincounts (the
      counts and, weighted in float64 -- exact below 2^53 --, the sums of q) and the squared errors in int64.  PyTorch rounds the softmax
      in its own order, so single pixels may land a q-unit beside the HIP kernel's: the differing cells are counted, not refused;
  the forward pass of the same batch (nn.Predictor, bf16) with the logits stored (what --prob_skill switches on) and not stored.

The frames: "realistic" is more than 95 % background with the classifier sure of it (the background's probability in the top bin at K =
20, spread over the top bins at K = 256) and blocky events of the two other classes; "uniform" has 3 * randn logits and uniform labels,
so that a wave's lanes fall into different cells.  The HIP integers of the realistic frames are first compared with the numpy checker of
tests/util_prob.py on one frame (pixels the checker calls ambiguous masked through the label, as the tests do).  Every call is timed
with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks.  Only standard output belongs in
the profile:

    python scripts/prob_skill_bench.py [--blocks 5] [--calls 20] 2>/dev/null > profiles/prob_skill.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, time_block  # noqa: E402

CLIMATOLOGY_TBS = 4.73                                # profiles/climatology.txt: accumulate, 16 channels


def realistic(rs):
    """(logits fp32 [B, 3, H, W], labels uint8 [B, H, W]): 16 x 16 blocks, 3 % of them an event of class 1 or 2"""
    coarse = rs.rand(B, H // 16, W // 16)
    cls = np.where(coarse < 0.03, rs.randint(1, 3, size=coarse.shape), 0).astype(np.uint8)
    labels = np.ascontiguousarray(cls.repeat(16, 1).repeat(16, 2))
    logits = rs.randn(B, 3, H, W).astype(np.float32)
    logits[:, 0] += 8.0 * (labels == 0)
    for c in (1, 2):
        logits[:, c] += 3.0 * (labels == c)
    return logits, labels


def uniform(rs):
    return (3 * rs.randn(B, 3, H, W)).astype(np.float32), rs.randint(0, 3, size=(B, H, W)).astype(np.uint8)


def torch_integers(logits: torch.Tensor, labels: torch.Tensor, K: int):
    """(hist int64 [3, 2, K, 2], rows int64 [B, 3]) by plain PyTorch operators; every label is a class here"""
    q = torch.round(torch.softmax(logits, dim=1) * 65536.0).to(torch.int64)                        # [B, 3, H, W]
    bins = torch.clamp((q * K) >> 16, max=K - 1)
    hist = torch.empty((3, 2, K, 2), dtype=torch.int64, device=logits.device)
    rows = torch.empty((logits.shape[0], 3), dtype=torch.int64, device=logits.device)
    for c in range(3):
        o = (labels == c).to(torch.int64)
        flat = (o * K + bins[:, c]).reshape(-1)
        hist[c, :, :, 0] = torch.bincount(flat, minlength=2 * K).reshape(2, K)
        hist[c, :, :, 1] = torch.bincount(flat, weights=q[:, c].reshape(-1).double(), minlength=2 * K).to(torch.int64).reshape(2, K)
        d = q[:, c] - o * 65536
        rows[:, c] = (d * d).sum(dim=(-2, -1))
    return hist, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="leave out the forward pass")
    ap.add_argument("--no_torch", action="store_true", help="leave out the plain PyTorch rows (0.1 - 0.2 s per call at K = 20)")
    a = ap.parse_args()
    import util_prob as up
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    rs = np.random.RandomState(17)
    frames = {"realistic": realistic(rs), "uniform": uniform(rs)}
    lg_h, lb_h = frames["realistic"]
    print(f"realistic frames: background {100 * (lb_h == 0).mean():.2f} % of the pixels")

    # one full-size frame against the checker
    for K in (20, 256):
        masked = lb_h[:1].astype(np.int64)
        masked[np.stack([up.ambiguous(lg_h[0])])] = 255
        ps = dnn.ProbabilitySkill(B, H, W, bins=K, device=dev)
        lb8 = np.concatenate([masked.astype(np.uint8), lb_h[1:]])
        ps(torch.from_numpy(lg_h).to(dev), torch.from_numpy(lb8).to(dev), n_valid=1)
        hist, rows, pixels = up.batch(lg_h[:1], masked, K)
        same = np.array_equal(ps.batch_hist().cpu().numpy(), hist) and np.array_equal(ps.frame_rows()[0].cpu().numpy(), rows) \
            and np.array_equal(ps.frame_rows()[1].cpu().numpy(), pixels)
        print(f"K = {K:3d}: one full-size frame against the numpy checker: {'equal' if same else 'DIFFERENT'} "
              f"({int(pixels[0, 1])} of {H * W} pixels masked as ambiguous)")

    routes, notes = {}, {}
    for kind, (lg_host, lb_host) in frames.items():
        lg, lb = torch.from_numpy(lg_host).to(dev), torch.from_numpy(lb_host).to(dev)
        for K in (20, 256):
            ps = dnn.ProbabilitySkill(B, H, W, bins=K, device=dev)
            ps(lg, lb)
            got_hist, got_rows = ps.batch_hist().clone(), ps.frame_rows()[0].clone()
            ref_hist, ref_rows = torch_integers(lg, lb, K)
            top = ps.batch_hist()[0, :, K - 1, 0].sum().item() / (B * H * W)
            notes[(kind, K)] = (f"class 0 in its top bin: {100 * top:.1f} % of the pixels; plain PyTorch differs in "
                                f"{int((got_hist != ref_hist).sum())} of {got_hist.numel()} cells, {int((got_rows != ref_rows).sum())} of "
                                f"{got_rows.numel()} rows")
            routes[f"dc_prob_score, {kind}, K = {K}"] = (lambda ps=ps, lg=lg, lb=lb: ps(lg, lb))
            if not a.no_torch:
                routes[f"plain PyTorch, {kind}, K = {K}"] = (lambda lg=lg, lb=lb, K=K: torch_integers(lg, lb, K))
    predictor = None
    if not a.no_forward:
        g = torch.Generator().manual_seed(5)
        x = torch.rand(B, 16, H, W, generator=g).to(dev)
        net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
        net.materialize(1, H, W)
        net.eval()
        predictor = dnn.Predictor(net, B, H, W)

        def forward(store):
            predictor.store_logits = store
            predictor(x)
        routes["forward pass (nn.Predictor, bf16), logits not stored"] = lambda: forward(False)
        routes["forward pass (nn.Predictor, bf16), logits stored"] = lambda: forward(True)
    for fn in routes.values():                        # warm-up: code objects, weight repack, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(a.blocks):                         # alternating blocks
        for name, fn in routes.items():
            times[name].append(time_block(fn, a.calls))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name, v in times.items():
        print(f"    {name:55s} {med[name]:9.3f} ms/batch   blocks {' '.join(f'{t:.3f}' for t in v)}")
    nbytes = B * H * W * 13                           # uint8 labels
    for kind in frames:
        for K in (20, 256):
            ms = med[f"dc_prob_score, {kind}, K = {K}"]
            pt = med.get(f"plain PyTorch, {kind}, K = {K}", float("nan"))
            print(f"{kind}, K = {K}: {notes[(kind, K)]}")
            print(f"    reads {nbytes / 1e6:.1f} MB per call: {nbytes / ms / 1e9:.2f} TB/s at {ms:.3f} ms (the climatology pass streams at "
                  f"{CLIMATOLOGY_TBS} TB/s: {nbytes / CLIMATOLOGY_TBS / 1e9:.3f} ms for these bytes); plain PyTorch / HIP = {pt / ms:.1f} x")
    if predictor is not None:
        off, on = med["forward pass (nn.Predictor, bf16), logits not stored"], med["forward pass (nn.Predictor, bf16), logits stored"]
        worst = max(med[f"dc_prob_score, {kind}, K = {K}"] for kind in frames for K in (20, 256))
        print(f"forward pass: storing the logits costs {on - off:+.3f} ms ({100 * (on - off) / off:+.2f} %); the slowest dc_prob_score row "
              f"is {100 * worst / off:.2f} % of the forward pass")
        predictor.close()


if __name__ == "__main__":
    main()
