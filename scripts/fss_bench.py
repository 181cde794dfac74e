#!/usr/bin/env python3
"""Times the neighbourhood verification (dc_fss_score; nn.FractionsSkill) at batch 8, 768 x 1152, the default windows 1, 3, 9, 17, 33, 65,
129, periodic columns, on the blob masks of scripts/event_match_bench.py (a = prediction, b = labels), and prints beside it

  the bytes the design moves and the bandwidth that makes of the time -- the horizontal pass reads both masks once (one byte per pixel
      and side, the halo of the widest window per strip on top) and writes one word per pixel and window; the vertical pass reads, per
      window, segment of TR rows and column, the 2 r + 1 words of the warm-up and 2 (TR - 1) words while it slides.  Most of the vertical
      pass's reads are re-reads of words a neighbouring segment or an earlier row also asked for, which the caches serve, so the figure
      is a rate of REQUESTED bytes, not an HBM rate;
  the forward pass of the same batch (nn.Predictor, bf16), the thing the score runs behind;
  a plain PyTorch evaluation of the same sums on the same GPU: circular padding in longitude, zero padding at the poles, two int64
      cumulative sums per window (an integral image) and four gathers of it, then the squared terms in int64 -- checked for equality with
      the HIP rows before it is timed.

The HIP rows of the full-size batch are first compared with the numpy checker of tests/util_fss.py.  Every call is timed with HIP events;
a block's figure is the median of its calls, a row's figure the median of its blocks.  Only standard output belongs in the profile:

    python scripts/fss_bench.py [--blocks 5] [--calls 10] 2>/dev/null > profiles/fss.txt"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, blob_masks, time_block  # noqa: E402


def design_bytes(windows) -> int:
    """the bytes one call requests under the kernels' rules (module docstring)"""
    cols, seg = C.c_int(0), C.c_int(0)
    L.check(L.load().dc_fss_block(C.byref(cols), C.byref(seg)))
    TC, TR = cols.value, seg.value
    strips, segments = -(-W // TC), -(-H // TR)
    radii = [(n - 1) // 2 for n in windows]
    # the horizontal pass: both masks with the halo of the widest window, one word per pixel and window
    total = 2 * B * H * (W + strips * 2 * max(radii)) + 4 * B * H * W * len(radii)
    for r in radii:                                   # the vertical pass: warm-up and slide, clipped to the frame
        rows = 0
        for s in range(segments):
            i0, i1 = s * TR, min(H, (s + 1) * TR)
            rows += min(i0 + r, H - 1) - max(i0 - r, 0) + 1
            rows += sum((i + 1 + r < H) + (i - r >= 0) for i in range(i0, i1 - 1))
        total += 4 * B * W * rows
    return total


def torch_rows(pred: torch.Tensor, truth: torch.Tensor, windows) -> torch.Tensor:
    """int64 [B, 2, S, 3] by plain PyTorch operators: an integral image of the padded indicator fields per window"""
    ind = torch.stack([pred == 1, truth == 1, pred == 2, truth == 2], dim=1).to(torch.int64)        # [B, 4, H, W]
    out = torch.empty((pred.shape[0], 2, len(windows), 3), dtype=torch.int64, device=pred.device)
    for s, n in enumerate(windows):
        r = (n - 1) // 2
        wide = torch.cat([ind[..., ind.shape[-1] - r:], ind, ind[..., :r]], dim=-1) if r else ind
        wide = torch.nn.functional.pad(wide, (1, 0, r + 1, r))                                      # a zero row and column in front: I[0] = 0
        integral = wide.cumsum(dim=-2).cumsum(dim=-1)
        box = integral[..., n:, n:] - integral[..., :-n, n:] - integral[..., n:, :-n] + integral[..., :-n, :-n]
        F, O = box[:, 0::2], box[:, 1::2]                                                           # [B, 2, H, W] each
        out[:, :, s, 0] = ((F - O) ** 2).sum(dim=(-2, -1))
        out[:, :, s, 1] = (F * F).sum(dim=(-2, -1))
        out[:, :, s, 2] = (O * O).sum(dim=(-2, -1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no_checker", action="store_true", help="leave out the numpy checker at full size (about a minute of host time)")
    a = ap.parse_args()
    import util_fss as uf
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    windows = list(dnn.FSS_WINDOWS)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, windows {windows}, periodic columns; {a.blocks} blocks of {a.calls} calls "
          f"per figure, HIP events, medians")
    pred_h, truth_h = blob_masks(np.random.RandomState(7))
    pred, truth = torch.from_numpy(pred_h).to(dev), torch.from_numpy(truth_h).to(dev)
    fs = dnn.FractionsSkill(B, H, W, windows=windows, device=dev)
    fs(pred, truth)
    rows = fs.frame_rows()[0].clone()
    torch.cuda.synchronize()
    if not a.no_checker:
        t0 = time.perf_counter()
        ref = uf.batch_rows(pred_h, truth_h, windows)[0]
        same = np.array_equal(rows.cpu().numpy(), ref)
        print(f"full size against the numpy checker: {'equal' if same else 'DIFFERENT'} (the checker took {time.perf_counter() - t0:.1f} s on "
              f"the host, {1000 * (time.perf_counter() - t0) / B:.0f} ms per frame)")
    plain = torch_rows(pred, truth, windows)
    print(f"plain PyTorch evaluation against the HIP rows: {'equal' if torch.equal(plain, rows) else 'DIFFERENT'}")
    res = fs.result()
    for k in (1, 2):
        c = res[f"class_{k}"]
        print(f"    class {k}: base rate {c['base_rate']:.4f}, useful {c['useful']:.4f}, skilful from window {c['skilful_window']}; FSS "
              + " ".join(f"{f:.4f}" for f in c["fss"]))
    del plain

    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 16, H, W, generator=g).to(dev)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(1, H, W)
    net.eval()
    predictor = dnn.Predictor(net, B, H, W)
    routes = {"dc_fss_score (nn.FractionsSkill)": lambda: fs(pred, truth),
              "plain PyTorch, int64 cumulative sums": lambda: torch_rows(pred, truth, windows),
              "forward pass (nn.Predictor, bf16)": lambda: predictor(x)}
    for fn in routes.values():                        # warm-up: code objects, weight repack, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(a.blocks):                         # alternating blocks
        for name, fn in routes.items():
            times[name].append(time_block(fn, a.calls))
    med = {name: statistics.median(v) for name, v in times.items()}
    nbytes = design_bytes(windows)
    ms = med["dc_fss_score (nn.FractionsSkill)"]
    print(f"workspace {fs._ws.numel() * 4 / 1e6:.1f} MB ({len(windows)} slabs of B * H * W words); launches per call: 3")
    for name, v in times.items():
        print(f"    {name:40s} {med[name]:9.3f} ms/batch   blocks {' '.join(f'{t:.3f}' for t in v)}")
    print(f"    the design requests {nbytes / 1e6:.1f} MB per call: {nbytes / ms / 1e9:.2f} TB/s of requested bytes at {ms:.3f} ms")
    print(f"    plain PyTorch / HIP = {med['plain PyTorch, int64 cumulative sums'] / ms:.1f} x; HIP / forward pass = "
          f"{100 * ms / med['forward pass (nn.Predictor, bf16)']:.2f} %")
    predictor.close()


if __name__ == "__main__":
    main()
