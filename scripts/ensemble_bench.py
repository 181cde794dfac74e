#!/usr/bin/env python3
"""Times the view ensemble (dc_input_view_hwc, dc_ensemble_add, dc_ensemble_pool; nn.ViewEnsemble, nn.view_input) at batch 8, 768 x 1152,
for 1, 2 and 4 views, and records beside it, in the same process,

  the three passes on their own -- one view of the input (bf16 NHWC out), member 0 (a store), a further member (a read-modify-write)
      through the 16-byte and through the 4-byte kernel, the pool -- with the bytes each moves and what a streaming read of as many bytes
      would take at the 4.73 TB/s the climatology pass recorded (profiles/climatology.txt);
  what the ensemble adds to a batch for M views: M - 1 views of the input, M members, one pool;
  the same integers through plain PyTorch operators on the same GPU: torch.roll / flip of the logits, softmax, round, a weighted sum,
      the first maximum and the log of the ratio;
  the forward pass of the same batch (nn.Predictor, bf16, logits stored), of which M views cost M.

Every call is timed with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks, and the blocks
of the rows alternate.  Only standard output belongs in the profile:

    python scripts/ensemble_bench.py [--blocks 5] [--calls 20] 2>/dev/null > profiles/ensemble.txt"""
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
from prob_skill_bench import realistic  # noqa: E402

STREAM_TBS = 4.73                                   # profiles/climatology.txt: the vector accumulate pass
MARGIN = 8
VIEWS = {1: [(0, False)], 2: [(0, False), (W // 2, False)], 4: [(0, False), (W // 4, False), (W // 2, False), (3 * W // 4, False)]}


def torch_pool(members, weights):
    """(S int64 [B, 3, H, W], L fp32 [B, 3, H, W]) by plain PyTorch operators; members: (logits in view coordinates, roll, flip)"""
    S = None
    for (logits, roll, flip), wt in zip(members, weights):
        src = torch.roll(logits.flip(2) if flip else logits, roll, dims=3)
        q = torch.round(torch.softmax(src, dim=1) * 65536.0).to(torch.int64) * wt
        S = q if S is None else S + q
    top = S.amax(dim=1, keepdim=True)
    L_ = torch.log(S.clamp_min(1).double() / top.double()).float()
    return S, L_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="leave out the forward pass")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    rs = np.random.RandomState(23)
    logits = torch.from_numpy(realistic(rs)[0]).to(dev)
    g = torch.Generator().manual_seed(5)
    raw = (torch.rand(B, H, W, 16, generator=g) * torch.linspace(1, 300, 16) - 40.0).to(dev)
    shift = raw.amin(dim=(0, 1, 2)).contiguous()
    scale = (1.0 / (raw.amax(dim=(0, 1, 2)) - shift)).contiguous()
    xv = torch.empty((B, H, W, 16), dtype=torch.bfloat16, device=dev)
    # host arrays: ViewEnsemble uploads each once and knows its extremes without a read-back
    weights = {s: dnn.seam_weights(W, s, MARGIN) for s in [s for s, _ in VIEWS[4]] + [1]}
    wide = {s: torch.from_numpy(w.astype(np.int64)).to(dev).view(1, 1, 1, W) for s, w in weights.items()}

    ens = dnn.ViewEnsemble(B, H, W, device=dev)

    def batch(M):
        ens.begin()
        for s, flip in VIEWS[M]:
            if s or flip:
                dnn.view_input(raw, None, shift, scale, s, flip, None, xv)
            ens.add(logits, s, flip, weights[s])
        ens.pool()

    # the same integers by PyTorch operators, once, for the record
    S_t, L_t = torch_pool([(logits, s, f) for s, f in VIEWS[2]], [wide[s] for s, _ in VIEWS[2]])
    batch(2)
    S_d = (ens.state_buffer[:, :3].to(torch.int64) & 0xFFFFFFFF)
    differ = int((S_d != S_t).any(dim=1).sum())
    close = bool(torch.allclose(ens.logits_buffer, L_t, rtol=0, atol=1e-4))
    print(f"2 views against PyTorch operators: S differs at {differ} of {B * H * W} pixels (torch.softmax is not prob_q's chain: a q on a "
          f"rounding boundary may differ by one); pooled logits within 1e-4: {close}")
    del S_t, L_t

    px = B * H * W
    routes = {
        "view of the input (bf16 out), roll W/2": (lambda: dnn.view_input(raw, None, shift, scale, W // 2, False, None, xv), px * (64 + 32)),
        "view of the input (bf16 out), roll W/2 + flip": (lambda: dnn.view_input(raw, None, shift, scale, W // 2, True, None, xv), px * (64 + 32)),
        "member 0, ensemble_add_vec (store)": (lambda: ens.begin().add(logits, 0, False, weights[0]), px * (12 + 16)),
        "further member, ensemble_add_vec": (lambda: ens.add(logits, W // 2, False, weights[W // 2]) if ens.members < 60 else ens.begin().add(logits), px * (12 + 32)),
        "further member, ensemble_add (roll 1)": (lambda: ens.add(logits, 1, False, weights[1]) if ens.members < 60 else ens.begin().add(logits), px * (12 + 32)),
        "pool": (lambda: ens.pool(), px * (16 + 12)),
    }
    for M in VIEWS:
        routes[f"ensemble of {M} view(s): views + members + pool"] = (lambda M=M: batch(M), px * ((M - 1) * 96 + 28 + (M - 1) * 44 + 28))
        routes[f"PyTorch operators, {M} view(s)"] = (lambda M=M: torch_pool([(logits, s, f) for s, f in VIEWS[M]], [wide[s] for s, _ in VIEWS[M]]), 0)
    predictor = None
    if not a.no_forward:
        x = torch.rand(B, 16, H, W, generator=g).to(dev)
        net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
        net.materialize(1, H, W)
        net.eval()
        predictor = dnn.Predictor(net, B, H, W)
        predictor.store_logits = True
        routes["forward pass (nn.Predictor, bf16), logits stored"] = (lambda: predictor(x), 0)
    batch(1)
    for fn, _ in routes.values():                     # warm-up: code objects, weight repack, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(a.blocks):                         # alternating blocks
        for name, (fn, _) in routes.items():
            if name == "pool":
                batch(2)
            times[name].append(time_block(fn, a.calls))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name, v in times.items():
        nbytes = routes[name][1]
        floor = f"{nbytes / 1e6:8.1f} MB  {nbytes / med[name] / 1e9:5.2f} TB/s  streaming read at {STREAM_TBS} TB/s: {nbytes / STREAM_TBS / 1e9:6.3f} ms" if nbytes else ""
        print(f"    {name:52s} {med[name]:9.3f} ms/batch   {floor}   blocks {' '.join(f'{t:.3f}' for t in v)}")
    for M in VIEWS:
        own, ref = med[f"ensemble of {M} view(s): views + members + pool"], med[f"PyTorch operators, {M} view(s)"]
        line = f"{M} view(s): the ensemble's passes {own:.3f} ms per batch, PyTorch operators {ref:.3f} ms ({ref / own:.1f} x)"
        if predictor is not None:
            fwd = med["forward pass (nn.Predictor, bf16), logits stored"]
            line += f"; {M} forward pass(es) {M * fwd:.3f} ms: the passes are {100 * own / (M * fwd):.2f} % of them"
        print(line)
    if predictor is not None:
        predictor.close()


if __name__ == "__main__":
    main()
