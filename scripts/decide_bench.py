#!/usr/bin/env python3
"""Times the decision rule (dc_logits_decide, dc_hysteresis_select; nn.DecisionRule) at batch 8, 768 x 1152, on two kinds of frames, and
records beside it, in the same process,

  the plain route (one pass: decide_q_vec) and the hysteresis route (decide_q_vec, dc_mask_components on the candidates, decide_mark,
      decide_select), and the hysteresis route's three parts on their own;
  dc_prob_score (K = 20) on the same logits: decide_q* does strictly less per pixel (no histogram, no LDS atomics, no squared errors),
      so it should not be slower;
  nn.EventFilter on the mask the hysteresis route leaves (components + statistics + shape + select): the hysteresis route (components +
      mark + select) should not be slower;
  the forward pass of the same batch (nn.Predictor, bf16, logits stored): its code is what the parent commit has.

The frames: "realistic" is about 97 % background with the classifier sure of it and blocky events of the two other classes, whose
probabilities spread across the two thresholds; "uniform" has 3 * randn logits, so that candidates and seeds are specks everywhere.  One
full-size frame per kind is first compared with the numpy checker of tests/util_decide.py outside the pixels where fp32 and float64 may
round apart.  Every call is timed with HIP events; a block's figure is the median of its calls, a row's figure the median of its blocks,
and the blocks of the rows alternate.  Only standard output belongs in the profile:

    python scripts/decide_bench.py [--blocks 5] [--calls 20] 2>/dev/null > profiles/decide.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from event_match_bench import B, H, W, time_block  # noqa: E402
from prob_skill_bench import realistic, uniform  # noqa: E402

LOW, HIGH = (0.5, 0.5), (0.9, 0.9)


def against_checker(kind, logits_host, dev):
    """frame 0 through both routes against tests/util_decide.py; returns the line to print"""
    import util_decide as ud
    import util_prob as up
    lg = torch.from_numpy(logits_host).to(dev)
    qlow, qhigh = [dnn.decision_q(v) for v in LOW], [dnn.decision_q(v) for v in HIGH]
    s = up.scaled_softmax(logits_host[0])
    near = np.zeros((H, W), bool)
    for c in (1, 2):
        for t in (qlow[c - 1], qhigh[c - 1]):
            near |= np.abs(s[c] - (t - 0.5)) < up.EPS
    q = up.quantise(logits_host[0])
    near |= (q[1] >= qlow[0]) & (q[2] >= qlow[1]) & up.ambiguous(logits_host[0])
    rule = dnn.DecisionRule(B, H, W, low=LOW, high=HIGH, device=dev)
    out = rule(lg, n_valid=1)[0].cpu().numpy()
    cand = rule.candidate_buffer[0].cpu().numpy()
    counts = rule.counts()[0].cpu().numpy()
    ref_cand, _, ref_out, ref_counts = ud.frame(logits_host[0], qlow, qhigh)
    if near.any():                                    # a pixel that may round apart can change its whole component: compare the candidates
        same = np.array_equal(cand[~near], ref_cand[~near])
        what = f"candidates equal outside {int(near.sum())} pixels near a rounding boundary" if same else "candidates DIFFERENT"
    else:
        same = np.array_equal(cand, ref_cand) and np.array_equal(out, ref_out) and np.array_equal(counts, ref_counts)
        what = "candidates, mask and the 12 counters equal" if same else "DIFFERENT"
    return f"{kind}: one full-size frame against the numpy checker: {what}; counters {counts.tolist()}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="leave out the forward pass")
    ap.add_argument("--no_checker", action="store_true", help="leave out the comparison with the numpy checker (a flood fill in Python)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"{torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}; {a.blocks} blocks of {a.calls} calls per figure, HIP events, medians")
    print(f"thresholds: low {LOW}, high {HIGH} (class 1, class 2), connectivity 8, periodic columns")
    rs = np.random.RandomState(17)
    frames = {"realistic": realistic(rs), "uniform": uniform(rs)}
    print(f"realistic frames: background {100 * (frames['realistic'][1] == 0).mean():.2f} % of the pixels")
    if not a.no_checker:
        for kind, (lg_host, _) in frames.items():
            print(against_checker(kind, lg_host, dev))

    routes, notes = {}, {}
    st = L.stream_ptr()
    for kind, (lg_host, lb_host) in frames.items():
        lg, lb = torch.from_numpy(lg_host).to(dev), torch.from_numpy(lb_host).to(dev)
        plain = dnn.DecisionRule(B, H, W, low=LOW, device=dev)
        hyst = dnn.DecisionRule(B, H, W, low=LOW, high=HIGH, device=dev)
        plain(lg)
        mask = hyst(lg).clone()
        c = hyst.counts().sum(dim=0).cpu().tolist()
        notes[kind] = (f"candidates {100 * (c[0] + c[5]) / (B * H * W):.2f} % of the pixels, seeds {100 * (c[1] + c[6]) / (B * H * W):.2f} %, kept "
                       f"{100 * (c[2] + c[7]) / (B * H * W):.2f} %; events {c[3] + c[8]} of which kept {c[4] + c[9]}; conflicts {c[11]}")
        ps = dnn.ProbabilitySkill(B, H, W, bins=20, device=dev)
        efilter = dnn.EventFilter(dnn.EventCatalog(B, H, W, device=dev), min_pixels=(16, 16), min_length_km=(0, 500))
        routes[f"DecisionRule, plain, {kind}"] = (lambda r=plain, lg=lg: r(lg))
        routes[f"DecisionRule, hysteresis, {kind}"] = (lambda r=hyst, lg=lg: r(lg))
        routes[f"  dc_logits_decide with seeds, {kind}"] = (lambda r=hyst, lg=lg: L.call(
            "dc_logits_decide", B, B, H, W, L.dptr(lg), r.low[0], r.low[1], r.high[0], r.high[1], L.dptr(r._cand), L.dptr(r._seed),
            L.dptr(r._counts), st))
        routes[f"  dc_mask_components on the candidates, {kind}"] = (lambda r=hyst: L.call(
            "dc_mask_components", B, B, H, W, L.dptr(r._cand), 8, 1, L.dptr(r._labels), L.dptr(r._ws), st))
        routes[f"  dc_hysteresis_select, {kind}"] = (lambda r=hyst: L.call(
            "dc_hysteresis_select", B, B, H, W, L.dptr(r._cand), L.dptr(r._seed), L.dptr(r._labels), L.dptr(r._flags), L.dptr(r._out),
            L.dptr(r._counts), st))
        routes[f"dc_prob_score, K = 20, {kind}"] = (lambda ps=ps, lg=lg, lb=lb: ps(lg, lb))
        routes[f"EventFilter on the decided mask, {kind}"] = (lambda f=efilter, m=mask: f(m))
    predictor = None
    if not a.no_forward:
        g = torch.Generator().manual_seed(5)
        x = torch.rand(B, 16, H, W, generator=g).to(dev)
        net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
        net.materialize(1, H, W)
        net.eval()
        predictor = dnn.Predictor(net, B, H, W)
        predictor.store_logits = True
        routes["forward pass (nn.Predictor, bf16), logits stored"] = lambda: predictor(x)
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
    for kind in frames:
        plain, hyst = med[f"DecisionRule, plain, {kind}"], med[f"DecisionRule, hysteresis, {kind}"]
        prob, filt = med[f"dc_prob_score, K = 20, {kind}"], med[f"EventFilter on the decided mask, {kind}"]
        nbytes = B * H * W * 13                       # 12 bytes of logits in, one byte of candidates out
        print(f"{kind}: {notes[kind]}")
        print(f"    plain route: {nbytes / 1e6:.1f} MB per call, {nbytes / plain / 1e9:.2f} TB/s at {plain:.3f} ms; dc_prob_score {prob:.3f} ms: "
              f"decide / prob_score = {plain / prob:.2f} ({'not slower, as expected' if plain <= prob else 'SLOWER than expected'})")
        print(f"    hysteresis route {hyst:.3f} ms, EventFilter route {filt:.3f} ms: hysteresis / filter = {hyst / filt:.2f} "
              f"({'not slower, as expected' if hyst <= filt else 'SLOWER than expected'})")
    if predictor is not None:
        fwd = med["forward pass (nn.Predictor, bf16), logits stored"]
        worst = max(med[f"DecisionRule, hysteresis, {kind}"] for kind in frames)
        print(f"forward pass {fwd:.3f} ms: the slowest hysteresis row is {100 * worst / fwd:.2f} % of it")
        predictor.close()


if __name__ == "__main__":
    main()
