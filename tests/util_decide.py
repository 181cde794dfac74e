"""Checker of the decision rule (nn.DecisionRule, dc_logits_decide / dc_hysteresis_select): the definition of include/deepcam_hip.h in
numpy, with no knowledge of the kernels' workgroups, waves, flags or union-find.

Per pixel with logits l0, l1, l2: q = util_prob.quantise (float64 softmax, rint(p * 65536)).  The rule is four integers in [0, 65537],
low[1], low[2], high[1], high[2], high >= low, 65537 = never.  Class c in {1, 2} QUALIFIES iff q_c >= low[c]; the candidate class is 0 if
neither qualifies, the qualifying class if one does, the class with the larger q if both do (class 1 on equal q).  A pixel is a SEED iff
its candidate class c != 0 and q_c >= high[c] (the class that lost a conflict seeds nothing).  A pixel with a logit that is not finite is
background, no seed, and counted.  out[p] = cand[p] iff the connected component of cand that holds p (one class, connectivity 4 or 8,
columns periodic with wrap, rows never: util_events' flood fill) holds a seed, else 0.
The 12 counters: per class (1, then 2) candidate pixels, seed pixels, kept pixels, candidate events, kept events; pixels with a non-finite
logit; pixels where both classes qualified.  On the plain route (high == low, no component pass) kept pixels = candidate pixels and the
event words are 0.
The device rounds p * 65536 in fp32, this checker in float64: smooth_logits builds data that stand clear of every rounding boundary."""
import numpy as np

import util_events as ue
import util_prob as up

ONE = 65536
NEVER = ONE + 1
COUNTS = 12


def candidates(logits, low, high):
    """logits float32 [3, H, W]; low, high: (class 1, class 2) integers -> (cand uint8, seed uint8, nonfinite bool, both bool), each [H, W]"""
    l = np.asarray(logits, np.float32)
    nonfinite = ~np.isfinite(l).all(axis=0)
    q = up.quantise(np.where(nonfinite[None], np.float32(0), l))
    a1, a2 = (q[1] >= int(low[0])) & ~nonfinite, (q[2] >= int(low[1])) & ~nonfinite
    both = a1 & a2
    cand = np.where(both, np.where(q[2] > q[1], 2, 1), np.where(a1, 1, np.where(a2, 2, 0))).astype(np.uint8)
    seed = (((cand == 1) & (q[1] >= int(high[0]))) | ((cand == 2) & (q[2] >= int(high[1])))).astype(np.uint8)
    return cand, seed, nonfinite, both


def keep_seeded(cand, seed, connectivity, wrap):
    """(out uint8 [H, W], per class (candidate events, kept events)): the components of cand that hold a seed"""
    H, W = cand.shape
    zeros_h, zeros_w = np.zeros(H, np.int64), np.zeros(W, np.int64)
    labels, rows = ue.label_one(cand, connectivity, wrap, zeros_h, zeros_w, zeros_w)
    seeded = np.unique(labels[seed != 0])
    assert (seeded > 0).all()
    out = np.where(np.isin(labels, seeded), cand, 0).astype(np.uint8)
    events = []
    for c in (1, 2):
        roots = rows[rows[:, 1] == c, 0] + 1
        events.append((len(roots), int(np.isin(roots, seeded).sum())))
    return out, events


def frame(logits, low, high, connectivity=8, wrap=True, plain=False):
    """(cand, seed, out uint8 [H, W], counts int64 [12]) of one frame.  plain: the route without a component pass (asserts high == low):
    out = cand, kept pixels = candidate pixels, no events."""
    cand, seed, nonfinite, both = candidates(logits, low, high)
    if plain:
        assert tuple(low) == tuple(high)
        out, events = cand.copy(), [(0, 0), (0, 0)]
    else:
        out, events = keep_seeded(cand, seed, connectivity, wrap)
    counts = np.zeros(COUNTS, np.int64)
    for k, c in enumerate((1, 2)):
        counts[5 * k:5 * k + 5] = [(cand == c).sum(), ((seed != 0) & (cand == c)).sum(), (out == c).sum(), events[k][0], events[k][1]]
    counts[10], counts[11] = nonfinite.sum(), both.sum()
    return cand, seed, out, counts


def batch(logits, low, high, connectivity=8, wrap=True, plain=False):
    """frame() over the leading axis: (cand, seed, out [n, H, W], counts [n, 12])"""
    got = [frame(l, low, high, connectivity, wrap, plain) for l in logits]
    return tuple(np.stack([g[k] for g in got]) for k in range(4))


def clear_triples(q1, q2, min_clearance=0.25):
    """float32 logits [3, ...] whose quantised softmax is exactly (65536 - q1 - q2, q1, q2): integer triples >= 1 summing to 65536 through
    util_prob.logits_of, every pixel at least min_clearance q-units clear of a rounding boundary in float64 (asserted).  A triple that
    fails as plain log(q / 65536) is nudged by a per-pixel shift of the three logits, which changes the fp32 roundings, not the softmax."""
    q1, q2 = np.asarray(q1, np.int64), np.asarray(q2, np.int64)
    q = np.stack([ONE - q1 - q2, q1, q2])
    assert (q >= 1).all(), "every class needs q >= 1"
    logits = up.logits_of(q)
    for shift in (0.5, -0.75, 1.25, -2.0, 3.0, 0.3, -0.1, 0.7):
        bad = (up.distance_to_boundary(logits) < min_clearance) | (up.quantise(logits) != q).any(axis=0)
        if not bad.any():
            break
        logits[:, bad] = up.logits_of(q[:, bad], shift)
    assert up.distance_to_boundary(logits).min() >= min_clearance and np.array_equal(up.quantise(logits), q)
    return logits


def smooth_logits(rs, H, W, peak1=40000, peak2=50000, blobs=24):
    """(logits float32 [3, H, W], q int64 [3, H, W]): a spatially smooth field of probabilities -- per class a few dozen periodic bumps of
    mixed height and width over a noisy floor, so that thresholds between floor and peak cut regions of which only some hold a high
    pixel --, built as integer triples and turned into logits by clear_triples"""
    rr, cc = np.mgrid[0:H, 0:W]
    field = []
    for peak in (peak1, peak2):
        f = rs.randint(1, 400, size=(H, W)).astype(np.float64)
        for _ in range(blobs):
            r0, c0, sr, sc = rs.randint(0, H), rs.randint(0, W), rs.uniform(0.8, max(H / 14, 1.5)), rs.uniform(1.0, max(W / 20, 2.5))
            dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))               # periodic columns: bumps cross the seam
            f += peak * rs.uniform(0.12, 1.0) * np.exp(-0.5 * (((rr - r0) / sr) ** 2 + (dc / sc) ** 2))
        field.append(np.clip(np.rint(f), 1, 32000).astype(np.int64))
    logits = clear_triples(field[0], field[1])
    return logits, up.quantise(logits)
