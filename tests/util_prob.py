"""Checker of the probabilistic verification (nn.ProbabilitySkill, dc_prob_score): the definition of include/deepcam_hip.h in numpy, the
softmax in float64, everything from q on in int64 and Python ints, with no knowledge of the kernel's workgroups, waves or LDS cells.

Per pixel with logits l0, l1, l2 and label y: p_c = softmax_c, q_c = rint(p_c * 65536), o_c = (y == c), bin_c = min(K - 1, (q_c * K) >> 16).
A pixel whose label is outside [0, 3) counts in pixels[1] and nowhere else; otherwise one with a logit that is not finite counts in
pixels[2] and nowhere else; every other pixel counts in pixels[0], in hist[c][o_c][bin_c] = (n, sum q_c) and in rows[c] = sum (q_c - o_c *
65536)^2.  The device rounds p_c * 65536 in fp32: ambiguous() marks the pixels where float64 stands within eps q-units of a rounding
boundary, which the tests then mask through the label."""
import numpy as np

ONE = 65536
EPS = 1.0 / 16                                       # q-units: twice the ~2^-5 that eight fp32 roundings below 2^-24 can add up to at 2^16


def scaled_softmax(logits):
    """float64 [3, ...]: softmax over axis 0 times 65536 (finite logits)"""
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True) * ONE


def quantise(logits):
    """int64 [3, ...]: q = rint(p * 65536)"""
    return np.rint(scaled_softmax(logits)).astype(np.int64)


def distance_to_boundary(logits):
    """float64 [...]: the smallest | frac(p_c * 65536) - 0.5 | over the classes"""
    s = scaled_softmax(logits)
    return np.abs(s - np.floor(s) - 0.5).min(axis=0)


def ambiguous(logits, eps=EPS):
    """bool [...]: a class's p_c * 65536 lies within eps of a rounding boundary"""
    return distance_to_boundary(logits) < eps


def frame(logits, labels, K):
    """(hist int64 [3, 2, K, 2], rows int64 [3], pixels int64 [3]) of one frame: logits [3, H, W], labels integers [H, W]"""
    logits = np.asarray(logits, np.float32)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    l = logits.reshape(3, -1)
    bad = (y < 0) | (y > 2)
    nonfinite = ~bad & ~np.isfinite(l).all(axis=0)
    scored = ~bad & ~nonfinite
    pixels = np.asarray([scored.sum(), bad.sum(), nonfinite.sum()], np.int64)
    hist = np.zeros((3, 2, K, 2), np.int64)
    rows = np.zeros(3, np.int64)
    if scored.any():
        q = quantise(l[:, scored])
        ys = y[scored]
        for c in range(3):
            o = (ys == c).astype(np.int64)
            b = np.minimum(K - 1, (q[c] * K) >> 16)
            flat = o * K + b
            sums = np.zeros(2 * K, np.int64)
            np.add.at(sums, flat, q[c])
            hist[c, :, :, 0] = np.bincount(flat, minlength=2 * K).reshape(2, K)
            hist[c, :, :, 1] = sums.reshape(2, K)
            d = q[c] - o * ONE
            rows[c] = int((d * d).sum())
    return hist, rows, pixels


def batch(logits, labels, K):
    """(hist [3, 2, K, 2] summed over the frames, rows [n, 3], pixels [n, 3]) of n frames"""
    hist = np.zeros((3, 2, K, 2), np.int64)
    rows = np.zeros((len(logits), 3), np.int64)
    pixels = np.zeros((len(logits), 3), np.int64)
    for b in range(len(logits)):
        h, rows[b], pixels[b] = frame(logits[b], labels[b], K)
        hist += h
    return hist, rows, pixels


def totals(batches, K):
    """the state after the batches, each (logits [n, 3, H, W], labels [n, H, W]), on top of zeros -- what nn.ProbabilitySkill.state()
    returns: hist int64 [3, 2, K, 2], sq [3] Python ints, pixels [3] ints, frames"""
    hist = np.zeros((3, 2, K, 2), np.int64)
    sq, pixels, frames = [0, 0, 0], [0, 0, 0], 0
    for logits, labels in batches:
        h, rows, px = batch(logits, labels, K)
        hist += h
        frames += len(rows)
        for c in range(3):
            sq[c] += sum(int(v) for v in rows[:, c])
            pixels[c] += int(px[:, c].sum())
    return {"hist": hist, "sq": sq, "pixels": pixels, "frames": frames}


def same_state(a, b):
    return np.array_equal(a["hist"], b["hist"]) and a["hist"].dtype == b["hist"].dtype and list(a["sq"]) == list(b["sq"]) \
        and list(a["pixels"]) == list(b["pixels"]) and a["frames"] == b["frames"]


def _div(a, b):
    return None if b == 0 else a / b


def decode(hist, sq, pixels, K):
    """the definitions of nn.ProbabilitySkill.decode, written a second time from the contingency table of every threshold"""
    h = np.asarray(hist, np.int64)
    out = {"bins": K, "pixels": {"scored": int(pixels[0]), "bad_label": int(pixels[1]), "not_finite": int(pixels[2])}}
    for c in range(3):
        n = [[int(h[c, o, k, 0]) for k in range(K)] for o in range(2)]
        s = [int(h[c, 0, k, 1]) + int(h[c, 1, k, 1]) for k in range(K)]
        nk = [n[0][k] + n[1][k] for k in range(K)]
        N0, N1 = sum(n[0]), sum(n[1])
        N = N0 + N1
        base = _div(N1, N)
        f = [_div(s[k], nk[k] * ONE) for k in range(K)]
        o = [_div(n[1][k], nk[k]) for k in range(K)]
        rel = res = ece = mce = None
        if N:
            rel = res = ece = 0.0
            mce = 0.0
            for k in range(K):
                if nk[k]:
                    rel += nk[k] * (f[k] - o[k]) ** 2
                    res += nk[k] * (o[k] - base) ** 2
                    ece += nk[k] * abs(f[k] - o[k])
                    mce = max(mce, abs(f[k] - o[k]))
            rel, res, ece = rel / N, res / N, ece / N
        pod, pofd, csi, bias = [], [], [], []
        for k in range(K + 1):
            a = sum(n[1][k:])                         # hits: labelled, forecast
            b = sum(n[0][k:])                         # false alarms
            m = sum(n[1][:k])                         # misses
            pod.append(_div(a, a + m)), pofd.append(_div(b, N0)), csi.append(_div(a, a + b + m)), bias.append(_div(a + b, a + m))
        auc = None
        if N0 and N1:
            auc = sum((pofd[k] - pofd[k + 1]) * (pod[k] + pod[k + 1]) / 2 for k in range(K))
        have = [k for k in range(K + 1) if csi[k] is not None]
        best = max(have, key=lambda k: (csi[k], -k)) if have else None
        unc = None if base is None else base * (1.0 - base)
        brier = _div(int(sq[c]), N << 32)
        out[f"class_{c}"] = {
            "n": N, "base_rate": base, "mean_probability": _div(sum(s), N * ONE), "brier": brier,
            "brier_skill": None if brier is None or not unc else 1.0 - brier / unc, "reliability": rel, "resolution": res, "uncertainty": unc,
            "ece": ece, "mce": mce, "curve": {"mean_probability": f, "observed_frequency": o, "n": nk}, "sharpness": [_div(v, N) for v in nk],
            "pod": pod, "pofd": pofd, "csi": csi, "bias": bias, "auc": auc, "best_csi": None if best is None else csi[best],
            "best_csi_threshold": None if best is None else best / K}
    return out


def constructed(rs, n, shift=True):
    """(logits float32 [3, n], q int64 [3, n]): integer triples >= 1 summing to 65536 and logits log(q / 65536) (+ a per-pixel constant),
    whose float64 softmax stands clear of every rounding boundary (the caller asserts by how much)"""
    a = rs.randint(1, ONE - 1, size=n)
    b = rs.randint(1, ONE - 1, size=n)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    hi = np.where(hi == lo, lo + 1, hi)               # three parts of [0, 65536): lo >= 1, hi - lo >= 1, 65536 - hi >= 1
    q = np.stack([lo, hi - lo, ONE - hi]).astype(np.int64)
    assert (q >= 1).all() and (q.sum(axis=0) == ONE).all()
    return logits_of(q, rs.uniform(-8.0, 8.0, size=n) if shift else 0.0), q


def logits_of(q, shift=0.0):
    """float32 logits [3, ...] whose softmax is q / 65536 (q >= 1, summing to 65536), plus a per-pixel shift"""
    return (np.log(np.asarray(q, np.float64) / ONE) + shift).astype(np.float32)
