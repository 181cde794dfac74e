"""Checker of the view ensemble (nn.ViewEnsemble, nn.view_input; dc_input_view_hwc, dc_ensemble_add, dc_ensemble_pool): the definitions
of include/deepcam_hip.h in numpy, the softmax in float64 through util_prob.quantise, with no knowledge of workgroups, waves or LDS cells
and of the packing only the documented bit layout.

A VIEW is (roll, flip), 0 <= roll < W: view pixel (h, w) shows source pixel src(h, w) = (H - 1 - h if flip else h, (w + roll) mod W).
The view of the input is out[n, h, w, j] = scale[j] * (sign[j] * x[n, src(h, w), channels[j]] - shift[j]).
A MEMBER is fp32 logits [3, H, W] in view coordinates, its view and a weight per SOURCE column (uint16 >= 1, None: 1).  At source pixel p,
with the logits of the view pixel that shows p: not all finite -> bad[p] += 1 and nothing else; otherwise q = quantise(l), S_c[p] +=
wt[col(p)] * q_c and votes[argmax_first(l)][p] += 1; member 0 sets first[p] = argmax_first(l), 3 where it was not finite.
The STATE is uint32 [4, H, W]: S_0, S_1, S_2, and votes_0 | votes_1 << 6 | votes_2 << 12 | bad << 18 | first << 24.
The POOL, where bad == 0: top = the first class with the largest S_c, L_c = float32(log(max(S_c, 1) / S_top)) (float64 inside); three NaNs
where bad > 0.  ROWS int64 [208]: word 64 c + k the pixels with exactly k votes for class c, word 192 + 4 i + j the pixels whose first is i
and whose pooled class is j (3: not finite).
The device rounds p * 65536 in fp32, this checker in float64: the tests' constructed logits stand clear of every rounding boundary."""
import numpy as np

import util_prob as up

ROW = 208
CHANGED = 192
MAX_MEMBERS = 63


def source_of(h, w, H, W, roll, flip):
    """src(h, w)"""
    return (H - 1 - h if flip else h), (w + roll) % W


def to_source(a, roll, flip):
    """an array [..., H, W] in view coordinates -> source coordinates: out[..., src(h, w)] = a[..., h, w]"""
    a = np.asarray(a)
    return np.roll(a[..., ::-1, :] if flip else a, roll, axis=-1)


def to_view(a, roll, flip):
    """an array [..., H, W] in source coordinates -> view coordinates: out[..., h, w] = a[..., src(h, w)]"""
    a = np.roll(np.asarray(a), -roll, axis=-1)
    return a[..., ::-1, :] if flip else a


def view_input(x, channels, sign, shift, scale, roll, flip):
    """float64 [N, H, W, C] of x float32 [N, H, W, Cfile]: scale[j] * (sign[j] * x[n, src(h, w), channels[j]] - shift[j])"""
    x = np.asarray(x, np.float64)
    C = len(shift)
    channels = np.arange(C) if channels is None else np.asarray(channels)
    sign = np.ones(C) if sign is None else np.asarray(sign, np.float64)
    v = np.moveaxis(to_view(np.moveaxis(x[..., channels], -1, 1), roll, flip), 1, -1)
    return np.asarray(scale, np.float64) * (sign * v - np.asarray(shift, np.float64))


def argmax_first(logits):
    """int64 [...]: the first maximum over axis 0 (torch.max's class)"""
    return np.argmax(np.asarray(logits), axis=0).astype(np.int64)


def seam_weights(W, roll, margin):
    """uint16 [W] in source coordinates: min(d + 1, margin), d the distance of the pixel's view column to the nearer edge of the view"""
    out = np.zeros(W, np.uint16)
    for ws in range(W):
        w = (ws - roll) % W
        out[ws] = min(min(w, W - 1 - w) + 1, margin)
    return out


def accumulate(members):
    """members: a list of (logits float32 [3, H, W] in view coordinates, roll, flip, weights uint16 [W] or None), member 0 first ->
    (S int64 [3, H, W], votes int64 [3, H, W], bad int64 [H, W], first int64 [H, W]) in source coordinates"""
    assert 1 <= len(members) <= MAX_MEMBERS
    _, H, W = np.asarray(members[0][0]).shape
    S, votes = np.zeros((3, H, W), np.int64), np.zeros((3, H, W), np.int64)
    bad, first = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for m, (logits, roll, flip, weights) in enumerate(members):
        l = to_source(np.asarray(logits, np.float32), roll, flip)
        finite = np.isfinite(l).all(axis=0)
        q = up.quantise(np.where(finite[None], l, np.float32(0)))
        am = argmax_first(l)
        wt = np.ones(W, np.int64) if weights is None else np.asarray(weights).astype(np.int64)
        assert wt.shape == (W,) and (wt >= 1).all()
        S += np.where(finite[None], q * wt[None, None, :], 0)
        for c in range(3):
            votes[c] += finite & (am == c)
        bad += ~finite
        if m == 0:
            first = np.where(finite, am, 3)
    assert S.max() < 2 ** 32
    return S, votes, bad, first


def pack(S, votes, bad, first):
    """uint32 [4, H, W]: the documented state words"""
    assert votes.max() <= 63 and bad.max() <= 63 and first.max() <= 3
    packed = votes[0] | (votes[1] << 6) | (votes[2] << 12) | (bad << 18) | (first << 24)
    return np.concatenate([S, packed[None]]).astype(np.uint32)


def unpack(words):
    """(S, votes, bad, first) int64 of uint32 words [4, H, W]"""
    w = np.asarray(words).astype(np.int64)
    pk = w[3]
    return w[:3], np.stack([pk & 63, (pk >> 6) & 63, (pk >> 12) & 63]), (pk >> 18) & 63, (pk >> 24) & 3


def top_class(S, bad):
    """int64 [H, W]: the first class with the largest S_c, 3 where bad > 0"""
    return np.where(bad > 0, 3, np.argmax(S, axis=0)).astype(np.int64)


def pool(S, bad):
    """(L float64 [3, H, W] BEFORE the rounding to fp32 -- NaN where bad > 0 --, top int64 [H, W])"""
    top = top_class(S, bad)
    s_top = np.maximum(S.max(axis=0), 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        L = np.log(np.maximum(S, 1).astype(np.float64) / s_top[None])
    return np.where((bad > 0)[None], np.nan, L), top


def rows(votes, first, top):
    """int64 [208] of one frame"""
    out = np.zeros(ROW, np.int64)
    for c in range(3):
        out[64 * c:64 * c + 64] = np.bincount(votes[c].reshape(-1), minlength=64)
    out[CHANGED:] = np.bincount((4 * first + top).reshape(-1), minlength=16)
    return out


def frame(members):
    """(state uint32 [4, H, W], L float64 [3, H, W], top int64 [H, W], rows int64 [208]) of one frame's members"""
    S, votes, bad, first = accumulate(members)
    L, top = pool(S, bad)
    return pack(S, votes, bad, first), L, top, rows(votes, first, top)


def shares(S):
    """float64 [3, ...]: 65536 * max(S_c, 1) / sum_k max(S_k, 1), what prob_q of the pooled logits stands for"""
    s = np.maximum(np.asarray(S, np.int64), 1).astype(np.float64)
    return 65536.0 * s / s.sum(axis=0, keepdims=True)


def brute_frame(members):
    """frame() a second time, one pixel and one member at a time, in Python integers: (state, L, top, rows)"""
    import math
    _, H, W = np.asarray(members[0][0]).shape
    state = np.zeros((4, H, W), np.uint32)
    L = np.full((3, H, W), np.nan, np.float64)
    top = np.zeros((H, W), np.int64)
    out_rows = [0] * ROW
    for hs in range(H):
        for ws in range(W):
            S, votes, bad, first = [0, 0, 0], [0, 0, 0], 0, 0
            for m, (logits, roll, flip, weights) in enumerate(members):
                h = H - 1 - hs if flip else hs
                w = (ws - roll) % W
                assert source_of(h, w, H, W, roll, flip) == (hs, ws)
                l = [float(np.float32(logits[c][h][w])) for c in range(3)]
                if not all(math.isfinite(v) for v in l):
                    bad += 1
                    if m == 0:
                        first = 3
                    continue
                big = max(l)
                e = [math.exp(v - big) for v in l]
                q = [int(np.rint(v / sum(e) * 65536.0)) for v in e]
                am = l.index(big)
                wt = 1 if weights is None else int(weights[ws])
                for c in range(3):
                    S[c] += wt * q[c]
                votes[am] += 1
                if m == 0:
                    first = am
            state[:3, hs, ws] = S
            state[3, hs, ws] = votes[0] | votes[1] << 6 | votes[2] << 12 | bad << 18 | first << 24
            t = 3
            if bad == 0:
                t = S.index(max(S))
                for c in range(3):
                    L[c, hs, ws] = math.log(max(S[c], 1) / S[t])
            top[hs, ws] = t
            for c in range(3):
                out_rows[64 * c + votes[c]] += 1
            out_rows[CHANGED + 4 * first + t] += 1
    return state, L, top, np.asarray(out_rows, np.int64)


def decode(totals, frames, members):
    """the definitions of nn.ViewEnsemble.decode, written a second time"""
    t = [int(v) for v in totals]
    pixels = sum(t[0:64])
    changed = [[t[CHANGED + 4 * i + j] for j in range(4)] for i in range(4)]
    div = lambda a, b: None if b == 0 else a / b  # noqa: E731
    out = {"frames": int(frames), "members": int(members), "pixels": pixels, "not_finite": sum(changed[i][3] for i in range(4)),
           "unanimous": div(t[members] + t[64 + members] + t[128 + members], pixels) if members else None, "changed": changed}
    for c in range(3):
        out[f"class_{c}"] = {"vote_share": [div(t[64 * c + k], pixels) for k in range(members + 1)],
                             "mean_votes": div(sum(k * t[64 * c + k] for k in range(64)), pixels),
                             "gained": sum(changed[i][c] for i in range(4)) - changed[c][c],
                             "lost": sum(changed[c]) - changed[c][c]}
    return out
