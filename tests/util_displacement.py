"""Checker of the displacement verification (nn.DisplacementSkill, dc_displacement_score): the definition of include/deepcam_hip.h in numpy
and Python ints, by two algorithms that share nothing with the kernels' bit planes, funnel shifts and popcounts, and little with each other.

The prediction moved by (dy, dx), |dy|, |dx| <= R, is P'_k(y, x) = P_k(y - dy, (x - dx) mod W) where 0 <= y - dy < H, else 0: columns are
periodic, rows never.  hits[k][dy][dx] counts the pixels of the band row0 <= y < row1 with T_k = P'_k = 1; kept[k][dy] the predicted pixels
(y', x) with row0 <= y' + dy < row1; pixels[k] = (predicted pixels of the whole frame, labelled pixels inside the band).  A table is int64
[2][2 R + 1][2 R + 2]: cells 0 .. 2 R of row dy + R the hits for dx = -R .. R, the last cell kept.

table_by_pairs   lists the coordinates of the predicted pixels and of the labelled pixels inside the band, forms all pair differences dy =
                 y_T - y_P and dx = (x_T - x_P) mod W folded into (-W / 2, W / 2], and histograms those inside the window -- unique because
                 2 R + 1 <= W.  kept comes from the row sums of the prediction.  For sparse frames.
table_by_shifts  per (dy, dx) moves the rows with zero fill, np.rolls the columns, ANDs and sums; kept is the sum of the moved field inside
                 the band.  For dense frames, and to hold the first against."""
import ctypes as C
import functools
import math

import numpy as np


def classes(mask):
    """the two indicator fields of a mask of integers of any width: only the full-width values 1 and 2 are classes"""
    m = np.asarray(mask).astype(np.int64)
    return [m == 1, m == 2]


def _band(H, row_range):
    row0, row1 = (0, H) if row_range is None else (int(row_range[0]), int(row_range[1]))
    assert 0 <= row0 < row1 <= H
    return row0, row1


def table_by_pairs(pred, truth, R, row_range=None, chunk=1024):
    """(rows int64 [2, 2 R + 1, 2 R + 2], pixels int64 [2, 2]) of one frame"""
    H, W = np.asarray(pred).shape
    row0, row1 = _band(H, row_range)
    assert R >= 1 and 2 * R + 1 <= W
    S = 2 * R + 1
    rows, pixels = np.zeros((2, S, S + 1), np.int64), np.zeros((2, 2), np.int64)
    for k, (P, T) in enumerate(zip(classes(pred), classes(truth))):
        py, px = (a.astype(np.int64) for a in np.nonzero(P))
        ty, tx = (a.astype(np.int64) for a in np.nonzero(T))
        inside = (ty >= row0) & (ty < row1)
        ty, tx = ty[inside], tx[inside]
        pixels[k] = len(py), len(ty)
        hist = np.zeros(S * S, np.int64)
        for s in range(0, len(ty), chunk):
            dy = ty[s:s + chunk, None] - py[None, :]
            dx = (tx[s:s + chunk, None] - px[None, :]) % W
            dx = np.where(2 * dx > W, dx - W, dx)                               # into (-W / 2, W / 2]
            ok = (np.abs(dy) <= R) & (np.abs(dx) <= R)
            hist += np.bincount((dy[ok] + R) * S + dx[ok] + R, minlength=S * S)
        rows[k, :, :S] = hist.reshape(S, S)
        per_row = P.sum(axis=1).astype(np.int64)
        for dy in range(-R, R + 1):                                             # y' + dy inside the band
            lo, hi = max(0, row0 - dy), min(H, row1 - dy)
            rows[k, dy + R, S] = per_row[lo:hi].sum() if hi > lo else 0
    return rows, pixels


def moved(P, dy, dx):
    """P'(y, x) = P(y - dy, (x - dx) mod W), zero where y - dy is outside the frame"""
    H = P.shape[0]
    out = np.zeros_like(P)
    lo, hi = max(0, dy), min(H, H + dy)
    if hi > lo:
        out[lo:hi] = P[lo - dy:hi - dy]
    return np.roll(out, dx, axis=1)


def table_by_shifts(pred, truth, R, row_range=None):
    H, W = np.asarray(pred).shape
    row0, row1 = _band(H, row_range)
    assert R >= 1 and 2 * R + 1 <= W
    S = 2 * R + 1
    rows, pixels = np.zeros((2, S, S + 1), np.int64), np.zeros((2, 2), np.int64)
    for k, (P, T) in enumerate(zip(classes(pred), classes(truth))):
        pixels[k] = P.sum(), T[row0:row1].sum()
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                m = moved(P, dy, dx)[row0:row1]
                rows[k, dy + R, dx + R] = (m & T[row0:row1]).sum()
            rows[k, dy + R, S] = m.sum()
    return rows, pixels


def best_of(table, R):
    """(dy, dx, hits, kept[dy]) of one class's table: the most hits, then the smaller dy^2 + dx^2, then the smaller dy, then the smaller dx"""
    best = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            h = int(table[dy + R][dx + R])
            cand = (-h, dy * dy + dx * dx, dy, dx)
            if best is None or cand < best:
                best = cand
    dy, dx = best[2], best[3]
    return dy, dx, -best[0], int(table[dy + R][2 * R + 1])


def maxima_of(table, R):
    """the number of shifts that reach the table's largest hit count"""
    t = np.asarray(table)[:, :2 * R + 1]
    return int((t == t.max()).sum())


def batch_rows(pred, truth, R, row_range=None, algorithm=table_by_pairs):
    """(rows [n, 2, S, S + 1], pixels [n, 2, 2], best [n, 2, 4]) of n frames"""
    S = 2 * R + 1
    both = [algorithm(p, t, R, row_range) for p, t in zip(pred, truth)]
    rows = np.stack([b[0] for b in both]) if both else np.zeros((0, 2, S, S + 1), np.int64)
    pixels = np.stack([b[1] for b in both]) if both else np.zeros((0, 2, 2), np.int64)
    best = np.asarray([[best_of(r[k], R) for k in range(2)] for r in rows], np.int64).reshape(len(rows), 2, 4)
    return rows, pixels, best


def totals_of_rows(batches, R):
    """The state after the batches, each (rows [n, 2, S, S + 1], pixels [n, 2, 2], ...), on top of zeros -- what
    nn.DisplacementSkill.state() returns, as Python ints."""
    S = 2 * R + 1
    total = [[[0] * (S + 1) for _ in range(S)] for _ in range(2)]
    pix, frames = [[0, 0], [0, 0]], 0
    for batch in batches:
        rows, pixels = batch[0], batch[1]
        frames += len(rows)
        for b in range(len(rows)):
            for k in range(2):
                for c in range(2):
                    pix[k][c] += int(pixels[b, k, c])
                for i in range(S):
                    for j in range(S + 1):
                        total[k][i][j] += int(rows[b, k, i, j])
    return {"total": total, "pixels": pix, "frames": frames}


def _div(a, b):
    return None if b == 0 else a / b


def decode(total, pixels, frames, R, H, W, row_range=None):
    """the measures of nn.DisplacementSkill.decode, written independently"""
    row0, row1 = _band(H, row_range)
    N = int(frames) * (row1 - row0) * W
    S = 2 * R + 1
    out = {}
    for k in range(2):
        t = total[k]
        dy, dx, hits, kept = best_of(t, R)
        P, T = int(pixels[k][0]), int(pixels[k][1])
        h0, k0 = int(t[R][R]), int(t[R][S])
        e = {"pixels": {"predicted": P, "labelled": T}, "best": [dy, dx, hits, kept]}
        e["shift"] = {"rows": dy, "cols": dx, "pixels": math.sqrt(float(dy * dy + dx * dx)), "lat_deg": None if H < 2 else dy * 180.0 / (H - 1),
                      "lon_deg": None if W < 2 else dx * 360.0 / (W - 1)}
        e["at_edge"] = max(abs(dy), abs(dx)) == R
        e["hits_unshifted"], e["hits_shifted"] = h0, hits
        e["csi"] = {"unshifted": _div(h0, k0 + T - h0), "shifted": _div(hits, kept + T - hits)}
        e["pod"] = {"unshifted": _div(h0, T), "shifted": _div(hits, T)}
        e["far"] = {"unshifted": _div(k0 - h0, k0), "shifted": _div(kept - hits, kept)}
        if N == 0:
            for name in ("mse_total", "mse_shifted", "mse_displacement", "mse_volume", "mse_pattern"):
                e[name] = None
            e["share"] = {"displacement": None, "volume": None, "pattern": None}
        else:
            e["mse_total"] = (k0 + T - 2 * h0) / N
            e["mse_shifted"] = (kept + T - 2 * hits) / N
            e["mse_displacement"] = e["mse_total"] - e["mse_shifted"]
            e["mse_volume"] = ((kept - T) / N) ** 2
            e["mse_pattern"] = e["mse_shifted"] - e["mse_volume"]
            e["share"] = {n: _div(e[f"mse_{n}"], e["mse_total"]) for n in ("displacement", "volume", "pattern")}
        out[f"class_{k + 1}"] = e
    return out


def csi_surface(table, labelled, R):
    """float64 [S][S]: hits / (kept[dy] + labelled - hits), NaN where that is 0 / 0"""
    S = 2 * R + 1
    out = np.full((S, S), np.nan)
    for i in range(S):
        for j in range(S):
            union = int(table[i][S]) + int(labelled) - int(table[i][j])
            if union > 0:
                out[i, j] = int(table[i][j]) / union
    return out


def seam_hits(pred, truth, k, dy, dx, row_range=None):
    """the hits of class k under (dy, dx) whose predicted pixel lies on the other side of the seam: x - dx outside [0, W)"""
    P, T = classes(pred)[k - 1], classes(truth)[k - 1]
    H, W = P.shape
    row0, row1 = _band(H, row_range)
    hit = moved(P, dy, dx) & T
    hit[:row0], hit[row1:] = False, False
    x = np.nonzero(hit)[1]
    return int(((x - dx < 0) | (x - dx >= W)).sum())


# ---------------------------------------------------------------------------------------------------------------- the tests' masks
def ellipse(mask, cy, cx, a, b, value):
    """paints (y - cy)^2 / a^2 + dx^2 / b^2 <= 1, dx the periodic column difference; rows outside the frame are cut off"""
    H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W]
    d = (xx - cx) % W
    d = np.where(2 * d > W, d - W, d)
    mask[((yy - cy) * (yy - cy) * b * b + d * d * a * a) <= a * a * b * b] = value


def sparse_frames(n, H, W, R, seed):
    """(pred, truth, shifts) with uint8 [n, H, W] masks of ellipses, some 2 to 3 % of the pixels per class, and shifts [n][2] the planted
    (dy, dx): per class the prediction holds the labels' ellipses moved by (-dy, -dx), so that the labels meet the prediction moved by
    (dy, dx); the labels also hold a small ellipse the prediction misses, the prediction a small one of its own.  Class 1 of frame 0 has an
    ellipse on the seam; class 2 of frame 1 one whose copy on one side sits at the first row, class 1 of frame 2 one at the last row: a
    shift moves them over the pole.  The values 3 and 255 sit among the background of both masks."""
    rs = np.random.RandomState(seed)
    pred, truth = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.uint8)
    shifts = []
    amax, bmax = max(2, H // 14), max(4, W // 30)
    for f in range(n):
        frame_shifts = []
        for k in (1, 2):
            lo, hi = (0, H // 2) if k == 1 else (H // 2, H)                      # class 1 keeps to the upper half, class 2 to the lower
            my, mx = min(R, 4), min(R, 9)
            while True:
                dy, dx = int(rs.randint(-my, my + 1)), int(rs.randint(-mx, mx + 1))
                if dy != 0 and dx != 0:
                    break
            frame_shifts.append((dy, dx))
            objects = []
            area = 0
            while area < 0.022 * H * W or len(objects) < 2:
                a, b = int(rs.randint(1, amax + 1)), int(rs.randint(2, bmax + 1))
                objects.append((int(rs.randint(lo + a + my, max(lo + a + my + 1, hi - a - my))), int(rs.randint(0, W)), a, b))
                area += math.pi * a * b
            if f == 0 and k == 1:
                objects[0] = (objects[0][0], 0, objects[0][2], max(objects[0][3], 3))           # on the seam
            if f == 1 and k == 2:
                objects[0] = (max(dy, 0), objects[0][1], 1, objects[0][3])                       # one side's copy sits on row 0
            if f == 2 and k == 1:
                objects[0] = (H - 1 + min(dy, 0), objects[0][1], 1, objects[0][3])               # ... on row H - 1
            for cy, cx, a, b in objects:
                ellipse(truth[f], cy, cx, a, b, k)
                ellipse(pred[f], cy - dy, cx - dx, a, b, k)
            ellipse(truth[f], (lo + hi) // 2 + 1, int(rs.randint(0, W)), 1, 2, k)    # a small miss
            ellipse(pred[f], (lo + hi) // 2, int(rs.randint(0, W)), 1, 2, k)         # a small false alarm
        shifts.append(frame_shifts)
        for m in (truth[f], pred[f]):
            for value in (3, 255):
                for y, x in zip(rs.randint(0, H, 4), rs.randint(0, W, 4)):
                    if m[y, x] == 0:
                        m[y, x] = value
    return pred, truth, shifts


def dense_frames(n, H, W, seed):
    """uniform-random masks over {0, 1, 2, 3}"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 4, (n, H, W)).astype(np.uint8), rs.randint(0, 4, (n, H, W)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- the shapes and shared batches of the tests
B, NV = 4, 3
SHAPES = ("small", "word", "large", "large-r5")


@functools.lru_cache(maxsize=None)
def block():
    from mlperf_deepcam_amd import lib as _lib
    bits, rows = C.c_int(0), C.c_int(0)
    assert _lib.load().dc_displacement_block(C.byref(bits), C.byref(rows)) == 0 and bits.value > 1 and rows.value > 1
    return bits.value, rows.value


@functools.lru_cache(maxsize=None)
def shape(name):
    """(H, W, R) from the kernels' constants (64 pixels a word, 32 rows a segment: (23, 37, 18), (19, 128, 7), (141, 549, 40), (141, 549, 5)).
    "small" is narrower than a word and shorter than a segment, the window the whole ring; "word" two full words, no tail bits; "large"
    eight words and 37 tail bits, two waves of dx, four segments and a ragged fifth; "large-r5" the same frame with a small window."""
    bits, seg = block()
    if name == "small":
        W = bits - 27
        return seg - 9, W, (W - 1) // 2
    if name == "word":
        return seg - 13, 2 * bits, 7
    H, W = 4 * seg + 13, 8 * bits + 37
    return H, W, (min(63, bits // 2 + 8) if name == "large" else 5)


def bands(name):
    """full, interior, touching row 0, a single row"""
    H = shape(name)[0]
    return {"full": None, "interior": (3, H - 5), "top": (0, H // 2 + 1), "one-row": (H // 4, H // 4 + 1)}


def _seed(name):
    H, W, _ = shape(name)
    return 11 + H + W


@functools.lru_cache(maxsize=None)
def plain_batch(name, n=7):
    """n unmodified frames of sparse_frames with their planted shifts; "large" and "large-r5" share their frames.  Never modified."""
    H, W, R = shape(name)
    pred, truth, shifts = sparse_frames(n, H, W, min(R, 5) if name.startswith("large") else R, _seed(name))
    pred.setflags(write=False), truth.setflags(write=False)
    return pred, truth, shifts


TIE = (2, 5)                                          # row and column of the tie's labelled pixel in frame 1 of the standard batch


@functools.lru_cache(maxsize=None)
def standard_batch(name):
    """The standard batch of four with n_valid = 3: a plain frame; a frame whose class 1 is the tie alone -- one labelled pixel between two
    predicted ones in one row --; a frame whose prediction lacks class 2; and a padding frame, all class 1 on both sides, which would
    change every sum if read.  Shared and never modified."""
    pred, truth, _ = plain_batch(name)
    pred, truth = pred[:B].copy(), truth[:B].copy()
    pred[1][pred[1] == 1] = 0
    truth[1][truth[1] == 1] = 0
    y, x = TIE
    truth[1, y, x] = 1
    pred[1, y, x - 1] = pred[1, y, x + 1] = 1
    pred[2][pred[2] == 2] = 0
    pred[3], truth[3] = 1, 1
    pred.setflags(write=False), truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def reference(name, band="full", which="standard"):
    """(rows, pixels, best, state) of the standard batch's valid frames or of the plain batch, by table_by_pairs.  Never modified."""
    R = shape(name)[2]
    if which == "standard":
        pred, truth = (m[:NV] for m in standard_batch(name))
    else:
        pred, truth = plain_batch(name)[:2]
    out = batch_rows(pred, truth, R, bands(name)[band])
    for a in out:
        a.setflags(write=False)
    return out + (totals_of_rows([out], R),)
