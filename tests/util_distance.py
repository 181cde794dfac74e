"""Checker of the distance-map verification (nn.DistanceSkill, dc_distance_score): the definition of include/deepcam_hip.h in numpy and
Python ints, with no knowledge of the kernels' separable passes, strips, segments, packed words or histograms.  NOT separable: per frame,
side and class it lists the coordinates of the class's pixels and takes, for every pixel of the frame, the minimum of dy^2 + dx^2 over
that list by broadcasting (in chunks of pixels); then it applies the cap.

d^2((y, x), (y', x')) = (y - y')^2 + dx^2, dx = min(|x - x'|, W - |x - x'|) with wrap and |x - x'| without; rows are never periodic.  The map
value is the minimum where that is <= R^2 and R^2 + 1 ("beyond") otherwise, also when the class has no pixel.  ring(v) is the smallest j
with j^2 >= v, dq(v) = rint(sqrt(v) * 256) in float64.  Direction 0 ("miss") takes the labelled pixels as sources and the distance to the
nearest predicted pixel, direction 1 ("false alarm") the reverse.  rows[b][k - 1][direction] = the sources per ring 0 .. R + 1 (R + 1:
beyond), then sum dq and sum d^2 over the sources within the cap; baddeley[b][k - 1] = sum over pixels of (w_P - w_T)^2, w = dq within the
cap and 256 R beyond.  Only sources and Baddeley pixels in the rows row0 <= i < row1 count."""
import ctypes as C
import functools
import math

import numpy as np


def classes(mask):
    """the two indicator fields of a mask of integers of any width: only the full-width values 1 and 2 are classes"""
    m = np.asarray(mask).astype(np.int64)
    return [m == 1, m == 2]


def distance_map(ind, R, wrap, chunk=4096):
    """int64 [H, W]: per pixel min over the pixels of `ind` (bool [H, W]) of dy^2 + dx^2, capped at R^2 + 1"""
    ind = np.asarray(ind, bool)
    H, W = ind.shape
    assert R >= 1 and (not wrap or 2 * R + 1 <= W)
    cap = R * R + 1
    out = np.full(H * W, cap, np.int64)
    ys, xs = np.nonzero(ind)
    if len(ys) == 0:
        return out.reshape(H, W)
    ys, xs = ys.astype(np.int64)[None, :], xs.astype(np.int64)[None, :]
    py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
    for s in range(0, H * W, chunk):
        dy = py[s:s + chunk, None] - ys
        dx = np.abs(px[s:s + chunk, None] - xs)
        if wrap:
            dx = np.minimum(dx, W - dx)
        out[s:s + chunk] = (dy * dy + dx * dx).min(axis=1)
    return np.minimum(out, cap).reshape(H, W)


def frame_maps(pred, truth, R, wrap=True):
    """int64 [2 sides, 2 classes, H, W]: side 0 the prediction, side 1 the labels"""
    return np.stack([np.stack([distance_map(f, R, wrap) for f in classes(side)]) for side in (pred, truth)])


def ring_of(v):
    j = math.isqrt(int(v))
    return j + (j * j < int(v))


def dq_of(v):
    return int(np.rint(np.sqrt(np.float64(v)) * 256))


def table(R):
    """(ring [R^2 + 2], dq [R^2 + 2]) as int64 arrays; the last entry is beyond: ring R + 1, dq 0"""
    ring = np.asarray([ring_of(v) for v in range(R * R + 1)] + [R + 1], np.int64)
    dq = np.asarray([dq_of(v) for v in range(R * R + 1)] + [0], np.int64)
    return ring, dq


def rows_from_maps(maps, R, row_range=None):
    """(int64 [2, 2, R + 4], int64 [2]) of one frame from its maps [2, 2, H, W]"""
    H, W = maps.shape[2:]
    row0, row1 = (0, H) if row_range is None else row_range
    assert 0 <= row0 < row1 <= H
    ring, dq = table(R)
    cap = R * R + 1
    rows = np.zeros((2, 2, R + 4), np.int64)
    baddeley = np.zeros(2, np.int64)
    band = maps[:, :, row0:row1]
    for k in range(2):
        dP, dT = band[0, k], band[1, k]
        w = [np.where(d >= cap, 256 * R, dq[d]) for d in (dP, dT)]
        baddeley[k] = ((w[0] - w[1]) ** 2).sum()
        for direction, (own, other) in enumerate(((dT, dP), (dP, dT))):      # miss: labelled sources; false alarm: predicted sources
            d2 = other[own == 0]
            rows[k, direction, :R + 2] = np.bincount(ring[d2], minlength=R + 2)
            near = d2[d2 < cap]
            rows[k, direction, R + 2] = dq[near].sum()
            rows[k, direction, R + 3] = near.sum()
    return rows, baddeley


def frame_rows(pred, truth, R, wrap=True, row_range=None):
    return rows_from_maps(frame_maps(pred, truth, R, wrap), R, row_range)


def batch_rows(pred, truth, R, wrap=True, row_range=None):
    """(int64 [n, 2, 2, R + 4], int64 [n, 2]) of n frames"""
    both = [frame_rows(p, t, R, wrap, row_range) for p, t in zip(pred, truth)]
    return (np.stack([b[0] for b in both]) if both else np.zeros((0, 2, 2, R + 4), np.int64),
            np.stack([b[1] for b in both]) if both else np.zeros((0, 2), np.int64))


def totals_of_rows(batches, R):
    """The state after the batches, each (rows [n, 2, 2, R + 4], baddeley [n, 2]), on top of zeros -- what nn.DistanceSkill.state()
    returns: total [2][2][R + 4] and baddeley [2] as Python ints, frames."""
    total = [[[0] * (R + 4) for _ in range(2)] for _ in range(2)]
    bad, frames = [0, 0], 0
    for rows, baddeley in batches:
        frames += len(rows)
        for b in range(len(rows)):
            for k in range(2):
                bad[k] += int(baddeley[b, k])
                for d in range(2):
                    for c in range(R + 4):
                        total[k][d][c] += int(rows[b, k, d, c])
    return {"total": total, "baddeley": bad, "frames": frames}


def totals(batches, R, wrap=True, row_range=None):
    """the same from the masks: batches of (pred [n, H, W], truth [n, H, W])"""
    return totals_of_rows([batch_rows(p, t, R, wrap, row_range) for p, t in batches], R)


def decode(total, total_baddeley, frames, R, H, W, row_range=None):
    """the measures of nn.DistanceSkill.decode, written independently"""
    row0, row1 = (0, H) if row_range is None else row_range
    cells = int(frames) * (row1 - row0) * W
    out = {}
    for k in range(2):
        e = {}
        quant, top, any_beyond, count = [], -1, False, []
        for d, (name, curve) in enumerate((("miss", "pod_within"), ("false_alarm", "success_within"))):
            cell = [int(v) for v in total[k][d]]
            n = sum(cell[:R + 2])
            count.append(n)
            inside = n - cell[R + 1]
            e[curve] = [None if n == 0 else sum(cell[:r + 1]) / n for r in range(R + 1)]
            e[f"med_{name}"] = None if inside == 0 else cell[R + 2] / 256 / inside
            e[f"rms_{name}"] = None if inside == 0 else math.sqrt(cell[R + 3] / inside)
            e[f"beyond_{name}"] = None if n == 0 else cell[R + 1] / n
            any_beyond |= cell[R + 1] > 0
            top = max([top] + [j for j in range(R + 1) if cell[j]])
            if n:
                run = 0
                for j in range(R + 2):
                    run += cell[j]
                    if 10 * run >= 9 * n:
                        quant.append(j)
                        break
        e["pixels"] = {"labelled": count[0], "predicted": count[1]}
        e["hausdorff"] = None if any_beyond or top < 0 else top
        e["hausdorff_q90"] = None if not quant or max(quant) > R else max(quant)
        e["baddeley"] = None if cells == 0 else math.sqrt(int(total_baddeley[k]) / cells) / 256
        out[f"class_{k + 1}"] = e
    return out


# ---------------------------------------------------------------------------------------------------------------- the tests' masks
def _disc(mask, cy, cx, r, value, wrap_cols=True):
    H, W = mask.shape
    for y in range(max(0, cy - r), min(H, cy + r + 1)):
        for x in range(cx - r, cx + r + 1):
            if (y - cy) ** 2 + (x - cx) ** 2 <= r * r and (wrap_cols or 0 <= x < W):
                mask[y, x % W] = value


def _rect(mask, y0, x0, h, w, value):
    H, W = mask.shape
    for y in range(max(0, y0), min(H, y0 + h)):
        for x in range(x0, x0 + w):
            mask[y, x % W] = value


def sparse_masks(n, H, W, R, seed):
    """(pred, truth) uint8 [n, H, W], sparse.  Class 1 keeps to the upper half of the rows and class 2 to the lower.  Per class and frame
    the labels hold a rectangle on row 0 (class 1) or row H - 1 (class 2), a rectangle across the seam, a few jittered rectangles and discs
    in the left half of the columns and one rectangle displaced by three columns only; the prediction is the copy displaced by R // 2 + 2
    to R // 2 + 5 columns (the seam object by one row), so that the rings above R / 2 fill.  Where the frame is wide enough a labelled
    object is missing from the prediction and a predicted speck from the labels, each more than R columns from everything of its class:
    beyond.  A labelled speck in column 2 has its nearest predicted pixel in column W - 1: across the seam with wrap, elsewhere or nowhere
    without.  The values 3 and 255 sit among the background of both masks."""
    rs = np.random.RandomState(seed)
    pred, truth = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.uint8)
    wide = W >= 6 * R + 64
    for b in range(n):
        t, p = truth[b], pred[b]
        for k in (1, 2):
            lo, hi = (0, H // 2) if k == 1 else (H // 2, H)
            mid = (lo + hi) // 2
            S = R // 2 + 2 + int(rs.randint(0, 4)) if wide else 2
            edge = 0 if k == 1 else H - 2
            _rect(t, edge, W // 3 + 7 * k, 2, 5, k)
            _rect(p, edge, W // 3 + 7 * k + S, 2, 5, k)
            _rect(t, mid, W - 2, 2, 4, k)                                      # columns W - 2, W - 1, 0, 1
            _rect(p, mid + 1, W - 2, 2, 4, k)
            t[lo + 4, 2] = k                                                   # the pair across the seam, three columns apart
            p[lo + 4, W - 1] = k
            for cx in ((W // 8, W // 4, W // 2) if wide else (W // 2,)):
                cy, cx = int(rs.randint(lo + 6, hi - 6)) if hi - lo > 14 else mid, cx + int(rs.randint(-5, 6)) * wide
                dy = int(rs.randint(-2, 3))
                if rs.rand() < 0.5:
                    r = int(rs.randint(1, 4)) if wide else 1
                    _disc(t, cy, cx, r, k)
                    _disc(p, cy + dy, cx + S, r, k)
                else:
                    h, w = int(rs.randint(1, 4)), int(rs.randint(2, 8)) if wide else 2
                    _rect(t, cy, cx, h, w, k)
                    _rect(p, cy + dy, cx + S, h, w, k)
            if wide:
                _rect(t, mid - 8, 3 * W // 8, 2, 3, k)                         # displaced by three columns only
                _rect(p, mid - 8, 3 * W // 8 + 3, 2, 3, k)
                _rect(t, mid + 6, (85 * W) // 100, 2, 3, k)                    # missing from the prediction
                p[mid - 5, (69 * W) // 100] = k                                # a stray speck
        for m in (t, p):
            for value in (3, 255):
                for y, x in zip(rs.randint(0, H, 12), rs.randint(0, W, 12)):
                    if m[y, x] == 0:
                        m[y, x] = value
    return pred, truth


# ------------------------------------------------------------------------------------------------- the shapes and shared batches of the tests
B, NV = 3, 2


@functools.lru_cache(maxsize=None)
def block():
    from mlperf_deepcam_amd import lib as _lib
    cols, rows = C.c_int(0), C.c_int(0)
    assert _lib.load().dc_distance_block(C.byref(cols), C.byref(rows)) == 0 and cols.value > 1 and rows.value > 1
    return cols.value, rows.value


@functools.lru_cache(maxsize=None)
def shape(name):
    """(H, W, R): "small" is narrower than a strip and shorter than a segment, of odd width, the window the whole ring; "large" has a
    ragged last strip and a ragged last segment and a halo longer than a segment where the cap allows it; "large-r5" the same frame at R = 5"""
    TC, TR = block()
    if name == "small":
        W = min(TC - 1, 37)
        W -= W % 2 == 0
        H = min(TR - 1, 23)
        assert W % 2 == 1 and 0 < W < TC and 0 < H < TR
        return H, W, (W - 1) // 2
    W, H = 2 * TC + 37, 2 * TR + 13
    return H, W, (min(127, TR + 2) if name == "large" else 5)


@functools.lru_cache(maxsize=None)
def standard_batch(name):
    """The standard batch of three: a frame whose prediction lacks class 1 (all its labelled pixels of class 1 are beyond); a frame without
    class 1 on either side (zero rows); and a padding frame, all class 1 on both sides, behind n_valid = 2.  Shared and never modified."""
    H, W, R = shape(name)
    pred, truth = sparse_masks(B, H, W, R, 60 + H + R)
    pred[0][pred[0] == 1] = 0
    pred[1][pred[1] == 1] = 0
    truth[1][truth[1] == 1] = 0
    pred[2], truth[2] = 1, 1
    pred.setflags(write=False), truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def plain_batch(name, n=7):
    """n unmodified frames of sparse_masks: both classes on both sides in every frame.  Shared and never modified."""
    H, W, R = shape(name)
    pred, truth = sparse_masks(n, H, W, R, 7 + R)
    pred.setflags(write=False), truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def reference_maps(name, wrap, which="standard"):
    """int64 [n, 2, 2, H, W] of the standard batch's valid frames or of the plain batch.  Shared and never modified."""
    pred, truth = standard_batch(name) if which == "standard" else plain_batch(name)
    n = NV if which == "standard" else len(pred)
    maps = np.stack([frame_maps(pred[b], truth[b], shape(name)[2], wrap) for b in range(n)])
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def reference(name, wrap, row_range=None, which="standard"):
    """(rows [n, 2, 2, R + 4], baddeley [n, 2], state)"""
    R = shape(name)[2]
    both = [rows_from_maps(m, R, row_range) for m in reference_maps(name, wrap, which)]
    rows, bad = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    rows.setflags(write=False), bad.setflags(write=False)
    return rows, bad, totals_of_rows([(rows, bad)], R)
