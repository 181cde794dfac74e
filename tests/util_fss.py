"""Checker of the neighbourhood verification (nn.FractionsSkill, dc_fss_score): the definition of include/deepcam_hip.h in numpy on int64
and Python ints, through integral images of a padded frame, with no knowledge of the kernel's strips, segments, packed words or slab.

For frame b, class k in {1, 2} and a window of n = 2 r + 1 pixels a side: F(i, j) = the number of pixels of pred[b] == k in the n x n window
centred on (i, j), O(i, j) the same of truth[b]; rows outside [0, H) count nothing, columns are taken modulo W with wrap and count nothing
outside [0, W) without.  rows[b][k - 1][s] = (sum (F - O)^2, sum F^2, sum O^2) over row0 <= i < row1 and all j; pixels[b][k - 1] = (# pred ==
k, # truth == k) over the same rows.  The totals are the sums over all frames as Python ints; fss = 1.0 - A / (B + C) by true division of
the exact integers, None where B + C == 0."""
import numpy as np


def box_counts(ind, n, wrap):
    """int64 [H, W]: per pixel the sum of `ind` (bool or integer [H, W]) over the n x n window centred on it"""
    ind = np.asarray(ind).astype(np.int64)
    H, W = ind.shape
    assert n % 2 == 1 and n >= 1 and (not wrap or n <= W)
    r = (n - 1) // 2
    if wrap:
        wide = np.concatenate([ind[:, W - r:], ind, ind[:, :r]], axis=1)
    else:
        wide = np.pad(ind, ((0, 0), (r, r)))
    wide = np.pad(wide, ((r, r), (0, 0)))                               # the poles: zeros
    assert wide.shape == (H + 2 * r, W + 2 * r)
    integral = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    integral[1:, 1:] = np.cumsum(np.cumsum(wide, axis=0), axis=1)
    out = integral[n:, n:] - integral[:-n, n:] - integral[n:, :-n] + integral[:-n, :-n]
    assert out.shape == (H, W)
    return out


def classes(mask):
    """the two indicator fields of a mask of integers of any width: only the values 1 and 2 are classes"""
    m = np.asarray(mask).astype(np.int64)
    return [m == 1, m == 2]


def frame_rows(pred, truth, windows, wrap=True, row_range=None):
    """(int64 [2, S, 3], int64 [2, 2]) of one frame"""
    H, W = np.asarray(pred).shape
    row0, row1 = (0, H) if row_range is None else row_range
    assert 0 <= row0 < row1 <= H
    rows = np.zeros((2, len(windows), 3), np.int64)
    pixels = np.zeros((2, 2), np.int64)
    for k, (p, t) in enumerate(zip(classes(pred), classes(truth))):
        pixels[k] = [p[row0:row1].sum(), t[row0:row1].sum()]
        for s, n in enumerate(windows):
            F = box_counts(p, n, wrap)[row0:row1]
            O = box_counts(t, n, wrap)[row0:row1]
            rows[k, s] = [((F - O) ** 2).sum(), (F * F).sum(), (O * O).sum()]
    return rows, pixels


def batch_rows(pred, truth, windows, wrap=True, row_range=None):
    """(int64 [n, 2, S, 3], int64 [n, 2, 2]) of n frames"""
    both = [frame_rows(p, t, windows, wrap, row_range) for p, t in zip(pred, truth)]
    S = len(windows)
    return (np.stack([b[0] for b in both]) if both else np.zeros((0, 2, S, 3), np.int64),
            np.stack([b[1] for b in both]) if both else np.zeros((0, 2, 2), np.int64))


def totals(batches, windows, wrap=True, row_range=None):
    """The state after the batches, each (pred [n, H, W], truth [n, H, W]), on top of zeros: total [2][S][3] as Python ints, pixels
    [2][2] and frames as ints -- what nn.FractionsSkill.state() returns."""
    S = len(windows)
    total = [[[0, 0, 0] for _ in range(S)] for _ in range(2)]
    pixels = [[0, 0], [0, 0]]
    frames = 0
    for pred, truth in batches:
        rows, px = batch_rows(pred, truth, windows, wrap, row_range)
        frames += len(rows)
        for b in range(len(rows)):
            for k in range(2):
                for s in range(S):
                    for t in range(3):
                        total[k][s][t] += int(rows[b, k, s, t])
                for side in range(2):
                    pixels[k][side] += int(px[b, k, side])
    return {"total": total, "pixels": pixels, "frames": frames}


def fss(a, b, c):
    a, b, c = int(a), int(b), int(c)
    return None if b + c == 0 else 1.0 - a / (b + c)


def decode(total, pixels, frames, windows, rows, width):
    """per class the pooled scores, the base rate of the labels in the scored band, the useful score and the smallest skilful window"""
    out = {}
    cells = int(frames) * int(rows) * int(width)
    for k in range(2):
        scores = [fss(*total[k][s]) for s in range(len(windows))]
        base = int(pixels[k][1]) / cells if cells else None
        useful = None if base is None else 0.5 + base / 2
        skilful = None
        for n, f in sorted(zip(windows, scores)):
            if useful is not None and f is not None and f >= useful:
                skilful = int(n)
                break
        out[f"class_{k + 1}"] = {"fss": scores, "base_rate": base, "useful": useful, "skilful_window": skilful}
    return out
