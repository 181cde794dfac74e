"""A numpy checker for the scale-separation verification (dc_scale_score, nn.ScaleSkill), with two algorithms that share no code with the
kernels and little with each other, an exact decode, and the inputs the CPU and GPU tests share.
  rows_by_blocks     roll the frame by the origin, reshape the band into blocks of side 2^j, sum, square
  rows_by_transform  the explicit 2-D Haar components: block sums from an integral image of the (never rolled) band with modular column
                     indices, per level the field of detail coefficients 4 S_child - S_parent, whose sum of squares is 16 Q_j - 4 Q_{j+1},
                     and the father component; Q_j is recovered from the top down
Everything is a Python int or an int64; tests compare for equality."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

B, NV = 4, 3
# name -> (H, W, L, origins, {band name -> (row0, row1) or None}); the extents follow from the workgroup tile (test_scale_cpu asserts it)
SHAPES = {
    "partial": (12, 20, 2, (0, 1, 3), {"full": None}),
    "two-tiles": (40, 136, 3, (0, 5), {"full": None, "band": (8, 32)}),
    "tile": (64, 192, 6, (0, 17, 63), {"full": None}),
    "coarse": (320, 384, 7, (0, 100), {"band": (37, 293)}),
    "deep": (256, 512, 8, (0, 1, 63, 64, 255), {"full": None}),
}
CASES = [(name, band) for name, s in SHAPES.items() for band in s[4]]


def block():
    from mlperf_deepcam_amd import lib as L
    cols, rows = C.c_int(0), C.c_int(0)
    assert L.load().dc_scale_block(C.byref(cols), C.byref(rows)) == 0
    return cols.value, rows.value


def shape(name):
    return SHAPES[name][:4]


def band_of(name, band):
    H = SHAPES[name][0]
    r = SHAPES[name][4][band]
    return (0, H) if r is None else r


# ------------------------------------------------------------------------------------------------------------------ the two algorithms
def _sides(pred, truth, k):
    return (np.asarray(pred) == k).astype(np.int64), (np.asarray(truth) == k).astype(np.int64)


def rows_by_blocks(pred, truth, L, origins, band=None):
    """(rows int64 [2, O, L + 1, 3], pixels int64 [2, 2]) of one frame"""
    H, W = pred.shape
    r0, r1 = (0, H) if band is None else band
    rows, pixels = np.zeros((2, len(origins), L + 1, 3), np.int64), np.zeros((2, 2), np.int64)
    for k in (1, 2):
        f, o = (m[r0:r1] for m in _sides(pred, truth, k))
        pixels[k - 1] = f.sum(), o.sum()
        for i, c in enumerate(origins):
            fr, orr = np.roll(f, -c, axis=1), np.roll(o, -c, axis=1)           # the grid starts at column c
            for j in range(L + 1):
                n = 1 << j
                sf = fr.reshape((r1 - r0) // n, n, W // n, n).sum(axis=(1, 3))
                so = orr.reshape((r1 - r0) // n, n, W // n, n).sum(axis=(1, 3))
                rows[k - 1, i, j] = ((sf - so) ** 2).sum(), (sf ** 2).sum(), (so ** 2).sum()
    return rows, pixels


def _block_sums(field, c, n):
    """the sums of the blocks of side n of a band [R, W] on the grid that starts at column c, columns modulo W, from an integral image"""
    R, W = field.shape
    wide = np.concatenate([field, field], axis=1)                                # columns c .. c + W - 1 without a roll
    ii = np.zeros((R + 1, 2 * W + 1), np.int64)
    ii[1:, 1:] = wide.cumsum(0).cumsum(1)
    ys, xs = np.arange(0, R + 1, n), c + np.arange(0, W + 1, n)
    corner = ii[np.ix_(ys, xs)]
    return corner[1:, 1:] - corner[:-1, 1:] - corner[1:, :-1] + corner[:-1, :-1]


def rows_by_transform(pred, truth, L, origins, band=None):
    H, W = pred.shape
    r0, r1 = (0, H) if band is None else band
    rows, pixels = np.zeros((2, len(origins), L + 1, 3), np.int64), np.zeros((2, 2), np.int64)
    for k in (1, 2):
        f, o = (m[r0:r1] for m in _sides(pred, truth, k))
        pixels[k - 1] = int(np.count_nonzero(f)), int(np.count_nonzero(o))
        for i, c in enumerate(origins):
            for term, field in enumerate((f - o, f, o)):
                sums = [_block_sums(field, c, 1 << j) for j in range(L + 1)]
                q = [0] * (L + 1)
                q[L] = int((sums[L] ** 2).sum())                                 # the father component: 4^L times its energy
                for j in range(L - 1, -1, -1):
                    detail = 4 * sums[j] - np.kron(sums[j + 1], np.ones((2, 2), np.int64))      # 4^(j+1) times the component's field
                    g = int((detail ** 2).sum())                                 # = 16 Q_j - 4 Q_{j+1}
                    assert (g + 4 * q[j + 1]) % 16 == 0
                    q[j] = (g + 4 * q[j + 1]) // 16
                rows[k - 1, i, :, term] = q
    return rows, pixels


def haar_energies(field, c, L):
    """the energies of the explicit Haar components of a band [R, W] as Fractions: sum over the pixels of (mean over the block of side
    2^j - mean over the block of side 2^(j+1))^2 for j < L, and of the squared tile means for j = L -- computed on the pixel grid"""
    out, R, W = [], *field.shape
    rolled = np.roll(field, -c, axis=1)
    means = []
    for j in range(L + 1):
        n = 1 << j
        s = rolled.reshape(R // n, n, W // n, n).sum(axis=(1, 3))
        means.append(np.kron(s, np.ones((n, n), np.int64)) * (4 ** (L - j)))     # the field of block means, times 4^L
    for j in range(L):
        out.append(Fraction(int(((means[j] - means[j + 1]) ** 2).sum()), 16 ** L))
    out.append(Fraction(int((means[L] ** 2).sum()), 16 ** L))
    return out


def batch_rows(pred, truth, L, origins, band=None, algorithm=rows_by_blocks):
    got = [algorithm(p, t, L, origins, band) for p, t in zip(pred, truth)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def totals_of_rows(parts, L, O):
    """the state nn.ScaleSkill.state() must report after the calls whose (rows, pixels) are listed"""
    total = [[[[0, 0, 0] for _ in range(L + 1)] for _ in range(O)] for _ in range(2)]
    pixels, frames = [[0, 0], [0, 0]], 0
    for rows, px in parts:
        frames += len(rows)
        for r, p in zip(np.asarray(rows).tolist(), np.asarray(px).tolist()):
            for k in range(2):
                pixels[k] = [pixels[k][0] + int(p[k][0]), pixels[k][1] + int(p[k][1])]
                for o in range(O):
                    for j in range(L + 1):
                        total[k][o][j] = [a + int(b) for a, b in zip(total[k][o][j], r[k][o][j])]
    return {"total": total, "pixels": pixels, "frames": frames}


# ------------------------------------------------------------------------------------------------------------------ the exact decode
LISTS = ("mse", "mse_share", "skill", "energy_pred", "energy_truth", "energy_rel_diff")


def components(q):
    """E_j as the difference of the mean-square sums of neighbouring levels: Q_j / 4^j - Q_{j+1} / 4^(j+1); E_L = Q_L / 4^L"""
    L = len(q) - 1
    ms = [Fraction(int(q[j]), 4 ** j) for j in range(L + 1)]
    return [ms[j] - ms[j + 1] for j in range(L)] + [ms[L]]


def _f(v):
    return None if v is None else float(v)


def decode(total, pixels, frames, L, rows_in_band, width, origins=None):
    N = frames * rows_in_band * width
    out = {}
    for k in range(2):
        O = len(total[k])
        names = list(range(O)) if origins is None else list(origins)
        P, T = int(pixels[k][0]), int(pixels[k][1])
        rnd = None
        if N:
            p, o = Fraction(P, N), Fraction(T, N)
            rnd = p * (1 - o) + o * (1 - p)
        per = []
        for oi in range(O):
            e = [components([total[k][oi][j][t] for j in range(L + 1)]) for t in range(3)]
            a0 = int(total[k][oi][0][0])
            per.append({"mse": [Fraction(x) / N if N else None for x in e[0]], "mse_share": [x / a0 if a0 else None for x in e[0]],
                        "energy_pred": [x / N if N else None for x in e[1]], "energy_truth": [x / N if N else None for x in e[2]]})
        mean = {n: [None if per[0][n][j] is None else Fraction(sum(q[n][j] for q in per), O) for j in range(L + 1)] for n in per[0]}
        for entry in per + [mean]:
            entry["skill"] = [None if (rnd is None or rnd == 0) else 1 - (L + 1) * m / rnd for m in entry["mse"]]
            entry["energy_rel_diff"] = [None if (a is None or a + b == 0) else (a - b) / (a + b)
                                        for a, b in zip(entry["energy_pred"], entry["energy_truth"])]
        skilful = None
        for j in range(L):
            if all(mean["skill"][i] is not None and mean["skill"][i] > 0 for i in range(j, L)):
                skilful = 1 << j
                break
        entry = {"pixels": {"predicted": P, "labelled": T}, "base_rate": _f(Fraction(T, N)) if N else None,
                 "bias": _f(Fraction(P, T)) if T else None, "mse_random": _f(rnd), "scales": [2 ** j for j in range(L + 1)]}
        for n in LISTS:
            entry[n] = [_f(v) for v in mean[n]]
        entry["by_origin"] = [dict([("origin", c)] + [(n, [_f(v) for v in q[n]]) for n in LISTS]) for c, q in zip(names, per)]
        entry["origin_spread"] = [_f(max(q["mse"][j] for q in per) - min(q["mse"][j] for q in per)) if N else None for j in range(L + 1)]
        entry["skilful_scale"] = skilful
        out[f"class_{k + 1}"] = entry
    return out


# ------------------------------------------------------------------------------------------------------------------ the shared inputs
def ellipse(mask, cy, cx, ry, rx, value):
    """an ellipse of `value`, columns periodic, rows clipped"""
    H, W = mask.shape
    y, x = np.mgrid[0:H, 0:W]
    dx = np.minimum((x - cx) % W, (cx - x) % W)
    mask[((y - cy) / ry) ** 2 + (dx / rx) ** 2 <= 1.0] = value


def sparse_frames(n, H, W, seed):
    """n frames of sparse ellipses: the labels, and a prediction that holds them displaced by a few pixels, with objects of its own and a
    little speckle, so that every level of either class carries error"""
    rs = np.random.RandomState(seed)
    pred, truth = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.uint8)
    for f in range(n):
        for k in (1, 2):
            for _ in range(3):
                cy, cx = rs.randint(0, H), rs.randint(0, W)
                ry, rx = 1 + rs.rand() * max(1.0, H / 8), 1 + rs.rand() * max(1.0, W / 10)
                ellipse(truth[f], cy, cx, ry, rx, k)
                ellipse(pred[f], cy + rs.randint(-2, 3), cx + rs.randint(-3, 4), ry * (0.7 + 0.6 * rs.rand()), rx, k)
            ellipse(pred[f], rs.randint(0, H), rs.randint(0, W), 1.5, 2.5, k)    # an object of its own
        speck = rs.rand(H, W) < 0.01
        pred[f][speck] = rs.randint(0, 3, size=int(speck.sum()))
        truth[f][rs.rand(H, W) < 0.005] = 3                                      # a value that is background
    return pred, truth


@functools.lru_cache(maxsize=None)
def standard_batch(name):
    """B = 4 frames of which NV = 3 are valid: sparse ellipses with a displaced prediction; class 2 absent from the prediction and class
    1 from the labels; an ellipse across the seam on both sides; and a padding frame full of class 1 that changes every sum if read"""
    H, W, L, origins = shape(name)
    pred, truth = sparse_frames(B, H, W, 11 + H)
    pred[1][pred[1] == 2] = 0
    truth[1][truth[1] == 1] = 0
    ellipse(truth[2], H // 2, 0, max(2.0, H / 6), max(3.0, W / 12), 1)
    ellipse(pred[2], H // 2 + 1, W - 1, max(2.0, H / 6), max(3.0, W / 12), 1)
    pred[3], truth[3] = 1, 1
    pred.flags.writeable = truth.flags.writeable = False
    return pred, truth


@functools.lru_cache(maxsize=None)
def plain_batch(name):
    """seven valid frames, for the cut into batches"""
    H, W, L, origins = shape(name)
    pred, truth = sparse_frames(7, H, W, 5 + W)
    pred.flags.writeable = truth.flags.writeable = False
    return pred, truth


@functools.lru_cache(maxsize=None)
def full_batch(name):
    """two frames: class 1 everywhere on both sides; class 1 everywhere in the prediction and class 2 everywhere in the labels.  On a
    256 x 256 block a sum is 2^16 and a square 2^32"""
    H, W, L, origins = shape(name)
    pred, truth = np.ones((2, H, W), np.uint8), np.ones((2, H, W), np.uint8)
    truth[1] = 2
    pred.flags.writeable = truth.flags.writeable = False
    return pred, truth


@functools.lru_cache(maxsize=None)
def reference(name, band, kind="standard"):
    """(rows, pixels, state) of the valid frames of a shared batch, computed once"""
    H, W, L, origins = shape(name)
    pred, truth = {"standard": standard_batch, "plain": plain_batch, "full": full_batch}[kind](name)
    n = NV if kind == "standard" else len(pred)
    rows, pixels = batch_rows(pred[:n], truth[:n], L, origins, SHAPES[name][4][band])
    rows.flags.writeable = pixels.flags.writeable = False
    return rows, pixels, totals_of_rows([(rows, pixels)], L, len(origins))
