"""Checker of the mask morphology (nn.MaskMorphology; dc_mask_morph): the header's text restated on byte arrays with padding, no bits
packed and no code shared with the library, and the masks its tests use."""
import numpy as np

N4 = [(-1, 0), (1, 0), (0, -1), (0, 1)]
N8 = N4 + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def shifts(x, offs, wrap, pad):
    """x moved by every offset: rows outside the frame are `pad`, columns too unless wrap"""
    H, W = x.shape
    p = np.pad(x, 1, constant_values=pad)
    if wrap:
        p[1:-1, 0], p[1:-1, -1] = x[:, -1], x[:, 0]
    return [p[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] for dr, dc in offs]


def octagon(x, r, wrap, dilate):
    """DILATE r or ERODE r: N4 shifts on odd steps, N8 on even ones; what lies outside is background for DILATE, foreground for ERODE"""
    for j in range(1, r + 1):
        x = (np.logical_or if dilate else np.logical_and).reduce([x] + shifts(x, N4 if j % 2 else N8, wrap, not dilate))
    return x


def grow(seed, inside, offs, wrap):
    """everything of `inside` connected to seed (a subset of it): grow by one pixel until nothing changes"""
    while True:
        new = inside & np.logical_or.reduce([seed] + shifts(seed, offs, wrap, False))
        if (new == seed).all():
            return seed
        seed = new


def fill(x, wrap):
    c = ~x
    marker = np.zeros_like(x)
    marker[0] = marker[-1] = True
    if not wrap:
        marker[:, 0] = marker[:, -1] = True
    return x | (c & ~grow(c & marker, c, N4, wrap))


def run_plane(x, steps, wrap):
    orig = x
    for step in steps:
        x = {"dilate": lambda: octagon(x, step[1], wrap, True), "erode": lambda: octagon(x, step[1], wrap, False),
             "fill": lambda: fill(x, wrap), "reconstruct": lambda: grow(x & orig, orig, N8, wrap)}[step[0]]()
    return x


def morph(mask, steps_1, steps_2, wrap):
    """(out uint8 [B, H, W], counts int64 [B, 2, 4], ran bool [2, 8]: the steps that propagate) of masks [B, H, W] of any integers"""
    out, counts = np.zeros(mask.shape, np.uint8), np.zeros((len(mask), 2, 4), np.int64)
    for b, m in enumerate(mask):
        x1, x2 = run_plane(m == 1, steps_1, wrap), run_plane(m == 2, steps_2, wrap)
        o = np.where(m >= 3, m, np.where((m == 1) & x1, 1, np.where((m == 2) & x2, 2, np.where(x1, 1, np.where(x2, 2, 0)))))
        out[b] = o
        counts[b] = [[(m == k).sum(), (o == k).sum(), ((o == k) & (m != k)).sum(), ((m == k) & (o != k)).sum()] for k in (1, 2)]
    ran = np.zeros((2, 8), bool)
    for k, steps in enumerate((steps_1, steps_2)):
        ran[k, :len(steps)] = [s[0] in ("fill", "reconstruct") for s in steps]
    return out, counts, ran


def noise_mask(H, W, nb, seed):
    """thresholded smoothed noise: blobs with holes, gaps and specks of both classes"""
    f = np.random.RandomState(seed).rand(nb, H, W)
    for _ in range(2):
        f = sum(np.roll(np.roll(f, dr, 1), dc, 2) for dr in (-1, 0, 1) for dc in (-1, 0, 1)) / 9.0
    lo, hi = np.quantile(f, 0.2), np.quantile(f, 0.75)
    return np.where(f > hi, 1, np.where(f < lo, 2, 0)).astype(np.uint8)


def spiral_mask(H, W):
    """[2, H, W]: frame 0 is class 1 everywhere but a one-pixel-wide spiral corridor that opens on row 0 (nothing of it is a hole);
    frame 1 is that spiral as a class 2 line, joined along row 0 to a 5 x 5 block (what an erosion by 2 leaves a seed in)"""
    w, D = W - 8, [(0, 1), (1, 0), (0, -1), (-1, 0)]
    p = np.zeros((H, w), bool)
    p[0, 1] = p[1, 1] = True
    r, c, d = 1, 1, 0
    free = lambda r, c, d: 1 <= r + D[d][0] < H - 1 and 1 <= c + D[d][1] < w - 1 and not p[r + D[d][0], c + D[d][1]] \
        and not p[min(max(r + 2 * D[d][0], 0), H - 1), min(max(c + 2 * D[d][1], 0), w - 1)]  # noqa: E731
    while True:
        if free(r, c, d):
            r, c = r + D[d][0], c + D[d][1]
            p[r, c] = True
        elif free(r, c, (d + 1) % 4):
            d = (d + 1) % 4
        else:
            break
    path = np.pad(p, ((0, 0), (8, 0)))
    line = path.copy()
    line[0:5, 1:6] = line[0, 6:10] = True
    return np.stack([np.where(path, 0, 1), np.where(line, 2, 0)]).astype(np.uint8)
