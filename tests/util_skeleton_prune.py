"""Checker of spur pruning (dc_skeleton_prune; nn.EventAxis(prune=)) and of the filter's axis criterion (dc_event_select_axis), and the
drawn inputs their tests use.  prune_plane() is the header's text on rolled Boolean arrays: no bits are packed, no words exist."""
import numpy as np

RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # P2 .. P9, clockwise from north


def ring(s, wrap):
    """the eight neighbour planes of the bool plane s"""
    H, W = s.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = s
    if wrap:
        p[1:-1, 0], p[1:-1, -1] = s[:, -1], s[:, 0]
    return [p[1 + dr:H + 1 + dr, 1 + dc:W + 1 + dc] for dr, dc in RING]


def endpoints(s, wrap):
    """(E(s), isolated pixels of s, pixels with a backward neighbour)"""
    p = ring(s, wrap)
    count = sum(x.astype(np.int32) for x in p)
    pair = np.zeros_like(s)
    for j in range(8):
        pair |= p[j] & p[(j + 1) % 8]
    return s & ((count == 1) | ((count == 2) & pair)), s & (count == 0), p[6] | p[7] | p[0] | p[1]     # backward: P8, P9, P2, P3


def shrink_plane(s, wrap, spur):
    """X1: the plane after the shrink rounds"""
    s = np.asarray(s, bool)
    for _ in range(spur):
        e, _, back = endpoints(s, wrap)
        a = e & back
        s1 = s & ~a
        b = (e & ~a) & np.logical_or.reduce(ring(s1, wrap))
        if not (a.any() or b.any()):
            break
        s = s1 & ~b
    return s


def prune_plane(x0, wrap, spur):
    x0 = np.asarray(x0, bool)
    s = shrink_plane(x0, wrap, spur)
    d = x0 & ~s
    e, alone, _ = endpoints(s, wrap)
    g = e | alone
    for _ in range(spur):
        add = np.logical_or.reduce(ring(g, wrap)) & d & ~g
        if not add.any():
            break
        g = g | add
    return s | g


def prune(skel, n_valid, wrap, spur):
    """skel uint8 [B, H, W] -> (pruned uint8 [n_valid, H, W], removed int32 [n_valid, 2])"""
    skel = np.asarray(skel)
    out, removed = np.zeros((n_valid,) + skel.shape[1:], np.uint8), np.zeros((n_valid, 2), np.int32)
    for b in range(n_valid):
        for k in (1, 2):
            kept = prune_plane(skel[b] == k, wrap, spur)
            out[b][kept] = k
            removed[b, k - 1] = int((skel[b] == k).sum() - kept.sum())
    return out, removed


def select_axis(table, ncomp, axis_rows, min_m, keep, counts):
    """the numpy loop of dc_event_select_axis on copies: (keep, counts)"""
    keep, counts = keep.copy(), counts.copy()
    cap = table.shape[1]
    for b in range(len(table)):
        for k in range(min(max(int(ncomp[b, 0]), 0), cap)):
            cls = int(table[b, k, 1])
            if cls in (1, 2) and keep[b, k] and min_m[cls - 1] > 0 and axis_rows[b, k, 6] < min_m[cls - 1]:
                keep[b, k] = 0
                counts[b, cls - 1, 0] -= 1
                counts[b, cls - 1, 1] += 1
    return keep, counts


def _line(m, r0, c0, dr, dc, n, cls=1):
    for j in range(n):
        m[(r0 + j * dr), (c0 + j * dc) % m.shape[1]] = cls


def drawn(name, H, W):
    """uint8 [H, W], H >= 8 and W >= 64: the hand-drawn inputs.  `spurs`: a course from column 2 to W - 3 that steps down a row behind
    columns 20 and 40, as a thinned course does where a branch leaves it; SPUR_2 (2 pixels) leaves the first step, SPUR_7 the second."""
    m = np.zeros((H, W), np.uint8)
    if name == "spurs":
        _line(m, 5, 2, 0, 1, 19)
        _line(m, 6, 21, 0, 1, 20)
        _line(m, 7, 41, 0, 1, W - 43)
        for r, c in SPUR_2 + SPUR_7:
            m[r, c] = 1
    elif name == "two":
        m[3, 10:12] = 1
    elif name == "single":
        m[3, 10] = 2
    elif name == "ring":
        m[1, 9:14] = m[6, 9:14] = 1
        m[2:6, 8] = m[2:6, 14] = 1
    elif name == "stairs":                             # a staircase diagonal: each step two pixels wide
        for j in range(min(H - 1, 7)):
            m[j, 5 + j:7 + j] = 1
    elif name == "seam":
        _line(m, 2, W - 9, 0, 1, 18, 2)
    elif name == "vee":                                # both arms end backward of the tip; the exposed tip points forward
        _line(m, 6, 30, -1, -1, 6)
        _line(m, 6, 30, -1, 1, 6)
    elif name == "touching":                           # the two classes side by side, each with a spur into the other
        _line(m, 3, 4, 0, 1, 30, 1)
        _line(m, 4, 4, 0, 1, 30, 2)
        m[2, 12], m[5, 13], m[6, 13] = 1, 2, 2
    else:
        raise KeyError(name)
    return m


SPUR_2 = [(4, 21), (3, 22)]
SPUR_7 = [(5, 41), (4, 42), (3, 43), (2, 44), (1, 45), (0, 46), (0, 47)]
DRAWN = ("spurs", "two", "single", "ring", "stairs", "seam", "vee", "touching")


def polylines(H, W, seed=3):
    """uint8 [H, W]: long one-pixel polylines of both classes with spurs of 2 .. 30 pixels every 50 columns, one across the seam"""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    for j, r0 in enumerate(range(40, H - 40, 60)):
        cls, r = 1 + j % 2, r0
        for c in range(j * 7, j * 7 + W - 100 + (120 if j == 3 else 0)):
            r += int(rs.randint(-1, 2)) if c % 3 == 0 else 0
            r = min(max(r, r0 - 25), r0 + 25)
            m[r, c % W] = cls
            if c % 50 == 25:
                _line(m, r + 1, c, 1, int(rs.randint(-1, 2)), int(rs.randint(2, 31)), cls)
    return m
