"""Checkers of the event skeletons (nn.EventAxis; dc_mask_thin, dc_skeleton_stats) and the masks their tests use.  thin() is the header's
text in plain numpy on padded uint8 planes, no bit packing and no words; stats() is a per-pixel Python loop over the skeleton."""
import zlib

import numpy as np

import util_events as ue

FIELDS = 7
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # P2 .. P9, clockwise from north


def thin_plane(f, wrap, max_iters):
    """f: bool [H, W] -> (skeleton bool [H, W], passes, converged)"""
    f = np.asarray(f).astype(np.uint8)
    H, W = f.shape
    for passes in range(1, max_iters + 1):
        deleted = 0
        for sub in (0, 1):
            p = np.zeros((H + 2, W + 2), np.uint8)
            p[1:-1, 1:-1] = f
            if wrap:
                p[1:-1, 0], p[1:-1, -1] = f[:, -1], f[:, 0]
            p2, p3, p4, p5, p6, p7, p8, p9 = (p[1 + dr:H + 1 + dr, 1 + dc:W + 1 + dc].astype(bool) for dr, dc in RING)
            i = lambda x: x.astype(np.int32)  # noqa: E731
            C = i(~p2 & (p3 | p4)) + i(~p4 & (p5 | p6)) + i(~p6 & (p7 | p8)) + i(~p8 & (p9 | p2))
            N = np.minimum(i(p9 | p2) + i(p3 | p4) + i(p5 | p6) + i(p7 | p8), i(p2 | p3) + i(p4 | p5) + i(p6 | p7) + i(p8 | p9))
            m = ((p6 | p7 | ~p9) & p8) if sub == 0 else ((p2 | p3 | ~p5) & p4)
            dele = f.astype(bool) & (C == 1) & (N >= 2) & (N <= 3) & ~m
            deleted += int(dele.sum())
            f = f & ~dele
        if deleted == 0:
            return f.astype(bool), passes, 1
    return f.astype(bool), max_iters, 0


def thin(mask, n_valid, wrap, max_iters):
    """mask [B, H, W] of any integer dtype -> (skeleton uint8 [n_valid, H, W], iters int32 [n_valid, 2, 2])"""
    mask = np.asarray(mask)
    skel = np.zeros((n_valid,) + mask.shape[1:], np.uint8)
    iters = np.zeros((n_valid, 2, 2), np.int32)
    for b in range(n_valid):
        for k in (1, 2):
            s, iters[b, k - 1, 0], iters[b, k - 1, 1] = thin_plane(mask[b] == k, wrap, max_iters)
            skel[b][s] = k
    return skel, iters


def stats(skel, labels, roots, cap, wrap, link):
    """skel uint8 [H, W], labels int32 [H, W], roots: the catalogue's roots in rank order -> rows int64 [cap, 7]"""
    H, W = skel.shape
    rank = {int(r): k for k, r in enumerate(roots)}
    rows = np.zeros((cap, FIELDS), np.int64)

    def nb(r, c, dr, dc):
        rr, cc = r + dr, c + dc
        if rr < 0 or rr >= H or ((cc < 0 or cc >= W) and not wrap):
            return 0
        return int(skel[rr, cc % W] != 0 and labels[rr, cc % W] == labels[r, c])

    for r, c in zip(*np.nonzero(skel)):
        k = rank[int(labels[r, c]) - 1]
        if k >= cap:
            continue
        n = [nb(r, c, dr, dc) for dr, dc in RING]                      # n[0] = P2 ... n[7] = P9
        ew, ns = n[2], n[4]
        diag = int(n[3] and not n[2] and not n[4]) + int(n[5] and not n[6] and not n[4])
        rows[k] += [1, sum(n) == 1, sum(n[(j + 1) % 8] > n[j] for j in range(8)) >= 3, ew, ns, diag,
                    ew * int(link[r, 0]) + ns * int(link[r, 1]) + diag * int(link[r, 2])]
    return rows


def reference(mask, n_valid, conn, wrap, cap, max_iters, tables, link):
    """the whole chain on the host: {"skeleton", "iters", "rows" [n_valid, cap, 7]}"""
    mask = np.asarray(mask)
    skel, iters = thin(mask, n_valid, wrap, max_iters)
    labels, _, _, every = ue.catalogue(np.where((mask == 1) | (mask == 2), mask, 0).astype(np.uint8), n_valid, conn, wrap, *tables, cap)
    rows = np.stack([stats(skel[b], labels[b], every[b][:, 0], cap, wrap, link) for b in range(n_valid)])
    return {"skeleton": skel, "iters": iters, "rows": rows}


def _disc(m, r0, c0, rad, cls):
    H, W = m.shape
    rr, cc = np.mgrid[0:H, 0:W]
    dc = (cc - c0 + W / 2) % W - W / 2
    m[(rr - r0) ** 2 + dc ** 2 <= rad * rad] = cls


def make_mask(name, H, W, nb=2):
    """uint8 [nb, H, W]; both classes appear in every kind that has room for them"""
    rs = np.random.RandomState(zlib.crc32(f"axis {name} {H} {W}".encode()))
    m = np.zeros((nb, H, W), np.uint8)
    rr, cc = np.mgrid[0:H, 0:W]
    for b in range(nb):
        if name == "blobs":                                            # random discs of both classes, some across the seam and the word borders
            for _ in range(max(H * W // 250, 3)):
                _disc(m[b], rs.randint(H), rs.randint(W), rs.uniform(0.8, min(H, 24) / 4), rs.randint(1, 3))
            m[b][rs.rand(H, W) < 0.01] = 3                             # other values are background
        elif name == "band":                                           # a thick diagonal band that crosses the seam
            m[b][((cc - 2 * rr - 5 * b) % W) < max(H // 3, 3)] = 1 + b
        elif name == "full":
            m[b] = 1 + b
        elif name == "checker":
            m[b] = 1 + (rr + cc + b) % 2
        elif name == "small":                                          # 2 x 2 squares and single pixels, at the corners and the word borders too
            for r, c in ((0, 0), (H - 2, W - 2), (3, 62), (3, W - 1)):
                m[b, r:r + 2, c:c + 2] = 1
            for r, c in ((0, W - 4), (H - 1, 0), (5, 63 % W), (5, 3)):
                m[b, r, c] = 2
        elif name == "ring":
            d2 = (rr - H / 2) ** 2 + ((cc - 5 * b + W / 2) % W - W / 2) ** 2
            m[b][(d2 <= (H / 2 - 0.5) ** 2) & (d2 >= (H / 4) ** 2)] = 2 - b
        elif name == "rect":                                           # touches the first and the last row
            m[b, :, W // 3:W // 3 + 9] = 1
            m[b, :, W - 3:] = 2
            m[b, :, :2] = 2
        elif name == "field":                                          # full size: some forty blobs and one long curved band
            for _ in range(40):
                _disc(m[b], rs.randint(H), rs.randint(W), rs.uniform(2, 10), rs.randint(1, 3))
            m[b][np.abs(rr - H / 2 - H / 4 * np.sin(cc * 2 * np.pi / W)) < 6] = 2
        else:
            raise KeyError(name)
    return m
