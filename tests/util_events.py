"""Checker of the event catalogue (nn.EventCatalog, dc_mask_components / dc_component_stats): a breadth-first flood fill in plain Python
that implements the definition literally -- deliberately another algorithm than the kernels' union-find.

Classes 1 and 2 are foreground, everything else background.  A component is a maximal set of pixels of one class connected under
connectivity 4 or 8; rows never wrap, with `wrap` column W-1 touches column 0 (diagonally too under 8).  Labels: 0 for background, else
1 + the smallest r * W + c of the component.  Table row k: the component with the k-th smallest root:
root, class, pixels, sum wy[r], sum r, sum cx[c], sum sx[c], first row, last row, seam (pixels in column 0 and in column W-1)."""
from collections import deque

import numpy as np

FIELDS = 10


def label_one(mask, connectivity, wrap, wy, cx, sx):
    """mask uint8 [H, W] -> (labels int32 [H, W], rows int64 [n, 10] in root order)"""
    H, W = mask.shape
    m = np.where((mask == 1) | (mask == 2), mask, 0).astype(np.int64).tolist()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    elif connectivity != 4:
        raise ValueError("connectivity must be 4 or 8")
    lab = [[0] * W for _ in range(H)]
    rows = []
    for r0 in range(H):
        for c0 in range(W):
            cl = m[r0][c0]
            if cl == 0 or lab[r0][c0]:
                continue
            root = r0 * W + c0                     # row-major scan: the first pixel met is the component's smallest index
            lab[r0][c0] = root + 1
            q = deque([(r0, c0)])
            n = area = sr = scx = ssx = 0
            rmin, rmax, first, last = r0, r0, False, False
            while q:
                r, c = q.popleft()
                n += 1
                area += int(wy[r])
                sr += r
                scx += int(cx[c])
                ssx += int(sx[c])
                rmin, rmax = min(rmin, r), max(rmax, r)
                first, last = first or c == 0, last or c == W - 1
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if rr < 0 or rr >= H:
                        continue
                    if cc < 0 or cc >= W:
                        if not wrap:
                            continue
                        cc %= W
                    if m[rr][cc] == cl and not lab[rr][cc]:
                        lab[rr][cc] = root + 1
                        q.append((rr, cc))
            rows.append([root, cl, n, area, sr, scx, ssx, rmin, rmax, int(first and last)])
    return np.asarray(lab, dtype=np.int32).reshape(H, W), np.asarray(rows, dtype=np.int64).reshape(-1, FIELDS)


def catalogue(mask, n_valid, connectivity, wrap, wy, cx, sx, cap):
    """mask uint8 [B, H, W] -> (labels int32 [n_valid, H, W], table int64 [n_valid, cap, 10], ncomp int32 [n_valid, 3], rows: the uncapped
    rows per sample) of the first n_valid samples"""
    mask = np.asarray(mask)
    _, H, W = mask.shape
    labels = np.zeros((n_valid, H, W), np.int32)
    table = np.zeros((n_valid, cap, FIELDS), np.int64)
    ncomp = np.zeros((n_valid, 3), np.int32)
    every = []
    for b in range(n_valid):
        labels[b], rows = label_one(mask[b], connectivity, wrap, wy, cx, sx)
        k = min(len(rows), cap)
        table[b, :k] = rows[:k]
        ncomp[b] = [len(rows), int((rows[:, 1] == 1).sum()), int((rows[:, 1] == 2).sum())]
        every.append(rows)
    return labels, table, ncomp, every
