"""Checker of the main course of an event (dc_skeleton_course; nn.EventAxis(course=True)): the text of include/deepcam_hip.h in plain
Python -- the link graph from the skeleton and a flood-fill label map, heapq Dijkstra in Python ints, the double sweep with its ties --
and the hand-drawn cases of its tests."""
import heapq

import numpy as np

from util_event_axis import RING

FIELDS = 7
LINK = ((-1, 1), (-1, 2), (0, 0), (0, 2), (0, 1), (0, 2), (0, 0), (-1, 2))     # per RING direction: the upper end's row offset, the table's column

# name -> strokes (class, row, column, d row, d column, pixels); a negative column counts from the right edge.  Drawn for 24 x 70 and up.
CASES = {
    "seam": [(1, 3, -4, 0, 1, 9)],                                              # a straight line across the seam
    "rows": [(1, 2, 5, 0, 1, 12), (2, 11, 5, 0, 1, 12)],                        # the same straight row at two latitudes
    "ypsilon": [(2, 12, 11, 0, 1, 10), (2, 11, 21, -1, 1, 4), (2, 13, 21, 1, 1, 6)],      # arms of 9, 4 and 6 links
    "detour": [(1, 1, 30, 0, 1, 31), (1, 2, 45, 1, 0, 8)],                      # many short links near the pole, few long ones down a meridian
    "plus": [(1, 12, 35, 0, 1, 11), (1, 10, 40, 1, 0, 5)],                      # E and W tips tie
    "ring": [(2, 4, 50, 0, 1, 9), (2, 9, 50, 0, 1, 9), (2, 5, 50, 1, 0, 4), (2, 5, 58, 1, 0, 4)],
    "tail": [(1, 14, 8, 0, 1, 6), (1, 18, 8, 0, 1, 6), (1, 15, 8, 1, 0, 3), (1, 15, 13, 1, 0, 3), (1, 16, 14, 0, 1, 9)],
    "corner": [(1, 15, 5, 1, 0, 3), (1, 17, 6, 0, 1, 2), (2, 4, 4, 1, 1, 5)],   # an L, and a pure diagonal
    "stairs": [(1, 18, 10, 0, 1, 2), (1, 19, 11, 0, 1, 2), (1, 20, 12, 0, 1, 2), (1, 21, 13, 0, 1, 2)],
    "block": [(2, 6, 30, 0, 1, 2), (2, 7, 30, 0, 1, 2)],
    "dots": [(1, 0, 0, 0, 1, 1), (2, 0, -1, 0, 1, 1), (1, 23, -1, 0, 1, 1), (2, 12, 33, 0, 1, 1)],
    "touch": [(1, 6, 10, 0, 1, 5), (2, 7, 15, 0, 1, 5), (1, 16, 10, 0, 1, 5), (1, 17, 15, 0, 1, 5)],   # two classes; one class, two events under 4
}
TREES = ("seam", "rows", "ypsilon", "detour", "plus", "corner", "stairs", "dots", "touch")


def drawn(name, H, W):
    m = np.zeros((H, W), np.uint8)
    for cls, r, c, dr, dc, n in CASES[name]:
        for i in range(n):
            m[r + i * dr, (c + i * dc) % W] = cls
    return m


def graph(skel, labels, roots, cap, wrap, link, cls):
    """{pixel: (rank, [(neighbour pixel, metres), ...])} of the nodes of class cls"""
    H, W = skel.shape
    rank = {int(r): k for k, r in enumerate(roots)}

    def nb(r, c, dr, dc):
        rr, cc = r + dr, c + dc
        if rr < 0 or rr >= H or ((cc < 0 or cc >= W) and not wrap):
            return None
        return rr * W + cc % W if skel[rr, cc % W] == cls and labels[rr, cc % W] == labels[r, c] else None

    g = {}
    for r, c in zip(*np.nonzero(skel == cls)):
        k = rank.get(int(labels[r, c]) - 1, cap)
        if k >= cap:
            continue
        n = [nb(r, c, dr, dc) for dr, dc in RING]
        g[int(r) * W + int(c)] = (k, [(q, int(link[r + LINK[j][0], LINK[j][1]])) for j, q in enumerate(n) if q is not None and
                                      not (j % 2 == 1 and (n[j - 1] is not None or n[(j + 1) % 8] is not None))])
    return g


def distances(g, src):
    d, heap = {src: 0}, [(0, src)]
    while heap:
        dp, p = heapq.heappop(heap)
        if dp > d[p]:
            continue
        for q, w in g[p][1]:
            if dp + w < d.get(q, dp + w + 1):
                d[q] = dp + w
                heapq.heappush(heap, (dp + w, q))
    return d


def farthest(d):
    """(distance, node): the largest distance, ties to the smallest pixel index"""
    v, p = max((v, -p) for p, v in d.items())
    return v, -p


def diameter(g, members):
    """all pairs: the geodesic diameter of one event"""
    return max(max(distances(g, p).values()) for p in members)


def course(skel, labels, roots, cap, wrap, link, node_cap):
    """one frame -> (rows int64 [cap, 7], course uint8 [H, W], status [[nodes, overflow]] per class -- the rounds are not determined)"""
    rows, cmap, status = np.zeros((cap, FIELDS), np.int64), np.zeros(skel.shape, np.uint8), []
    for cls in (1, 2):
        g = graph(skel, labels, roots, cap, wrap, link, cls)
        status.append([len(g), int(len(g) > node_cap)])
        events = {}
        for p, (k, _) in g.items():
            events.setdefault(k, []).append(p)
        for k, members in events.items():
            if len(g) > node_cap:
                rows[k, 0], rows[k, 6] = len(members), -1
                continue
            s = min(members)
            ecc, a = farthest(distances(g, s))
            da = distances(g, a)
            length, b = farthest(da)
            db = distances(g, b)
            on = [p for p in members if p in da and p in db and da[p] + db[p] == length]
            rows[k] = [len(members), s, ecc, a, b, len(on), length]
            cmap.reshape(-1)[on] = cls
    return rows, cmap, status
