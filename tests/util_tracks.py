"""Checker of the event tracks (nn.EventTracker, dc_track_append / dc_track_link / dc_track_resolve) in numpy, on top of the flood fill of
tests/util_events.py -- a plain union-find with path halving over the events of the whole stack, deliberately not the kernels' atomicMin
forest and with no notion of batches.

Frames are numbered 0, 1, 2, ...  The events of a frame are the rows of its catalogue table (rank k < min(ncomp, cap)); the event number
of (frame f, rank k) is the count of events in the frames before f, plus k; events with a number >= event_cap are counted, not stored.
Two stored events of consecutive frames are linked when they have the same class, share at least one pixel at which both masks hold that
class, and each has at least max(min_pixels, 1) pixels.  A track is a connected component of the stored events; its id is the smallest
event number it holds, rows are ordered by id:  id, class, events, first frame, last frame, pixels, peak, area  with
peak = max over the events of (pixels << 32) | (0xFFFFFFFF - frame)."""
import numpy as np

import util_events as ue

STORE, TRACK = 12, 8


def checkerboard(T, H, W):
    """uint8 [T, H, W], mask[t] = 1 + (r + c + t) % 2: under 4-connectivity every pixel is an event, and its class alternates from frame to
    frame, so nothing links -- T * H * W events and as many tracks, the way to more than 256 chunks of either at a small frame"""
    t, r, c = np.ogrid[:T, :H, :W]
    return (1 + (r + c + t) % 2).astype(np.uint8)


def track(masks, connectivity, wrap, wy, cx, sx, cap=4096, event_cap=1 << 19, track_cap=None, min_pixels=0, cuts=()):
    """masks uint8 [T, H, W] -> {"state" int64 [4], "store" int64 [n, 12], "track_of" int32 [n], "tracks" int64 [m, 8], "ntracks" int64 [4],
    "first" int64 [T]}.  cuts: frame numbers that are NOT linked to the frame before them (EventTracker.cut())."""
    masks = np.asarray(masks, np.uint8)
    T = masks.shape[0]
    track_cap = event_cap if track_cap is None else track_cap
    labels, table, ncomp, _ = ue.catalogue(masks, T, connectivity, wrap, wy, cx, sx, cap)
    fg = np.where((masks == 1) | (masks == 2), masks, 0)
    counts = [min(int(ncomp[f, 0]), cap) for f in range(T)]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(first[T])
    n = min(total, event_cap)
    state = np.array([n, T, total - n, sum(1 for f in range(T) if int(ncomp[f, 0]) > cap)], np.int64)
    store = np.zeros((n, STORE), np.int64)
    for f in range(T):
        for k in range(counts[f]):
            e = int(first[f]) + k
            if e < n:
                store[e, 0], store[e, 1], store[e, 2:] = f, k, table[f, k]
    # rank of every root, per frame
    rank_of = [{int(table[f, k, 0]) + 1: k for k in range(counts[f])} for f in range(T)]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    need = max(int(min_pixels), 1)
    for f in range(1, T):
        if f in cuts:
            continue
        both = (fg[f - 1] != 0) & (fg[f - 1] == fg[f])
        pairs = np.unique(np.stack([labels[f - 1][both], labels[f][both]], axis=1), axis=0) if both.any() else np.zeros((0, 2), np.int64)
        for la, lb in pairs.tolist():
            if la not in rank_of[f - 1] or lb not in rank_of[f]:
                continue                                   # a component beyond its frame's table is no event
            ea, eb = int(first[f - 1]) + rank_of[f - 1][la], int(first[f]) + rank_of[f][lb]
            if ea >= n or eb >= n or store[ea, 4] < need or store[eb, 4] < need:
                continue
            ra, rb = find(ea), find(eb)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = [find(e) for e in range(n)]
    ids = sorted(set(roots))
    row = {r: i for i, r in enumerate(ids)}
    m = min(len(ids), track_cap)
    tracks = np.zeros((m, TRACK), np.int64)
    track_of = np.full(n, -1, np.int32)
    peak = [0] * m
    for e in range(n):
        t = row[roots[e]]
        if t >= m:
            continue
        track_of[e] = t
        fr, px = int(store[e, 0]), int(store[e, 4])
        if tracks[t, 2] == 0:
            tracks[t, :2] = [ids[t], store[ids[t], 3]]
            tracks[t, 3] = tracks[t, 4] = fr
        tracks[t, 2] += 1
        tracks[t, 3], tracks[t, 4] = min(tracks[t, 3], fr), max(tracks[t, 4], fr)
        tracks[t, 5] += px
        peak[t] = max(peak[t], (px << 32) | (0xFFFFFFFF - fr))
        tracks[t, 7] += store[e, 5]
    tracks[:, 6] = np.array(peak, np.uint64).view(np.int64) if m else 0
    c1 = sum(1 for r in ids if store[r, 3] == 1)
    ntracks = np.array([len(ids), c1, len(ids) - c1, m], np.int64)
    return {"state": state, "store": store, "track_of": track_of, "tracks": tracks, "ntracks": ntracks, "first": first[:T]}


def flood_tracks(masks, connectivity, wrap):
    """An independent brute force: a breadth-first fill of the [T, H, W] stack, 2-D connectivity inside a frame and same pixel, same class
    between consecutive frames.  Returns the tracks as a sorted list of (class, sorted tuple of (frame, root)) -- root = the smallest
    r * W + c of a 2-D component, which this fill finds by itself."""
    from collections import deque
    masks = np.asarray(masks)
    T, H, W = masks.shape
    m = np.where((masks == 1) | (masks == 2), masks, 0).astype(np.int64).tolist()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    seen = [[[False] * W for _ in range(H)] for _ in range(T)]
    out = []
    for t0 in range(T):
        for r0 in range(H):
            for c0 in range(W):
                cl = m[t0][r0][c0]
                if cl == 0 or seen[t0][r0][c0]:
                    continue
                seen[t0][r0][c0] = True
                q = deque([(t0, r0, c0)])
                pix = []
                while q:
                    t, r, c = q.popleft()
                    pix.append((t, r, c))
                    nb = [(t - 1, r, c), (t + 1, r, c)]
                    for dr, dc in steps:
                        rr, cc = r + dr, c + dc
                        if rr < 0 or rr >= H:
                            continue
                        if cc < 0 or cc >= W:
                            if not wrap:
                                continue
                            cc %= W
                        nb.append((t, rr, cc))
                    for tt, rr, cc in nb:
                        if 0 <= tt < T and m[tt][rr][cc] == cl and not seen[tt][rr][cc]:
                            seen[tt][rr][cc] = True
                            q.append((tt, rr, cc))
                out.append((cl, pix))
    # cut every 3-D component into its 2-D components: a second, 2-D fill restricted to the component's own pixels of one frame
    tracks = []
    for cl, pix in out:
        events = set()
        by_frame = {}
        for t, r, c in pix:
            by_frame.setdefault(t, set()).add((r, c))
        for t, px in by_frame.items():
            left = set(px)
            while left:
                start = min(left)
                comp, q = {start}, deque([start])
                while q:
                    r, c = q.popleft()
                    for dr, dc in steps:
                        rr, cc = r + dr, c + dc
                        if cc < 0 or cc >= W:
                            if not wrap:
                                continue
                            cc %= W
                        if (rr, cc) in left and (rr, cc) not in comp:
                            comp.add((rr, cc))
                            q.append((rr, cc))
                left -= comp
                events.add((t, min(r * W + c for r, c in comp)))
        tracks.append((cl, tuple(sorted(events))))
    return sorted(tracks)
