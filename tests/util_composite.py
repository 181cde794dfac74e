"""Checker of the storm-centred composites (nn.StormComposite, dc_composite_centers / dc_composite_accumulate): the definition of
include/deepcam_hip.h restated as a plain numpy loop over events and cells, with no knowledge of the kernel's worklists, slices and
quads.  It works from what the catalogue and EventFields produced -- label maps, catalogue rows, field rows -- and from the fields and
the radius table.

centres: row k < min(ncomp[b, 0], cap) of a frame with group in [0, G) falls into the first category that applies: other_class,
below_min_pixels, no_center (min word -1 / max word 0), else composited with centre = the pixel in the low half of the word, bin = the
number of edges whose key is <= the key in the high half; uncatalogued += max(ncomp - cap, 0).
windows: for every composited event with centre (r0, c0), group g, and every cell (i, j), di = i - R, dj = j - R: southern iff flip and
2 r0 < H - 1; r = r0 - di if southern else r0 + di; c = (c0 + dj) mod W; rows off the grid add nothing; events[g] += 1; inside += labels
== root + 1; q = rint(ldexp(double(v), bits)); finite v with |q| <= 2^28 only; negated for a southern event where the channel's bit is
set; sum += q, n += 1; k = rbin[r0, (r - r0) + R, |dj|] < NB: rsum[g, k] += q, rn[g, k] += 1."""
import numpy as np

LIMIT = float(2 ** 28)
KEYS = ("events", "sum", "n", "inside", "rsum", "rn")
COUNTS = ("composited", "no_center", "below_min_pixels", "other_class", "uncatalogued")


def key(v):
    """the order-preserving 32-bit key of one float32 value, as a Python int"""
    u = int(np.asarray(v, np.float32).reshape(1).view(np.uint32)[0])
    return (u ^ 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def empty(GT, R, C, NB):
    S = 2 * R + 1
    return {"events": np.zeros(GT, np.int64), "sum": np.zeros((GT, S, S, C), np.int64), "n": np.zeros((GT, S, S, C), np.int32),
            "inside": np.zeros((GT, S, S), np.int32), "rsum": np.zeros((GT, NB, C), np.int64), "rn": np.zeros((GT, NB, C), np.int64),
            "counts": dict.fromkeys(COUNTS, 0)}


def centers(table, ncomp, ftable, H, W, center_channel, stat, classes, min_pixels, frame_group, G, edges, counts):
    """(centers, egroup) int32 [B, cap] of one batch, -1 where a row is not composited; `counts` (a dict over COUNTS) is advanced in
    place.  Frames from len(frame_group) on do not exist for the checker: pass the valid frames only."""
    table, ftable = np.asarray(table, np.int64), np.asarray(ftable, np.int64)
    n, cap = len(frame_group), table.shape[1]
    cen = np.full((n, cap), -1, np.int32)
    egr = np.full((n, cap), -1, np.int32)
    edge_keys = [key(e) for e in edges]
    for b in range(n):
        g = int(frame_group[b])
        if g < 0 or g >= G:
            continue
        total = int(ncomp[b][0])
        counts["uncatalogued"] += max(total - cap, 0)
        for k in range(min(total, cap)):
            cls, pixels = int(table[b, k, 1]), int(table[b, k, 2])
            word = int(ftable[b, k, center_channel, 0 if stat == "min" else 1]) & 0xFFFFFFFFFFFFFFFF
            if cls not in classes:
                counts["other_class"] += 1
            elif pixels < min_pixels:
                counts["below_min_pixels"] += 1
            elif word == (0xFFFFFFFFFFFFFFFF if stat == "min" else 0):
                counts["no_center"] += 1
            else:
                counts["composited"] += 1
                low = word & 0xFFFFFFFF
                cen[b, k] = low if stat == "min" else 0xFFFFFFFF - low
                assert 0 <= cen[b, k] < H * W
                egr[b, k] = g * (len(edges) + 1) + sum(1 for e in edge_keys if (word >> 32) >= e)
    return cen, egr


def accumulate(state, cen, egr, table, labels, fields, chan, bits, negate, flip_south, rbin, R):
    """Adds the windows of one batch to `state` (in place; also returned).  cen, egr as centers() leaves them; table int64 [n, cap, 10];
    labels int32 [n, H, W]; fields float32 [n, H, W, ldc]; chan: the selected channels; bits per selected channel; negate: positions of
    selected channels; rbin uint8 [H, S, R + 1] or None."""
    labels, fields = np.asarray(labels), np.asarray(fields, np.float32)
    _, H, W = labels.shape
    S, C = 2 * R + 1, len(chan)
    NB = state["rsum"].shape[1]
    sign = np.asarray([-1 if c in negate else 1 for c in range(C)], np.int64)
    sh = np.asarray(bits, np.int32)
    for b in range(cen.shape[0]):
        for k in range(cen.shape[1]):
            p, g = int(cen[b, k]), int(egr[b, k])
            if p < 0:
                continue
            r0, c0 = divmod(p, W)
            root = int(table[b, k, 0])
            south = bool(flip_south) and 2 * r0 < H - 1
            state["events"][g] += 1
            for i in range(S):
                di = i - R
                r = r0 - di if south else r0 + di
                if r < 0 or r >= H:
                    continue
                for j in range(S):
                    dj = j - R
                    c = (c0 + dj) % W
                    state["inside"][g, i, j] += int(labels[b, r, c]) == root + 1
                    v = fields[b, r, c, chan]
                    with np.errstate(over="ignore", invalid="ignore"):
                        q = np.rint(np.ldexp(v.astype(np.float64), sh))
                        ok = np.isfinite(v) & (np.abs(q) <= LIMIT)
                    q = np.where(ok, q, 0.0).astype(np.int64)
                    if south:
                        q = q * sign
                    state["sum"][g, i, j] += q
                    state["n"][g, i, j] += ok
                    if rbin is not None:
                        kb = int(rbin[r0, (r - r0) + R, abs(dj)])
                        if kb < NB:
                            state["rsum"][g, kb] += q
                            state["rn"][g, kb] += ok
    return state


def assert_state(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].dtype, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())
    assert got["counts"] == ref["counts"], (what, got["counts"], ref["counts"])
