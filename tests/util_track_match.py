"""Checker of the track verification (nn.TrackMatcher, dc_track_match_append / dc_track_match_resolve) in numpy and plain Python, on top of
the track checker of tests/util_tracks.py and the flood fill of tests/util_events.py.  It shares no algorithm with the kernels: overlaps
come from comparing the two label maps pixel by pixel, track pairs and distinct frames from Python dicts and sets; nothing is hashed,
nothing knows about batches.

Side a is the prediction, side b the labels; both are tracked by util_tracks.track.  An OVERLAP is a pair of stored events of one frame
(rank below min(ncomp, cap), event number below event_cap) that have the same class 1 or 2 and share at least one pixel; it is a LINK
(event a, event b, shared pixels).  A link belongs to the track pair (track_of_a[event a], track_of_b[event b]); links with a -1 on either
side are counted and skipped.  Per pair: row a, row b, class, overlaps, DISTINCT common frames, shared pixels, first and last common frame.
Per track: matched frames (the distinct frames in which one of its events has a link) and shared pixels.  A track is scored when
last - first + 1 >= max(min_frames, 1); it is matched when matched >= 1 and matched * 1024 >= cover_q * frames.  scores [2, 4] per class:
hits (matched b), misses (unmatched b), false alarms (unmatched a), matched detections (matched a)."""
import zlib

import numpy as np

import util_events as ue
import util_tracks as ut

T = 8
OVERLAP_PAIR_CAP = 8192                                  # nn.EventMatcher's default pair_cap: the per-frame table the links come from


def sequence(name, H, W):
    """(masks_a, masks_b) uint8 [T, H, W]: the prediction and the labels of a named sequence of T = 8 frames; all fit a 31 x 61 frame"""
    a, b = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W), np.uint8)
    if name in ("identical", "other_class"):             # a class-1 blob that moves 2 columns per frame, a resting class-2 blob
        for t in range(T):
            a[t, 4:10, 5 + 2 * t:13 + 2 * t] = 1
            a[t, 14:19, 20:27] = 2
        b[:] = a if name == "identical" else np.where(a == 0, 0, 3 - a)
    elif name == "lag":                                  # the labels live in frames 0 .. 6, the prediction shows every frame one frame late
        for t in range(T - 1):
            b[t, 4:10, 5 + 2 * t:13 + 2 * t] = 1
            a[t + 1] = b[t]
    elif name == "merged":                               # one labelled storm, predicted as two with a gap of 4 columns
        b[:, 6:12, 10:30] = 2
        a[:, 6:12, 10:18] = a[:, 6:12, 22:30] = 2
    elif name == "missing_middle":                       # the prediction misses frame 4 of a resting storm
        b[:, 5:11, 7:19] = 1
        a[:] = b
        a[T // 2] = 0
    elif name == "drift":                                # both cross the seam, the prediction 5 columns per frame, the labels 4; class 2 rests
        for t in range(T):
            for c in range(8):
                a[t, 4:10, (W - 18 + 5 * t + c) % W] = 1
                b[t, 4:10, (W - 18 + 4 * t + c) % W] = 1
            a[t, 14:19, 20:27] = 2
            b[t, 15:20, 22:29] = 2
    elif name == "random":                               # independent frames on both sides: many pairs, several links per (pair, frame)
        rs = np.random.RandomState(zlib.crc32(f"track match random {H} {W}".encode()))
        a[:] = (rs.rand(T, H, W) < 0.45) * rs.randint(1, 3, (T, H, W))
        b[:] = (rs.rand(T, H, W) < 0.45) * rs.randint(1, 3, (T, H, W))
    else:
        raise KeyError(name)
    return a, b


def frame_links(lab_a, rows_a, cls_a, lab_b, rows_b, cls_b, cap):
    """One frame: (links as sorted (rank a, rank b, shared) of the same-class pairs with both ranks below cap, the number of pairs of ANY
    classes with both ranks below cap -- what the per-frame pair table has to hold)"""
    rank_a = {int(r) + 1: k for k, r in enumerate(rows_a[:cap, 0])}
    rank_b = {int(r) + 1: k for k, r in enumerate(rows_b[:cap, 0])}
    both = (lab_a != 0) & (lab_b != 0)
    same = both & (cls_a == cls_b)
    count = {}
    listed = set()
    for la, lb, s in zip(lab_a[both].tolist(), lab_b[both].tolist(), same[both].tolist()):
        if la in rank_a and lb in rank_b:
            listed.add((la, lb))
            if s:
                count[(la, lb)] = count.get((la, lb), 0) + 1
    return sorted((rank_a[la], rank_b[lb], n) for (la, lb), n in count.items()), len(listed)


def match(masks_a, masks_b, connectivity, wrap, wy, cx, sx, cap=4096, event_cap=1 << 19, track_cap_a=None, track_cap_b=None, min_pixels=0,
          link_cap=1 << 20, pair_cap=1 << 16, min_frames=1, cover_q=512, overlap_pair_cap=OVERLAP_PAIR_CAP):
    """The whole answer as a dict: "a", "b" (util_tracks.track of the two sides), "links" int64 [n, 3] (ALL links, sorted), "state" int64
    [4], "all_pairs" int64 [p, 8] (ALL track pairs, sorted by (row a, row b)), "pairs" (the same when p <= pair_cap, else None: which rows
    are kept is unspecified), "counts" int64 [4], "cover_a" int64 [ma, 2], "cover_b" int64 [mb, 2], "scores" int64 [2, 4].  Everything
    behind "state" is computed from ALL links: with n > link_cap the device's results are those of the links it kept."""
    masks_a, masks_b = np.asarray(masks_a, np.uint8), np.asarray(masks_b, np.uint8)
    frames = masks_a.shape[0]
    side_a = ut.track(masks_a, connectivity, wrap, wy, cx, sx, cap=cap, event_cap=event_cap, track_cap=track_cap_a, min_pixels=min_pixels)
    side_b = ut.track(masks_b, connectivity, wrap, wy, cx, sx, cap=cap, event_cap=event_cap, track_cap=track_cap_b, min_pixels=min_pixels)
    lab_a, _, ncomp_a, rows_a = ue.catalogue(masks_a, frames, connectivity, wrap, wy, cx, sx, cap)
    lab_b, _, ncomp_b, rows_b = ue.catalogue(masks_b, frames, connectivity, wrap, wy, cx, sx, cap)
    cls = lambda m: np.where((m == 1) | (m == 2), m, 0)  # noqa: E731
    na, nb = int(side_a["state"][0]), int(side_b["state"][0])
    links, truncated = [], 0
    for f in range(frames):
        per_frame, listed = frame_links(lab_a[f], rows_a[f], cls(masks_a[f]), lab_b[f], rows_b[f], cls(masks_b[f]), cap)
        if listed > overlap_pair_cap or int(ncomp_a[f, 0]) > cap or int(ncomp_b[f, 0]) > cap:
            truncated += 1
        assert listed <= overlap_pair_cap, "the checker does not model a truncated per-frame pair table"
        for ra, rb, n in per_frame:
            ea, eb = int(side_a["first"][f]) + ra, int(side_b["first"][f]) + rb
            if ea < na and eb < nb:
                assert side_a["store"][ea, 3] == side_b["store"][eb, 3] and side_a["store"][ea, 0] == f == side_b["store"][eb, 0]
                links.append((ea, eb, n))
    links.sort()
    stored = min(len(links), link_cap)
    out = {"a": side_a, "b": side_b, "links": np.array(links, np.int64).reshape(-1, 3),
           "state": np.array([stored, len(links) - stored, frames, truncated], np.int64)}
    out.update(resolve(out["links"], side_a, side_b, pair_cap=pair_cap, min_frames=min_frames, cover_q=cover_q))
    return out


def resolve(links, side_a, side_b, pair_cap=1 << 16, min_frames=1, cover_q=512):
    """The resolve of a list of links (event a, event b, shared) against the two sides' tracks: "all_pairs", "pairs", "counts", "cover_a",
    "cover_b", "scores" as match() documents them.  Also what the device must give for whichever links it kept when its store overflowed."""
    ma, mb = len(side_a["tracks"]), len(side_b["tracks"])
    pairs, skipped = {}, 0
    frames_a, frames_b = [set() for _ in range(ma)], [set() for _ in range(mb)]
    cover_a, cover_b = np.zeros((ma, 2), np.int64), np.zeros((mb, 2), np.int64)
    for ea, eb, n in np.asarray(links, np.int64).reshape(-1, 3).tolist():
        ta, tb = int(side_a["track_of"][ea]), int(side_b["track_of"][eb])
        if ta < 0 or tb < 0:
            skipped += 1
            continue
        f = int(side_a["store"][ea, 0])
        p = pairs.setdefault((ta, tb), {"class": int(side_a["tracks"][ta, 1]), "links": 0, "frames": set(), "shared": 0})
        p["links"] += 1
        p["frames"].add(f)
        p["shared"] += n
        frames_a[ta].add(f)
        frames_b[tb].add(f)
        cover_a[ta, 1] += n
        cover_b[tb, 1] += n
    cover_a[:, 0] = [len(s) for s in frames_a]
    cover_b[:, 0] = [len(s) for s in frames_b]
    all_pairs = np.array([[ta, tb, p["class"], p["links"], len(p["frames"]), p["shared"], min(p["frames"]), max(p["frames"])]
                          for (ta, tb), p in sorted(pairs.items())], np.int64).reshape(-1, 8)
    counts = np.array([min(len(all_pairs), pair_cap), int(len(all_pairs) > pair_cap), skipped, 0], np.int64)
    scores = np.zeros((2, 4), np.int64)
    for tracks, cover, unmatched, matched in ((side_b["tracks"], cover_b, 1, 0), (side_a["tracks"], cover_a, 2, 3)):
        for row, cov in zip(tracks.tolist(), cover.tolist()):
            n = row[4] - row[3] + 1
            if row[1] not in (1, 2) or n < max(min_frames, 1):
                continue
            hit = cov[0] >= 1 and cov[0] * 1024 >= cover_q * n
            scores[row[1] - 1, matched if hit else unmatched] += 1
    return {"all_pairs": all_pairs, "pairs": all_pairs if len(all_pairs) <= pair_cap else None, "counts": counts, "cover_a": cover_a,
            "cover_b": cover_b, "scores": scores}


def assert_inside_caps(ref):
    """nothing of this answer was cut: every comparison with the device may be row for row"""
    assert ref["state"][1] == 0 and ref["state"][3] == 0, f"links dropped or frames truncated: {ref['state'].tolist()}"
    assert ref["counts"][1] == 0 and ref["counts"][2] == 0 and ref["pairs"] is not None, f"pairs cut or links skipped: {ref['counts'].tolist()}"
    for side in (ref["a"], ref["b"]):
        assert side["state"][2] == 0 and side["state"][3] == 0 and side["ntracks"][0] == side["ntracks"][3], "a tracker's tables were cut"


def decoded(ref, H, W):
    """the two sides' tracks as nn.EventTracker.decode gives them, one dict per track row"""
    from mlperf_deepcam_amd import nn as dnn
    return [dnn.EventTracker.decode(s["store"], s["track_of"], s["tracks"], H, W) for s in (ref["a"], ref["b"])]


def rows_of(ref):
    """the checker's answer in the form of nn.TrackMatcher.rows()"""
    return {"state": ref["state"], "counts": ref["counts"], "scores": ref["scores"], "pairs": ref["pairs"], "cover_a": ref["cover_a"],
            "cover_b": ref["cover_b"], "tracks_a": ref["a"]["tracks"], "tracks_b": ref["b"]["tracks"]}
