"""Checker of the event matching (nn.EventMatcher, dc_component_overlap / dc_event_scores) in numpy, on top of the flood fill of
tests/util_events.py.  Everything follows the definitions literally:

  pairs     np.unique over the (label a, label b) of the pixels where both are non-zero, with counts; labels become ranks through the
            rows' roots; pairs with a rank >= its cap are not listed; sorted by (rank a, rank b)
  coverage  per component of rank < cap: the number of its pixels at which the other mask has the same class
  scores    a component of class 1 or 2 is scored when pixels >= max(min_pixels, 1) and rank < cap; it is matched when cover >= 1 and
            cover * 1024 >= cover_q * pixels; per class: hits (matched in b), misses (unmatched in b), false alarms (unmatched in a),
            matched detections (matched in a)"""
import numpy as np

import util_events as ue


def classes(mask):
    mask = np.asarray(mask)
    return np.where((mask == 1) | (mask == 2), mask, 0).astype(np.int64)


def pairs_one(lab_a, rows_a, lab_b, rows_b, cap_a, cap_b):
    """int64 [n, 3] (rank a, rank b, pixels), sorted, and the number of listable pairs"""
    both = (lab_a != 0) & (lab_b != 0)
    if not both.any():
        return np.zeros((0, 3), np.int64)
    ab = np.stack([lab_a[both].astype(np.int64), lab_b[both].astype(np.int64)], axis=1)
    uniq, cnt = np.unique(ab, axis=0, return_counts=True)
    rank_a = {int(r) + 1: k for k, r in enumerate(rows_a[:, 0])}
    rank_b = {int(r) + 1: k for k, r in enumerate(rows_b[:, 0])}
    out = [(rank_a[int(u)], rank_b[int(v)], int(n)) for (u, v), n in zip(uniq, cnt)]
    out = sorted(p for p in out if p[0] < cap_a and p[1] < cap_b)
    return np.asarray(out, np.int64).reshape(-1, 3)


def cover_one(lab, rows, cls_self, cls_other, cap):
    """int64 [cap]: per row k < cap the pixels of that component where the other mask has the same class"""
    out = np.zeros(cap, np.int64)
    same = (cls_self != 0) & (cls_self == cls_other)
    # every pixel of a component carries root + 1: count the `same` pixels per label, then pick the rows' labels
    counts = np.bincount(lab[same].astype(np.int64), minlength=int(lab.max()) + 2 if lab.size else 2)
    for k, row in enumerate(rows[:cap]):
        out[k] = counts[int(row[0]) + 1]
    return out


def scores_one(rows_a, cover_a, rows_b, cover_b, cap_a, cap_b, min_pixels, cover_q):
    """int64 [2, 4]"""
    out = np.zeros((2, 4), np.int64)
    for rows, cover, cap, unmatched, matched in ((rows_b, cover_b, cap_b, 1, 0), (rows_a, cover_a, cap_a, 2, 3)):
        for k, row in enumerate(rows[:cap]):
            cls, px, cov = int(row[1]), int(row[2]), int(cover[k])
            if cls not in (1, 2) or px < max(min_pixels, 1):
                continue
            hit = cov >= 1 and cov * 1024 >= cover_q * px
            out[cls - 1, matched if hit else unmatched] += 1
    return out


def match(mask_a, mask_b, n_valid, connectivity, wrap, wy, cx, sx, cap_a, cap_b=None, min_pixels=0, cover_q=512, pair_cap=None):
    """The whole answer for the first n_valid samples, as a dict:
    pairs (list of sorted [n, 3], ALL listable pairs), cover_a [n_valid, cap_a], cover_b, scores [n_valid, 2, 4], rows_a, rows_b (uncapped),
    ncomp_a, ncomp_b, truncated (samples with more components than a cap or, when pair_cap is given, more pairs than pair_cap)"""
    cap_b = cap_a if cap_b is None else cap_b
    mask_a, mask_b = np.asarray(mask_a), np.asarray(mask_b)
    lab_a, _, ncomp_a, rows_a = ue.catalogue(mask_a, n_valid, connectivity, wrap, wy, cx, sx, cap_a)
    lab_b, _, ncomp_b, rows_b = ue.catalogue(mask_b, n_valid, connectivity, wrap, wy, cx, sx, cap_b)
    out = {"pairs": [], "cover_a": np.zeros((n_valid, cap_a), np.int64), "cover_b": np.zeros((n_valid, cap_b), np.int64),
           "scores": np.zeros((n_valid, 2, 4), np.int64), "rows_a": rows_a, "rows_b": rows_b, "ncomp_a": ncomp_a, "ncomp_b": ncomp_b,
           "labels_a": lab_a, "labels_b": lab_b, "truncated": 0}
    for s in range(n_valid):
        ca, cb = classes(mask_a[s]), classes(mask_b[s])
        out["pairs"].append(pairs_one(lab_a[s], rows_a[s], lab_b[s], rows_b[s], cap_a, cap_b))
        out["cover_a"][s] = cover_one(lab_a[s], rows_a[s], ca, cb, cap_a)
        out["cover_b"][s] = cover_one(lab_b[s], rows_b[s], cb, ca, cap_b)
        out["scores"][s] = scores_one(rows_a[s], out["cover_a"][s], rows_b[s], out["cover_b"][s], cap_a, cap_b, min_pixels, cover_q)
        if len(rows_a[s]) > cap_a or len(rows_b[s]) > cap_b or (pair_cap is not None and len(out["pairs"][s]) > pair_cap):
            out["truncated"] += 1
    return out
