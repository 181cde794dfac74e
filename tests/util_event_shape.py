"""Checker of the event shapes and the shape filter (nn.EventShape, nn.EventFilter; dc_component_shape, dc_event_select, dc_mask_select):
literal per-pixel loops in Python ints over the labels of the flood fill (tests/util_events.py), and the decode formula of
include/deepcam_hip.h per event with the math module.

Shape row of an event, twelve words: boundary pixels, exposed vertical faces, exposed horizontal faces weighted by wy[r], then
S_x, S_y, S_z, S_xx, S_xy, S_yy, S_xz, S_yz, S_zz.  A 4-neighbour is "not of the same component" when its label differs or when it lies off
the grid; rows are never periodic, columns are with `wrap`.  Keep rule per class: pixels >= min_pixels, area >= min_area,
12 lambda+ >= min_len2, lambda+ >= min_aspect2 lambda-; 0 switches a criterion off; a zeroth moment of 0 fails the last two when active."""
import math

import numpy as np

import util_events as ue

FIELDS = 12
SCALE = 1 << 20


def shape_rows(labels, rows, wrap, rowt, colt):
    """labels int32 [H, W] and the catalogue rows [n, 10] (root order) of ONE sample -> int64 [n, 12] (uncapped)"""
    H, W = labels.shape
    lab = np.asarray(labels).tolist()
    rt, ct = np.asarray(rowt).tolist(), np.asarray(colt).tolist()
    rank = {int(r[0]) + 1: k for k, r in enumerate(np.asarray(rows).tolist())}
    out = [[0] * FIELDS for _ in range(len(rank))]
    for r in range(H):
        wy, c2, cs, c3, c2s, cs2 = (rt[k][r] for k in range(6))
        for c in range(W):
            v = lab[r][c]
            if v == 0:
                continue
            o = out[rank[v]]
            up = r == 0 or lab[r - 1][c] != v
            dn = r == H - 1 or lab[r + 1][c] != v
            if wrap:
                lf, rg = lab[r][(c - 1) % W] != v, lab[r][(c + 1) % W] != v
            else:
                lf, rg = c == 0 or lab[r][c - 1] != v, c == W - 1 or lab[r][c + 1] != v
            cx, sx, cxx, cxy, cyy = (ct[k][c] for k in range(5))
            o[0] += int(up or dn or lf or rg)
            o[1] += int(lf) + int(rg)
            o[2] += (int(up) + int(dn)) * wy
            o[3] += c2 * cx
            o[4] += c2 * sx
            o[5] += cs * SCALE
            o[6] += c3 * cxx
            o[7] += c3 * cxy
            o[8] += c3 * cyy
            o[9] += c2s * cx
            o[10] += c2s * sx
            o[11] += cs2 * SCALE
    assert all(abs(x) < 1 << 63 for o in out for x in o)
    return np.asarray(out, dtype=np.int64).reshape(-1, FIELDS)


def eigenvalues(shape_row, area):
    """(lambda+, lambda-) of one event by the header's decode formula, or None when the zeroth moment is 0"""
    s = [float(int(v)) for v in shape_row]
    if int(area) <= 0:
        return None
    s0 = float(int(area)) * float(SCALE)
    m = [s[3] / s0, s[4] / s0, s[5] / s0]
    idx = {(0, 0): 6, (0, 1): 7, (1, 1): 8, (0, 2): 9, (1, 2): 10, (2, 2): 11}
    C = [[s[idx[(min(i, j), max(i, j))]] / s0 - m[i] * m[j] for j in range(3)] for i in range(3)]
    norm = math.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
    c = [x / norm for x in m] if norm > 0 else [1.0, 0.0, 0.0]
    lat, lon = math.asin(max(-1.0, min(1.0, c[2]))), math.atan2(c[1], c[0])
    e = [-math.sin(lon), math.cos(lon), 0.0]
    n = [-math.sin(lat) * math.cos(lon), -math.sin(lat) * math.sin(lon), math.cos(lat)]
    quad = lambda u, v: sum(u[i] * C[i][j] * v[j] for i in range(3) for j in range(3))  # noqa: E731
    a, b, d = quad(e, e), quad(e, n), quad(n, n)
    rad = math.sqrt(((a - d) / 2) ** 2 + b * b)
    return max((a + d) / 2 + rad, 0.0), max((a + d) / 2 - rad, 0.0)


def keep_flags(rows, srows, criteria):
    """rows [n, 10], srows [n, 12] of one sample; criteria: two (min_pixels, min_area, min_len2, min_aspect2) -> list of bool"""
    out = []
    for r, s in zip(np.asarray(rows).tolist(), srows):
        mp, ma, ml, mq = (criteria[int(r[1]) - 1][k] for k in range(4))
        ok = True
        if mp > 0 and r[2] < mp:
            ok = False
        if ma > 0 and r[3] < ma:
            ok = False
        if ml > 0 or mq > 0:
            lam = eigenvalues(s, r[3])
            if ml > 0 and not (lam is not None and 12.0 * lam[0] >= ml):
                ok = False
            if mq > 0 and not (lam is not None and lam[0] >= mq * lam[1]):
                ok = False
        out.append(ok)
    return out


def margins(rows, srows, criteria):
    """per event the relative distances of 12 lambda+ and lambda+ / lambda- from the ACTIVE thresholds of its class (what the GPU test's
    precondition bounds from below); events whose zeroth moment is 0 have none (they fail by rule, not by comparison)"""
    out = []
    for r, s in zip(np.asarray(rows).tolist(), srows):
        _, _, ml, mq = (criteria[int(r[1]) - 1][k] for k in range(4))
        lam = eigenvalues(s, r[3])
        if lam is None:
            continue
        if ml > 0:
            out.append(abs(12.0 * lam[0] - ml) / ml)
        if mq > 0:
            ratio = lam[0] / lam[1] if lam[1] > 0 else (math.inf if lam[0] > 0 else 1.0)     # 0 / 0: a point, as wide as long
            out.append(abs(ratio - mq) / mq)
    return out


def reference(mask, n_valid, connectivity, wrap, tables, shape_tables, cap, criteria=None):
    """mask uint8 [B, H, W] -> dict of the first n_valid samples: labels, table, ncomp, rows (uncapped, per sample), shape int64
    [n_valid, cap, 12], srows (uncapped, per sample) and, with criteria, keep uint8 [n_valid, cap], flags (uncapped lists), out_mask uint8
    [n_valid, H, W], counts int64 [n_valid, 2, 4] (per class: events kept, dropped among ranks < cap; pixels kept, dropped)."""
    mask = np.asarray(mask)
    labels, table, ncomp, every = ue.catalogue(mask, n_valid, connectivity, wrap, *tables, cap)
    rowt, colt = shape_tables
    H, W = mask.shape[1:]
    shape = np.zeros((n_valid, cap, FIELDS), np.int64)
    srows = []
    for b in range(n_valid):
        s = shape_rows(labels[b], every[b], wrap, rowt, colt)
        srows.append(s)
        k = min(len(s), cap)
        shape[b, :k] = s[:k]
    ref = {"labels": labels, "table": table, "ncomp": ncomp, "rows": every, "shape": shape, "srows": srows}
    if criteria is None:
        return ref
    keep = np.zeros((n_valid, cap), np.uint8)
    out = mask[:n_valid].copy()
    counts = np.zeros((n_valid, 2, 4), np.int64)
    flags = []
    for b in range(n_valid):
        fl = keep_flags(every[b], srows[b].tolist(), criteria)
        flags.append(fl)
        lab = labels[b]
        for k, (r, f) in enumerate(zip(every[b].tolist(), fl)):
            cls = int(r[1]) - 1
            if k >= cap:
                counts[b, cls, 2] += r[2]             # no row: nothing was evaluated, the pixels stay
                continue
            keep[b, k] = int(f)
            counts[b, cls, 0 if f else 1] += 1
            counts[b, cls, 2 if f else 3] += r[2]
            if not f:
                out[b][lab == r[0] + 1] = 0
    ref.update({"keep": keep, "flags": flags, "out_mask": out, "counts": counts})
    return ref
