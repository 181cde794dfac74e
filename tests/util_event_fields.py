"""Checker of the per-event field statistics (nn.EventFields, dc_component_fields): the definition of include/deepcam_hip.h implemented
literally, a plain loop over pixels and channels on Python integers, on top of the flood fill of tests/util_events.py (labels, ranks).

Row (rank k, channel ch) = min, max, sum, wsum, nonfinite, saturated.  For every foreground pixel p = r * W + c whose component has rank
k < cap and every channel value v:  NaN / +-Inf: nonfinite += 1, nothing else.  key(v) = bits ^ 0xFFFFFFFF for a set sign bit, else
bits | 0x80000000.  min = the unsigned minimum of (key << 32) | p, empty 2^64 - 1; max = the unsigned maximum of (key << 32) |
(0xFFFFFFFF - p), empty 0.  q = rint(ldexp(double(v), bits[ch])); |q| > 2^40: saturated += 1, no part in the sums; else sum += q and
wsum += rint(ldexp(double(v), bits[ch]) * (double(wy[r]) * 2^-20))."""
import numpy as np

import util_events as ue

STATS = 6
EMPTY_ROW = (-1, 0, 0, 0, 0, 0)
LIMIT = float(2 ** 40)


def key(v) -> int:
    """the order-preserving 32-bit key of one float32 value"""
    bits = int(np.float32(v).view(np.uint32))
    return bits ^ 0xFFFFFFFF if bits & 0x80000000 else bits | 0x80000000


def unkey(k: int) -> np.float32:
    bits = k ^ 0x80000000 if k & 0x80000000 else k ^ 0xFFFFFFFF
    return np.uint32(bits).view(np.float32)


def signed(word: int) -> int:
    """an unsigned 64-bit word as the int64 that holds its bits"""
    return word - (1 << 64) if word >= 1 << 63 else word


def field_rows(labels, rows, cap, fields, C, bits, wy):
    """One sample.  labels int32 [H, W] and rows [n, 10] in root order (ue.label_one), fields float32 [H, W, ldc] -> int64 [cap, C, 6].
    The per-value quantities (key, q, the weighted product) are evaluated elementwise by numpy, the reduction is the plain loop."""
    H, W = labels.shape
    v = np.ascontiguousarray(np.asarray(fields, np.float32)[:, :, :C])
    u = v.view(np.uint32).astype(np.int64)
    keys = np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000).tolist()
    finite = np.isfinite(v).tolist()
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.ldexp(v.astype(np.float64), np.asarray(bits, np.int32)[:C])                   # exact: a power of two
        q = np.rint(s)
        wf = np.asarray(wy, np.int64).astype(np.float64) * np.float64(2.0 ** -20)              # exact
        wq = np.rint(s * wf[:, None, None])                                                    # one rounded product, then rint
        fits = np.abs(q) <= LIMIT
        q, wq = np.where(fits, q, 0).astype(np.int64).tolist(), np.where(fits, wq, 0).astype(np.int64).tolist()
    fits = fits.tolist()
    rank = {int(r[0]): k for k, r in enumerate(rows)}
    lo = [[(1 << 64) - 1] * C for _ in range(cap)]
    hi = [[0] * C for _ in range(cap)]
    acc = [[[0, 0, 0, 0] for _ in range(C)] for _ in range(cap)]             # sum, wsum, nonfinite, saturated
    lab = labels.tolist()
    for r in range(H):
        for c in range(W):
            if lab[r][c] <= 0:
                continue
            k = rank[lab[r][c] - 1]
            if k < 0 or k >= cap:
                continue
            p = r * W + c
            for ch in range(C):
                a = acc[k][ch]
                if not finite[r][c][ch]:
                    a[2] += 1
                    continue
                kv = keys[r][c][ch]
                lo[k][ch] = min(lo[k][ch], (kv << 32) | p)
                hi[k][ch] = max(hi[k][ch], (kv << 32) | (0xFFFFFFFF - p))
                if not fits[r][c][ch]:
                    a[3] += 1
                    continue
                a[0] += q[r][c][ch]
                a[1] += wq[r][c][ch]
    out = np.empty((cap, C, STATS), np.int64)
    out[:] = EMPTY_ROW
    for k in range(min(cap, len(rows))):
        for ch in range(C):
            out[k, ch] = [signed(lo[k][ch]), signed(hi[k][ch])] + acc[k][ch]
    return out


def field_table(mask, n_valid, connectivity, wrap, wy, cx, sx, cap, fields, C, bits):
    """mask uint8 [B, H, W], fields float32 [B, H, W, ldc] -> (ftable int64 [n_valid, cap, C, 6], the catalogue of ue.catalogue)"""
    cat = ue.catalogue(mask, n_valid, connectivity, wrap, wy, cx, sx, cap)
    labels, every = cat[0], cat[3]
    ftable = np.stack([field_rows(labels[b], every[b], cap, np.asarray(fields[b]), C, bits, wy) for b in range(n_valid)])
    return ftable, cat


VALUES = ("min", "min_lat", "min_lon", "max", "max_lat", "max_lon", "mean", "area_mean")


def values_from_decode(decoded, C):
    """nn.EventFields.decode's dicts -> float64 [n, C, 8] (VALUES), NaN for None: what nn.EventFields.values must equal"""
    out = np.full((len(decoded), C, len(VALUES)), np.nan, np.float64)
    for k, per in enumerate(decoded):
        for ch, d in enumerate(per):
            out[k, ch] = [np.nan if d[name] is None else d[name] for name in VALUES]
    return out
