"""The frame renderer's checker: the rule of include/deepcam_hip.h (dc_render_frames) in numpy, written from the rule and not from the
kernel.  Outlines through np.roll (periodic columns) and shifted slices (rows that exist), the colour index in float32 with one rounding
per operation, the blends on integer arrays.  One 768 x 1152 frame takes a fraction of a second."""
import numpy as np

COLOURS = {"missing": 0x404040, "line": 0x50FFFFFF, "class1": 0xFFFF4030, "class2": 0xFFFFE040}


def edges(mask, k):
    """bool [H, W]: pixels of class k with a 4-neighbour that is not of class k; rows r +- 1 only where they exist, columns periodic"""
    m = np.asarray(mask) == k
    other = ~np.roll(m, 1, axis=1) | ~np.roll(m, -1, axis=1)
    other[1:] |= ~m[:-1]
    other[:-1] |= ~m[1:]
    return m & other


def outline(mask, k, width):
    """bool [H, W]: pixels with an edge pixel of class k within (width - 1) / 2 rows and columns (columns periodic, rows in range)"""
    R = (width - 1) // 2
    e = edges(mask, k)
    hor = np.zeros_like(e)
    for dx in range(-R, R + 1):
        hor |= np.roll(e, dx, axis=1)
    out = hor.copy()
    for dy in range(1, R + 1):
        out[dy:] |= hor[:-dy]
        out[:-dy] |= hor[dy:]
    return out


def colour_index(values, lo, scale, nlut):
    """(index int64, finite bool) of float32 values: t = fl32(fl32(v - lo) * scale); 0 unless t > 0, nlut - 1 if t >= 1, else
    min(nlut - 1, (int)fl32(t * nlut))"""
    v = np.asarray(values, np.float32)
    finite = np.isfinite(v)
    with np.errstate(all="ignore"):
        t = (np.where(finite, v, np.float32(0)) - np.float32(lo)) * np.float32(scale)
        assert t.dtype == np.float32
        inside = (t > 0) & (t < 1)
        mid = (np.where(inside, t, np.float32(0)) * np.float32(nlut)).astype(np.int64)
    idx = np.where(t >= 1, nlut - 1, np.where(inside, np.minimum(nlut - 1, mid), 0))
    return idx.astype(np.int64), finite


def _rgb(v):
    return np.asarray([(v >> 16) & 255, (v >> 8) & 255, v & 255], np.int64)


def blend(rgb, where, argb):
    """rgb int64 [..., 3]; where bool [...]: every channel (fg * a + old * (255 - a) + 127) / 255 there"""
    a = (argb >> 24) & 255
    mixed = (_rgb(argb) * a + rgb * (255 - a) + 127) // 255
    return np.where(where[..., None], mixed, rgb)


def render(fields, ch, lo, scale, lut, masks, src_row, shift, row_line, col_line, width, colours=None, n_valid=None):
    """uint8 [n_valid, P, Ho, W, 3] for fields float32 [B, H, W, ldc] and masks = one or two integer arrays [B, H, W]"""
    col = dict(COLOURS, **(colours or {}))
    fields = np.asarray(fields, np.float32)
    B, H, W = fields.shape[:3]
    nv = B if n_valid is None else n_valid
    lut = np.asarray(lut, np.uint8).astype(np.int64)
    r = np.clip(np.asarray(src_row, np.int64), 0, H - 1)
    c = (np.arange(W) + shift) % W
    line = (np.asarray(row_line) != 0)[:, None] | (np.asarray(col_line) != 0)[None, :]
    out = np.zeros((nv, len(masks), len(r), W, 3), np.uint8)
    for b in range(nv):
        idx, finite = colour_index(fields[b, :, :, ch], lo, scale, len(lut))
        src = np.where(finite[..., None], lut[idx], _rgb(col["missing"]))
        base = blend(src[r][:, c], line, col["line"])
        for p, m in enumerate(masks):
            rgb = base
            for k, name in ((1, "class1"), (2, "class2")):
                rgb = blend(rgb, outline(np.asarray(m[b]), k, width)[r][:, c], col[name])
            out[b, p] = rgb.astype(np.uint8)
    return out
