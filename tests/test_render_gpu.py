"""The frame renderer on the GPU (dc_render_frames of csrc/render.hip, nn.FrameRenderer, predict.py --plots, train.py --plots) against the
numpy checker of tests/util_render.py.  The picture is integer arithmetic behind a colour index of two separately rounded fp32
operations that numpy repeats: every comparison is equality of bytes, without a tolerance.

Shapes come from the kernel's own source tile (dc_render_tile): the smallest frame the call takes, a frame with ragged tiles on both
axes, one of whole tiles, and the drivers' small frame.  The combinations are hand-picked, not the full product: every mask on every
shape, every width and every row table on every shape, and every mask type, field layout, shift and panel count spread over them."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from mlperf_deepcam_amd import png  # noqa: E402
import util_render as ur  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
GUARD = 256                                        # bytes behind `out` that no launch may touch
LO, HI = -3.5, 12.25
SCALE = np.float32(1.0) / (np.float32(HI) - np.float32(LO))
COLOURS = ur.COLOURS


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_render_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


TH, TW = _tile()
SHAPES = {"min": (5, 8), "ragged": (TH + 3, TW + 4), "tiles": (2 * TH, 2 * TW), "small": (64, 96)}
MASKS = ["empty", "all1", "pixel", "seam", "stripe", "checker", "poles", "random"]
WIDTHS = [1, 3, 7]
DTYPES = [np.uint8, np.int32, np.int64]
LAYOUTS = [(1, 0), (16, 0), (5, 3)]                # (ldc, ch)
ROWS = ["identity", "flipped", "repeat", "zigzag", "clamped"]
SHIFTS = ["0", "half", "3"]


def _mask(name, H, W, seed=0):
    """uint8 [H, W]"""
    rs = np.random.RandomState(zlib.crc32(f"{name} {H} {W} {seed}".encode()))
    m = np.zeros((H, W), np.uint8)
    if name == "all1":
        m[:] = 1
    elif name == "pixel":
        m[rs.randint(0, H), rs.randint(0, W)] = 1 + seed % 2
    elif name == "seam":                           # a block across the seam
        m[1:H - 1, [W - 2, W - 1, 0]] = 1 + seed % 2
    elif name == "stripe":                         # through every tile border, on both sides of it
        m[:, [c for c in range(W) if c % TW in (0, TW - 1)]] = 1
        m[[r for r in range(H) if r % TH in (0, TH - 1)], :] = 2
        m[H // 2, :] = 1
    elif name == "checker":
        rr, cc = np.mgrid[0:H, 0:W]
        m[:] = 1 + (rr + cc + seed) % 2
    elif name == "poles":                          # regions that touch the first and the last row
        m[0:2, 1:W - 2] = 2
        m[H - 2:H, 0:W // 2] = 1
        m[0, W - 1] = 1
    elif name == "random":
        m[:] = rs.choice(np.asarray([0, 1, 2, 3, 255], np.uint8), size=(H, W), p=[0.5, 0.2, 0.2, 0.05, 0.05])
    elif name != "empty":
        raise KeyError(name)
    return m


def _typed(m, dtype, seed=0):
    """the mask in a wider type: 255 becomes -1, and part of the background takes values whose low byte or low word is a class"""
    if dtype == np.uint8:
        return m
    rs = np.random.RandomState(77 + seed)
    w = m.astype(np.int64)
    w[m == 255] = -1
    odd = [0, 0, -1, 3, 257, 258, -255] + ([(1 << 32) + 1, (1 << 40) + 2, -(1 << 32) + 1] if dtype == np.int64 else [65537, (1 << 24) + 2])
    w = np.where(m == 0, rs.choice(np.asarray(odd, np.int64), size=m.shape), w)
    return w.astype(dtype)


def _rows(name, H):
    if name == "identity":
        return np.arange(H, dtype=np.int32)
    if name == "flipped":
        return np.arange(H - 1, -1, -1, dtype=np.int32)
    if name == "repeat":                           # repeated and skipped rows, Ho != H
        return np.asarray(sorted(list(range(0, H, 3)) * 2 + [H - 1] * 3), np.int32)
    if name == "zigzag":                           # not monotone
        rs = np.random.RandomState(H)
        return rs.randint(0, H, size=H + 5).astype(np.int32)
    if name == "clamped":                          # entries outside [0, H - 1]
        return np.asarray([-5, -1] + list(range(H)) + [H, H + 5, -(1 << 31), (1 << 31) - 1], np.int64).astype(np.int32)
    raise KeyError(name)


def _shift(name, W):
    return {"0": 0, "half": W // 2, "3": 3}[name]


@functools.lru_cache(maxsize=None)
def _fields(B, H, W, ldc, seed=0):
    """float32 [B, H, W, ldc] around [LO, HI] with values outside it and a few non-finite ones; callers do not modify it"""
    rs = np.random.RandomState(zlib.crc32(f"fields {B} {H} {W} {ldc} {seed}".encode()))
    f = (LO + (HI - LO) * (1.4 * rs.random_sample((B, H, W, ldc)) - 0.2)).astype(np.float32)
    k = max(B * H * W * ldc // 50, 3)
    flat = f.reshape(-1)
    flat[rs.randint(0, flat.size, k)] = rs.choice(np.asarray([np.nan, np.inf, -np.inf, -0.0, LO, HI], np.float32), size=k)
    return f


@functools.lru_cache(maxsize=None)
def _lines(Ho, W, seed=0):
    rs = np.random.RandomState(Ho * 131 + W + seed)
    rl = (rs.random_sample(Ho) < 0.15).astype(np.uint8) * rs.randint(1, 256, Ho).astype(np.uint8)      # any non-zero value is a line
    cl = (rs.random_sample(W) < 0.15).astype(np.uint8) * rs.randint(1, 256, W).astype(np.uint8)
    return rl, cl


def _render(fields, ch, lo, scale, lut, masks, rows, shift, row_line, col_line, width, n_valid=None, colours=None, names=None, offset=0):
    """dc_render_frames on an `out` pre-filled with the sentinel (`offset` bytes off its allocation); returns (out uint8
    [B, P, Ho, W, 3], the guard bytes behind it) on the host"""
    B, H, W, ldc = fields.shape
    nv = B if n_valid is None else n_valid
    P, Ho = len(masks), len(rows)
    col = dict(COLOURS, **(colours or {}))
    signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v  # noqa: E731
    n = B * P * Ho * W * 3
    store = torch.full((offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = store[offset:]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    f, lt, rw, rl, cl = dev(fields), dev(np.asarray(lut, np.uint8)), dev(np.asarray(rows, np.int32)), dev(row_line), dev(col_line)
    ms = [dev(m) for m in masks]
    ws_bytes = L.load().dc_render_workspace(B, P, H, W)
    assert ws_bytes >= B * P * H * W and ws_bytes % 256 == 0
    ws = torch.full((ws_bytes,), 0x3, dtype=torch.uint8, device=DEV)                                   # stale outline bits everywhere
    args = (B, nv, H, W, L.dptr(f), ch, ldc, float(lo), float(scale), L.dptr(lt), len(lut), L.dptr(ms[0]), ms[0].element_size(),
            L.dptr(ms[1]) if P == 2 else None, ms[1].element_size() if P == 2 else 0, L.dptr(rw), Ho, shift, L.dptr(rl), L.dptr(cl),
            signed(col["missing"]), signed(col["line"]), signed(col["class1"]), signed(col["class2"]), width, L.dptr(out), L.dptr(ws),
            L.stream_ptr())
    if names is None:
        L.call("dc_render_frames", *args)
    else:
        with served("dc_render_frames") as got:
            L.call("dc_render_frames", *args)
        names.extend(got)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[:n].reshape(B, P, Ho, W, 3), host[n:]


def _assert_equal(got, ref, nv=None):
    out, guard = got
    nv = len(ref) if nv is None else nv
    if not np.array_equal(out[:nv], ref):
        bad = np.argwhere((out[:nv] != ref).any(axis=4))
        raise AssertionError(f"{len(bad)} pixels differ, first (b, p, y, x) {bad[:4].tolist()}: got {out[:nv][tuple(bad[0])].tolist()}, "
                             f"want {ref[tuple(bad[0])].tolist()}")
    assert (out[nv:] == SENTINEL).all(), "the padding samples' pixels were written"
    assert (guard == SENTINEL).all(), "bytes behind the output were written"


def _case(shape, mask, width, panels, dtype, layout, rows, shift):
    """one comparison: B = 2 samples with their own masks; the second panel (if any) is the random mask in another type"""
    H, W = SHAPES[shape]
    ldc, ch = layout
    B = 2
    f = _fields(B, H, W, ldc)
    a = np.stack([_typed(_mask(mask, H, W, b), dtype, b) for b in range(B)])
    masks = [a]
    if panels == 2:
        other = DTYPES[(DTYPES.index(dtype) + 1) % 3]
        masks.append(np.stack([_typed(_mask("random", H, W, 10 + b), other, b) for b in range(B)]))
    rw = _rows(rows, H)
    rl, cl = _lines(len(rw), W)
    lut = dnn.render_palette()
    sh = _shift(shift, W)
    ref = ur.render(f, ch, LO, SCALE, lut, masks, rw, sh, rl, cl, width)
    _assert_equal(_render(f, ch, LO, SCALE, lut, masks, rw, sh, rl, cl, width), ref)
    return ref, masks


def _cases():
    out = []
    k = 0
    for shape in SHAPES:                           # every mask on every shape; the other axes cycle with different periods
        for mask in MASKS:
            out.append((shape, mask, WIDTHS[k % 3], 1 + (k // 3) % 2, DTYPES[(k // 2) % 3], LAYOUTS[(k // 4 + k) % 3], ROWS[k % 5],
                        SHIFTS[(k // 5 + k) % 3]))
            k += 1
    for shape in SHAPES:                           # every width and every row table on every shape, on the masks that stress them
        for i, width in enumerate(WIDTHS):
            out.append((shape, "random", width, 2, DTYPES[i], LAYOUTS[(i + 1) % 3], ROWS[(i + 2) % 5], SHIFTS[i]))
            out.append((shape, "stripe", width, 1, DTYPES[(i + 1) % 3], LAYOUTS[i], "identity", SHIFTS[(i + 1) % 3]))
        for i, rows in enumerate(ROWS):
            out.append((shape, "poles", WIDTHS[(i + 1) % 3], 1 + i % 2, DTYPES[i % 3], LAYOUTS[(i + 2) % 3], rows, SHIFTS[(i + 2) % 3]))
    for i, dtype in enumerate(DTYPES):             # every mask type with every layout and shift at the ragged shape
        for j, layout in enumerate(LAYOUTS):
            out.append(("ragged", "seam" if j else "checker", WIDTHS[(i + j) % 3], 2, dtype, layout, ROWS[(i * 3 + j) % 5], SHIFTS[(i + j + 1) % 3]))
    seen, uniq = set(), []
    for c in out:
        key = tuple(str(v) for v in c)
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


CASES = _cases()


def _id(c):
    shape, mask, width, panels, dtype, layout, rows, shift = c
    return f"{shape}-{mask}-w{width}-p{panels}-{np.dtype(dtype).name}-ld{layout[0]}c{layout[1]}-{rows}-s{shift}"


# ------------------------------------------------------------------------------------------------------------------ 1. kernels vs checker
def test_the_case_table_covers_what_it_claims():
    assert len(CASES) <= 150
    for shape in SHAPES:
        mine = [c for c in CASES if c[0] == shape]
        assert {c[1] for c in mine} == set(MASKS) and {c[2] for c in mine} == set(WIDTHS) and {c[6] for c in mine} == set(ROWS)
        assert {c[3] for c in mine} == {1, 2} and {c[7] for c in mine} == set(SHIFTS)
        assert {c[4] for c in mine} == set(DTYPES) and {c[5] for c in mine} == set(LAYOUTS)
    assert {(c[4], c[5]) for c in CASES} == {(d, l) for d in DTYPES for l in LAYOUTS}
    assert SHAPES["ragged"][0] % TH and SHAPES["ragged"][1] % TW and SHAPES["ragged"][1] % 4 == 0 and SHAPES["tiles"] == (2 * TH, 2 * TW)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_frames_vs_checker(case):
    ref, masks = _case(*case)
    shape, mask, width = case[:3]
    if mask == "empty":                            # the checker itself: no class, no outline colour anywhere
        assert not ur.outline(masks[0][0], 1, width).any() and not ur.outline(masks[0][0], 2, width).any()
    if mask == "all1" and case[3] == 1:            # one class over the periodic field: edges only where rows end ... which do not count
        assert not ur.outline(masks[0][0], 1, width).any()


@pytest.mark.parametrize("W", [9, 10, 11, 70])
@pytest.mark.parametrize("width", [3, 7])
def test_widths_that_are_no_multiple_of_four_take_the_byte_stores(W, width):
    H, B = 7, 2
    f = _fields(B, H, W, 3)
    masks = [np.stack([_mask("random", H, W, b) for b in range(B)]), np.stack([_typed(_mask("seam", H, W, b), np.int64, b) for b in range(B)])]
    rw = _rows("repeat", H)
    rl, cl = _lines(len(rw), W)
    lut = dnn.render_palette(50)
    for shift in (0, W // 2, W - 1):
        ref = ur.render(f, 2, LO, SCALE, lut, masks, rw, shift, rl, cl, width)
        _assert_equal(_render(f, 2, LO, SCALE, lut, masks, rw, shift, rl, cl, width), ref)


def test_an_output_that_is_not_word_aligned_takes_the_byte_stores():
    H, W = SHAPES["ragged"]
    f = _fields(1, H, W, 16)
    masks = [_mask("random", H, W)[None]]
    rw = _rows("flipped", H)
    rl, cl = _lines(len(rw), W)
    lut = dnn.render_palette()
    ref = ur.render(f, 0, LO, SCALE, lut, masks, rw, 4, rl, cl, 3)
    for offset in (1, 2, 3):
        _assert_equal(_render(f, 0, LO, SCALE, lut, masks, rw, 4, rl, cl, 3, offset=offset), ref)


# ------------------------------------------------------------------------------------------------------------------ 2. the colour index
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-2.5, 7.3), (250.0, 330.0)], ids=["unit", "mixed", "kelvin"])
@pytest.mark.parametrize("nlut", [1, 50, 64, 256])
def test_colour_index_at_the_bin_edges(nlut, lo, hi):
    lo32, hi32 = np.float32(lo), np.float32(hi)
    scale = np.float32(1.0) / (hi32 - lo32)
    edges64 = lo + np.arange(nlut + 1, dtype=np.float64) * (hi - lo) / nlut
    edges32 = (lo32 + np.arange(nlut + 1, dtype=np.float32) * ((hi32 - lo32) / np.float32(nlut))).astype(np.float32)
    mids = (lo + (np.arange(nlut, dtype=np.float64) + 0.5) * (hi - lo) / nlut).astype(np.float32)       # one value well inside every bin
    e = np.concatenate([edges64.astype(np.float32), edges32, mids])
    vals = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)),
                           np.asarray([lo - 1.0, lo - 1e30, hi + 1.0, hi + 1e30, 3e38, -3e38, np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45,
                                       -1e-45], np.float32)]).astype(np.float32)
    W = 16
    H = -(-len(vals) // W)
    f = np.full((1, H, W, 2), np.nan, np.float32)
    f.reshape(-1, 2)[:len(vals), 1] = vals
    rs = np.random.RandomState(nlut)
    lut = rs.randint(0, 256, (nlut, 3)).astype(np.uint8)
    lut[:, 0] = np.arange(nlut)                    # the red byte is the index
    masks = [np.zeros((1, H, W), np.uint8)]
    rw, none_r, none_c = _rows("identity", H), np.zeros(H, np.uint8), np.zeros(W, np.uint8)
    ref = ur.render(f, 1, lo32, scale, lut, masks, rw, 0, none_r, none_c, 1)
    got = _render(f, 1, lo32, scale, lut, masks, rw, 0, none_r, none_c, 1)
    _assert_equal(got, ref)
    red = got[0][0, 0, :, :, 0].reshape(-1)[:len(vals)]
    finite = np.isfinite(vals)
    assert (got[0][0, 0].reshape(-1, 3)[:len(vals)][~finite] == [0x40, 0x40, 0x40]).all() and int((~finite).sum()) == 4
    assert set(red[finite].tolist()) == set(range(nlut))                                   # every entry is reached
    below, above = finite & (vals <= lo32), finite & (vals >= hi32)
    assert (red[below] == 0).all() and (red[above] == nlut - 1).all() and below.sum() >= 4 and above.sum() >= 4
    order = np.argsort(vals[finite], kind="stable")
    assert (np.diff(red[finite][order].astype(int)) >= 0).all()                            # the index never falls as the value grows


# ------------------------------------------------------------------------------------------------------------------ 3. other kernel cases
def test_padding_samples_are_neither_read_nor_written():
    H, W = SHAPES["ragged"]
    B, nv = 3, 2
    f = _fields(B, H, W, 16).copy()
    f[nv:] = np.nan
    masks = [np.stack([_mask("random", H, W, b) for b in range(B)]), np.stack([_mask("poles", H, W, b) for b in range(B)])]
    for m in masks:
        m[nv:] = 255
    rw = _rows("repeat", H)
    rl, cl = _lines(len(rw), W)
    lut = dnn.render_palette()
    ref = ur.render(f, 0, LO, SCALE, lut, masks, rw, W // 2, rl, cl, 3, n_valid=nv)
    assert ref.shape[0] == nv
    _assert_equal(_render(f, 0, LO, SCALE, lut, masks, rw, W // 2, rl, cl, 3, n_valid=nv), ref, nv=nv)
    one = ur.render(f, 0, LO, SCALE, lut, masks[:1], rw, W // 2, rl, cl, 3, n_valid=1)
    _assert_equal(_render(f, 0, LO, SCALE, lut, masks[:1], rw, W // 2, rl, cl, 3, n_valid=1), one, nv=1)


def test_two_calls_with_another_mask_in_between_agree():
    H, W = SHAPES["tiles"]
    B = 2
    r = dnn.FrameRenderer(B, H, W, channel=0, ldc=16, lo=LO, hi=HI, projection="plate", outline=7, panels=2)
    f = torch.from_numpy(_fields(B, H, W, 16)).to(DEV)
    a = torch.from_numpy(np.stack([_mask("random", H, W, b) for b in range(B)])).to(DEV)
    b = torch.from_numpy(np.stack([_mask("poles", H, W, b) for b in range(B)])).to(DEV)
    full = torch.from_numpy(np.stack([_mask("checker", H, W, b) for b in range(B)])).to(DEV)
    first = r(f, a, b).clone()
    other = r(f, full, full).clone()               # outlines on every pixel: what the next call must not inherit
    again = r(f, a, b)
    torch.cuda.synchronize()
    assert not torch.equal(other, first) and torch.equal(again, first)
    ref = ur.render(_fields(B, H, W, 16), 0, LO, SCALE, r.palette, [a.cpu().numpy(), b.cpu().numpy()], r.rows, r.shift, *r.lines, 7)
    assert np.array_equal(first.cpu().numpy().reshape(ref.shape), ref)


def test_the_launches_are_named():
    H, W = SHAPES["ragged"]
    f = _fields(1, H, W, 16)
    rw = _rows("identity", H)
    rl, cl = _lines(len(rw), W)
    for masks in ([_mask("random", H, W)[None]], [_mask("random", H, W)[None], _mask("seam", H, W)[None]]):
        names = []
        _render(f, 0, LO, SCALE, dnn.render_palette(), masks, rw, 0, rl, cl, 3, names=names)
        assert names == ["render_paint", "render_gather"]
    names = []
    _render(_fields(1, 7, 10, 3), 0, LO, SCALE, dnn.render_palette(), [_mask("random", 7, 10)[None]], _rows("identity", 7), 0, *_lines(7, 10), 3,
            names=names)
    assert names == ["render_paint", "render_gather"]                                      # the byte-store form carries the same name


def test_argument_errors_leave_a_message():
    lib = L.load()
    H, W, B = 5, 8, 2
    buf = torch.zeros(1 << 14, dtype=torch.int64, device=DEV)                              # read as fields, masks and tables: all zero
    out = torch.full((B * 2 * H * W * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(max(lib.dc_render_workspace(B, 2, H, W), 256), dtype=torch.uint8, device=DEV)
    p = L.dptr(buf)
    order = (("B", B), ("nv", B), ("H", H), ("W", W), ("fields", p), ("ch", 0), ("ldc", 1), ("lo", 0.0), ("scale", 1.0), ("lut", p),
             ("nlut", 4), ("mask_a", p), ("a_bytes", 1), ("mask_b", p), ("b_bytes", 8), ("rows", p), ("Ho", H), ("shift", 0), ("row_line", p),
             ("col_line", p), ("missing", 0), ("line", 0), ("c1", -1), ("c2", -1), ("width", 3), ("out", L.dptr(out)), ("ws", L.dptr(ws)),
             ("st", None))
    rf = lambda **kw: lib.dc_render_frames(*[kw.get(k, v) for k, v in order])  # noqa: E731
    assert not set(k for k, _ in order) - {"B", "nv", "H", "W", "fields", "ch", "ldc", "lo", "scale", "lut", "nlut", "mask_a", "a_bytes",
                                           "mask_b", "b_bytes", "rows", "Ho", "shift", "row_line", "col_line", "missing", "line", "c1", "c2",
                                           "width", "out", "ws", "st"}
    for kw, word in (({"width": 2}, "width"), ({"width": 4}, "width"), ({"width": 9}, "width"), ({"width": 0}, "width"),
                     ({"nlut": 0}, "nlut"), ({"nlut": 257}, "nlut"), ({"ch": 1}, "ch"), ({"ch": 16, "ldc": 16}, "ch"), ({"ch": -1}, "ch"),
                     ({"shift": W}, "shift"), ({"shift": -1}, "shift"), ({"a_bytes": 2}, "a_bytes"), ({"b_bytes": 2}, "b_bytes"),
                     ({"W": 4}, "W"), ({"nv": 0}, "n_valid"), ({"nv": B + 1}, "n_valid"), ({"out": None}, "null"), ({"fields": None}, "null"),
                     ({"ws": None}, "null"), ({"Ho": 0}, "Ho"), ({"H": 0}, "H")):
        assert rf(**kw) != 0, kw
        assert word in L.last_error(), (kw, L.last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                   # nothing was launched
    assert lib.dc_render_workspace(0, 1, H, W) == 0 and lib.dc_render_workspace(1, 3, H, W) == 0 and lib.dc_render_workspace(1, 0, H, W) == 0
    assert lib.dc_render_workspace(1, 1, H, 4) == 0 and lib.dc_render_workspace(1, 1, 0, W) == 0 and lib.dc_render_workspace(1, 2, 65536, 32768) == 0
    assert lib.dc_render_tile(None, None) != 0 and "null" in L.last_error()
    assert rf() == 0, L.last_error()                                                       # the same arguments, complete: two empty panels
    torch.cuda.synchronize()
    n = B * 2 * H * W * 3
    assert bool((out[:n] == 0).all()) and bool((out[n:] == SENTINEL).all())                # lut[0] = (0, 0, 0) everywhere, nothing behind


# ------------------------------------------------------------------------------------------------------------------ 4. nn.FrameRenderer
def test_frame_renderer_end_to_end_with_the_gall_table():
    H, W = SHAPES["small"]
    B, nv = 3, 2
    fields = _fields(B, H, W, 16)
    pred = np.stack([_mask("random", H, W, b) for b in range(B)])
    label = np.stack([_typed(_mask("poles" if b else "seam", H, W, b), np.int64, b) for b in range(B)])
    r = dnn.FrameRenderer(B, H, W, channel=0, ldc=16, lo=LO, hi=HI)
    assert r.Ho == 74 and np.array_equal(r.rows, dnn.gall_rows(H, W)) and r.shift == W // 2 and r.outline == 3 and r.P == 2
    assert np.array_equal(r.palette, dnn.render_palette()) and r.lines[0].sum() == 5 and r.lines[1].sum() == 6
    out = r(torch.from_numpy(fields).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), n_valid=nv)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (nv, 2 * r.Ho, W, 3)
    ref = ur.render(fields, 0, np.float32(r.lo), np.float32(r.scale), r.palette, [pred, label], r.rows, r.shift, *r.lines, 3, n_valid=nv)
    assert np.array_equal(out.cpu().numpy(), ref.reshape(nv, 2 * r.Ho, W, 3))
    assert np.float32(r.scale) == SCALE and r.colours == ur.COLOURS
    # one panel, the plate table, another channel and other colours
    own = {"class1": 0x8000FF00, "line": 0xFF000000}
    r1 = dnn.FrameRenderer(B, H, W, channel=3, ldc=16, lo=LO, hi=HI, projection="plate", outline=1, panels=1, colours=own, shift=5,
                           palette=dnn.render_palette(256))
    out1 = r1(torch.from_numpy(fields).to(DEV), torch.from_numpy(label).to(DEV))
    ref1 = ur.render(fields, 3, np.float32(LO), SCALE, dnn.render_palette(256), [label], dnn.plate_rows(H), 5, *r1.lines, 1, colours=own)
    assert tuple(out1.shape) == (B, H, W, 3) and np.array_equal(out1.cpu().numpy(), ref1.reshape(B, H, W, 3))
    table = np.asarray([3, 3, 70, -2, 0], np.int32)
    r2 = dnn.FrameRenderer(B, H, W, lo=LO, hi=HI, projection=table, panels=1, parallels=0, meridians=0)
    out2 = r2(torch.from_numpy(fields).to(DEV), torch.from_numpy(pred).to(DEV))
    ref2 = ur.render(fields, 0, np.float32(LO), SCALE, r2.palette, [pred], table, W // 2, np.zeros(5, np.uint8), np.zeros(W, np.uint8), 3)
    assert np.array_equal(out2.cpu().numpy(), ref2.reshape(B, 5, W, 3))


def test_frame_renderer_refuses_wrong_inputs():
    H, W = SHAPES["small"]
    B = 2
    r = dnn.FrameRenderer(B, H, W, lo=LO, hi=HI)
    f = torch.from_numpy(_fields(B, H, W, 16)).to(DEV)
    m = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    r(f, m, m)
    for bad in (f.double(), f[:, :, :, :4], f[:1], f.cpu(), f.transpose(1, 2)):
        with pytest.raises(L.DeepcamHipError):
            r(bad, m, m)
    for bad in (m.to(torch.int16), m.float(), m[:1], m.cpu(), m.transpose(1, 2), m[:, :, :W - 1]):
        with pytest.raises(L.DeepcamHipError):
            r(f, bad, m)
        with pytest.raises(L.DeepcamHipError):
            r(f, m, bad)
    with pytest.raises(L.DeepcamHipError):
        r(f, m)                                    # two panels were asked for
    with pytest.raises(L.DeepcamHipError):
        r(f, m, m, n_valid=B + 1)
    with pytest.raises(L.DeepcamHipError):
        r(f, m, m, n_valid=0)
    for kw in ({"outline": 2}, {"panels": 3}, {"channel": 16}, {"projection": "mercator"}, {"shift": W}, {"palette": np.zeros((0, 3), np.uint8)},
               {"palette": np.zeros((4, 3), np.float32)}, {"colours": {"class3": 1}}):
        with pytest.raises(L.DeepcamHipError):
            dnn.FrameRenderer(B, H, W, **kw)
    with pytest.raises(L.DeepcamHipError):
        dnn.FrameRenderer(B, H, 4)


def _discs(H, W, n, seed):
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    rr, cc = np.mgrid[0:H, 0:W]
    for _ in range(n):
        r0, c0, rad, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(max(min(H, W) // 40, 2), max(min(H, W) // 10, 4)), rs.randint(1, 3)
        dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
        m[(rr - r0) ** 2 + dc ** 2 <= rad * rad] = cl
    return m


def test_one_full_size_frame():
    H, W = 768, 1152
    rs = np.random.RandomState(2026)
    fields = np.empty((1, H, W, 16), np.float32)
    fields[...] = rs.random_sample((H, W, 1)).astype(np.float32) * np.float32(80.0) + np.linspace(-5, 5, 16, dtype=np.float32)
    fields[0, rs.randint(0, H, 500), rs.randint(0, W, 500), 0] = np.nan
    pred, label = _discs(H, W, 25, 1)[None], _discs(H, W, 25, 2).astype(np.int64)[None]
    r = dnn.FrameRenderer(1, H, W, channel=0, ldc=16, lo=0.0, hi=70.0)
    assert r.Ho == 885
    out = r(torch.from_numpy(fields).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV))
    ref = ur.render(fields, 0, np.float32(r.lo), np.float32(r.scale), r.palette, [pred, label], r.rows, r.shift, *r.lines, 3)
    assert np.array_equal(out.cpu().numpy(), ref.reshape(1, 2 * 885, W, 3))
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 64                                 # table, lines, both outlines and their mixtures


# ------------------------------------------------------------------------------------------------------------------ 5. drivers
def _h5_write(path, datasets):
    """an HDF5 file through whichever backend data.CamDataset reads with; no backend at all is an error, not a skip"""
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with h5.File(path, "w") as f:
        for name, array in datasets.items():
            if backend == "h5py":
                f.create_dataset(name, data=array)
            else:
                f.write(name, array)


def _h5_read(path, name):
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    if backend == "h5py":
        with h5.File(path, "r") as f:
            return f[name][...]
    with h5.File(path) as f:
        return f.read(name)


def _files(tmp_path, n):
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(21)
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(n)]
    truth = [_discs(H, W, 7, 300 + i).astype(np.int64) for i in range(n)]
    names = [f"data-{i:02d}.h5" for i in range(n)]
    for name, d, t in zip(names, fields, truth):
        _h5_write(os.path.join(root, name), {"climate/data": d, "climate/labels_0": t})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    quarter = (hi[2] - lo[2]) / np.float32(4.0)
    lo[2], hi[2] = lo[2] + quarter, hi[2] - quarter                                        # channel 2: values outside the recorded range
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)

    def run(out, *extra):
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
               out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.load(open(os.path.join(out, "summary.json")))

    return run, names, fields, truth, lo, hi


def _picture(field, ch, lo, hi, masks):
    """the checker's picture of one file: Gall rows, default table, graticule, roll by W / 2, width 3; panels stacked"""
    H, W = field.shape[:2]
    rows = dnn.gall_rows(H, W)
    scale = np.float32(1.0) / (np.float32(hi) - np.float32(lo))
    out = ur.render(field[None], ch, np.float32(lo), scale, dnn.render_palette(), [m[None] for m in masks], rows, W // 2,
                    *dnn.graticule(rows, W, W // 2, height=H), 3)
    return out.reshape(len(masks) * len(rows), W, 3)


def test_predict_cli_with_plots(tmp_path):
    run, names, fields, truth, lo, hi = _files(tmp_path, 5)                                # batches of two: a ragged last batch
    out = str(tmp_path / "verified")
    summary = run(out, "--plots", "--verify")
    assert summary["plots"] == 5 and sorted(os.listdir(os.path.join(out, "plots"))) == [n[:-3] + ".png" for n in names]
    outlined = 0
    for name, d, t in zip(names, fields, truth):
        p = _h5_read(os.path.join(out, name), "prediction")
        img = png.read_png(os.path.join(out, "plots", name[:-3] + ".png"))
        want = _picture(d, 0, lo[0], hi[0], [p, t])
        assert img.shape == want.shape == (2 * 74, util_val.W, 3) and np.array_equal(img, want), name
        outlined += int((want[74:] != _picture(d, 0, lo[0], hi[0], [np.zeros_like(t)])).any())
    assert outlined == 5                                                                   # the labels' outlines are in every picture
    assert [rec["plot"] for rec in summary["files"]] == [n[:-3] + ".png" for n in names]
    # every second file, one panel, another channel with values outside the recorded range
    out2 = str(tmp_path / "second")
    summary = run(out2, "--plots", "--plot_every", "2", "--plot_channel", "2")
    assert summary["plots"] == 3 and sorted(os.listdir(os.path.join(out2, "plots"))) == [n[:-3] + ".png" for n in names[::2]]
    assert ["plot" in rec for rec in summary["files"]] == [True, False, True, False, True]
    for name, d in list(zip(names, fields))[::2]:
        p = _h5_read(os.path.join(out2, name), "prediction")
        img = png.read_png(os.path.join(out2, "plots", name[:-3] + ".png"))
        assert np.array_equal(img, _picture(d, 2, lo[2], hi[2], [p])), name
        assert _h5_read(os.path.join(out, name), "prediction").tobytes() == p.tobytes()        # plotting changes no mask


def test_frame_plotter_draws_the_sample_it_names(tmp_path):
    """train.py's FramePlotter on a batch whose samples all differ: both panels of every picture are the checker's picture of the sample
    the file name stands for, so an index that reached the prediction, the labels or the fields of another sample would show"""
    from mlperf_deepcam_amd import train
    H, W = SHAPES["small"]
    B = 3
    fields = _fields(B, H, W, 16, seed=4)
    pred = np.stack([_mask("random", H, W, 20 + b).astype(np.int64) for b in range(B)])
    label = np.stack([_discs(H, W, 5, 40 + b).astype(np.int64) for b in range(B)])

    class Source:                                  # what FramePlotter reads of a dataset: the recorded range per file channel
        minval, maxval = np.full(16, LO, np.float32), np.full(16, HI, np.float32)

    plotter = train.FramePlotter(str(tmp_path), Source(), [1, 0], H, W, DEV)                   # the first SELECTED channel is drawn: 1
    names = [f"/data/train/data-2000-0{b}.h5" for b in range(B)]
    f, p, t = (torch.from_numpy(a).to(DEV) for a in (fields, pred, label))
    seen = set()
    for _ in range(12):
        path = plotter.plot("training", f, p, t, names)
        base = os.path.basename(path)
        assert os.path.dirname(path) == str(tmp_path / "plots") and base.startswith("training-2000-0") and base.endswith(".png")
        b = int(base[len("training-2000-0")])
        seen.add(b)
        assert np.array_equal(png.read_png(path), _picture(fields[b], 1, LO, HI, [pred[b], label[b]])), base
    assert seen == {0, 1, 2}                                                               # (12 draws of 3: all but certainly every sample)
    one = plotter.plot("validation", f, p.to(torch.uint8), t, names[:1])                      # a ragged batch names its valid samples only
    assert os.path.basename(one) == "validation-2000-00.png"
    assert np.array_equal(png.read_png(one), _picture(fields[0], 1, LO, HI, [pred[0], label[0]]))


def _train_run(out, *extra):
    common = ["--wireup_method", "single", "--run_tag", "t", "--synthetic_samples", "8", "--local_batch_size", "2", "--height", "64",
              "--width", "96", "--logging_frequency", "1", "--validation_frequency", "2", "--save_frequency", "0", "--amp_opt_level", "O1",
              "--max_epochs", "1", "--max_steps", "2"]
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.train", "--output_dir", out, *common, *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.loads(line[9:]) for line in r.stdout.splitlines() if line.startswith(":::MLLOG ")]


def _lower_panel_is_the_files_own(path, H, W):
    """the lower panel of a driver's picture against the checker's picture of that synthetic file's own field and labels"""
    from mlperf_deepcam_amd import data as ddata
    name = os.path.basename(path)
    img = png.read_png(path)
    assert img.shape == (2 * 74, W, 3) and img.dtype == np.uint8
    src = ddata.SyntheticHWC(1, H, W)
    src.files = ["data-" + name.split("-", 1)[1].replace(".png", ".h5")]
    d, t = np.empty((H, W, 16), np.float32), np.empty((H, W), np.int64)
    src.read_into(0, d, t)
    assert np.array_equal(img[74:], _picture(d, 0, src._lo[0], src._hi[0], [t])), name
    assert not np.array_equal(img[:74], img[74:]), name                                    # the prediction is not the labels


def test_train_cli_plots_with_batched_validation(tmp_path):
    """--validation_batch_size 2: the picture comes from nn.ValStep's stored logits; one validation sample, so the batch is ragged"""
    out = str(tmp_path / "batched")
    ev = _train_run(out, "--plots", "--validation_batch_size", "2", "--training_visualization_frequency", "0",
                    "--validation_visualization_frequency", "3")
    assert os.listdir(os.path.join(out, "plots")) == ["validation-synthetic-000000.png"]      # training frequency 0: off
    _lower_panel_is_the_files_own(os.path.join(out, "plots", "validation-synthetic-000000.png"), 64, 96)
    assert [x["key"] for x in ev].count("eval_accuracy") == 1


def test_train_cli_with_plots(tmp_path):
    H, W = 64, 96
    freq = ["--training_visualization_frequency", "1", "--validation_visualization_frequency", "1"]
    run = lambda out, *extra: _train_run(out, *freq, *extra)  # noqa: E731
    out = str(tmp_path / "plots_on")
    ev = run(out, "--plots")
    made = sorted(os.listdir(os.path.join(out, "plots")))
    training = [n for n in made if n.startswith("training-synthetic-")]
    validation = [n for n in made if n.startswith("validation-synthetic-")]
    assert len(training) == 2 and len(validation) == 1 and len(made) == 3, made
    for name in made:
        _lower_panel_is_the_files_own(os.path.join(out, "plots", name), H, W)
    out2 = str(tmp_path / "plots_off")
    ev2 = run(out2)
    assert not os.path.exists(os.path.join(out2, "plots"))
    # plotting draws nothing from the generators the run uses: the same losses with and without it.  The training losses (logged through
    # a float32 tensor) and the IoU (from integer counts) are compared exactly.  The validation loss is a float64 sum whose workgroup
    # partials arrive by atomicAdd (csrc/pixel_score.h), in an order that differs from process to process: a sum of n <= 64 * 96
    # positive terms moves by at most (n - 1) * 2^-53 = 7e-13 of its value under reordering, hence rel = 1e-12 there.
    values = lambda e, *keys: [x["value"] for x in e if x["key"] in keys]  # noqa: E731
    assert values(ev, "train_loss", "eval_accuracy") == values(ev2, "train_loss", "eval_accuracy") and len(values(ev, "train_loss")) == 2
    assert len(values(ev, "eval_accuracy")) == 1 and values(ev, "eval_loss") == pytest.approx(values(ev2, "eval_loss"), rel=1e-12, abs=0)
    assert len(values(ev, "eval_loss")) == 1
