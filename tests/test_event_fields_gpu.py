"""Event intensities on the GPU (dc_component_fields of csrc/event_fields.hip, nn.EventFields, predict.py --event_fields) against the loop of
tests/util_event_fields.py.  Every result is an integer that does not depend on the order of arrival: every comparison is torch.equal on
int64 tables, without a tolerance.

Shapes, batch and padding are the catalogue tests': (2 TH + 3, 2 TW + 5) and (TH - 1, TW - 3) from the kernel's own tile, batch 3 with
n_valid = 2.  The padding sample is all class 1 with NaN fields, and its part of the table is pre-filled with a sentinel that must come
back untouched."""
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
import util_event_fields as uf  # noqa: E402
import util_events as ue  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV, CAP = 3, 2, 4096
CONN, WRAP = 8, True
SENTINEL = -77
GUARD = 64                                         # words behind the table that no launch may touch
LAYOUTS = [(16, 16), (3, 5), (1, 1)]               # (C, ldc): 16-byte loads; scalar loads with unused channels; a single channel
MASKS = ["random0.45", "spiral", "band", "uniform"]
SETS = ["ints", "scaled", "specials", "scaled_bgnan"]


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


TH, TW = _tile()
SHAPES = {"tiles": (2 * TH + 3, 2 * TW + 5), "one": (TH - 1, TW - 3)}


def _spiral(H, W):
    """a one-pixel-wide path from (0, 0) inwards, one empty pixel between its turns"""
    m = np.zeros((H, W), np.uint8)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = 1
    stuck = 0
    while stuck < 2:
        nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if 0 <= nr < H and 0 <= nc < W and not m[nr, nc] and not (0 <= fr < H and 0 <= fc < W and m[fr, fc]):
            r, c, stuck = nr, nc, 0
            m[r, c] = 1
        else:
            dr, dc, stuck = dc, -dr, stuck + 1
    return m


def _mask(name, H, W):
    """uint8 [3, H, W]; sample 2 is padding (all class 1: if it were read, its NaN fields would show in the table)"""
    rs = np.random.RandomState(zlib.crc32(f"{name} {H} {W}".encode()))
    m = np.zeros((B, H, W), np.uint8)
    if name.startswith("random"):
        m[:NV] = (rs.rand(NV, H, W) < float(name[6:])) * rs.randint(1, 3, (NV, H, W))
    elif name == "spiral":                       # one long event through every tile
        m[0] = _spiral(H, W)
        m[1] = 2 * _spiral(W, H).T
    elif name == "band":                         # joined across the seam: on one row, and on neighbouring rows
        m[0, 5, :10] = 1
        m[0, 5, W - 10:] = 1
        m[1, 5, :10] = 1
        m[1, 6, W - 10:] = 1
    elif name == "uniform":                      # sample 0 has no event, sample 1 one over the whole field
        m[1] = 2
    elif name == "checker":
        rr, cc = np.mgrid[0:H, 0:W]
        m[0] = 1 + (rr + cc) % 2
        m[1] = 2 - (rr + cc) % 2
    else:
        raise KeyError(name)
    m[NV:] = 1
    return m


def _discs(H, W, n, seed):
    """n discs of radius 6..22 and class 1 or 2 (later ones overwrite earlier ones), some across the seam"""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    rr, cc = np.mgrid[0:H, 0:W]
    for _ in range(n):
        r0, c0, rad, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(6, 23), rs.randint(1, 3)
        dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
        m[(rr - r0) ** 2 + dc ** 2 <= rad * rad] = cl
    return m


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


def _lds_slots():
    n = C.c_int()
    assert L.load().dc_component_fields_lds_slots(C.byref(n)) == 0
    return n.value


@functools.lru_cache(maxsize=None)
def _catalogue(name, shape, conn=CONN, wrap=WRAP, nv=NV):
    H, W = SHAPES[shape]
    return ue.catalogue(_mask(name, H, W), nv, conn, wrap, *_tables(H, W), CAP)


def _scaled(rs, H, W, ldc):
    """normal values times per-channel magnitudes from 1e-6 to 1e5"""
    mag = np.logspace(-6, 5, ldc) if ldc > 1 else np.asarray([250.0])
    return (rs.standard_normal((B, H, W, ldc)) * mag).astype(np.float32)


def _bits_of(f, C_):
    finite = np.where(np.isfinite(f[:NV]), f[:NV], 0)
    return dnn.event_field_bits(finite.min(axis=(0, 1, 2))[:C_], finite.max(axis=(0, 1, 2))[:C_])


@functools.lru_cache(maxsize=None)
def _fields(kind, name, shape, C_, ldc):
    """(fields float32 [3, H, W, ldc] with a NaN padding sample, bits int32 [C]); callers do not modify them"""
    H, W = SHAPES[shape]
    rs = np.random.RandomState(zlib.crc32(f"fields {kind.split('_')[0]} {H} {W} {ldc}".encode()))
    if kind == "ints":
        f = rs.randint(-2, 3, (B, H, W, ldc)).astype(np.float32)                           # ties everywhere
        bits = dnn.event_field_bits(np.full(C_, -2.0), np.full(C_, 2.0))
    else:
        f = _scaled(rs, H, W, ldc)
        bits = _bits_of(f, C_)
    if kind == "scaled_bgnan":
        f[:NV][_mask(name, H, W)[:NV] == 0] = np.nan                                        # the classes here are 0, 1, 2: 0 is the background
    if kind == "specials":
        labels, _, _, rows = _catalogue(name, shape)
        top = np.abs(f[:NV]).max(axis=(0, 1, 2))
        for b in range(NV):
            fg = np.argwhere(labels[b] > 0)
            if len(fg) == 0:
                continue
            picks = fg[rs.choice(len(fg), size=min(len(fg), 60), replace=False)]
            for i, (r, c) in enumerate(picks):
                ch = int(rs.randint(0, C_))
                f[b, r, c, ch] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-39, 8 * top[ch], -8 * top[ch]][i % 9]
        if sum(len(r) for r in rows) * C_ >= 2:                                             # one row without any finite value
            b = int(np.argmax([len(r) for r in rows]))
            k = int(np.argmin(rows[b][:, 2]))
            f[b, :, :, C_ - 1][labels[b] == int(rows[b][k, 0]) + 1] = np.nan
    f[NV:] = np.nan
    return f, bits


@functools.lru_cache(maxsize=None)
def _reference(kind, name, shape, C_, ldc):
    """the checker's table, computed once per case and shared (callers do not modify it)"""
    H, W = SHAPES[shape]
    f, bits = _fields(kind, name, shape, C_, ldc)
    labels, _, _, rows = _catalogue(name, shape)
    wy = _tables(H, W)[0]
    return np.stack([uf.field_rows(labels[b], rows[b], CAP, f[b], C_, bits, wy) for b in range(NV)])


def _run(mask, fields, C_, bits, cap=CAP, n_valid=NV, conn=CONN, wrap=WRAP, offset=0, names=None):
    """the catalogue's two calls, then dc_component_fields on a table pre-filled with the sentinel; offset: floats in front of the fields
    (a base that is not 16-byte aligned).  Returns (ftable [nb, cap, C, 6], the guard words behind it, ncomp) on the host."""
    nb, H, W = mask.shape
    ldc = fields.shape[3]
    wy, cx, sx = (torch.from_numpy(t).to(DEV) for t in _tables(H, W))
    m = torch.from_numpy(mask).to(DEV)
    store = torch.zeros(fields.size + offset, dtype=torch.float32, device=DEV)
    f = store[offset:].view(nb, H, W, ldc)
    f.copy_(torch.from_numpy(fields))
    labels = torch.zeros((nb, H, W), dtype=torch.int32, device=DEV)
    table = torch.zeros((nb, cap, ue.FIELDS), dtype=torch.int64, device=DEV)
    ncomp = torch.zeros((nb, 3), dtype=torch.int32, device=DEV)
    ws = torch.empty(L.load().dc_mask_components_workspace(nb, H, W), dtype=torch.uint8, device=DEV)
    n = nb * cap * C_ * uf.STATS
    flat = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    sb = torch.from_numpy(np.asarray(bits, np.int32)).to(DEV)
    st = L.stream_ptr()
    L.call("dc_mask_components", nb, n_valid, H, W, L.dptr(m), conn, int(wrap), L.dptr(labels), L.dptr(ws), st)
    L.call("dc_component_stats", nb, n_valid, H, W, L.dptr(m), L.dptr(labels), L.dptr(wy), L.dptr(cx), L.dptr(sx), cap, L.dptr(table),
           L.dptr(ncomp), L.dptr(ws), st)
    if names is None:
        L.call("dc_component_fields", nb, n_valid, H, W, L.dptr(labels), L.dptr(ws), cap, L.dptr(f), C_, ldc, L.dptr(sb), L.dptr(wy), L.dptr(flat), st)
    else:
        with served("dc_component_fields") as got:
            L.call("dc_component_fields", nb, n_valid, H, W, L.dptr(labels), L.dptr(ws), cap, L.dptr(f), C_, ldc, L.dptr(sb), L.dptr(wy),
                   L.dptr(flat), st)
        names.extend(got)
    torch.cuda.synchronize()
    host = flat.cpu()
    return host[:n].view(nb, cap, C_, uf.STATS), host[n:], ncomp.cpu()


def _assert_equal(got, ref, nv=NV):
    ftable, guard, _ = got
    want = torch.from_numpy(ref)
    assert torch.equal(ftable[:nv], want), f"rows differ first at {torch.nonzero((ftable[:nv] != want).any(dim=3))[:4].tolist()}"
    assert bool((ftable[nv:] == SENTINEL).all()), "the padding samples' rows were written"
    assert bool((guard == SENTINEL).all()), "words behind the table were written"


# ------------------------------------------------------------------------------------------------------------------ 1. kernels vs checker
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=[f"c{c}-ld{ld}" for c, ld in LAYOUTS])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", MASKS)
def test_fields_vs_checker(name, shape, layout, kind):
    H, W = SHAPES[shape]
    C_, ldc = layout
    f, bits = _fields(kind, name, shape, C_, ldc)
    ref = _reference("scaled" if kind == "scaled_bgnan" else kind, name, shape, C_, ldc)   # NaN on the background changes nothing
    _assert_equal(_run(_mask(name, H, W), f, C_, bits), ref)
    rows = _catalogue(name, shape)[3]
    filled = [min(len(r), CAP) for r in rows]
    for b in range(NV):                                                      # the checker itself: empty rows exactly behind the events
        assert (ref[b, filled[b]:] == np.asarray(uf.EMPTY_ROW)).all()
    if kind == "specials":
        assert ref[..., 4].sum() > 0 and ref[..., 5].sum() > 0              # non-finite and saturated values were met
        if sum(filled) * C_ >= 2:                                            # (one event with one channel cannot hold both)
            hollow = [(ref[b, :filled[b], :, 0] == -1) & (ref[b, :filled[b], :, 4] > 0) for b in range(NV)]
            assert any(h.any() for h in hollow), "no event row without a finite value"
    elif kind == "ints":
        assert ref[..., 4].sum() == 0 and ref[..., 5].sum() == 0
        if name == "uniform":                                                # one event over the whole field: every value occurs, ties at both ends
            lo, hi = int(ref[1, 0, 0, 0]), int(ref[1, 0, 0, 1])
            first = lambda v: int(np.argwhere(f[1, :, :, 0].reshape(-1) == v)[0, 0])  # noqa: E731
            assert lo == uf.signed((uf.key(-2.0) << 32) | first(-2.0)) and hi == uf.signed((uf.key(2.0) << 32) | (0xFFFFFFFF - first(2.0)))
            assert int(ref[1, 0, 0, 2]) == int(f[1, :, :, 0].astype(np.int64).sum()) << int(bits[0])


# ------------------------------------------------------------------------------------------------------------------ 2. LDS table overflow
@pytest.mark.parametrize("shape,cap", [("tiles", 100), ("one", 4096)])
def test_more_roots_in_a_tile_than_the_lds_table_holds(shape, cap):
    """The checkerboard under 4-connectivity puts one root on every pixel: far more roots per tile than LDS slots, so most runs go to the
    global rows directly.  cap 100: exact rows for the first 100 roots and nothing written for the others."""
    H, W = SHAPES[shape]
    assert min(TH, H) * min(TW, W) > 4 * _lds_slots()
    mask = _mask("checker", H, W)
    C_, ldc = 16, 16
    f, bits = _fields("scaled", "checker", shape, C_, ldc)
    labels, _, ncomp, rows = ue.catalogue(mask, NV, 4, False, *_tables(H, W), cap)
    assert ncomp[0, 0] == H * W and (cap < H * W) == (shape == "tiles")
    wy = _tables(H, W)[0]
    ref = np.stack([uf.field_rows(labels[b], rows[b], cap, f[b], C_, bits, wy) for b in range(NV)])
    got = _run(mask, f, C_, bits, cap=cap, conn=4, wrap=False)
    _assert_equal(got, ref)
    assert got[2][:NV].tolist() == ncomp.tolist()
    k = min(cap, H * W)                                                      # one pixel per event: both extremes are the value at pixel k
    want = [uf.signed((uf.key(v) << 32) | p) for p, v in enumerate(f[0, :, :, 3].reshape(-1)[:k])]
    assert got[0][0, :k, 3, 0].tolist() == want


# ------------------------------------------------------------------------------------------------------------------ 3. other kernel cases
def test_every_sample_valid_and_a_single_sample():
    H, W = SHAPES["tiles"]
    mask = _mask("random0.45", H, W)
    f = _fields("scaled", "random0.45", "tiles", 16, 16)[0].copy()
    f[NV:] = _scaled(np.random.RandomState(77), H, W, 16)[NV:]               # the third sample: one event over the whole field, finite values
    bits = dnn.event_field_bits(f.min(axis=(0, 1, 2)), f.max(axis=(0, 1, 2)))
    wy = _tables(H, W)[0]
    labels, _, ncomp, rows = ue.catalogue(mask, B, CONN, WRAP, *_tables(H, W), CAP)
    assert ncomp[2].tolist() == [1, 1, 0]
    ref = np.stack([uf.field_rows(labels[b], rows[b], CAP, f[b], 16, bits, wy) for b in range(B)])
    _assert_equal(_run(mask, f, 16, bits, n_valid=B), ref, nv=B)
    assert int(ref[2, 0, 0, 2]) == int(np.rint(np.ldexp(f[2, :, :, 0].astype(np.float64), int(bits[0]))).sum())
    # a single sample, its fields 4 bytes off a 16-byte boundary: the scalar loads serve a layout the vector loads would take
    _assert_equal(_run(mask[:1], f[:1], 16, bits, n_valid=1, offset=1), ref[:1], nv=1)


def test_vector_loads_with_a_partial_last_group():
    """C = 6 of ldc = 8: the second 16-byte load carries two channels that are used and two that are not"""
    H, W = SHAPES["one"]
    f, bits = _fields("scaled", "random0.45", "one", 6, 8)
    labels, _, _, rows = _catalogue("random0.45", "one")
    ref = np.stack([uf.field_rows(labels[b], rows[b], CAP, f[b], 6, bits, _tables(H, W)[0]) for b in range(NV)])
    _assert_equal(_run(_mask("random0.45", H, W), f, 6, bits), ref)


def test_two_calls_with_another_mask_in_between_agree():
    H, W = SHAPES["tiles"]
    cat = dnn.EventCatalog(B, H, W, connectivity=CONN, wrap=WRAP)
    f, bits = _fields("scaled", "random0.45", "tiles", 16, 16)
    ef = dnn.EventFields(cat, 16, bits)
    fd = torch.from_numpy(f).to(DEV)
    m = torch.from_numpy(_mask("random0.45", H, W)).to(DEV)
    other = torch.from_numpy(_mask("checker", H, W)).to(DEV)
    cat(m, n_valid=NV)
    first = ef(fd).table.clone()
    cat(other, n_valid=NV)
    ef(fd)                                                                   # two events over everything: rows the next call has to clear
    assert not torch.equal(ef.table, first)
    cat(m, n_valid=NV)
    again = ef(fd).table
    torch.cuda.synchronize()
    assert torch.equal(again, first) and tuple(again.shape) == (NV, CAP, 16, 6)
    assert torch.equal(first.cpu(), torch.from_numpy(_reference("scaled", "random0.45", "tiles", 16, 16)))


# ------------------------------------------------------------------------------------------------------------------ 4. launches, arguments
def test_two_launches_named_cc_fields_behind_the_catalogue():
    H, W = SHAPES["tiles"]
    f, bits = _fields("ints", "band", "tiles", 16, 16)
    names = []
    _run(_mask("band", H, W), f, 16, bits, names=names)
    assert names == ["cc_fields", "cc_fields"]
    cat = dnn.EventCatalog(B, H, W)
    ef = dnn.EventFields(cat, 16, bits)
    fd, m = torch.from_numpy(f).to(DEV), torch.from_numpy(_mask("band", H, W)).to(DEV)
    with served("EventCatalog + EventFields") as both:
        cat(m, n_valid=NV)
        ef(fd)
    torch.cuda.synchronize()
    assert both[-2:] == ["cc_fields", "cc_fields"] and "cc_fields" not in both[:-2] and both[0] == "cc_tile" and "cc_stats" in both


def test_argument_errors_leave_a_message():
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)             # read as labels, ranks, fields, bits and weights: all zero
    out = torch.full((2 * 4 * 6 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    p = L.dptr(buf)
    cf = lambda **kw: lib.dc_component_fields(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 1), ("nv", 1), ("H", 4), ("W", 4), ("labels", p), ("rank", p), ("cap", 2), ("fields", p), ("C", 4), ("ldc", 4), ("bits", p),
        ("wy", p), ("ftable", L.dptr(out)), ("st", None))])
    assert cf(C=0) != 0 and "C must lie in [1, 32]" in L.last_error()
    assert cf(C=33, ldc=33) != 0 and "C must lie in [1, 32]" in L.last_error()
    assert cf(C=4, ldc=3) != 0 and "ldc" in L.last_error()
    assert cf(H=2048, W=2049, labels=None, rank=None, fields=None, bits=None, wy=None, ftable=None) != 0 and "2^22" in L.last_error()
    assert cf(fields=None) != 0 and "null" in L.last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                     # nothing was launched
    assert cf() == 0, L.last_error()                                         # the same arguments, complete: no event, two channels' empty rows
    torch.cuda.synchronize()
    assert out[:48].view(8, 6).tolist() == [list(uf.EMPTY_ROW)] * 8 and bool((out[48:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ 5. nn.EventFields
def test_event_fields_object_against_the_checker():
    H, W = SHAPES["tiles"]
    C_, ldc = 3, 5
    f, bits = _fields("specials", "random0.45", "tiles", C_, ldc)
    cat = dnn.EventCatalog(B, H, W, connectivity=CONN, wrap=WRAP)
    ef = dnn.EventFields(cat, C_, bits, ldc=ldc)
    m = torch.from_numpy(_mask("random0.45", H, W)).to(DEV)
    fd = torch.from_numpy(f).to(DEV)
    cat(m, n_valid=NV)
    assert ef(fd) is ef                                                      # n_valid: the catalogue's
    ref = _reference("specials", "random0.45", "tiles", C_, ldc)
    rows = _catalogue("random0.45", "tiles")[3]
    assert torch.equal(ef.table.cpu(), torch.from_numpy(ref))
    host = ef.rows()
    assert [len(r) for r in host] == [len(r) for r in rows] and all(np.array_equal(h, ref[b, :len(h)]) for b, h in enumerate(host))
    assert ef.stats() == [dnn.EventFields.decode(ref[b, :len(rows[b])], rows[b], H, W, bits) for b in range(NV)]
    big = ef.stats(min_pixels=20)
    keep = [rows[b][:, 2] >= 20 for b in range(NV)]
    assert big == [dnn.EventFields.decode(ref[b, :len(rows[b])][keep[b]], rows[b][keep[b]], H, W, bits) for b in range(NV)]
    assert [len(s) for s in big] == [len(e) for e in cat.events(min_pixels=20)] and sum(len(s) for s in big) > 0
    for bad in (fd.double(), fd[:, :, :, :4], fd[:2], fd.cpu(), fd.transpose(1, 2)):
        with pytest.raises(L.DeepcamHipError):
            ef(bad)
    with pytest.raises(L.DeepcamHipError):
        ef(fd, n_valid=B + 1)


# ------------------------------------------------------------------------------------------------------------------ 6. driver
def _cli(tmp_path, labelled):
    from mlperf_deepcam_amd import h5lite
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(12)
    n = 3 if labelled else 2
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(n)]
    truth = [_discs(H, W, 7, 300 + i).astype(np.int64) for i in range(n)]
    names = [f"data-{i:02d}.h5" for i in range(n)]
    for name, d, t in zip(names, fields, truth):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
            if labelled:
                f.write("climate/labels_0", t)
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", lo)
        f.write("climate/maxval", hi)
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)

    def run(out, *extra):
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
               out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.load(open(os.path.join(out, "summary.json")))

    return run, names, fields, dnn.event_field_bits(lo, hi)


def _check_outputs(out, names, fields, bits, summary, min_px):
    """every file's event_fields / event_field_values / event_field_bits against the checker on its own data and stored prediction"""
    from mlperf_deepcam_amd import h5lite
    H, W = util_val.H, util_val.W
    totals, events = [0, 0], 0
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(out, name)) as f:
            p, ev, fr, fv, fb = (f.read(k) for k in ("prediction", "events", "event_fields", "event_field_values", "event_field_bits"))
        assert fr.dtype == np.int64 and fv.dtype == np.float64 and fb.dtype == np.int32 and np.array_equal(fb, bits)
        ftable, cat = uf.field_table(p[None], 1, 8, True, *_tables(H, W), CAP, d[None], 16, bits)
        rows = cat[3][0]
        keep = rows[:, 2] >= min_px
        assert np.array_equal(ev, rows[keep]), name
        assert fr.shape == (int(keep.sum()), 16, 6) and np.array_equal(fr, ftable[0, :len(rows)][keep]), name
        want = uf.values_from_decode(dnn.EventFields.decode(fr, ev, H, W, bits), 16)
        assert fv.shape == (len(ev), 16, 8) and np.array_equal(fv, want, equal_nan=True), name
        totals = [totals[0] + int(fr[..., 4].sum()), totals[1] + int(fr[..., 5].sum())]
        events += len(ev)
    assert summary["event_fields"] == {"channels": 16, "scale_bits": [int(b) for b in bits], "nonfinite": totals[0], "saturated": totals[1]}
    print(f"predict.py --event_fields (min pixels {min_px}): {events} events in {len(names)} files")
    return events


def test_predict_cli_with_event_fields(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    run, names, fields, bits = _cli(tmp_path, labelled=False)
    out = str(tmp_path / "fields")
    every = _check_outputs(out, names, fields, bits, run(out, "--events", "--event_fields"), 0)
    out20 = str(tmp_path / "fields20")
    large = _check_outputs(out20, names, fields, bits, run(out20, "--event_fields", "--min_event_pixels", "20"), 20)
    assert 0 < large < every                                                 # (the masks hold events, small ones among them)
    # without the flag: the files and the summary of before, the same bytes
    plain = str(tmp_path / "plain")
    summary = run(plain, "--events")
    assert "event_fields" not in summary and all("event_field_counts" not in rec for rec in summary["files"])
    for name in names:
        with h5lite.File(os.path.join(plain, name)) as f:
            assert all(k not in f for k in ("event_fields", "event_field_values", "event_field_bits"))
            p, ev = f.read("prediction"), f.read("events")
        with h5lite.File(os.path.join(out, name)) as f:
            assert f.read("prediction").tobytes() == p.tobytes() and np.array_equal(f.read("events"), ev)


def test_predict_cli_with_event_fields_under_verify(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    run, names, fields, bits = _cli(tmp_path, labelled=True)
    out = str(tmp_path / "verified")
    summary = run(out, "--verify", "--event_fields", "--min_event_pixels", "2")           # three files in batches of two: a ragged last batch
    _check_outputs(out, names, fields, bits, summary, 2)
    assert "event_verification" in summary
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f:
            ev, ma = f.read("events"), f.read("matches")
            assert all(k in f for k in ("truth_events", "event_scores")) and (len(ma) == 0 or int(ma[:, 0].max()) < len(ev))
