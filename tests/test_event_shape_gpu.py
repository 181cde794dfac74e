"""Event shapes and the shape filter on the GPU (csrc/event_shape.hip: dc_component_shape, dc_event_select, dc_mask_select; nn.EventShape,
nn.EventFilter; predict.py --event_shape / --event_filter) against the checker of tests/util_event_shape.py.  Integer equality
throughout: shape rows, keep flags, filtered mask, counts.

Every raw call runs on buffers wrapped in guard bands of poison (shape, keep) and pre-filled with poison (counts, the filtered mask), so
that a store past a table or into a padding sample shows.  Grids 40 x 72 and 33 x 130 are ragged against the 32 x 64 tile and have more
than one tile each way; 40 x 72 has H * W divisible by 4 (the mask pass's 4-byte path), 33 x 130 has not (its byte path).

The filter cases first assert, on the checker's float64 values, that every event's 12 lambda+ and lambda+ / lambda- differ from the active
thresholds by at least 1e-6 relative: the device's fp64 and numpy's may differ in the last places.  A single pixel has lambda+ = lambda- =
0 up to rounding, so its ratio is noise on either side: the cases with an aspect threshold also set min_pixels >= 2 for that class, which
drops such events by an integer comparison whatever the ratio says."""
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
import util_event_shape as us  # noqa: E402
import util_events as ue  # noqa: E402
import util_val  # noqa: E402
from util_launch import assert_served, served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, CAP, GUARD = 2, 4096, 64
POISON64, POISON8 = -0x0123456789ABCDEF, 0xA5
SHAPES = {"40x72": (40, 72), "33x130": (33, 130)}
OFF = ((0, 0, 0.0, 0.0), (0, 0, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------------------------ masks
def _ellipse(m, r0, c0, a, b, angle, cls, wrap=True):
    """an ellipse of half-axes a, b (pixels) rotated by `angle`, centre (r0, c0); columns periodic"""
    H, W = m.shape
    rr, cc = np.mgrid[0:H, 0:W]
    dc = (cc - c0 + W / 2) % W - W / 2 if wrap else cc - c0
    dr = rr - r0
    u, v = dc * np.cos(angle) + dr * np.sin(angle), -dc * np.sin(angle) + dr * np.cos(angle)
    m[(u / a) ** 2 + (v / b) ** 2 <= 1.0] = cls


def _mask(name, H, W, nb=B):
    rs = np.random.RandomState(zlib.crc32(f"shape {name} {H} {W}".encode()))
    m = np.zeros((nb, H, W), np.uint8)
    if name == "random":
        m[:] = (rs.rand(nb, H, W) < 0.45) * rs.randint(1, 3, (nb, H, W))
        m[rs.rand(nb, H, W) < 0.03] = 3                      # values >= 3 are background and pass through the filter
        m[rs.rand(nb, H, W) < 0.01] = 255
    elif name == "blobs":
        for b in range(nb):
            _ellipse(m[b], H // 2, W // 2 - 4, W / 5, 2.2, 0.35 + b, 2)          # long and narrow, through the tile corner
            _ellipse(m[b], 31.5, 12 + 3 * b, 4, 3, 0.0, 1)                        # across the tile rows' border
            _ellipse(m[b], 8, 63.5, 5, 2, 1.2, 1)                                 # across the tile columns' border
            _ellipse(m[b], 20, 0, 7, 2, 0.1, 2)                                   # across the seam
            _ellipse(m[b], 5, W - 1, 2, 2, 0.0, 1)                                # compact, at the seam
            _ellipse(m[b], H - 3, W // 3, 3, 1.5, 0.0, 2)
            m[b, 2, 30] = 1                                                       # speckles
            m[b, 3, 33:35] = 2
            m[b, H - 2, W - 9] = 1
    elif name == "rows":
        m[0, 0, :] = 1                                       # events touching row 0 and row H - 1: rows do not wrap
        m[0, H - 1, 5:W - 7] = 2
        m[0, H - 3:, 2] = 1
        m[1, :3, W // 2] = 2
        m[1, H - 1, :] = 2
        m[1, 0, ::2] = 1
    elif name == "single":
        m[0, H // 2, W // 3] = 1
        m[1, 0, 0] = 2                                       # the corner: three of its four faces are the grid's edge without wrap
    elif name == "full":
        m[0] = 1
        m[1] = 2
    elif name == "checker":
        rr, cc = np.mgrid[0:H, 0:W]
        m[0] = 1 + (rr + cc) % 2
        m[1] = 2 - (rr + cc) % 2
    else:
        raise KeyError(name)
    return m


MASKS = ["random", "blobs", "rows", "single", "full"]


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W), dnn.event_shape_tables(H, W)


def _criteria(H, W, min_pixels=(0, 0), min_area_km2=(0, 0), min_length_km=(0, 0), min_aspect=(0, 0)):
    """the helpers' rows as hashable tuples (what the checker reads) -- the device gets the same numbers"""
    return tuple(tuple(r) for r in dnn.EventFilter.criteria_rows(H, W, min_pixels, min_area_km2, min_length_km, min_aspect).tolist())


@functools.lru_cache(maxsize=None)
def _reference(name, shape, conn, wrap, cap=CAP, n_valid=B, criteria=OFF):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    H, W = shape
    wt, st = _tables(H, W)
    return us.reference(_mask(name, H, W), n_valid, conn, wrap, wt, st, cap, criteria)


def _guarded(n, dtype, poison):
    buf = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _run(mask, conn, wrap, cap=CAP, n_valid=None, criteria=OFF):
    """catalogue, shape, select, mask-select through the raw entry points; returns host tensors and asserts the guard bands"""
    nb, H, W = mask.shape
    nv = nb if n_valid is None else n_valid
    (wy, cx, sx), (rowt, colt) = _tables(H, W)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    wy, cx, sx, rowt, colt, m = d(wy), d(cx), d(sx), d(rowt), d(colt), d(mask)
    labels = torch.zeros((nb, H, W), dtype=torch.int32, device=DEV)
    table = torch.zeros((nb, cap, ue.FIELDS), dtype=torch.int64, device=DEV)
    ncomp = torch.zeros((nb, 3), dtype=torch.int32, device=DEV)
    ws = torch.empty(L.load().dc_mask_components_workspace(nb, H, W), dtype=torch.uint8, device=DEV)
    shape_all, shape = _guarded(nb * cap * us.FIELDS, torch.int64, POISON64)
    keep_all, keep = _guarded(nb * cap, torch.uint8, POISON8)
    counts = torch.full((nb, 2, 4), POISON64, dtype=torch.int64, device=DEV)
    out = torch.full((nb, H, W), POISON8, dtype=torch.uint8, device=DEV)
    crit = np.zeros(2, dnn.EventFilter.CRITERIA)
    for k in range(2):
        crit[k] = criteria[k]
    crit = d(crit.view(np.int64))
    st = L.stream_ptr()
    L.call("dc_mask_components", nb, nv, H, W, L.dptr(m), conn, int(wrap), L.dptr(labels), L.dptr(ws), st)
    L.call("dc_component_stats", nb, nv, H, W, L.dptr(m), L.dptr(labels), L.dptr(wy), L.dptr(cx), L.dptr(sx), cap, L.dptr(table),
           L.dptr(ncomp), L.dptr(ws), st)
    L.call("dc_component_shape", nb, nv, H, W, L.dptr(labels), L.dptr(ws), cap, int(wrap), L.dptr(rowt), L.dptr(colt), L.dptr(shape), st)
    L.call("dc_event_select", nb, nv, cap, L.dptr(table), L.dptr(ncomp), L.dptr(shape), L.dptr(crit), L.dptr(keep), L.dptr(counts), st)
    L.call("dc_mask_select", nb, nv, H, W, L.dptr(m), L.dptr(labels), L.dptr(ws), cap, L.dptr(keep), L.dptr(out), L.dptr(counts), st)
    torch.cuda.synchronize()
    for whole, poison in ((shape_all, POISON64), (keep_all, POISON8)):
        assert bool((whole[:GUARD] == poison).all()) and bool((whole[-GUARD:] == poison).all()), "a store outside the table"
    return {"table": table.cpu().numpy(), "ncomp": ncomp.cpu().numpy(), "shape": shape.view(nb, cap, us.FIELDS).cpu().numpy(),
            "keep": keep.view(nb, cap).cpu().numpy(), "counts": counts.cpu().numpy(), "out_mask": out.cpu().numpy()}


def _assert_equal(got, ref, nv, nb=B):
    assert np.array_equal(got["ncomp"][:nv], ref["ncomp"]) and np.array_equal(got["table"][:nv], ref["table"])
    bad = np.nonzero((got["shape"][:nv] != ref["shape"]).any(axis=2))
    assert len(bad[0]) == 0, f"shape rows differ first at (sample, rank) {list(zip(*bad))[:3]}: " \
        f"{got['shape'][bad[0][0], bad[1][0]].tolist()} vs {ref['shape'][bad[0][0], bad[1][0]].tolist()}"
    assert np.array_equal(got["keep"][:nv], ref["keep"]), f"{int((got['keep'][:nv] != ref['keep']).sum())} keep flags differ"
    assert np.array_equal(got["out_mask"][:nv], ref["out_mask"]), f"{int((got['out_mask'][:nv] != ref['out_mask']).sum())} pixels differ"
    assert got["counts"][:nv].tolist() == ref["counts"].tolist()
    # the padding samples: neither read nor written
    assert bool((got["shape"][nv:] == POISON64).all()) and bool((got["keep"][nv:] == POISON8).all())
    assert bool((got["out_mask"][nv:] == POISON8).all()) and bool((got["counts"][nv:] == POISON64).all())


# ------------------------------------------------------------------------------------------------------------------ 1. shape rows
@pytest.mark.parametrize("wrap", [False, True], ids=["nowrap", "wrap"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", MASKS)
def test_shape_rows_vs_checker(name, shape, conn, wrap):
    """with every criterion off the filter keeps everything: the filtered mask is the mask, values >= 3 included"""
    H, W = SHAPES[shape]
    mask = _mask(name, H, W)
    ref = _reference(name, (H, W), conn, wrap)
    _assert_equal(_run(mask, conn, wrap), ref, B)
    assert np.array_equal(ref["out_mask"], mask) and int(ref["counts"][:, :, 1].sum()) == 0 and int(ref["counts"][:, :, 3].sum()) == 0
    assert int(ref["ncomp"][:, 0].max()) <= CAP
    if name == "full":                                                     # one event per sample; its faces are the grid's edge
        wy = _tables(H, W)[0][0].astype(np.int64)
        edge = [2 * W + 2 * (H - 2), 2 * H, W * int(wy[0] + wy[-1])] if not wrap else [2 * W, 0, W * int(wy[0] + wy[-1])]
        assert ref["ncomp"][:, 0].tolist() == [1, 1] and ref["shape"][0, 0, :3].tolist() == edge
    if name == "single":
        assert ref["shape"][0, 0, :2].tolist() == [1, 2] and ref["shape"][1, 0, :2].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------------------------ 2. LDS overflow
@pytest.mark.parametrize("wrap", [False, True], ids=["nowrap", "wrap"])
def test_checkerboards_overflow_the_lds_table(wrap):
    """64 x 128 checkerboards of both classes under 4-connectivity: every pixel is an event, 2048 roots per tile against 128 slots of the
    workgroup's table, so most runs take the probe-overflow path to the global rows -- the same integers."""
    H, W, cap = 64, 128, 8192
    mask = _mask("checker", H, W)
    ref = _reference("checker", (H, W), 4, wrap, cap)
    assert ref["ncomp"][:, 0].tolist() == [H * W, H * W]
    _assert_equal(_run(mask, 4, wrap, cap=cap), ref, B)
    assert bool((ref["shape"][:, :, 0] == 1).all()) and bool((ref["shape"][:, :, 1] == 2).all())


# ------------------------------------------------------------------------------------------------------------------ 3. cap, n_valid
@pytest.mark.parametrize("shape", list(SHAPES))
def test_more_events_than_rows(shape):
    """cap = 4: ranks below cap are right, nothing is written past the tables (the guard bands in _run), and the mask pass keeps the
    pixels of the events without a row although the criteria drop every event that has one."""
    H, W = SHAPES[shape]
    crit = _criteria(H, W, min_pixels=(10 ** 6, 10 ** 6))
    ref = _reference("random", (H, W), 8, True, 4, B, crit)
    assert int(ref["ncomp"][:, 0].min()) > 4
    got = _run(_mask("random", H, W), 8, True, cap=4, criteria=crit)
    _assert_equal(got, ref, B)
    assert int(got["keep"].sum()) == 0 and got["counts"][:, :, 0].tolist() == [[0, 0], [0, 0]]
    assert int(got["counts"][:, :, 1].sum()) == 8 and int(got["counts"][:, :, 2].sum()) > 0
    for b in range(B):
        first = ref["labels"][b] == 0
        for r in ref["rows"][b][:4]:
            first |= ref["labels"][b] == r[0] + 1
        assert np.array_equal(got["out_mask"][b][~first], _mask("random", H, W)[b][~first])
        assert not np.isin(got["out_mask"][b][first], (1, 2)).any()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_padding_samples_keep_their_poison(shape):
    H, W = SHAPES[shape]
    crit = _criteria(H, W, min_pixels=(3, 3))
    ref = _reference("random", (H, W), 8, True, CAP, 1, crit)
    _assert_equal(_run(_mask("random", H, W), 8, True, n_valid=1, criteria=crit), ref, 1)


# ------------------------------------------------------------------------------------------------------------------ 4. full size
def test_full_size_extreme_sums():
    """768 x 1152, B = 1.  The all-foreground frame is one event with the largest sums there are; its row is computed exactly in Python
    ints from the tables (the sums factor into row sum x column sum; the faces are the first and the last row).  Forty blobs go through
    the per-pixel checker."""
    H, W = 768, 1152
    (wy, _, _), (rowt, colt) = _tables(H, W)
    rs_, cs_ = [int(t.astype(np.int64).sum()) for t in rowt], [int(t.astype(np.int64).sum()) for t in colt]
    full = [2 * W, 0, W * (int(wy[0]) + int(wy[-1])), rs_[1] * cs_[0], rs_[1] * cs_[1], rs_[2] * W << 20, rs_[3] * cs_[2], rs_[3] * cs_[3],
            rs_[3] * cs_[4], rs_[4] * cs_[0], rs_[4] * cs_[1], rs_[5] * W << 20]
    got = _run(np.ones((1, H, W), np.uint8), 8, True, cap=16)
    assert got["ncomp"].tolist() == [[1, 1, 0]] and got["shape"][0, 0].tolist() == full and int(np.abs(got["shape"][0, 1:]).sum()) == 0
    assert got["counts"].tolist() == [[[1, 0, H * W, 0], [0, 0, 0, 0]]]
    rs = np.random.RandomState(77)
    m = np.zeros((1, H, W), np.uint8)
    for k in range(40):
        _ellipse(m[0], rs.randint(0, H), rs.randint(0, W), rs.uniform(6, 60), rs.uniform(2, 12), rs.uniform(0, np.pi), 1 + k % 2)
    crit = _criteria(H, W, min_length_km=(0, 2000), min_aspect=(0, 2), min_pixels=(0, 2))
    wt, st = _tables(H, W)
    ref = us.reference(m, 1, 8, True, wt, st, 64, crit)
    assert 10 <= int(ref["ncomp"][0, 0]) <= 64
    assert min(us.margins(ref["rows"][0], ref["srows"][0].tolist(), crit)) >= 1e-6
    _assert_equal(_run(m, 8, True, cap=64, criteria=crit), ref, 1, nb=1)
    assert int(ref["counts"][0, 1, 0]) > 0 and int(ref["counts"][0, 1, 1]) > 0


# ------------------------------------------------------------------------------------------------------------------ 5. the filter
FILTERS = {
    # thresholds through the helpers, chosen (on the CPU, with these seeds) so that each class keeps some events and drops some
    "pixels_area": dict(min_pixels=(3, 4), min_area_km2=(0, 1.2e6)),
    "length": dict(min_length_km=(900, 2000)),
    "river": dict(min_pixels=(2, 2), min_length_km=(0, 1500), min_aspect=(1.3, 2.0)),
}


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["blobs", "random"])
def test_filter_vs_checker(name, shape, filt):
    H, W = SHAPES[shape]
    crit = _criteria(H, W, **FILTERS[filt])
    ref = _reference(name, (H, W), 8, True, CAP, B, crit)
    # the precondition on the chosen inputs: no event sits within 1e-6 of an active shape threshold (no event is excluded)
    for b in range(B):
        marg = us.margins(ref["rows"][b], ref["srows"][b].tolist(), crit)
        assert not marg or min(marg) >= 1e-6, f"an event within {min(marg):.1e} of a threshold: choose another threshold"
    _assert_equal(_run(_mask(name, H, W), 8, True, criteria=crit), ref, B)
    kept, dropped = ref["counts"][:, :, 0].sum(axis=0), ref["counts"][:, :, 1].sum(axis=0)
    assert all(int(k) > 0 for k in kept) and all(int(d) > 0 for d in dropped), f"kept {kept.tolist()}, dropped {dropped.tolist()}"


# ------------------------------------------------------------------------------------------------------------------ 6. downstream, names
@pytest.mark.parametrize("name", ["blobs", "random"])
def test_catalogue_of_the_filtered_mask_is_the_kept_rows(name):
    """EventFilter -> EventCatalog on the filtered mask: exactly the kept rows of the raw catalogue, in order.  Two catalogues, as in the
    driver: the filter's own of the raw mask, and the one downstream."""
    H, W = SHAPES["40x72"]
    kw = FILTERS["river"]
    raw, down = dnn.EventCatalog(B, H, W), dnn.EventCatalog(B, H, W)
    filt = dnn.EventFilter(raw, **kw)
    assert filt.catalog is raw and filt.shape.catalog is raw and raw is not down
    m = torch.from_numpy(_mask(name, H, W)).to(DEV)
    before = m.clone()
    fm = filt(m)
    down(filt.mask_buffer)
    torch.cuda.synchronize()
    assert torch.equal(m, before) and fm.data_ptr() == filt.mask_buffer.data_ptr() and fm.data_ptr() != m.data_ptr()
    ref = _reference(name, (H, W), 8, True, CAP, B, _criteria(H, W, **kw))
    assert np.array_equal(fm.cpu().numpy(), ref["out_mask"]) and np.array_equal(filt.keep.cpu().numpy(), ref["keep"])
    assert filt.counts().cpu().tolist() == ref["counts"].tolist()
    _, raw_rows = raw.rows()
    _, down_rows = down.rows()
    for b in range(B):
        assert np.array_equal(raw_rows[b], ref["rows"][b])
        assert np.array_equal(down_rows[b], ref["rows"][b][np.asarray(ref["flags"][b], bool)])
        assert 0 < len(down_rows[b]) < len(raw_rows[b])
    # the shapes' host views
    srows = filt.shape.rows()
    assert all(np.array_equal(s, r) for s, r in zip(srows, ref["srows"]))
    dec = filt.shape.shapes()
    assert [len(d) for d in dec] == [len(r) for r in raw_rows] and set(dec[0][0]) == set(dnn.EVENT_SHAPE_VALUES)
    want = dnn.EventShape.values(ref["srows"][0], ref["rows"][0], H, W)       # (an event on a pole row has no area: NaN centroid)
    assert np.array_equal(np.asarray([[d[k] for k in dnn.EVENT_SHAPE_VALUES] for d in dec[0]], np.float64), want, equal_nan=True)
    with pytest.raises(L.DeepcamHipError):
        L.call("dc_mask_select", B, B, H, W, L.dptr(m), L.dptr(raw._labels), L.dptr(raw._ws), raw.cap, L.dptr(filt._keep), L.dptr(m),
               L.dptr(filt._counts), L.stream_ptr())


def test_cc_shape_serves_the_three_calls():
    H, W = SHAPES["40x72"]
    cat = dnn.EventCatalog(B, H, W)
    filt = dnn.EventFilter(cat, min_pixels=(3, 3))
    m = torch.from_numpy(_mask("random", H, W)).to(DEV)
    with served("EventFilter") as names:
        filt(m)
    torch.cuda.synchronize()
    assert names[:3] == ["cc_tile", "cc_merge", "cc_flatten"] and names[-3:] == ["cc_shape"] * 3 and set(names[3:-3]) == {"cc_stats"}
    st = L.stream_ptr()
    with served("dc_component_shape") as names:
        filt.shape()
    assert_served(names, ["cc_shape"], "dc_component_shape")
    with served("dc_event_select") as names:
        L.call("dc_event_select", B, B, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(filt.shape._shape), L.dptr(filt._criteria),
               L.dptr(filt._keep), L.dptr(filt._counts), st)
    assert_served(names, ["cc_shape"], "dc_event_select")
    with served("dc_mask_select") as names:
        L.call("dc_mask_select", B, B, H, W, L.dptr(m), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(filt._keep), L.dptr(filt._out),
               L.dptr(filt._counts), st)
    assert_served(names, ["cc_shape"], "dc_mask_select")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 7. driver
def test_predict_cli_with_event_shape_and_filter(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "unlabelled")
    os.makedirs(root)
    rs = np.random.RandomState(12)
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(2)]
    names = [f"data-{i:02d}.h5" for i in range(2)]
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    out = str(tmp_path / "out")
    min_pixels = (3, 4)
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
           out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", "--events",
           "--event_shape", "--event_filter", "--filter_min_pixels", str(min_pixels[0]), str(min_pixels[1])]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    (wt, st) = _tables(H, W)
    total = np.zeros((2, 4), np.int64)
    for i, name in enumerate(names):
        with h5lite.File(os.path.join(out, name)) as f:
            p, pf, ev, es, esv = (f.read(k) for k in ("prediction", "prediction_filtered", "events", "event_shape", "event_shape_values"))
            order = bytes(f.read("event_shape_value_names")).decode().split(",")
        assert order == list(dnn.EVENT_SHAPE_VALUES)
        ref = us.reference(p[None], 1, 8, True, wt, st, 4096, _criteria(H, W, min_pixels=min_pixels))
        assert np.array_equal(pf, ref["out_mask"][0])
        labels, rows = ue.label_one(pf, 8, True, *wt)                      # `events` are those of the FILTERED mask
        assert ev.dtype == np.int64 and np.array_equal(ev, rows)
        assert es.dtype == np.int64 and np.array_equal(es, us.shape_rows(labels, rows, True, *st))
        assert esv.dtype == np.float64 and np.array_equal(esv, dnn.EventShape.values(es, ev, H, W), equal_nan=True)
        rec = summary["files"][i]["event_filter"]
        got = np.asarray([[c[k] for k in dnn.EVENT_FILTER_COUNTS] for c in rec], np.int64)
        assert got.tolist() == ref["counts"][0].tolist()
        # the counts add up to the raw catalogue's
        raw = ref["rows"][0]
        for k in range(2):
            assert got[k, 0] + got[k, 1] == int((raw[:, 1] == k + 1).sum()) and got[k, 2] + got[k, 3] == int((p == k + 1).sum())
        assert summary["files"][i]["events"] == [int(got[0, 0]), int(got[1, 0])]
        total += got
    sf = summary["event_filter"]
    assert sf["min_pixels"] == [3.0, 4.0] and sf["min_length_km"] == [0.0, 0.0]
    assert [[c[k] for k in dnn.EVENT_FILTER_COUNTS] for c in sf["classes"]] == total.tolist()
    assert summary["events"] == [int(total[0, 0]), int(total[1, 0])]
