"""Storm-centred composites on the GPU (dc_composite_centers / dc_composite_accumulate of csrc/composite.hip, nn.StormComposite,
predict.py --composites) against the numpy checker of tests/util_composite.py.  Everything is an integer: every comparison is equality.
The checker works from what the catalogue and EventFields left on the device (label maps, rows, field rows), read back once per batch.
Shapes: (H, W, R) = (25, 20, 3) -- an odd H has a row at latitude 0 exactly, which must not flip -- and (40, 33, 5), a width that is no
multiple of 4.  Layouts: 16 of 16 channels (the vector form) and channels 4, 0, 2 of 5 (the scalar form); 20 of 20 channels serve the
one case whose radial table does not fit the workgroup's LDS."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_composite as uc  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV = 5, 4
CAP = 64
CC = 1                                                 # the centre channel: not among the scalar layout's selection
GUARD, SENTINEL = 64, 0x5A
SHAPES = {"odd": (25, 20, 3), "even": (40, 33, 5)}
LAYOUTS = {"c16-vec": (16, 16, None), "c3-ldc5": (3, 5, [4, 0, 2]), "c20-vec": (20, 20, None)}   # (C, ldc, chan); None: the identity over ldc
SERVED = {"c16-vec": "composite_accumulate_vec", "c3-ldc5": "composite_accumulate_scalar", "c20-vec": "composite_accumulate_vec"}
EDGES = (-52.0, 100.0)                                 # -52 is the centre value of the event east of the seam: the >= rule
CASES = [(s, l) for s in SHAPES for l in ("c16-vec", "c3-ldc5")]
CASE_IDS = [f"{s}-{l}" for s, l in CASES]


def _chan(lid):
    C_, ldc, chan = LAYOUTS[lid]
    return list(range(C_)) if chan is None else chan


def _bits(lid):
    return [(3 * c) % 7 for c in range(LAYOUTS[lid][0])]      # values of a few thousand times at most 2^6: far inside 2^28


def _negate(lid):
    return (0, 2)                                       # positions among the selected channels


@functools.lru_cache(maxsize=None)
def _chunk():
    n = C.c_int(0)
    assert L.load().dc_composite_chunk(C.byref(n)) == 0 and n.value > 0
    return n.value


@functools.lru_cache(maxsize=None)
def _frames(shape, ldc):
    """Five frames (shared, read-only) and the centres the first two are built to have.
    0: events centred at (0, 0) and (H-1, W-1), and within R of the seam on both sides; NaN, +-Inf, a saturated value and the largest
       value that fits inside the first one's window
    1: centres on the row below the equator, on it (odd H) and above it, with overlapping windows; an event of class 2; a one-pixel event
       (below min_pixels = 2); an event whose centre channel is NaN throughout (no centre)
    2: random, 45 % foreground: more events than the catalogue's cap
    3: two events far from every border
    4: random, sparse (the padding frame of the n_valid cases)"""
    H, W, R = SHAPES[shape]
    rs = np.random.RandomState(H * 100 + ldc)
    mask = np.zeros((B, H, W), np.uint8)
    fields = ((rs.rand(B, H, W, ldc) - 0.3) * 4000.0).astype(np.float32)
    fields[..., CC] = (500.0 + 100.0 * rs.rand(B, H, W)).astype(np.float32)       # the centre channel: positive but at the planted minima
    want = {0: [], 1: []}

    def plant(b, pixels, centre, value, cls=1):
        for r, c in pixels:
            mask[b, r, c] = cls
        if centre is not None:
            assert centre in pixels
            fields[b, centre[0], centre[1], CC] = value
            if cls == 1 and len(pixels) >= 2 and b in want:
                want[b].append(centre[0] * W + centre[1])

    plant(0, [(0, 0), (0, 1), (1, 0)], (0, 0), -50.0)
    plant(0, [(H - 1, W - 1), (H - 1, W - 2), (H - 2, W - 1)], (H - 1, W - 1), -51.0)
    plant(0, [(6, W - 2), (6, W - 3)], (6, W - 2), -52.0)
    plant(0, [(9, 1), (9, 2)], (9, 1), -53.0)
    fields[0, 1, 1, :] = np.nan                          # inside the window of (0, 0), outside its pixels
    fields[0, 0, 2, :] = np.inf
    fields[0, 2, 0, :] = -np.inf
    fields[0, 2, 1, :] = 2.0 ** 28                       # fits where bits == 0, saturated elsewhere
    fields[0, 2, 2, :] = np.nextafter(np.float32(2.0 ** 28), np.float32(np.inf))
    fields[0, 1, 2, :] = -1e12
    m = (H - 1) // 2
    plant(1, [(m - 1, 2), (m - 1, 3)], (m - 1, 2), -60.0)
    plant(1, [(m, 6), (m, 7)], (m, 7), -61.0)
    plant(1, [(m + 1, 10), (m + 1, 11)], (m + 1, 10), -62.0)
    plant(1, [(3, 12), (3, 13), (3, 14)], (3, 13), -63.0, cls=2)
    plant(1, [(m + 6, 3)], (m + 6, 3), -64.0)
    plant(1, [(3, 4), (3, 5)], None, None)
    fields[1, 3, 4:6, CC] = np.nan
    mask[2] = rs.choice(np.asarray([0, 1, 2], np.uint8), size=(H, W), p=[0.55, 0.22, 0.23])
    plant(3, [(m + 3, W // 2), (m + 4, W // 2)], (m + 4, W // 2), -70.0)
    plant(3, [(m - 4, 4), (m - 4, 5), (m - 5, 5)], (m - 5, 5), 150.0)
    mask[4] = rs.choice(np.asarray([0, 1, 2], np.uint8), size=(H, W), p=[0.90, 0.07, 0.03])
    mask.setflags(write=False), fields.setflags(write=False)
    return mask, fields, want


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared frames are read-only


class _Pipe:
    """a catalogue and an EventFields over `batch` frames; run() launches both and reads back what the checker works from"""

    def __init__(self, shape, lid, batch=B, cap=CAP, connectivity=8):
        self.H, self.W, self.R = SHAPES[shape] if isinstance(shape, str) else shape
        self.lid, self.ldc, self.batch = lid, LAYOUTS[lid][1], batch
        self.catalog = dnn.EventCatalog(batch, self.H, self.W, connectivity=connectivity, wrap=True, cap=cap, device=DEV)
        self.efields = dnn.EventFields(self.catalog, self.ldc, [4] * self.ldc)

    def run(self, mask, fields, nv=None):
        n = len(mask)
        nv = n if nv is None else nv
        m = np.ones((self.batch, self.H, self.W), np.uint8)                       # padding: all class 1 over NaN
        f = np.full((self.batch, self.H, self.W, self.ldc), np.nan, np.float32)
        m[:n], f[:n] = mask, fields
        self.host_fields, self.nv = f, nv
        self.dev_fields = _dev(f)
        self.catalog(_dev(m), n_valid=nv)
        self.efields(self.dev_fields, n_valid=nv)
        self.labels = self.catalog.labels.cpu().numpy()
        self.table = self.catalog.table.cpu().numpy()
        self.ncomp = self.catalog.counts().cpu().numpy()
        self.ftable = self.efields.table.cpu().numpy()
        return self

    def comp(self, **kw):
        kw = {"radius": self.R, "channels": _chan(self.lid), "bits": _bits(self.lid), "classes": (1,), "min_pixels": 2, "groups": 2,
              "intensity_edges": EDGES, "negate": _negate(self.lid), "bin_km": 400.0, "bins": 6, **kw}
        return dnn.StormComposite(self.efields, CC, **kw)

    def reference(self, comp, groups, state=None):
        """the checker on the last batch: (centers, egroup) of the valid frames, and `state` (or zeros) advanced"""
        state = uc.empty(comp.GT, comp.R, comp.C, comp.NB) if state is None else state
        groups = [g for g in groups][:self.nv]
        cen, egr = uc.centers(self.table, self.ncomp, self.ftable, self.H, self.W, comp.center_channel, comp.center_stat, comp.classes,
                              comp.min_pixels, groups, comp.G, comp.edges, state["counts"])
        uc.accumulate(state, cen, egr, self.table, self.labels, self.host_fields[:self.nv], comp.channels, comp.bits, comp.negate,
                      comp.flip_south, comp.radius_table, comp.R)
        return cen, egr, state


@functools.lru_cache(maxsize=None)
def _standard(shape, lid):
    """the standard batch through the catalogue and the checker, once: (pipe, centers, egroup, state)"""
    mask, fields, _ = _frames(shape, LAYOUTS[lid][1])
    pipe = _Pipe(shape, lid).run(mask, fields, NV)
    cen, egr, state = pipe.reference(pipe.comp(), [0, 1, 1, 0, 0])
    return pipe, cen, egr, state


# ------------------------------------------------------------------------------------------------------------------ 1. the checker's equal
@pytest.mark.parametrize("shape,lid", CASES, ids=CASE_IDS)
def test_state_equals_the_checker(shape, lid):
    H, W, R = SHAPES[shape]
    pipe, cen, egr, ref = _standard(shape, lid)
    _, _, want = _frames(shape, LAYOUTS[lid][1])
    comp = pipe.comp()
    with served("StormComposite") as names:
        comp(pipe.dev_fields, groups=[0, 1, 1, 0, 0], n_valid=NV)
    assert names == ["composite_centers", SERVED[lid]]
    assert np.array_equal(comp.centers.cpu().numpy(), cen) and np.array_equal(comp.event_groups.cpu().numpy(), egr)
    uc.assert_state(comp.state(), ref, f"{shape} {lid}")
    # the frames are what they were built to be
    for b in (0, 1):
        assert set(want[b]) <= set(cen[b].tolist()), (b, want[b], cen[b][cen[b] >= 0].tolist())
    assert {0, H * W - 1, 6 * W + W - 2, 9 * W + 1} == set(want[0])
    m = (H - 1) // 2
    assert [p // W for p in want[1]] == [m - 1, m, m + 1] and (2 * m == H - 1) == (H % 2 == 1)
    c = ref["counts"]
    assert c["other_class"] > 0 and c["below_min_pixels"] > 0 and c["no_center"] == 1 and c["uncatalogued"] > 0 and c["composited"] > 8
    assert pipe.ncomp[2, 0] > CAP and (cen[2] >= 0).any()
    k = cen[0].tolist().index(6 * W + W - 2)                                       # the event whose centre value is an edge: the bin above
    assert egr[0, k] == 1 and egr[0, cen[0].tolist().index(9 * W + 1)] == 0 and len(set(egr[egr >= 0].tolist())) >= 5
    assert (ref["n"][:, 2 * R, :, :] < ref["events"][:, None, None]).any()          # a window row off the grid somewhere
    assert ref["rn"].any() and ref["inside"].max() >= 1 and int(ref["events"].sum()) == c["composited"]


# ------------------------------------------------------------------------------------------------------------------ 2. cuts and order
@pytest.mark.parametrize("shape,lid", [("odd", "c16-vec"), ("even", "c3-ldc5")], ids=["odd-c16-vec", "even-c3-ldc5"])
def test_the_cut_into_batches_and_the_order_do_not_matter(shape, lid):
    mask, fields, _ = _frames(shape, LAYOUTS[lid][1])
    groups = [0, 1, 1, 0, 1]
    states = []
    for batch, cuts, order in ((5, [5], range(B)), (3, [2, 3], range(B)), (1, [1] * 5, range(B)), (5, [5], range(B - 1, -1, -1))):
        order = list(order)
        pipe = _Pipe(shape, lid, batch=batch)
        comp, ref, at = pipe.comp(), None, 0
        for n in cuts:
            idx = order[at:at + n]
            at += n
            pipe.run(mask[idx], fields[idx], n)
            comp(pipe.dev_fields, groups=[groups[i] for i in idx] + [0] * (batch - n), n_valid=n)
            if not states:
                ref = pipe.reference(comp, [groups[i] for i in idx], ref)[2]
        states.append(comp.state())
        if ref is not None:
            uc.assert_state(states[0], ref, "five frames at once")
    for s, what in zip(states[1:], ("2 + 3", "1 x 5", "reversed")):
        uc.assert_state(s, states[0], what)
    assert states[0]["events"].sum() > 20


# ------------------------------------------------------------------------------------------------------------------ 3. no trace
@pytest.mark.parametrize("shape,lid", [("odd", "c3-ldc5"), ("even", "c16-vec")], ids=["odd-c3-ldc5", "even-c16-vec"])
def test_skipped_frames_and_padding_leave_no_trace(shape, lid):
    pipe = _standard(shape, lid)[0]
    comp = pipe.comp()
    stores = {}
    for name in ("_events", "_sum", "_n", "_inside", "_rsum", "_rn", "_counts", "_centers", "_egroup"):
        t = getattr(comp, name)
        store = torch.zeros(t.numel() + 2 * GUARD, dtype=t.dtype, device=DEV)
        store[:GUARD] = SENTINEL
        store[GUARD + t.numel():] = SENTINEL
        stores[name] = store
        setattr(comp, name, store[GUARD:GUARD + t.numel()].view(t.shape))
    comp._centers.fill_(SENTINEL), comp._egroup.fill_(SENTINEL)
    guards_ok = lambda: all(bool((s[:GUARD] == SENTINEL).all()) and bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())  # noqa: E731
    table = [1, -1, 0, 1, 0]                             # frame 1 is skipped, frame 4 is padding
    comp(pipe.dev_fields, groups=table, n_valid=NV)
    cen, egr, ref = pipe.reference(comp, table)
    uc.assert_state(comp.state(), ref, "guarded")
    assert guards_ok()
    got_c, got_g = comp._centers.cpu().numpy(), comp._egroup.cpu().numpy()
    assert np.array_equal(got_c[:NV], cen) and np.array_equal(got_g[:NV], egr)
    assert (got_c[1] == -1).all() and (got_g[1] == -1).all()                       # the skipped frame: -1 everywhere, nothing counted
    assert (got_c[NV:] == SENTINEL).all() and (got_g[NV:] == SENTINEL).all()       # the padding frame: not written
    assert pipe.ncomp[1, 0] > 0
    comp.reset()
    assert guards_ok() and all(not bool(stores[k][GUARD:-GUARD].any()) for k in ("_events", "_sum", "_n", "_inside", "_rsum", "_rn", "_counts"))
    comp(pipe.dev_fields, groups=table, n_valid=NV)      # after a reset: the same state again
    uc.assert_state(comp.state(), ref, "after reset")
    with served("all skipped") as names:                 # nothing to add: nothing is launched
        comp(pipe.dev_fields, groups=[-1] * B, n_valid=NV)
        comp(pipe.dev_fields, groups=0, n_valid=0)
    assert names == []
    uc.assert_state(comp.state(), ref, "after skipped calls")


# ------------------------------------------------------------------------------------------------------------------ 4. the options
@pytest.mark.parametrize("shape,lid", CASES, ids=CASE_IDS)
def test_options_differ_exactly_as_the_checker_says(shape, lid):
    pipe, _, _, standard = _standard(shape, lid)
    groups = [0, 1, 1, 0, 0]
    variants = {"no flip": {"flip_south": False}, "no negate": {"negate": ()},
                "max, both classes, no edges": {"center_stat": "max", "classes": (1, 2), "intensity_edges": (), "min_pixels": 0, "groups": 3},
                "no radial": {"bins": 0}, "many bins": {"bins": 255, "bin_km": 20.0}}
    for what, kw in variants.items():
        comp = pipe.comp(**kw)
        comp(pipe.dev_fields, groups=groups, n_valid=NV)
        cen, egr, ref = pipe.reference(comp, groups)
        assert np.array_equal(comp.centers.cpu().numpy(), cen) and np.array_equal(comp.event_groups.cpu().numpy(), egr), what
        got = comp.state()
        uc.assert_state(got, ref, what)
        if what in ("no flip", "no negate"):
            assert not np.array_equal(got["sum"], standard["sum"]) and np.array_equal(got["events"], standard["events"]), what
        if what == "no negate":
            assert np.array_equal(got["n"], standard["n"]) and np.array_equal(np.abs(got["sum"][..., 1]), np.abs(standard["sum"][..., 1]))
        if what == "no radial":
            assert got["rsum"].shape == (comp.GT, 0, comp.C) and np.array_equal(got["sum"], standard["sum"])
        if what == "max, both classes, no edges":
            assert ref["counts"]["other_class"] == 0 and ref["counts"]["below_min_pixels"] == 0 and not ref["events"][2]


def test_a_radial_table_too_large_for_lds_goes_to_global_memory():
    """255 bins of 20 channels are more radial words than the workgroup's LDS table holds: the adds go to global memory directly"""
    shape, lid = "odd", "c20-vec"
    mask, fields, _ = _frames(shape, LAYOUTS[lid][1])
    pipe = _Pipe(shape, lid).run(mask, fields, NV)
    comp = pipe.comp(bins=255, bin_km=20.0)
    with served("StormComposite") as names:
        comp(pipe.dev_fields, groups=[0, 1, 1, 0, 0], n_valid=NV)
    assert names == ["composite_centers", SERVED[lid]]
    ref = pipe.reference(comp, [0, 1, 1, 0, 0])[2]
    uc.assert_state(comp.state(), ref, "255 bins x 20 channels")
    assert ref["rn"].any() and comp.NB * comp.C > 4096


def test_a_null_radius_table_leaves_the_radial_sums_untouched():
    pipe, cen, egr, standard = _standard("odd", "c16-vec")
    comp = pipe.comp()
    comp(pipe.dev_fields, groups=[0, 1, 1, 0, 0], n_valid=NV)                      # leaves centers and egroup behind
    comp.reset()
    comp._rsum.fill_(SENTINEL), comp._rn.fill_(SENTINEL)
    cat = pipe.catalog
    L.call("dc_composite_accumulate", cat.B, NV, cat.H, cat.W, cat.cap, comp.R, comp.GT, L.dptr(comp._centers), L.dptr(comp._egroup),
           L.dptr(cat._table), L.dptr(cat._labels), L.dptr(pipe.dev_fields), comp.C, pipe.ldc, None, L.dptr(comp._bits), comp.negate_mask,
           1, None, 0, L.dptr(comp._events), L.dptr(comp._sum), L.dptr(comp._n), L.dptr(comp._inside), L.dptr(comp._rsum), L.dptr(comp._rn),
           L.stream_ptr())
    assert bool((comp._rsum == SENTINEL).all()) and bool((comp._rn == SENTINEL).all())
    for k in ("events", "sum", "n", "inside"):
        assert np.array_equal(getattr(comp, "_" + k).cpu().numpy(), standard[k]), k


# ------------------------------------------------------------------------------------------------------------------ 5. a long worklist
@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5"])
def test_more_events_in_a_frame_than_a_worklist_chunk(lid):
    """a lattice of one-pixel events (4-connectivity keeps diagonal neighbours apart): more than a chunk of them in ONE frame, so the
    frame's worklist is worked off in several rounds; three groups' worth of intensity bins so that a chunk holds several groups"""
    W = 48
    need = _chunk() + 40
    H = 2 * (-(-need // (W // 2)))
    R, ldc = 2, LAYOUTS[lid][1]
    rs = np.random.RandomState(5)
    mask = np.zeros((2, H, W), np.uint8)
    mask[0, ::2, ::2] = 1
    mask[1, 1::2, 1::4] = 1
    fields = ((rs.rand(2, H, W, ldc) - 0.5) * 2000.0).astype(np.float32)
    pipe = _Pipe((H, W, R), lid, batch=2, cap=need + 100, connectivity=4).run(mask, fields)
    comp = pipe.comp(min_pixels=0, groups=1, intensity_edges=(-300.0, 300.0), bins=3, bin_km=900.0)
    comp(pipe.dev_fields)
    cen, egr, ref = pipe.reference(comp, [0, 0])
    assert (cen[0] >= 0).sum() == (H // 2) * (W // 2) > _chunk() and ref["events"].min() > 0
    assert np.array_equal(comp.centers.cpu().numpy(), cen) and np.array_equal(comp.event_groups.cpu().numpy(), egr)
    uc.assert_state(comp.state(), ref, "lattice")


# ------------------------------------------------------------------------------------------------------------------ 6. errors, the bound
def test_errors_raise_and_launch_nothing():
    pipe = _standard("odd", "c3-ldc5")[0]
    comp = pipe.comp()
    f = pipe.dev_fields
    bad_calls = [lambda: comp(f[:4]), lambda: comp(f.double()), lambda: comp(f.cpu()), lambda: comp(f[..., :4].contiguous()),
                 lambda: comp(f, groups=[0, 1, 2, 0, 0]), lambda: comp(f, groups=2), lambda: comp(f, groups=[0] * 4), lambda: comp(f, n_valid=B + 1)]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"radius": 0}, {"radius": 41}, {"radius": 10}, {"channels": [5]}, {"channels": []}, {"bits": [0]}, {"classes": ()},
                   {"classes": (3,)}, {"min_pixels": -1}, {"groups": 0}, {"intensity_edges": (2.0, 1.0)}, {"intensity_edges": (float("nan"),)},
                   {"negate": (3,)}, {"bins": 256}, {"bin_km": 0.0}, {"center_stat": "mean"}):
            with pytest.raises(L.DeepcamHipError):
                pipe.comp(**kw)
                pytest.fail(f"{kw} was accepted")
        with pytest.raises(L.DeepcamHipError):
            dnn.StormComposite(pipe.efields, pipe.ldc)
    assert names == []
    assert not comp.state()["events"].any()
    comp._events[1] = dnn.COMPOSITE_MAX_EVENTS                                      # the bound of the integer sums
    with pytest.raises(L.DeepcamHipError, match="events"):
        comp.state()


# ------------------------------------------------------------------------------------------------------------------ 7. driver
def _h5_write(path, datasets):
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with h5.File(path, "w") as f:
        for name, array in datasets.items():
            if backend == "h5py":
                f.create_dataset(name, data=array)
            else:
                f.write(name, array)


def _h5_read(path, names):
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with (h5.File(path, "r") if backend == "h5py" else h5.File(path)) as f:
        return {n: (f[n][...] if backend == "h5py" else f.read(n)) for n in names}


def test_predict_cli_with_composites(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(29)
    dates = ["2003-01-05", "2003-01-17", "2003-02-10"]                                   # two of January, one of February
    names = [f"data-{d}-00-1.h5" for d in dates]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    for name, d in zip(names, fields):
        _h5_write(os.path.join(root, name), {"climate/data": d})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "fp32", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2"]
    out = str(tmp_path / "out")
    chans, cc, R, NB, km = [3, 0, 7], 5, 4, 5, 300.0
    edge = float(np.float32(np.median([d[..., cc].min() for d in fields]) + 0.5))
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", *base, "--output_dir", out, "--batch_size", "2", "--composites",
           "--composite_center_channel", str(cc), "--composite_radius", str(R), "--composite_channels", *map(str, chans), "--composite_negate", "0",
           "--composite_classes", "1", "2", "--composite_min_pixels", "3", "--composite_by", "month", "--composite_intensity_edges", str(edge),
           "--composite_bin_km", str(km), "--composite_bins", str(NB)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)       # batches of two: a ragged last batch
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["events_overflowed_files"] == 0
    bits = [int(b) for b in dnn.composite_bits(lo, hi)[chans]]
    rbin = dnn.composite_radius_table(H, W, R, km, NB)
    catalog = dnn.EventCatalog(1, H, W, connectivity=8, device=DEV)
    ref = uc.empty(12 * 2, R, len(chans), NB)
    for name, d, g in zip(names, fields, [0, 0, 1]):
        f = _h5_read(os.path.join(out, name), ["prediction", "events", "event_fields"])
        rows, frows = f["events"].reshape(-1, 10), f["event_fields"].reshape(-1, 16, 6)
        labels = catalog(_dev(f["prediction"].astype(np.uint8)[None])).labels.cpu().numpy()
        cen, egr = uc.centers(rows[None], [[len(rows), 0, 0]], frows[None], H, W, cc, "min", (1, 2), 3, [g], 12, [edge], ref["counts"])
        uc.accumulate(ref, cen, egr, rows[None], labels, d[None], chans, bits, [1], True, rbin, R)
    got = _h5_read(os.path.join(out, "composites.h5"), list(uc.KEYS) + ["counts", "bits", "channels", "edges", "group_names", "mean", "footprint",
                                                                         "radial_mean", "radius_km", "radius_of_max_km"])
    counts = got.pop("counts")
    got["counts"] = dict(zip(uc.COUNTS, counts.tolist()))
    uc.assert_state(got, ref, "composites.h5")
    assert ref["events"].sum() > 0 and ref["events"][4:].sum() == 0
    assert got["bits"].tolist() == bits and got["channels"].tolist() == chans and got["edges"].tolist() == [np.float32(edge)]
    assert bytes(got["group_names"]).decode().split(",")[:3] == ["01.bin0", "01.bin1", "02.bin0"]
    dec = dnn.StormComposite.decode(*(ref[k] for k in uc.KEYS), bits, km)
    for k, v in dec.items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    entry = summary["composites"]
    assert entry["counts"] == ref["counts"] and entry["events"] == ref["events"].tolist() and entry["channels"] == chans
    # without the flag: the same files and nothing of the family launched
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "3", "--event_fields"])
    with served("predict without --composites") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("composite")]
    assert sorted(os.listdir(plain)) == sorted(set(os.listdir(out)) - {"composites.h5"})
    assert "composites" not in json.load(open(os.path.join(plain, "summary.json")))
    for n in names:
        a, b = (_h5_read(os.path.join(p, n), ["prediction", "events", "event_fields"]) for p in (plain, out))
        assert all(np.array_equal(a[k], b[k]) for k in a)
