"""Climatology on the GPU (dc_climatology_accumulate / dc_climatology_maps of csrc/climatology.hip, nn.Climatology, predict.py
--climatology) against the numpy checker of tests/util_climatology.py.  Everything is an integer, or an fp32 word made by two defined
roundings: every comparison is equality.  The shapes come from the kernel's own workgroup (dc_climatology_block): one frame smaller than
a workgroup with an odd pixel count, one of three workgroups with a ragged last one; widths >= 8 that are no multiple of 4."""
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
import util_climatology as uc  # noqa: E402
import util_render as ur  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV = 5, 4
GUARD, SENTINEL = 64, 0x5A

LAYOUTS = [(16, 16, None), (3, 5, [4, 0, 2]), (1, 1, [0]), (0, 0, [])]            # (C, ldc, chan); None: the identity over ldc
LAYOUT_IDS = ["c16-vec", "c3-ldc5", "c1", "c0"]
SERVED = {"c16-vec": "climatology_accumulate_vec", "c3-ldc5": "climatology_accumulate_scalar", "c1": "climatology_accumulate_scalar",
          "c0": "climatology_accumulate_scalar"}


@functools.lru_cache(maxsize=None)
def _block():
    p = C.c_int(0)
    assert L.load().dc_climatology_block(C.byref(p)) == 0 and p.value > 0
    return p.value


@functools.lru_cache(maxsize=None)
def _shape(name):
    P = _block()
    if name == "small":                              # fewer pixels than a workgroup, an odd count
        W = 9
        H = max((P - 1) // W, 1)
        H -= (H * W) % 2 == 0
        assert 0 < H * W < P and (H * W) % 2 == 1
    else:                                            # three workgroups, the last one ragged
        W = 17
        H = 2 * P // W + 2
        assert 2 * P < H * W < 3 * P and (H * W) % P != 0
    assert W >= 8 and W % 4 != 0
    return H, W


def _chan(layout):
    C_, ldc, chan = layout
    return list(range(C_)) if chan is None else chan


def _bits(C_):
    return [(3 * c) % 7 for c in range(C_)]            # values of a few thousand times at most 2^6: far inside 2^40


def _masks(n, H, W, seed):
    """uint8 [n, H, W]: about 45 % foreground, with values 3 and 255 (background) among the rest"""
    rs = np.random.RandomState(seed)
    return rs.choice(np.asarray([0, 1, 2, 3, 255], np.uint8), size=(n, H, W), p=[0.45, 0.25, 0.20, 0.05, 0.05])


def _fields(n, H, W, ldc, seed):
    rs = np.random.RandomState(seed + 1)
    return ((rs.rand(n, H, W, max(ldc, 1)) - 0.3) * 4000.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(shape, ldc):
    """The standard batch of five: random, all background, uniformly class 2, random, and a padding frame (all class 1 over NaN fields)
    that must leave no trace.  Shared and never modified."""
    H, W = _shape(shape)
    mask = _masks(B, H, W, 40 + H)
    mask[1], mask[2], mask[4] = 0, 2, 1
    fields = _fields(B, H, W, ldc, 50 + H)
    fields[4] = np.nan
    mask.setflags(write=False), fields.setflags(write=False)
    return mask, fields


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared batches are read-only


def _make(batch, H, W, layout, G=1):
    C_, ldc, chan = layout
    return dnn.Climatology(batch, H, W, channels=_chan(layout), bits=_bits(C_), ldc=ldc, groups=G, device=DEV)


def _assert_state(got, ref, what=""):
    for k in uc.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())


def _with_fields(layout, fields):
    return fields if layout[0] else None


# ------------------------------------------------------------------------------------------------------------------ 1. layouts and masks
@functools.lru_cache(maxsize=None)
def _standard_reference(shape, lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    H, W = _shape(shape)
    mask, fields = _batch(shape, layout[1])
    group = [0] * NV + [-1] * (B - NV)
    return uc.reference([(mask, _with_fields(layout, fields), group)], 1, H, W, _chan(layout), _bits(layout[0]))


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("shape", ["small", "large"])
def test_accumulators_equal_the_checker(shape, lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    H, W = _shape(shape)
    mask, fields = _batch(shape, layout[1])
    clim = _make(B, H, W, layout)
    with served("Climatology") as names:
        clim(_dev(mask), _dev(_with_fields(layout, fields)), n_valid=NV)
    assert names == [SERVED[lid]]
    ref = _standard_reference(shape, lid)
    _assert_state(clim.state(), ref, lid)
    assert ref["frames"].tolist() == [NV] and clim.host_frames == [NV]
    assert (ref["count"][0, 1] >= 1).all() and ref["count"].max() <= NV          # the class-2 frame reached every pixel, the padding none
    if layout[0]:
        assert ref["n"][0, 0].min() == NV and 0 < ref["n"][0, 1].max() < NV


# ------------------------------------------------------------------------------------------------------------------ 2. mask element sizes
@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64], ids=["u8", "i32", "i64"])
def test_mask_element_sizes(dtype):
    layout, lid = LAYOUTS[0], LAYOUT_IDS[0]
    H, W = _shape("large")
    mask, fields = _batch("large", layout[1])
    assert (mask == 3).any() and (mask == 255).any()
    m = mask.astype(dtype)
    if dtype != np.uint8:                             # background whose low byte or low word is a class
        rs = np.random.RandomState(3)
        m[(mask == 0) & (rs.rand(*mask.shape) < 0.5)] = 256 + 1
        m[mask == 255] = -1
        if dtype == np.int64:
            m[mask == 3] = (1 << 32) + 2
    clim = _make(B, H, W, layout)
    clim(_dev(m), _dev(fields), n_valid=NV)
    _assert_state(clim.state(), _standard_reference("large", lid), str(dtype))


# ------------------------------------------------------------------------------------------------------------------ 3. groups
@pytest.mark.parametrize("table,untouched", [([1, 1, -1, 2, 1], 0), ([0, 2, 2, 0, -1], 1)], ids=["change-skip-return", "return-empty"])
@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5"])
def test_groups(lid, table, untouched):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    H, W = _shape("large")
    mask, fields = _batch("large", layout[1])
    clim = _make(B, H, W, layout, G=3)
    clim(_dev(mask), _dev(fields), groups=table)
    got = clim.state()
    _assert_state(got, uc.reference([(mask, fields, table)], 3, H, W, _chan(layout), _bits(layout[0])), str(table))
    assert got["frames"][untouched] == 0 and not got["count"][untouched].any() and not got["sum"][untouched].any() \
        and not got["n"][untouched].any()
    assert clim.host_frames == got["frames"].tolist()


# ------------------------------------------------------------------------------------------------------------------ 4. the cut into batches
@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5"])
def test_the_cut_into_batches_does_not_matter(lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    H, W = _shape("large")
    n = 7
    mask, fields = _masks(n, H, W, 7), _fields(n, H, W, layout[1], 8)
    groups = [0, 0, 1, 1, 0, 1, 1]
    ref = uc.reference([(mask, fields, groups)], 2, H, W, _chan(layout), _bits(layout[0]))
    for batch in (7, 4, 1):
        clim = _make(batch, H, W, layout, G=2)
        for s in range(0, n, batch):
            nv = min(batch, n - s)
            m = np.ones((batch, H, W), np.uint8)                                   # padding: all class 1 over NaN
            f = np.full((batch, H, W, layout[1]), np.nan, np.float32)
            m[:nv], f[:nv] = mask[s:s + nv], fields[s:s + nv]
            clim(_dev(m), _dev(f), groups=groups[s:s + nv] + [0] * (batch - nv), n_valid=nv)
        _assert_state(clim.state(), ref, f"batch {batch}")
    # two calls on one object: one checker pass over both batches
    clim = _make(B, H, W, layout, G=2)
    first, second = _batch("large", layout[1]), (mask[:B], fields[:B])
    tables = ([0, 1, 1, 0, -1], [1, 1, 0, -1, 1])
    for (m, f), t in zip((first, second), tables):
        clim(_dev(m), _dev(f), groups=t)
    _assert_state(clim.state(), uc.reference([(*first, tables[0]), (*second, tables[1])], 2, H, W, _chan(layout), _bits(layout[0])), "two calls")


# ------------------------------------------------------------------------------------------------------------------ 5. special values
@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5"])
def test_special_values(lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    C_, ldc = layout[0], layout[1]
    H, W = _shape("large")
    mask = _masks(2, H, W, 90)
    bits = [2] * C_
    largest = np.float32(2.0 ** 38)                                                # 2^38 * 2^2 = 2^40: the largest value that still fits
    beyond = np.nextafter(largest, np.float32(np.inf))
    excluded = np.asarray([np.nan, np.inf, -np.inf, beyond, -beyond, 1e30, -3e38], np.float32)
    included = np.asarray([-0.0, 0.0, 1e-45, -1e-40, 1.1754942e-38, largest, -largest, 0.125, 0.375, -0.125, 2.5], np.float32)
    values = np.concatenate([excluded, included])
    rs = np.random.RandomState(91)
    fields = rs.choice(values, size=(2, H, W, ldc)).astype(np.float32)
    clim = dnn.Climatology(2, H, W, channels=_chan(layout), bits=bits, ldc=ldc, device=DEV)
    clim(_dev(mask), _dev(fields))
    got = clim.state()
    _assert_state(got, uc.reference([(mask, fields, [0, 0])], 1, H, W, _chan(layout), bits), "special")
    counted = ~np.isin(np.ascontiguousarray(fields[..., _chan(layout)]).view(np.uint32), excluded.view(np.uint32))    # by bit pattern: NaN included
    assert np.array_equal(got["n"][0, 0], counted.sum(axis=0)) and 0 < counted.sum() < counted.size
    assert np.abs(got["sum"]).max() >= 1 << 40                                     # the limit itself was added somewhere


# ------------------------------------------------------------------------------------------------------------------ 6. guard words, reset
@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5", "c0"])
def test_guard_words_and_reset(lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    H, W = _shape("large")
    mask, fields = _batch("large", layout[1])
    clim = _make(B, H, W, layout, G=2)
    stores = {}
    for name in ("_frames", "_count", "_sum", "_n"):
        t = getattr(clim, name)
        if t is None:
            continue
        store = torch.zeros(t.numel() + GUARD, dtype=t.dtype, device=DEV)
        store[t.numel():] = SENTINEL
        stores[name] = store
        setattr(clim, name, store[:t.numel()].view(t.shape))
    guards_ok = lambda: all(bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())  # noqa: E731
    table = [1, 0, 1, 1, -1]
    clim(_dev(mask), _dev(_with_fields(layout, fields)), groups=table)
    ref = uc.reference([(mask, _with_fields(layout, fields), table)], 2, H, W, _chan(layout), _bits(layout[0]))
    _assert_state(clim.state(), ref, "guarded")
    assert guards_ok()
    clim.reset()
    assert guards_ok() and all(not bool(s[:-GUARD].any()) for s in stores.values()) and clim.host_frames == [0, 0]
    clim(_dev(mask), _dev(_with_fields(layout, fields)), groups=table)           # after a reset: the same state again
    _assert_state(clim.state(), ref, "after reset")
    assert guards_ok()


# ------------------------------------------------------------------------------------------------------------------ 7. maps
def _products(C_):
    return [("frequency", 1), ("mean", 0, 0), ("share", C_ - 1, 2), ("mean", C_ - 1, 1), ("frequency", 2), ("share", 0, 1), ("mean", 1 % C_, "class2")]


@pytest.mark.parametrize("lid", ["c16-vec", "c3-ldc5"])
def test_maps_equal_the_checker_bit_for_bit(lid):
    layout = LAYOUTS[LAYOUT_IDS.index(lid)]
    C_ = layout[0]
    H, W = _shape("large")
    mask, fields = _batch("large", layout[1])
    fields = fields.copy()
    fields[:, 0, :3] = np.nan                           # pixels without a value: n == 0
    fields[:, 1, :3] = 0.0                              # pixels whose sums are zero: sum_all == 0
    table = [0, 2, 2, 0, -1]                            # group 1 receives nothing: frames == 0
    clim = _make(B, H, W, layout, G=3)
    clim(_dev(mask), _dev(fields), groups=table)
    state = clim.state()
    assert state["frames"][1] == 0 and (state["n"][0, 0] == 0).any() and ((state["sum"][0, 0] == 0) & (state["n"][0, 0] > 0)).any()
    products = _products(C_)
    numeric = [(p[0],) + tuple(dnn.CLIMATOLOGY_ROWS.index(a) if isinstance(a, str) else a for a in p[1:]) for p in products]
    f1 = uc.product(state, clim.bits, ("frequency", 1))
    exact = float(np.unique(f1[(f1 > 0) & (f1 < 1)])[0])                            # a frequency that occurs: the equality case of >=
    for t1, t2 in ((exact, 0.5), (0.75, float(np.nextafter(np.float32(0.5), np.float32(1))))):
        with served("Climatology.fields") as names:
            out, contour = clim.fields(products, t1, t2)
        assert names == ["climatology_maps"]
        ref_out, ref_contour = uc.maps(state, clim.bits, numeric, t1, t2)
        assert out.dtype == torch.float32 and tuple(out.shape) == (3, H, W, len(products)) and contour.dtype == torch.uint8
        assert uc.same_bits(out.cpu().numpy(), ref_out)
        assert np.array_equal(contour.cpu().numpy(), ref_contour)
        assert set(np.unique(ref_contour[0]).tolist()) == {0, 1, 2} and not ref_contour[1].any()
    assert (uc.maps(state, clim.bits, numeric, exact, 0.5)[1] == 1).sum() > (uc.maps(state, clim.bits, numeric, np.nextafter(np.float32(exact), np.float32(1)), 0.5)[1] == 1).sum()
    assert np.isnan(ref_out[1, ..., 1]).all() and not ref_out[1, ..., 0].any()   # the empty group: means NaN, frequencies 0
    assert np.isnan(ref_out[0, 0, :3, 1]).all() and np.isnan(ref_out[0, 1, :3, 5]).all()
    # the host maps are the same quotients before the second rounding
    m = clim.maps()
    assert np.array_equal(m["frequency"][0, 0].astype(np.float32), ref_out[0, ..., 0])
    assert uc.same_bits(m["mean"][0, 0, :, :, 0].astype(np.float32), ref_out[0, ..., 1])


# ------------------------------------------------------------------------------------------------------------------ 8. rendering
def test_the_maps_render_through_the_frame_renderer():
    layout = LAYOUTS[1]
    H, W = _shape("large")
    mask, fields = _batch("large", layout[1])
    G, table = 2, [0, 1, 1, 0, -1]
    clim = _make(B, H, W, layout, G=G)
    clim(_dev(mask), _dev(fields), groups=table)
    products = [("frequency", 1), ("mean", 2, 0), ("frequency", 2)]
    out, contour = clim.fields(products, 0.5, 0.5)
    r = dnn.FrameRenderer(G, H, W, channel=2, ldc=len(products), lo=0.0, hi=1.0, panels=1, device=DEV)
    img = r(out, contour)
    ref_out, ref_contour = uc.maps(clim.state(), clim.bits, products, 0.5, 0.5)
    ref = ur.render(ref_out, 2, np.float32(r.lo), np.float32(r.scale), r.palette, [ref_contour], r.rows, r.shift, *r.lines, 3)
    assert np.array_equal(img.cpu().numpy(), ref.reshape(G, r.Ho, W, 3))
    assert set(np.unique(ref_contour).tolist()) == {0, 1, 2}


# ------------------------------------------------------------------------------------------------------------------ 9. driver
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


def test_predict_cli_with_climatology(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(23)
    dates = ["2003-01-05", "2003-01-17", "2003-01-29", "2003-02-10", "2003-02-22"]       # three of January, two of February
    names = [f"data-{d}-00-1.h5" for d in dates]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    truth = [rs.choice(np.asarray([0, 1, 2], np.int64), size=(H // 8, W // 8), p=[0.6, 0.2, 0.2]).repeat(8, 0).repeat(8, 1) for _ in names]
    for name, d, t in zip(names, fields, truth):
        _h5_write(os.path.join(root, name), {"climate/data": d, "climate/labels_0": t})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "fp32", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2"]
    out = str(tmp_path / "out")
    chans = [0, 3]
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", *base, "--output_dir", out, "--batch_size", "2", "--climatology",
           "--climatology_by", "month", "--climatology_channels", "0", "3", "--verify", "--plots", "--plot_every", "5", "--climatology_contour", "0.5"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)       # batches of two: January and February share one
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    pred = [_h5_read(os.path.join(out, n), ["prediction"])["prediction"] for n in names]
    bits = [int(b) for b in dnn.event_field_bits(lo, hi)[chans]]
    group = [0, 0, 0, 1, 1]
    got = _h5_read(os.path.join(out, "climatology.h5"), ["frames", "count", "sum", "n", "bits", "channels", "truth_count", "truth_sum", "truth_n"])
    ref = uc.reference([(np.stack(pred), np.stack(fields), group)], 12, H, W, chans, bits)
    ref_truth = uc.reference([(np.stack(truth), np.stack(fields), group)], 12, H, W, chans, bits)
    _assert_state(got, ref, "prediction")
    _assert_state({"frames": got["frames"], **{k: got["truth_" + k] for k in ("count", "sum", "n")}}, ref_truth, "labels")
    assert got["bits"].tolist() == bits and got["channels"].tolist() == chans and got["bits"].dtype == np.int32
    assert ref["frames"].tolist() == [3, 2] + [0] * 10 and ref_truth["count"][:2].any() and ref_truth["sum"][0, 1].any()
    maps = dnn.Climatology.decode(*(ref[k] for k in uc.KEYS), bits, H, W)
    maps_truth = dnn.Climatology.decode(*(ref_truth[k] for k in uc.KEYS), bits, H, W)
    entry = summary["climatology"]
    plots = sorted(predict.climatology_plot_name(g, k) for g in ("01", "02") for k in (1, 2))
    assert entry.pop("plots") == plots
    assert entry == predict.climatology_summary("month", ref["frames"], maps, maps_truth, chans)
    assert entry["frames"][:3] == [3, 2, 0] and entry["area_frequency"]["class_1"][2] is None and entry["truth_area_frequency"]["class_2"][0] > 0
    Ho = len(dnn.gall_rows(H, W))
    from mlperf_deepcam_amd import png
    for name in plots:
        path = os.path.join(out, "plots", name)
        assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n", name
        assert png.read_png(path).shape == (2 * Ho, W, 3)                               # the prediction above the labels
    assert len([p for p in os.listdir(os.path.join(out, "plots")) if p.startswith("climatology-")]) == 4
    # without the flag: no file, no entry, and no launch of the family (one batch of all five files, recorded on this thread)
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "5", "--climatology_by", "month"])
    with served("predict without --climatology") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("climatology")]
    assert not os.path.exists(os.path.join(plain, "climatology.h5")) and os.path.exists(os.path.join(plain, names[0]))
    assert "climatology" not in json.load(open(os.path.join(plain, "summary.json")))
    for n, p in zip(names, pred):
        assert np.array_equal(_h5_read(os.path.join(plain, n), ["prediction"])["prediction"], p)


# ------------------------------------------------------------------------------------------------------------------ 10. errors
def test_errors_raise_and_launch_nothing():
    layout = LAYOUTS[1]
    H, W = _shape("small")
    clim = _make(B, H, W, layout, G=2)
    mask = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    fields = torch.zeros((B, H, W, layout[1]), dtype=torch.float32, device=DEV)
    bad_calls = [
        lambda: clim(mask[:, :, :-1].contiguous(), fields),                       # a wrong mask shape
        lambda: clim(mask[:4], fields),
        lambda: clim(mask.to(torch.int16), fields),
        lambda: clim(mask.cpu(), fields),
        lambda: clim(mask, fields.double()),                                       # fields of another dtype
        lambda: clim(mask, fields.half()),
        lambda: clim(mask, fields[..., :4].contiguous()),
        lambda: clim(mask, None),                                                  # channels were selected
        lambda: clim(mask, fields, groups=[0, 1, 2, 0, 0]),                        # a group index >= G
        lambda: clim(mask, fields, groups=2),
        lambda: clim(mask, fields, groups=[0, 1, 0, 1]),                           # a table of the wrong length
        lambda: clim(mask, fields, groups=[0] * 6),
        lambda: clim(mask, fields, n_valid=B + 1),
        lambda: clim.fields([("frequency", 3)]),
        lambda: clim.fields([("mean", 3, 0)]),
        lambda: clim.fields([("share", 0, 0)]),
        lambda: clim.fields([("median", 0, 0)]),
        lambda: clim.fields([]),
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
    assert names == []
    state = clim.state()
    assert clim.host_frames == [0, 0] and not state["frames"].any() and not state["count"].any() and not state["sum"].any()
    clim.host_frames[1] = dnn.CLIMATOLOGY_MAX_FRAMES - 2                            # the frame bound, counted on the host
    with served("bound") as names:
        with pytest.raises(L.DeepcamHipError, match="frames"):
            clim(mask, fields, groups=[1, 1, 1, 0, 0])
    assert names == [] and clim.host_frames[0] == 0
    for kw in ({"channels": list(range(33)), "bits": [0] * 33}, {"channels": [5], "bits": [0], "ldc": 5}, {"channels": [0], "bits": []},
               {"groups": 0}, {"channels": [-1], "bits": [0]}):
        with pytest.raises(L.DeepcamHipError):
            dnn.Climatology(B, H, W, **{"device": DEV, **kw})
    with pytest.raises(L.DeepcamHipError):
        dnn.Climatology(0, H, W, device=DEV)
    with served("all skipped") as names:                                            # nothing to add: nothing is launched
        clim(mask, fields, groups=[-1] * B)
        clim(mask, fields, n_valid=0)
    assert names == []
