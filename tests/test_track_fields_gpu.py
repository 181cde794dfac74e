"""Storm life cycles on the GPU (dc_track_fields_append / dc_track_cycles of csrc/tracks.hip, nn.TrackFields, predict.py --track_fields)
against the numpy checker of tests/util_track_fields.py, which test_track_fields_cpu.py holds against a brute force over pixels.  Everything
is integer: every comparison is np.array_equal.

The frames are those of tests/util_track_fields.py (test_track_fields_cpu.py asserts that they contain steps of several events, extremes
that tie across fragments and across frames, tracks the selection filters and more track rows than one workgroup ranks).  A sequence is
fed as batches whose padding samples are all class 1 with huge field values -- they would join and outbid everything if they were read --
and every buffer the calls fill is pre-filled with a sentinel, so that rows behind the filled parts are seen to be untouched."""
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
import util_track_fields as uf  # noqa: E402
import util_tracks as ut  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
CAP, EVENT_CAP, SENTINEL = 512, 8192, -77
LAYOUTS = [(1, 1), (3, 4), (3, 5), (16, 16)]          # (C, ldc): ldc 4 and 16 take the field pass's 16-byte loads, 1 and 5 its scalar ones
LAYOUT_IDS = ["c1", "c3-ldc4", "c3-ldc5", "c16"]
TABLES = ("ncycles", "offsets", "steps", "step_fields", "track_fields")


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


def _frames(kind, name, C_, ldc, special=False):
    return uf.drawn(name, C_, ldc) if kind == "drawn" else uf.random_sequence(name, C_, ldc, special)


@functools.lru_cache(maxsize=None)
def _reference(kind, name, C_, ldc, special=False, frames=None, conn=8, wrap=True, **kw):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    masks, fields = _frames(kind, name, C_, ldc, special)
    masks, fields = masks[:frames], fields[:frames]
    return uf.reference(masks, fields, conn, wrap, _tables(*masks.shape[1:]), C_, uf.scale_bits(C_), **{"cap": CAP, "event_cap": EVENT_CAP, **kw})


# ------------------------------------------------------------------------------------------------------------------ running a sequence
def _objects(B, H, W, C_, ldc, conn=8, wrap=True, cap=CAP, event_cap=EVENT_CAP, track_cap=None, min_pixels=0, step_cap=None):
    cat = dnn.EventCatalog(B, H, W, connectivity=conn, wrap=wrap, cap=cap, device=DEV)
    trk = dnn.EventTracker(cat, event_cap=event_cap, track_cap=track_cap, min_pixels=min_pixels)
    fld = dnn.EventFields(cat, C_, uf.scale_bits(C_), ldc=ldc)
    tf = dnn.TrackFields(trk, fld, step_cap=step_cap)
    for t in (tf._fstore, tf._offsets, tf._steps, tf._step_fields, tf._track_fields, tf._ncycles):
        t.fill_(SENTINEL)
    return cat, trk, fld, tf


def _feed(objs, masks, fields):
    """one call of each object: the frames, then padding up to the catalogue's batch"""
    cat, trk, fld, tf = objs
    nv = len(masks)
    m = np.ones((cat.B, cat.H, cat.W), np.uint8)
    f = np.full((cat.B, cat.H, cat.W, fld.ldc), 1e9, np.float32)
    m[:nv], f[:nv] = masks, fields
    mask, raw = torch.from_numpy(m).to(DEV), torch.from_numpy(f).to(DEV)
    cat(mask, n_valid=nv)
    trk(mask, n_valid=nv)
    fld(raw, n_valid=nv)
    tf()


def _feed_all(objs, masks, fields, start=0, stop=None):
    """frames start .. stop in calls of B, B - 1, B - 2, B, ... frames (at least one): ragged n_valid whatever the batch"""
    B, k, i = objs[0].B, start, 0
    stop = len(masks) if stop is None else stop
    while k < stop:
        n = min(max(B - i % 3, 1), stop - k)
        _feed(objs, masks[k:k + n], fields[k:k + n])
        k, i = k + n, i + 1


def _result(objs, **sel):
    """rows(), the filed field rows, and a look behind every filled part"""
    cat, trk, fld, tf = objs
    for t in (tf._offsets, tf._steps, tf._step_fields, tf._track_fields, tf._ncycles):     # an earlier read may have filled more rows
        t.fill_(SENTINEL)
    r = tf.rows(**sel)
    n, m, s = int(trk._state[0].item()), len(r["tracks"]), len(r["steps"])
    assert m == int(trk._ntracks[3].item()) and s == int(r["counts"][2]) and len(r["offsets"]) == len(r["track_fields"]) == m
    for name, t, k in (("fstore", tf._fstore, n), ("offsets", tf._offsets, m), ("steps", tf._steps, s), ("step_fields", tf._step_fields, s),
                       ("track_fields", tf._track_fields, m)):
        assert (t[k:] == SENTINEL).all().item(), f"{name}: something was written behind the {k} filled rows"
    return {"ncycles": r["counts"], "offsets": r["offsets"], "steps": r["steps"], "step_fields": r["step_fields"],
            "track_fields": r["track_fields"], "tracks": r["tracks"], "frows": tf._fstore[:n].cpu().numpy()}


def _assert_equal(got, ref, keys=TABLES + ("tracks", "frows")):
    for key in keys:
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), \
            f"{key} differs: {got[key].tolist() if got[key].size < 60 else got[key].shape} vs {ref[key].tolist() if ref[key].size < 60 else ref[key].shape}"


def _run(kind, name, C_, ldc, B, special=False, sel=None, **kw):
    masks, fields = _frames(kind, name, C_, ldc, special)
    objs = _objects(B, *masks.shape[1:], C_, ldc, **kw)
    _feed_all(objs, masks, fields)
    return _result(objs, **(sel or {}))


# ------------------------------------------------------------------------------------------------------------------ 1. drawn sequences
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", uf.DRAWN)
def test_drawn_sequences_against_the_checker(name, layout):
    C_, ldc = layout
    B = 1 + (uf.DRAWN.index(name) + LAYOUTS.index(layout)) % 4
    ref = _reference("drawn", name, C_, ldc)
    got = _run("drawn", name, C_, ldc, B)
    _assert_equal(got, ref)
    W, life, steps = uf.DRAWN_SHAPE[1], got["track_fields"], got["steps"]
    frame_of_min, frame_of_max = life[:, 0, 0] & 0xFFFFFFFF, 0xFFFFFFFF - (life[:, 0, 2] & 0xFFFFFFFF)
    if name == "hold":                                   # the minimum of frames 1 and 2 is frame 1's, the maximum of 3 and 4 frame 3's
        assert (frame_of_min[0], life[0, 0, 1], frame_of_max[0], life[0, 0, 3]) == (1, 7 * W + 6, 3, 8 * W + 10)
    elif name == "split_merge":                          # two fragments with equal extremes: the smaller pixel, which is the right fragment's
        assert steps[:, 2].tolist() == [2, 2, 1, 1, 2, 2] and (got["step_fields"][0, 0, 0] & 0xFFFFFFFF) == 7 * W + 16
        assert (frame_of_min[0], life[0, 0, 1], frame_of_max[0], life[0, 0, 3]) == (0, 7 * W + 16, 0, 8 * W + 17)
    elif name == "seam":                                 # one event per frame although it lies on both edges
        assert len(got["tracks"]) == 1 and steps[:, 2].tolist() == [1] * uf.DRAWN_FRAMES and (frame_of_min[0], life[0, 0, 1]) == (3, 6 * W)
    else:                                                # the cyclone and the river keep their own steps
        assert got["tracks"][:, 1].tolist() == [1, 2] and steps[:, :2].tolist() == [[0, f] for f in range(4)] + [[1, f] for f in range(2, 6)]


# ------------------------------------------------------------------------------------------------------------------ 2. random sequences, batching
@pytest.mark.parametrize("case,layout", [("small", (1, 1)), ("wide", (3, 4)), ("large", (16, 16))], ids=["small-c1", "wide-c3", "large-c16"])
def test_the_cut_into_batches_does_not_matter(case, layout):
    C_, ldc = layout
    ref = _reference("random", case, C_, ldc, conn=4)
    assert ref["state"][2] == 0 and ref["state"][3] == 0 and ref["ntracks"][0] == ref["ntracks"][3] and ref["ncycles"][3] == 0
    for B in (1, 2, 3, 4):
        _assert_equal(_run("random", case, C_, ldc, B, conn=4), ref)


# ------------------------------------------------------------------------------------------------------------------ 3. values
@pytest.mark.parametrize("layout", [(3, 4), (3, 5), (1, 1)], ids=["c3-ldc4", "c3-ldc5", "c1"])
def test_special_values(layout):
    C_, ldc = layout
    ref = _reference("random", "wide", C_, ldc, special=True)
    sf = ref["step_fields"]
    assert (sf[:, 0, 4] > 0).any() and (sf[:, 0, 5] > 0).any()                      # NaN / Inf and saturated values in the steps
    if C_ == 3:                                          # empty rows and empty lifetime extremes; -0.0 below +0.0
        assert (sf[:, 1, 0] == -1).any() and (ref["track_fields"][:, 1] == [-1, -1, 0, -1]).all(axis=1).any()
        assert ((ref["track_fields"][:, 2, 0] >> 32 == 0x7FFFFFFF) & (ref["track_fields"][:, 2, 2] >> 32 == -0x80000000)).any()
    _assert_equal(_run("random", "wide", C_, ldc, 3, special=True), ref)


# ------------------------------------------------------------------------------------------------------------------ 4. selection
@pytest.mark.parametrize("sel", [{"min_frames": uf.MIN_FRAMES}, {"classes": (1,)}, {"classes": (2,), "min_frames": 2}, {"min_frames": 0}],
                         ids=["min_frames", "class1", "class2-min2", "min0"])
def test_selection(sel):
    mask = dnn.TrackFields.class_mask(sel.get("classes", (1, 2)))
    ref = _reference("random", "wide", 3, 4, min_frames=sel.get("min_frames", 1), class_mask=mask)
    every = _reference("random", "wide", 3, 4)
    if sel == {"min_frames": 0}:
        assert np.array_equal(ref["offsets"], every["offsets"])                     # 0 selects what 1 selects
    else:
        assert 0 < ref["ncycles"][0] < every["ncycles"][0] and (ref["offsets"] == -1).any()
    _assert_equal(_run("random", "wide", 3, 4, 2, sel=sel), ref)


# ------------------------------------------------------------------------------------------------------------------ 5. capacities
def test_fewer_step_rows_than_needed():
    every = _reference("random", "wide", 3, 4)
    step_cap = int(every["ncycles"][1]) // 2
    ref = _reference("random", "wide", 3, 4, step_cap=step_cap)
    assert (ref["offsets"] == -2).any() and ref["ncycles"][3] > 0 and ref["ncycles"][2] <= step_cap < ref["ncycles"][1] == every["ncycles"][1]
    got = _run("random", "wide", 3, 4, 3, step_cap=step_cap)                        # _result looks at the tail of the step tables
    _assert_equal(got, ref)
    left = ref["offsets"] == -2
    assert (got["track_fields"][left] == [-1, -1, 0, -1]).all() and np.array_equal(got["steps"], every["steps"][:len(got["steps"])])


def test_more_tracks_than_rows():
    every = _reference("random", "wide", 3, 4)
    track_cap = int(every["ntracks"][0]) // 3
    ref = _reference("random", "wide", 3, 4, track_cap=track_cap)
    assert (ref["track_of"] == -1).sum() > 0 and len(ref["offsets"]) == track_cap and ref["ncycles"][1] < every["ncycles"][1]
    _assert_equal(_run("random", "wide", 3, 4, 4, track_cap=track_cap), ref)


def test_more_events_than_the_store_holds():
    total = int(_reference("random", "wide", 3, 4)["state"][0])
    event_cap = total // 2 + 1
    ref = _reference("random", "wide", 3, 4, event_cap=event_cap, step_cap=EVENT_CAP)
    assert ref["state"].tolist()[::2] == [event_cap, total - event_cap] and len(ref["frows"]) == event_cap
    _assert_equal(_run("random", "wide", 3, 4, 3, event_cap=event_cap, step_cap=EVENT_CAP), ref)


def test_more_components_than_the_catalogue_holds():
    ref = _reference("random", "wide", 3, 4, cap=5)
    assert ref["state"][3] > 0
    _assert_equal(_run("random", "wide", 3, 4, 3, cap=5), ref)


def test_more_chunks_of_tracks_than_one_block_of_the_offsets_pass():
    """dc_track_cycles ranks the selected track rows in chunks of 256 and ONE workgroup turns the chunks' frame counts into offsets, 256
    chunks at a time with a carry from block to block (the tracker's resolve does the same with the events).  The checkerboard of
    util_tracks on test_tracks_gpu.py's "tiles" shape gives 71288 events that are 71288 one-frame tracks, 279 chunks of either."""
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    T, H, W = 8, 2 * th.value + 3, 2 * tw.value + 5
    masks = ut.checkerboard(T, H, W)
    fields = np.random.RandomState(77).standard_normal((T, H, W, 1)).astype(np.float32) * 40.0
    kw = {"cap": 16384, "event_cap": 1 << 17, "step_cap": 1 << 17}
    ref = uf.reference(masks, fields, 4, False, _tables(H, W), 1, uf.scale_bits(1), min_frames=1, **kw)
    assert ref["state"].tolist() == [T * H * W, T, 0, 0] and ref["ncycles"].tolist() == [T * H * W, T * H * W, T * H * W, 0]
    objs = _objects(3, H, W, 1, 1, conn=4, wrap=False, **kw)
    _feed_all(objs, masks, fields)
    got = _result(objs, min_frames=1)
    assert int(objs[1]._state[0].item()) > 65536 and int(objs[1]._ntracks[3].item()) > 65536, "fewer than 257 chunks: no carry"
    _assert_equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------ 6. series control
def test_cut_reset_and_reading_in_the_middle():
    masks, fields = _frames("random", "wide", 3, 4)
    other_masks, other_fields = _frames("random", "wide", 3, 4, special=True)
    objs = _objects(3, *masks.shape[1:], 3, 4)
    cat, trk, fld, tf = objs
    # rows() after 5 frames, then the rest: the early read changes nothing later
    _feed_all(objs, masks, fields, 0, 5)
    _assert_equal(_result(objs), _reference("random", "wide", 3, 4, frames=5))
    _feed_all(objs, masks, fields, 5)
    full = _reference("random", "wide", 3, 4)
    _assert_equal(_result(objs), full)
    _assert_equal(_result(objs, min_frames=uf.MIN_FRAMES), _reference("random", "wide", 3, 4, min_frames=uf.MIN_FRAMES))   # and a second read
    # reset(): another series from frame 0
    trk.reset()
    tf._fstore.fill_(SENTINEL)
    empty = _result(objs)
    assert empty["ncycles"].tolist() == [0, 0, 0, 0] and len(empty["steps"]) == 0 and tf.cycles() == []
    _feed_all(objs, other_masks, other_fields)
    _assert_equal(_result(objs), _reference("random", "wide", 3, 4, special=True))
    # cut() before frame 4: no track spans it
    trk.reset()
    tf._fstore.fill_(SENTINEL)
    _feed_all(objs, masks, fields, 0, 4)
    trk.cut()
    _feed_all(objs, masks, fields, 4)
    ref = _reference("random", "wide", 3, 4, cuts=(4,))
    assert ((full["tracks"][:, 3] < 4) & (full["tracks"][:, 4] >= 4)).any() and not ((ref["tracks"][:, 3] < 4) & (ref["tracks"][:, 4] >= 4)).any()
    got = _result(objs)
    _assert_equal(got, ref)
    assert not ((got["tracks"][:, 3] < 4) & (got["tracks"][:, 4] >= 4)).any()


def test_cycles_decodes_what_rows_reads():
    masks, fields = _frames("drawn", "split_merge", 3, 4)
    objs = _objects(2, *masks.shape[1:], 3, 4)
    _feed_all(objs, masks, fields)
    ref = _reference("drawn", "split_merge", 3, 4)
    H, W = masks.shape[1:]
    want = dnn.TrackFields.decode(ref["tracks"], ref["offsets"], ref["steps"], ref["step_fields"], ref["track_fields"], H, W, uf.scale_bits(3),
                                  center_channel=0)
    got = objs[3].cycles(center_channel=0)
    assert got == want and len(got) == 1 and got[0]["fields"][0]["min"] == -7.0 and got[0]["fields"][0]["min_frame"] == 0
    lat, lon = np.linspace(-90.0, 90.0, H), np.linspace(-180.0, 180.0, W)
    assert (got[0]["series"][0]["center_lat"], got[0]["series"][0]["center_lon"]) == (float(lat[7]), float(lon[16]))


def test_two_runs_give_equal_bytes():
    runs = [_run("random", "large", 16, 16, 4, conn=4) for _ in range(2)]
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in runs[0])


# ------------------------------------------------------------------------------------------------------------------ 7. errors, launch record
def test_argument_errors():
    H, W = uf.DRAWN_SHAPE
    cat, trk, fld, tf = _objects(2, H, W, 3, 4)
    other = dnn.EventCatalog(2, H, W, device=DEV)
    with pytest.raises(L.DeepcamHipError, match="same EventCatalog"):
        dnn.TrackFields(trk, dnn.EventFields(other, 3, uf.scale_bits(3)))
    with pytest.raises(L.DeepcamHipError, match="same EventCatalog"):
        dnn.TrackFields(dnn.EventTracker(other, event_cap=64), fld)
    with pytest.raises(L.DeepcamHipError, match="EventTracker"):
        dnn.TrackFields(cat, fld)
    for bad in (0, 1 << 31):
        with pytest.raises(L.DeepcamHipError, match="step_cap"):
            dnn.TrackFields(trk, fld, step_cap=bad)
    with pytest.raises(L.DeepcamHipError, match="same batch"):                     # nothing was called yet
        tf()
    mask = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    raw = torch.zeros((2, H, W, 4), dtype=torch.float32, device=DEV)
    cat(mask, n_valid=2)
    trk(mask)
    fld(raw, n_valid=1)                                                              # the fields of another n_valid than the tracker's
    with pytest.raises(L.DeepcamHipError, match="same batch"):
        tf()
    fld(raw)
    tf()
    for bad in ((), (0,), (3,)):
        with pytest.raises(L.DeepcamHipError, match="class"):
            tf.rows(classes=bad)
    assert tf.rows()["counts"].tolist() == [0, 0, 0, 0] and tf.cycles() == []
    assert dnn.TrackFields(trk, fld).step_cap == trk.event_cap


def test_every_launch_is_recorded_as_cc_track_fields():
    masks, fields = _frames("drawn", "hold", 3, 5)
    objs = _objects(3, *masks.shape[1:], 3, 5)
    _feed(objs, masks[:3], fields[:3])
    with served("TrackFields") as names:
        objs[3]()
    assert names == ["cc_track_fields"]
    with served("TrackFields.launch") as names:
        objs[3].launch()
    assert names == ["cc_tracks"] * 5 + ["cc_track_fields"] * 7


# ------------------------------------------------------------------------------------------------------------------ 8. driver
def test_predict_cli_with_track_fields(tmp_path):
    from mlperf_deepcam_amd import h5lite, predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "series")
    os.makedirs(root)
    rs = np.random.RandomState(21)
    n_files = 5
    base = (rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32)
    fields = [(base + 0.05 * i * (rs.rand(H, W, 16) * np.linspace(1, 300, 16))).astype(np.float32) for i in range(n_files)]   # a slowly changing scene
    names = [f"data-{i:02d}.h5" for i in range(n_files)]
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", lo)
        f.write("climate/maxval", hi)
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    min_frames, min_px = 2, 2

    def run(out, *extra):
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
               out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2",
               "--min_track_frames", str(min_frames), "--min_track_pixels", str(min_px), *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # batch 2 over five files: the last batch is ragged
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.load(open(os.path.join(out, "summary.json")))

    old = ("tracks", "track_events", "track_state")
    new = ("track_step_offsets", "track_steps", "track_step_fields", "track_fields", "track_cycle_counts")
    out, plain = str(tmp_path / "out"), str(tmp_path / "plain")
    summary = run(out, "--track_fields", "--track_center_channel", "0")
    before = run(plain, "--tracks", "--event_fields")                               # what the flag implies, without it
    masks = []
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f, h5lite.File(os.path.join(plain, name)) as g:
            masks.append(f.read("prediction"))
            for key in ("prediction", "events", "event_fields", "event_field_values", "event_field_bits"):
                a, b = f.read(key), g.read(key)
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)
    with h5lite.File(os.path.join(out, "tracks.h5")) as f, h5lite.File(os.path.join(plain, "tracks.h5")) as g:
        assert all(k not in g for k in new)
        for key in old:
            assert f.read(key).tobytes() == g.read(key).tobytes(), key
        got = {k: f.read(k) for k in old + new}
    assert "track_fields" not in before and before == {k: v for k, v in summary.items() if k != "track_fields"}
    # the checker on the stored predictions and the files' own fields
    bits = dnn.event_field_bits(lo, hi)
    ref = uf.reference(np.stack(masks), np.stack(fields), 8, True, _tables(H, W), 16, [int(b) for b in bits], cap=4096, event_cap=1 << 19,
                       min_pixels=min_px, min_frames=min_frames)
    assert all(got[k].dtype == np.int64 for k in new)
    for key, want in (("tracks", ref["tracks"]), ("track_state", ref["state"]), ("track_step_offsets", ref["offsets"]),
                      ("track_steps", ref["steps"]), ("track_step_fields", ref["step_fields"]), ("track_fields", ref["track_fields"]),
                      ("track_cycle_counts", ref["ncycles"])):
        assert got[key].shape == want.shape and np.array_equal(got[key], want), key
    assert np.array_equal(got["track_events"][:, :12], ref["store"])
    rows = {"counts": ref["ncycles"], "tracks": ref["tracks"], "offsets": ref["offsets"], "track_fields": ref["track_fields"]}
    assert summary["track_fields"] == predict.track_fields_summary(rows, H, W, center_channel=0)
    frames = ref["tracks"][:, 4] - ref["tracks"][:, 3] + 1
    assert 0 < ref["ncycles"][0] < len(frames) and ref["ncycles"][0] == (frames >= min_frames).sum(), "no track here lives two frames, or all do"
    assert summary["track_fields"]["tracks_selected"] == int(ref["ncycles"][0]) and summary["track_fields"]["center_channel"] == 0
    if (ref["tracks"][ref["offsets"] >= 0, 1] == 1).any():
        deepest = summary["track_fields"]["deepest_class_1"]
        cyc = dnn.TrackFields.decode(ref["tracks"], ref["offsets"], ref["steps"], ref["step_fields"], ref["track_fields"], H, W, bits)
        best = min((c for c in cyc if c["class"] == 1), key=lambda c: c["fields"][0]["min"])
        assert deepest["value"] == best["fields"][0]["min"] and deepest["frame"] == best["fields"][0]["min_frame"]
