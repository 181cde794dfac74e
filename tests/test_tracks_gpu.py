"""Event tracks on the GPU (dc_track_append / dc_track_link / dc_track_resolve of csrc/tracks.hip, nn.EventTracker, predict.py --tracks)
against the numpy checker of tests/util_tracks.py.  Everything is integer: every comparison is exact.

Shapes come from the labelling kernel's tile (dc_mask_components_tile), as in test_event_match_gpu.py: (2 TH + 3, 2 TW + 5) has ragged
tiles on both edges, (TH - 1, TW - 3) is one partial tile; neither width is a multiple of 4, so the link pass reads the masks bytewise.
(TH + 1, TW + 4) is the smallest frame of more than one tile whose width IS a multiple of 4: the pass reads the masks as words there.
A sequence has 8 frames.  It is fed as batches whose padding samples are all class 1 -- they would link everything if they were read --
and the buffers the calls fill are pre-filled with sentinels."""
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
import util_tracks as ut  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
T, CAP, EVENT_CAP = 8, 4096, 1 << 15
FIRST_SENTINEL, STORE_SENTINEL, PARENT_SENTINEL, TRACK_OF_SENTINEL = -77, -3, -4, -5


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


TH, TW = _tile()
SHAPES = {"tiles": (2 * TH + 3, 2 * TW + 5), "one": (TH - 1, TW - 3), "words": (TH + 1, TW + 4)}
assert SHAPES["tiles"][1] % 4 and SHAPES["one"][1] % 4 and SHAPES["words"][1] % 4 == 0
CONN_WRAP = [(4, False), (4, True), (8, False), (8, True)]
CW_IDS = ["c4-nowrap", "c4-wrap", "c8-nowrap", "c8-wrap"]
SEQUENCES = ["drift", "merge_split", "class_change", "gap", "one_pixel", "random"]


# ------------------------------------------------------------------------------------------------------------------ sequences
@functools.lru_cache(maxsize=None)
def _seq(name, H, W):
    """uint8 [T, H, W] (callers do not modify it)"""
    m = np.zeros((T, H, W), np.uint8)
    if name == "drift":                                  # a 6 x 8 blob that crosses the seam, 5 columns per frame; a resting one of class 2
        for t in range(T):
            for c in range(8):
                m[t, 4:10, (W - 18 + 5 * t + c) % W] = 1
            m[t, 14:19, 20:27] = 2
    elif name == "merge_split":                          # two blobs approach, are one for three frames, part again
        gap = [8, 4, 2, 0, 0, 0, 2, 6]
        for t in range(T):
            m[t, 6:12, 10:20] = 2
            m[t, 6:12, 20 + gap[t]:30 + gap[t]] = 2
            if gap[t] == 0:
                m[t, 8, 18:24] = 2
    elif name == "class_change":                         # the same pixels, another class in every other frame: no link at all
        for t in range(T):
            m[t, 3:9, 5:17] = 1 + t % 2
            m[t, 12:15, 30:40] = 2 - t % 2
    elif name == "gap":                                  # a resting blob and an empty frame in the middle: two tracks
        for t in range(T):
            if t != T // 2:
                m[t, 5:11, 7:19] = 1
    elif name == "one_pixel":                            # 4 x 4 squares stepping by 3 in both directions: consecutive ones share one pixel
        for t in range(T):
            m[t, 2 + 3 * t:6 + 3 * t, 2 + 3 * t:6 + 3 * t] = 1
        assert 6 + 3 * (T - 1) <= H
    elif name == "random":                               # independent frames: many events, late merges of tracks that were long apart
        rs = np.random.RandomState(zlib.crc32(f"tracks random {H} {W}".encode()))
        m[:] = (rs.rand(T, H, W) < 0.45) * rs.randint(1, 3, (T, H, W))
    elif name == "checker":                              # every pixel an event of its own that links to nothing (connectivity 4)
        m[:] = ut.checkerboard(T, H, W)
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, conn, wrap, cap=CAP, event_cap=EVENT_CAP, track_cap=None, min_pixels=0, cuts=()):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    H, W = SHAPES[shape]
    return ut.track(_seq(name, H, W), conn, wrap, *_tables(H, W), cap=cap, event_cap=event_cap, track_cap=track_cap, min_pixels=min_pixels,
                    cuts=cuts)


# ------------------------------------------------------------------------------------------------------------------ running a sequence
def _tracker(B, H, W, conn, wrap, cap=CAP, event_cap=EVENT_CAP, track_cap=None, min_pixels=0):
    """a catalogue and a tracker on it whose buffers hold sentinels where the calls are to write"""
    cat = dnn.EventCatalog(B, H, W, connectivity=conn, wrap=wrap, cap=cap, device=DEV)
    trk = dnn.EventTracker(cat, event_cap=event_cap, track_cap=track_cap, min_pixels=min_pixels)
    trk._first.fill_(FIRST_SENTINEL)
    trk._store.fill_(STORE_SENTINEL)
    trk._parent.fill_(PARENT_SENTINEL)
    trk._track_of.fill_(TRACK_OF_SENTINEL)
    trk._tracks.fill_(1)                                 # the resolve zeroes it
    return cat, trk


def _feed(cat, trk, frames, n_valid=None):
    """one call: the frames, then padding of class 1 up to the catalogue's batch"""
    nv = len(frames) if n_valid is None else n_valid
    m = np.ones((cat.B, cat.H, cat.W), np.uint8)
    m[:len(frames)] = frames
    mask = torch.from_numpy(m).to(DEV)
    trk._first.fill_(FIRST_SENTINEL)
    cat(mask, n_valid=nv)
    trk(mask, n_valid=nv)
    first = trk._first.cpu().numpy()
    assert (first[nv:] == FIRST_SENTINEL).all(), "a padding frame's entry of `first` was written"
    return first[:nv]


def _result(trk):
    state, store, track_of, tracks = trk.rows()
    n = int(state[0])
    rest = trk._store[n:].cpu().numpy(), trk._parent[n:].cpu().numpy(), trk._track_of[n:].cpu().numpy(), trk._tracks[len(tracks):].cpu().numpy()
    assert (rest[0] == STORE_SENTINEL).all() and (rest[1] == PARENT_SENTINEL).all() and (rest[2] == TRACK_OF_SENTINEL).all(), \
        "something was written behind the stored events"
    assert not rest[3].any(), "track rows behind the stored ones are not zero"
    parent = trk._parent[:n].cpu().numpy()
    assert np.array_equal(parent, np.where(track_of >= 0, tracks[np.maximum(track_of, 0), 0] if len(tracks) else 0, parent)), \
        "after a resolve every entry of the forest names its track's id"
    return {"state": state, "store": store, "track_of": track_of, "tracks": tracks, "ntracks": trk.track_counts()}


def _run(masks, batch, conn, wrap, **kw):
    """the whole sequence in calls of `batch` frames (the last one ragged), then the result"""
    _, H, W = masks.shape
    cat, trk = _tracker(batch, H, W, conn, wrap, **kw)
    first = [_feed(cat, trk, masks[k:k + batch]) for k in range(0, len(masks), batch)]
    got = _result(trk)
    got["first"] = np.concatenate(first)
    return got


def _assert_equal(got, ref):
    for key in ("state", "ntracks", "first", "store", "track_of", "tracks"):
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), \
            f"{key} differs: {got[key].tolist() if got[key].size < 40 else got[key].shape} vs {ref[key].tolist() if ref[key].size < 40 else ref[key].shape}"


# ------------------------------------------------------------------------------------------------------------------ 1. sequences
@pytest.mark.parametrize("conn,wrap", CONN_WRAP, ids=CW_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", SEQUENCES)
def test_sequences_against_the_checker(name, shape, conn, wrap):
    H, W = SHAPES[shape]
    ref = _reference(name, shape, conn, wrap)
    assert ref["state"][2] == 0 and ref["state"][3] == 0 and ref["ntracks"][0] == ref["ntracks"][3]       # nothing truncated here
    _assert_equal(_run(_seq(name, H, W), 3, conn, wrap), ref)
    tr = ref["tracks"]
    if name == "drift":                                  # the blob is one track of all frames wherever the seam joins or a fragment bridges
        assert (tr[tr[:, 1] == 2][:, 2:5] == [T, 0, T - 1]).all() and len(tr[tr[:, 1] == 2]) == 1
        assert len(tr[tr[:, 1] == 1]) == (1 if wrap else 2)      # without wrap nothing joins the two fragments of the frame on the edge
    elif name == "merge_split":
        assert len(tr) == 1 and tr[0, 2] == 2 * T - 3 and tr[0, 3:5].tolist() == [0, T - 1]
    elif name == "class_change":
        assert len(tr) == 2 * T and (tr[:, 2] == 1).all()
    elif name == "gap":
        assert tr[:, 2:5].tolist() == [[T // 2, 0, T // 2 - 1], [T - T // 2 - 1, T // 2 + 1, T - 1]]
    elif name == "one_pixel":
        assert len(tr) == 1 and tr[0, 2:6].tolist() == [T, 0, T - 1, 16 * T]
    else:
        frames = tr[:, 4] - tr[:, 3] + 1                  # many events, tracks that last, and tracks that hold merges or splits
        assert ref["state"][0] > 40 * T and (frames >= T // 2).any() and (tr[:, 2] > frames + 2).any()


@pytest.mark.parametrize("conn,wrap", CONN_WRAP, ids=CW_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_sequence_with_a_pixel_threshold(shape, conn, wrap):
    H, W = SHAPES[shape]
    ref = _reference("random", shape, conn, wrap, min_pixels=4)
    assert ref["ntracks"][0] > _reference("random", shape, conn, wrap)["ntracks"][0]                       # the threshold unlinks something
    _assert_equal(_run(_seq("random", H, W), 3, conn, wrap, min_pixels=4), ref)


# ------------------------------------------------------------------------------------------------------------------ 2. batching
@pytest.mark.parametrize("conn,wrap", [(4, True), (8, False)], ids=["c4-wrap", "c8-nowrap"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["random", "drift"])
def test_the_cut_into_batches_does_not_matter(name, shape, conn, wrap):
    H, W = SHAPES[shape]
    ref = _reference(name, shape, conn, wrap)
    assert T % 3 != 0                                    # batches of 3: the last call has n_valid < B
    for batch in (1, 3, T):
        _assert_equal(_run(_seq(name, H, W), batch, conn, wrap), ref)


# ------------------------------------------------------------------------------------------------------------------ 3. resolve in the middle
@pytest.mark.parametrize("shape", ["tiles", "words"])
def test_reading_tracks_in_the_middle_changes_nothing(shape):
    H, W = SHAPES[shape]
    masks, ref = _seq("random", H, W), _reference("random", shape, 8, True)
    cat, trk = _tracker(3, H, W, 8, True)
    _feed(cat, trk, masks[0:3])
    _feed(cat, trk, masks[3:6])
    mid = trk.tracks()
    half = ut.track(masks[:6], 8, True, *_tables(H, W), event_cap=EVENT_CAP)
    assert mid == dnn.EventTracker.decode(half["store"], half["track_of"], half["tracks"], H, W) and len(mid) == half["ntracks"][0]
    assert trk.state() == {"events": int(half["state"][0]), "frames": 6, "events_dropped": 0, "frames_truncated": 0}
    _feed(cat, trk, masks[6:8])                          # unions through the flattened entries
    got = _result(trk)
    again = _result(trk)                                 # and a second resolve of the same state
    for key in ("state", "ntracks", "store", "track_of", "tracks"):
        assert np.array_equal(got[key], ref[key]) and np.array_equal(again[key], ref[key]), key
    assert trk.tracks(min_frames=3) == [t for t in dnn.EventTracker.decode(got["store"], got["track_of"], got["tracks"], H, W) if t["frames"] >= 3]


# ------------------------------------------------------------------------------------------------------------------ 4. truncation
def test_more_events_than_the_store_holds():
    H, W = SHAPES["tiles"]
    total = int(_reference("random", "tiles", 8, True)["state"][0])
    event_cap = total // 2 + 1
    ref = _reference("random", "tiles", 8, True, event_cap=event_cap)
    assert ref["state"].tolist() == [event_cap, T, total - event_cap, 0] and len(ref["store"]) == event_cap
    for batch in (3, T):
        _assert_equal(_run(_seq("random", H, W), batch, 8, True, event_cap=event_cap), ref)


def test_more_components_than_the_catalogue_holds():
    H, W = SHAPES["tiles"]
    ref = _reference("random", "tiles", 4, True, cap=8)
    assert ref["state"].tolist() == [8 * T, T, 0, T]
    _assert_equal(_run(_seq("random", H, W), 3, 4, True, cap=8), ref)
    ref = _reference("drift", "tiles", 4, True, cap=1)   # one row per frame: the class-2 blob is no event
    assert ref["state"].tolist() == [T, T, 0, T] and ref["ntracks"].tolist() == [1, 1, 0, 1]
    _assert_equal(_run(_seq("drift", H, W), 3, 4, True, cap=1), ref)


def test_more_tracks_than_rows():
    H, W = SHAPES["tiles"]
    full = _reference("random", "tiles", 4, False)
    track_cap = int(full["ntracks"][0]) // 3
    ref = _reference("random", "tiles", 4, False, track_cap=track_cap)
    assert ref["ntracks"].tolist() == full["ntracks"][:3].tolist() + [track_cap] and (ref["track_of"] == -1).sum() > 0
    got = _run(_seq("random", H, W), 3, 4, False, track_cap=track_cap)
    _assert_equal(got, ref)
    assert np.array_equal(got["tracks"], full["tracks"][:track_cap]) and got["track_of"].max() == track_cap - 1


# ------------------------------------------------------------------------------------------------------------------ 4b. many chunks
def test_more_chunks_of_events_than_one_block_of_the_offsets_pass():
    """The resolve ranks roots in chunks of 256 events and ONE workgroup turns the chunks' counts into offsets, 256 chunks at a time with a
    carry from block to block.  71288 events that are 71288 tracks make 279 chunks: the carry is taken once, and every table is compared."""
    H, W = SHAPES["tiles"]
    kw = {"cap": 16384, "event_cap": 1 << 17}
    ref = _reference("checker", "tiles", 4, False, **kw)
    assert ref["state"].tolist() == [T * H * W, T, 0, 0] and ref["ntracks"].tolist() == [T * H * W, T * H * W // 2, T * H * W // 2, T * H * W]
    got = _run(_seq("checker", H, W), 3, 4, False, **kw)
    assert got["state"][0] > 65536 and got["ntracks"][3] > 65536, "fewer than 257 chunks: the offsets pass never carries"
    _assert_equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------ 5. cut and reset
def test_cut_and_reset():
    H, W = SHAPES["one"]
    masks = _seq("drift", H, W)
    cat, trk = _tracker(3, H, W, 8, True)
    _feed(cat, trk, masks[0:3])
    trk.cut()
    _feed(cat, trk, masks[3:6])                          # frame 3 is not linked to frame 2; frames 4 and 5 are linked as ever
    _feed(cat, trk, masks[6:8])
    got = _result(trk)
    ref = _reference("drift", "one", 8, True, cuts=(3,))
    for key in ("state", "ntracks", "store", "track_of", "tracks"):
        assert np.array_equal(got[key], ref[key]), key
    assert ref["tracks"][:, 3:5].tolist() == [[0, 2], [0, 2], [3, T - 1], [3, T - 1]] and got["store"][-1, 0] == T - 1   # numbering goes on
    trk.reset()
    assert trk.state() == {"events": 0, "frames": 0, "events_dropped": 0, "frames_truncated": 0} and trk.tracks() == []
    assert trk.track_counts().tolist() == [0, 0, 0, 0]
    other = _seq("merge_split", H, W)
    first = [_feed(cat, trk, other[k:k + 3]) for k in range(0, T, 3)]
    ref = _reference("merge_split", "one", 8, True)
    got = trk.rows()
    assert first[0][0] == 0 and np.array_equal(np.concatenate(first), ref["first"])
    assert all(np.array_equal(g, ref[k]) for g, k in zip(got, ("state", "store", "track_of", "tracks")))


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_runs_give_equal_bytes():
    H, W = SHAPES["tiles"]
    masks = _seq("random", H, W)
    runs = []
    for _ in range(2):
        cat, trk = _tracker(3, H, W, 4, True)
        with served("EventTracker") as names:
            for k in range(0, T, 3):
                _feed(cat, trk, masks[k:k + 3])
        assert names.count("cc_tracks") == 3 * 2 + 3 + 2          # append: two launches; link inside the batch; link to the carry
        with served("resolve") as names:
            trk.resolve()
        assert names == ["cc_tracks"] * 5
        runs.append([a.tobytes() for a in trk.rows()] + [trk.track_counts().tobytes()])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------------ 7. arguments
def test_argument_errors():
    H, W = SHAPES["one"]
    cat = dnn.EventCatalog(2, H, W, device=DEV)
    for kw in ({"event_cap": 0}, {"event_cap": (1 << 30) + 1}, {"event_cap": 16, "track_cap": 17}, {"event_cap": 16, "track_cap": 0},
               {"min_pixels": -1}):
        with pytest.raises(L.DeepcamHipError):
            dnn.EventTracker(cat, **kw)
    with pytest.raises(L.DeepcamHipError, match="2\\^63"):
        dnn.EventTracker(dnn.EventCatalog(1, 1024, 1024, device=DEV), event_cap=1 << 23)
    trk = dnn.EventTracker(cat, event_cap=64)
    mask = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.DeepcamHipError, match="catalogue"):        # no catalogue call yet
        trk(mask)
    cat(mask, n_valid=1)
    with pytest.raises(L.DeepcamHipError, match="n_valid"):          # another n_valid than the catalogue's
        trk(mask, n_valid=2)
    for bad in (mask.to(torch.int32), mask[:, :-1].contiguous(), mask[:1], mask.cpu(), mask.transpose(1, 2)):
        with pytest.raises(L.DeepcamHipError, match="mask"):
            trk(bad)
    assert trk.state()["frames"] == 0                                # none of these reached the device
    trk(mask)                                                        # n_valid defaults to the catalogue's
    assert trk.state() == {"events": 0, "frames": 1, "events_dropped": 0, "frames_truncated": 0} and trk.tracks() == []


# ------------------------------------------------------------------------------------------------------------------ 8. driver
def test_predict_cli_with_tracks(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
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
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    out, min_frames, min_px = str(tmp_path / "out"), 2, 2
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir", out,
           "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", "--events", "--tracks",
           "--min_track_frames", str(min_frames), "--min_track_pixels", str(min_px)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)          # batch 2 over five files: the last batch is ragged
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert [f["file"] for f in summary["files"]] == names
    masks, events = [], []
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f:
            masks.append(f.read("prediction"))
            events.append(f.read("events"))
    with h5lite.File(os.path.join(out, "tracks.h5")) as f:
        tracks, track_events, state = f.read("tracks"), f.read("track_events"), f.read("track_state")
    assert tracks.dtype == track_events.dtype == state.dtype == np.int64 and tracks.shape[1:] == (8,) and track_events.shape[1:] == (13,)
    # the tracker run directly on the same masks, all frames in one call
    cat = dnn.EventCatalog(n_files, H, W, device=DEV)
    trk = dnn.EventTracker(cat, min_pixels=min_px)
    m = torch.from_numpy(np.stack(masks)).to(DEV)
    cat(m)
    trk(m)
    w_state, w_store, w_of, w_tracks = trk.rows()
    assert np.array_equal(state, w_state) and np.array_equal(tracks, w_tracks)
    assert np.array_equal(track_events[:, :12], w_store) and np.array_equal(track_events[:, 12], w_of.astype(np.int64))
    assert len(tracks) > 0 and int(state[0]) == sum(len(e) for e in events) and state.tolist()[1:] == [n_files, 0, 0]
    for row in track_events:                             # (frame, rank) joins a row to the `events` of that frame's file
        assert np.array_equal(events[int(row[0])][int(row[1])], row[2:12])
    from mlperf_deepcam_amd import predict
    assert summary["tracks"] == predict.track_summary(w_state, w_tracks, min_frames)
    frames = w_tracks[:, 4] - w_tracks[:, 3] + 1
    for cls in (1, 2):
        assert summary["tracks"][f"class_{cls}"]["tracks"] == int((w_tracks[:, 1] == cls).sum())
        assert summary["tracks"][f"class_{cls}"]["tracks_min_frames"] == int(((w_tracks[:, 1] == cls) & (frames >= min_frames)).sum())
    assert frames.max() >= 2, "no event of these masks lives longer than a frame: the test links nothing"
