"""Track verification on the GPU (dc_track_match_append / dc_track_match_resolve of csrc/track_match.hip, nn.TrackMatcher, predict.py
--verify_tracks) against the numpy checker of tests/util_track_match.py.  Everything is integer: every comparison is exact.

Shapes come from the labelling kernel's tile (dc_mask_components_tile), as in test_tracks_gpu.py: (2 TH + 3, 2 TW + 5) has ragged tiles
on both edges, (TH - 1, TW - 3) is one partial tile.  A sequence has 8 frames and is fed in three cuts: all 8 in one call, 3 then 5, and
eight calls of one frame through a batch of 4.  Padding samples are all class 1 on BOTH sides -- they would overlap everywhere if they
were read -- and the buffers the calls fill are pre-filled with sentinels."""
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
import util_track_match as um  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
T, CAP, EVENT_CAP = um.T, 4096, 1 << 15
LINK_SENTINEL = -7
CUTS = {"whole": (8, (8,)), "3+5": (8, (3, 5)), "singles": (4, (1,) * 8)}          # batch, valid frames per call


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


TH, TW = _tile()
SHAPES = {"tiles": (2 * TH + 3, 2 * TW + 5), "one": (TH - 1, TW - 3)}
CONN_WRAP = [(4, True), (8, False)]
CW_IDS = ["c4-wrap", "c8-nowrap"]
SEQUENCES = ["identical", "lag", "merged", "missing_middle", "other_class", "drift", "random"]


@functools.lru_cache(maxsize=None)
def _seq(name, shape):
    a, b = um.sequence(name, *SHAPES[shape])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, conn, wrap, **kw):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    a, b = _seq(name, shape)
    return um.match(a, b, conn, wrap, *_tables(*SHAPES[shape]), cap=kw.pop("cap", CAP), event_cap=EVENT_CAP, **kw)


# ------------------------------------------------------------------------------------------------------------------ running a sequence
def _build(B, H, W, conn, wrap, cap=CAP, track_cap_a=None, track_cap_b=None, **kw):
    m = dnn.EventMatcher(B, H, W, connectivity=conn, wrap=wrap, cap=cap, device=DEV)
    ta = dnn.EventTracker(m.a, event_cap=EVENT_CAP, track_cap=track_cap_a)
    tb = dnn.EventTracker(m.b, event_cap=EVENT_CAP, track_cap=track_cap_b)
    tm = dnn.TrackMatcher(m, ta, tb, **kw)
    tm._links.fill_(LINK_SENTINEL)
    for t in (tm._tpairs, tm._cover_a, tm._cover_b, tm._scores, tm._counts):      # the resolve zeroes them
        t.fill_(1)
    return m, ta, tb, tm


def _feed(objs, frames_a, frames_b):
    """one call of all four objects: the frames, then padding of class 1 on both sides up to the batch"""
    m, ta, tb, tm = objs
    nv = len(frames_a)
    a, b = np.ones((m.B, m.H, m.W), np.uint8), np.ones((m.B, m.H, m.W), np.uint8)
    a[:nv], b[:nv] = frames_a, frames_b
    mask_a, mask_b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    m(mask_a, mask_b, n_valid=nv)
    ta(mask_a, n_valid=nv)
    tb(m.mask_b, n_valid=nv)
    tm()


def _result(objs):
    tm = objs[3]
    r = tm.rows()
    n, p = int(r["state"][0]), int(r["counts"][0])
    links = tm._links.cpu().numpy()
    assert (links[n:] == LINK_SENTINEL).all(), "something was written behind the stored links"
    assert not tm._tpairs[p:].any().item(), "pair rows behind the stored ones are not zero"
    assert not tm._cover_a[len(r["cover_a"]):].any().item() and not tm._cover_b[len(r["cover_b"]):].any().item(), \
        "cover rows behind the stored tracks are not zero"
    r["links"] = links[:n][np.lexsort((links[:n, 2], links[:n, 1], links[:n, 0]))]
    return r


def _run(name, shape, conn, wrap, cut, resolve_after=(), **kw):
    H, W = SHAPES[shape]
    a, b = _seq(name, shape)
    batch, calls = CUTS[cut]
    objs = _build(batch, H, W, conn, wrap, **kw)
    k = 0
    for i, n in enumerate(calls):
        _feed(objs, a[k:k + n], b[k:k + n])
        k += n
        if i in resolve_after:
            objs[3].rows()
    return _result(objs)


KEYS = ("state", "counts", "scores", "links", "pairs", "cover_a", "cover_b", "tracks_a", "tracks_b")


def _assert_equal(got, ref, keys=KEYS):
    want = dict(ref, tracks_a=ref["a"]["tracks"], tracks_b=ref["b"]["tracks"])
    for key in keys:
        g, w = got[key], want[key]
        assert g.shape == w.shape and np.array_equal(g, w), f"{key} differs: {g.tolist() if g.size < 60 else g.shape} vs " \
            f"{w.tolist() if w.size < 60 else w.shape}"


# ------------------------------------------------------------------------------------------------------------------ 1. sequences and cuts
@pytest.mark.parametrize("conn,wrap", CONN_WRAP, ids=CW_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", SEQUENCES)
def test_sequences_against_the_checker_in_three_cuts(name, shape, conn, wrap):
    ref = _reference(name, shape, conn, wrap)
    um.assert_inside_caps(ref)                            # nothing is cut: every table is compared row for row
    runs = [_run(name, shape, conn, wrap, cut) for cut in CUTS]
    for got in runs:
        _assert_equal(got, ref)
    for got in runs[1:]:                                  # and the cuts agree with each other
        for key in KEYS:
            assert np.array_equal(got[key], runs[0][key]), key
    pairs, sc = ref["pairs"], ref["scores"].tolist()
    if name == "identical":
        assert sc == [[1, 0, 0, 1], [1, 0, 0, 1]] and pairs[:, 3:5].tolist() == [[T, T], [T, T]]
    elif name == "lag":
        assert sc[0] == [1, 0, 0, 1] and pairs[:, 4:].tolist() == [[T - 2, 36 * (T - 2), 1, T - 2]]
    elif name == "merged":
        assert sc[1] == [1, 0, 0, 2] and pairs[:, :2].tolist() == [[0, 0], [1, 0]]
    elif name == "missing_middle":
        assert sc[0] == [1, 0, 0, 2] and ref["cover_b"].tolist() == [[T - 1, 72 * (T - 1)]]
    elif name == "other_class":
        assert sc == [[0, 1, 1, 0], [0, 1, 1, 0]] and len(pairs) == 0 and ref["state"][0] == 0
    elif name == "drift":                                 # the blobs overlap in every frame, wherever the seam cuts them
        cls1 = pairs[pairs[:, 2] == 1]
        assert cls1[:, 4].sum() >= T and sc[1] == [1, 0, 0, 1] and (wrap or len(cls1) > 1)
    else:                                                 # many pairs, several links of one pair in one frame
        assert len(pairs) > 100 and (pairs[:, 3] > pairs[:, 4]).any() and (pairs[:, 4] > 1).any()


def test_missing_middle_is_a_miss_at_full_cover():
    ref = _reference("missing_middle", "one", 8, False, cover_q=1024)
    got = _run("missing_middle", "one", 8, False, "3+5", min_cover=1.0)
    _assert_equal(got, ref)
    assert got["scores"].tolist() == [[0, 1, 0, 2], [0, 0, 0, 0]]
    ref = _reference("random", "one", 8, False, min_frames=3, cover_q=768)
    _assert_equal(_run("random", "one", 8, False, "3+5", min_frames=3, min_cover=0.75), ref)
    assert ref["scores"].sum() < _reference("random", "one", 8, False)["scores"].sum()          # fewer tracks are scored


# ------------------------------------------------------------------------------------------------------------------ 2. resolve in the middle
@pytest.mark.parametrize("shape", list(SHAPES))
def test_resolving_in_the_middle_changes_nothing(shape):
    ref = _reference("random", shape, 8, True)
    H, W = SHAPES[shape]
    a, b = _seq("random", shape)
    objs = _build(8, H, W, 8, True)
    _feed(objs, a[:3], b[:3])
    mid = _result(objs)
    half = um.match(a[:3], b[:3], 8, True, *_tables(H, W), event_cap=EVENT_CAP)
    _assert_equal(mid, half)
    assert objs[3].state() == {"links": int(half["state"][0]), "links_dropped": 0, "frames": 3, "frames_truncated": 0}
    _feed(objs, a[3:], b[3:])
    got = _result(objs)
    again = _result(objs)                                 # and a second resolve of the same state
    _assert_equal(got, ref)
    _assert_equal(again, ref)
    _assert_equal(_run("random", shape, 8, True, "singles", resolve_after=(0, 4)), ref)


# ------------------------------------------------------------------------------------------------------------------ 3. overflow
def test_more_links_than_the_store_holds():
    full = _reference("random", "tiles", 4, True)
    total = len(full["links"])
    link_cap = total // 2
    true_links = {tuple(r) for r in full["links"].tolist()}
    for cut in ("whole", "singles"):
        got = _run("random", "tiles", 4, True, cut, link_cap=link_cap)
        assert got["state"].tolist() == [link_cap, total - link_cap, T, 0]
        kept = [tuple(r) for r in got["links"].tolist()]
        assert len(set(kept)) == link_cap and set(kept) <= true_links, "a stored link is not a true overlap with its full count"
        # the resolve of exactly the links that were kept: nothing else about the run is unspecified
        want = um.resolve(got["links"], full["a"], full["b"])
        for key in ("counts", "scores", "pairs", "cover_a", "cover_b"):
            assert np.array_equal(got[key], want[key]), key


def test_more_track_pairs_than_rows():
    full = _reference("random", "tiles", 4, True)
    pair_cap = len(full["all_pairs"]) // 3
    ref = _reference("random", "tiles", 4, True, pair_cap=pair_cap)
    assert ref["counts"].tolist() == [pair_cap, 1, 0, 0] and ref["pairs"] is None
    true_rows = {tuple(r) for r in full["all_pairs"].tolist()}
    for cut in ("whole", "3+5"):
        got = _run("random", "tiles", 4, True, cut, pair_cap=pair_cap)
        _assert_equal(got, ref, keys=("state", "counts", "scores", "links", "cover_a", "cover_b"))       # exact under this overflow
        rows = [tuple(r) for r in got["pairs"].tolist()]
        assert len(rows) == pair_cap and len({r[:2] for r in rows}) == pair_cap and set(rows) <= true_rows, \
            "a stored pair row is not a distinct true pair with its full counts"
    # a table of the smallest size, every slot taken: keys are given up only after the whole table was probed
    got = _run("random", "tiles", 4, True, "whole", pair_cap=1)
    assert got["counts"].tolist() == [1, 1, 0, 0] and tuple(got["pairs"][0].tolist()) in true_rows
    assert np.array_equal(got["cover_a"], full["cover_a"]) and np.array_equal(got["scores"], full["scores"])


def test_more_tracks_than_rows():
    full = _reference("random", "tiles", 4, True)
    caps = {"track_cap_a": int(full["a"]["ntracks"][0]) // 3, "track_cap_b": int(full["b"]["ntracks"][0]) // 2}
    ref = _reference("random", "tiles", 4, True, **caps)
    assert ref["counts"][2] > 0 and ref["counts"][1] == 0 and 0 < len(ref["pairs"]) < len(full["pairs"])
    for cut in ("whole", "3+5"):                          # which tracks have rows is fixed (the first by id), so every table is exact
        got = _run("random", "tiles", 4, True, cut, **caps)
        _assert_equal(got, ref)
        assert len(got["cover_a"]) == caps["track_cap_a"] and len(got["cover_b"]) == caps["track_cap_b"]


def test_more_components_than_the_catalogues_hold():
    ref = _reference("random", "tiles", 4, True, cap=8)
    assert ref["state"][3] == T and ref["state"][0] > 0   # every frame is truncated, and still there are links
    _assert_equal(_run("random", "tiles", 4, True, "3+5", cap=8), ref)


# ------------------------------------------------------------------------------------------------------------------ 4. launches, reset, refusals
def test_served_reset_and_two_runs_give_equal_bytes():
    H, W = SHAPES["one"]
    a, b = _seq("drift", "one")
    ref = _reference("drift", "one", 4, True)
    objs = _build(8, H, W, 4, True)
    m, ta, tb, tm = objs
    _feed(objs, a[:3], b[:3])
    mask_a, mask_b = torch.from_numpy(a.copy()).to(DEV), torch.from_numpy(b.copy()).to(DEV)
    tm.reset()
    ta.reset()
    tb.reset()
    assert tm.state() == {"links": 0, "links_dropped": 0, "frames": 0, "frames_truncated": 0}
    m(mask_a, mask_b)
    ta(mask_a)
    tb(m.mask_b)
    with served("TrackMatcher") as names:
        tm()
    assert names == ["cc_track_match"]                    # one launch per batch
    with served("TrackMatcher.resolve") as names:
        tm.resolve()
    assert names == ["cc_tracks"] * 10 + ["cc_track_match"] * 6
    _assert_equal(_result(objs), ref)
    again = _run("drift", "one", 4, True, "whole")
    assert all(_result(objs)[k].tobytes() == again[k].tobytes() for k in KEYS)
    assert tm.matches() == dnn.TrackMatcher.decode(ref["pairs"], *um.decoded(ref, H, W))
    assert tm.result() == dnn.TrackMatcher.summarize(um.rows_of(ref), dnn.TrackMatcher.decode(ref["pairs"], *um.decoded(ref, H, W)), 1, 512)
    assert np.array_equal(tm.pairs(), ref["pairs"]) and np.array_equal(tm.scores(), ref["scores"])
    assert all(np.array_equal(g, w) for g, w in zip(tm.cover(), (ref["cover_a"], ref["cover_b"])))


def test_refusals_come_before_any_launch():
    H, W = SHAPES["one"]
    m = dnn.EventMatcher(2, H, W, device=DEV)
    other = dnn.EventMatcher(2, H, W, device=DEV)
    ta, tb = dnn.EventTracker(m.a, event_cap=64), dnn.EventTracker(m.b, event_cap=64)
    for args in ((m, tb, ta), (m, ta, dnn.EventTracker(other.b, event_cap=64)), (m, dnn.EventTracker(other.a, event_cap=64), tb), (m.a, ta, tb)):
        with pytest.raises(L.DeepcamHipError, match="matcher|EventMatcher"):       # catalogues that are not the matcher's
            dnn.TrackMatcher(*args)
    for kw in ({"link_cap": 0}, {"link_cap": (1 << 26) + 1}, {"pair_cap": 0}, {"pair_cap": (1 << 24) + 1}, {"min_frames": -1}, {"min_cover": 0.0}):
        with pytest.raises(L.DeepcamHipError):
            dnn.TrackMatcher(m, ta, tb, **kw)
    tm = dnn.TrackMatcher(m, ta, tb, link_cap=64, pair_cap=16)
    mask = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    with served("refused") as names:
        with pytest.raises(L.DeepcamHipError, match="same batch"):                 # nothing was called yet
            tm()
        m(mask, mask, n_valid=2)
        ta(mask, n_valid=2)
        with pytest.raises(L.DeepcamHipError, match="same batch"):                 # one tracker has not seen the batch
            tm()
        tb(m.mask_b, n_valid=2)
        m(mask, mask, n_valid=1)
        with pytest.raises(L.DeepcamHipError, match="n_valid"):                    # the matcher's last call had another n_valid
            tm()
        m(mask, mask, n_valid=2)
    assert "cc_track_match" not in names
    tm()
    with pytest.raises(L.DeepcamHipError, match="frames"):                         # the same batch filed twice
        tm()
    assert tm.state() == {"links": 0, "links_dropped": 0, "frames": 2, "frames_truncated": 0}
    r = tm.rows()
    assert r["counts"].tolist() == [0, 0, 0, 0] and r["scores"].tolist() == [[0] * 4] * 2 and len(r["pairs"]) == 0 and tm.matches() == []


# ------------------------------------------------------------------------------------------------------------------ 5. driver
def test_predict_cli_with_verify_tracks(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "series")
    os.makedirs(root)
    rs = np.random.RandomState(21)
    n_files = 3
    base = (rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32)
    fields = [(base + 0.05 * i * (rs.rand(H, W, 16) * np.linspace(1, 300, 16))).astype(np.float32) for i in range(n_files)]   # a slowly changing scene
    truth = []
    for i in range(n_files):                             # stripes of both classes, 12 columns wide, that move 4 columns per frame
        t = np.zeros((H, W), np.int64)
        t[8:H - 8] = 1 + ((np.arange(W) + 4 * i) // 12) % 2
        t[:, ::12] = 0
        truth.append(t)
    names = [f"data-{i:02d}.h5" for i in range(n_files)]
    for name, d, t in zip(names, fields, truth):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
            f.write("climate/labels_0", t)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    out, min_frames, min_px, cover = str(tmp_path / "out"), 2, 2, 0.75
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir", out,
           "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", "--verify_tracks",
           "--min_track_frames", str(min_frames), "--min_track_pixels", str(min_px), "--min_track_cover", str(cover)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)          # batch 2 over three files: the last batch is ragged
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    masks = []
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f:
            masks.append(f.read("prediction"))
    keys = ("tracks", "track_events", "track_state", "truth_tracks", "truth_track_events", "truth_track_state", "track_pairs", "track_cover",
            "truth_track_cover", "track_scores", "track_match_state")
    with h5lite.File(os.path.join(out, "tracks.h5")) as f:
        got = {k: f.read(k) for k in keys}
    assert all(v.dtype == np.int64 for v in got.values())
    ref = um.match(np.stack(masks).astype(np.uint8), np.stack(truth).astype(np.uint8), 8, True, *_tables(H, W), min_pixels=min_px,
                   min_frames=min_frames, cover_q=768)
    um.assert_inside_caps(ref)
    for key, side in (("", "a"), ("truth_", "b")):
        s = ref[side]
        assert np.array_equal(got[key + "tracks"], s["tracks"]) and np.array_equal(got[key + "track_state"], s["state"])
        assert np.array_equal(got[key + "track_events"], np.concatenate([s["store"], s["track_of"].astype(np.int64)[:, None]], axis=1))
    for key, want in (("track_pairs", "pairs"), ("track_cover", "cover_a"), ("truth_track_cover", "cover_b"), ("track_scores", "scores"),
                      ("track_match_state", "state")):
        assert got[key].shape == ref[want].shape and np.array_equal(got[key], ref[want]), key
    want = dnn.TrackMatcher.summarize(um.rows_of(ref), dnn.TrackMatcher.decode(ref["pairs"], *um.decoded(ref, H, W)), min_frames, 768)
    assert summary["track_verification"] == json.loads(json.dumps(want))
    assert ref["state"].tolist()[1:] == [0, n_files, 0] and len(ref["pairs"]) > 0, "the prediction overlaps no labelled storm: nothing was joined"
    assert "event_verification" in summary and "tracks" in summary                          # the flags it implies
