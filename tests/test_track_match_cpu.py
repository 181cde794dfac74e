"""The track verification's host side (no GPU): the checker of tests/util_track_match.py against hand-counted sequences of 8 frames,
nn.TrackMatcher.decode / summarize on those rows, the host-only entry point and the argument checks of the C ABI, the constructor's
refusals that need no device, and the driver's flag."""
import ctypes as C
import functools

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_track_match as um

H, W = 24, 48


@functools.lru_cache(maxsize=None)
def _ref(name, cover_q=512, min_frames=1):
    a, b = um.sequence(name, H, W)
    ref = um.match(a, b, 8, True, *dnn.event_weight_tables(H, W), cover_q=cover_q, min_frames=min_frames)
    um.assert_inside_caps(ref)
    return ref


def _lists(ref):
    return {k: ref[k].tolist() for k in ("state", "pairs", "cover_a", "cover_b", "scores", "counts")}


# ------------------------------------------------------------------------------------------------------------------ the checker by hand
def test_identical_sides():
    r = _lists(_ref("identical"))
    # track rows are ordered by their first event: the class-1 blob (rows 4 .. 9) comes before the class-2 blob (rows 14 .. 18)
    assert r["state"] == [16, 0, 8, 0] and r["counts"] == [2, 0, 0, 0]
    assert r["pairs"] == [[0, 0, 1, 8, 8, 8 * 6 * 8, 0, 7], [1, 1, 2, 8, 8, 8 * 5 * 7, 0, 7]]
    assert r["cover_a"] == r["cover_b"] == [[8, 384], [8, 280]]
    assert r["scores"] == [[1, 0, 0, 1], [1, 0, 0, 1]]
    ref = _ref("identical")
    for side in ("a", "b"):                              # every track is a hit over its whole life: common_frames == frames
        tr = ref[side]["tracks"]
        assert (tr[:, 4] - tr[:, 3] + 1 == ref["pairs"][:, 4]).all()


def test_the_prediction_lags_by_one_frame():
    ref = _ref("lag")
    r = _lists(ref)
    # frames 1 .. 6 hold both blobs, two columns apart: 6 rows x 6 columns shared
    assert r["state"] == [6, 0, 8, 0] and r["pairs"] == [[0, 0, 1, 6, 6, 6 * 36, 1, 6]]
    assert r["cover_a"] == r["cover_b"] == [[6, 216]] and r["scores"] == [[1, 0, 0, 1], [0, 0, 0, 0]]
    assert ref["a"]["tracks"][0, 3:5].tolist() == [1, 7] and ref["b"]["tracks"][0, 3:5].tolist() == [0, 6]
    m = dnn.TrackMatcher.decode(ref["pairs"], *um.decoded(ref, H, W))
    assert len(m) == 1 and (m[0]["genesis_error"], m[0]["lysis_error"], m[0]["duration_error"]) == (1, 1, 0)
    assert (m[0]["frames_a"], m[0]["frames_b"], m[0]["common_frames"], m[0]["id_a"], m[0]["id_b"], m[0]["class"]) == (7, 7, 6, 0, 0, 1)
    # the paths are two columns apart on the same rows: the separation is the great circle between the two centroids of any common frame
    pa, pb = um.decoded(ref, H, W)[0][0]["path"], um.decoded(ref, H, W)[1][0]["path"]
    want = np.mean([dnn.great_circle_km(pa[f - 1]["lat"], pa[f - 1]["lon"], pb[f]["lat"], pb[f]["lon"]) for f in range(1, 7)])
    assert m[0]["mean_separation_km"] == pytest.approx(want, rel=1e-12) and 0 < want < 2 * 40030.0 / (W - 1) * 1.01


def test_one_labelled_storm_predicted_as_two():
    r = _lists(_ref("merged"))
    assert r["state"] == [16, 0, 8, 0] and r["counts"] == [2, 0, 0, 0]
    assert r["pairs"] == [[0, 0, 2, 8, 8, 8 * 48, 0, 7], [1, 0, 2, 8, 8, 8 * 48, 0, 7]]         # two pairs on one b track
    assert r["cover_a"] == [[8, 384], [8, 384]] and r["cover_b"] == [[8, 768]]
    assert r["scores"] == [[0, 0, 0, 0], [1, 0, 0, 2]]                                           # one hit, no false alarm


def test_the_prediction_misses_the_middle_frame():
    r = _lists(_ref("missing_middle"))
    assert r["state"] == [7, 0, 8, 0]
    assert r["pairs"] == [[0, 0, 1, 4, 4, 4 * 72, 0, 3], [1, 0, 1, 3, 3, 3 * 72, 5, 7]]          # two a tracks, one b track
    assert r["cover_a"] == [[4, 288], [3, 216]] and r["cover_b"] == [[7, 504]]                    # 7 of 8 frames matched
    assert r["scores"] == [[1, 0, 0, 2], [0, 0, 0, 0]]                                           # a hit at min_cover 0.5 ...
    r = _lists(_ref("missing_middle", cover_q=1024))
    assert r["cover_b"] == [[7, 504]] and r["scores"] == [[0, 1, 0, 2], [0, 0, 0, 0]]            # ... a miss at 1.0
    r = _lists(_ref("missing_middle", min_frames=4))                                             # the 3-frame fragment is not scored
    assert r["scores"] == [[1, 0, 0, 1], [0, 0, 0, 0]]


def test_the_same_pixels_with_the_other_class():
    r = _lists(_ref("other_class"))
    assert r["state"] == [0, 0, 8, 0] and r["pairs"] == [] and r["counts"] == [0, 0, 0, 0]
    assert r["cover_a"] == r["cover_b"] == [[0, 0], [0, 0]]
    assert r["scores"] == [[0, 1, 1, 0], [0, 1, 1, 0]]                                           # all misses and false alarms


def test_checker_caps():
    a, b = um.sequence("merged", H, W)
    tables = dnn.event_weight_tables(H, W)
    ref = um.match(a, b, 8, True, *tables, link_cap=5, pair_cap=1)
    assert ref["state"].tolist() == [5, 11, 8, 0] and ref["counts"].tolist() == [1, 1, 0, 0] and ref["pairs"] is None
    assert len(ref["all_pairs"]) == 2 and ref["cover_b"].tolist() == [[8, 768]]
    ref = um.match(a, b, 8, True, *tables, track_cap_a=1)                                        # the second a track has no row
    assert ref["counts"].tolist() == [1, 0, 8, 0] and ref["pairs"].tolist() == [[0, 0, 2, 8, 8, 384, 0, 7]]
    assert ref["cover_a"].tolist() == [[8, 384]] and ref["cover_b"].tolist() == [[8, 384]] and ref["scores"].tolist() == [[0, 0, 0, 0], [1, 0, 0, 1]]
    with pytest.raises(AssertionError):
        um.assert_inside_caps(ref)
    ref = um.match(a, b, 8, True, *tables, cap=1)                                                # one row per frame: the right half is no event
    assert ref["state"].tolist() == [8, 0, 8, 8] and ref["pairs"].tolist() == [[0, 0, 2, 8, 8, 384, 0, 7]]


# ------------------------------------------------------------------------------------------------------------------ decode and summarize
def _track(tid, cls, f0, f1, lat=0.0, lon=0.0):
    return {"id": tid, "class": cls, "first_frame": f0, "last_frame": f1, "frames": f1 - f0 + 1,
            "path": [{"frame": f, "events": 1, "pixels": 4, "lat": lat, "lon": lon + f} for f in range(f0, f1 + 1)]}


def test_decode_by_hand():
    ta = [_track(0, 1, 0, 3), _track(7, 1, 5, 7, lat=10.0), _track(9, 2, 2, 2)]
    tb = [_track(0, 1, 0, 7, lon=2.0), _track(4, 2, 2, 4)]
    pairs = np.array([[0, 0, 1, 4, 4, 90, 0, 3], [1, 0, 1, 5, 3, 60, 5, 7], [2, 1, 2, 1, 1, 5, 2, 2]], np.int64)
    m = dnn.TrackMatcher.decode(pairs, ta, tb)
    assert [(p["row_a"], p["row_b"], p["id_a"], p["id_b"], p["class"]) for p in m] == [(0, 0, 0, 0, 1), (1, 0, 7, 0, 1), (2, 1, 9, 4, 2)]
    assert [(p["genesis_error"], p["lysis_error"], p["duration_error"]) for p in m] == [(0, -4, -4), (5, 0, -5), (0, -2, -2)]
    assert [(p["overlaps"], p["common_frames"], p["shared_pixels"], p["first_common_frame"], p["last_common_frame"]) for p in m] == \
        [(4, 4, 90, 0, 3), (5, 3, 60, 5, 7), (1, 1, 5, 2, 2)]
    assert m[0]["mean_separation_km"] == pytest.approx(dnn.great_circle_km(0.0, 0.0, 0.0, 2.0), rel=1e-12)       # two degrees along the equator
    assert m[0]["mean_separation_km"] == pytest.approx(2.0 * np.pi * dnn.EARTH_RADIUS_KM / 180.0, rel=1e-9)
    assert m[1]["mean_separation_km"] == pytest.approx(dnn.great_circle_km(10.0, 5.0, 0.0, 7.0), rel=1e-9)
    assert [p["row_a"] for p in dnn.TrackMatcher.decode(pairs, ta, tb, min_frames=3)] == [0, 1]                  # the one-frame track drops out
    assert dnn.TrackMatcher.decode(pairs[:0], ta, tb) == []
    assert dnn.great_circle_km(0.0, 179.0, 0.0, -179.0) == pytest.approx(dnn.great_circle_km(0.0, 0.0, 0.0, 2.0), rel=1e-9)   # across the seam
    assert dnn.great_circle_km(90.0, 0.0, -90.0, 77.0) == pytest.approx(np.pi * dnn.EARTH_RADIUS_KM, rel=1e-12)


def test_summarize_by_hand_with_ties_and_none():
    # b row 0 (class 1, 8 frames) has three partners: rows a 0 and 1 tie in common frames, row 1 wins by shared pixels; rows a 1 and 2 tie
    # in both, the smaller row wins.  b row 1 (class 1) is matched but its pair was not stored; b row 2 (class 1) is not matched.
    ta = [_track(0, 1, 0, 3), _track(5, 1, 2, 6), _track(6, 1, 2, 6), _track(30, 1, 0, 0)]
    tb = [_track(0, 1, 1, 8, lon=1.0), _track(2, 1, 0, 1), _track(3, 1, 0, 5)]
    pairs = np.array([[0, 0, 1, 3, 3, 50, 1, 3], [1, 0, 1, 3, 3, 70, 2, 4], [2, 0, 1, 3, 3, 70, 2, 4]], np.int64)
    tracks_b = np.array([[0, 1, 8, 1, 8, 0, 0, 0], [2, 1, 2, 0, 1, 0, 0, 0], [3, 1, 6, 0, 5, 0, 0, 0]], np.int64)
    rows = {"state": [9, 0, 9, 0], "counts": [3, 1, 0, 0], "scores": [[2, 1, 1, 3], [0, 0, 0, 0]], "pairs": pairs,
            "cover_b": np.array([[6, 190], [1, 4], [2, 9]], np.int64), "tracks_b": tracks_b}
    s = dnn.TrackMatcher.summarize(rows, dnn.TrackMatcher.decode(pairs, ta, tb), 1, 512)
    assert (s["frames"], s["links"], s["links_dropped"], s["frames_truncated"], s["pairs"], s["pairs_overflowed"], s["links_without_track"]) == \
        (9, 9, 0, 0, 3, True, 0)
    assert s["truncated"] is True and s["min_frames"] == 1 and s["min_cover"] == 0.5
    c1 = s["class_1"]
    assert (c1["hits"], c1["misses"], c1["false_alarms"], c1["matched"]) == (2, 1, 1, 3)
    assert c1["pod"] == 2 / 3 and c1["far"] == 1 / 4 and c1["csi"] == 2 / 4
    assert c1["partnered"] == 1 and c1["mean_partners"] == 3.0                                    # b row 1 is matched but has no stored pair
    assert c1["mean_abs_genesis_error"] == 1.0 and c1["mean_abs_lysis_error"] == 2.0              # the best partner is row a 1: frames 2 .. 6
    assert c1["mean_separation_km"] == pytest.approx(dnn.great_circle_km(0.0, 0.0, 0.0, 1.0), rel=1e-9)
    c2 = s["class_2"]
    assert all(c2[k] is None for k in ("pod", "far", "csi", "mean_abs_genesis_error", "mean_abs_lysis_error", "mean_separation_km",
                                       "mean_partners")) and c2["partnered"] == 0
    # a higher min_frames: b row 1 (2 frames) is no longer scored -- the scores come from the device, the partners follow the same rule
    s = dnn.TrackMatcher.summarize(dict(rows, counts=[3, 0, 0, 0]), dnn.TrackMatcher.decode(pairs, ta, tb), 9, 512)
    assert s["class_1"]["partnered"] == 0 and s["class_1"]["mean_partners"] is None and s["truncated"] is False


def test_summarize_of_the_checked_sequences():
    for name, want in (("identical", (0.0, 0.0, 1.0)), ("lag", (1.0, 1.0, 1.0)), ("merged", (0.0, 0.0, 2.0)), ("missing_middle", (0.0, 4.0, 2.0))):
        ref = _ref(name)
        s = dnn.TrackMatcher.summarize(um.rows_of(ref), dnn.TrackMatcher.decode(ref["pairs"], *um.decoded(ref, H, W)), 1, 512)
        cls = "class_2" if name == "merged" else "class_1"
        assert (s[cls]["mean_abs_genesis_error"], s[cls]["mean_abs_lysis_error"], s[cls]["mean_partners"]) == want, name
        assert s[cls]["pod"] == 1.0 and s[cls]["far"] == 0.0 and s["truncated"] is False
    ref = _ref("other_class")
    s = dnn.TrackMatcher.summarize(um.rows_of(ref), [], 1, 512)
    assert s["class_1"]["pod"] == 0.0 and s["class_1"]["far"] == 1.0 and s["class_1"]["csi"] == 0.0 and s["class_1"]["mean_partners"] is None


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
def test_host_entry_point_and_argument_checks_without_a_device():
    lib = L.load()
    ws = lib.dc_track_match_workspace
    al = lambda v: (v + 255) // 256 * 256  # noqa: E731
    # pair table 2 * 2^16 slots of 48 bytes, frame table 2 * 2^20 words, the counter, a byte per step, tickets, offsets and chunks per side
    assert ws(1 << 15, 1 << 15, 1 << 15, 1 << 15, 1 << 20, 1 << 16) == \
        (1 << 17) * 48 + (1 << 21) * 8 + 256 + 2 * (1 << 15) + (1 << 16) * 4 + 2 * ((1 << 15) * 8 + 128 * 16 + 128 * 8)
    assert ws(1, 1, 1, 1, 1, 1) == al(16 * 48) + al(16 * 8) + 256 + 2 * 256 + 256 + 2 * 3 * 256
    for bad in ((0, 1, 1, 1, 1, 1), (1, (1 << 30) + 1, 1, 1, 1, 1), (4, 4, 5, 1, 1, 1), (4, 4, 1, 0, 1, 1), (4, 4, 1, 1, 0, 1),
                (4, 4, 1, 1, (1 << 26) + 1, 1), (4, 4, 1, 1, 1, 0), (4, 4, 1, 1, 1, (1 << 24) + 1)):
        assert ws(*bad) == 0, bad
    assert ws(4, 4, 4, 4, 1 << 26, 1 << 24) > 0
    fake = C.c_void_p(4096)                                                        # never dereferenced: the checks come before any launch
    ap = lambda **kw: lib.dc_track_match_append(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("nv", 2), ("cap_a", 4), ("cap_b", 4), ("pair_cap", 8), ("pairs", fake), ("npairs", fake), ("ncomp_a", fake), ("first_a", fake),
        ("event_cap_a", 16), ("store_a", fake), ("ncomp_b", fake), ("first_b", fake), ("event_cap_b", 16), ("store_b", fake), ("link_cap", 8),
        ("links", fake), ("state", fake), ("st", None))])
    assert ap(nv=0) != 0 and "n_valid" in L.last_error()
    assert ap(nv=3) != 0
    assert ap(cap_b=0) != 0 and "cap" in L.last_error()
    assert ap(event_cap_a=0) != 0 and "event_cap" in L.last_error()
    assert ap(link_cap=0) != 0 and "link_cap" in L.last_error()
    assert ap(link_cap=(1 << 26) + 1) != 0 and ap(pair_cap=0) != 0 and ap(pair_cap=(1 << 24) + 1) != 0
    assert ap(first_b=None) != 0 and "null" in L.last_error()
    rs = lambda **kw: lib.dc_track_match_resolve(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("event_cap_a", 16), ("event_cap_b", 16), ("track_cap_a", 16), ("track_cap_b", 16), ("link_cap", 8), ("pair_cap", 8), ("min_frames", 1),
        ("cover_q", 512), ("state", fake), ("links", fake), ("store_a", fake), ("track_of_a", fake), ("tracks_a", fake), ("ntracks_a", fake),
        ("track_of_b", fake), ("tracks_b", fake), ("ntracks_b", fake), ("tpairs", fake), ("cover_a", fake), ("cover_b", fake), ("scores", fake),
        ("counts", fake), ("ws", fake), ("st", None))])
    assert rs(track_cap_b=17) != 0 and "track_cap" in L.last_error()
    assert rs(link_cap=(1 << 26) + 1) != 0 and "link_cap" in L.last_error()
    assert rs(pair_cap=0) != 0 and "pair_cap" in L.last_error()
    assert rs(min_frames=-1) != 0 and "min_frames" in L.last_error()
    assert rs(cover_q=0) != 0 and "cover_q" in L.last_error() and rs(cover_q=1025) != 0
    assert rs(counts=None) != 0 and "null" in L.last_error()
    assert rs(ws=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()


def test_the_new_calls_are_bound():
    for name in ("dc_track_match_workspace", "dc_track_match_append", "dc_track_match_resolve"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert len(L._SIGS["dc_track_match_append"][1]) == 19 and len(L._SIGS["dc_track_match_resolve"][1]) == 24
    assert len(dnn.TRACK_PAIR_FIELDS) == 8 and len(dnn.TRACK_COVER_FIELDS) == 2 and dnn.TrackMatcher.SCORE_FIELDS == dnn.EventMatcher.SCORE_FIELDS


def test_constructor_refusals_that_need_no_device():
    for kw, word in (({"link_cap": 0}, "link_cap"), ({"link_cap": (1 << 26) + 1}, "link_cap"), ({"pair_cap": 0}, "pair_cap"),
                     ({"pair_cap": (1 << 24) + 1}, "pair_cap"), ({"min_frames": -1}, "min_frames"), ({"min_cover": 0.0}, "min_cover"),
                     ({"min_cover": 1.5}, "min_cover"), ({}, "EventMatcher")):
        with pytest.raises(L.DeepcamHipError, match=word):
            dnn.TrackMatcher(None, None, None, **kw)                               # the ranges are checked before anything is built


def test_driver_verify_tracks_implies_verify_and_tracks():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert not hasattr(a, "verify_tracks") and not hasattr(a, "min_track_cover") and a.verify is False and a.tracks is False
    a = predict.build_parser().parse_args(base + ["--verify_tracks"])
    assert a.verify_tracks is True and a.verify is True and a.tracks is True and a.events is True
    a = predict.build_parser().parse_args(base + ["--verify_tracks", "--min_track_cover", "0.75", "--min_track_frames", "3"])
    assert a.min_track_cover == 0.75 and a.min_track_frames == 3
    a = predict.build_parser().parse_args(base + ["--verify", "--tracks"])
    assert not hasattr(a, "verify_tracks") and a.verify is True and a.tracks is True
    assert "--verify_tracks" in predict.build_parser().format_help()
