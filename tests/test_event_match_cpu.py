"""The event matching's host side (no GPU): the checker of tests/util_event_match.py against a hand-drawn example, the rates and the summary
of nn.EventMatcher, the host-only entry point and the argument checks of the C ABI, and the driver's flags and its renumbering of matches."""
import ctypes as C

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_match as um

# 6 x 8, 4-connectivity, no wrap.  Components in root order --
#   a: A0 class 1, 4 px (root 0)   A1 class 2, 4 px (root 5)   A2 class 1, 3 px (root 25)   A3 class 2, 2 px (root 38)
#   b: B0 class 1, 4 px (root 1)   B1 class 1, 2 px (root 5)   B2 class 1, 1 px (root 25)   B3 class 1, 1 px (root 27)   B4 class 2, 1 px (root 40)
MASK_A = [[1, 1, 0, 0, 0, 2, 2, 0],
          [1, 1, 0, 0, 0, 2, 2, 0],
          [0, 0, 0, 0, 0, 0, 0, 0],
          [0, 1, 1, 1, 0, 0, 0, 0],
          [0, 0, 0, 0, 0, 0, 2, 2],
          [0, 0, 0, 0, 0, 0, 0, 0]]
MASK_B = [[0, 1, 1, 0, 0, 1, 0, 0],
          [0, 1, 1, 0, 0, 1, 0, 0],
          [0, 0, 0, 0, 0, 0, 0, 0],
          [0, 1, 0, 1, 0, 0, 0, 0],
          [0, 0, 0, 0, 0, 0, 0, 0],
          [2, 0, 0, 0, 0, 0, 0, 0]]


def _match(**kw):
    a, b = np.asarray([MASK_A], np.uint8), np.asarray([MASK_B], np.uint8)
    wy, cx, sx = dnn.event_weight_tables(6, 8)
    args = {"cap_a": 8, "min_pixels": 0, "cover_q": 512}
    args.update(kw)
    return um.match(a, b, 1, 4, False, wy, cx, sx, **args)


def test_checker_by_hand():
    m = _match()
    assert [int(r[0]) for r in m["rows_a"][0]] == [0, 5, 25, 38] and [int(r[0]) for r in m["rows_b"][0]] == [1, 5, 25, 27, 40]
    # A0 and B0 share (0, 1) and (1, 1); A1 lies over B1 with ANOTHER class: listed, not covered; A2 holds both B2 and B3
    assert m["pairs"][0].tolist() == [[0, 0, 2], [1, 1, 2], [2, 2, 1], [2, 3, 1]]
    assert m["cover_a"][0].tolist() == [2, 0, 2, 0, 0, 0, 0, 0] and m["cover_b"][0].tolist() == [2, 0, 1, 1, 0, 0, 0, 0]
    # half of B0 is covered: exactly the threshold, a hit; B1 and B4 are missed; A1 and A3 answer to nothing of their class
    assert m["scores"][0].tolist() == [[3, 1, 0, 2], [0, 1, 2, 0]] and m["truncated"] == 0
    # full coverage asked for: only the single pixels B2 and B3 are still found, and no detection is fully covered
    assert _match(cover_q=1024)["scores"][0].tolist() == [[2, 2, 2, 0], [0, 1, 2, 0]]
    # any overlap of the own class suffices: as at one half here
    assert _match(cover_q=1)["scores"][0].tolist() == [[3, 1, 0, 2], [0, 1, 2, 0]]
    # events below two pixels are not scored (B2, B3, B4); they still cover A2
    assert _match(min_pixels=2)["scores"][0].tolist() == [[1, 1, 0, 2], [0, 0, 2, 0]]
    # tables of two rows: pairs and scores of the first two components of each side only, and the sample counts as truncated
    m = _match(cap_a=2)
    assert m["pairs"][0].tolist() == [[0, 0, 2], [1, 1, 2]] and m["cover_a"][0].tolist() == [2, 0] and m["cover_b"][0].tolist() == [2, 0]
    assert m["scores"][0].tolist() == [[1, 1, 0, 1], [0, 0, 1, 0]] and m["truncated"] == 1
    assert _match(pair_cap=3)["truncated"] == 1 and _match(pair_cap=4)["truncated"] == 0


def test_checker_counts_cover_from_components_beyond_the_other_cap():
    wy, cx, sx = dnn.event_weight_tables(6, 8)
    a, b = np.asarray([MASK_A], np.uint8), np.asarray([MASK_B], np.uint8)
    m = um.match(a, b, 1, 4, False, wy, cx, sx, cap_a=8, cap_b=2)
    assert m["pairs"][0].tolist() == [[0, 0, 2], [1, 1, 2]]                  # B2 and B3 have no row ...
    assert m["cover_a"][0].tolist()[:4] == [2, 0, 2, 0]                        # ... and still cover A2


def test_rates_by_hand():
    r = dnn.EventMatcher.rates
    assert r(3, 1, 0, 2) == {"pod": 0.75, "far": 0.0, "csi": 0.75}
    assert r(0, 1, 2, 0) == {"pod": 0.0, "far": 1.0, "csi": 0.0}
    assert r(6, 2, 2, 6) == {"pod": 0.75, "far": 0.25, "csi": 0.6}
    assert r(0, 0, 0, 0) == {"pod": None, "far": None, "csi": None}
    assert r(0, 0, 3, 0) == {"pod": None, "far": 1.0, "csi": 0.0}
    assert r(2, 2, 0, 0) == {"pod": 0.5, "far": None, "csi": 0.5}
    s = dnn.EventMatcher.summarize([3, 1, 0, 2, 0, 1, 2, 0, 1, 0])
    assert s["samples"] == 1 and s["truncated"] is False
    assert s["class_1"] == {"hits": 3, "misses": 1, "false_alarms": 0, "matched": 2, "pod": 0.75, "far": 0.0, "csi": 0.75, "truncated": False}
    assert s["class_2"] == {"hits": 0, "misses": 1, "false_alarms": 2, "matched": 0, "pod": 0.0, "far": 1.0, "csi": 0.0, "truncated": False}
    assert dnn.EventMatcher.summarize([0] * 9 + [2])["truncated"] is True


def test_matcher_refuses_a_threshold_outside_its_range():
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(L.DeepcamHipError, match="min_cover"):
            dnn.EventMatcher(1, 8, 8, min_cover=bad)


def test_sorting_and_joining_on_the_host():
    rows = np.array([[2, 3, 1], [0, 0, 2], [2, 2, 1], [1, 1, 2]], np.int64)
    assert dnn.EventMatcher.sort_pairs(rows).tolist() == [[0, 0, 2], [1, 1, 2], [2, 2, 1], [2, 3, 1]]
    assert dnn.EventMatcher.sort_pairs(rows[:0]).shape == (0, 3)
    m = _match()
    joined = dnn.EventMatcher.join(m["pairs"][0], m["rows_a"][0], m["rows_b"][0], 6, 8)
    assert [(j["a"]["root"], j["b"]["root"], j["class_a"], j["class_b"], j["pixels"]) for j in joined] == \
        [(0, 1, 1, 1, 2), (5, 5, 2, 1, 2), (25, 25, 1, 1, 1), (25, 27, 1, 1, 1)]
    assert [j["iou"] for j in joined] == [2 / 6, 2 / 4, 1 / 3, 1 / 3]
    assert joined[0]["a"] == dnn.EventCatalog.decode(m["rows_a"][0][:1], 6, 8)[0]
    assert [(j["a"]["root"], j["b"]["root"]) for j in dnn.EventMatcher.join(m["pairs"][0], m["rows_a"][0], m["rows_b"][0], 6, 8, min_pixels=2)] == \
        [(0, 1), (5, 5)]


def test_host_entry_point_and_argument_checks_without_a_device():
    lib = L.load()
    # the table (twice the rows, a power of two, key and count), a counter per sample, a slot index per row
    assert lib.dc_component_overlap_workspace(8, 8192) == 8 * 16384 * 16 + 256 + 8 * 8192 * 4
    assert lib.dc_component_overlap_workspace(1, 4) == 3 * 256 and lib.dc_component_overlap_workspace(1, 9) == 32 * 16 + 2 * 256
    assert lib.dc_component_overlap_workspace(0, 4) == 0 and lib.dc_component_overlap_workspace(1, 0) == 0
    assert lib.dc_component_overlap_workspace(1, (1 << 24) + 1) == 0
    fake = C.c_void_p(4096)                                                        # never dereferenced: the checks come before any launch
    ov = lambda **kw: lib.dc_component_overlap(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("nv", 2), ("H", 8), ("W", 8), ("ma", fake), ("la", fake), ("ra", fake), ("cap_a", 4), ("mb", fake), ("lb", fake), ("rb", fake),
        ("cap_b", 4), ("pair_cap", 8), ("pairs", fake), ("npairs", fake), ("ca", fake), ("cb", fake), ("ws", fake), ("st", None))])
    assert ov(nv=0) != 0 and "n_valid" in L.last_error()
    assert ov(nv=3) != 0
    assert ov(cap_b=0) != 0 and "cap" in L.last_error()
    assert ov(pair_cap=0) != 0 and "pair_cap" in L.last_error()
    assert ov(rb=None) != 0 and "null" in L.last_error()
    assert ov(ws=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
    sc = lambda **kw: lib.dc_event_scores(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("nv", 2), ("cap_a", 4), ("ta", fake), ("na", fake), ("ca", fake), ("cap_b", 4), ("tb", fake), ("nb", fake), ("cb", fake),
        ("npairs", fake), ("min_pixels", 0), ("cover_q", 512), ("scores", fake), ("acc", fake), ("st", None))])
    assert sc(cover_q=0) != 0 and "cover_q" in L.last_error()
    assert sc(cover_q=1025) != 0
    assert sc(nv=3) != 0 and "n_valid" in L.last_error()
    assert sc(acc=None) != 0 and "null" in L.last_error()


def test_driver_verify_implies_events():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False and a.min_event_cover == 0.5
    a = predict.build_parser().parse_args(base + ["--verify"])
    assert a.verify is True and a.events is True
    a = predict.build_parser().parse_args(base + ["--verify", "--min_event_cover", "0.25", "--events"])
    assert a.verify is True and a.events is True and a.min_event_cover == 0.25
    a = predict.build_parser().parse_args(base + ["--events"])
    assert a.verify is False and a.events is True


def test_driver_renumbers_matches_to_the_rows_it_stores():
    from mlperf_deepcam_amd import predict
    m = _match()
    ra, rb, p = predict.filter_matches(m["rows_a"][0], m["rows_b"][0], m["pairs"][0], 0)
    assert np.array_equal(ra, m["rows_a"][0]) and np.array_equal(rb, m["rows_b"][0]) and np.array_equal(p, m["pairs"][0])
    # at least three pixels: A0, A1, A2 and B0 stay; of the four pairs only (A0, B0)
    ra, rb, p = predict.filter_matches(m["rows_a"][0], m["rows_b"][0], m["pairs"][0], 3)
    assert ra[:, 0].tolist() == [0, 5, 25] and rb[:, 0].tolist() == [1] and p.tolist() == [[0, 0, 2]]
    # at least two: B2 and B3 go, and with them A2's pairs
    ra, rb, p = predict.filter_matches(m["rows_a"][0], m["rows_b"][0], m["pairs"][0], 2)
    assert ra[:, 0].tolist() == [0, 5, 25, 38] and rb[:, 0].tolist() == [1, 5] and p.tolist() == [[0, 0, 2], [1, 1, 2]]
    ra, rb, p = predict.filter_matches(m["rows_a"][0][:0], m["rows_b"][0], m["pairs"][0][:0], 0)
    assert ra.shape == (0, 10) and p.shape == (0, 3) and p.dtype == np.int64
