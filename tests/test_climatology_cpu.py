"""The climatology's host side (no GPU): the checker of tests/util_climatology.py against an example worked out by hand,
nn.Climatology.decode on hand-made accumulators, nn.climatology_group, the three entry points in the header, the binding table and the
thunks, the host-only entry point and the argument checks of the C ABI, and the driver's flags and summary."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_climatology as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_climatology_block", "dc_climatology_accumulate", "dc_climatology_maps")
NAN, INF = float("nan"), float("inf")


def _hand_made():
    """2 x 3 pixels, two groups, one selected channel (file channel 1 of 2) at bits = 1, so q = rint(2 v): four frames, the second one
    skipped (all class 1 with NaN fields: it must leave no trace)."""
    masks = np.array([[[1, 0, 2], [0, 3, 1]],
                      [[1, 1, 1], [1, 1, 1]],
                      [[2, 2, 0], [0, 0, 0]],
                      [[1, 1, 0], [0, 0, 255]]], np.uint8)
    ch1 = np.array([[[1.25, NAN, 3.0], [0.5, -2.0, 1e13]],         # 2.5 -> 2 (ties to even); NaN; 6; 1; -4; 2e13 > 2^40: saturated
                    [[NAN] * 3] * 2,
                    [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]],
                    [[0.75, 1.0, -INF], [0.25, 0.0, 7.0]]], np.float32)   # 1.5 -> 2; 2; -Inf; 0.5 -> 0; 0; 14
    fields = np.stack([np.full_like(ch1, 1e30), ch1], axis=-1)       # channel 0 is not selected: its values must not matter
    group = [0, -1, 1, 0]
    want = uc.empty(2, 2, 3, 1)
    want["frames"][:] = [2, 1]
    want["count"][0, 0] = [[2, 1, 0], [0, 0, 1]]
    want["count"][0, 1] = [[0, 0, 1], [0, 0, 0]]
    want["count"][1, 1] = [[1, 1, 0], [0, 0, 0]]
    want["sum"][0, 0, :, :, 0] = [[4, 2, 6], [1, -4, 14]]
    want["n"][0, 0, :, :, 0] = [[2, 1, 1], [2, 2, 1]]
    want["sum"][0, 1, :, :, 0] = [[4, 2, 0], [0, 0, 0]]              # the saturated value of pixel (1, 2) is class 1: counted, not summed
    want["n"][0, 1, :, :, 0] = [[2, 1, 0], [0, 0, 0]]
    want["sum"][0, 2, :, :, 0] = [[0, 0, 6], [0, 0, 0]]
    want["n"][0, 2, :, :, 0] = [[0, 0, 1], [0, 0, 0]]
    want["sum"][1, 0, :, :, 0] = [[2, 4, 6], [8, 10, 12]]
    want["n"][1, 0, :, :, 0] = 1
    want["sum"][1, 2, :, :, 0] = [[2, 4, 0], [0, 0, 0]]
    want["n"][1, 2, :, :, 0] = [[1, 1, 0], [0, 0, 0]]
    return masks, fields, group, want


def _assert_state(got, want):
    for k in uc.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def test_the_checker_against_a_hand_computed_example():
    masks, fields, group, want = _hand_made()
    _assert_state(uc.reference([(masks, fields, group)], 2, 2, 3, [1], [1]), want)
    # cut in two, and in another order: the same integers
    cut = uc.reference([(masks[2:], fields[2:], group[2:]), (masks[:2], fields[:2], group[:2])], 2, 2, 3, [1], [1])
    _assert_state(cut, want)
    # wider mask types give the same classes; no channel selected: counts and frames only
    wide = uc.reference([(masks.astype(np.int64), None, group)], 2, 2, 3, [], [])
    assert np.array_equal(wide["count"], want["count"]) and np.array_equal(wide["frames"], want["frames"]) and wide["sum"].size == 0


def test_the_checkers_maps_against_hand_computed_values():
    masks, fields, group, state = _hand_made()
    state["frames"][1] = 0                                            # a group without a frame: frequency 0, not NaN
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    assert uc.same_bits(uc.product(state, [1], ("frequency", 1)), f32([[[1, 0.5, 0], [0, 0, 0.5]], [[0] * 3] * 2]))
    mean = uc.product(state, [1], ("mean", 0, 1))                     # class-1 mean of group 0: 4 / 2 / 2, 2 / 2 / 1, none elsewhere
    assert uc.same_bits(mean[0], f32([[1.0, 1.0, NAN], [NAN, NAN, NAN]])) and np.isnan(mean[1]).all()
    assert mean.view(np.uint32)[0, 0, 2] == 0x7FC00000
    share = uc.product(state, [1], ("share", 0, 2))
    assert uc.same_bits(share[0], f32([[0, 0, 1], [0, -0.0, 0]]))              # 0 / -4: the quotient's sign is kept
    assert uc.same_bits(share[1], f32([[1, 1, 0], [0, 0, 0]]))
    state["sum"][0, 0, 0, 0, 0] = 0                                   # sum_all == 0: NaN
    assert np.isnan(uc.product(state, [1], ("share", 0, 1))[0, 0, 0])
    third = uc.empty(1, 1, 1, 1)                                      # the two roundings: 1 / 3 in fp64, then fp32
    third["frames"][0], third["count"][0, 0, 0, 0] = 3, 1
    assert uc.product(third, [1], ("frequency", 1))[0, 0, 0] == np.float32(np.float64(1) / np.float64(3))
    out, contour = uc.maps(state, [1], [("frequency", 1), ("frequency", 2)], 0.5, 0.5)
    assert out.shape == (2, 2, 3, 2) and contour.dtype == np.uint8
    assert contour.tolist() == [[[1, 1, 2], [0, 0, 1]], [[0, 0, 0], [0, 0, 0]]]      # equality counts; class 1 wins over class 2
    assert uc.maps(state, [1], [("frequency", 1)], 0.0, 0.5)[1].min() == 1           # 0 >= 0 everywhere, the empty group included


def test_decode_of_hand_made_accumulators():
    H, W = 3, 4                                                       # latitudes -90, 0, 90: wy = (0, 2^20, 0)
    assert dnn.event_weight_tables(H, W)[0].tolist() == [0, 1 << 20, 0]
    frames = np.array([4, 0], np.int64)
    count = np.zeros((2, 2, H, W), np.int32)
    count[0, 0, 1] = [4, 2, 0, 0]                                     # on the equator
    count[0, 0, 0] = [4, 4, 4, 4]                                     # at the pole: no area
    count[0, 1, 1, 3] = 1
    total = np.zeros((2, 3, H, W, 2), np.int64)
    n = np.zeros((2, 3, H, W, 2), np.int32)
    total[0, 0, 1, 0], n[0, 0, 1, 0] = [48, -6], [4, 3]
    total[0, 1, 1, 0], n[0, 1, 1, 0] = [12, -6], [1, 3]
    m = dnn.Climatology.decode(frames, count, total, n, [3, 1], H, W)
    assert m["frequency"].shape == (2, 2, H, W) and m["mean"].shape == (2, 3, H, W, 2) and m["share"].shape == (2, 2, H, W, 2)
    assert m["zonal_frequency"].shape == (2, 2, H) and m["area_frequency"].shape == (2, 2)
    assert all(v.dtype == np.float64 for v in m.values())
    assert m["frequency"][0, 0, 1].tolist() == [1.0, 0.5, 0.0, 0.0] and np.isnan(m["frequency"][1]).all()
    assert m["mean"][0, 0, 1, 0].tolist() == [48 / 8 / 4, -6 / 2 / 3] and m["mean"][0, 1, 1, 0].tolist() == [12 / 8, -1.0]
    assert np.isnan(m["mean"][0, 2]).all() and np.isnan(m["mean"][0, 0, 0]).all() and np.isnan(m["mean"][1]).all()
    assert m["share"][0, 0, 1, 0].tolist() == [0.25, 1.0] and m["share"][0, 1, 1, 0].tolist() == [0.0, 0.0]
    assert np.isnan(m["share"][0, :, 1, 1]).all() and np.isnan(m["share"][1]).all()
    assert m["zonal_frequency"][0, 0].tolist() == [1.0, 6 / 16, 0.0] and m["zonal_frequency"][0, 1].tolist() == [0.0, 1 / 16, 0.0]
    assert m["area_frequency"][0].tolist() == [6 / 16, 1 / 16] and np.isnan(m["area_frequency"][1]).all()
    none = dnn.Climatology.decode(frames, count, np.zeros((2, 3, H, W, 0)), np.zeros((2, 3, H, W, 0)), [], H, W)
    assert none["mean"].shape == (2, 3, H, W, 0) and none["area_frequency"][0].tolist() == [6 / 16, 1 / 16]


def test_climatology_group():
    g = dnn.climatology_group
    assert g("data-2006-07-14-00-1.h5", "all") == 0 and g("no date here", "all") == 0
    assert [g(f"data-1999-{m:02d}-03-12-2.h5", "month") for m in range(1, 13)] == list(range(12))
    assert [g(f"data-1999-{m:02d}-03-12-2.h5", "season") for m in range(1, 13)] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0]
    assert g("/somewhere/2001-01-01/data-2003-12-31-00-1.h5", "season") == 0 and g("/a/2001-01-01/data-2003-12-31.h5", "month") == 11
    assert g("run-1850-02-03_to_1850-09-09.h5", "month") == 1                   # the first date counts
    for by in ("month", "season"):
        for bad in ("data-00.h5", "data-20060714.h5", "data-2006-13-01.h5"):
            with pytest.raises(L.DeepcamHipError, match="YYYY-MM-DD"):
                g(bad, by)
    with pytest.raises(L.DeepcamHipError, match="by must be"):
        g("data-2006-07-14.h5", "year")
    assert {k: len(v) for k, v in dnn.CLIMATOLOGY_GROUPS.items()} == {"all": 1, "month": 12, "season": 4}


def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_climatology", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert f"int {name}(" in header and name in L.EXPORTS and hasattr(L.load(), name)
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_climatology_accumulate"][1]) == 17 and len(L._SIGS["dc_climatology_maps"][1]) == 16
    for word in ("climatology_accumulate_vec", "climatology_accumulate_scalar", "climatology_maps"):
        assert word in header.split("int dc_launch_log_begin")[0]


def test_block_and_argument_checks_without_a_device():
    lib = L.load()
    pixels = C.c_int(0)
    assert lib.dc_climatology_block(C.byref(pixels)) == 0 and pixels.value > 0
    assert lib.dc_climatology_block(None) != 0 and "null" in L.last_error()
    fake = C.c_void_p(4096)                                                        # never dereferenced: the checks come before any launch
    acc = lambda **kw: lib.dc_climatology_accumulate(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("H", 5), ("W", 8), ("G", 2), ("mask", fake), ("mask_bytes", 1), ("fields", fake), ("C", 3), ("ldc", 5), ("chan", fake),
        ("bits", fake), ("group", fake), ("frames", fake), ("count", fake), ("sum", fake), ("n", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert acc(mask_bytes=3) != 0 and "mask_bytes" in L.last_error()
        assert acc(mask_bytes=2) != 0 and acc(mask_bytes=0) != 0
        assert acc(C=33) != 0 and "C must" in L.last_error()
        assert acc(C=-1) != 0 and "C must" in L.last_error()
        assert acc(G=0) != 0 and "G must" in L.last_error()
        assert acc(B=0) != 0 and acc(H=0) != 0 and acc(W=0) != 0 and "positive" in L.last_error()
        assert acc(H=1 << 16, W=1 << 15) != 0 and "2^31" in L.last_error()
        assert acc(ldc=0) != 0 and "ldc" in L.last_error()
        assert acc(chan=None, ldc=2) != 0 and "ldc" in L.last_error()            # the identity over 3 channels needs 3
        assert acc(C=0) != 0 and "C = 0" in L.last_error()                        # fields without a channel
        for name in ("mask", "group", "frames", "count", "fields", "bits", "sum", "n"):
            assert acc(**{name: None}) != 0 and "null" in L.last_error(), name
        assert acc(mask_bytes=8, mask=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert acc(sum=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        maps = lambda **kw: lib.dc_climatology_maps(*[kw.get(k, v) for k, v in (  # noqa: E731
            ("G", 2), ("H", 5), ("W", 8), ("C", 3), ("frames", fake), ("count", fake), ("sum", fake), ("n", fake), ("bits", fake), ("K", 2),
            ("products", fake), ("t1", 0.1), ("t2", 0.1), ("out", fake), ("contour", fake), ("st", None))])
        assert maps(G=0) != 0 and "G must" in L.last_error()
        assert maps(C=33) != 0 and "C must" in L.last_error()
        assert maps(K=0) != 0 and maps(K=257) != 0 and "K must" in L.last_error()
        assert maps(H=0) != 0 and maps(H=1 << 16, W=1 << 15) != 0 and "2^31" in L.last_error()
        for name in ("frames", "count", "sum", "n", "bits", "products", "out", "contour"):
            assert maps(**{name: None}) != 0 and "null" in L.last_error(), name
        assert maps(out=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                                                        # nothing was launched


def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.climatology is False and a.climatology_by == "all" and a.climatology_channels == [] and a.climatology_contour == 0.1
    a = predict.build_parser().parse_args(base + ["--climatology", "--climatology_by", "month", "--climatology_channels", "0", "3"])
    assert a.climatology is True and a.climatology_by == "month" and a.climatology_channels == [0, 3]
    assert a.events is False and a.verify is False and a.plots is False       # the flag implies nothing else
    a = predict.build_parser().parse_args(base + ["--climatology", "--climatology_by", "season", "--climatology_contour", "0.25"])
    assert a.climatology_by == "season" and a.climatology_channels == [] and a.climatology_contour == 0.25
    # like --min_track_frames without --tracks: the family's options parse without its switch and are ignored
    a = predict.build_parser().parse_args(base + ["--climatology_by", "month"])
    assert a.climatology is False and a.climatology_by == "month"
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(base + ["--climatology", "--climatology_by", "year"])
    assert "maps over time" in predict.build_parser().format_help()


def test_driver_summary_entry():
    from mlperf_deepcam_amd import predict
    maps = {"area_frequency": np.array([[0.25, 0.5], [NAN, NAN], [0.0, 1.0], [0.125, 0.0]])}
    truth = {"area_frequency": np.array([[0.5, 0.5], [NAN, NAN], [0.0, 0.0], [1.0, 0.0]])}
    s = predict.climatology_summary("season", np.array([3, 0, 1, 2]), maps, truth, channels=[0, 3])
    assert s == {"by": "season", "groups": ["DJF", "MAM", "JJA", "SON"], "frames": [3, 0, 1, 2], "channels": [0, 3],
                 "area_frequency": {"class_1": [0.25, None, 0.0, 0.125], "class_2": [0.5, None, 1.0, 0.0]},
                 "truth_area_frequency": {"class_1": [0.5, None, 0.0, 1.0], "class_2": [0.5, None, 0.0, 0.0]}}
    assert "truth_area_frequency" not in predict.climatology_summary("season", np.array([3, 0, 1, 2]), maps)
    assert predict.climatology_plot_name("01", 2) == "climatology-01-class2.png"
