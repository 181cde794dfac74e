"""The event catalogue's host side (no GPU): the checker of tests/util_events.py against hand-written labels and tables, the two host-only
entry points and the argument checks of the C ABI, nn.EventCatalog's decoding and weight tables, and the driver's flags."""
import ctypes as C
import math

import numpy as np

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_events as ue


def _check(mask, conn, wrap, wy, cx, sx, labels, rows):
    got_l, got_r = ue.label_one(np.asarray(mask, np.uint8), conn, wrap, wy, cx, sx)
    assert got_l.tolist() == labels, (conn, wrap)
    assert got_r.tolist() == rows, (conn, wrap)


def test_checker_two_classes_by_hand():
    mask = [[1, 1, 0, 2],
            [0, 1, 0, 2],
            [2, 0, 0, 0]]
    wy, cx, sx = [10, 20, 30], [1, 2, 3, 4], [-1, -2, -3, -4]
    labels = [[1, 1, 0, 4],
              [0, 1, 0, 4],
              [9, 0, 0, 0]]
    rows = [[0, 1, 3, 40, 1, 5, -5, 0, 1, 0],
            [3, 2, 2, 30, 1, 8, -8, 0, 1, 0],
            [8, 2, 1, 30, 2, 1, -1, 2, 2, 0]]
    for conn, wrap in ((4, False), (4, True), (8, False)):      # class 1 in column 0 and class 2 in column 3 of row 0 never join
        _check(mask, conn, wrap, wy, cx, sx, labels, rows)
    # periodic columns and 8-connectivity: (2, 0) meets (1, 3) diagonally across the seam
    _check(mask, 8, True, wy, cx, sx, [[1, 1, 0, 4], [0, 1, 0, 4], [4, 0, 0, 0]],
           [[0, 1, 3, 40, 1, 5, -5, 0, 1, 0], [3, 2, 3, 60, 3, 9, -9, 0, 2, 1]])
    lab, table, ncomp, _ = ue.catalogue(np.asarray([mask, mask], np.uint8), 1, 4, True, wy, cx, sx, cap=2)
    assert lab.shape == (1, 3, 4) and ncomp.tolist() == [[3, 1, 2]]              # counts are not capped ...
    assert table.tolist() == [rows[:2]]                                          # ... the table holds the first cap rows by root


def test_checker_diagonal_and_background_values_by_hand():
    mask = [[1, 0, 3],
            [0, 1, 0],
            [0, 0, 1]]
    wy, cx, sx = [1, 2, 3], [5, 6, 7], [0, 1, 2]
    for wrap in (False, True):
        _check(mask, 4, wrap, wy, cx, sx, [[1, 0, 0], [0, 5, 0], [0, 0, 9]],
               [[0, 1, 1, 1, 0, 5, 0, 0, 0, 0], [4, 1, 1, 2, 1, 6, 1, 1, 1, 0], [8, 1, 1, 3, 2, 7, 2, 2, 2, 0]])
        _check(mask, 8, wrap, wy, cx, sx, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 3, 6, 3, 18, 3, 0, 2, 1]])


def test_checker_seam_by_hand():
    mask = [[2, 0, 0, 0],
            [0, 0, 0, 2],
            [2, 0, 0, 2]]
    wy, cx, sx = [1, 2, 3], [1, 2, 3, 4], [10, 20, 30, 40]
    apart = [[1, 0, 0, 0], [0, 0, 0, 8], [9, 0, 0, 8]]
    apart_rows = [[0, 2, 1, 1, 0, 1, 10, 0, 0, 0], [7, 2, 2, 5, 3, 8, 80, 1, 2, 0], [8, 2, 1, 3, 2, 1, 10, 2, 2, 0]]
    _check(mask, 4, False, wy, cx, sx, apart, apart_rows)
    _check(mask, 8, False, wy, cx, sx, apart, apart_rows)
    # columns periodic, 4-connectivity: (2, 0) meets (2, 3) across the seam
    _check(mask, 4, True, wy, cx, sx, [[1, 0, 0, 0], [0, 0, 0, 8], [8, 0, 0, 8]],
           [[0, 2, 1, 1, 0, 1, 10, 0, 0, 0], [7, 2, 3, 8, 5, 9, 90, 1, 2, 1]])
    # 8-connectivity: (0, 0) also meets (1, 3) diagonally across the seam
    _check(mask, 8, True, wy, cx, sx, [[1, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1]], [[0, 2, 4, 9, 5, 10, 100, 0, 2, 1]])


def test_host_entry_points_answer_without_a_device():
    lib = L.load()
    th, tw = C.c_int(), C.c_int()
    assert lib.dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    assert th.value >= 8 and tw.value >= 8
    assert lib.dc_mask_components_tile(None, C.byref(tw)) != 0
    small, large = lib.dc_mask_components_workspace(1, 64, 96), lib.dc_mask_components_workspace(8, 768, 1152)
    assert 0 < small < large and large % 256 == 0
    assert large >= 8 * 768 * 1152 * 4 and large < 2 * 8 * 768 * 1152 * 4      # one int32 per pixel and little else
    fake = C.c_void_p(4096)                                                    # never dereferenced: the checks come before any launch
    assert lib.dc_mask_components(2, 2, 8, 8, fake, 6, 1, fake, fake, None) != 0
    assert "connectivity must be 4 or 8" in L.last_error()
    assert lib.dc_mask_components(2, 0, 8, 8, fake, 8, 1, fake, fake, None) != 0
    assert "n_valid" in L.last_error()
    assert lib.dc_mask_components(2, 3, 8, 8, fake, 8, 1, fake, fake, None) != 0
    assert lib.dc_mask_components(1, 1, 46341, 46341, fake, 8, 1, fake, fake, None) != 0
    assert "2^31" in L.last_error()
    assert lib.dc_component_stats(2, 2, 8, 8, fake, fake, fake, fake, fake, 0, fake, fake, fake, None) != 0
    assert "cap" in L.last_error()
    assert lib.dc_component_stats(2, 0, 8, 8, fake, fake, fake, fake, fake, 4, fake, fake, fake, None) != 0
    assert lib.dc_component_stats(2, 2, 8, 8, fake, None, fake, fake, fake, 4, fake, fake, fake, None) != 0


def test_weight_tables_are_pinned():
    wy, cx, sx = dnn.event_weight_tables(5, 9)
    assert wy.dtype == cx.dtype == sx.dtype == np.int32
    assert wy.tolist() == [0, 741455, 1048576, 741455, 0]                       # 2^20 cos(45 deg) = 741455.2
    assert cx.tolist() == [-1048576, -741455, 0, 741455, 1048576, 741455, 0, -741455, -1048576]
    assert sx.tolist() == [0, -741455, -1048576, -741455, 0, 741455, 1048576, 741455, 0]
    wy, cx, sx = dnn.event_weight_tables(768, 1152)
    assert wy.shape == (768,) and cx.shape == sx.shape == (1152,)
    lat = math.radians(-90 + 180 * 100 / 767)
    assert int(wy[100]) == int(round(math.cos(lat) * 2 ** 20)) and int(wy[0]) == 0 and int(wy.max()) <= 2 ** 20
    assert dnn.EVENT_FIELDS == ("root", "class", "pixels", "area", "sum_row", "sum_cx", "sum_sx", "row_min", "row_max", "seam")


def test_event_decoding_of_a_hand_made_table():
    H, W = 5, 9
    rows = np.array([[10, 1, 4, 4 * 741455, 4, 0, -4 * 1048576, 1, 1, 0],        # four pixels of row 1, centred on lon -90
                     [20, 2, 2, 2 * 1048576, 4, -2 * 1048576, 0, 2, 2, 1],       # two pixels of the equator, on the seam
                     [40, 2, 1, 0, 4, 1048576, 0, 4, 4, 0]], np.int64)           # one pixel at the pole
    ev = dnn.EventCatalog.decode(rows, H, W)
    assert [e["class"] for e in ev] == [1, 2, 2] and [e["pixels"] for e in ev] == [4, 2, 1] and [e["root"] for e in ev] == [10, 20, 40]
    whole = 9 * (2 * 741455 + 1048576)
    assert ev[0]["area_fraction"] == 4 * 741455 / whole and ev[1]["area_fraction"] == 2 * 1048576 / whole and ev[2]["area_fraction"] == 0.0
    assert ev[0]["lat"] == -45.0 and ev[1]["lat"] == 0.0 and ev[2]["lat"] == 90.0
    assert ev[0]["lon"] == -90.0 and abs(ev[1]["lon"]) == 180.0 and ev[2]["lon"] == 0.0
    assert [(e["row_min"], e["row_max"], e["crosses_seam"]) for e in ev] == [(1, 1, False), (2, 2, True), (4, 4, False)]
    assert [e["root"] for e in dnn.EventCatalog.decode(rows, H, W, min_pixels=2)] == [10, 20]
    assert dnn.EventCatalog.decode(rows[:0], H, W) == []


def test_driver_accepts_the_event_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.events is False and a.min_event_pixels == 0 and a.event_connectivity == 8
    a = predict.build_parser().parse_args(base + ["--events", "--min_event_pixels", "25", "--event_connectivity", "4"])
    assert a.events is True and a.min_event_pixels == 25 and a.event_connectivity == 4
