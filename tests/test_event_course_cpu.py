"""The main course without a GPU: the checker of util_event_course.py on cases with answers worked by hand, the double sweep against an
all-pairs brute force (equal on every tree of the table, a lower bound on the rings), and the host code of nn.EventAxis / nn.EventFilter."""
import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_course as uc
import util_events as ue

H, W, CAP = 24, 70, 64
LINK = dnn.axis_link_table(H, W)


def solve(name, wrap=1, conn=8, cap=CAP):
    """-> (rows of the drawn case's events, course map, status, labels, roots)"""
    m = uc.drawn(name, H, W)
    labels, _, _, every = ue.catalogue(m[None], 1, conn, wrap, *dnn.event_weight_tables(H, W), cap)
    return uc.course(m, labels[0], every[0][:, 0], cap, wrap, LINK, 8192) + (labels[0], every[0][:, 0])


def test_cases_worked_by_hand():
    rows, cmap, status = solve("rows")[:3]
    assert rows[0].tolist() == [12, 2 * W + 5, 11 * LINK[2, 0], 2 * W + 16, 2 * W + 5, 12, 11 * LINK[2, 0]]       # start = end_b: the west tip
    assert rows[1, 6] == 11 * LINK[11, 0] > 3 * rows[0, 6] and status == [[12, 0], [12, 0]] and (cmap != 0).sum() == 24
    rows = solve("seam")[0]                                             # s = (3, 0): both tips are 4 links away, the smaller index is end_a
    assert rows[0].tolist() == [9, 3 * W, 4 * LINK[3, 0], 3 * W + 4, 3 * W + 66, 9, 8 * LINK[3, 0]]
    assert [r[6] for r in solve("seam", wrap=0)[0][:2]] == [4 * LINK[3, 0], 3 * LINK[3, 0]]      # cut at the seam: two events
    rows, cmap = solve("plus")[:2]                                      # the W and E tips tie for the farthest from the N tip
    assert rows[0, 3:].tolist() == [12 * W + 35, 12 * W + 45, 11, 10 * LINK[12, 0]] and (cmap[12, 35:46] == 1).all() and cmap.sum() == 11
    rows, cmap = solve("detour")[:2]                                    # 30 links along row 1 are shorter than 8 down the meridian
    assert 30 * LINK[1, 0] < 8 * LINK[1, 1] and rows[0, 3] == 9 * W + 45 and rows[0, 2] == rows[0, 6] == 15 * LINK[1, 0] + 8 * LINK[1, 1]
    assert rows[0, 4] == 1 * W + 30 and rows[0, 5] == 8 + 16 and cmap[1, 30] == 1 and cmap[1, 60] == 0      # (1, 30) and (1, 60) tie from (9, 45)
    rows, cmap = solve("dots")[:2]
    assert all(r[0] == 1 and r[1] == r[3] == r[4] and r[2] == r[6] == 0 and r[5] == 1 for r in rows[:4].tolist()) and (cmap != 0).sum() == 4
    rows = solve("ypsilon")[0]                                          # the two longest arms: 9 links west, 6 links south-east
    assert rows[0, 6] == 9 * LINK[12, 0] + sum(LINK[12:18, 2]) and rows[0, 5] == 16 and len(solve("touch", conn=4)[4]) == 4


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("wrap", [0, 1])
def test_exact_on_trees_and_a_lower_bound_on_rings(wrap, conn):
    for name in uc.CASES:
        rows, _, _, labels, roots = solve(name, wrap, conn)
        m = uc.drawn(name, H, W)
        for cls in (1, 2):
            g = uc.graph(m, labels, roots, CAP, wrap, LINK, cls)
            for k in {k for k, _ in g.values()}:
                full = uc.diameter(g, [p for p, (e, _) in g.items() if e == k])
                assert rows[k, 6] == full if name in uc.TREES else rows[k, 6] <= full, (name, k)
    ring = solve("ring")[0][0]                                           # 26 pixels in a cycle: half way round, both ways on the course or one
    assert ring[0] == 26 and 0 < ring[6] <= 8 * LINK[9, 0] + 5 * LINK[4, 1]


def test_decode_and_argument_checks():
    rows = solve("rows")[0]
    ev = np.zeros((2, 10), np.int64)
    ev[:, 1] = [1, 2]
    axis = np.zeros((2, 7), np.int64)
    axis[:, 6] = [2 * rows[0, 6], 0]
    rows[1, 6] = -1
    d = dnn.EventAxis.decode(axis, ev, H, W, course_rows=rows[:2])
    lat, lon = np.linspace(-90, 90, H), np.linspace(-180, 180, W)
    assert d[0]["course_km"] == rows[0, 6] / 1000.0 and d[0]["course_share"] == 0.5 and d[0]["course_pixels"] == 12
    assert d[0]["course_ends"] == ((lat[2], lon[16]), (lat[2], lon[5]))
    assert d[0]["sinuosity"] == pytest.approx(d[0]["course_km"] / dnn.great_circle_km(lat[2], lon[16], lat[2], lon[5])) and d[0]["sinuosity"] > 1
    assert d[1]["course_km"] is None and d[1]["course_share"] is None and d[1]["sinuosity"] is None
    assert "course_km" not in dnn.EventAxis.decode(axis, ev, H, W)[0] and dnn.EVENT_COURSE_FIELDS[6] == "course_m"
    cat = type("Cat", (), {})()
    plain = object.__new__(dnn.EventAxis)
    plain.catalog, plain.course = cat, False
    for member in ("course_table", "course_buffer", "course_rows", "course_status"):
        with pytest.raises(L.DeepcamHipError, match="only with course=True"):
            getattr(plain, member)() if member in ("course_rows", "course_status") else getattr(plain, member)
    with pytest.raises(L.DeepcamHipError, match="needs an axis built with course=True"):
        dnn.EventFilter(cat, min_axis_km=(0, 2000), axis=plain, axis_measure="course")
    with pytest.raises(L.DeepcamHipError, match="axis_measure must be"):
        dnn.EventFilter(cat, min_axis_km=(0, 2000), axis=plain, axis_measure="longest")
    assert L.load().dc_course_node_cap() >= 8192
