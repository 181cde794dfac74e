"""Spur pruning without a GPU: the checker of util_skeleton_prune.py against the cases worked by hand and the properties that follow from
the rule in include/deepcam_hip.h, and the host code of nn.EventFilter's axis criterion."""
import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_axis as ua
import util_events as ue
import util_skeleton_prune as up

SHAPES = [(8, 64), (9, 65), (40, 72), (64, 200)]
THINNED = ("blobs", "band", "ring")


def gpu_inputs(shape, wrap):
    """every input of the GPU test at one shape: {name: uint8 [H, W]}"""
    out = {name: up.drawn(name, *shape) for name in up.DRAWN}
    for name in THINNED:
        out["thin-" + name] = ua.thin(ua.make_mask(name, *shape), 2, wrap, max(shape))[0][1]
    return out


def test_drawn_cases_at_spur_3():
    m = up.drawn("spurs", 8, 64)
    want = m.copy()
    for r, c in up.SPUR_2:
        want[r, c] = 0
    got, removed = up.prune(m[None], 1, 0, 3)
    assert np.array_equal(got[0], want) and removed.tolist() == [[2, 0]]          # the 2-pixel spur goes, the 7-pixel spur stays in full
    ring = up.drawn("ring", 8, 64)
    assert np.array_equal(up.prune(ring[None], 1, 1, 3)[0][0], ring)
    two = up.drawn("two", 8, 64) == 1
    assert int(up.shrink_plane(two, 0, 3).sum()) == 1 and np.array_equal(up.prune_plane(two, 0, 3), two)   # keeps one pixel; regrown
    e, alone, _ = up.endpoints(up.drawn("stairs", 8, 64) == 1, 0)
    assert e.sum() == 2 and e[0, 5] and e[6, 12] and not alone.any()              # the tips of a staircase are endpoints


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 8, 40])
@pytest.mark.parametrize("step", [(0, 1), (1, 0), (1, 1), (1, -1)], ids=["ew", "ns", "se", "sw"])
def test_a_straight_line_comes_back_exactly(n, step):
    m = np.zeros((48, 64), np.uint8)
    up._line(m, 4, 60 if step[1] else 63, step[0], step[1], n)                    # the horizontal and diagonal ones cross the seam
    assert np.array_equal(up.prune(m[None], 1, 1, 3)[0][0], m)
    # one shrink round takes exactly one pixel off each end, whichever way it points; the last pixel stays
    s = m == 1
    e, _, back = up.endpoints(s, 1)
    a = e & back
    s2 = s & ~a & ~((e & ~a) & np.logical_or.reduce(up.ring(s & ~a, 1)))
    assert int(s2.sum()) == max(n - 2, 1)


@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_component_is_lost(shape, wrap):
    """on every input the GPU test uses: each 8-connected component of the input keeps a pixel through the shrink rounds, before any
    regrowth, and the pruned map lies between the shrunk one and the input"""
    tables = dnn.event_weight_tables(*shape)
    for name, m in gpu_inputs(shape, wrap).items():
        labels = ue.catalogue(m[None], 1, 8, wrap, *tables, 4096)[0][0]
        for spur in (1, 3, 16):
            x1 = sum(k * up.shrink_plane(m == k, wrap, spur).astype(np.uint8) for k in (1, 2))
            got = up.prune(m[None], 1, wrap, spur)[0][0]
            assert ((x1 == 0) | (x1 == got)).all() and ((got == 0) | (got == m)).all(), name
            assert set(np.unique(labels[m != 0])) == set(np.unique(labels[x1 != 0])), f"{name}, spur {spur}: a component vanished"


def test_filter_refuses_min_axis_km_without_an_axis_and_converts_thresholds():
    class Cat:                                         # the constructor checks its arguments before it touches the catalogue
        pass
    with pytest.raises(L.DeepcamHipError, match="min_axis_km needs axis"):
        dnn.EventFilter(Cat(), min_axis_km=(0, 2000))
    other = type("Axis", (), {"catalog": Cat()})()
    with pytest.raises(L.DeepcamHipError, match="min_axis_km needs axis"):
        dnn.EventFilter(Cat(), min_axis_km=(0, 2000), axis=other)
    for km in (0, 0.0004, 1, 1999.9996, 2000, 12345.678):
        m = dnn.EventFilter.axis_units(km)
        assert isinstance(m, int) and m >= km * 1000 > m - 1 and dnn.EventFilter.axis_units(dnn.EventFilter.axis_km(m)) == m
    rows = dnn.EventFilter.criteria_rows(768, 1152, min_pixels=(5, 0), min_axis_km=(0, 2000))
    assert rows["min_axis_m"].tolist() == [0, 2000000] and rows["min_pixels"].tolist() == [5, 0]
    assert dnn.EventFilter.criteria_rows(768, 1152).dtype == dnn.EventFilter.CRITERIA
