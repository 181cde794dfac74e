"""The checkers of tests/util_event_axis.py against hand-worked cases written out as literals, and the host side of nn.EventAxis that
needs no GPU: the link table and dc_thin_lds_bytes."""
import math

import numpy as np

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_axis as ua


def _plane(text):
    return np.array([[ch == "#" for ch in row] for row in text.split()])


THIN = {   # name: (plane, skeleton, passes)
    "a 2 x 2 square thins to one pixel": (".... .##. .##. ....", ".... ..#. .... ....", 2),
    "a single pixel is kept": ("... .#. ...", "... .#. ...", 1),
    "a 3-wide bar keeps its middle row, shortened at both ends": ("............ .##########. .##########. .##########. ............",
                                                                  "............ ............ ..########.. ............ ............", 2),
    # C == 1, N == 2 and m == 0 hold at the corner pixel of an L in sub-pass A: the rule takes it and leaves the arms diagonally joined
    "an L of one-pixel width loses its corner pixel only": ("....... .#..... .#..... .#####. .......",
                                                            "....... .#..... .#..... ..####. .......", 2),
    "a closed ring of one-pixel width is a fixed point": ("...... ..##.. .#..#. .#..#. ..##.. ......", "...... ..##.. .#..#. .#..#. ..##.. ......", 1),
}


def test_thinning_checker_on_hand_worked_planes():
    for name, (plane, skeleton, passes) in THIN.items():
        for wrap in (0, 1):
            got, n, converged = ua.thin_plane(_plane(plane), wrap, 10)
            assert np.array_equal(got, _plane(skeleton)) and (n, converged) == (passes, 1), name
    skel, iters = ua.thin(np.array([[[0, 1, 1, 0, 2], [0, 1, 1, 0, 3]]]), 1, 0, 10)          # both classes of one frame; 3 is background
    assert skel.tolist() == [[[0, 0, 1, 0, 2], [0, 0, 0, 0, 0]]] and iters.tolist() == [[[2, 1], [1, 1]]]
    assert ua.thin_plane(_plane(THIN["a 2 x 2 square thins to one pixel"][0]), 0, 1)[1:] == (1, 0)      # stopped by max_iters


def test_statistics_checker_on_hand_worked_skeletons():
    link = np.array([[100, 70, 120]] * 5, np.int32) * np.arange(1, 6, dtype=np.int32)[:, None]     # row i: (i + 1) x (100, 70, 120)
    one = lambda text: ua.stats(_plane(text).astype(np.uint8), _plane(text).astype(np.int32) * 9, [8], 2, 0, link)[0].tolist()  # noqa: E731
    # an L: 3 N-S links (rows 0, 1, 2) and 3 E-W links on row 3; the diagonal from (2, 1) to (3, 2) runs beside the corner pixel: not a link
    assert one(".#.... .#.... .#.... .####. ......") == [7, 2, 0, 3, 3, 0, 3 * 400 + 70 + 140 + 210]
    # the same without its corner pixel: that diagonal is now the link, from row 2
    assert one(".#.... .#.... .#.... ..###. ......") == [6, 2, 0, 2, 2, 1, 2 * 400 + 70 + 140 + 360]
    # a closed ring: no endpoints; four diagonals (rows 0, 0, 2, 2), two E-W (rows 0, 3) and two N-S links (row 1)
    ring = one("..##.. .#..#. .#..#. ..##.. ......")
    assert ring == [8, 0, 0, 2, 2, 4, 100 + 400 + 2 * 140 + 2 * 120 + 2 * 360]
    # a T with arms of two pixels: three endpoints, and only the pixel where the arms meet sees three separate runs of neighbours
    assert one("..#.. ..#.. ##### ..... .....")[:3] == [7, 3, 1]
    d = dnn.EventAxis.decode([ring, [5, 3, 1, 2, 2, 0, 2500]], np.array([[8, 2, 20, 0, 0, 0, 0, 0, 3, 0]] * 2), 5, 6)
    assert d[0] == {"class": 2, "skeleton_pixels": 8, "endpoints": 0, "junctions": 0, "branches": 0, "axis_km": 1.74, "closed": True}
    assert (d[1]["branches"], d[1]["closed"], d[1]["axis_km"]) == (1, False, 2.5)
    # two events side by side, and columns that wrap: labels keep diagonal neighbours of different events apart
    skel = _plane("#..#. .##.# .....").astype(np.uint8)
    labels = np.array([[1, 0, 0, 4, 0], [0, 1, 4, 0, 1], [0, 0, 0, 0, 0]], np.int32)
    assert ua.stats(skel, labels, [0, 3], 2, 1, link).tolist() == [[3, 2, 0, 0, 0, 2, 240], [2, 2, 0, 0, 0, 1, 120]]
    assert ua.stats(skel, labels, [0, 3], 1, 0, link).tolist() == [[3, 2, 0, 0, 0, 1, 120]]      # no wrap: (1, 4) has no neighbour; cap 1


def test_link_table_and_lds_bytes_without_gpu():
    H, W, R = 768, 1152, 6371.0
    t = dnn.axis_link_table(H, W)
    assert t.shape == (H, 3) and t.dtype == np.int32 and dnn.EVENT_AXIS_FIELDS[6] == "length_m" and len(dnn.EVENT_AXIS_FIELDS) == ua.FIELDS
    lat = lambda i: math.radians(-90.0 + 180.0 * i / (H - 1))  # noqa: E731
    dlon = 2.0 * math.pi / W
    assert t[384, 0] == round(R * 1000 * math.cos(lat(384)) * dlon) and 34000 < t[384, 0] < 35000
    assert t[100, 1] == round(R * 1000 * math.pi / (H - 1)) == 26095
    h = math.sin((lat(201) - lat(200)) / 2) ** 2 + math.cos(lat(200)) * math.cos(lat(201)) * math.sin(dlon / 2) ** 2
    assert t[200, 2] == round(2 * R * 1000 * math.asin(math.sqrt(h))) and t[H - 1, 2] == 0 and t[0, 0] == 0
    lds = L.load().dc_thin_lds_bytes
    assert lds(768, 1152) == 110592 + 64 and lds(8, 64) == 64 + 64 and lds(9, 65) == 9 * 2 * 8 + 64
    assert lds(1279, 1024) == 1279 * 128 + 64 and lds(1280, 1024) == 0 and lds(1024, 2048) == 0 and lds(0, 64) == 0
    fake = 4096
    assert L.load().dc_mask_thin(1, 1, 1024, 2048, fake, 1, 1, 10, 1 << 30, fake, None) != 0 and "does not fit the LDS" in L.last_error()
    assert L.load().dc_mask_thin(1, 1, 8, 64, fake, 2, 1, 10, 1 << 30, fake, None) != 0 and "mask_bytes" in L.last_error()
    assert L.load().dc_mask_thin(1, 1, 8, 64, fake, 1, 1, 0, 1 << 30, fake, None) != 0 and "max_iters" in L.last_error()
    assert L.load().dc_mask_thin(1, 1, 8, 64, fake, 1, 1, 10, fake + 8, fake, None) != 0 and "alias" in L.last_error()
    assert L.load().dc_skeleton_stats(1, 1, 8, 64, fake, fake, fake, 0, 1, fake, fake, None) != 0 and "cap" in L.last_error()
