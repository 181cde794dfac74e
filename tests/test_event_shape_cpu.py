"""Event shapes and the shape filter, host side (no GPU): the checker of tests/util_event_shape.py and nn.EventShape.decode against
analysis, the faces by hand, the int64 budget, the threshold helpers, the argument checks of the C ABI and the driver's flags.

The analytic side evaluates the SAME formulas (the decode of include/deepcam_hip.h) from exact float64 trigonometry with no integer tables:
a table entry is off by at most 2^-21, a per-pixel product of two by at most 2^-20, an entry of C (a weighted mean of products, minus a
product of two such means) by at most 3 * 2^-20, and the spectral norm of a symmetric 2 x 2 matrix is at most twice its largest entry:
2^-16 leaves about 2.7 x."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_shape as us
import util_events as ue

H, W = 181, 360
R = dnn.EARTH_RADIUS_KM
DLAT, DLON = dnn.EventShape.steps(H, W)
EIG_TOL = 2.0 ** -16


def _strip_zonal(shift=0):
    m = np.zeros((H, W), np.uint8)
    m[90, 100:160] = 2
    return np.roll(m, shift, axis=1)


def _strip_meridional():
    m = np.zeros((H, W), np.uint8)
    m[60:120, 180] = 2
    return m


def _disc():
    rr, cc = np.mgrid[0:H, 0:W]
    return (((rr - 100) ** 2 + (cc - 200) ** 2) <= 15 ** 2).astype(np.uint8)


SHAPES = {"zonal": _strip_zonal, "seam": functools.partial(_strip_zonal, 230), "meridional": _strip_meridional, "disc": _disc}


@functools.lru_cache(maxsize=None)
def _decoded(name):
    """(mask, catalogue rows, shape rows, decode's dicts) of one test shape through the integer tables"""
    mask = SHAPES[name]()
    labels, rows = ue.label_one(mask, 8, True, *dnn.event_weight_tables(H, W))
    srows = us.shape_rows(labels, rows, True, *dnn.event_shape_tables(H, W))
    assert len(rows) == 1
    return mask, rows, srows, dnn.EventShape.decode(srows, rows, H, W)


def _analytic(mask):
    """lambda+, lambda- from float64 trigonometry: the decode formula with exact weights and unit vectors"""
    lat, lon = np.deg2rad(np.linspace(-90.0, 90.0, H)), np.deg2rad(-180.0 + 360.0 * np.arange(W) / W)
    rr, cc = np.nonzero(mask)
    cl, sl, co, so = np.cos(lat[rr]), np.sin(lat[rr]), np.cos(lon[cc]), np.sin(lon[cc])
    u = np.stack([cl * co, cl * so, sl], axis=1)
    s0 = cl.sum()
    m = (cl[:, None] * u).sum(axis=0) / s0
    cov = np.einsum("k,ki,kj->ij", cl, u, u) / s0 - np.outer(m, m)
    c = m / np.linalg.norm(m)
    la, lo = math.asin(c[2]), math.atan2(c[1], c[0])
    e = np.array([-math.sin(lo), math.cos(lo), 0.0])
    n = np.array([-math.sin(la) * math.cos(lo), -math.sin(la) * math.sin(lo), math.cos(la)])
    a, b, d = e @ cov @ e, e @ cov @ n, n @ cov @ n
    rad = math.sqrt(((a - d) / 2) ** 2 + b * b)
    return max((a + d) / 2 + rad, 0.0), max((a + d) / 2 - rad, 0.0), math.degrees(la), math.degrees(lo)


# ------------------------------------------------------------------------------------------------------------------ tables
def test_shape_tables():
    """the catalogue's latitudes; the longitudes of a periodic grid of W columns (a roll by k columns is a rotation by k steps)"""
    rows, cols = dnn.event_shape_tables(H, W)
    wy, cx, sx = dnn.event_weight_tables(H, W)
    assert rows.shape == (6, H) and cols.shape == (5, W) and rows.dtype == np.int32 and cols.dtype == np.int32
    assert np.array_equal(rows[0], wy)
    assert cols[0, 0] == -(1 << 20) and cols[1, 0] == 0 and cols[0, W // 2] == 1 << 20          # -180 and 0 degrees
    assert (cols[0, W - 1], cols[1, W - 1]) == (cols[0, 1], -cols[1, 1])                           # one step west of column 0
    assert (cx[0], cx[W - 1]) == (-(1 << 20), -(1 << 20))                                           # the catalogue's own holds the seam twice
    assert dnn.EventShape.steps(H, W) == (math.pi / (H - 1), 2 * math.pi / W)
    lat, lon = np.deg2rad(np.linspace(-90.0, 90.0, H)), np.deg2rad(-180.0 + 360.0 * np.arange(W) / W)
    exact_r = [np.cos(lat), np.cos(lat) ** 2, np.cos(lat) * np.sin(lat), np.cos(lat) ** 3, np.cos(lat) ** 2 * np.sin(lat),
               np.cos(lat) * np.sin(lat) ** 2]
    exact_c = [np.cos(lon), np.sin(lon), np.cos(lon) ** 2, np.cos(lon) * np.sin(lon), np.sin(lon) ** 2]
    for t, x in zip(list(rows) + list(cols), exact_r + exact_c):
        assert np.abs(t / 2.0 ** 20 - x).max() <= 2.0 ** -21 + 1e-15 and np.abs(t).max() <= 1 << 20


# ------------------------------------------------------------------------------------------------------------------ checker vs analysis
@pytest.mark.parametrize("name", list(SHAPES))
def test_eigenvalues_against_float64_trigonometry(name):
    mask, rows, srows, dec = _decoded(name)
    lp, lm, lat, lon = _analytic(mask)
    got = us.eigenvalues(srows[0].tolist(), rows[0, 3])
    _, _, _, _, _, mp, mm, _ = dnn.EventShape.moments(srows, rows)
    print(f"{name}: lambda+ {got[0]:.9e} vs {lp:.9e} (diff {got[0] - lp:+.2e}), lambda- {got[1]:.9e} vs {lm:.9e} (diff {got[1] - lm:+.2e})")
    assert lp >= 1e-2                                                      # so that 2^-16 absolute means something
    assert abs(got[0] - lp) <= EIG_TOL and abs(got[1] - lm) <= EIG_TOL
    assert abs(mp[0] - lp) <= EIG_TOL and abs(mm[0] - lm) <= EIG_TOL       # nn's array form of the same formula
    assert abs(mp[0] - got[0]) <= 1e-12 and abs(mm[0] - got[1]) <= 1e-12
    assert abs(dec[0]["lat"] - lat) <= 1e-3 and abs((dec[0]["lon"] - lon + 180.0) % 360.0 - 180.0) <= 1e-3
    theta = dec[0]["length_km"] / R                                         # the great-circle arc with this second moment
    assert 6.0 * (1.0 - math.sin(theta) / theta) == pytest.approx(12 * mp[0], rel=1e-9) and theta >= math.sqrt(12 * mp[0])
    assert dec[0]["aspect"] == (pytest.approx(math.sqrt(mp[0] / mm[0]), rel=1e-12) if mm[0] > 0 else math.inf)
    assert dec[0]["width_km"] == pytest.approx(R * math.sqrt(12 * mm[0]), rel=1e-12)


def test_orientation_and_aspect_of_the_strips_and_the_disc():
    zonal, merid, disc = _decoded("zonal")[3][0], _decoded("meridional")[3][0], _decoded("disc")[3][0]
    assert abs(zonal["orientation_deg"]) < 0.1 or abs(abs(zonal["orientation_deg"]) - 180.0) < 0.1
    assert abs(abs(merid["orientation_deg"]) - 90.0) < 0.1 and -90.0 < merid["orientation_deg"] <= 90.0
    assert zonal["aspect"] > 30 and merid["aspect"] > 30 and 1.0 <= disc["aspect"] < 1.2
    assert 0.5 < disc["compactness"] < 0.7                                 # a disc drawn in squares has its bounding square's perimeter: pi^2 / 16
    assert disc["area_km2"] == pytest.approx(float(_decoded("disc")[0].sum()) * dnn.EventFilter.pixel_area_km2(H, W) * math.cos(math.radians(10)),
                                             rel=0.02)


def test_zonal_strip_length_within_one_percent():
    """60 pixels on the equator: length_km within 1 % of 60 dlon R.  R sqrt(12 lambda+) alone, the chord-space figure, is 2.7 % short of
    this strip; length_km is the great-circle arc with that second moment."""
    want = 60 * DLON * R
    got = _decoded("zonal")[3][0]["length_km"]
    print(f"zonal strip: length_km {got:.1f} vs 60 dlon R = {want:.1f} ({100 * (got / want - 1):+.2f} %)")
    assert abs(got / want - 1.0) <= 0.01
    chord = R * math.sqrt(12 * us.eigenvalues(_decoded("zonal")[2][0].tolist(), _decoded("zonal")[1][0, 3])[0])
    assert 0.02 < 1.0 - chord / want < 0.03


def test_seam_copy_has_the_perimeter_and_faces_of_the_unrolled_strip():
    a, b = _decoded("zonal"), _decoded("seam")
    assert b[0][90, 0] and b[0][90, W - 1] and int(b[1][0, 9]) == 1        # it does cross the seam
    assert a[2][0, :3].tolist() == b[2][0, :3].tolist() == [60, 2, 120 << 20]
    assert b[3][0]["perimeter_km"] == pytest.approx(a[3][0]["perimeter_km"], rel=1e-4)
    assert a[3][0]["perimeter_km"] == pytest.approx(R * (2 * DLAT + 120 * DLON), rel=1e-12)


def test_seam_copy_has_the_length_of_the_unrolled_strip():
    """within 1e-4 relative: the 2^-16 bound on lambda+ (>= 1e-2) allows 8e-4 of lambda+, 4e-4 of its root; the columns are a periodic
    grid, so the roll is a rotation and only the tables' rounding differs (observed: 7e-10)."""
    a, b = _decoded("zonal")[3][0], _decoded("seam")[3][0]
    print(f"length_km unrolled {a['length_km']:.3f}, across the seam {b['length_km']:.3f} (rel {b['length_km'] / a['length_km'] - 1:+.3e})")
    assert b["length_km"] == pytest.approx(a["length_km"], rel=1e-4)


# The rolled strip's width against the unrolled strip's, both through the integer tables: the observed difference is 0 -- both widths ARE 0
#  --, and twice that is the margin.  The pixels are points: a one-pixel-wide strip on the equator lies in the plane
# z = 0, rcs[90] = 0 exactly, so S_z, S_xz, S_yz, S_zz, with them b and d, and lambda- = a / 2 - |a| / 2 are exact zeros for either copy.
WIDTH_SEAM_MARGIN = 0.0


def test_seam_copy_has_the_width_of_the_unrolled_strip():
    """The 2^-16 bound says nothing about the width of a one-pixel-wide strip and a roll shifts the column tables, so the margin comes
    from the pipeline itself: twice the difference observed through the integer tables, which H and W fix."""
    a, b = _decoded("zonal")[3][0], _decoded("seam")[3][0]
    diff = abs(b["width_km"] - a["width_km"])
    rel = diff / a["width_km"] if a["width_km"] > 0 else (0.0 if diff == 0 else math.inf)
    print(f"width_km unrolled {a['width_km']:.4f}, across the seam {b['width_km']:.4f} (rel {rel:.3e}, margin {WIDTH_SEAM_MARGIN:.1e})")
    assert rel <= WIDTH_SEAM_MARGIN


# ------------------------------------------------------------------------------------------------------------------ faces by hand
def _faces(mask, conn=4, wrap=False):
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    labels, rows = ue.label_one(mask, conn, wrap, *dnn.event_weight_tables(h, w))
    return rows, us.shape_rows(labels, rows, wrap, *dnn.event_shape_tables(h, w)), dnn.event_weight_tables(h, w)[0].astype(np.int64)


def test_faces_of_a_rectangle():
    m = np.zeros((12, 16), np.uint8)
    m[3:7, 5:12] = 1                                                       # 4 rows x 7 columns
    rows, s, wy = _faces(m)
    assert len(rows) == 1 and s[0, :3].tolist() == [2 * (4 + 7) - 4, 2 * 4, 7 * int(wy[3] + wy[6])]
    # against the grid's edges every side is exposed too: rows never wrap, columns only with wrap
    m = np.ones((3, 5), np.uint8)
    rows, s, wy = _faces(m)
    assert s[0, :3].tolist() == [12, 6, 5 * int(wy[0] + wy[2])]
    rows, s, wy = _faces(m, wrap=True)
    assert s[0, :3].tolist() == [10, 0, 5 * int(wy[0] + wy[2])]


def test_faces_of_a_shape_with_a_hole():
    m = np.zeros((9, 9), np.uint8)
    m[2:7, 2:7] = 2
    m[4, 4] = 0
    rows, s, wy = _faces(m)
    assert len(rows) == 1 and int(rows[0, 2]) == 24
    assert s[0, :3].tolist() == [16 + 4, 2 * 5 + 2, 5 * int(wy[2] + wy[6]) + int(wy[3] + wy[5])]
    m[4, 4] = 1                                                            # another event in the hole: still "not of the same component"
    rows, s, wy = _faces(m)
    assert len(rows) == 2 and s[0, :3].tolist() == [20, 12, 5 * int(wy[2] + wy[6]) + int(wy[3] + wy[5])]
    assert s[1, :3].tolist() == [1, 2, 2 * int(wy[4])]


def test_two_diagonal_pixels_are_one_event_with_eight_faces():
    m = np.zeros((6, 6), np.uint8)
    m[2, 2] = m[3, 3] = 1
    rows, s, wy = _faces(m, conn=8)
    assert len(rows) == 1 and s[0, :3].tolist() == [2, 4, 2 * int(wy[2] + wy[3])]
    rows, s, wy = _faces(m, conn=4)
    assert len(rows) == 2 and s[:, 1].tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------------------------ int64 budget
def test_the_sums_of_a_whole_frame_fit_int64():
    """768 x 1152, all foreground, one event: the nine sums factor into (row sum) x (column sum); Python ints, no pixel loop."""
    h, w = 768, 1152
    rows, cols = (t.astype(object) for t in dnn.event_shape_tables(h, w))
    rs, cs = [int(sum(r)) for r in rows], [int(sum(c)) for c in cols]
    wy, c2, cs_, c3, c2s, cs2 = rs
    cx, sx, cxx, cxy, cyy = cs
    sums = [c2 * cx, c2 * sx, cs_ * (1 << 20) * w, c3 * cxx, c3 * cxy, c3 * cyy, c2s * cx, c2s * sx, cs2 * (1 << 20) * w]
    worst = [int(sum(abs(int(v)) for v in r)) * int(sum(abs(int(v)) for v in c)) for r in rows[1:] for c in cols]     # no cancellation
    assert all(abs(v) < 1 << 63 for v in sums) and all(v < 1 << 63 for v in worst)
    assert h * w <= 1 << 22 and max(int(np.abs(t).max()) for t in dnn.event_shape_tables(h, w)) <= 1 << 20
    assert wy * w * (1 << 20) < 1 << 63                                    # the zeroth moment, field 3 times 2^20
    assert 2 * w * int(rows[0].max()) < 1 << 63 and 2 * h * w < 1 << 63    # the faces


# ------------------------------------------------------------------------------------------------------------------ thresholds
def test_threshold_helpers_round_trip():
    F = dnn.EventFilter
    for km in (0.0, 500.0, 2000.0, 6371.0):
        assert F.length_km(F.length_units(km)) == pytest.approx(km, rel=1e-9, abs=1e-6)
    assert F.length_units(2000.0) == pytest.approx(6.0 * (1.0 - math.sin(2000.0 / R) / (2000.0 / R)), rel=1e-12)
    assert F.length_units(2000.0) < (2000.0 / R) ** 2
    with pytest.raises(L.DeepcamHipError):
        F.length_units(30000.0)
    for a in (0.0, 1.0, 2.0, 3.5):
        assert F.aspect(F.aspect_units(a)) == pytest.approx(a, rel=1e-12)
    for km2 in (0.0, 1.0e4, 2.5e5, 1.0e6):
        u = F.area_units(km2, 768, 1152)
        assert isinstance(u, int) and F.area_km2(u, 768, 1152) >= km2 * (1 - 1e-12)
        assert u == 0 or F.area_km2(u - 1, 768, 1152) < km2                # the smallest integer area that reaches km2
    assert F.pixel_area_km2(181, 360) == pytest.approx((R * math.pi / 180) ** 2, rel=1e-12)
    rows = F.criteria_rows(768, 1152, (3, 10), (0, 2.5e5), (0, 2000), (0, 2))
    assert rows.dtype.itemsize == 32 and rows["min_pixels"].tolist() == [3, 10]
    assert rows["min_area"].tolist() == [0, F.area_units(2.5e5, 768, 1152)]
    assert rows["min_len2"].tolist() == [0.0, F.length_units(2000)] and rows["min_aspect2"].tolist() == [0.0, 4.0]
    # the checker's keep rule reads the same rows: a 60-pixel strip is a river by these, a disc is not
    crit = [tuple(r) for r in F.criteria_rows(H, W, (0, 0), (0, 0), (2000, 2000), (2, 2)).tolist()]
    for name, want in (("zonal", True), ("meridional", True)):
        _, r, s, _ = _decoded(name)
        assert us.keep_flags(r, s.tolist(), crit) == [want]
    _, r, s, _ = _decoded("disc")
    r = r.copy()
    r[0, 1] = 2
    assert us.keep_flags(r, s.tolist(), crit) == [False]


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_argument_checks_without_a_gpu():
    lib = L.load()
    fake = C.c_void_p(4096)
    assert lib.dc_component_shape(1, 1, 2049, 2048, fake, fake, 4, 1, fake, fake, fake, None) != 0      # H * W > 2^22
    assert "2^22" in L.last_error()
    assert lib.dc_component_shape(2, 3, 8, 8, fake, fake, 4, 1, fake, fake, fake, None) != 0
    assert lib.dc_component_shape(2, 2, 8, 8, fake, fake, 0, 1, fake, fake, fake, None) != 0
    assert lib.dc_component_shape(2, 2, 8, 8, fake, fake, 4, 2, fake, fake, fake, None) != 0
    assert lib.dc_component_shape(2, 2, 8, 8, fake, None, 4, 1, fake, fake, fake, None) != 0
    assert lib.dc_event_select(2, 0, 4, fake, fake, fake, fake, fake, fake, None) != 0
    assert lib.dc_event_select(2, 2, 4, fake, fake, fake, None, fake, fake, None) != 0
    assert lib.dc_mask_select(2, 2, 8, 8, fake, fake, fake, 4, fake, fake, fake, None) != 0               # out_mask aliases mask
    assert "alias" in L.last_error()
    assert lib.dc_mask_select(2, 2, 8, 8, fake, fake, fake, 4, fake, C.c_void_p(4096 + 64), fake, None) != 0   # overlapping
    assert lib.dc_mask_select(2, 2, 8, 8, fake, fake, fake, 0, fake, C.c_void_p(8192), fake, None) != 0


# ------------------------------------------------------------------------------------------------------------------ driver flags
BASE = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
TODAY = {'checkpoint': 'c', 'data_dir': 'd', 'stats_file': 's', 'output_dir': 'o', 'batch_size': 8, 'channels': list(range(16)),
         'amp_opt_level': 'O1', 'dtype': None, 'confidence': False, 'events': False, 'min_event_pixels': 0, 'event_connectivity': 8,
         'verify': False, 'min_event_cover': 0.5, 'event_fields': False, 'plots': False, 'plot_every': 1, 'plot_channel': 0, 'tracks': False,
         'min_track_frames': 1, 'min_track_pixels': 0, 'track_fields': False, 'track_center_channel': None, 'climatology': False,
         'climatology_by': 'all', 'climatology_channels': [], 'climatology_contour': 0.1, 'height': 768, 'width': 1152,
         'max_inter_threads': 4}


def test_driver_flags():
    from mlperf_deepcam_amd import predict
    ap = predict.build_parser()
    plain = vars(ap.parse_args(BASE))
    assert {k: plain[k] for k in TODAY} == TODAY                           # the existing attributes are what they were
    new = {k: v for k, v in plain.items() if k not in TODAY}
    assert new == {"event_shape": False, "event_filter": False, "filter_min_pixels": [0, 0], "filter_min_area_km2": [0.0, 0.0],
                   "filter_min_length_km": [0.0, 0.0], "filter_min_aspect": [0.0, 0.0]}
    ns = ap.parse_args(BASE + ["--event_shape"])
    assert ns.event_shape is True and ns.events is True and ns.event_filter is False
    ns = ap.parse_args(BASE + ["--event_filter", "--filter_min_pixels", "3", "10", "--filter_min_area_km2", "0", "2.5e5",
                               "--filter_min_length_km", "0", "2000", "--filter_min_aspect", "0", "2"])
    assert ns.event_filter is True and ns.events is False and ns.filter_min_pixels == [3, 10]
    assert ns.filter_min_area_km2 == [0.0, 2.5e5] and ns.filter_min_length_km == [0.0, 2000.0] and ns.filter_min_aspect == [0.0, 2.0]
    assert "NOT filtered" in ap.format_help()
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ["--filter_min_aspect", "2"])
