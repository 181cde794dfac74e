"""Storm-centred composites without a GPU: the numpy checker of tests/util_composite.py against cases worked by hand, nn.composite_bits,
nn.composite_radius_table, the arithmetic of nn.StormComposite.decode, and predict.py's --composite_* flags."""
import math
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_composite as uc


def _word(value, pixel, stat):
    low = pixel if stat == "min" else 0xFFFFFFFF - pixel
    w = (uc.key(value) << 32) | low
    return w - (1 << 64) if w >= 1 << 63 else w


# ------------------------------------------------------------------------------------------------------------------ the checker, by hand
def _hand_case(r0, c0):
    """H = 4, W = 5, one channel holding 10 r + c, bits 1 (q = 20 r + 2 c), R = 1; the event's pixels are its centre and the pixel one row
    towards the grid's middle; a hand-made radius table of two bins"""
    H, W, R = 4, 5, 1
    fields = (10.0 * np.arange(H)[:, None] + np.arange(W)[None, :]).astype(np.float32).reshape(1, H, W, 1)
    inner = r0 + 1 if r0 == 0 else r0 - 1
    root = min(r0, inner) * W + c0
    labels = np.zeros((1, H, W), np.int32)
    labels[0, r0, c0] = labels[0, inner, c0] = root + 1
    table = np.zeros((1, 1, 10), np.int64)
    table[0, 0, :3] = root, 1, 2
    cen = np.asarray([[r0 * W + c0]], np.int32)
    egr = np.asarray([[0]], np.int32)
    rbin = np.full((H, 3, 2), 255, np.uint8)
    rbin[:, 1] = [0, 1]                                # the centre's own row: the centre, one column away
    rbin[:, 0] = rbin[:, 2] = [1, 2]                   # a row away: bin 1 straight above / below, bin 2 (>= NB: nothing) on the diagonal
    return H, W, R, fields, labels, table, cen, egr, rbin


def test_checker_southern_event_in_row_zero_with_a_negated_channel():
    H, W, R, fields, labels, table, cen, egr, rbin = _hand_case(0, 0)
    st = uc.accumulate(uc.empty(1, R, 1, 2), cen, egr, table, labels, fields, [0], [1], negate=[0], flip_south=True, rbin=rbin, R=R)
    # southern (2 * 0 < 3): window row i reads source row 0 - (i - 1); columns 4, 0, 1 (the seam).  i = 0: row 1 -> v = 14, 10, 11;
    # i = 1: row 0 -> v = 4, 0, 1; i = 2: row -1, off the grid.  q = 2 v, negated.
    assert st["events"].tolist() == [1]
    assert st["sum"][0, :, :, 0].tolist() == [[-28, -20, -22], [-8, 0, -2], [0, 0, 0]]
    assert st["n"][0, :, :, 0].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
    assert st["inside"][0].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]
    # bin 0: the centre (0); bin 1: the two neighbours in the row (-8, -2) and the pixel of row 1 straight "above" (-20)
    assert st["rsum"][0, :, 0].tolist() == [0, -30] and st["rn"][0, :, 0].tolist() == [1, 3]
    # as it lies: no reflection, no negation -- row -1 is now window row 0
    st = uc.accumulate(uc.empty(1, R, 1, 2), cen, egr, table, labels, fields, [0], [1], negate=[0], flip_south=False, rbin=rbin, R=R)
    assert st["sum"][0, :, :, 0].tolist() == [[0, 0, 0], [8, 0, 2], [28, 20, 22]]
    assert st["n"][0, :, :, 0].tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1]]
    assert st["inside"][0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 0]]
    assert st["rsum"][0, :, 0].tolist() == [0, 30]
    # without a table nothing radial moves
    st = uc.accumulate(uc.empty(1, R, 1, 2), cen, egr, table, labels, fields, [0], [1], negate=[], flip_south=True, rbin=None, R=R)
    assert not st["rsum"].any() and not st["rn"].any() and st["sum"][0, 0, :, 0].tolist() == [28, 20, 22]


def test_checker_northern_event_in_the_last_row():
    H, W, R, fields, labels, table, cen, egr, rbin = _hand_case(3, 2)
    st = uc.accumulate(uc.empty(1, R, 1, 2), cen, egr, table, labels, fields, [0], [1], negate=[0], flip_south=True, rbin=rbin, R=R)
    # northern (2 * 3 >= 3): window row i reads row 3 + (i - 1): rows 2, 3 and 4 (off); columns 1, 2, 3; nothing is negated
    assert st["sum"][0, :, :, 0].tolist() == [[42, 44, 46], [62, 64, 66], [0, 0, 0]]
    assert st["n"][0, :, :, 0].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
    assert st["inside"][0].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert st["rsum"][0, :, 0].tolist() == [64, 62 + 66 + 44] and st["rn"][0, :, 0].tolist() == [1, 3]


def test_checker_excludes_nonfinite_and_saturated_values():
    H, W, R, fields, labels, table, cen, egr, rbin = _hand_case(3, 2)
    fields = fields.copy()
    fields[0, 2, 1, 0], fields[0, 2, 2, 0], fields[0, 2, 3, 0] = np.nan, np.inf, 2.0 ** 27      # 2^27 * 2 = 2^28: the largest that fits
    fields[0, 3, 1, 0] = np.nextafter(np.float32(2.0 ** 27), np.float32(np.inf))
    st = uc.accumulate(uc.empty(1, R, 1, 2), cen, egr, table, labels, fields, [0], [1], negate=[], flip_south=True, rbin=rbin, R=R)
    assert st["sum"][0, :, :, 0].tolist() == [[0, 0, 1 << 28], [0, 64, 66], [0, 0, 0]]
    assert st["n"][0, :, :, 0].tolist() == [[0, 0, 1], [0, 1, 1], [0, 0, 0]]


def test_checker_centers_categories_and_the_edge_rule():
    H, W, cap, Cf = 4, 5, 4, 2
    table = np.zeros((2, cap, 10), np.int64)
    ftable = np.zeros((2, cap, Cf, 6), np.int64)
    ftable[..., 0] = -1
    table[0, :, 1] = [2, 1, 1, 1]                      # class 2; too small; no finite value; composited
    table[0, :, 2] = [9, 1, 5, 5]
    ftable[0, 0, 1, 0] = _word(1.0, 3, "min")
    ftable[0, 1, 1, 0] = _word(1.0, 4, "min")
    ftable[0, 3, 1, 0] = _word(-3.5, 7, "min")
    ftable[0, 3, 1, 1] = _word(-0.0, 11, "max")
    table[1, 0, 1:3] = 1, 5                            # a frame outside the groups: not looked at
    ftable[1, 0, 1, 0] = _word(0.0, 2, "min")
    ncomp = np.asarray([[5, 4, 1], [1, 1, 0]], np.int32)
    counts = dict.fromkeys(uc.COUNTS, 0)
    cen, egr = uc.centers(table, ncomp, ftable, H, W, 1, "min", (1,), 2, [1, -1], 2, [-3.5, 0.0], counts)
    assert cen.tolist() == [[-1, -1, -1, 7], [-1] * 4]
    assert egr.tolist() == [[-1, -1, -1, 1 * 3 + 1], [-1] * 4]                    # -3.5 >= -3.5, not >= 0: bin 1 of group 1
    assert counts == {"composited": 1, "no_center": 1, "below_min_pixels": 1, "other_class": 1, "uncatalogued": 1}
    counts = dict.fromkeys(uc.COUNTS, 0)
    cen, egr = uc.centers(table, ncomp, ftable, H, W, 1, "max", (1, 2), 0, [0, 1], 2, [0.0], counts)
    # the max words: rows 0 - 2 of frame 0 are empty (0), row 3 holds -0.0 at pixel 11: -0.0 < +0.0, bin 0; frame 1 has no max either
    assert cen.tolist() == [[-1, -1, -1, 11], [-1] * 4] and egr[0, 3] == 0
    assert counts == {"composited": 1, "no_center": 4, "below_min_pixels": 0, "other_class": 0, "uncatalogued": 1}
    assert uc.key(-0.0) + 1 == uc.key(0.0) and uc.key(-1.0) < uc.key(-0.5) < uc.key(1e-45) < uc.key(2.0)
    assert all(uc.key(v) == int(dnn.event_field_key(v)) for v in (-3.5, -0.0, 0.0, 1e-45, 7.25))


# ------------------------------------------------------------------------------------------------------------------ the helpers of nn.py
def test_composite_bits_hand_values():
    got = dnn.composite_bits([0.0, -3.0, 0.0, -100000.0, 0.0, 0.0, -np.inf], [1.0, 2.0, 0.75, 5.0, 0.0, np.nan, 1.0])
    # frexp: 1 = 0.5 * 2^1; 3 = 0.75 * 2^2; 0.75 = 0.75 * 2^0; 1e5 = 0.76 * 2^17
    assert got.dtype == np.int32 and got.tolist() == [26, 25, 27, 10, 0, 0, 0]
    for m, b in ((1.0, 26), (3.0, 25), (100000.0, 10)):
        assert abs(math.ldexp(m, b)) < 2 ** 27 and abs(math.ldexp(2 * m, b)) <= 2 ** 28
    assert (dnn.event_field_bits([-3.0], [2.0]) - dnn.composite_bits([-3.0], [2.0])).tolist() == [12]


def test_composite_radius_table():
    H, W, R, km, bins = 5, 8, 2, 1000.0, 12
    t = dnn.composite_radius_table(H, W, R, km, bins)
    assert t.dtype == np.uint8 and t.shape == (H, 2 * R + 1, R + 1)
    step = 2.0 * math.pi * dnn.EARTH_RADIUS_KM / W                                 # 5003.8 km: bins 0, 5, 10
    assert t[2, R].tolist() == [0, int(step // km), int(2 * step // km)] == [0, 5, 10]
    assert np.array_equal(t[2, R + 1], t[2, R - 1]) and np.array_equal(t[2, R + 2], t[2, R - 2])     # the equator row: symmetric in d
    quarter = math.pi * dnn.EARTH_RADIUS_KM / 4                                     # one row of H = 5 is 45 degrees: 5003.8 km again
    assert t[2, R + 1, 0] == int(quarter // km) == 5 and t[2, R + 2, 0] == 10
    assert (t[0, :R] == 255).all() and (t[H - 1, R + 1:] == 255).all() and (t[1, 0] == 255).all() and (t[1, 1] != 255).any()
    assert t[0, R].tolist() == [0, 0, 0]                                            # the pole: every column is the same point
    tight = dnn.composite_radius_table(H, W, R, km, 10)                             # 255 beyond the bins
    assert tight[2, R].tolist() == [0, 5, 255] and np.array_equal(tight[t < 10], t[t < 10]) and (tight[t >= 10] == 255).all()
    wide = dnn.composite_radius_table(H, W, R, 10.0, 255)                           # a bin that would not fit a byte
    assert wide[2, R].tolist() == [0, 255, 255]
    assert dnn.composite_radius_table(7, 9, 1, 25.0, 0).tolist() == np.full((7, 3, 2), 255).tolist()
    for bad in ((0, 8, 1, 25.0, 4), (5, 8, 0, 25.0, 4), (5, 8, 41, 25.0, 4), (5, 8, 1, 0.0, 4), (5, 8, 1, 25.0, 256)):
        with pytest.raises(L.DeepcamHipError):
            dnn.composite_radius_table(*bad)


def test_decode_arithmetic_and_radius_of_max_with_ties():
    GT, S, C, NB = 2, 3, 2, 4
    events = np.asarray([4, 0], np.int64)
    total = np.zeros((GT, S, S, C), np.int64)
    n = np.zeros((GT, S, S, C), np.int32)
    inside = np.zeros((GT, S, S), np.int32)
    total[0, 1, 1], n[0, 1, 1] = [12, -10], [4, 2]
    inside[0, 1, 1], inside[0, 0, 2] = 4, 1
    rsum = np.zeros((GT, NB, C), np.int64)
    rn = np.zeros((GT, NB, C), np.int64)
    rsum[0, :, 0], rn[0, :, 0] = [8, 24, 36, 5], [2, 4, 6, 0]                      # means 1, 1.5, 1.5, none: the tie goes to bin 1
    rsum[0, :, 1], rn[0, :, 1] = [-4, -8, 0, 0], [1, 1, 0, 0]                      # means -0.5, -1: bin 0
    d = dnn.StormComposite.decode(events, total, n, inside, rsum, rn, bits=[2, 3], bin_km=50.0)
    assert d["mean"].shape == (GT, S, S, C) and d["mean"][0, 1, 1].tolist() == [12 / 4 / 4, -10 / 8 / 2]
    assert np.isnan(d["mean"][0, 0, 0]).all() and np.isnan(d["mean"][1]).all()
    assert d["footprint"][0, 1, 1] == 1.0 and d["footprint"][0, 0, 2] == 0.25 and d["footprint"][0, 0, 0] == 0.0 and np.isnan(d["footprint"][1]).all()
    assert d["radial_mean"][0, :3, 0].tolist() == [1.0, 1.5, 1.5] and np.isnan(d["radial_mean"][0, 3, 0])
    assert d["radial_mean"][0, :2, 1].tolist() == [-0.5, -1.0]
    assert d["radius_km"].tolist() == [25.0, 75.0, 125.0, 175.0]
    assert d["radius_of_max_km"][0].tolist() == [75.0, 25.0] and np.isnan(d["radius_of_max_km"][1]).all()
    none = dnn.StormComposite.decode(events, total, n, inside, np.zeros((GT, 0, C), np.int64), np.zeros((GT, 0, C), np.int64), [2, 3])
    assert none["radial_mean"].shape == (GT, 0, C) and none["radius_km"].shape == (0,) and np.isnan(none["radius_of_max_km"]).all()


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_entry_points_are_declared_bound_and_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deepcam_hip.h")).read()
    for name in ("dc_composite_centers", "dc_composite_accumulate", "dc_composite_chunk"):
        assert f"int {name}(" in hdr and name in L.EXPORTS
    assert "composite.hip" in open(os.path.join(root, "mlperf-deepcam_amd", "csrc", "Makefile")).read()
    doc = hdr[hdr.index("Storm-centred composites"):hdr.index("int dc_composite_chunk")]
    for word in dnn.COMPOSITE_COUNTS + ("2^21", "2^28", "negate_mask", "flip_south", "periodic", "poles"):
        assert word in doc, word
    assert dnn.COMPOSITE_MAX_EVENTS == 1 << 21 and dnn.COMPOSITE_COUNTS == uc.COUNTS and dnn.COMPOSITE_KEYS == uc.KEYS


# ------------------------------------------------------------------------------------------------------------------ the driver's flags
BASE = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]


def test_composite_flags_are_parsed_and_validated():
    from mlperf_deepcam_amd import predict
    parse = predict.build_parser().parse_args
    plain = parse(BASE)
    assert not [k for k in vars(plain) if k.startswith("composite")] and plain.event_fields is False and plain.events is False
    every = parse(BASE + ["--composites", "--composite_center_channel", "0", "--composite_center_stat", "min", "--composite_radius", "1",
                          "--composite_channels", "0", "--composite_negate", "--composite_classes", "1", "--composite_min_pixels", "0",
                          "--composite_by", "all", "--composite_intensity_edges", "--composite_no_flip", "--composite_bin_km", "1",
                          "--composite_bins", "1"])
    assert sorted(predict.COMPOSITE_DEFAULTS) == sorted(k for k in vars(every) if k.startswith("composite_"))     # a default for every flag
    a = parse(BASE + ["--composites", "--composite_center_channel", "5"])
    assert a.composites and a.event_fields and a.events
    kw = predict.composite_options(a, 16, 1152)
    assert kw == {"center_channel": 5, "center_stat": "min", "radius": 32, "channels": list(range(16)), "classes": (1,), "min_pixels": 0,
                  "groups": 1, "intensity_edges": (), "flip_south": True, "negate": (), "bin_km": 25.0, "bins": 40}
    a = parse(BASE + ["--composites", "--composite_center_channel", "2", "--composite_center_stat", "max", "--composite_radius", "7",
                      "--composite_channels", "4", "0", "9", "--composite_negate", "9", "4", "--composite_classes", "2", "1",
                      "--composite_min_pixels", "12", "--composite_by", "season", "--composite_intensity_edges", "-5.5", "980", "--composite_no_flip",
                      "--composite_bin_km", "50", "--composite_bins", "20"])
    kw = predict.composite_options(a, 16, 64)
    assert kw == {"center_channel": 2, "center_stat": "max", "radius": 7, "channels": [4, 0, 9], "classes": (1, 2), "min_pixels": 12,
                  "groups": 4, "intensity_edges": (-5.5, 980.0), "flip_south": False, "negate": (2, 0), "bin_km": 50.0, "bins": 20}
    assert predict.composite_group_names("season", kw["intensity_edges"])[:4] == ["DJF.bin0", "DJF.bin1", "DJF.bin2", "MAM.bin0"]
    assert predict.composite_group_names("all", ()) == ["all"]
    with pytest.raises(ValueError, match="composite_center_channel"):              # --composites without a centre channel
        predict.composite_options(parse(BASE + ["--composites"]), 16, 1152)
    bad = [["--composite_center_channel", "16"], ["--composite_center_channel", "0", "--composite_channels", "16"],
           ["--composite_center_channel", "0", "--composite_channels", "1", "1"],
           ["--composite_center_channel", "0", "--composite_channels", "1", "2", "--composite_negate", "3"],
           ["--composite_center_channel", "0", "--composite_radius", "41"], ["--composite_center_channel", "0", "--composite_radius", "0"],
           ["--composite_center_channel", "0", "--composite_intensity_edges", "2", "1"],
           ["--composite_center_channel", "0", "--composite_intensity_edges", "nan"],
           ["--composite_center_channel", "0", "--composite_min_pixels", "-1"], ["--composite_center_channel", "0", "--composite_bins", "256"],
           ["--composite_center_channel", "0", "--composite_bin_km", "0"]]
    for extra in bad:
        with pytest.raises(ValueError):
            predict.composite_options(parse(BASE + ["--composites"] + extra), 16, 1152)
    with pytest.raises(ValueError):                                                 # a window wider than the grid
        predict.composite_options(parse(BASE + ["--composites", "--composite_center_channel", "0", "--composite_radius", "8"]), 16, 16)
    for extra in (["--composite_center_stat", "mean"], ["--composite_by", "year"], ["--composite_classes", "3"]):
        with pytest.raises(SystemExit):
            parse(BASE + ["--composites", "--composite_center_channel", "0"] + extra)
