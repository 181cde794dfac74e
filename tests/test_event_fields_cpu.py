"""The event intensities' host side (no GPU): the checker of tests/util_event_fields.py against a hand-computed example, the float keys,
the tie rule, nn.event_field_bits, nn.EventFields.decode on hand-built rows, the argument checks of the C ABI and the driver's flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_fields as uf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

# 4 x 6, 4-connectivity, wrap.  Components in root order: A class 1 {(0,0) (0,1) (1,1)} root 0; B class 2 {(0,5) (1,5)} root 5 (it touches
# A across the seam, but A has another class); C class 2 {(3,0) (3,5)} root 18, joined across the seam
MASK = [[1, 1, 0, 0, 0, 2],
        [0, 1, 0, 0, 0, 2],
        [0, 0, 0, 0, 0, 0],
        [2, 0, 0, 0, 0, 2]]
# one channel, bits = 1 (q = rint(2 v)); 99 marks background values, which nothing may read
FIELD = [[1.25, -3.0, 99, 99, 99, NAN],
         [99, 1.25, 99, 99, 99, -0.0],
         [99, 99, 99, 99, 99, 99],
         [0.75, 99, 99, 99, 99, 1e13]]
WY = [0, 1 << 19, 1 << 20, 1 << 19]               # row weights 0, 1/2, 1, 1/2


def _word(value, p, is_max=False):
    bits = int(np.float32(value).view(np.uint32))
    k = bits ^ 0xFFFFFFFF if bits >> 31 else bits | 0x80000000
    return uf.signed((k << 32) | ((0xFFFFFFFF - p) if is_max else p))


def _hand_case(cap=4):
    mask = np.asarray([MASK], np.uint8)
    fields = np.asarray([FIELD], np.float32)[..., None]
    _, cx, sx = dnn.event_weight_tables(4, 6)
    return uf.field_table(mask, 1, 4, True, np.asarray(WY, np.int32), cx, sx, cap, fields, 1, [1])


def test_checker_by_hand():
    ftable, cat = _hand_case()
    assert [int(r[0]) for r in cat[3][0]] == [0, 5, 18] and [int(r[2]) for r in cat[3][0]] == [3, 2, 2]
    assert ftable.shape == (1, 4, 1, 6) and ftable.dtype == np.int64
    # A: minimum -3 at pixel 1; 1.25 twice, at pixels 0 and 7: the maximum names pixel 0.  q = rint(2.5) = 2 (ties to even), -6, 2: sum -2.
    # Row 0 weighs nothing; (1,1): rint(2.5 * 0.5) = rint(1.25) = 1
    assert ftable[0, 0, 0].tolist() == [_word(-3.0, 1), _word(1.25, 0, True), -2, 1, 0, 0]
    # B: NaN counts and does nothing else; -0.0 at pixel 11 is both extremes, and adds nothing
    assert ftable[0, 1, 0].tolist() == [_word(-0.0, 11), _word(-0.0, 11, True), 0, 0, 1, 0]
    # C: 1e13 * 2 is beyond 2^40: an extreme, not a summand.  0.75: q = rint(1.5) = 2, weighted rint(0.75) = 1
    assert ftable[0, 2, 0].tolist() == [_word(0.75, 18), _word(1e13, 23, True), 2, 1, 0, 1]
    assert ftable[0, 3, 0].tolist() == list(uf.EMPTY_ROW)
    # the words as written out: key(-3.0) = ~0xC0400000, key(1.25) = 0x3FA00000 | 0x80000000
    assert _word(-3.0, 1) == (0x3FBFFFFF << 32) | 1 and _word(1.25, 0, True) == uf.signed((0xBFA00000 << 32) | 0xFFFFFFFF)
    # a table of two rows: C has no row
    short, _ = _hand_case(cap=2)
    assert np.array_equal(short[0], ftable[0, :2])


def test_keys_keep_the_order_and_come_back():
    tiny = np.float32(1e-45)                                                 # the smallest denormal
    big = np.finfo(np.float32).max
    ordered = np.asarray([-big, -1.5, -np.finfo(np.float32).tiny, -tiny, -0.0, 0.0, tiny, np.finfo(np.float32).tiny, 1.5, big], np.float32)
    keys = dnn.event_field_key(ordered)
    assert keys.dtype == np.uint32 and bool((np.diff(keys.astype(np.int64)) > 0).all())        # -0.0 below +0.0, denormals in place
    assert int(keys.min()) > 0                                               # no finite value has key 0: a max word of 0 means "empty"
    back = dnn.event_field_value(keys)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), ordered.view(np.uint32))
    assert [uf.key(v) for v in ordered] == keys.tolist() and [uf.unkey(k).view(np.uint32) for k in keys.tolist()] == ordered.view(np.uint32).tolist()
    rs = np.random.RandomState(5)
    v = (rs.standard_normal(4000) * np.exp(rs.uniform(-60, 60, 4000))).astype(np.float32)
    k = dnn.event_field_key(v)
    order = np.argsort(v, kind="stable")
    assert bool((np.diff(k[order].astype(np.int64)) >= 0).all())
    assert bool(((np.diff(k[order].astype(np.int64)) == 0) == (np.diff(v[order]) == 0)).all())
    assert np.array_equal(dnn.event_field_value(k).view(np.uint32), v.view(np.uint32))


def test_ties_name_the_smallest_pixel():
    mask = np.ones((1, 3, 5), np.uint8)
    fields = np.full((1, 3, 5, 2), 7.0, np.float32)
    fields[0, :, :, 1] = [[2, 9, 9, 1, 2], [1, 9, 2, 2, 1], [9, 1, 2, 2, 2]]
    wy, cx, sx = dnn.event_weight_tables(3, 5)
    ftable, cat = uf.field_table(mask, 1, 8, False, wy, cx, sx, 2, fields, 2, [3, 3])
    dec = dnn.EventFields.decode(ftable[0, :1], cat[3][0], 3, 5, [3, 3])[0]
    assert (dec[0]["min"], dec[0]["min_row"], dec[0]["min_col"], dec[0]["max"], dec[0]["max_row"], dec[0]["max_col"]) == (7.0, 0, 0, 7.0, 0, 0)
    assert (dec[1]["min"], dec[1]["min_row"], dec[1]["min_col"]) == (1.0, 0, 3)               # 1 at pixels 3, 5, 9, 11
    assert (dec[1]["max"], dec[1]["max_row"], dec[1]["max_col"]) == (9.0, 0, 1)               # 9 at pixels 1, 2, 6, 10
    assert dec[0]["mean"] == 7.0 and dec[1]["mean"] == 54 / 15


def test_event_field_bits():
    b = dnn.event_field_bits([-1e5, 0.25, -3e-7], [2.0, 1.0, 1e-7])
    assert b.dtype == np.int32 and b.tolist() == [22, 38, 60]
    assert dnn.event_field_bits([0.0, -INF, NAN, -5.0], [0.0, 1.0, 1.0, INF]).tolist() == [0, 0, 0, 0]
    assert dnn.event_field_bits(-1.0, 1.0).tolist() == [38]
    # inside the range |q| < 2^39, up to twice outside it still at most 2^40, eight times outside beyond it
    for m in (1e5, 1.0, 3e-7, 1e-30, 3e38):
        bits = int(dnn.event_field_bits(-m, m / 2)[0])
        assert abs(np.ldexp(np.float64(np.float32(m)), bits)) < 2.0 ** 39
        assert abs(np.ldexp(np.float64(np.float32(m)) * 2, bits)) <= uf.LIMIT < abs(np.ldexp(np.float64(np.float32(m)) * 8, bits))


def test_decode_hand_built_rows():
    H, W = 5, 8
    lat, lon = np.linspace(-90, 90, H), np.linspace(-180, 180, W)
    wy = dnn.event_weight_tables(H, W)[0]
    bits = [2, 0]
    # an event of 4 pixels across the seam: (1, 0), (1, 7), (2, 0), (2, 7); the second row stays empty (beyond the events)
    area = 2 * int(wy[1]) + 2 * int(wy[2])
    rows = np.asarray([[8, 2, 4, area, 6, 0, 0, 1, 2, 1]], np.int64)
    fr = np.asarray([[[_word(-1.5, 15), _word(2.25, 8, True), 12, 7, 0, 0],              # sum = (-1.5 + 0.5 + 1.75 + 2.25) * 4
                      [-1, 0, 0, 0, 3, 1]]], np.int64)                                   # no finite value that fits: three NaN, one saturated
    dec = dnn.EventFields.decode(fr, rows, H, W, bits)
    assert len(dec) == 1 and len(dec[0]) == 2
    d = dec[0][0]
    assert (d["min"], d["min_row"], d["min_col"], d["min_lat"], d["min_lon"]) == (-1.5, 1, 7, lat[1], lon[7])
    assert (d["max"], d["max_row"], d["max_col"], d["max_lat"], d["max_lon"]) == (2.25, 1, 0, lat[1], lon[0])
    assert d["mean"] == 0.75 and d["area_mean"] == 7 / (4 * (area * 2.0 ** -20)) and (d["nonfinite"], d["saturated"]) == (0, 0)
    e = dec[0][1]
    assert all(e[k] is None for k in ("min", "min_row", "min_col", "min_lat", "min_lon", "max", "max_row", "max_col", "max_lat", "max_lon"))
    assert e["mean"] is None and e["area_mean"] == 0.0 and (e["nonfinite"], e["saturated"]) == (3, 1)
    # an event on the pole rows only has no area: no area-weighted mean
    rows0 = np.asarray([[0, 1, 2, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    assert dnn.EventFields.decode(fr[:, :1], rows0, H, W, bits)[0][0]["area_mean"] is None
    assert dnn.EventFields.decode(fr[:0], rows[:0], H, W, bits) == []
    # the checker's rows decode to the hand case's values
    ftable, cat = _hand_case()
    dec = dnn.EventFields.decode(ftable[0, :3], cat[3][0], 4, 6, [1])
    assert [(e[0]["min"], e[0]["max"]) for e in dec] == [(-3.0, 1.25), (0.0, 0.0), (0.75, float(np.float32(1e13)))]
    assert [e[0]["mean"] for e in dec] == [-1 / 3, 0.0, 1.0] and str(dec[1][0]["min"]) == "-0.0"
    # the array form: decode's numbers to the bit, NaN for None
    assert dnn.EventFields.FIELD_VALUES == uf.VALUES
    vals = dnn.EventFields.values(ftable[0, :3], cat[3][0], 4, 6, [1])
    assert vals.shape == (3, 1, 8) and vals.dtype == np.float64 and vals[0, 0, 0] == -3.0 and vals[2, 0, 6] == 1.0
    assert np.array_equal(vals, uf.values_from_decode(dec, 1), equal_nan=True) and np.signbit(vals[1, 0, 0])
    both = dnn.EventFields.values(fr, rows, H, W, bits)
    assert np.isnan(both[0, 1, :7]).all() and both[0, 1, 7] == 0.0
    assert np.array_equal(both, uf.values_from_decode(dnn.EventFields.decode(fr, rows, H, W, bits), 2), equal_nan=True)
    assert dnn.EventFields.values(fr[:0], rows[:0], H, W, bits).shape == (0, 2, 8)


def test_values_equal_decode_on_random_fields():
    rs = np.random.RandomState(3)
    H, W, C_ = 9, 14, 3
    mask = ((rs.rand(1, H, W) < 0.5) * rs.randint(1, 3, (1, H, W))).astype(np.uint8)
    fields = (rs.standard_normal((1, H, W, C_)) * [1e-6, 3.0, 1e5]).astype(np.float32)
    fields[0, :, :7, 0] = np.nan                                             # events without a finite value in channel 0
    fields[0, 2, :, 2] = 9e5                                                 # beyond twice the range: saturated
    bits = dnn.event_field_bits([-1e-6, -3.0, -1e5], [1e-6, 3.0, 1e5])
    ftable, cat = uf.field_table(mask, 1, 8, True, *dnn.event_weight_tables(H, W), 64, fields, C_, bits)
    rows = cat[3][0]
    fr = ftable[0, :len(rows)]
    assert len(rows) > 3 and fr[..., 4].sum() > 0 and fr[..., 5].sum() > 0 and (fr[..., 0] == -1).any()
    dec = dnn.EventFields.decode(fr, rows, H, W, bits)
    assert np.array_equal(dnn.EventFields.values(fr, rows, H, W, bits), uf.values_from_decode(dec, C_), equal_nan=True)
    # a mean is within half a quantum per value of the float64 mean of the values it stands for
    lab = cat[0][0]
    for k, r in enumerate(rows):
        v = fields[0][lab == int(r[0]) + 1][:, 1].astype(np.float64)
        assert abs(dec[k][1]["mean"] - v.mean()) <= 2.0 ** -(int(bits[1]) + 1) + 1e-15


def test_host_entry_point_and_argument_checks_without_a_device():
    lib = L.load()
    n = C.c_int()
    assert lib.dc_component_fields_lds_slots(C.byref(n)) == 0 and 1 <= n.value <= 2048
    assert lib.dc_component_fields_lds_slots(None) != 0
    fake = C.c_void_p(4096)                                                  # never dereferenced: the checks come before any launch
    cf = lambda **kw: lib.dc_component_fields(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("nv", 2), ("H", 8), ("W", 8), ("labels", fake), ("rank", fake), ("cap", 4), ("fields", fake), ("C", 16), ("ldc", 16),
        ("bits", fake), ("wy", fake), ("ftable", fake), ("st", None))])
    assert cf(C=0) != 0 and "C must lie in [1, 32]" in L.last_error()
    assert cf(C=33, ldc=40) != 0 and "C must lie in [1, 32]" in L.last_error()
    assert cf(C=5, ldc=4) != 0 and "ldc" in L.last_error()
    assert cf(cap=0) != 0 and "cap" in L.last_error()
    assert cf(nv=0) != 0 and "n_valid" in L.last_error()
    assert cf(nv=3) != 0
    assert cf(H=2048, W=2049, labels=None, rank=None, fields=None, ftable=None) != 0 and "2^22" in L.last_error()   # sizes before pointers
    assert cf(H=2048, W=2048, wy=None) != 0 and "null" in L.last_error()     # exactly 2^22 pixels pass the size check
    assert cf(ftable=C.c_void_p(4104)) != 0 and "aligned" in L.last_error()


def test_header_bindings_and_vocabulary_agree():
    hdr = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("dc_component_fields", "dc_component_fields_lds_slots"):
        assert re.search(r"\b" + name + r"\s*\(", code) and name in L.EXPORTS and hasattr(L.load(), name)
    assert len(L._SIGS["dc_component_fields"][1]) == 14
    doc = hdr[hdr.index("Launch record"):hdr.index("int dc_launch_log_begin")]
    assert "cc_fields" in doc
    assert dnn.EVENT_FIELD_STATS == ("min", "max", "sum", "wsum", "nonfinite", "saturated") and uf.STATS == len(dnn.EVENT_FIELD_STATS)


def test_driver_event_fields_implies_events():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.event_fields is False and a.events is False
    a = predict.build_parser().parse_args(base + ["--event_fields"])
    assert a.event_fields is True and a.events is True and a.verify is False
    a = predict.build_parser().parse_args(base + ["--verify", "--event_fields", "--min_event_pixels", "20"])
    assert a.event_fields is True and a.events is True and a.verify is True and a.min_event_pixels == 20
    a = predict.build_parser().parse_args(base + ["--events"])
    assert a.event_fields is False and a.events is True


def test_event_fields_refuses_bad_arguments_before_any_launch():
    class Cat:                                                               # what the constructor looks at before it allocates
        B, H, W, cap = 1, 4096, 2048, 4
    for kw in ({"channels": 0, "bits": []}, {"channels": 33, "bits": [0] * 33}, {"channels": 4, "bits": [0] * 4, "ldc": 3},
               {"channels": 4, "bits": [0] * 3}, {"channels": 2, "bits": [0, 0]}):
        with pytest.raises(L.DeepcamHipError):
            dnn.EventFields(Cat(), **kw)
