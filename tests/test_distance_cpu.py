"""The distance-map verification's host side (no GPU): the checker of tests/util_distance.py on hand-made cases, nn.distance_table against
math.isqrt and float64, nn.DistanceSkill.decode on hand-made totals, the three entry points in the header, the binding table and the
thunks, the host-only entry points and the argument checks of the C ABI, every constructor argument that is refused, the driver's flags
and summary, and the conditions the GPU test's inputs must satisfy (tests/test_distance_gpu.py takes its masks from the same functions)."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_distance as ud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_distance_block", "dc_distance_workspace", "dc_distance_score")
B, NV = ud.B, ud.NV
DECODE, TABLE, FROM_ROWS = dnn.DistanceSkill.decode, dnn.distance_table, dnn.distance_from_rows   # the whole file is about these


block, shape, standard_batch, plain_batch, reference_maps, reference = (ud.block, ud.shape, ud.standard_batch, ud.plain_batch,
                                                                        ud.reference_maps, ud.reference)


# ------------------------------------------------------------------------------------------------------------------ hand-made cases
def _one_pixel_each(H, W, p, t, R, wrap, k=1):
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int64)
    pred[p], truth[t] = k, k
    return ud.frame_rows(pred, truth, R, wrap)


def test_one_pixel_per_side_at_a_known_offset():
    R = 10
    rows, bad = _one_pixel_each(31, 41, (12, 20), (15, 24), R, True)          # offset (3, 4): d = 5 exactly
    for d in range(2):
        cells = rows[0, d]
        assert cells[5] == 1 and cells[:R + 2].sum() == 1 and cells[R + 2] == 5 * 256 and cells[R + 3] == 25
    assert not rows[1].any() and bad[1] == 0 and bad[0] > 0
    rows, _ = _one_pixel_each(31, 41, (12, 20), (13, 21), R, True, k=2)       # offset (1, 1): d^2 = 2, ring 2, dq = rint(sqrt 2 * 256) = 362
    assert rows[1, 0, 2] == 1 and rows[1, 0, R + 2] == 362 and rows[1, 0, R + 3] == 2 and not rows[0].any()
    rows, bad = _one_pixel_each(31, 41, (12, 20), (12, 20), R, True)          # the same pixel: ring 0 is |P and T|, Baddeley 0
    assert rows[0, 0, 0] == rows[0, 1, 0] == 1 and rows[0, :, R + 2:].sum() == 0 and bad[0] == 0


def test_across_the_seam_with_wrap_and_without():
    R, H, W = 6, 9, 40
    rows, _ = _one_pixel_each(H, W, (4, W - 2), (4, 1), R, True)              # three columns apart across the seam
    assert rows[0, 0, 3] == 1 and rows[0, 1, 3] == 1 and rows[0, 0, R + 3] == 9
    rows, _ = _one_pixel_each(H, W, (4, W - 2), (4, 1), R, False)             # 37 columns apart: beyond
    assert rows[0, 0, R + 1] == 1 and rows[0, 1, R + 1] == 1 and rows[0, :, R + 2:].sum() == 0
    maps = ud.frame_maps(*[np.pad(np.ones((1, 1), np.uint8), ((4, 4), (0, W - 1)))] * 2, R, True)
    assert maps[0, 0, 4, W - 1] == 1 and maps[0, 0, 4, W - 6] == 36 and maps[0, 0, 4, W - 7] == R * R + 1
    assert ud.frame_maps(*[np.pad(np.ones((1, 1), np.uint8), ((4, 4), (0, W - 1)))] * 2, R, False)[0, 0, 4, W - 1] == R * R + 1


def test_rows_are_never_periodic():
    R, H, W = 5, 8, 21
    for wrap in (True, False):
        rows, _ = _one_pixel_each(H, W, (0, 10), (H - 1, 10), R, wrap)        # seven rows apart, one if rows wrapped
        assert rows[0, 0, R + 1] == 1 and rows[0, 1, R + 1] == 1 and rows[0, :, :R + 1].sum() == 0


def test_the_cap_is_inclusive_at_r_squared():
    R = 5
    rows, _ = _one_pixel_each(21, 31, (10, 10), (13, 14), R, True)            # (3, 4): d^2 = 25 = R^2, within
    assert rows[0, 0, R] == 1 and rows[0, 0, R + 1] == 0 and rows[0, 0, R + 3] == 25 and rows[0, 0, R + 2] == 5 * 256
    rows, _ = _one_pixel_each(21, 31, (10, 10), (15, 11), R, True)            # (5, 1): d^2 = 26 = R^2 + 1, beyond although |dy|, |dx| <= R
    assert rows[0, 0, R] == 0 and rows[0, 0, R + 1] == 1 and rows[0, 0, R + 2] == 0 and rows[0, 0, R + 3] == 0
    maps = ud.frame_maps(np.pad(np.ones((1, 1), np.uint8), ((10, 10), (10, 20))), np.zeros((21, 31), np.uint8), R, True)
    assert maps[0, 0, 15, 10] == 25 and maps[0, 0, 15, 11] == 26 and maps[0, 0, 16, 10] == 26 and maps.max() == 26
    assert (maps[0, 1] == 26).all() and (maps[1] == 26).all()                 # no pixel of the class: beyond everywhere


def test_only_the_full_width_values_are_classes_and_the_band_selects_sources():
    R, H, W = 4, 10, 15
    pred = np.zeros((H, W), np.int64)
    truth = np.zeros((H, W), np.int64)
    pred[2, 3], pred[2, 5], pred[3, 3], pred[4, 4] = 257, (1 << 32) + 1, -1, 1
    truth[8, 4], truth[5, 5], truth[1, 1] = 1, 258, 3
    rows, bad = ud.frame_rows(pred, truth, R, True)
    assert rows[0, 0, 4] == 1 and rows[0, 1, 4] == 1 and rows[0, :, :R + 2].sum() == 2 and not rows[1].any()
    band_rows, band_bad = ud.frame_rows(pred, truth, R, True, (0, 6))         # the labelled pixel lies outside the band, the target still counts
    assert band_rows[0, 0].sum() == 0 and band_rows[0, 1, 4] == 1 and 0 < band_bad[0] < bad[0]


def test_distance_table_against_isqrt_and_float64():
    for R in (1, 2, 5, 64, 127):
        t = dnn.distance_table(R)
        assert t.dtype == np.int32 and t.shape == (R * R + 2,)
        ring, dq = ud.table(R)
        assert np.array_equal(t & 0xFF, ring) and np.array_equal(t >> 8, dq)
        for v in {0, 1, min(2, R * R), R * R - 1, R * R}:
            j = math.isqrt(v)
            assert (t[v] & 0xFF) == (j if j * j == v else j + 1) and (t[v] >> 8) == int(np.rint(np.sqrt(np.float64(v)) * 256))
        assert t[R * R] == (R | (256 * R) << 8) and t[R * R + 1] == R + 1     # the cap itself; beyond: ring R + 1, dq 0
    assert dnn.distance_table(127).max() < 1 << 24
    for bad in (0, 128, -1):
        with pytest.raises(L.DeepcamHipError):
            dnn.distance_table(bad)


def test_decode_of_hand_made_totals():
    R, H, W = 3, 10, 10
    #              ring 0  1  2  3  beyond  sum dq            sum d^2
    total = [[[6, 2, 1, 1, 0, 256 * 2 + 512 + 768, 2 + 4 + 9],                 # class 1 miss: 10 labelled pixels, none beyond
              [6, 0, 3, 0, 1, 3 * 500, 3 * 4]],                                # class 1 false alarm: 10 predicted, one beyond
             [[0] * 7, [0, 0, 0, 0, 4, 0, 0]]]                                 # class 2: no labelled pixel, four predicted ones, all beyond
    bad = [4 * 256 * 256 * 50, 0]
    out = dnn.DistanceSkill.decode(total, bad, frames=2, radius=R, height=H, width=W, row_range=(2, 7))
    assert out == ud.decode(total, bad, 2, R, H, W, (2, 7))
    c1, c2 = out["class_1"], out["class_2"]
    assert c1["pixels"] == {"labelled": 10, "predicted": 10}
    assert c1["pod_within"] == [0.6, 0.8, 0.9, 1.0] and c1["success_within"] == [0.6, 0.6, 0.9, 0.9]
    assert c1["med_miss"] == (256 * 2 + 512 + 768) / 256 / 10 and c1["med_false_alarm"] == 1500 / 256 / 9
    assert c1["rms_miss"] == math.sqrt(15 / 10) and c1["rms_false_alarm"] == math.sqrt(12 / 9)
    assert c1["beyond_miss"] == 0.0 and c1["beyond_false_alarm"] == 0.1
    assert c1["hausdorff"] is None                                              # a source beyond the cap: the distance is not known
    assert c1["hausdorff_q90"] == 2                                             # miss: 9 of 10 within ring 2; false alarm: 9 of 10 within ring 2
    assert c1["baddeley"] == math.sqrt(4 * 256 * 256 * 50 / (2 * 5 * 10)) / 256
    assert c2["pixels"] == {"labelled": 0, "predicted": 4} and c2["pod_within"] == [None] * 4 and c2["success_within"] == [0.0] * 4
    assert c2["med_miss"] is None and c2["med_false_alarm"] is None and c2["rms_false_alarm"] is None and c2["beyond_miss"] is None
    assert c2["beyond_false_alarm"] == 1.0 and c2["hausdorff"] is None and c2["hausdorff_q90"] is None and c2["baddeley"] == 0.0
    total[0][1] = [6, 0, 3, 1, 0, 3 * 500 + 768, 3 * 4 + 9]                    # nothing beyond any more: the largest ring over both directions
    out = dnn.DistanceSkill.decode(total, bad, 2, R, H, W)
    assert out["class_1"]["hausdorff"] == 3 and out["class_1"]["hausdorff_q90"] == 2
    assert out["class_1"]["baddeley"] == math.sqrt(4 * 256 * 256 * 50 / 200) / 256
    none = dnn.DistanceSkill.decode([[[0] * 7] * 2] * 2, [0, 0], 0, R, H, W)    # nothing yet
    assert all(none[c][key] is None for c in none for key in ("med_miss", "rms_miss", "beyond_miss", "hausdorff", "hausdorff_q90", "baddeley"))
    with pytest.raises(L.DeepcamHipError):
        dnn.DistanceSkill.decode([[[0] * 6] * 2] * 2, [0, 0], 1, R, H, W)
    assert json.loads(json.dumps(out)) == out
    single = dnn.distance_from_rows(np.asarray([total, total]), np.asarray([bad, [0, 0]]), R, H, W)
    assert single[0] == dnn.DistanceSkill.decode(total, bad, 1, R, H, W) and single[1]["class_1"]["baddeley"] == 0.0
    with pytest.raises(L.DeepcamHipError):
        dnn.distance_from_rows(np.zeros((2, 2, 7), np.int64), np.zeros((2,), np.int64), R, H, W)


def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_distance", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert "int dc_distance_block(" in header and "size_t dc_distance_workspace(" in header and "int dc_distance_score(" in header
    for name in ("dc_distance_block", "dc_distance_score"):
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_distance_score"][1]) == 21 and L._SIGS["dc_distance_workspace"][0] is C.c_size_t
    for word in ("dist_vert", "dist_horz", "dist_total"):
        assert word in header.split("int dc_launch_log_begin")[0]
    source = open(os.path.join(L.CSRC, "distance.hip")).read()
    assert all(f'DC_LAUNCHED("{w}")' in source for w in ("dist_vert", "dist_horz", "dist_total"))
    assert "distance.hip" in open(os.path.join(L.CSRC, "Makefile")).read()
    assert "ring(v) | dq(v) << 8" in header                                     # the table's packing is documented


def test_block_workspace_and_argument_checks_without_a_device():
    lib = L.load()
    TC, TR = block()
    rows = C.c_int(0)
    assert lib.dc_distance_block(None, C.byref(rows)) != 0 and "null" in L.last_error()
    ws = lib.dc_distance_workspace
    assert ws(8, 768, 1152, 64) == 8 * 768 * 1152 * 4 and ws(1, 1, 1, 1) == 4   # one packed word per pixel
    for bad in ((0, 8, 8, 1), (4096, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 8, 128), (1, 1 << 16, 1 << 15, 1), (-1, 8, 8, 1)):
        assert ws(*bad) == 0, bad
    fake = C.c_void_p(4096)                                                     # never dereferenced: the checks come before any launch
    score = lambda **kw: lib.dc_distance_score(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("n_valid", 2), ("H", 8), ("W", 12), ("pred", fake), ("pred_bytes", 1), ("truth", fake), ("truth_bytes", 8), ("R", 3),
        ("table", fake), ("wrap", 1), ("row0", 0), ("row1", 8), ("rows", fake), ("baddeley", fake), ("total", fake), ("total_baddeley", fake),
        ("frames", fake), ("maps", None), ("workspace", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert score(B=0) != 0 and score(B=4096) != 0 and score(H=0) != 0 and score(W=0) != 0 and "positive" in L.last_error()
        assert score(H=1 << 16, W=1 << 15, row1=1) != 0 and "2^31" in L.last_error()
        assert score(n_valid=-1) != 0 and score(n_valid=3) != 0 and "n_valid" in L.last_error()
        for side in ("pred_bytes", "truth_bytes"):
            for b in (0, 2, 3, 16):
                assert score(**{side: b}) != 0 and "mask_bytes" in L.last_error()
        assert score(R=0) != 0 and score(R=128) != 0 and score(R=-1) != 0 and "radius" in L.last_error()
        assert score(wrap=2) != 0 and score(wrap=-1) != 0 and "wrap must" in L.last_error()
        assert score(R=6) != 0 and "wider than the frame" in L.last_error()     # 2 R + 1 = 13 > W = 12 under wrap
        for r0, r1 in ((-1, 8), (0, 9), (4, 4), (5, 4), (8, 8)):
            assert score(row0=r0, row1=r1) != 0 and "row range" in L.last_error()
        for name in ("pred", "truth", "table", "rows", "baddeley", "total", "total_baddeley", "frames", "workspace"):
            assert score(**{name: None}) != 0 and "null" in L.last_error(), name
        assert score(truth=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert score(pred_bytes=4, pred=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        for name in ("table", "rows", "baddeley", "total", "total_baddeley", "frames", "workspace"):
            assert score(**{name: C.c_void_p(4098)}) != 0 and "aligned" in L.last_error(), name
        assert score(maps=C.c_void_p(4097)) != 0 and "aligned" in L.last_error()
        assert score(n_valid=0) == 0 and score(n_valid=0, R=6, wrap=0) == 0     # nothing valid: accepted, and nothing is launched
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                                                     # nothing was launched
    assert TC >= 64 and TR >= 2


def test_rejected_constructor_arguments():
    ok = {"radius": 3, "device": "cpu"}
    for kw in ({"radius": 0}, {"radius": 128}, {"radius": -2}, {"radius": 6}, {"row_range": (4, 4)}, {"row_range": (0, 9)}, {"row_range": (-1, 4)},
               {"row_range": (5, 2)}):
        with pytest.raises(L.DeepcamHipError):
            dnn.DistanceSkill(2, 8, 12, **{**ok, **kw})
    for dims in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, 1 << 15), (1, 0, 12), (1, 8, 0)):
        with pytest.raises(L.DeepcamHipError):
            dnn.DistanceSkill(*dims, **ok)
    with pytest.raises(L.DeepcamHipError) as e:                                 # 2 R + 1 = 13 > 12 is refused for what it is ...
        dnn.DistanceSkill(2, 8, 12, radius=6, wrap=True, device="cpu")
    assert "wider than the frame" in str(e.value)
    d = dnn.DistanceSkill(2, 8, 12, radius=6, wrap=False, row_range=(1, 7), device="cpu")    # ... and accepted without wrap
    assert (d.R, d.wrap, d.row_range, d.keep_maps) == (6, False, (1, 7), False)
    with pytest.raises(L.DeepcamHipError):
        d.maps()                                                                # without keep_maps
    assert d.frame_rows()[0].shape == (0, 2, 2, 10) and d.frame_rows()[1].shape == (0, 2)
    assert d.state() == {"total": [[[0] * 10] * 2] * 2, "baddeley": [0, 0], "frames": 0}


def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False
    assert not [k for k in vars(a) if k.startswith("distance")]                 # flags that were not given leave no attribute behind
    assert predict.DISTANCE_DEFAULTS == {"distance_skill": False, "distance_radius": 64, "distance_rows": None, "distance_no_wrap": False}
    assert predict.distance_options(a) == {"radius": 64, "wrap": True, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--distance_skill"])
    assert a.distance_skill is True and a.verify is True and a.events is True   # the labels are needed: the flag implies --verify
    assert predict.distance_options(a) == {"radius": 64, "wrap": True, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--distance_skill", "--distance_radius", "20", "--distance_rows", "256", "512", "--distance_no_wrap"])
    assert a.distance_radius == 20 and a.distance_rows == [256, 512] and a.distance_no_wrap is True
    assert predict.distance_options(a) == {"radius": 20, "wrap": False, "row_range": (256, 512)}
    a = predict.build_parser().parse_args(base + ["--distance_radius", "3"])    # the options parse without the switch and are ignored
    assert not hasattr(a, "distance_skill") and a.verify is False and a.distance_radius == 3
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(base + ["--distance_skill", "--distance_rows", "3"])
    assert "distance-map verification" in predict.build_parser().format_help()


def test_driver_summary_entry_on_checker_output():
    from mlperf_deepcam_amd import predict
    H, W, R = shape("small")
    pred, truth = plain_batch("small")
    band = (2, H - 3)
    state = ud.totals([(pred[:2], truth[:2]), (pred[2:3], truth[2:3])], R, True, band)
    s = predict.distance_summary(R, True, band, H, W, state)
    ref = ud.decode(state["total"], state["baddeley"], 3, R, H, W, band)
    assert s["radius"] == R and s["wrap"] is True and s["rows"] == list(band) and s["frames"] == 3
    for k in (1, 2):
        entry = dict(s[f"class_{k}"])
        assert entry.pop("total") == state["total"][k - 1] and entry.pop("total_baddeley") == state["baddeley"][k - 1]
        assert entry == ref[f"class_{k}"] and entry["med_miss"] > 0 and entry["baddeley"] > 0
        assert entry["pod_within"] == sorted(entry["pod_within"]) and 0 < entry["pod_within"][0] < entry["pod_within"][-1] <= 1.0
    assert json.loads(json.dumps(s)) == s


# ------------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
@pytest.mark.parametrize("name", ["small", "large", "large-r5"])
def test_the_gpu_inputs_are_sparse_and_touch_the_edges(name):
    H, W, R = shape(name)
    TC, TR = block()
    if name == "small":
        assert W % 2 == 1 and W < TC and H < TR and 2 * R + 1 == W
    else:
        assert 2 * TC < W < 3 * TC and 2 * TR < H < 3 * TR and (R == 5 or R == min(127, TR + 2)) and 2 * R + 1 <= W
    for which, (pred, truth) in enumerate((standard_batch(name), plain_batch(name))):
        fg = ((pred == 1) | (pred == 2) | (truth == 1) | (truth == 2))[:NV]
        assert 0 < fg.mean() < (0.15 if name == "small" else 0.01)              # sparse
        assert (truth == 3).any() and (truth == 255).any() and (pred == 3).any() and (pred == 255).any()
        for m in (pred[0], truth[0]) if which else (truth[0],):                 # (the standard batch's first prediction lost its class 1)
            cls = (m == 1) | (m == 2)
            assert cls[0].any() and cls[H - 1].any() and cls[:, 0].any() and cls[:, W - 1].any()
    pred, truth = standard_batch(name)
    assert not (pred[0] == 1).any() and (truth[0] == 1).any()                   # class 1 absent from the prediction only
    assert not (pred[1] == 1).any() and not (truth[1] == 1).any()               # ... from both sides
    assert (pred[2] == 1).all() and (truth[2] == 1).all()                       # the padding frame
    rows, bad, _ = reference(name, True)
    n1 = int((truth[0] == 1).sum())
    assert rows[0, 0, 0, R + 1] == n1 and rows[0, 0, 0].sum() == n1 and not rows[0, 0, 1].any() and bad[0, 0] > 0
    assert not rows[1, 0].any() and bad[1, 0] == 0 and rows[:, 1, :, :R + 2].sum(axis=2).all()


@pytest.mark.parametrize("name", ["large", "large-r5"])
def test_the_large_inputs_fill_the_far_rings_the_beyond_cell_and_the_seam(name):
    """Every class and direction has a non-empty ring above R / 2 and a non-empty beyond cell -- in every frame of the plain batch, and for
    class 2 in the standard batch, whose class 1 is removed from the prediction on purpose --, and some source's nearest target lies across
    the seam: the rows with wrap and without differ."""
    H, W, R = shape(name)
    rows, _, _ = reference(name, True, None, "plain")
    flat, _, _ = reference(name, False, None, "plain")
    assert (rows[:, :, :, R // 2 + 1:R + 1].sum(axis=3) > 0).all() and (rows[:, :, :, R + 1] > 0).all()
    assert (rows[:, :, :, 0] > 0).all() and (rows[:, :, 0, 0] == rows[:, :, 1, 0]).all()     # ring 0 of both directions is |P and T|
    assert all(not np.array_equal(rows[b, k, d], flat[b, k, d]) for b in range(len(rows)) for k in range(2) for d in range(2))
    std, _, _ = reference(name, True)
    std_flat, _, _ = reference(name, False)
    assert (std[:, 1, :, R // 2 + 1:R + 1].sum(axis=2) > 0).all() and (std[:, 1, :, R + 1] > 0).all()
    assert not np.array_equal(std, std_flat)
    maps, maps_flat = reference_maps(name, True, "plain"), reference_maps(name, False, "plain")
    pred, truth = plain_batch(name)
    for k in (1, 2):                                                            # the labelled speck in column 2: three columns from W - 1
        ys = np.flatnonzero(truth[0][:, 2] == k)
        assert any(maps[0, 0, k - 1, y, 2] == 9 and maps_flat[0, 0, k - 1, y, 2] > 9 for y in ys)
