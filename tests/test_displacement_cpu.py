"""The displacement verification's host side (no GPU): the two checker algorithms of tests/util_displacement.py on hand-made cases and
against each other, nn.DisplacementSkill.decode on hand-made totals, the symmetry and the bounds of the table, the entry points in the
header, the binding table and the thunks, the host-only entry points and the argument checks of the C ABI, every constructor argument that
is refused, the driver's flags and summary, and the conditions the GPU test's inputs must satisfy (tests/test_displacement_gpu.py takes its
masks from the same functions)."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_displacement as ud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_displacement_block", "dc_displacement_workspace", "dc_displacement_score")
KERNELS = ("disp_pack", "disp_corr", "disp_best", "disp_total")
DECODE, FROM_ROWS = dnn.DisplacementSkill.decode, dnn.displacement_from_rows                      # the whole file is about these


def _both(pred, truth, R, band=None):
    """the table by both algorithms, which must agree"""
    a, b = ud.table_by_pairs(pred, truth, R, band), ud.table_by_shifts(pred, truth, R, band)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return a


# ------------------------------------------------------------------------------------------------------------------ hand-made cases
def test_one_pixel_per_side_at_a_known_offset():
    H, W, R = 12, 20, 5
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int64)
    pred[4, 9], truth[7, 5] = 1, 1                    # the label lies 3 rows on and 4 columns back
    rows, pixels = _both(pred, truth, R)
    assert rows[0, :, :2 * R + 1].sum() == 1 and rows[0, 3 + R, -4 + R] == 1 and not rows[1].any()
    assert ud.best_of(rows[0], R) == (3, -4, 1, 1) and dnn.displacement_best(rows[0], R) == (3, -4, 1, 1)
    assert pixels.tolist() == [[1, 1], [0, 0]]
    assert ud.best_of(rows[1], R) == (0, 0, 0, 0)     # a table without hits
    d = DECODE(rows.tolist(), pixels.tolist(), 1, R, H, W)["class_1"]
    assert d["shift"]["rows"] == 3 and d["shift"]["cols"] == -4 and d["shift"]["pixels"] == 5.0 and d["at_edge"] is False
    assert d["shift"]["lat_deg"] == 3 * 180.0 / (H - 1) and d["shift"]["lon_deg"] == -4 * 360.0 / (W - 1)
    assert d["csi"] == {"unshifted": 0.0, "shifted": 1.0} and d["share"] == {"displacement": 1.0, "volume": 0.0, "pattern": 0.0}


def test_a_pair_across_the_seam():
    H, W, R = 6, 15, 3
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    pred[2, W - 1], truth[2, 1] = 2, 2                # two columns on, over the seam
    rows, _ = _both(pred, truth, R)
    assert ud.best_of(rows[1], R) == (0, 2, 1, 1) and rows[1, :, :2 * R + 1].sum() == 1
    assert ud.seam_hits(pred, truth, 2, 0, 2) == 1
    pred[:], truth[:] = 0, 0
    pred[2, 0], truth[2, W - 2] = 2, 2                # and two columns back
    assert ud.best_of(_both(pred, truth, R)[0][1], R) == (0, -2, 1, 1)


def test_rows_are_never_periodic():
    H, W, R = 9, 11, 5
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    pred[0, 4], truth[H - 1, 4] = 1, 1                # R < H - 1: out of reach, and never over the pole
    rows, pixels = _both(pred, truth, R)
    assert not rows[0, :, :2 * R + 1].any() and ud.best_of(rows[0], R) == (0, 0, 0, 1)
    d = DECODE(rows.tolist(), pixels.tolist(), 1, R, H, W)
    assert d["class_1"]["csi"] == {"unshifted": 0.0, "shifted": 0.0} and d["class_1"]["shift"]["pixels"] == 0.0
    assert d["class_2"]["csi"] == {"unshifted": None, "shifted": None} and d["class_2"]["pod"]["shifted"] is None
    assert d["class_2"]["far"]["unshifted"] is None and d["class_2"]["share"]["displacement"] is None


def test_pixels_moved_over_a_pole_are_lost():
    H, W, R = 10, 13, 4
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    pred[1, 3:6], pred[6, 3:6], truth[5, 3:6] = 1, 1, 1
    rows, _ = _both(pred, truth, R)
    kept = rows[0, :, 2 * R + 1]
    assert kept[R] == 6 and kept[R - 2] == 3 and kept[R - 1] == 6 and kept[R + 4] == 3            # dy = -2 loses row 1, dy = 4 row 6
    assert (kept <= kept[R]).all()
    band = (4, 8)                                     # a band: row 1 enters it at dy >= 3, row 6 leaves it at dy >= 2
    kept = _both(pred, truth, R, band)[0][0, :, 2 * R + 1]
    assert kept[R] == 3 and kept[R + 3] == 3 and kept[R + 2] == 0 and kept[R - 3] == 0 and kept[R - 2] == 3


def test_the_tie_goes_to_the_smaller_dx():
    H, W, R = 5, 9, 2
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    truth[2, 4], pred[2, 3], pred[2, 5] = 1, 1, 1
    rows, _ = _both(pred, truth, R)
    assert rows[0, R, R - 1] == rows[0, R, R + 1] == 1 and ud.maxima_of(rows[0], R) == 2
    assert ud.best_of(rows[0], R) == (0, -1, 1, 2) == dnn.displacement_best(rows[0], R)
    pred[:] = 0
    pred[1, 4], pred[3, 4] = 1, 1                     # the same across rows: the smaller dy
    assert ud.best_of(_both(pred, truth, R)[0][0], R)[:2] == (-1, 0)
    pred[2, 5] = 1                                    # (0, -1) has the same length: the smaller dy still
    assert ud.best_of(_both(pred, truth, R)[0][0], R)[:2] == (-1, 0)


def test_a_planted_displacement_is_recovered():
    H, W, R = 40, 90, 8
    truth = np.zeros((H, W), np.uint8)
    ud.ellipse(truth, 14, 2, 3, 7, 1)                 # on the seam
    ud.ellipse(truth, 27, 50, 2, 9, 1)
    ud.ellipse(truth, 20, 30, 4, 4, 2)
    for dy, dx in ((3, -6), (-2, 8), (0, 1)):
        pred = np.zeros_like(truth)
        for k in (1, 2):
            pred[ud.moved(truth == k, -dy, -dx)] = k
        ud.ellipse(pred, 5, 70, 1, 3, 1)              # a false alarm
        rows, pixels = ud.table_by_pairs(pred, truth, R)
        for k in (1, 2):
            best = ud.best_of(rows[k - 1], R)
            assert best[:2] == (dy, dx) and best[2] == (truth == k).sum() and ud.maxima_of(rows[k - 1], R) == 1
        d = DECODE(rows.tolist(), pixels.tolist(), 1, R, H, W)
        assert d["class_2"]["csi"]["shifted"] == 1.0 and d["class_2"]["mse_shifted"] == 0.0 and d["class_2"]["share"]["displacement"] == 1.0
        assert d["class_1"]["csi"]["shifted"] > d["class_1"]["csi"]["unshifted"] and d["class_1"]["at_edge"] is (dx == 8)
    assert ud.seam_hits(pred, truth, 1, 0, 1) > 0


@pytest.mark.parametrize("name", ud.SHAPES)
def test_the_two_algorithms_agree_on_the_test_shapes(name):
    H, W, R = ud.shape(name)
    pred, truth = ud.standard_batch(name)
    frames = (0, 1, 2) if R <= 18 else (0,)            # R = 40: 6561 shifts of the whole frame, one frame and two bands are enough
    for band_name, band in ud.bands(name).items():
        if R > 18 and band_name in ("interior", "top"):
            continue
        for f in frames:
            a, b = ud.table_by_pairs(pred[f], truth[f], R, band), ud.table_by_shifts(pred[f], truth[f], R, band)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, band_name, f)
    dp, dt = ud.dense_frames(1, H, W, 5)
    if H * W < 4096:                                  # a dense frame's pair list grows with the square of its pixels
        a, b = ud.table_by_pairs(dp[0], dt[0], R), ud.table_by_shifts(dp[0], dt[0], R)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ properties
def test_swapping_the_sides_mirrors_the_table_on_the_full_band():
    for name in ("small", "word"):
        H, W, R = ud.shape(name)
        pred, truth, _ = ud.plain_batch(name)
        S = 2 * R + 1
        for f in (0, 1):
            a, pa = ud.table_by_pairs(pred[f], truth[f], R)
            b, pb = ud.table_by_pairs(truth[f], pred[f], R)
            assert np.array_equal(a[:, :, :S], b[:, ::-1, S - 1::-1]) and a[:, :, :S].any()      # hits[dy][dx] = swapped hits[-dy][-dx]
            assert np.array_equal(pa, pb[:, ::-1])


@pytest.mark.parametrize("name", ud.SHAPES)
def test_hits_are_bounded_by_kept_and_labelled(name):
    R = ud.shape(name)[2]
    S = 2 * R + 1
    for band in ud.bands(name):
        rows, pixels, best, _ = ud.reference(name, band)
        assert (rows[:, :, :, :S] <= rows[:, :, :, S:]).all() and (rows[:, :, :, :S] <= pixels[:, :, None, None, 1]).all()
        assert (rows[:, :, :, S] <= pixels[:, :, None, 0]).all()                # kept never exceeds the predicted pixels
        assert (best[:, :, 2] == rows[:, :, :, :S].max(axis=(2, 3))).all()


# ------------------------------------------------------------------------------------------------------------------ decode
def test_decode_of_hand_made_totals():
    R, H, W, band, frames = 2, 10, 20, (2, 8), 3
    S = 2 * R + 1
    total = np.zeros((2, S, S + 1), np.int64)
    total[0, :, S] = (50, 58, 60, 60, 55)             # kept per dy
    total[0, R, R] = 12                               # unshifted
    total[0, R + 1, R - 2] = 40                       # the best shift (1, -2): at the edge in dx
    total[0, R + 1, R + 1] = 39
    total[1, :, S] = 7                                # class 2: predicted but no label
    pixels = [[64, 48], [7, 0]]
    d = DECODE(total.tolist(), pixels, frames, R, H, W, band)
    c = d["class_1"]
    N = frames * 6 * W
    assert c["best"] == [1, -2, 40, 60] and c["at_edge"] is True and c["hits_unshifted"] == 12 and c["hits_shifted"] == 40
    assert c["pixels"] == {"predicted": 64, "labelled": 48}
    assert c["shift"] == {"rows": 1, "cols": -2, "pixels": math.sqrt(5.0), "lat_deg": 180.0 / 9, "lon_deg": -2 * 360.0 / 19}
    assert c["csi"] == {"unshifted": 12 / (60 + 48 - 12), "shifted": 40 / (60 + 48 - 40)}
    assert c["pod"] == {"unshifted": 12 / 48, "shifted": 40 / 48} and c["far"] == {"unshifted": 48 / 60, "shifted": 20 / 60}
    assert c["mse_total"] == (60 + 48 - 24) / N and c["mse_shifted"] == (60 + 48 - 80) / N and c["mse_volume"] == (12 / N) ** 2
    parts = [c["mse_displacement"], c["mse_volume"], c["mse_pattern"]]
    assert all(p >= 0 for p in parts) and math.isclose(sum(parts), c["mse_total"], rel_tol=1e-15)
    assert math.isclose(sum(c["share"].values()), 1.0, rel_tol=1e-15)
    e = d["class_2"]
    assert e["best"] == [0, 0, 0, 7] and e["at_edge"] is False and e["csi"] == {"unshifted": 0.0, "shifted": 0.0}
    assert e["pod"] == {"unshifted": None, "shifted": None} and e["far"] == {"unshifted": 1.0, "shifted": 1.0}
    assert e["mse_displacement"] == 0.0 and e["mse_total"] == 7 / N
    assert d == ud.decode(total.tolist(), pixels, frames, R, H, W, band)
    assert json.loads(json.dumps(d)) == d
    surface = DECODE(total.tolist(), pixels, frames, R, H, W, band, surface=True)
    want = ud.csi_surface(total[0], 48, R)
    got = surface["class_1"]["csi_surface"]
    assert got.dtype == np.float64 and got.shape == (S, S) and np.array_equal(got, want) and got[R + 1, R - 2] == c["csi"]["shifted"]
    empty = DECODE(np.zeros((2, S, S + 1), np.int64).tolist(), [[0, 0], [0, 0]], 0, R, H, W, surface=True)["class_1"]
    assert empty["mse_total"] is None and empty["share"]["volume"] is None and np.isnan(empty["csi_surface"]).all()
    with pytest.raises(L.DeepcamHipError):
        DECODE(total[:, :, :S].tolist(), pixels, frames, R, H, W)
    with pytest.raises(L.DeepcamHipError):
        FROM_ROWS(np.zeros((2, 2, S, S), np.int64), np.zeros((2, 2, 2), np.int64), R, H, W)


@pytest.mark.parametrize("name", ["small", "word", "large-r5"])
def test_decode_and_from_rows_against_the_checker(name):
    H, W, R = ud.shape(name)
    for band_name in ("full", "one-row"):
        band = ud.bands(name)[band_name]
        rows, pixels, best, state = ud.reference(name, band_name, "plain")
        got = DECODE(state["total"], state["pixels"], state["frames"], R, H, W, band)
        assert got == ud.decode(state["total"], state["pixels"], state["frames"], R, H, W, band)
        for k in (1, 2):
            c = got[f"class_{k}"]
            if c["mse_total"]:
                assert c["mse_volume"] >= 0 and c["mse_pattern"] >= 0
                # on the full band kept[dy] <= kept[0]: the shift cannot add predicted pixels, only hits; into a band it can carry some
                assert band is not None or c["mse_displacement"] >= 0
        singles = FROM_ROWS(rows, pixels, R, H, W, band)
        assert singles == [ud.decode(rows[b].tolist(), pixels[b].tolist(), 1, R, H, W, band) for b in range(len(rows))]
        assert [[s[f"class_{k}"]["best"] for k in (1, 2)] for s in singles] == best.tolist()


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_displacement", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert "int dc_displacement_block(" in header and "size_t dc_displacement_workspace(" in header and "int dc_displacement_score(" in header
    for name in ("dc_displacement_block", "dc_displacement_score"):
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_displacement_score"][1]) == 19 and L._SIGS["dc_displacement_workspace"][0] is C.c_size_t
    source = open(os.path.join(L.CSRC, "displacement.hip")).read()
    for word in KERNELS:
        assert word in header.split("int dc_launch_log_begin")[0] and f'DC_LAUNCHED("{word}")' in source
    assert "displacement.hip" in open(os.path.join(L.CSRC, "Makefile")).read()
    assert "hits << 27 | (8191 - (dy^2 + dx^2)) << 14" in header                # the key is documented


def test_block_workspace_and_argument_checks_without_a_device():
    lib = L.load()
    bits, seg = ud.block()
    assert bits == 64 and seg >= 2                    # a word is a wave's ballot
    rows = C.c_int(0)
    assert lib.dc_displacement_block(None, C.byref(rows)) != 0 and "null" in L.last_error()
    ws = lib.dc_displacement_workspace
    assert ws(8, 768, 1152, 16) == 8 * 2 * 768 * ((18 + 20) * 8 + 4) and ws(1, 1, 3, 1) == 2 * ((1 + 2) * 8 + 4)
    assert 0 < ws(8, 768, 1152, 63) < 8 << 20         # a few MB at batch 8
    for bad in ((0, 8, 8, 1), (4096, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 200, 64), (1, 8, 8, 4), (1, 1 << 16, 1 << 15, 1),
                (-1, 8, 8, 1)):
        assert ws(*bad) == 0, bad
    fake = C.c_void_p(4096)                                                     # never dereferenced: the checks come before any launch
    score = lambda **kw: lib.dc_displacement_score(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("n_valid", 2), ("H", 8), ("W", 12), ("pred", fake), ("pred_bytes", 1), ("truth", fake), ("truth_bytes", 8), ("R", 3),
        ("row0", 0), ("row1", 8), ("rows", fake), ("pixels", fake), ("best", fake), ("total", fake), ("total_pixels", fake), ("frames", fake),
        ("workspace", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert score(B=0) != 0 and score(B=4096) != 0 and score(H=0) != 0 and score(W=0) != 0 and "positive" in L.last_error()
        assert score(H=1 << 16, W=1 << 15, row1=1) != 0 and "2^31" in L.last_error()
        assert score(n_valid=-1) != 0 and score(n_valid=3) != 0 and "n_valid" in L.last_error()
        for side in ("pred_bytes", "truth_bytes"):
            for b in (0, 2, 3, 16):
                assert score(**{side: b}) != 0 and "mask_bytes" in L.last_error()
        assert score(R=0) != 0 and score(R=64, W=200) != 0 and score(R=-1) != 0 and "radius" in L.last_error()
        assert score(R=6) != 0 and "wider than the frame" in L.last_error()     # 2 R + 1 = 13 > W = 12
        for r0, r1 in ((-1, 8), (0, 9), (4, 4), (5, 4), (8, 8)):
            assert score(row0=r0, row1=r1) != 0 and "row range" in L.last_error()
        for name in ("pred", "truth", "rows", "pixels", "best", "total", "total_pixels", "frames", "workspace"):
            assert score(**{name: None}) != 0 and "null" in L.last_error(), name
        assert score(truth=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert score(pred_bytes=4, pred=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        for name in ("rows", "pixels", "best", "total", "total_pixels", "frames", "workspace"):
            assert score(**{name: C.c_void_p(4100)}) != 0 and "aligned" in L.last_error(), name
        assert score(n_valid=0) == 0                                            # nothing valid: accepted, and nothing is launched
        assert score(n_valid=0, R=6) != 0                                       # ... but still checked
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                                                     # nothing was launched


def test_rejected_constructor_arguments():
    ok = {"radius": 3, "device": "cpu"}
    for kw in ({"radius": 0}, {"radius": 64}, {"radius": -2}, {"radius": 6}, {"row_range": (4, 4)}, {"row_range": (0, 9)}, {"row_range": (-1, 4)},
               {"row_range": (5, 2)}):
        with pytest.raises(L.DeepcamHipError):
            dnn.DisplacementSkill(2, 8, 12, **{**ok, **kw})
    for dims in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, 1 << 15), (1, 0, 12), (1, 8, 0)):
        with pytest.raises(L.DeepcamHipError):
            dnn.DisplacementSkill(*dims, **ok)
    with pytest.raises(L.DeepcamHipError) as e:
        dnn.DisplacementSkill(2, 8, 12, radius=6, device="cpu")
    assert "wider than the frame" in str(e.value)
    assert dnn.DISPLACEMENT_RADIUS == 16 and dnn.DISPLACEMENT_MAX_RADIUS == 63
    d = dnn.DisplacementSkill(2, 8, 13, radius=6, row_range=(1, 7), device="cpu")
    assert (d.R, d.row_range) == (6, (1, 7))
    rows, pixels, best = d.frame_rows()
    assert rows.shape == (0, 2, 13, 14) and pixels.shape == (0, 2, 2) and best.shape == (0, 2, 4)
    assert d.state() == {"total": [[[0] * 14] * 13] * 2, "pixels": [[0, 0], [0, 0]], "frames": 0}
    for bad in (lambda: d(np.zeros((2, 8, 13), np.uint8), None), lambda: d(None, None, n_valid=1)):
        with pytest.raises(L.DeepcamHipError):
            bad()


# ------------------------------------------------------------------------------------------------------------------ the driver
def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False
    assert not [k for k in vars(a) if k.startswith("displacement")]             # flags that were not given leave no attribute behind
    assert predict.DISPLACEMENT_DEFAULTS == {"displacement": False, "displacement_radius": 16, "displacement_rows": None}
    assert predict.displacement_options(a) == {"radius": 16, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--displacement"])
    assert a.displacement is True and a.verify is True and a.events is True     # the labels are needed: the flag implies --verify
    assert predict.displacement_options(a) == {"radius": 16, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--displacement", "--displacement_radius", "20", "--displacement_rows", "256", "512"])
    assert a.displacement_radius == 20 and a.displacement_rows == [256, 512]
    assert predict.displacement_options(a) == {"radius": 20, "row_range": (256, 512)}
    a = predict.build_parser().parse_args(base + ["--displacement_radius", "3"])    # the options parse without the switch and are ignored
    assert not hasattr(a, "displacement") and a.verify is False and a.displacement_radius == 3
    for bad in (["--displacement_rows", "3"], ["--displacement_radius", "x"], ["--displacement_radius"], ["--displacement", "1"]):
        with pytest.raises(SystemExit):
            predict.build_parser().parse_args(base + ["--displacement"] + bad)
    assert "displacement verification" in predict.build_parser().format_help()


def test_driver_summary_entry_on_checker_output():
    from mlperf_deepcam_amd import predict
    H, W, R = ud.shape("small")
    band = ud.bands("small")["interior"]
    rows, pixels, best, state = ud.reference("small", "interior", "plain")
    s = predict.displacement_summary(R, band, H, W, state, best)
    ref = ud.decode(state["total"], state["pixels"], len(rows), R, H, W, band)
    assert s["radius"] == R and s["rows"] == list(band) and s["frames"] == len(rows) == 7
    for k in (1, 2):
        entry = dict(s[f"class_{k}"])
        shifts = entry.pop("frame_shifts")
        have = best[best[:, k - 1, 2] > 0, k - 1]
        assert shifts["frames"] == len(have) > 0
        assert math.isclose(shifts["mean_rows"], sum(int(v) for v in have[:, 0]) / len(have), rel_tol=1e-12, abs_tol=1e-12)
        assert math.isclose(shifts["mean_cols"], sum(int(v) for v in have[:, 1]) / len(have), rel_tol=1e-12, abs_tol=1e-12)
        assert math.isclose(shifts["mean_pixels"], sum(math.hypot(int(a), int(b)) for a, b in have[:, :2]) / len(have), rel_tol=1e-12)
        assert entry == ref[f"class_{k}"] and entry["best"] == list(ud.best_of(state["total"][k - 1], R))
    assert json.loads(json.dumps(s)) == s
    none = predict.displacement_summary(R, band, H, W, ud.totals_of_rows([], R), np.zeros((0, 2, 4), np.int64))
    assert none["frames"] == 0 and none["class_1"]["frame_shifts"] == {"frames": 0, "mean_rows": None, "mean_cols": None, "mean_pixels": None}


# ------------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
@pytest.mark.parametrize("name", ud.SHAPES)
def test_the_gpu_inputs_meet_their_conditions(name):
    H, W, R = ud.shape(name)
    assert ud.shape("small") == (23, 37, 18) and ud.shape("word") == (19, 128, 7) and ud.shape("large") == (141, 549, 40) and \
        ud.shape("large-r5") == (141, 549, 5)
    pred, truth, planted = ud.plain_batch(name)
    rows, pixels, best, _ = ud.reference(name, "full", "plain")
    assert len(pred) == 7
    share = [(m == k).mean() for m in (pred, truth) for k in (1, 2)]
    assert all(0.01 < s < 0.06 for s in share), share                           # sparse: the checker's pair lists stay short
    seam = lost = 0
    for f in range(len(pred)):
        for k in (1, 2):
            dy, dx, hits, kept = (int(v) for v in best[f, k - 1])
            assert (dy, dx) != (0, 0) and hits > 0, (f, k)                      # every class of the plain frames has a non-zero best shift
            assert ud.maxima_of(rows[f, k - 1], R) == 1, (f, k)                 # ... which no other shift equals
            assert (dy, dx) == planted[f][k - 1], (f, k)                        # ... the planted one
            seam += ud.seam_hits(pred[f], truth[f], k, dy, dx) > 0
            lost += bool((rows[f, k - 1, :, 2 * R + 1] < rows[f, k - 1, R, 2 * R + 1]).any())
    assert seam > 0 and lost > 0                                                # hits across the seam; pixels lost over a pole
    # the standard batch: the tie, and a class absent on one side
    spred, struth = ud.standard_batch(name)
    srows, spixels, sbest, _ = ud.reference(name, "full")
    assert len(spred) == ud.B == 4 and len(srows) == ud.NV == 3 and (spred[3] == 1).all() and (struth[3] == 1).all()
    assert sbest[1, 0].tolist() == [0, -1, 1, 2] and ud.maxima_of(srows[1, 0], R) == 2 and spixels[1, 0].tolist() == [2, 1]
    assert spixels[2, 1, 0] == 0 and spixels[2, 1, 1] > 0 and not srows[2, 1].any() and sbest[2, 1].tolist() == [0, 0, 0, 0]
    for band in ("interior", "top", "one-row"):                                 # every band holds labels and hits
        brows, bpixels, _, _ = ud.reference(name, band, "plain")
        assert bpixels[:, :, 1].sum() > 0 and brows[:, :, :, :2 * R + 1].any(), band
        assert not np.array_equal(brows, rows)
