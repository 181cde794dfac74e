"""The scale-separation verification's host side (no GPU): the two checker algorithms of tests/util_scale.py against each other and on
hand-made cases, the explicit Haar energies, nn.ScaleSkill.decode on hand-made totals and against the checker's exact decode, the entry
points in the header, the binding table and the thunks, the host-only entry points and the argument checks of the C ABI, every constructor
argument that is refused, the driver's flags and summary, and the conditions the GPU test's inputs must satisfy
(tests/test_scale_gpu.py takes its masks from the same functions)."""
import ctypes as C
import importlib.util
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_scale as us

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_scale_block", "dc_scale_workspace", "dc_scale_score")
KERNELS = ("scale_sums", "scale_coarse", "scale_total")
DECODE, FROM_ROWS = dnn.ScaleSkill.decode, dnn.scale_from_rows                  # the whole file is about these


def _both(pred, truth, levels, origins=(0,), band=None):
    """the rows by both algorithms, which must agree"""
    a, b = us.rows_by_blocks(pred, truth, levels, origins, band), us.rows_by_transform(pred, truth, levels, origins, band)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return a


# ------------------------------------------------------------------------------------------------------------------ hand-made cases
def test_one_mismatched_pixel():
    H, W, n = 16, 32, 3
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int64)
    pred[5, 9] = 1
    rows, pixels = _both(pred, truth, n, (0, 3))
    assert (rows[0, :, :, 0] == 1).all() and (rows[0, :, :, 1] == 1).all() and not rows[0, :, :, 2].any() and not rows[1].any()
    assert pixels.tolist() == [[1, 0], [0, 0]]
    e = us.components([int(v) for v in rows[0, 0, :, 0]])
    assert e == [Fraction(3, 4 ** (j + 1)) for j in range(n)] + [Fraction(1, 4 ** n)] and sum(e) == 1
    assert e == us.haar_energies((pred == 1).astype(np.int64) - (truth == 1), 0, n)
    d = DECODE(rows.tolist(), pixels.tolist(), 1, n, H, W, (0, 3))["class_1"]
    assert d["mse"] == [float(Fraction(3, 4 ** (j + 1)) / (H * W)) for j in range(n)] + [float(Fraction(1, 4 ** n) / (H * W))]
    assert d["mse_share"] == [3 / 4 ** (j + 1) for j in range(n)] + [1 / 4 ** n] and d["origin_spread"] == [0.0] * (n + 1)
    assert d["energy_truth"] == [0.0] * (n + 1) and d["energy_rel_diff"] == [1.0] * (n + 1) and d["bias"] is None


def test_a_constant_field_has_all_its_energy_in_the_father():
    H, W, n = 8, 24, 3
    pred, truth = np.full((H, W), 2, np.uint8), np.zeros((H, W), np.uint8)
    rows, pixels = _both(pred, truth, n, (0, 5))
    q = [int(v) for v in rows[1, 1, :, 1]]
    assert q == [H * W * 4 ** j for j in range(n + 1)]
    assert us.components(q) == [0] * n + [H * W] == us.haar_energies((pred == 2).astype(np.int64), 5, n)
    d = DECODE(rows.tolist(), pixels.tolist(), 1, n, H, W)["class_2"]
    assert d["mse"] == [0.0] * n + [1.0] and d["energy_pred"] == [0.0] * n + [1.0] and d["mse_random"] == 1.0
    assert d["skill"] == [1.0] * n + [1.0 - (n + 1)] and d["skilful_scale"] == 1


def test_a_checkerboard_has_all_its_energy_in_component_0():
    H, W, n = 8, 16, 2
    y, x = np.mgrid[0:H, 0:W]
    pred, truth = ((y + x) % 2).astype(np.uint8), np.zeros((H, W), np.uint8)
    for origins in ((0,), (1,), (0, 1, 2, 3)):
        rows, _ = _both(pred, truth, n, origins)
        for o in range(len(origins)):
            e = us.components([int(v) for v in rows[0, o, :, 1]])
            # every 2 x 2 block holds two pixels: the detail of level 0 carries +-1/2 per pixel, the block means are flat
            assert e == [Fraction(H * W, 4), 0, Fraction(H * W, 4)]
    assert us.haar_energies((pred == 1).astype(np.int64), 1, n) == [Fraction(H * W, 4), 0, Fraction(H * W, 4)]


@pytest.mark.parametrize("m", [1, 2, 3])
def test_an_aligned_square_and_the_same_square_off_the_grid(m):
    H, W, n = 32, 64, 4
    side = 1 << m
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    pred[8:8 + side, 16:16 + side] = 1
    rows, _ = _both(pred, truth, n, (0,))
    assert [int(v) for v in rows[0, 0, :, 1]] == [4 ** (m + j) if j <= m else 16 ** m for j in range(n + 1)]
    moved = np.roll(pred, 3, axis=1)                  # the same square moved by an odd origin: the grid of origin 3 sees it aligned
    got, _ = _both(moved, truth, n, (0, 3))
    assert np.array_equal(got[:, 1], rows[:, 0]) and not np.array_equal(got[:, 0], rows[:, 0])
    assert got[0, 0, 0, 1] == rows[0, 0, 0, 1] == side * side                  # level 0 never depends on the origin
    over = np.roll(pred, -17, axis=1)                 # across the seam: columns 63, 0, ...
    assert over[8, W - 1] == 1 and over[8, 0] == 1
    got, _ = _both(over, truth, n, (W - 17 - 16 * ((W - 17) // 16),))           # the origin that puts the square back on the grid
    assert np.array_equal(got[:, 0], rows[:, 0])


@pytest.mark.parametrize("name,band", us.CASES)
def test_the_two_algorithms_agree_on_the_test_shapes(name, band):
    H, W, n, origins = us.shape(name)
    pred, truth = us.standard_batch(name)
    frames = (0, 1, 2) if H * W <= 40000 else (2,)
    for f in frames:
        a = us.rows_by_blocks(pred[f], truth[f], n, origins, us.SHAPES[name][4][band])
        b = us.rows_by_transform(pred[f], truth[f], n, origins, us.SHAPES[name][4][band])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, band, f)


def test_the_components_are_the_explicit_transform_and_sum_to_the_error():
    H, W, n, origins = us.shape("two-tiles")
    pred, truth = us.standard_batch("two-tiles")
    r0, r1 = us.band_of("two-tiles", "band")
    rows, pixels, _ = us.reference("two-tiles", "band")
    for k in (1, 2):
        err = (pred[0, r0:r1] == k).astype(np.int64) - (truth[0, r0:r1] == k)
        for i, c in enumerate(origins):
            e = us.components([int(v) for v in rows[0, k - 1, i, :, 0]])
            assert e == us.haar_energies(err, c, n) and all(x >= 0 for x in e) and sum(e) == int((err != 0).sum()) == rows[0, k - 1, i, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ decode
def test_decode_of_hand_made_totals():
    n, rows_in_band, W, frames = 2, 8, 16, 3
    N = frames * rows_in_band * W
    # class 1, two origins: (A, B, C) per level; level 0 is the same for both
    total = [[[[20, 30, 26], [44, 90, 70], [100, 300, 200]], [[20, 30, 26], [40, 100, 66], [96, 340, 180]]],
             [[[0, 0, 0]] * 3, [[0, 0, 0]] * 3]]
    pixels = [[30, 26], [0, 0]]
    d = DECODE(total, pixels, frames, n, rows_in_band, W, (0, 2))
    c = d["class_1"]
    e0 = [Fraction(4 * 20 - 44, 4), Fraction(4 * 44 - 100, 16), Fraction(100, 16)]
    e1 = [Fraction(4 * 20 - 40, 4), Fraction(4 * 40 - 96, 16), Fraction(96, 16)]
    assert sum(e0) == sum(e1) == 20
    assert c["by_origin"][0]["origin"] == 0 and c["by_origin"][1]["origin"] == 2
    assert c["by_origin"][0]["mse"] == [float(x / N) for x in e0] and c["by_origin"][1]["mse"] == [float(x / N) for x in e1]
    assert c["mse"] == [float((a + b) / 2 / N) for a, b in zip(e0, e1)]
    assert c["mse_share"] == [float((a + b) / 2 / 20) for a, b in zip(e0, e1)]
    assert c["origin_spread"] == [float(abs(a - b) / N) for a, b in zip(e0, e1)]
    p, o = Fraction(30, N), Fraction(26, N)
    rnd = p * (1 - o) + o * (1 - p)
    assert c["mse_random"] == float(rnd) and c["base_rate"] == 26 / N and c["bias"] == 30 / 26 and c["scales"] == [1, 2, 4]
    assert c["skill"] == [float(1 - (a + b) / 2 / N * 3 / rnd) for a, b in zip(e0, e1)]
    assert c["pixels"] == {"predicted": 30, "labelled": 26}
    ep = [Fraction(4 * 30 - 90, 4), Fraction(4 * 90 - 300, 16), Fraction(300, 16)]
    et = [Fraction(4 * 26 - 70, 4), Fraction(4 * 70 - 200, 16), Fraction(200, 16)]
    assert c["by_origin"][0]["energy_pred"] == [float(x / N) for x in ep] and c["by_origin"][0]["energy_truth"] == [float(x / N) for x in et]
    assert c["by_origin"][0]["energy_rel_diff"] == [float((a - b) / (a + b)) for a, b in zip(ep, et)]
    sk = [1 - (a + b) / 2 / N * 3 / rnd for a, b in zip(e0, e1)]
    want = None
    for j in (1, 0):
        if sk[j] <= 0:
            break
        want = 1 << j
    assert c["skilful_scale"] == want
    z = d["class_2"]
    assert z["mse"] == [0.0] * 3 and z["mse_share"] == [None] * 3 and z["skill"] == [None] * 3 and z["energy_rel_diff"] == [None] * 3
    assert z["bias"] is None and z["base_rate"] == 0.0 and z["mse_random"] == 0.0 and z["skilful_scale"] is None
    assert d == us.decode(total, pixels, frames, n, rows_in_band, W, (0, 2))
    assert json.loads(json.dumps(d)) == d
    empty = DECODE(np.zeros((2, 1, 3, 3), np.int64).tolist(), [[0, 0], [0, 0]], 0, n, rows_in_band, W)["class_1"]
    assert empty["mse"] == [None] * 3 and empty["base_rate"] is None and empty["origin_spread"] == [None] * 3 and empty["by_origin"][0]["origin"] == 0
    with pytest.raises(L.DeepcamHipError):
        DECODE(total, pixels, frames, 3, rows_in_band, W)
    with pytest.raises(L.DeepcamHipError):
        DECODE(total, pixels, frames, n, rows_in_band, W, (0,))
    with pytest.raises(L.DeepcamHipError):
        FROM_ROWS(np.zeros((2, 2, 1, 3, 2), np.int64), np.zeros((2, 2, 2), np.int64), 2, 8, 16)


def test_skilful_scale_is_the_smallest_scale_from_which_every_detail_has_skill():
    n, R, W = 3, 8, 8
    # B and C do not matter here; A chosen so that the skills of the components 0 .. 2 are (-, +, +), (+, -, +) and (+, +, +)
    def total_of(e):                                  # A_j from the components: Q_j / 4^j = sum of E_i for i >= j
        q = [int(sum(e[j:]) * 4 ** j) for j in range(n + 1)]
        return [[[[a, 0, 0] for a in q]], [[[0, 0, 0]] * (n + 1)]]
    pixels = [[16, 16], [0, 0]]
    rnd = Fraction(2 * 16 * 48, 64 * 64)              # 0.375: a component has skill below 0.375 * 64 / 4 = 6 pixels of error
    assert rnd == Fraction(3, 8)
    for e, want in (([8, 2, 2, 4], 2), ([2, 8, 2, 4], 4), ([2, 2, 2, 4], 1), ([2, 2, 8, 4], None), ([2, 2, 2, 40], 1)):
        d = DECODE(total_of(e), pixels, 1, n, R, W)["class_1"]
        assert d["skilful_scale"] == want, e
        assert d == us.decode(total_of(e), pixels, 1, n, R, W)["class_1"]


@pytest.mark.parametrize("name,band", us.CASES)
def test_decode_and_from_rows_against_the_checker(name, band):
    H, W, n, origins = us.shape(name)
    r0, r1 = us.band_of(name, band)
    rows, pixels, state = us.reference(name, band)
    got = DECODE(state["total"], state["pixels"], state["frames"], n, r1 - r0, W, origins)
    assert got == us.decode(state["total"], state["pixels"], state["frames"], n, r1 - r0, W, origins)
    N = state["frames"] * (r1 - r0) * W
    for k in (1, 2):
        for o in range(len(origins)):
            e = us.components([state["total"][k - 1][o][j][0] for j in range(n + 1)])
            assert sum(e) / N == Fraction(state["total"][k - 1][o][0][0], N)     # the components sum to the per-pixel error rate, exactly
    singles = FROM_ROWS(rows, pixels, n, r1 - r0, W, origins)
    assert singles == [us.decode(rows[b].tolist(), pixels[b].tolist(), 1, n, r1 - r0, W, origins) for b in range(len(rows))]


def test_scale_levels():
    assert dnn.scale_levels(768, 1152) == 7 and dnn.scale_levels(256, 512) == 8 and dnn.scale_levels(1024, 2048) == 8
    assert dnn.scale_levels(12, 20) == 2 and dnn.scale_levels(7, 64) == 0 and dnn.scale_levels(64, 6) == 1 and dnn.scale_levels(256, 384) == 7


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_scale", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert "int dc_scale_block(" in header and "size_t dc_scale_workspace(" in header and "int dc_scale_score(" in header
    for name in ("dc_scale_block", "dc_scale_score"):
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_scale_score"][1]) == 20 and L._SIGS["dc_scale_workspace"][0] is C.c_size_t
    source = open(os.path.join(L.CSRC, "scale.hip")).read()
    for word in KERNELS:
        assert word in header.split("int dc_launch_log_begin")[0] and f'DC_LAUNCHED("{word}")' in source
    assert "scale.hip" in open(os.path.join(L.CSRC, "Makefile")).read()
    assert "asm" not in source                        # plain HIP C++


def test_block_workspace_and_argument_checks_without_a_device():
    lib = L.load()
    assert us.block() == (64, 64)
    rows = C.c_int(0)
    assert lib.dc_scale_block(None, C.byref(rows)) != 0 and "null" in L.last_error()
    ws = lib.dc_scale_workspace
    assert ws(8, 768, 1152, 7, 1) == 8 * 12 * 18 * 16 and ws(8, 768, 1152, 7, 4) == 4 * 8 * 12 * 18 * 16 and ws(1, 12, 20, 2, 3) == 3 * 16
    for bad in ((0, 8, 8, 1, 1), (4096, 8, 8, 1, 1), (1, 0, 8, 1, 1), (1, 8, 0, 1, 1), (1, 8, 8, 0, 1), (1, 512, 512, 9, 1), (1, 8, 8, 1, 0),
                (1, 8, 8, 1, 9), (1, 8, 12, 3, 1), (1, 4, 8, 3, 1), (1, 1 << 16, 1 << 15, 1, 1), (-1, 8, 8, 1, 1)):
        assert ws(*bad) == 0, bad
    fake = C.c_void_p(4096)                                                     # never dereferenced: the checks come before any launch
    score = lambda **kw: lib.dc_scale_score(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("n_valid", 2), ("H", 8), ("W", 12), ("pred", fake), ("pred_bytes", 1), ("truth", fake), ("truth_bytes", 8), ("L", 2),
        ("O", 2), ("origins", fake), ("row0", 0), ("row1", 8), ("rows", fake), ("pixels", fake), ("total", fake), ("total_pixels", fake),
        ("frames", fake), ("workspace", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert score(B=0) != 0 and score(B=4096) != 0 and score(H=0) != 0 and score(W=0) != 0 and "positive" in L.last_error()
        assert score(H=1 << 16, W=1 << 15, row1=4) != 0 and "2^31" in L.last_error()
        assert score(n_valid=-1) != 0 and score(n_valid=3) != 0 and "n_valid" in L.last_error()
        for side in ("pred_bytes", "truth_bytes"):
            for b in (0, 2, 3, 16):
                assert score(**{side: b}) != 0 and "mask_bytes" in L.last_error()
        assert score(L=0) != 0 and score(L=9) != 0 and score(L=-1) != 0 and "levels" in L.last_error()
        assert score(O=0) != 0 and score(O=9) != 0 and "origins" in L.last_error()
        for r0, r1 in ((-1, 8), (0, 9), (4, 4), (5, 4), (8, 8)):
            assert score(row0=r0, row1=r1) != 0 and "row range" in L.last_error()
        assert score(L=3) != 0 and "divide" in L.last_error()                   # 8 does not divide W = 12
        assert score(row0=1, row1=7) != 0 and "divide" in L.last_error()        # 4 does not divide 6 rows
        assert score(row0=3, row1=7, n_valid=0) == 0                            # ... but a band may start at any row
        for name in ("pred", "truth", "origins", "rows", "pixels", "total", "total_pixels", "frames", "workspace"):
            assert score(**{name: None}) != 0 and "null" in L.last_error(), name
        assert score(truth=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert score(pred_bytes=4, pred=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        for name in ("rows", "pixels", "total", "total_pixels", "frames"):
            assert score(**{name: C.c_void_p(4100)}) != 0 and "aligned" in L.last_error(), name
        for name in ("origins", "workspace"):
            assert score(**{name: C.c_void_p(4098)}) != 0 and "aligned" in L.last_error(), name
        assert score(n_valid=0) == 0                                            # nothing valid: accepted, and nothing is launched
        assert score(n_valid=0, L=3) != 0                                       # ... but still checked
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                                                     # nothing was launched


def test_rejected_constructor_arguments():
    ok = {"levels": 2, "device": "cpu"}
    for kw in ({"levels": 0}, {"levels": 9}, {"levels": -1}, {"levels": 3}, {"row_range": (4, 4)}, {"row_range": (0, 9)}, {"row_range": (-1, 3)},
               {"row_range": (5, 2)}, {"row_range": (1, 7)}, {"origins": ()}, {"origins": (0,) * 9}, {"origins": (4,)}, {"origins": (-1,)},
               {"origins": (0, 7)}, {"origins": 1}):
        with pytest.raises(L.DeepcamHipError):
            dnn.ScaleSkill(2, 8, 12, **{**ok, **kw})
            pytest.fail(f"{kw} was accepted")
    for dims in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, 1 << 15), (1, 0, 12), (1, 8, 0)):
        with pytest.raises(L.DeepcamHipError):
            dnn.ScaleSkill(*dims, **ok)
    for kw, word in (({"levels": 3}, "divide"), ({"origins": (4,)}, "origin"), ({"levels": 9}, "levels"), ({"row_range": (0, 9)}, "row_range"),
                     ({"origins": ()}, "origins")):
        with pytest.raises(L.DeepcamHipError) as e:
            dnn.ScaleSkill(2, 8, 12, **{**ok, **kw})
        assert word in str(e.value)
    with pytest.raises(L.DeepcamHipError) as e:
        dnn.ScaleSkill(2, 7, 12, device="cpu")        # levels=None finds no level
    assert "even" in str(e.value)
    assert dnn.SCALE_MAX_LEVELS == 8 and dnn.SCALE_MAX_ORIGINS == 8
    d = dnn.ScaleSkill(2, 11, 12, origins=(0, 3), row_range=(3, 11), device="cpu")        # levels=None: 4 divides 8 rows and 12 columns
    assert (d.L, d.O, d.origins, d.row_range) == (2, 2, [0, 3], (3, 11))
    rows, pixels = d.frame_rows()
    assert rows.shape == (0, 2, 2, 3, 3) and pixels.shape == (0, 2, 2)
    assert d.state() == {"total": [[[[0] * 3] * 3] * 2] * 2, "pixels": [[0, 0], [0, 0]], "frames": 0}
    for bad in (lambda: d(np.zeros((2, 11, 12), np.uint8), None), lambda: d(None, None, n_valid=1)):
        with pytest.raises(L.DeepcamHipError):
            bad()


# ------------------------------------------------------------------------------------------------------------------ the driver
def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False
    assert not [k for k in vars(a) if k.startswith("scale")]                    # flags that were not given leave no attribute behind
    assert predict.SCALE_DEFAULTS == {"scale_skill": False, "scale_levels": None, "scale_rows": None, "scale_origins": (0,)}
    assert predict.scale_options(a) == {"levels": None, "row_range": None, "origins": (0,)}
    a = predict.build_parser().parse_args(base + ["--scale_skill"])
    assert a.scale_skill is True and a.verify is True and a.events is True      # the labels are needed: the flag implies --verify
    a = predict.build_parser().parse_args(base + ["--scale_skill", "--scale_levels", "5", "--scale_rows", "256", "512", "--scale_origins",
                                                  "0", "7", "16"])
    assert a.scale_levels == 5 and a.scale_rows == [256, 512] and a.scale_origins == [0, 7, 16]
    assert predict.scale_options(a) == {"levels": 5, "row_range": (256, 512), "origins": (0, 7, 16)}
    a = predict.build_parser().parse_args(base + ["--scale_levels", "3"])       # the options parse without the switch and are ignored
    assert not hasattr(a, "scale_skill") and a.verify is False and a.scale_levels == 3
    for bad in (["--scale_rows", "3"], ["--scale_levels", "x"], ["--scale_levels"], ["--scale_skill", "1"], ["--scale_origins"]):
        with pytest.raises(SystemExit):
            predict.build_parser().parse_args(base + ["--scale_skill"] + bad)
    assert "scale-separation verification" in predict.build_parser().format_help()


def test_driver_summary_entry_on_checker_output():
    from mlperf_deepcam_amd import predict
    H, W, n, origins = us.shape("two-tiles")
    band = us.band_of("two-tiles", "band")
    rows, pixels, state = us.reference("two-tiles", "band")
    s = predict.scale_summary(n, origins, band, W, state)
    ref = us.decode(state["total"], state["pixels"], us.NV, n, band[1] - band[0], W, origins)
    assert s["levels"] == n and s["origins"] == list(origins) and s["rows"] == list(band) and s["frames"] == us.NV
    assert s["class_1"] == ref["class_1"] and s["class_2"] == ref["class_2"]
    assert json.loads(json.dumps(s)) == s


# ------------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
def test_the_shapes_follow_from_the_workgroup_tile():
    tc, tr = us.block()
    want = {"partial": (12, 20, 2), "two-tiles": (40, 2 * tc + 8, 3), "tile": (tr, 3 * tc, 6), "coarse": (5 * tr, 6 * tc, 7), "deep": (4 * tr, 8 * tc, 8)}
    assert {name: us.shape(name)[:3] for name in us.SHAPES} == want
    assert us.SHAPES["two-tiles"][4] == {"full": None, "band": (8, 32)} and us.SHAPES["coarse"][4] == {"band": (37, 293)}
    assert us.SHAPES["deep"][3] == (0, 1, 63, 64, 255) and (1 << us.shape("tile")[2]) == tc
    r0, r1 = us.band_of("coarse", "band")
    assert r0 % 2 == 1 and (r1 - r0) % 128 == 0      # the band's start is aligned to nothing
    for name, (H, W, n, origins, bands) in us.SHAPES.items():
        for band in bands:
            r0, r1 = us.band_of(name, band)
            assert (r1 - r0) % (1 << n) == 0 and W % (1 << n) == 0 and all(0 <= c < (1 << n) for c in origins)


@pytest.mark.parametrize("name,band", us.CASES)
def test_the_gpu_inputs_meet_their_conditions(name, band):
    H, W, n, origins = us.shape(name)
    r0, r1 = us.band_of(name, band)
    pred, truth = us.standard_batch(name)
    rows, pixels, state = us.reference(name, band)
    assert len(pred) == us.B == 4 and len(rows) == us.NV == 3 and (pred[3] == 1).all() and (truth[3] == 1).all()
    assert (rows[0][:, :, :, 0] > 0).all() and (rows[2][0, :, :, 0] > 0).all()   # every class of the standard frame: error at every level
    assert (np.asarray(state["total"])[:, :, :, 0] > 0).all()
    assert pixels[1, 1, 0] == 0 and pixels[1, 1, 1] > 0 and pixels[1, 0, 1] == 0 and pixels[1, 0, 0] > 0        # a class absent on one side
    assert (rows[:, :, :, 0, 0] == rows[:, :, :1, 0, 0]).all() and (rows[:, :, :, 0, 1] == pixels[:, :, None, 0]).all() and \
        (rows[:, :, :, 0, 2] == pixels[:, :, None, 1]).all()                    # level 0: no origin, and B, C are the pixel counts
    assert len(origins) > 1 and any((rows[:, :, 0] != rows[:, :, o]).any() for o in range(1, len(origins)))      # origins differ somewhere
    # a block across the seam with pixels on both sides: frame 2, class 1, the coarsest level of an origin that is not 0
    c = [c for c in origins if c][0]
    T = 1 << n
    seam = (truth[2, r0:r1] == 1)
    first = W - T + c                                  # the block that starts at column W - T + c ends at column c - 1
    assert seam[:, first:].any() and seam[:, :c].any()


def test_the_full_frames_reach_both_traps():
    H, W, n, origins = us.shape("deep")
    rows, pixels, state = us.reference("deep", "full", "full")
    assert n == 8 and H * W // 65536 == 2
    assert (rows[0, 0, :, 8] == [0, 2 << 32, 2 << 32]).all() and (rows[1, 0, :, 8] == [2 << 32, 2 << 32, 0]).all()
    assert (rows[1, 1, :, 8] == [2 << 32, 0, 2 << 32]).all() and not rows[0, 1].any()
    assert 1 << 16 == 65536 and rows[0, 0, 0, 8, 1] == 2 * 65536 ** 2           # a block sum of 2^16, a square of 2^32
    assert rows[0, 0, 0, 7, 1] == 8 * 16384 ** 2 and rows[0, 0, 0, 6, 1] == 32 * 4096 ** 2
