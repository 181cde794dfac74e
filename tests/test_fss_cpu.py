"""The neighbourhood verification's host side (no GPU): the checker of tests/util_fss.py against a naive quadruple loop and against the
analytic displaced-pixel case of the literature, nn.FractionsSkill.decode and the two-word totals on hand-made integers, the three entry
points in the header, the binding table and the thunks, the host-only entry points and the argument checks of the C ABI, and the driver's
flags and summary."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_fss as uf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_fss_block", "dc_fss_workspace", "dc_fss_score")


def _naive(pred, truth, windows, wrap, row_range):
    """the definition as four nested loops over Python ints"""
    H, W = pred.shape
    rows = np.zeros((2, len(windows), 3), np.int64)
    for k in (1, 2):
        for s, n in enumerate(windows):
            r = (n - 1) // 2
            a = b = c = 0
            for i in range(*row_range):
                for j in range(W):
                    f = o = 0
                    for di in range(-r, r + 1):
                        for dj in range(-r, r + 1):
                            y, x = i + di, j + dj
                            if not 0 <= y < H:
                                continue
                            if wrap:
                                x %= W
                            elif not 0 <= x < W:
                                continue
                            f += int(pred[y, x]) == k
                            o += int(truth[y, x]) == k
                    a, b, c = a + (f - o) ** 2, b + f * f, c + o * o
            rows[k - 1, s] = [a, b, c]
    return rows


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("row_range", [(0, 7), (2, 5), (6, 7)], ids=["full", "band", "one-row"])
def test_the_checker_equals_the_naive_loops(wrap, row_range):
    rs = np.random.RandomState(5)
    H, W = 7, 9
    pred = rs.choice(np.asarray([0, 1, 2, 3, 255], np.uint8), size=(H, W), p=[0.4, 0.25, 0.25, 0.05, 0.05])
    truth = rs.choice(np.asarray([0, 1, 2, -1, 257], np.int64), size=(H, W), p=[0.4, 0.25, 0.25, 0.05, 0.05])
    windows = [1, 3, 9]
    rows, pixels = uf.frame_rows(pred, truth, windows, wrap, row_range)
    assert rows.dtype == np.int64 and np.array_equal(rows, _naive(pred, truth, windows, wrap, row_range))
    band = slice(*row_range)
    assert pixels.tolist() == [[int((pred[band] == k).sum()), int((truth[band] == k).sum())] for k in (1, 2)]
    # window 1 is the per-pixel comparison: A counts the pixels where exactly one side has the class
    for k in (1, 2):
        assert rows[k - 1, 0].tolist() == [int(((pred[band] == k) != (truth[band] == k)).sum()), *pixels[k - 1].tolist()]


@pytest.mark.parametrize("seam", [False, True], ids=["inside", "across-the-seam"])
def test_one_displaced_pixel_scores_n_minus_d_over_n(seam):
    """Roberts & Lean (2008), the idealised case: one predicted and one labelled pixel, d columns apart, far from the poles: FSS = 0 for
    n <= d and exactly (n - d) / n for n > d (the windows holding exactly one of the two are 2 d n of the 2 n^2 that hold any)."""
    H, W, d = 41, 45, 4
    windows = [1, 3, 5, 7, 9, 15, 21]
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    c = W - 2 if seam else 20
    pred[20, c], truth[20, (c + d) % W] = 1, 1
    rows, pixels = uf.frame_rows(pred, truth, windows, wrap=True)
    assert pixels.tolist() == [[1, 1], [0, 0]]
    for s, n in enumerate(windows):
        a, b, c_ = (int(v) for v in rows[0, s])
        assert b == c_ == n * n
        if n <= d:
            assert a == 2 * n * n and uf.fss(a, b, c_) == 0.0
        else:
            assert a == 2 * d * n and uf.fss(a, b, c_) == 1.0 - (2 * d * n) / (2 * n * n)
            assert abs(uf.fss(a, b, c_) - (n - d) / n) < 1e-15
    assert dnn.fss_from_rows(rows)[0] == [uf.fss(*rows[0, s]) for s in range(len(windows))]
    assert dnn.fss_from_rows(rows)[1] == [None] * len(windows)                 # class 2 is absent from both masks
    if seam:                                                                    # without wrap the two never share a window below 2 * 41
        flat, _ = uf.frame_rows(pred, truth, windows, wrap=False)
        assert all(uf.fss(*flat[0, s]) == 0.0 for s in range(len(windows)))


def test_identical_masks_score_one_at_every_window():
    rs = np.random.RandomState(6)
    mask = rs.choice(np.asarray([0, 1, 2], np.uint8), size=(2, 12, 17), p=[0.6, 0.2, 0.2])
    windows = [1, 3, 9, 17]
    for wrap in (True, False):
        rows, _ = uf.batch_rows(mask, mask.astype(np.int64), windows, wrap, (1, 11))
        assert not rows[..., 0].any() and (rows[..., 1] == rows[..., 2]).all() and (rows[..., 1] > 0).all()
        assert dnn.fss_from_rows(rows) == [[[1.0] * len(windows)] * 2] * 2


def test_decode_of_hand_made_totals():
    windows = [1, 5, 3]                                                         # unordered: the skilful window is the smallest SIDE
    total = [[[90, 50, 50], [20, 100, 100], [30, 50, 50]],                      # class 1: 0.1, 0.9, 0.7
             [[0, 0, 0], [0, 0, 0], [0, 0, 0]]]                                 # class 2: absent from both masks
    pixels = [[40, 50], [0, 0]]
    out = dnn.FractionsSkill.decode(total, pixels, frames=5, windows=windows, rows=10, width=10)
    assert out == uf.decode(total, pixels, 5, windows, 10, 10)
    c1, c2 = out["class_1"], out["class_2"]
    assert c1["fss"] == [1.0 - 90 / 100, 1.0 - 20 / 200, 1.0 - 30 / 100] and c1["base_rate"] == 50 / 500 and c1["useful"] == 0.5 + 0.1 / 2
    assert c1["skilful_window"] == 3                                            # 0.7 >= 0.55 at 3; 0.1 at 1 is not
    assert c2 == {"fss": [None, None, None], "base_rate": 0.0, "useful": 0.5, "skilful_window": None}
    total[0][2] = [46, 50, 50]                                                  # 0.54 < 0.55: now only window 5 is skilful
    assert dnn.FractionsSkill.decode(total, pixels, 5, windows, 10, 10)["class_1"]["skilful_window"] == 5
    total[0][1] = [200, 100, 100]                                               # 0.0: none is
    assert dnn.FractionsSkill.decode(total, pixels, 5, windows, 10, 10)["class_1"]["skilful_window"] is None
    none = dnn.FractionsSkill.decode(total, pixels, 0, windows, 10, 10)         # no frame yet: no rate
    assert none["class_1"]["base_rate"] is None and none["class_1"]["useful"] is None and none["class_1"]["skilful_window"] is None
    # integers beyond 2^63 and beyond the 53 bits of a double: the quotient is taken from the exact integers
    big = [[[(1 << 70) + 1, 1 << 70, 1 << 70]], [[1, (1 << 90), 0]]]
    out = dnn.FractionsSkill.decode(big, pixels, 1, [9], 10, 10)
    assert out["class_1"]["fss"] == [1.0 - ((1 << 70) + 1) / (1 << 71)] and out["class_2"]["fss"] == [1.0 - 1 / (1 << 90)]


def test_the_two_word_total_recombines():
    words = np.zeros((2, 2, 3, 2), np.int64)
    words[0, 0, 0] = [-1, 0]                                                    # lo = 2^64 - 1: the top bit is set, the value is positive
    words[0, 0, 1] = [np.iinfo(np.int64).min, 3]                                # lo = 2^63
    words[0, 1, 2] = [5, 1]
    words[1, 1, 0] = [7, 0]
    got = dnn.FractionsSkill.combine(words)
    assert got[0][0][0] == (1 << 64) - 1 and got[0][0][1] == (3 << 64) + (1 << 63) and got[0][1][2] == (1 << 64) + 5 and got[1][1][0] == 7
    assert all(isinstance(v, int) and v >= 0 for cls in got for win in cls for v in win)
    assert got[1][0] == [0, 0, 0] and len(got) == 2 and len(got[0]) == 2 and len(got[0][0]) == 3
    with pytest.raises(L.DeepcamHipError):
        dnn.FractionsSkill.combine(np.zeros((2, 2, 3), np.int64))
    with pytest.raises(L.DeepcamHipError):
        dnn.fss_from_rows(np.zeros((2, 2), np.int64))


def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_fss", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert "int dc_fss_block(" in header and "size_t dc_fss_workspace(" in header and "int dc_fss_score(" in header
    for name in ("dc_fss_block", "dc_fss_score"):                               # the int-returning ones can be recorded
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_fss_score"][1]) == 20 and L._SIGS["dc_fss_workspace"][0] is C.c_size_t
    for word in ("fss_rows", "fss_cols", "fss_total"):
        assert word in header.split("int dc_launch_log_begin")[0]
    assert "fss.hip" in open(os.path.join(L.CSRC, "Makefile")).read()


def test_block_workspace_and_argument_checks_without_a_device():
    lib = L.load()
    cols, rows = C.c_int(0), C.c_int(0)
    assert lib.dc_fss_block(C.byref(cols), C.byref(rows)) == 0 and cols.value > 0 and rows.value > 0
    assert lib.dc_fss_block(None, C.byref(rows)) != 0 and "null" in L.last_error()
    ws = lib.dc_fss_workspace
    assert ws(8, 768, 1152, 7) == 8 * 7 * 768 * 1152 * 4 and ws(1, 1, 1, 1) == 4   # one word per pixel and window
    for bad in ((0, 8, 8, 1), (4096, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 8, 17), (1, 1 << 16, 1 << 15, 1), (-1, 8, 8, 1)):
        assert ws(*bad) == 0, bad
    fake = C.c_void_p(4096)                                                     # never dereferenced: the checks come before any launch
    score = lambda **kw: lib.dc_fss_score(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("n_valid", 2), ("H", 8), ("W", 12), ("pred", fake), ("pred_bytes", 1), ("truth", fake), ("truth_bytes", 8), ("S", 3),
        ("radius", fake), ("wrap", 1), ("row0", 0), ("row1", 8), ("rows", fake), ("pixels", fake), ("total", fake), ("total_pixels", fake),
        ("frames", fake), ("workspace", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert score(B=0) != 0 and score(B=4096) != 0 and score(H=0) != 0 and score(W=0) != 0 and "positive" in L.last_error()
        assert score(H=1 << 16, W=1 << 15, row1=1) != 0 and "2^31" in L.last_error()
        assert score(n_valid=-1) != 0 and score(n_valid=3) != 0 and "n_valid" in L.last_error()
        for side in ("pred_bytes", "truth_bytes"):
            for b in (0, 2, 3, 16):
                assert score(**{side: b}) != 0 and "mask_bytes" in L.last_error()
        assert score(S=0) != 0 and score(S=17) != 0 and "S must" in L.last_error()
        assert score(wrap=2) != 0 and score(wrap=-1) != 0 and "wrap" in L.last_error()
        for r0, r1 in ((-1, 8), (0, 9), (4, 4), (5, 4), (8, 8)):
            assert score(row0=r0, row1=r1) != 0 and "row range" in L.last_error()
        for name in ("pred", "truth", "radius", "rows", "pixels", "total", "total_pixels", "frames", "workspace"):
            assert score(**{name: None}) != 0 and "null" in L.last_error(), name
        assert score(truth=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert score(pred_bytes=4, pred=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        for name in ("radius", "rows", "pixels", "total", "total_pixels", "frames", "workspace"):
            assert score(**{name: C.c_void_p(4098)}) != 0 and "aligned" in L.last_error(), name
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                                                     # nothing was launched


def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False
    assert not [k for k in vars(a) if k.startswith("fss")]                      # flags that were not given leave no attribute behind
    assert predict.FSS_DEFAULTS == {"fss": False, "fss_windows": list(dnn.FSS_WINDOWS), "fss_rows": None, "fss_no_wrap": False}
    assert predict.fss_options(a) == {"windows": (1, 3, 9, 17, 33, 65, 129), "wrap": True, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--fss"])
    assert a.fss is True and a.verify is True and a.events is True              # the labels are needed: --fss implies --verify
    assert predict.fss_options(a) == {"windows": (1, 3, 9, 17, 33, 65, 129), "wrap": True, "row_range": None}
    a = predict.build_parser().parse_args(base + ["--fss", "--fss_windows", "5", "1", "21", "--fss_rows", "256", "512", "--fss_no_wrap"])
    assert a.fss_windows == [5, 1, 21] and a.fss_rows == [256, 512] and a.fss_no_wrap is True
    assert predict.fss_options(a) == {"windows": (5, 1, 21), "wrap": False, "row_range": (256, 512)}
    # like the other families: the options parse without the switch and are ignored
    a = predict.build_parser().parse_args(base + ["--fss_windows", "3"])
    assert not hasattr(a, "fss") and a.verify is False and a.fss_windows == [3]
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(base + ["--fss", "--fss_rows", "3"])
    assert "neighbourhood" in predict.build_parser().format_help()
    # what the constructor refuses, it refuses before it touches a device
    for kw in ({"windows": (1, 4)}, {"windows": (1, 257)}, {"windows": (-1,)}, {"windows": (3, 3)}, {"windows": ()}, {"windows": (13,)},
               {"windows": tuple(range(1, 35, 2))}, {"row_range": (4, 4)}, {"row_range": (0, 9)}, {"row_range": (-1, 4)}):
        with pytest.raises(L.DeepcamHipError):
            dnn.FractionsSkill(2, 8, 12, **{"windows": (1, 3), "device": "cpu", **kw})
    for shape in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, 1 << 15)):
        with pytest.raises(L.DeepcamHipError):
            dnn.FractionsSkill(*shape, windows=(1,), device="cpu")


def test_driver_summary_entry_on_checker_output():
    from mlperf_deepcam_amd import predict
    rs = np.random.RandomState(9)
    H, W, windows, band = 10, 14, (1, 3, 7), (2, 9)
    truth = rs.choice(np.asarray([0, 1, 2], np.int64), size=(3, H, W), p=[0.5, 0.3, 0.2])
    pred = np.roll(truth, 2, axis=2).astype(np.uint8)
    state = uf.totals([(pred[:2], truth[:2]), (pred[2:], truth[2:])], windows, True, band)
    s = predict.fss_summary(windows, band, W, state)
    ref = uf.decode(state["total"], state["pixels"], 3, windows, band[1] - band[0], W)
    assert s["windows"] == [1, 3, 7] and s["rows"] == [2, 9] and s["frames"] == 3
    for k in (1, 2):
        entry = dict(s[f"class_{k}"])
        assert entry.pop("total") == state["total"][k - 1] and entry.pop("pixels") == state["pixels"][k - 1]
        assert entry == ref[f"class_{k}"] and all(0.0 < f < 1.0 for f in entry["fss"])
        assert entry["fss"] == sorted(entry["fss"])                             # a displaced copy: the score grows with the window
    import json
    assert json.loads(json.dumps(s)) == s
