"""The probabilistic verification's host side (no GPU): the checker of tests/util_prob.py against naive per-pixel Python loops,
nn.ProbabilitySkill.decode and the two-word totals on hand-made integers, the entry points in the header, the binding table and the
thunks, the host-only entry point and the argument checks of the C ABI, and the driver's flags and summary."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_prob as up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_prob_block", "dc_prob_score")
ONE = 65536


def _naive(logits, labels, K):
    """the definition pixel by pixel in Python floats (float64) and ints"""
    hist = [[[[0, 0] for _ in range(K)] for _ in range(2)] for _ in range(3)]
    rows, pixels = [0, 0, 0], [0, 0, 0]
    flat = np.asarray(logits, np.float32).reshape(3, -1)
    for i, y in enumerate(np.asarray(labels).reshape(-1).tolist()):
        l = [float(flat[c, i]) for c in range(3)]
        if not 0 <= y < 3:
            pixels[1] += 1
            continue
        if not all(math.isfinite(v) for v in l):
            pixels[2] += 1
            continue
        pixels[0] += 1
        m = max(l)
        e = [math.exp(v - m) for v in l]
        for c in range(3):
            q = int(round(e[c] / sum(e) * ONE))       # never at .5 exactly on such data: round-half-even and rint agree anyway
            o = int(y == c)
            b = min(K - 1, (q * K) >> 16)
            hist[c][o][b][0] += 1
            hist[c][o][b][1] += q
            rows[c] += (q - o * ONE) ** 2
    return hist, rows, pixels


@pytest.mark.parametrize("K", [1, 10, 20, 256])
def test_the_checker_equals_the_naive_loops(K):
    rs = np.random.RandomState(11)
    H, W = 9, 13
    logits = (3 * rs.randn(3, H, W)).astype(np.float32)
    logits[0, 0, 0], logits[1, 0, 1], logits[2, 0, 2], logits[0, 0, 3] = np.nan, np.inf, -np.inf, np.nan
    labels = rs.choice(np.asarray([0, 1, 2, 3, 255, -1, (1 << 32) + 1], np.int64), size=(H, W), p=[0.5, 0.2, 0.2, 0.025, 0.025, 0.025, 0.025])
    labels[0, :3] = [0, 1, 2]
    labels[0, 3] = 255                                # a bad label AND a logit that is not finite: a bad label
    hist, rows, pixels = up.frame(logits, labels, K)
    want = _naive(logits, labels, K)
    assert hist.dtype == np.int64 and hist.tolist() == want[0] and rows.tolist() == want[1] and pixels.tolist() == want[2]
    assert pixels[2] == 3 and pixels[1] == int(((labels < 0) | (labels > 2)).sum()) and pixels.sum() == H * W
    assert hist[..., 0].sum(axis=(1, 2)).tolist() == [pixels[0]] * 3
    state = up.totals([(logits[None], labels[None]), (logits[None], labels[None])], K)
    assert state["frames"] == 2 and state["sq"] == [2 * v for v in want[1]] and np.array_equal(state["hist"], 2 * hist)


def test_constructed_probabilities_stand_clear_of_the_boundaries():
    rs = np.random.RandomState(12)
    logits, q = up.constructed(rs, 20000)
    assert up.distance_to_boundary(logits).min() >= 0.25 and np.array_equal(up.quantise(logits), q)
    assert not up.ambiguous(logits).any()
    noisy = (3 * rs.randn(3, 20000)).astype(np.float32)
    share = up.ambiguous(noisy).mean()
    assert 0.2 < share < 0.4                          # three classes, a band of 2 / 16 each


def _hist(K, cells):
    """hist [3][2][K][2] with class 1 filled from {(outcome, bin): (n, q of every pixel)}; the other classes stay empty"""
    h = np.zeros((3, 2, K, 2), np.int64)
    for (o, k), (n, q) in cells.items():
        h[1, o, k] = [n, n * q]
    return h


def _sq(cells):
    return sum(n * (q - o * ONE) ** 2 for (o, _), (n, q) in cells.items())


def test_decode_a_perfectly_reliable_forecast():
    K = 4                                             # bins of a quarter; q = 1/8, 3/8, 5/8, 7/8 and exactly that share labelled
    cells = {}
    for k in range(K):
        cells[(1, k)] = (2 * k + 1, (2 * k + 1) * ONE // 8)
        cells[(0, k)] = (8 - (2 * k + 1), (2 * k + 1) * ONE // 8)
    d = dnn.ProbabilitySkill.decode(_hist(K, cells), [0, _sq(cells), 0], [32, 0, 0], K)
    c = d["class_1"]
    assert c["n"] == 32 and c["reliability"] == 0.0 and c["ece"] == 0.0 and c["mce"] == 0.0 and c["base_rate"] == 0.5
    assert c["curve"]["mean_probability"] == c["curve"]["observed_frequency"] == [0.125, 0.375, 0.625, 0.875]
    assert c["sharpness"] == [0.25] * 4 and c["mean_probability"] == 0.5 and c["uncertainty"] == 0.25
    assert abs(c["brier"] - (c["reliability"] - c["resolution"] + c["uncertainty"])) < 1e-12 and c["resolution"] > 0
    assert d == up.decode(_hist(K, cells), [0, _sq(cells), 0], [32, 0, 0], K)


def test_decode_perfectly_separated_classes():
    K = 10
    cells = {(1, K - 1): (30, ONE), (0, 0): (70, 0)}
    c = dnn.ProbabilitySkill.decode(_hist(K, cells), [0, _sq(cells), 0], [100, 0, 0], K)["class_1"]
    assert c["auc"] == 1.0 and c["brier"] == 0.0 and c["best_csi"] == 1.0 and c["brier_skill"] == 1.0 and c["reliability"] == 0.0
    assert c["best_csi_threshold"] == 0.1             # the smallest among equals: every threshold from 1 / K to (K - 1) / K separates
    assert c["pod"] == [1.0] * K + [0.0] and c["pofd"] == [1.0] + [0.0] * K and c["bias"][1] == 1.0 and c["csi"][0] == 0.3
    assert abs(c["resolution"] - c["uncertainty"]) < 1e-15


def test_decode_identical_distributions_for_both_outcomes():
    K = 5
    cells = {}
    for k in range(K):
        cells[(1, k)] = (3 * (k + 1), (2 * k + 1) * ONE // 10)
        cells[(0, k)] = (9 * (k + 1), (2 * k + 1) * ONE // 10)
    c = dnn.ProbabilitySkill.decode(_hist(K, cells), [0, _sq(cells), 0], [180, 0, 0], K)["class_1"]
    assert abs(c["auc"] - 0.5) < 1e-15 and c["resolution"] == 0.0 and c["base_rate"] == 0.25
    assert c["pod"] == c["pofd"]
    assert abs(c["brier"] - (c["reliability"] - c["resolution"] + c["uncertainty"])) < 1e-12


def test_decode_murphy_identity_on_random_cells_with_one_q_per_bin():
    rs = np.random.RandomState(13)
    for K in (1, 7, 20, 256):
        cells = {}
        for k in range(K):
            q = int(rs.randint(k * ONE // K + 1, (k + 1) * ONE // K))       # inside bin k
            assert min(K - 1, (q * K) >> 16) == k
            cells[(0, k)] = (int(rs.randint(0, 1000)), q)
            cells[(1, k)] = (int(rs.randint(0, 1000)), q)
        h, sq = _hist(K, cells), [0, _sq(cells), 0]
        n = int(h[1, :, :, 0].sum())
        d = dnn.ProbabilitySkill.decode(h, sq, [n, 0, 0], K)
        c = d["class_1"]
        assert abs(c["brier"] - (c["reliability"] - c["resolution"] + c["uncertainty"])) < 1e-12
        assert 0.0 <= c["auc"] <= 1.0 and c["mce"] >= c["ece"] >= 0.0
        ref = up.decode(h, sq, [n, 0, 0], K)["class_1"]
        for key, v in c.items():
            if isinstance(v, float):
                assert abs(v - ref[key]) <= 1e-12, key
            else:
                assert v == ref[key] or key in ("pod", "pofd", "csi", "bias", "curve", "sharpness"), key
        for key in ("pod", "pofd", "csi", "bias"):
            assert np.allclose(np.asarray(c[key], float), np.asarray(ref[key], float), rtol=0, atol=1e-15, equal_nan=True)


def test_decode_empty_classes_give_none():
    K = 3
    d = dnn.ProbabilitySkill.decode(np.zeros((3, 2, K, 2), np.int64), [0, 0, 0], [0, 5, 1], K)
    assert d["pixels"] == {"scored": 0, "bad_label": 5, "not_finite": 1} and d["bins"] == K
    for c in range(3):
        e = d[f"class_{c}"]
        assert e["n"] == 0
        for key in ("base_rate", "mean_probability", "brier", "brier_skill", "reliability", "resolution", "uncertainty", "ece", "mce", "auc",
                    "best_csi", "best_csi_threshold"):
            assert e[key] is None, key
        assert e["pod"] == e["pofd"] == e["csi"] == e["bias"] == [None] * (K + 1) and e["sharpness"] == [None] * K
        assert e["curve"] == {"mean_probability": [None] * K, "observed_frequency": [None] * K, "n": [0] * K}
    assert json.loads(json.dumps(d)) == d             # no NaN, nothing json cannot hold
    # a class that is never labelled: no POD, no AUC, no skill, but a Brier score and a reliability
    cells = {(0, 0): (10, 100), (0, 2): (5, 60000)}
    e = dnn.ProbabilitySkill.decode(_hist(K, cells), [0, _sq(cells), 0], [15, 0, 0], K)["class_1"]
    assert e["pod"] == [None] * (K + 1) and e["auc"] is None and e["brier_skill"] is None and e["base_rate"] == 0.0
    assert e["brier"] > 0 and e["reliability"] > 0 and e["csi"][0] == 0.0 and e["csi"][K] is None and e["pofd"][0] == 1.0
    assert e == up.decode(_hist(K, cells), [0, _sq(cells), 0], [15, 0, 0], K)["class_1"]
    with pytest.raises(L.DeepcamHipError):
        dnn.ProbabilitySkill.decode(np.zeros((3, 2, K + 1, 2), np.int64), [0, 0, 0], [0, 0, 0], K)


def test_the_two_word_total_recombines_and_frames_score():
    words = np.asarray([[-1, 0], [np.iinfo(np.int64).min, 3], [5, 1]], np.int64)
    assert dnn.ProbabilitySkill.combine(words) == [(1 << 64) - 1, (3 << 64) + (1 << 63), (1 << 64) + 5]
    with pytest.raises(L.DeepcamHipError):
        dnn.ProbabilitySkill.combine(np.zeros((3,), np.int64))
    big = dnn.ProbabilitySkill.decode(_hist(2, {(1, 1): (1 << 40, ONE - 1)}), [0, 1 << 70, 0], [1 << 40, 0, 0], 2)["class_1"]
    assert big["brier"] == (1 << 70) / (1 << 72)      # beyond 2^63: the quotient of the exact integers
    rows = np.asarray([[1 << 32, 0, 3 << 31], [7, 7, 7]], np.int64)
    pixels = np.asarray([[2, 1, 0], [0, 9, 9]], np.int64)
    assert dnn.brier_from_rows(rows, pixels) == [[0.5, 0.0, 0.75], [None, None, None]]
    assert dnn.brier_from_rows(rows[0], pixels[0]) == [0.5, 0.0, 0.75]
    with pytest.raises(L.DeepcamHipError):
        dnn.brier_from_rows(rows, pixels[0])


def test_the_entry_points_are_declared_bound_and_have_current_thunks():
    header = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_thunks_for_prob", os.path.join(L.CSRC, "gen_thunks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    thunks = open(os.path.join(L.CSRC, "program_thunks.inc")).read()
    assert gen.generate() == thunks
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.load(), name)
        assert f"int {name}(" in header
        assert f'{{"{name}", &t_{name}, {len(L._SIGS[name][1])}, ' in thunks
    assert len(L._SIGS["dc_prob_score"][1]) == 16
    for word in ("prob_zero", "prob_hist_vec", "prob_hist", "prob_total"):
        assert word in header.split("int dc_launch_log_begin")[0]
    assert "probskill.hip" in open(os.path.join(L.CSRC, "Makefile")).read()


def test_block_and_argument_checks_without_a_device():
    lib = L.load()
    px, groups = C.c_int(0), C.c_int(-1)
    assert lib.dc_prob_block(C.byref(px), C.byref(groups)) == 0 and px.value > 0 and groups.value >= 0
    assert px.value <= 65535                          # what a workgroup's private cells can hold between flushes
    assert lib.dc_prob_block(None, C.byref(groups)) != 0 and "null" in L.last_error()
    fake = C.c_void_p(4096)                           # never dereferenced: the checks come before any launch
    score = lambda **kw: lib.dc_prob_score(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("n_valid", 2), ("H", 8), ("W", 12), ("logits", fake), ("labels", fake), ("label_bytes", 8), ("K", 20), ("hist", fake),
        ("rows", fake), ("pixels", fake), ("total_hist", fake), ("total_sq", fake), ("total_pixels", fake), ("frames", fake), ("st", None))])
    assert lib.dc_launch_log_begin() == 0
    try:
        assert score(B=0) != 0 and score(B=4096) != 0 and score(H=0) != 0 and score(W=0) != 0 and "positive" in L.last_error()
        assert score(H=1 << 16, W=(1 << 14) + 1) != 0 and "2^30" in L.last_error()
        assert score(n_valid=-1) != 0 and score(n_valid=3) != 0 and "n_valid" in L.last_error()
        for b in (0, 2, 3, 16):
            assert score(label_bytes=b) != 0 and "label_bytes" in L.last_error()
        assert score(K=0) != 0 and score(K=257) != 0 and score(K=-1) != 0 and "K must" in L.last_error()
        for name in ("logits", "labels", "hist", "rows", "pixels", "total_hist", "total_sq", "total_pixels", "frames"):
            assert score(**{name: None}) != 0 and "null" in L.last_error(), name
        assert score(labels=C.c_void_p(4100)) != 0 and "aligned" in L.last_error()
        assert score(label_bytes=4, labels=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        assert score(logits=C.c_void_p(4098)) != 0 and "aligned" in L.last_error()
        for name in ("hist", "rows", "pixels", "total_hist", "total_sq", "total_pixels", "frames"):
            assert score(**{name: C.c_void_p(4100)}) != 0 and "aligned" in L.last_error(), name
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                           # nothing was launched


def test_driver_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.verify is False and a.events is False
    assert not [k for k in vars(a) if k.startswith("prob")]                     # flags that were not given leave no attribute behind
    assert predict.PROB_DEFAULTS == {"prob_skill": False, "prob_bins": 20} and predict.prob_options(a) == {"bins": 20}
    a = predict.build_parser().parse_args(base + ["--prob_skill"])
    assert a.prob_skill is True and a.verify is True and a.events is True       # the labels are needed: --prob_skill implies --verify
    assert predict.prob_options(a) == {"bins": 20}
    a = predict.build_parser().parse_args(base + ["--prob_skill", "--prob_bins", "256"])
    assert a.prob_bins == 256 and predict.prob_options(a) == {"bins": 256}
    a = predict.build_parser().parse_args(base + ["--prob_bins", "1"])           # parses without the switch and is ignored
    assert not hasattr(a, "prob_skill") and a.verify is False and a.prob_bins == 1
    for bad in ("0", "257", "-3", "ten", "2.5"):
        with pytest.raises(SystemExit):
            predict.build_parser().parse_args(base + ["--prob_skill", "--prob_bins", bad])
    text = " ".join(predict.build_parser().format_help().split())
    assert "--event_filter does not change them" in text and "reliability" in text
    # what the constructor refuses, it refuses before it touches a device
    for kw in ({"bins": 0}, {"bins": 257}, {"bins": -1}):
        with pytest.raises(L.DeepcamHipError):
            dnn.ProbabilitySkill(2, 8, 12, device="cpu", **kw)
    for shape in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, (1 << 14) + 1), (1, 0, 4)):
        with pytest.raises(L.DeepcamHipError):
            dnn.ProbabilitySkill(*shape, device="cpu")


def test_driver_summary_entry_on_checker_output():
    from mlperf_deepcam_amd import predict
    rs = np.random.RandomState(14)
    K, n = 10, 3
    labels = rs.choice(np.asarray([0, 1, 2, 255], np.int64), size=(n, 12, 16), p=[0.6, 0.2, 0.15, 0.05])
    logits = rs.randn(n, 3, 12, 16).astype(np.float32)
    for c in range(3):                                # a forecast with some skill
        logits[:, c][labels == c] += 1.5
    state = up.totals([(logits[:2], labels[:2]), (logits[2:], labels[2:])], K)
    s = predict.prob_summary(K, state)
    ref = up.decode(state["hist"], state["sq"], state["pixels"], K)
    assert s["bins"] == K and s["frames"] == n and s["pixels"] == ref["pixels"] and s["pixels"]["bad_label"] == int((labels == 255).sum())
    for c in range(3):
        entry = s[f"class_{c}"]
        assert tuple(entry) == ("brier", "brier_skill", "reliability", "resolution", "ece", "auc", "best_csi_threshold", "base_rate")
        for key, v in entry.items():
            assert abs(v - ref[f"class_{c}"][key]) <= 1e-12, key
        assert entry["auc"] > 0.6 and 0.0 < entry["brier"] < 0.25 and entry["brier_skill"] > 0
    assert json.loads(json.dumps(s)) == s
    arrays = predict.prob_arrays(K, state)
    assert np.array_equal(arrays["hist"], state["hist"]) and arrays["sq_words"].tolist() == [[v, 0] for v in state["sq"]]
    assert arrays["pod"].shape == (3, K + 1) and arrays["curve_n"].shape == (3, K) and arrays["scalars"].shape == (3, len(predict.PROB_SCALARS))
    assert bytes(arrays["scalar_names"]).decode().split(",") == list(predict.PROB_SCALARS)
    state["sq"][1] = (5 << 64) + (1 << 63) + 9        # the words of a total beyond one word
    assert predict.prob_arrays(K, state)["sq_words"][1].tolist() == [np.iinfo(np.int64).min + 9, 5]
