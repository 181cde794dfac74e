"""The decision rule's host side (no GPU): the checker of tests/util_decide.py against a per-pixel Python loop with a brute-force flood
fill, nn.decision_q and nn.decision_q_from_bin (the latter exhaustively against ProbabilitySkill's bin definition), the thresholds from a
ProbabilitySkill result, the cross-check of the two checkers (a thresholded mask's hits and false alarms are util_prob's suffix sums),
the calls the C ABI refuses, and the driver's flags."""
import ctypes as C
import math

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_decide as ud
import util_prob as up

ONE, NEVER = 65536, 65537


# ------------------------------------------------------------------------------------------------------------------ 1. the checker
def _naive(logits, low, high, connectivity, wrap):
    """the definition pixel by pixel in Python floats and ints; components by repeated relaxation of a label map to its fixed point"""
    _, H, W = logits.shape
    cand = [[0] * W for _ in range(H)]
    seed = [[0] * W for _ in range(H)]
    counts = [0] * 12
    for r in range(H):
        for c in range(W):
            l = [float(logits[k, r, c]) for k in range(3)]
            if not all(math.isfinite(v) for v in l):
                counts[10] += 1
                continue
            m = max(l)
            e = [math.exp(v - m) for v in l]
            q = [int(round(v / sum(e) * ONE)) for v in e]
            a1, a2 = q[1] >= low[0], q[2] >= low[1]
            if a1 and a2:
                counts[11] += 1
                k = 2 if q[2] > q[1] else 1
            else:
                k = 1 if a1 else (2 if a2 else 0)
            cand[r][c] = k
            seed[r][c] = int(k != 0 and q[k] >= high[k - 1])
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    comp = [[r * W + c if cand[r][c] else -1 for c in range(W)] for r in range(H)]
    changed = True
    while changed:                                   # every pixel takes the smallest index among its neighbours of the same class
        changed = False
        for r in range(H):
            for c in range(W):
                if not cand[r][c]:
                    continue
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if not 0 <= rr < H or (not wrap and not 0 <= cc < W):
                        continue
                    cc %= W
                    if cand[rr][cc] == cand[r][c] and comp[rr][cc] < comp[r][c]:
                        comp[r][c] = comp[rr][cc]
                        changed = True
    seeded = {comp[r][c] for r in range(H) for c in range(W) if seed[r][c]}
    out = [[cand[r][c] if comp[r][c] in seeded else 0 for c in range(W)] for r in range(H)]
    for k in (1, 2):
        roots = {comp[r][c] for r in range(H) for c in range(W) if cand[r][c] == k}
        counts[5 * k - 5:5 * k] = [sum(row.count(k) for row in cand), sum(seed[r][c] for r in range(H) for c in range(W) if cand[r][c] == k),
                                   sum(row.count(k) for row in out), len(roots), len(roots & seeded)]
    return np.asarray(cand, np.uint8), np.asarray(seed, np.uint8), np.asarray(out, np.uint8), np.asarray(counts, np.int64)


def _seam_frame():
    """7 x 11 logits: a class-1 component that crosses the seam with one seed, an unseeded class-1 speck, a class-2 bar with a conflict
    pixel at each end (one won by each class), a diagonal class-2 pair, and a NaN pixel inside the bar"""
    H, W = 7, 11
    q1, q2 = np.full((H, W), 100, np.int64), np.full((H, W), 200, np.int64)
    q1[1, [9, 10, 0, 1]] = [9000, 9500, 9200, 30000]            # crosses the seam; (1, 1) is its seed
    q1[3, 5] = 9000                                             # a speck: no seed
    q2[5, 2:9] = 12000                                          # a bar with a seed in the middle
    q2[5, 5] = 40000
    q1[5, 2], q1[5, 8] = 20000, 9000                            # conflicts: class 1 wins at (5, 2), class 2 at (5, 8)
    q2[3, 9], q2[4, 10] = 12000, 41000                          # joined only diagonally
    logits = ud.clear_triples(q1, q2)
    logits[1, 5, 4] = np.nan
    return logits


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("wrap", [True, False])
def test_checker_against_the_definition_pixel_by_pixel(connectivity, wrap):
    logits = _seam_frame()
    low, high = (8000, 10000), (25000, 35000)
    got = ud.frame(logits, low, high, connectivity, wrap)
    want = _naive(logits, low, high, connectivity, wrap)
    for g, w, what in zip(got, want, ("cand", "seed", "out", "counts")):
        assert np.array_equal(g, w), (what, g.tolist(), w.tolist())
    cand, seed, out, counts = got
    assert counts[10] == 1 and counts[11] == 2 and cand[5, 2] == 1 and cand[5, 8] == 2 and cand[5, 4] == 0
    assert bool(out[1, 9]) == wrap and out[1, 0] == 1 and out[3, 5] == 0           # the seam-crossing part is kept only with wrap
    assert bool(out[3, 9]) == (connectivity == 8) and out[4, 10] == 2
    assert seed[5, 2] == 0 and out[5, 2] == 0                                      # class 1 won the conflict below ITS high; class 2 seeds nothing there
    assert out[5, 3] == 0 and out[5, 6] == 2                                       # the NaN pixel cuts the bar: the half without the seed goes
    # the plain route: high == low
    cand, seed, out, counts = ud.frame(logits, low, low, plain=True)
    assert np.array_equal(out, cand) and np.array_equal(seed, (cand != 0).astype(np.uint8))
    assert counts[2] == counts[0] and counts[7] == counts[5] and counts[[3, 4, 8, 9]].tolist() == [0, 0, 0, 0]
    assert np.array_equal(ud.frame(logits, low, low, connectivity, wrap)[2], cand)  # ... which the component route reproduces


# ------------------------------------------------------------------------------------------------------------------ 2. thresholds
@pytest.mark.parametrize("K", [1, 3, 10, 20, 256])
def test_decision_q_from_bin_is_the_bin_definition_exhaustively(K):
    q = np.arange(ONE + 1, dtype=np.int64)
    bins = np.minimum(K - 1, (q * K) >> 16)
    for k in range(K + 1):
        t = dnn.decision_q_from_bin(k, K)
        assert isinstance(t, int) and 0 <= t <= NEVER
        assert np.array_equal(bins >= k, q >= t), (K, k, t)
    assert dnn.decision_q_from_bin(0, K) == 0 and dnn.decision_q_from_bin(K, K) == NEVER
    for k, bad_k in ((-1, K), (K + 1, K), (0, 0), (0, 257)):
        with pytest.raises(L.DeepcamHipError):
            dnn.decision_q_from_bin(k, bad_k)


def test_decision_q():
    assert dnn.decision_q(0) == 0 and dnn.decision_q(0.0) == 0 and dnn.decision_q(-0.5) == 0
    assert dnn.decision_q(2.0 ** -16) == 1 and dnn.decision_q(2.0 ** -17) == 1 and dnn.decision_q(1.5 * 2.0 ** -16) == 2
    assert dnn.decision_q(0.5) == 32768 and dnn.decision_q(1.0) == ONE
    assert dnn.decision_q(math.nextafter(1.0, 2.0)) == NEVER and dnn.decision_q(7) == NEVER and dnn.decision_q(math.inf) == NEVER
    with pytest.raises(L.DeepcamHipError):
        dnn.decision_q(math.nan)
    for p in (0.1, 0.25, 0.3, 0.9999):                                             # q >= decision_q(p)  iff  q / 65536 >= p
        t = dnn.decision_q(p)
        assert t / ONE >= p > (t - 1) / ONE
    assert len(dnn.DECISION_COUNTS) == 12 and len(set(dnn.DECISION_COUNTS)) == 12
    assert dnn.DECISION_COUNTS[2] == "class1_kept_pixels" and dnn.DECISION_COUNTS[9] == "class2_kept_events"


def test_from_prob_skill():
    K = 20
    decoded = {"bins": K, "class_0": {"best_csi_threshold": 0.0}, "class_1": {"best_csi_threshold": 0.85}, "class_2": {"best_csi_threshold": 0.3}}
    assert dnn.DecisionRule.low_from_prob_skill(decoded) == (dnn.decision_q_from_bin(17, K), dnn.decision_q_from_bin(6, K)) == (55706, 19661)
    decoded["class_2"]["best_csi_threshold"] = 1.0                                  # "nowhere" was best: never
    assert dnn.DecisionRule.low_from_prob_skill(decoded)[1] == NEVER
    # the arrays of a prob_skill.h5
    names = ("n", "best_csi", "best_csi_threshold")
    arrays = {"scalars": np.asarray([[5.0, 0.5, 0.0], [5.0, 0.4, 7 / 256], [5.0, 0.3, 255 / 256]]), "bins": np.asarray([256], np.int32),
              "scalar_names": np.frombuffer(",".join(names).encode(), np.uint8)}
    assert dnn.DecisionRule.low_from_prob_skill(arrays) == (7 * 256, 255 * 256)
    # a class without a threshold: refused before a device is touched
    decoded["class_1"]["best_csi_threshold"] = None
    arrays["scalars"][2, 2] = np.nan
    for bad in (decoded, arrays):
        with pytest.raises(L.DeepcamHipError, match="best_csi_threshold"):
            dnn.DecisionRule.low_from_prob_skill(bad)
        with pytest.raises(L.DeepcamHipError, match="best_csi_threshold"):
            dnn.DecisionRule.from_prob_skill(bad, 2, 8, 12, device="cpu")
    # what the constructor refuses, it refuses before it touches a device
    for kw in ({"low": (0.5,)}, {"low": 0.5}, {"low": (0.5, "a")}, {"low": (0.5, True)}, {"low": (-1, 5)}, {"low": (5, 65538)},
               {"low": (0.5, 0.5), "high": (0.4, 0.6)}, {"low": (100, 100), "high": (100, 99)}, {"connectivity": 6}):
        with pytest.raises(L.DeepcamHipError):
            dnn.DecisionRule(2, 8, 12, device="cpu", **kw)
    for shape in ((0, 8, 12), (4096, 8, 12), (1, 1 << 16, (1 << 14) + 1), (1, 0, 4)):
        with pytest.raises(L.DeepcamHipError):
            dnn.DecisionRule(*shape, device="cpu")


# ------------------------------------------------------------------------------------------------------------------ 3. the two checkers
def test_thresholded_mask_reproduces_the_scored_forecast():
    """class 2 off, low1 = high1 = decision_q_from_bin(k, K): mask == 1 IS ProbabilitySkill's forecast "class 1 at k / K", so its hits and
    false alarms against the labels are the suffix sums of util_prob's histogram"""
    H, W, K = 9, 31, 20
    rs = np.random.RandomState(5)
    logits, q = up.constructed(rs, H * W)
    assert up.distance_to_boundary(logits).min() >= 0.25
    logits = logits.reshape(3, H, W)
    labels = rs.randint(0, 3, size=(H, W))
    hist, _, pixels = up.frame(logits, labels, K)
    assert pixels.tolist() == [H * W, 0, 0]
    for k in (0, 1, K // 2, K - 1, K):
        t = dnn.decision_q_from_bin(k, K)
        _, _, mask, counts = ud.frame(logits, (t, NEVER), (t, NEVER), plain=True)
        assert not (mask == 2).any() and counts[5:10].tolist() == [0] * 5
        hits, alarms = int(((mask == 1) & (labels == 1)).sum()), int(((mask == 1) & (labels != 1)).sum())
        assert (hits, alarms) == (int(hist[1, 1, k:, 0].sum()), int(hist[1, 0, k:, 0].sum())), k
    assert int(hist[1, :, 0:, 0].sum()) == H * W                                    # k = 0 says yes everywhere


# ------------------------------------------------------------------------------------------------------------------ 4. the C ABI
def test_abi_refuses_bad_calls_without_a_device():
    lib = L.load()
    px = C.c_int(0)
    assert lib.dc_decide_block(C.byref(px)) == 0 and px.value >= 1024 and px.value % 1024 == 0
    assert lib.dc_decide_block(None) != 0
    assert lib.dc_decide_workspace(3, 7, 11) >= 3 * 7 * 11 and lib.dc_decide_workspace(8, 768, 1152) >= 8 * 768 * 1152
    for bad in ((0, 7, 11), (4096, 7, 11), (1, 0, 4), (1, 4, -1), (1, 1 << 16, (1 << 14) + 1)):
        assert lib.dc_decide_workspace(*bad) == 0
    P = lambda v: C.c_void_p(v)  # noqa: E731 -- addresses that are never dereferenced: every call below fails its argument check
    B, NV, H, W = 3, 2, 7, 11
    good = dict(B=B, n_valid=NV, H=H, W=W, logits=P(1 << 20), low1=100, low2=200, high1=300, high2=400, cand=P(2 << 20), seed=P(3 << 20),
                counts=P(4 << 20))

    def decide(**kw):
        a = dict(good, **kw)
        return lib.dc_logits_decide(a["B"], a["n_valid"], a["H"], a["W"], a["logits"], a["low1"], a["low2"], a["high1"], a["high2"], a["cand"],
                                    a["seed"], a["counts"], None)

    sel_good = dict(B=B, n_valid=NV, H=H, W=W, cand=P(2 << 20), seed=P(3 << 20), labels=P(5 << 20), flags=P(6 << 20), out=P(7 << 20),
                    counts=P(4 << 20))

    def select(**kw):
        a = dict(sel_good, **kw)
        return lib.dc_hysteresis_select(a["B"], a["n_valid"], a["H"], a["W"], a["cand"], a["seed"], a["labels"], a["flags"], a["out"], a["counts"],
                                        None)

    assert lib.dc_launch_log_begin() == 0
    try:
        for kw, word in (({"high1": 99}, "below its low"), ({"high2": 199}, "below its low"), ({"low1": -1}, "[0, 65537]"),
                         ({"low2": 65538, "high2": 65538}, "[0, 65537]"), ({"high1": 65538}, "[0, 65537]"), ({"B": 0}, "B must"),
                         ({"B": 4096}, "B must"), ({"H": 0}, "positive"), ({"W": 0}, "positive"), ({"H": 1 << 16, "W": (1 << 14) + 1}, "2^30"),
                         ({"n_valid": B + 1}, "n_valid"), ({"n_valid": -1}, "n_valid"), ({"seed": None}, "seed may be null only"),
                         ({"logits": None}, "null"), ({"cand": None}, "null"), ({"counts": None}, "null"), ({"logits": P((1 << 20) + 2)}, "aligned"),
                         ({"counts": P((4 << 20) + 4)}, "aligned"), ({"seed": P((2 << 20) + 8)}, "alias")):
            assert decide(**kw) != 0 and word in L.last_error(), (kw, L.last_error())
        for kw, word in (({"out": P(2 << 20)}, "out_mask may not alias cand"), ({"out": P((2 << 20) + B * H * W - 1)}, "out_mask may not alias cand"),
                         ({"flags": P(3 << 20)}, "alias"), ({"B": 0}, "B must"), ({"B": 4096}, "B must"), ({"W": 0}, "positive"),
                         ({"H": 1 << 16, "W": (1 << 14) + 1}, "2^30"), ({"n_valid": B + 1}, "n_valid"), ({"seed": None}, "null"),
                         ({"labels": None}, "null"), ({"flags": None}, "null"), ({"out": None}, "null"), ({"cand": None}, "null"),
                         ({"counts": None}, "null"), ({"labels": P((5 << 20) + 2)}, "aligned")):
            assert select(**kw) != 0 and word in L.last_error(), (kw, L.last_error())
        # n_valid == 0 is a good call that launches nothing, and so touches no address and needs no device
        assert decide(n_valid=0) == 0 and select(n_valid=0) == 0
        assert decide(n_valid=0, seed=None, high1=100, high2=200) == 0              # the plain route takes no seed plane
    finally:
        buf = C.create_string_buffer(256)
        assert lib.dc_launch_log_end(buf, 256) == 0
    assert buf.value == b""                           # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ 5. the driver
PLAIN_NAMESPACE = ["amp_opt_level", "batch_size", "channels", "checkpoint", "climatology", "climatology_by", "climatology_channels",
                   "climatology_contour", "confidence", "data_dir", "dtype", "event_connectivity", "event_fields", "event_filter", "event_shape",
                   "events", "filter_min_area_km2", "filter_min_aspect", "filter_min_length_km", "filter_min_pixels", "height",
                   "max_inter_threads", "min_event_cover", "min_event_pixels", "min_track_frames", "min_track_pixels", "output_dir",
                   "plot_channel", "plot_every", "plots", "stats_file", "track_center_channel", "track_fields", "tracks", "verify", "width"]


def test_driver_flags(capsys):
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert sorted(vars(a)) == PLAIN_NAMESPACE                                      # the namespace of before: no flag of the family leaves a trace
    assert predict.decision_options(a) is None
    a = predict.build_parser().parse_args(base + ["--decision_low", "0.7", "0.4"])
    assert a.decision_low == [0.7, 0.4] and not hasattr(a, "decision_high") and a.verify is False and a.events is False
    assert predict.decision_options(a) == {"low": (0.7, 0.4), "high": None}
    a = predict.build_parser().parse_args(base + ["--decision_low", "0.7", "0.4", "--decision_high", "0.9", "0.8"])
    assert predict.decision_options(a) == {"low": (0.7, 0.4), "high": (0.9, 0.8)}
    a = predict.build_parser().parse_args(base + ["--decision_from", "x.h5", "--decision_high", "0.9", "0.8"])
    assert a.decision_from == "x.h5" and a.decision_high == [0.9, 0.8] and not hasattr(a, "decision_low")
    for bad in (["--decision_low", "0.5", "0.5", "--decision_from", "x.h5"], ["--decision_from", "x.h5", "--decision_low", "0.5", "0.5"],
                ["--decision_high", "0.9", "0.9"], ["--decision_low", "0.5"], ["--decision_low", "a", "b"], ["--decision_high", "0.5"]):
        with pytest.raises(SystemExit):
            predict.build_parser().parse_args(base + bad)
    assert "--decision_high needs --decision_low or --decision_from" in capsys.readouterr().err
    import argparse
    with pytest.raises(ValueError):                                                 # a namespace made by hand meets the same checks
        predict.decision_options(argparse.Namespace(decision_high=[0.9, 0.9]))
    with pytest.raises(ValueError):
        predict.decision_options(argparse.Namespace(decision_low=[0.5, 0.5], decision_from="x.h5"))
    text = " ".join(predict.build_parser().format_help().split())
    assert "--decision_low TC AR" in text and "--decision_high TC AR" in text and "--decision_from FILE" in text and "hysteresis" in text


def test_driver_reads_thresholds_from_a_prob_skill_file(tmp_path):
    """--decision_from: the arrays predict.prob_arrays writes are the arrays decision_options reads"""
    import argparse
    from mlperf_deepcam_amd import predict
    H, W, K = 9, 31, 10
    rs = np.random.RandomState(8)
    logits, q = up.constructed(rs, H * W)
    labels = np.where(rs.rand(H * W) < 0.7, np.argmax(q, axis=0), rs.randint(0, 3, size=H * W))
    state = up.totals([(logits.reshape(1, 3, H, W), labels.reshape(1, H, W))], K)
    path = str(tmp_path / "prob_skill.h5")
    predict.write_datasets(path, predict.prob_arrays(K, state))
    decoded = up.decode(state["hist"], state["sq"], state["pixels"], K)
    want = tuple(dnn.decision_q_from_bin(round(decoded[f"class_{c}"]["best_csi_threshold"] * K), K) for c in (1, 2))
    got = predict.decision_options(argparse.Namespace(decision_from=path, decision_high=[0.95, 0.9]))
    assert got == {"low": want, "high": (0.95, 0.9)} and all(isinstance(v, int) for v in got["low"])
    assert dnn.DecisionRule.low_from_prob_skill(dnn.ProbabilitySkill.decode(state["hist"], state["sq"], state["pixels"], K)) == want
