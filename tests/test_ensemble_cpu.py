"""The view ensemble without a GPU: the numpy checker of tests/util_ensemble.py against a second, per-pixel implementation; the host
helpers of nn (seam_weights, ViewEnsemble.decode, the refusals of ViewEnsemble.add, which come before any library call); the driver's
flags; and the error budget of property (P2) of include/deepcam_hip.h, evaluated in float64."""
import argparse

import numpy as np
import pytest
import torch

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_decide as ud
import util_ensemble as ue
import util_prob as up


# ------------------------------------------------------------------------------------------------------------------ 1. the checker
def _small_members(H=5, W=8):
    rs = np.random.RandomState(3)
    views = [(0, False, None), (3, True, ue.seam_weights(W, 3, 3)), (5, False, ue.seam_weights(W, 5, 2)), (W - 1, True, None)]
    members = []
    for roll, flip, wt in views:
        logits, q = ud.smooth_logits(rs, H, W, blobs=4)
        assert up.distance_to_boundary(logits).min() >= 0.25
        members.append((logits, roll, flip, wt))
    members[0][0][1, 2, 3] = np.nan                                               # member 0: first = 3 at source (2, 3)
    members[1][0][0, 0, 0] = np.inf                                               # member 1, view (0, 0): source (4, 3)
    members[3][0][2, 4, 7] = -np.inf                                              # member 3, view (4, 7): source (0, 6)
    return members


def test_checker_against_a_per_pixel_loop():
    H, W = 5, 8
    members = _small_members(H, W)
    for M in (1, 2, 4):
        state, Lp, top, rows = ue.frame(members[:M])
        bstate, bL, btop, brows = ue.brute_frame(members[:M])
        assert state.dtype == np.uint32 and np.array_equal(state, bstate) and np.array_equal(top, btop) and np.array_equal(rows, brows)
        assert np.array_equal(np.isnan(Lp), np.isnan(bL)) and np.allclose(Lp[~np.isnan(Lp)], bL[~np.isnan(bL)], rtol=1e-15, atol=0)
        S, votes, bad, first = ue.unpack(state)
        assert np.array_equal(ue.pack(S, votes, bad, first), state) and (votes.sum(axis=0) + bad == M).all()
        assert rows[:64].sum() == rows[64:128].sum() == rows[128:192].sum() == rows[192:].sum() == H * W
        assert first[2, 3] == 3 and bad[2, 3] == 1 and top[2, 3] == 3 and np.isnan(Lp[:, 2, 3]).all()
        if M >= 2:
            assert bad[4, 3] == 1 and first[4, 3] != 3 and top[4, 3] == 3
        if M == 4:
            assert bad[0, 6] == 1 and int(bad.sum()) == 3 and rows[ue.CHANGED + 15] == 1 and rows[[ue.CHANGED + 3, ue.CHANGED + 7, ue.CHANGED + 11]].sum() == 2
        finite = top < 3
        assert (np.take_along_axis(Lp, np.minimum(top, 2)[None], axis=0)[0][finite] == 0.0).all()
        assert np.array_equal(ue.argmax_first(Lp.astype(np.float32)[:, finite]), top[finite])      # (P1) in the checker itself


def test_view_maps_are_inverse_and_match_the_definition():
    H, W = 5, 8
    a = np.arange(H * W).reshape(H, W)
    for roll in (0, 1, 3, W - 1):
        for flip in (False, True):
            v = ue.to_view(a, roll, flip)
            assert np.array_equal(ue.to_source(v, roll, flip), a)
            for h in range(H):
                for w in range(W):
                    hs, ws = ue.source_of(h, w, H, W, roll, flip)
                    assert v[h, w] == a[hs, ws]
    x = np.random.RandomState(1).rand(2, H, W, 6).astype(np.float32)
    out = ue.view_input(x, [4, 0, 5], [1, -1, 1], [0.5, 0.25, 0.0], [2.0, 4.0, 1.0], 3, True)
    assert out.shape == (2, H, W, 3) and out[1, 0, 0, 1] == 4.0 * (-float(x[1, H - 1, 3, 0]) - 0.25) and out[0, 2, 7, 0] == 2.0 * (float(x[0, 2, 2, 4]) - 0.5)


# ------------------------------------------------------------------------------------------------------------------ 2. seam weights
def test_seam_weights():
    for W in (8, 96, 1152):
        for roll in (0, 1, W // 2, W - 1):
            assert dnn.seam_weights(W, roll, 1).tolist() == [1] * W               # the plain mean
            for margin in (2, 4, 8):
                wt = dnn.seam_weights(W, roll, margin)
                assert wt.dtype == np.uint16 and wt.shape == (W,) and np.array_equal(wt, ue.seam_weights(W, roll, margin))
                assert wt.min() == 1 and wt.max() == min(margin, W // 2)
                # the view's seam lies between its columns W - 1 and 0: source columns roll - 1 and roll
                assert np.flatnonzero(wt == 1).tolist() == sorted({(roll - 1) % W, roll})
                assert all(wt[(roll + d) % W] == wt[(roll - 1 - d) % W] == min(d + 1, margin) for d in range(W // 2))    # symmetric about it
    for bad in ((0, 0, 1), (8, 8, 1), (8, -1, 1), (8, 0, 0), (8, 0, 65536)):
        with pytest.raises(L.DeepcamHipError):
            dnn.seam_weights(*bad)


# ------------------------------------------------------------------------------------------------------------------ 3. decode
def test_decode_on_hand_made_totals():
    t = [0] * dnn.ENSEMBLE_ROW
    # 100 pixels, 3 members: 70 unanimous class 0, 10 unanimous class 1, 12 with (2, 1, 0) votes, 6 with (1, 1, 1), 2 not finite in one member (2, 0, 0)
    t[0 + 3], t[0 + 2], t[0 + 1], t[0 + 0] = 70, 12 + 2, 6, 10
    t[64 + 0], t[64 + 1], t[64 + 3] = 70 + 2, 12 + 6, 10
    t[128 + 0], t[128 + 1] = 70 + 10 + 12 + 2, 6
    changed = [[72, 5, 1, 2], [3, 12, 0, 0], [1, 0, 4, 0], [0, 0, 0, 0]]
    for i in range(4):
        t[192 + 4 * i:196 + 4 * i] = changed[i]
    d = dnn.ViewEnsemble.decode(t, 4, 3)
    assert d == ue.decode(t, 4, 3)
    assert d["frames"] == 4 and d["members"] == 3 and d["pixels"] == 100 and d["not_finite"] == 2 and d["unanimous"] == 0.8 and d["changed"] == changed
    assert d["class_0"]["vote_share"] == [0.1, 0.06, 0.14, 0.7] and d["class_0"]["mean_votes"] == (6 + 28 + 210) / 100
    assert d["class_1"]["vote_share"] == [0.72, 0.18, 0.0, 0.1] and d["class_2"]["vote_share"] == [0.94, 0.06, 0.0, 0.0]
    assert (d["class_0"]["gained"], d["class_0"]["lost"]) == (4, 8) and (d["class_1"]["gained"], d["class_1"]["lost"]) == (5, 3)
    assert (d["class_2"]["gained"], d["class_2"]["lost"]) == (1, 1)
    empty = dnn.ViewEnsemble.decode([0] * 208, 0, 2)
    assert empty["pixels"] == 0 and empty["unanimous"] is None and empty["class_1"]["vote_share"] == [None, None, None]
    for bad in (([0] * 207, 1, 1), ([0] * 208, 1, 64), ([0] * 208, 1, -1)):
        with pytest.raises(L.DeepcamHipError):
            dnn.ViewEnsemble.decode(*bad)


# ------------------------------------------------------------------------------------------------------------------ 4. the driver's flags
def test_driver_flags(capsys):
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert not [k for k in vars(a) if k.startswith("ensemble")]                     # no flag of the family leaves a trace
    assert predict.ensemble_options(a, 1152, a.channels) is None
    a = predict.build_parser().parse_args(base + ["--ensemble_rolls", "576", "288", "576", "0"])
    assert a.ensemble_rolls == [576, 288, 576, 0] and not hasattr(a, "ensemble_flip_lat") and not hasattr(a, "ensemble_seam_margin")
    assert predict.ensemble_options(a, 1152, a.channels) == {"views": [(0, False), (576, False), (288, False)], "margin": 1, "negate": []}
    a = predict.build_parser().parse_args(base + ["--ensemble_rolls", "48", "--ensemble_flip_lat", "--ensemble_negate", "2", "9", "--ensemble_seam_margin", "8"])
    assert predict.ensemble_options(a, 96, a.channels) == {"views": [(0, False), (48, False), (0, True), (48, True)], "margin": 8, "negate": [2, 9]}
    a = predict.build_parser().parse_args(base + ["--ensemble_flip_lat"])
    assert predict.ensemble_options(a, 96, a.channels)["views"] == [(0, False), (0, True)]
    for bad in (["--ensemble_negate", "2"], ["--ensemble_seam_margin", "4"], ["--ensemble_rolls"], ["--ensemble_rolls", "a"],
                ["--ensemble_rolls", "4", "--ensemble_negate", "2"]):
        with pytest.raises(SystemExit):
            predict.build_parser().parse_args(base + bad)
    err = capsys.readouterr().err
    assert "--ensemble_negate needs --ensemble_flip_lat" in err and "--ensemble_seam_margin needs --ensemble_rolls or --ensemble_flip_lat" in err
    ns = lambda **kw: argparse.Namespace(**kw)  # noqa: E731
    for bad in (ns(ensemble_rolls=[96]), ns(ensemble_rolls=[-1]), ns(ensemble_negate=[2]), ns(ensemble_seam_margin=2),
                ns(ensemble_flip_lat=True, ensemble_negate=[16]), ns(ensemble_rolls=[1], ensemble_seam_margin=0),
                ns(ensemble_rolls=[1], ensemble_seam_margin=40000), ns(ensemble_rolls=list(range(1, 33)), ensemble_flip_lat=True)):
        with pytest.raises(ValueError):
            predict.ensemble_options(bad, 96, list(range(16)))
    text = " ".join(predict.build_parser().format_help().split())
    assert "--ensemble_rolls S [S ...]" in text and "--ensemble_flip_lat" in text and "--ensemble_negate C [C ...]" in text and "--ensemble_seam_margin N" in text


# ------------------------------------------------------------------------------------------------------------------ 5. refusals on the host
def test_the_64th_member_and_a_weight_sum_above_65535_are_refused_before_any_library_call(monkeypatch):
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append(name))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    H, W = 4, 8
    ens = dnn.ViewEnsemble(2, H, W, device="cpu")
    lg = torch.zeros((2, 3, H, W))
    ens.add(lg, weights=np.full(W, 40000, np.uint16))
    assert calls == ["dc_ensemble_add"] and ens.members == 1
    with pytest.raises(L.DeepcamHipError, match="sum to at most 65535"):
        ens.add(lg, weights=np.full(W, 25536, np.uint16))
    with pytest.raises(L.DeepcamHipError, match="at least 1"):
        ens.add(lg, weights=np.arange(W).astype(np.uint16))
    assert calls == ["dc_ensemble_add"] and ens.members == 1
    ens.add(lg, weights=torch.from_numpy(np.full(W, 25535, np.uint16).view(np.int16).copy()))
    assert calls == ["dc_ensemble_add"] * 2 and ens.members == 2
    with pytest.raises(L.DeepcamHipError, match="sum to at most 65535"):
        ens.add(lg)                                                               # a member without weights weighs 1
    ens.begin()
    for m in range(63):
        ens.add(lg, roll=m % W)
    assert ens.members == 63 and len(calls) == 2 + 63
    with pytest.raises(L.DeepcamHipError, match="at most 63 members"):
        ens.add(lg)
    assert len(calls) == 2 + 63
    ens.pool()
    assert calls[-1] == "dc_ensemble_pool"


# ------------------------------------------------------------------------------------------------------------------ 6. the budget of (P2)
def test_error_budget_of_the_pooled_softmax():
    """(P2) allows 0.75 q-units between prob_q(L) and the exact share 65536 * max(S_c, 1) / sum_k max(S_k, 1): 0.5 for the rounding to an
    integer and 0.25 for everything in front of it, of which the arithmetic may use 0.15.  The chain is emulated in numpy's float32 --
    L rounded once from float64, then e = exp(L - max L), the sum, the quotient and the product with 65536, each rounded to fp32 -- over
    triples drawn up to 2^32 - 1, ties and empty classes included.  numpy's float32 exp stands for a correctly rounded expf; the device's
    may be 2 ulp off (2^-22 relative) in the numerator and in the sum, which moves a value of at most 65536 by at most 2 * 65536 * 2^-22 =
    0.03125 q-units, added below."""
    rs = np.random.RandomState(9)
    n = 200000
    S = np.floor(2.0 ** rs.uniform(0, 32, size=(3, n))).astype(np.int64)
    S = np.minimum(S, 2 ** 32 - 1)
    S[:, :1000] = rs.randint(0, 3, size=(3, 1000))                                # empty classes and small ties
    S[1, 1000:2000] = S[0, 1000:2000]                                             # exact ties at every size
    S[:, 2000:3000] = 2 ** 32 - 1 - rs.randint(0, 2, size=(3, 1000))
    S[0, 3000:4000] = 2 ** 32 - 1                                                 # the largest ratios
    top = S.max(axis=0)
    keep = top > 0
    S, top = S[:, keep], top[keep]
    L_ = np.log(np.maximum(S, 1).astype(np.float64) / top.astype(np.float64)).astype(np.float32)
    assert (L_.max(axis=0) == 0).all() and L_.min() >= np.float32(-23)
    e = np.exp(L_ - L_.max(axis=0, keepdims=True), dtype=np.float32)
    se = (e[0] + e[1]) + e[2]
    v = (e / se * np.float32(65536)).astype(np.float64)
    assert e.dtype == np.float32 and se.dtype == np.float32
    err = np.abs(v - ue.shares(S)).max() + 2 * 65536 * 2.0 ** -22
    print(f"(P2) arithmetic error in front of the rounding: {err:.4f} q-units (budget 0.15)")
    assert err <= 0.15
