"""The decision rule on the GPU (dc_logits_decide and dc_hysteresis_select of csrc/decide.hip, nn.DecisionRule, predict.py --decision_*)
against the numpy checker of tests/util_decide.py.  From q = rint(p * 65536) on everything is an integer: every comparison is equality.
The device rounds in fp32, the checker in float64, so the data stand clear of every rounding boundary by construction (asserted on the CPU
first, in util_decide.clear_triples); only the driver test, whose logits come from a network, excludes the pixels near a boundary.
The shapes come from the kernels' own constants.  With P from dc_decide_block: "tiny" is less than a wave and odd, so that planes 1 and 2
are not 16-byte aligned; "ragged" is odd, between 2 P and 3 P; "vector" is a multiple of 4 above 2 P whose last workgroup ends inside a
pass and inside a wave.  With (TH, TW) from dc_mask_components_tile: "tiles" = (2 TH + 3, 2 TW + 5) has interior tile borders, partial
tiles and a seam between different tiles.  Batch 3 with 2 valid samples; the padding sample has NaN logits and sentinel-filled outputs,
and guard words stand around every output."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_decide as ud  # noqa: E402
import util_events as ue  # noqa: E402
import util_prob as up  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = 3, 2
GUARD, SENTINEL = 64, 0x5A
ONE, NEVER = 65536, 65537
LOW, HIGH = (6000, 8000), (20000, 24000)             # for util_decide.smooth_logits, whose q stay below 32000


@functools.lru_cache(maxsize=None)
def _block():
    px = C.c_int(0)
    assert L.load().dc_decide_block(C.byref(px)) == 0 and px.value >= 256
    return px.value


@functools.lru_cache(maxsize=None)
def _tile():
    th, tw = C.c_int(0), C.c_int(0)
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0 and th.value >= 2 and tw.value >= 8
    return th.value, tw.value


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(H, W)"""
    P = _block()
    if name == "tiny":
        H, W = 3, 19
    elif name == "ragged":
        H = 101
        W = (5 * P // 2) // H | 1
        assert (H * W) % 2 == 1 and 2 * P < H * W < 3 * P
    elif name == "vector":
        H = 12
        W = (2 * P + P // 3) // H + 1
        assert (H * W) % 4 == 0 and H * W >= 2 * P and (H * W) % P % 256 != 0 and (H * W) % P % 1024 != 0
    else:
        TH, TW = _tile()
        H, W = 2 * TH + 3, 2 * TW + 5
    return H, W


def _kernel(shape):
    H, W = _shape(shape)
    return "decide_q_vec" if (H * W) % 4 == 0 else "decide_q"


def _batch(frames):
    """float32 [B, 3, H, W]: the valid frames, then the padding frame of NaN"""
    frames = np.asarray(frames, np.float32)
    assert frames.shape[0] == NV
    out = np.full((B,) + frames.shape[1:], np.nan, np.float32)
    out[:NV] = frames
    return out


@functools.lru_cache(maxsize=None)
def _smooth(shape):
    """logits [B, 3, H, W] of smooth constructed probabilities.  Shared and never modified."""
    H, W = _shape(shape)
    rs = np.random.RandomState(300 + H)
    logits = _batch([ud.smooth_logits(rs, H, W)[0] for _ in range(NV)])
    logits.setflags(write=False)
    return logits


@functools.lru_cache(maxsize=None)
def _reference(shape, low, high, connectivity, wrap, plain):
    """the checker's (cand, seed, out, counts) of _smooth(shape).  Shared and never modified."""
    ref = ud.batch(_smooth(shape)[:NV], low, high, connectivity, wrap, plain)
    for a in ref:
        a.setflags(write=False)
    return ref


def _guarded(n, dtype, fill=SENTINEL):
    """(store, view): n elements of `fill` with GUARD elements of SENTINEL on either side"""
    store = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    store[GUARD:GUARD + n] = fill
    return store, store[GUARD:GUARD + n]


def _run(logits, low, high, connectivity=8, wrap=True, route="hysteresis"):
    """The C ABI on guarded buffers: (cand, seed, out [NV, H, W], counts [NV, 12], launch names).  route "plain": no seed plane, no component
    pass (out is cand); "hysteresis": decide, components, select; "forced": the same with whatever thresholds, high == low included.
    Asserts that the guards and every output of the padding sample are untouched."""
    _, _, H, W = logits.shape
    n = B * H * W
    lg = torch.from_numpy(np.array(logits, np.float32, order="C")).to(DEV)
    stores = {}
    for name, dtype, size in (("cand", torch.uint8, n), ("seed", torch.uint8, n), ("out", torch.uint8, n), ("flags", torch.uint8, n),
                              ("labels", torch.int32, n), ("counts", torch.int64, B * 12)):
        stores[name] = _guarded(size, dtype)
    v = {k: s[1] for k, s in stores.items()}
    plain = route == "plain"
    st = L.stream_ptr()
    with served(route) as names:
        L.call("dc_logits_decide", B, NV, H, W, L.dptr(lg), low[0], low[1], high[0], high[1], L.dptr(v["cand"]),
               None if plain else L.dptr(v["seed"]), L.dptr(v["counts"]), st)
        if not plain:
            ws = torch.empty(max(L.load().dc_mask_components_workspace(B, H, W), 256), dtype=torch.uint8, device=DEV)
            L.call("dc_mask_components", B, NV, H, W, L.dptr(v["cand"]), connectivity, int(wrap), L.dptr(v["labels"]), L.dptr(ws), st)
            L.call("dc_hysteresis_select", B, NV, H, W, L.dptr(v["cand"]), L.dptr(v["seed"]), L.dptr(v["labels"]), L.dptr(v["flags"]),
                   L.dptr(v["out"]), L.dptr(v["counts"]), st)
    torch.cuda.synchronize()
    for name, (store, view) in stores.items():
        assert bool((store[:GUARD] == SENTINEL).all()) and bool((store[-GUARD:] == SENTINEL).all()), f"{name}: a guard word was written"
        per = view.numel() // B
        untouched = ("seed", "out", "flags", "labels") if plain else ()
        tail = view if name in untouched else view[NV * per:]
        assert bool((tail == SENTINEL).all()), f"{name}: the padding sample (or a buffer this route does not take) was written"
    host = {k: t.cpu().numpy() for k, t in v.items()}
    planes = [host[k].reshape(B, H, W)[:NV] for k in ("cand", "seed", "out")]
    if plain:
        planes[2] = planes[0]
    return planes[0], planes[1], planes[2], host["counts"].reshape(B, 12)[:NV], [x for x in names if not x.startswith("cc_")]


def _assert_equal(got, ref, what, plain=False):
    cand, seed, out, counts, _ = got
    assert np.array_equal(cand, ref[0]), (what, "cand", np.argwhere(cand != ref[0])[:6].tolist())
    if not plain:
        assert np.array_equal(seed, ref[1]), (what, "seed", np.argwhere(seed != ref[1])[:6].tolist())
    assert np.array_equal(out, ref[2]), (what, "out", np.argwhere(out != ref[2])[:6].tolist())
    want = ref[3].copy()
    if plain:                                        # the ABI leaves kept pixels to the caller on this route
        want[:, [2, 7]] = 0
    assert counts.dtype == np.int64 and np.array_equal(counts, want), (what, counts.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------------------------ 1. constructed fields
@pytest.mark.parametrize("route", ["plain", "hysteresis"])
@pytest.mark.parametrize("shape", ["tiny", "ragged", "vector"])
def test_smooth_fields_equal_the_checker(shape, route):
    plain = route == "plain"
    high = LOW if plain else HIGH
    got = _run(_smooth(shape), LOW, high, route=route)
    assert got[4] == [_kernel(shape)] + ([] if plain else ["decide_mark", "decide_select"])
    ref = _reference(shape, LOW, high, 8, True, plain)
    _assert_equal(got, ref, f"{shape} {route}", plain)
    if shape != "tiny":                              # the field exercises what it is meant to
        assert (ref[3][:, [0, 5, 11]] > 0).all() and ((ref[3][:, 1] > 0) | (ref[3][:, 6] > 0)).all()
    if not plain and shape != "tiny":
        assert (ref[2] != ref[0]).any() and ref[2].any()                         # something dropped, something kept


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_smooth_fields_on_tiles_every_connectivity_and_seam(connectivity, wrap):
    got = _run(_smooth("tiles"), LOW, HIGH, connectivity, wrap)
    ref = _reference("tiles", LOW, HIGH, connectivity, wrap, False)
    _assert_equal(got, ref, f"tiles c{connectivity} wrap={wrap}")
    assert (ref[3][:, [3, 8]] > 1).all() and (ref[2] != ref[0]).any() and ref[2].any()


# ------------------------------------------------------------------------------------------------------------------ 2. threshold edges
T1, T2 = 9000, 12000


def _edge_frame():
    """3 x 19 logits, one case per pixel of row 0 and 1 (the rest background), and the list of what they are"""
    H, W = _shape("tiny")
    q1, q2 = np.full((H, W), 50, np.int64), np.full((H, W), 70, np.int64)
    q1[0, 1], q1[0, 3] = T1, T1 - 1                                              # q == t, q == t - 1: class 1
    q2[0, 5], q2[0, 7] = T2, T2 - 1                                              # ... class 2
    q1[0, 9], q2[0, 9] = 20000, 15000                                            # conflicts: q1 > q2
    q1[0, 11], q2[0, 11] = 15000, 20000                                          # q2 > q1
    q1[0, 13], q2[0, 13] = 16000, 16000                                          # q1 == q2: class 1
    q1[0, 15], q2[0, 15] = 30000, 28000                                          # class 1 wins below high1; q2 >= high2 seeds nothing
    q2[0, 16] = T2 + 5                                                           # ... next to an unseeded class-2 candidate
    logits = ud.clear_triples(q1, q2)
    logits[:, 1, 1] = (0.0, -100.0, -100.0)                                      # q = (65536, 0, 0)
    logits[:, 1, 3] = (-100.0, 0.0, -100.0)                                      # q1 = 65536
    logits[:, 1, 5] = (-100.0, -100.0, 0.0)                                      # q2 = 65536
    q = up.quantise(logits)
    assert q[:, 1, 1].tolist() == [ONE, 0, 0] and q[1, 1, 3] == ONE and q[2, 1, 5] == ONE and up.distance_to_boundary(logits).min() >= 0.25
    return logits


def test_threshold_edge_cases():
    frame = _edge_frame()
    logits = _batch([frame, frame[:, ::-1, ::-1].copy()])                        # the second frame: the same cases in other lanes
    for low, high in (((T1, T2), (T1, T2)), ((0, NEVER), (0, NEVER)), ((NEVER, 0), (NEVER, 0)), ((0, 0), (0, 0)), ((ONE, ONE), (ONE, ONE)),
                      ((NEVER, NEVER), (NEVER, NEVER)), ((1, 1), (ONE, ONE))):
        got = _run(logits, low, high, route="plain" if low == high else "hysteresis")
        _assert_equal(got, ud.batch(logits[:NV], low, high, plain=low == high), f"low {low} high {high}", plain=low == high)
        cand = got[0][0]
        if low == (T1, T2):
            assert cand[0, [1, 3, 5, 7]].tolist() == [1, 0, 2, 0] and cand[0, [9, 11, 13]].tolist() == [1, 2, 1]
            assert cand[1, [1, 3, 5]].tolist() == [0, 1, 2] and got[3][0, 11] == 4    # 9, 11, 13, 15
        elif low == (0, NEVER):
            assert (cand == 1).all() and got[3][0, 11] == 0                      # t = 0 takes q = 0 too; 65537 never qualifies
        elif low == (NEVER, 0):
            assert (cand == 2).all()
        elif low == (0, 0):
            assert cand[1, [1, 3, 5]].tolist() == [1, 1, 2] and got[3][0, 11] == cand.size   # 0 == 0: class 1
        elif low == (ONE, ONE):
            assert cand[1, [1, 3, 5]].tolist() == [0, 1, 2] and int((cand != 0).sum()) == 2
        elif low == (NEVER, NEVER):
            assert not cand.any() and not got[3].any()
    # the lost conflict: class 1 at (0, 15) is below its high, and its q2 >= high2 seeds neither it nor the class-2 neighbour
    low, high = (8000, 8000), (31000, 25000)
    cand, seed, out, counts, _ = got = _run(logits, low, high)
    _assert_equal(got, ud.batch(logits[:NV], low, high), "lost conflict")
    assert cand[0, 0, 15] == 1 and cand[0, 0, 16] == 2 and seed[0, 0, 15] == 0 and seed[0, 0, 16] == 0 and not out[0, 0, 15:17].any()
    assert counts[0, [1, 6]].tolist() == [1, 1] and out[0, 1, 3] == 1 and out[0, 1, 5] == 2      # the only seeds: q1 = 65536 at (1, 3), q2 = 65536 at (1, 5)


# ------------------------------------------------------------------------------------------------------------------ 3. non-finite logits
@pytest.mark.parametrize("shape", ["tiny", "vector"])
def test_logits_that_are_not_finite_are_background_and_counted(shape):
    H, W = _shape(shape)
    q1 = np.full((NV, H, W), 30000, np.int64)                                    # every pixel a class-1 seed unless its logits say otherwise
    logits = _batch([ud.clear_triples(q1[b], np.full((H, W), 100, np.int64)) for b in range(NV)])
    spots = []
    for b in range(NV):
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            for plane in range(3):
                r, c = (k + b) % H, (3 * plane + k * 5 + 7 * b) % W
                assert (b, r, c) not in spots
                spots.append((b, r, c))
                logits[b, plane, r, c] = value
    low, high = (8000, 8000), (20000, 20000)
    for route, high in (("plain", low), ("hysteresis", high)):
        cand, seed, out, counts, _ = got = _run(logits, low, high, route=route)
        _assert_equal(got, ud.batch(logits[:NV], low, high, plain=route == "plain"), f"{shape} {route}", plain=route == "plain")
        assert counts[:, 10].tolist() == [9, 9] and counts[:, 0].tolist() == [H * W - 9] * NV
        for b, r, c in spots:
            assert cand[b, r, c] == 0 and out[b, r, c] == 0 and (route == "plain" or seed[b, r, c] == 0)


# ------------------------------------------------------------------------------------------------------------------ 4. hysteresis patterns
def _from_pattern(cls, seeds):
    """logits [3, H, W]: candidates of class cls[r, c] (0, 1, 2) under LOW, the pixels of `seeds` above HIGH"""
    q1 = np.where(cls == 1, np.where(seeds, 30000, 9000), 100)
    q2 = np.where(cls == 2, np.where(seeds, 31000, 11000), 200)
    return ud.clear_triples(q1, q2)


def _snake():
    """(pixels in order, H, W): one pixel wide, from column W - 20 eastwards across the seam and the first vertical tile border, then down
    a column across both horizontal tile borders"""
    H, W = _shape("tiles")
    TH, TW = _tile()
    path = [(3, c % W) for c in range(W - 20, W + TW + 6)] + [(r, TW + 5) for r in range(4, 2 * TH + 2)]
    assert len(set(path)) == len(path)
    return path, H, W


def _pattern(name):
    """(cls uint8 [NV, H, W], seeds bool [NV, H, W]); the second frame is the first with the classes swapped"""
    path, H, W = _snake()
    TH, TW = _tile()
    cls, seeds = np.zeros((H, W), np.uint8), np.zeros((H, W), bool)
    rows, cols = zip(*path)
    if name in ("snake", "snake-no-seed"):
        cls[rows, cols] = 1
        if name == "snake":
            seeds[path[-1]] = True                   # the far end: TH rows and a seam away from the head
    elif name == "touching":                         # a seeded class-1 block against an unseeded class-2 block, across a tile border
        cls[TH - 4:TH + 4, TW - 6:TW] = 1
        cls[TH - 4:TH + 4, TW:TW + 6] = 2
        seeds[TH - 1, TW - 3] = True
    elif name == "diagonal":                         # two blocks that meet at a tile corner, diagonally only
        cls[TH - 3:TH, TW - 3:TW] = 1
        cls[TH:TH + 3, TW:TW + 3] = 1
        seeds[TH - 2, TW - 2] = True
    elif name == "no-seed":
        cls[2:9, 5:40] = 1
        cls[TH:TH + 5, :] = 2
    else:                                            # "full": ONE component of H * W pixels, its only seed the last pixel
        cls[:] = 1
        seeds[H - 1, W - 1] = True
    swapped = np.where(cls == 1, 2, np.where(cls == 2, 1, 0)).astype(np.uint8)
    return np.stack([cls, swapped]), np.stack([seeds, seeds])


@pytest.mark.parametrize("name,connectivity,wrap", [("snake", 4, True), ("snake", 8, False), ("snake-no-seed", 8, True), ("touching", 8, True),
                                                    ("diagonal", 8, True), ("diagonal", 4, True), ("no-seed", 8, True), ("full", 4, True)])
def test_hysteresis_patterns(name, connectivity, wrap):
    cls, seeds = _pattern(name)
    logits = _batch([_from_pattern(cls[b], seeds[b]) for b in range(NV)])
    cand, seed, out, counts, _ = got = _run(logits, LOW, HIGH, connectivity, wrap)
    assert np.array_equal(cand, cls) and np.array_equal(seed != 0, seeds)
    _assert_equal(got, ud.batch(logits[:NV], LOW, HIGH, connectivity, wrap), f"{name} c{connectivity} wrap={wrap}")
    path, H, W = _snake()
    TH, TW = _tile()
    if name == "snake" and wrap:
        assert np.array_equal(out, cls) and counts[0, :5].tolist() == [len(path), 1, len(path), 1, 1] and counts[1, 5:10].tolist() == counts[0, :5].tolist()
    elif name == "snake":                            # the seam with wrap off: the 20 pixels west of it are a component without a seed
        assert not out[:, 3, W - 20:].any() and (out[0, 3, :TW + 6] == 1).all() and counts[0, :5].tolist() == [len(path), 1, len(path) - 20, 2, 1]
    elif name in ("snake-no-seed", "no-seed"):
        assert not out.any() and cand.any() and not counts[:, [1, 2, 4, 6, 7, 9]].any() and (counts[:, [3, 8]].sum(axis=1) > 0).all()
    elif name == "touching":
        assert np.array_equal(out[0], np.where(cls[0] == 1, 1, 0)) and np.array_equal(out[1], np.where(cls[1] == 2, 2, 0))
        assert counts[0].tolist() == [48, 1, 48, 1, 1, 48, 0, 0, 1, 0, 0, 0]
    elif name == "diagonal":
        both = connectivity == 8
        assert bool(out[0, TH, TW]) == both and out[0, TH - 1, TW - 1] == 1 and counts[0, :5].tolist() == [18, 1, 18 if both else 9, 1 if both else 2, 1]
    else:
        assert (out[0] == 1).all() and (out[1] == 2).all() and counts[0, :5].tolist() == [H * W, 1, H * W, 1, 1]


# ------------------------------------------------------------------------------------------------------------------ 5. properties
def test_properties_subset_monotone_and_both_routes_of_plain_thresholding():
    logits = _smooth("tiles")
    plain = _run(logits, LOW, LOW, route="plain")
    forced = _run(logits, LOW, LOW, route="forced")                              # high == low through the component pass
    assert plain[4] == ["decide_q"] and forced[4] == ["decide_q", "decide_mark", "decide_select"]
    assert np.array_equal(forced[2], plain[0]) and np.array_equal(forced[0], plain[0]) and np.array_equal(forced[1], (plain[0] != 0).astype(np.uint8))
    assert np.array_equal(forced[3][:, [2, 7]], forced[3][:, [0, 5]]) and np.array_equal(forced[3][:, [4, 9]], forced[3][:, [3, 8]])
    previous = forced[2]
    for high in ((10000, 12000), HIGH, (28000, 30000), (NEVER, NEVER)):          # raising high never adds a pixel
        cand, seed, out, counts, _ = _run(logits, LOW, high)
        assert np.array_equal(cand, plain[0])                                    # the candidates do not depend on high
        assert ((out == cand) | (out == 0)).all() and ((out == previous) | (out == 0)).all(), high
        assert int((out != 0).sum()) < int((previous != 0).sum()), high          # ... and on this field always drops some
        previous = out
    assert not previous.any()


# ------------------------------------------------------------------------------------------------------------------ 6. ProbabilitySkill
def test_thresholds_from_a_bin_reproduce_probability_skills_forecast():
    """The shared q: with class 2 off and low1 = high1 = decision_q_from_bin(k, K), mask == 1 is the forecast dc_prob_score counted in
    the bins >= k, so its hits and false alarms ARE the suffix sums of the device's own histogram of the same logits and labels."""
    H, W = _shape("vector")
    K = 20
    rs = np.random.RandomState(77)
    frames = []
    for _ in range(NV):
        l, q = up.constructed(rs, H * W)
        assert up.distance_to_boundary(l).min() >= 0.25
        frames.append(l.reshape(3, H, W))
    logits = torch.from_numpy(_batch(frames)).to(DEV)
    labels_np = rs.randint(0, 3, size=(B, H, W)).astype(np.int64)
    ps = dnn.ProbabilitySkill(B, H, W, bins=K, device=DEV)
    ps(logits, torch.from_numpy(labels_np).to(DEV), n_valid=NV)
    hist = ps.batch_hist().cpu().numpy()
    assert int(hist[1, :, :, 0].sum()) == NV * H * W
    for k in (0, 1, K // 2, K - 1, K):
        t = dnn.decision_q_from_bin(k, K)
        rule = dnn.DecisionRule(B, H, W, low=(t, NEVER), device=DEV)
        mask = rule(logits, n_valid=NV).cpu().numpy()
        assert mask.shape == (NV, H, W) and not (mask == 2).any()
        hits = int(((mask == 1) & (labels_np[:NV] == 1)).sum())
        alarms = int(((mask == 1) & (labels_np[:NV] != 1)).sum())
        assert (hits, alarms) == (int(hist[1, 1, k:, 0].sum()), int(hist[1, 0, k:, 0].sum())), k
        assert rule.counts()[:, 2].sum().item() == hits + alarms
    assert hits == alarms == 0                                                   # k = K: never


# ------------------------------------------------------------------------------------------------------------------ 7. nn.DecisionRule
def test_decision_rule_object_launch_record_and_refusals():
    H, W = _shape("vector")
    logits_np = _smooth("vector")
    logits = torch.from_numpy(np.array(logits_np)).to(DEV)
    plain = dnn.DecisionRule(B, H, W, low=LOW, device=DEV)
    hyst = dnn.DecisionRule(B, H, W, low=LOW, high=HIGH, connectivity=8, wrap=True, device=DEV)
    same = dnn.DecisionRule(B, H, W, low=LOW, high=LOW, device=DEV)
    assert not plain.hysteresis and not same.hysteresis and hyst.hysteresis and plain._seed is None and same._labels is None
    assert hyst.thresholds() == {"low_q": list(LOW), "high_q": list(HIGH), "low": [q / ONE for q in LOW], "high": [q / ONE for q in HIGH]}
    assert dnn.DecisionRule(B, H, W, low=(0.5, 1.5), device=DEV).thresholds()["low_q"] == [32768, NEVER]
    for rule in (plain, hyst):
        rule.mask_buffer.fill_(SENTINEL), rule.candidate_buffer.fill_(SENTINEL)
    with served("plain") as names:
        mask = plain(logits, n_valid=NV)
    assert names == ["decide_q_vec"] and mask.data_ptr() == plain.mask_buffer.data_ptr() == plain.candidate_buffer.data_ptr()
    ref = _reference("vector", LOW, LOW, 8, True, True)
    assert np.array_equal(mask.cpu().numpy(), ref[2]) and np.array_equal(plain.counts().cpu().numpy(), ref[3])      # kept = candidates
    assert bool((plain.mask_buffer[NV:] == SENTINEL).all())
    with served("hysteresis") as names:
        mask = hyst(logits, n_valid=NV)
    assert names == ["decide_q_vec", "cc_tile", "cc_merge", "cc_flatten", "decide_mark", "decide_select"]
    ref = _reference("vector", LOW, HIGH, 8, True, False)
    assert tuple(mask.shape) == (NV, H, W) and mask.dtype == torch.uint8 and mask.data_ptr() == hyst.mask_buffer.data_ptr()
    assert np.array_equal(mask.cpu().numpy(), ref[2]) and np.array_equal(hyst.candidate_buffer[:NV].cpu().numpy(), ref[0])
    counts = hyst.counts()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (NV, 12) and counts.is_cuda and np.array_equal(counts.cpu().numpy(), ref[3])
    assert bool((hyst.mask_buffer[NV:] == SENTINEL).all()) and bool((hyst.candidate_buffer[NV:] == SENTINEL).all())
    # a second call overwrites the first: nothing is left of the counters or the flags
    assert np.array_equal(hyst(logits, n_valid=NV).cpu().numpy(), ref[2]) and np.array_equal(hyst.counts().cpu().numpy(), ref[3])
    bad_calls = [
        lambda: hyst(logits[:, :, :, :-1].contiguous()), lambda: hyst(logits[:2]), lambda: hyst(logits.half()), lambda: hyst(logits.cpu()),
        lambda: hyst(logits.permute(0, 1, 3, 2)), lambda: hyst(None), lambda: hyst(logits, n_valid=B + 1), lambda: hyst(logits, n_valid=-1),
        lambda: L.call("dc_logits_decide", B, NV, H, W, L.dptr(logits), 10, 10, 9, 10, L.dptr(hyst._cand), L.dptr(hyst._seed), L.dptr(hyst._counts),
                       L.stream_ptr()),
        lambda: L.call("dc_logits_decide", B, NV, H, W, L.dptr(logits), 10, 10, 11, 10, L.dptr(hyst._cand), None, L.dptr(hyst._counts), L.stream_ptr()),
        lambda: L.call("dc_hysteresis_select", B, NV, H, W, L.dptr(hyst._cand), L.dptr(hyst._seed), L.dptr(hyst._labels), L.dptr(hyst._flags),
                       L.dptr(hyst._cand), L.dptr(hyst._counts), L.stream_ptr()),
    ]
    with served("refused") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        empty = hyst(logits, n_valid=0)                                          # nothing valid: nothing launched
    assert names == [] and tuple(empty.shape) == (0, H, W) and tuple(hyst.counts().shape) == (0, 12)
    assert np.array_equal(hyst.mask_buffer[:NV].cpu().numpy(), ref[2])           # ... and nothing written


def test_decision_rule_behind_a_bf16_predictor_with_stored_logits():
    H, W = util_val.H, util_val.W
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(2, H, W)
    net.load_state_dict(util_val.perturbed_state())
    net.eval()
    x, _ = util_val.val_inputs(n=2)
    pr = dnn.Predictor(net, 2, H, W)
    try:
        pr.store_logits = True
        pr(x.to(DEV))
        assert tuple(pr.logits_buffer.shape) == (2, 3, H, W) and pr.logits_buffer.dtype == torch.float32
        # thresholds from the logits themselves, so that whatever the network says there are candidates, seeds and regions to drop
        q = up.quantise(pr.logits.cpu().numpy().transpose(1, 0, 2, 3).reshape(3, -1))
        low = tuple(int(np.percentile(q[c], 70)) for c in (1, 2))
        high = tuple(int(np.percentile(q[c], 97)) + 1 for c in (1, 2))
        a = dnn.DecisionRule(2, H, W, low=low, high=high, device=DEV)
        b = dnn.DecisionRule(2, H, W, low=low, high=high, device=DEV)
        with served("DecisionRule behind Predictor") as names:
            on_buffer = a(pr.logits_buffer).clone()
        assert names[0] == "decide_q_vec" and names[-2:] == ["decide_mark", "decide_select"]
        fresh = pr.logits_buffer.clone()
        on_copy = b(fresh)
        assert torch.equal(on_buffer, on_copy) and torch.equal(a.counts(), b.counts()) and torch.equal(a.candidate_buffer, b.candidate_buffer)
        counts = a.counts().cpu().numpy()
        assert counts[:, [0, 5]].sum() > 0 and (counts[:, 2] == (on_buffer == 1).sum(dim=(1, 2)).cpu().numpy()).all()
        assert (counts[:, 7] == (on_buffer == 2).sum(dim=(1, 2)).cpu().numpy()).all() and not counts[:, 10].any()
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the driver
def _h5_write(path, datasets):
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with h5.File(path, "w") as f:
        for name, array in datasets.items():
            if backend == "h5py":
                f.create_dataset(name, data=array)
            else:
                f.write(name, array)


def _h5_read(path, names):
    """name -> array, None where the file has no such dataset"""
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with (h5.File(path, "r") if backend == "h5py" else h5.File(path)) as f:
        return {n: ((f[n][...] if backend == "h5py" else f.read(n)) if n in f else None) for n in names}


def test_predict_cli_with_a_decision_rule(tmp_path, monkeypatch):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(31)
    names = [f"data-2003-01-{d:02d}-00-1.h5" for d in (5, 6, 7)]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    for name, d in zip(names, fields):
        _h5_write(os.path.join(root, name), {"climate/data": d})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "bf16", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2", "--batch_size", "2"]

    # without the flags: no datasets, no entry, no launch of the family
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain])
    with served("predict without --decision_*") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("decide")]
    assert "decision" not in json.load(open(os.path.join(plain, "summary.json")))
    argmax = []
    for n in names:
        g = _h5_read(os.path.join(plain, n), ["prediction", "prediction_decided", "decision"])
        assert g["prediction_decided"] is None and g["decision"] is None
        argmax.append(g["prediction"])

    # The driver writes no logits: the test listens where they are decided.
    seen = []
    real_call = dnn.DecisionRule.__call__

    def listening(self, logits, n_valid=None):
        seen.append(logits[:n_valid].cpu().numpy())
        return real_call(self, logits, n_valid)

    monkeypatch.setattr(dnn.DecisionRule, "__call__", listening)
    wy, cx, sx = dnn.event_weight_tables(H, W)
    # (0.5, 0.5): this untrained network gives no class half of the probability anywhere (its softmax stays within 0.2 .. 0.5), so the
    # decided mask is empty there; (0.36, 0.34) lies inside its range and decides over a third of the pixels
    for low in ((0.5, 0.5), (0.36, 0.34)):
        del seen[:]
        out = str(tmp_path / f"out-{low[0]}")
        args = predict.build_parser().parse_args([*base, "--output_dir", out, "--events", "--decision_low", *(str(v) for v in low)])
        with served("predict --decision_low") as launched:                       # batches of two and one: a padded last batch
            predict.main(args)
        assert "decide_q_vec" in launched and not {"decide_mark", "decide_select"} & set(launched) and [len(lg) for lg in seen] == [2, 1]
        frames = [lg[j] for lg in seen for j in range(len(lg))]
        summary = json.load(open(os.path.join(out, "summary.json")))
        qlow = [dnn.decision_q(v) for v in low]
        assert summary["decision"]["low_q"] == qlow == summary["decision"]["high_q"] and summary["decision"]["low"] == [q / ONE for q in qlow]
        assert summary["decision"]["connectivity"] == 8 and summary["decision"]["hysteresis"] is False
        totals = np.zeros(12, np.int64)
        excluded = 0
        for name, lg, am in zip(names, frames, argmax):
            g = _h5_read(os.path.join(out, name), ["prediction", "prediction_decided", "decision", "events"])
            decided, counts = g["prediction_decided"], g["decision"]
            assert decided.dtype == np.uint8 and decided.shape == (H, W) and counts.dtype == np.int64 and counts.shape == (12,)
            assert np.array_equal(g["prediction"], am)                           # stays the argmax mask
            # the checker, outside the pixels where fp32 and float64 may round apart
            s = up.scaled_softmax(lg)
            near = (np.abs(s[1] - (qlow[0] - 0.5)) < up.EPS) | (np.abs(s[2] - (qlow[1] - 0.5)) < up.EPS)
            _, _, ref, _ = ud.frame(lg, qlow, qlow, plain=True)
            q = up.quantise(lg)
            near |= (q[1] >= qlow[0]) & (q[2] >= qlow[1]) & up.ambiguous(lg)
            excluded += int(near.sum())
            print(f"low {low} {name}: decided {(decided != 0).sum()} pixels, excluded {int(near.sum())}, differing {(decided != ref).sum()}")
            assert np.array_equal(decided[~near], ref[~near])
            assert counts[2] == (decided == 1).sum() == counts[0] and counts[7] == (decided == 2).sum() == counts[5] and counts[10] == 0
            assert not counts[[3, 4, 8, 9]].any()
            totals += counts
            # everything downstream takes the decided mask: the catalogue's rows are ITS components
            _, rows = ue.label_one(decided, 8, True, wy, cx, sx)
            assert len(rows) <= 4096 and np.array_equal(g["events"], rows)
        assert excluded <= 0.01 * len(frames) * H * W                             # a condition on the data, not a measurement
        assert summary["decision"]["counts"] == dict(zip(dnn.DECISION_COUNTS, (int(v) for v in totals)))
        assert [r["decision"] for r in summary["files"]] == [_h5_read(os.path.join(out, n), ["decision"])["decision"].tolist() for n in names]
        if low != (0.5, 0.5):
            assert totals[0] > 0 and totals[5] > 0 and totals[[0, 5]].sum() < len(frames) * H * W

    # hysteresis in front of the shape filter: decide -> filter -> catalogue
    monkeypatch.setattr(dnn.DecisionRule, "__call__", real_call)
    chain = str(tmp_path / "chain")
    args = predict.build_parser().parse_args([*base, "--output_dir", chain, "--events", "--decision_low", "0.34", "0.32", "--decision_high", "0.38",
                                              "0.36", "--event_filter", "--filter_min_pixels", "4", "4"])
    with served("predict --decision_high --event_filter") as launched:
        predict.main(args)
    assert {"decide_q_vec", "decide_mark", "decide_select"} <= set(launched)
    summary = json.load(open(os.path.join(chain, "summary.json")))
    assert summary["decision"]["hysteresis"] is True and summary["decision"]["high_q"] == [dnn.decision_q(0.38), dnn.decision_q(0.36)]
    for name in names:
        g = _h5_read(os.path.join(chain, name), ["prediction_decided", "prediction_filtered", "decision", "events"])
        decided, filtered = g["prediction_decided"], g["prediction_filtered"]
        print(f"chain {name}: counters {g['decision'].tolist()}")
        assert ((filtered == decided) | (filtered == 0)).all() and g["decision"][2] == (decided == 1).sum() and g["decision"][7] == (decided == 2).sum()
        labels, rows = ue.label_one(decided, 8, True, wy, cx, sx)
        assert [int((rows[:, 1] == c).sum()) for c in (1, 2)] == [int(g["decision"][4]), int(g["decision"][9])]     # kept events
        small = rows[rows[:, 2] < 4, 0] + 1
        assert np.array_equal(filtered, np.where(np.isin(labels, small), 0, decided))                            # the filter took the decided mask
        assert np.array_equal(g["events"], ue.label_one(filtered, 8, True, wy, cx, sx)[1][:4096])
    assert summary["decision"]["counts"]["class1_candidate_pixels"] > 0 and summary["decision"]["counts"]["class2_candidate_pixels"] > 0
