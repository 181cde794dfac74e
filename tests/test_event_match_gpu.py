"""Event matching on the GPU (dc_component_overlap / dc_event_scores of csrc/event_match.hip, nn.EventMatcher, predict.py --verify) against
the numpy checker of tests/util_event_match.py.  Everything is integer: every comparison is exact.

Shapes come from the labelling kernel's tile (dc_mask_components_tile), as in test_events_gpu.py: (2 TH + 3, 2 TW + 5) has ragged tiles
on both edges and a width that is no multiple of 8, (TH - 1, TW - 3) is one partial tile.  Batch 3 with n_valid = 2: the third sample is
padding -- all class 1 on both sides, one huge pair if it were read -- and its slices of the outputs are pre-filled with sentinels."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_event_match as um  # noqa: E402
import util_events as ue  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV, CAP = 3, 2, 4096
COUNT_SENTINEL, SCORE_SENTINEL = -5, -9


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def _lds_slots():
    n = C.c_int()
    assert L.load().dc_component_overlap_lds_slots(C.byref(n)) == 0
    return n.value


TH, TW = _tile()
LDS_SLOTS = _lds_slots()            # the per-workgroup pair table of ov_pixel_kernel
SHAPES = {"tiles": (2 * TH + 3, 2 * TW + 5), "one": (TH - 1, TW - 3)}
CONN_WRAP = [(4, False), (4, True), (8, False), (8, True)]
CW_IDS = ["c4-nowrap", "c4-wrap", "c8-nowrap", "c8-wrap"]


# ------------------------------------------------------------------------------------------------------------------ masks
def _mask(name, H, W):
    """uint8 [3, H, W]; sample 2 is padding.  The name carries the side where the two sides differ."""
    rs = np.random.RandomState(zlib.crc32(f"match {name} {H} {W}".encode()))
    m = np.zeros((B, H, W), np.uint8)
    if name.startswith("random"):                       # "random0.45/a": density, then a salt that makes the sides independent
        p = float(name[6:].split("/")[0])
        m[:NV] = (rs.rand(NV, H, W) < p) * rs.randint(1, 3, (NV, H, W))
    elif name == "checker":
        rr, cc = np.mgrid[0:H, 0:W]
        m[0] = 1 + (rr + cc) % 2
        m[1] = 2 - (rr + cc) % 2
    elif name == "band/a":                              # crosses the seam: one component under wrap (sample 1: with 8-connectivity only)
        m[0, 5, :10] = 1
        m[0, 5, W - 10:] = 1
        m[1, 5, :10] = 2
        m[1, 6, W - 10:] = 2
    elif name == "band/b":                              # two pieces either side of the seam that do not reach it
        m[0, 5, 2:8] = 1
        m[0, 5, W - 8:W - 2] = 1
        m[1, 5, 2:8] = 2
        m[1, 6, W - 8:W - 2] = 2
    elif name == "rect/a":
        m[0, 3:11, 4:21] = 1
        m[1, 3:11, 4:21] = 2
    elif name == "rect/b":                              # the other class over part of it
        m[0, 5:13, 10:31] = 2
        m[1, 5:13, 10:31] = 1
    elif name == "empty":
        pass
    else:
        raise KeyError(name)
    m[NV:] = 1
    return m


def _discs(H, W, n, seed):
    """n discs of radius 6..22 and class 1 or 2 (later ones overwrite earlier ones), some across the seam"""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    rr, cc = np.mgrid[0:H, 0:W]
    for _ in range(n):
        r0, c0, rad, cl = rs.randint(0, H), rs.randint(0, W), rs.randint(6, 23), rs.randint(1, 3)
        dc = np.minimum(np.abs(cc - c0), W - np.abs(cc - c0))
        m[(rr - r0) ** 2 + dc ** 2 <= rad * rad] = cl
    return m


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


@functools.lru_cache(maxsize=None)
def _reference(name_a, name_b, shape, conn, wrap, cap=CAP, min_pixels=0, cover_q=512, pair_cap=None):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    H, W = SHAPES[shape]
    return um.match(_mask(name_a, H, W), _mask(name_b, H, W), NV, conn, wrap, *_tables(H, W), cap_a=cap, min_pixels=min_pixels,
                    cover_q=cover_q, pair_cap=pair_cap)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _run(mask_a, mask_b, conn, wrap, pair_cap, cap=CAP, min_pixels=0, cover_q=512, n_valid=NV):
    """both catalogues, then the two new calls on buffers pre-filled with sentinels (counts, scores) and with ones (what the call zeroes)"""
    nb, H, W = mask_a.shape
    lib, st = L.load(), L.stream_ptr()
    wy, cx, sx = (torch.from_numpy(t).to(DEV) for t in _tables(H, W))
    side = []
    for mask in (mask_a, mask_b):
        m = torch.from_numpy(mask).to(DEV)
        labels = torch.full((nb, H, W), -7, dtype=torch.int32, device=DEV)
        table = torch.ones((nb, cap, ue.FIELDS), dtype=torch.int64, device=DEV)
        ncomp = torch.full((nb, 3), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
        ws = torch.empty(lib.dc_mask_components_workspace(nb, H, W), dtype=torch.uint8, device=DEV)
        L.call("dc_mask_components", nb, n_valid, H, W, L.dptr(m), conn, int(wrap), L.dptr(labels), L.dptr(ws), st)
        L.call("dc_component_stats", nb, n_valid, H, W, L.dptr(m), L.dptr(labels), L.dptr(wy), L.dptr(cx), L.dptr(sx), cap, L.dptr(table),
               L.dptr(ncomp), L.dptr(ws), st)
        side.append((m, labels, table, ncomp, ws))
    (ma, la, ta, na, wa), (mb, lb, tb, nb_, wb) = side
    pairs = torch.ones((nb, pair_cap, 3), dtype=torch.int64, device=DEV)
    npairs = torch.full((nb, 2), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    cover_a = torch.ones((nb, cap), dtype=torch.int64, device=DEV)
    cover_b = torch.ones((nb, cap), dtype=torch.int64, device=DEV)
    scores = torch.full((nb, 2, 4), SCORE_SENTINEL, dtype=torch.int64, device=DEV)
    acc = torch.zeros(10, dtype=torch.int64, device=DEV)
    nbytes = lib.dc_component_overlap_workspace(nb, pair_cap)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=DEV)        # the call clears its table itself
    L.call("dc_component_overlap", nb, n_valid, H, W, L.dptr(ma), L.dptr(la), L.dptr(wa), cap, L.dptr(mb), L.dptr(lb), L.dptr(wb), cap,
           pair_cap, L.dptr(pairs), L.dptr(npairs), L.dptr(cover_a), L.dptr(cover_b), L.dptr(ws), st)
    L.call("dc_event_scores", nb, n_valid, cap, L.dptr(ta), L.dptr(na), L.dptr(cover_a), cap, L.dptr(tb), L.dptr(nb_), L.dptr(cover_b),
           L.dptr(npairs), min_pixels, cover_q, L.dptr(scores), L.dptr(acc), st)
    torch.cuda.synchronize()
    return {"pairs": pairs.cpu().numpy(), "npairs": npairs.cpu().numpy(), "cover_a": cover_a.cpu().numpy(), "cover_b": cover_b.cpu().numpy(),
            "scores": scores.cpu().numpy(), "acc": acc.cpu().numpy()}


def _assert_rest(got, ref, nv=NV):
    """coverage, scores, running sums and the padding: what holds whether or not the pair table overflowed"""
    assert np.array_equal(got["cover_a"][:nv], ref["cover_a"]), "cover_a differs"
    assert np.array_equal(got["cover_b"][:nv], ref["cover_b"]), "cover_b differs"
    assert np.array_equal(got["scores"][:nv], ref["scores"]), f"scores {got['scores'][:nv].tolist()} vs {ref['scores'].tolist()}"
    assert got["acc"][:8].tolist() == ref["scores"].sum(axis=0).reshape(8).tolist() and int(got["acc"][8]) == nv
    # the padding: pairs and coverage zeroed, counts and scores untouched
    assert not got["pairs"][nv:].any() and not got["cover_a"][nv:].any() and not got["cover_b"][nv:].any()
    assert (got["npairs"][nv:] == COUNT_SENTINEL).all() and (got["scores"][nv:] == SCORE_SENTINEL).all()


def _assert_equal(got, ref, nv=NV):
    """the table fits: every pair of the checker, sorted, nothing behind them, flag 0"""
    for s in range(nv):
        want = ref["pairs"][s]
        assert got["npairs"][s].tolist() == [len(want), 0], f"sample {s}: stored, flag {got['npairs'][s].tolist()}, expected {len(want)} pairs"
        assert np.array_equal(dnn.EventMatcher.sort_pairs(got["pairs"][s, :len(want)]), want), f"sample {s}: pairs differ"
        assert not got["pairs"][s, len(want):].any()
    _assert_rest(got, ref, nv)
    assert int(got["acc"][9]) == ref["truncated"]


def _fit(ref):
    """pair_cap from the checker's pair count: the test itself asserts that the table fits"""
    return max(max(len(p) for p in ref["pairs"]), 1)


# ------------------------------------------------------------------------------------------------------------------ 1. independent masks
@pytest.mark.parametrize("conn,wrap", CONN_WRAP, ids=CW_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("p", ["0.1", "0.45", "0.8"])
def test_independent_random_masks(p, shape, conn, wrap):
    H, W = SHAPES[shape]
    a, b = f"random{p}/a", f"random{p}/b"
    ref = _reference(a, b, shape, conn, wrap)
    assert max(len(q) for q in ref["pairs"]) > 3
    _assert_equal(_run(_mask(a, H, W), _mask(b, H, W), conn, wrap, pair_cap=_fit(ref)), ref)


# ------------------------------------------------------------------------------------------------------------------ 2. the global fallback
@pytest.mark.parametrize("wrap", [False, True], ids=["nowrap", "wrap"])
def test_more_pairs_in_a_tile_than_the_lds_table_holds(wrap):
    """Every pixel of the 4-connected checkerboard is a component of its own: a tile meets far more distinct pairs than its workgroup's
    table has slots, and the runs that find none go to the global table directly."""
    H, W = SHAPES["tiles"]
    cap = 16384                                          # H * W components: all of them have a row
    assert H * W <= cap
    ref = _reference("checker", "random0.45/b", "tiles", 4, wrap, cap=cap)
    for s in range(NV):
        la, lb = ref["labels_a"][s][:TH, :TW], ref["labels_b"][s][:TH, :TW]
        both = (la != 0) & (lb != 0)
        assert len(np.unique(np.stack([la[both], lb[both]], axis=1), axis=0)) > 2 * LDS_SLOTS
    _assert_equal(_run(_mask("checker", H, W), _mask("random0.45/b", H, W), 4, wrap, pair_cap=_fit(ref), cap=cap), ref)
    # and the other way round: the many components on side b
    ref = _reference("random0.45/b", "checker", "tiles", 4, wrap, cap=cap)
    _assert_equal(_run(_mask("random0.45/b", H, W), _mask("checker", H, W), 4, wrap, pair_cap=_fit(ref), cap=cap), ref)


# ------------------------------------------------------------------------------------------------------------------ 3. - 6. drawn cases
@pytest.mark.parametrize("conn,wrap", CONN_WRAP, ids=CW_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_band_across_the_seam(shape, conn, wrap):
    H, W = SHAPES[shape]
    ref = _reference("band/a", "band/b", shape, conn, wrap)
    got = _run(_mask("band/a", H, W), _mask("band/b", H, W), conn, wrap, pair_cap=_fit(ref))
    _assert_equal(got, ref)
    # sample 0: under wrap ONE band of 20 pixels holds both pieces (12 of its pixels: found, and both pieces hit); else two halves
    assert ref["pairs"][0].tolist() == ([[0, 0, 6], [0, 1, 6]] if wrap else [[0, 0, 6], [1, 1, 6]])
    assert ref["cover_a"][0][:2].tolist() == ([12, 0] if wrap else [6, 6])
    assert got["scores"][0].tolist() == [[2, 0, 0, 1 if wrap else 2], [0, 0, 0, 0]]
    joined = wrap and conn == 8                          # sample 1: the halves sit on neighbouring rows
    assert ref["pairs"][1].tolist() == ([[0, 0, 6], [0, 1, 6]] if joined else [[0, 0, 6], [1, 1, 6]])


@pytest.mark.parametrize("conn,wrap", [(4, False), (8, True)], ids=["c4-nowrap", "c8-wrap"])
def test_class_mismatch_is_listed_but_not_covered(conn, wrap):
    H, W = SHAPES["tiles"]
    ref = _reference("rect/a", "rect/b", "tiles", conn, wrap)
    got = _run(_mask("rect/a", H, W), _mask("rect/b", H, W), conn, wrap, pair_cap=_fit(ref))
    _assert_equal(got, ref)
    assert [q.tolist() for q in got["pairs"][:NV, 0]] == [[0, 0, 6 * 11], [0, 0, 6 * 11]]
    assert not got["cover_a"].any() and not got["cover_b"].any()
    # class 1 over class 2: a false alarm of class 1 and a miss of class 2; sample 1 the other way round
    assert got["scores"][0].tolist() == [[0, 0, 1, 0], [0, 1, 0, 0]] and got["scores"][1].tolist() == [[0, 1, 0, 0], [0, 0, 1, 0]]


@pytest.mark.parametrize("conn,wrap", [(4, True), (8, False)], ids=["c4-wrap", "c8-nowrap"])
def test_identical_masks(conn, wrap):
    H, W = SHAPES["tiles"]
    ref = _reference("random0.45/a", "random0.45/a", "tiles", conn, wrap)
    got = _run(_mask("random0.45/a", H, W), _mask("random0.45/a", H, W), conn, wrap, pair_cap=_fit(ref))
    _assert_equal(got, ref)
    for s in range(NV):
        n, n1, n2 = ref["ncomp_a"][s].tolist()
        assert got["npairs"][s, 0] == n and got["scores"][s].tolist() == [[n1, 0, 0, n1], [n2, 0, 0, n2]]      # every event a hit
        rows = dnn.EventMatcher.sort_pairs(got["pairs"][s, :n])
        assert rows[:, 0].tolist() == rows[:, 1].tolist() == list(range(n)) and rows[:, 2].tolist() == ref["rows_a"][s][:, 2].tolist()


@pytest.mark.parametrize("empty", ["a", "b"])
def test_an_empty_side(empty):
    H, W = SHAPES["one"]
    names = ("empty", "random0.45/b") if empty == "a" else ("random0.45/a", "empty")
    ref = _reference(*names, "one", 8, True)
    got = _run(_mask(names[0], H, W), _mask(names[1], H, W), 8, True, pair_cap=8)
    _assert_equal(got, ref)
    for s in range(NV):
        _, n1, n2 = (ref["ncomp_b"] if empty == "a" else ref["ncomp_a"])[s].tolist()
        assert n1 > 0 and n2 > 0 and got["npairs"][s].tolist() == [0, 0]
        assert got["scores"][s].tolist() == ([[0, n1, 0, 0], [0, n2, 0, 0]] if empty == "a" else [[0, 0, n1, 0], [0, 0, n2, 0]])


# ------------------------------------------------------------------------------------------------------------------ 7. - 9. caps, thresholds
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pair_table_overflow(shape):
    H, W = SHAPES[shape]
    a, b, pair_cap = "random0.45/a", "random0.45/b", 4
    ref = _reference(a, b, shape, 8, True, pair_cap=pair_cap)
    assert all(len(q) > pair_cap for q in ref["pairs"]) and ref["truncated"] == NV
    got = _run(_mask(a, H, W), _mask(b, H, W), 8, True, pair_cap=pair_cap)
    for s in range(NV):
        stored, flag = got["npairs"][s].tolist()
        assert flag == 1 and 0 < stored <= pair_cap
        rows = [tuple(r) for r in got["pairs"][s, :stored].tolist()]
        assert len(set(r[:2] for r in rows)) == stored                                     # distinct ...
        assert set(rows) <= set(tuple(r) for r in ref["pairs"][s].tolist())                # ... true pairs with their full counts
        assert not got["pairs"][s, stored:].any()
    _assert_rest(got, ref)                                                                  # coverage and scores do not depend on the table
    assert int(got["acc"][9]) == NV


@pytest.mark.parametrize("conn,wrap", [(4, True), (8, False)], ids=["c4-wrap", "c8-nowrap"])
def test_more_components_than_the_tables_hold(conn, wrap):
    H, W = SHAPES["tiles"]
    a, b, cap = "random0.8/a", "random0.8/b", 8
    ref = _reference(a, b, "tiles", conn, wrap, cap=cap)
    assert all(len(r) > cap for r in ref["rows_a"]) and all(len(r) > cap for r in ref["rows_b"]) and ref["truncated"] == NV
    got = _run(_mask(a, H, W), _mask(b, H, W), conn, wrap, pair_cap=_fit(ref), cap=cap)
    _assert_equal(got, ref)
    assert all(len(q) > 0 for q in ref["pairs"]) and int(got["pairs"][:, :, :2].max()) < cap
    assert int(got["scores"][:NV].sum()) <= 2 * cap * NV                                    # only the components that have a row are scored


THRESHOLDS = [(0, 1), (0, 512), (0, 1024), (4, 512), (8, 300)]


def test_thresholds_change_the_scores_as_in_the_checker():
    H, W = SHAPES["tiles"]
    a, b = "random0.45/a", "random0.45/b"
    ref0 = _reference(a, b, "tiles", 4, True)
    seen = set()
    for min_pixels, cover_q in THRESHOLDS:
        ref = _reference(a, b, "tiles", 4, True, min_pixels=min_pixels, cover_q=cover_q)
        got = _run(_mask(a, H, W), _mask(b, H, W), 4, True, pair_cap=_fit(ref0), min_pixels=min_pixels, cover_q=cover_q)
        _assert_equal(got, ref)
        seen.add(tuple(ref["scores"].reshape(-1).tolist()))
    assert len(seen) == len(THRESHOLDS)                  # each setting scores differently on these masks: the comparison discriminates


def test_every_sample_valid_and_a_single_sample():
    H, W = SHAPES["one"]
    ma, mb = _mask("random0.45/a", H, W), _mask("random0.45/b", H, W)
    ref = um.match(ma, mb, B, 8, True, *_tables(H, W), cap_a=CAP)
    _assert_equal(_run(ma, mb, 8, True, pair_cap=_fit(ref), n_valid=B), ref, nv=B)
    assert ref["pairs"][2].tolist() == [[0, 0, H * W]]                                      # the third sample: all class 1 on both sides
    ref = um.match(ma[:1], mb[:1], 1, 8, True, *_tables(H, W), cap_a=CAP)
    _assert_equal(_run(ma[:1], mb[:1], 8, True, pair_cap=_fit(ref), n_valid=1), ref, nv=1)


# ------------------------------------------------------------------------------------------------------------------ 10. - 13. nn.EventMatcher
def test_two_calls_agree_and_the_sums_add_up():
    H, W = SHAPES["tiles"]
    a, b = "random0.45/a", "random0.45/b"
    ref = _reference(a, b, "tiles", 8, True)
    ma, mb = torch.from_numpy(_mask(a, H, W)).to(DEV), torch.from_numpy(_mask(b, H, W)).to(DEV)
    other = torch.from_numpy(_mask("checker", H, W)).to(DEV)
    m = dnn.EventMatcher(B, H, W, connectivity=8, wrap=True)
    with served("EventMatcher") as names:
        m(ma, mb, n_valid=NV)
    first = (m.pairs(), m.cover(), m.scores())
    assert names[-3:] == ["cc_overlap"] * 3 and "cc_overlap" not in names[:-3]             # 12.: pixel pass and compaction, then the scores
    m(other, mb, n_valid=NV)                                                                # other pairs: rows the next call has to clear
    assert m.pairs()[0][0].shape != first[0][0][0].shape
    m.reset()
    assert m.result()["samples"] == 0 and not m.acc.cpu().any()
    m(ma, mb, n_valid=NV)
    m(ma, mb, n_valid=NV)
    torch.cuda.synchronize()
    again = (m.pairs(), m.cover(), m.scores())
    assert all(np.array_equal(x, y) for x, y in zip(first[0][0], again[0][0])) and first[0][1] == again[0][1] == [0, 0]
    assert all(np.array_equal(x, y) for x, y in zip(first[1], again[1])) and np.array_equal(first[2], again[2])
    assert all(np.array_equal(x, y) for x, y in zip(again[0][0], ref["pairs"]))
    assert np.array_equal(again[1][0], ref["cover_a"]) and np.array_equal(again[1][1], ref["cover_b"]) and np.array_equal(again[2], ref["scores"])
    assert not m.pair_table[:, max(len(q) for q in ref["pairs"]):].cpu().any()
    acc = m.acc.cpu().numpy()
    assert acc[:8].tolist() == (2 * ref["scores"].sum(axis=0)).reshape(8).tolist() and acc[8:].tolist() == [2 * NV, 0]
    res = m.result()
    assert res == dnn.EventMatcher.summarize(acc) and res["samples"] == 2 * NV and res["truncated"] is False
    h, mi = res["class_1"]["hits"], res["class_1"]["misses"]
    assert h + mi == 2 * int(ref["ncomp_b"][:, 1].sum()) and res["class_1"]["pod"] == h / (h + mi)
    m.reset()
    assert not m.acc.cpu().any()
    with pytest.raises(L.DeepcamHipError):
        m(ma, mb, n_valid=B + 1)


def test_launch_log_names_the_family_for_both_entry_points():
    H, W = SHAPES["one"]
    ma, mb = _mask("rect/a", H, W), _mask("rect/b", H, W)
    lib, st = L.load(), L.stream_ptr()
    z = lambda *shape, dtype=torch.int64: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    m = dnn.EventMatcher(B, H, W, cap=16, pair_cap=16)
    ta, tb = torch.from_numpy(ma).to(DEV), torch.from_numpy(mb).to(DEV)
    m(ta, tb, n_valid=NV)
    pairs, npairs, ca, cb, scores, acc = z(B, 16, 3), z(B, 2, dtype=torch.int32), z(B, 16), z(B, 16), z(B, 2, 4), z(10)
    ws = torch.empty(lib.dc_component_overlap_workspace(B, 16), dtype=torch.uint8, device=DEV)
    with served("dc_component_overlap") as names:
        L.call("dc_component_overlap", B, NV, H, W, L.dptr(ta), L.dptr(m.a._labels), L.dptr(m.a.rank_map), 16, L.dptr(tb),
               L.dptr(m.b._labels), L.dptr(m.b.rank_map), 16, 16, L.dptr(pairs), L.dptr(npairs), L.dptr(ca), L.dptr(cb), L.dptr(ws), st)
    assert names == ["cc_overlap", "cc_overlap"]
    with served("dc_event_scores") as names:
        L.call("dc_event_scores", B, NV, 16, L.dptr(m.a._table), L.dptr(m.a._ncomp), L.dptr(ca), 16, L.dptr(m.b._table), L.dptr(m.b._ncomp),
               L.dptr(cb), L.dptr(npairs), 0, 512, L.dptr(scores), L.dptr(acc), st)
    assert names == ["cc_overlap"]
    torch.cuda.synchronize()
    # rank_map: at every root pixel the row of its component
    for cat in (m.a, m.b):
        rank, rows = cat.rank_map.cpu().numpy(), cat.rows()[1]
        assert rank.shape == (NV, H, W) and rank.dtype == np.int32
        for s in range(NV):
            assert [int(rank[s].reshape(-1)[int(r[0])]) for r in rows[s]] == list(range(len(rows[s])))


def test_matcher_end_to_end_with_int64_labels():
    H, W = SHAPES["tiles"]
    a, b = "random0.45/a", "random0.45/b"
    ref = _reference(a, b, "tiles", 8, True, min_pixels=3, cover_q=256)
    ma = torch.from_numpy(_mask(a, H, W)).to(DEV)
    lb = torch.from_numpy(_mask(b, H, W).astype(np.int64)).to(DEV)
    m = dnn.EventMatcher(B, H, W, min_pixels=3, min_cover=0.25)
    assert m.cover_q == 256 and (m.a.cap, m.b.cap, m.pair_cap) == (4096, 4096, 8192)
    m(ma, lb, n_valid=NV)
    pairs, flags = m.pairs()
    assert flags == [0, 0] and all(np.array_equal(x, y) for x, y in zip(pairs, ref["pairs"])) and np.array_equal(m.scores(), ref["scores"])
    assert all(np.array_equal(x, y) for x, y in zip(m.a.rows()[1], ref["rows_a"])) and all(np.array_equal(x, y) for x, y in zip(m.b.rows()[1], ref["rows_b"]))
    got = m.matches()
    for s in range(NV):
        want = dnn.EventMatcher.join(ref["pairs"][s], ref["rows_a"][s], ref["rows_b"][s], H, W, min_pixels=3)
        assert got[s] == want and 0 < len(want) < len(ref["pairs"][s])
        ev_a, ev_b = dnn.EventCatalog.decode(ref["rows_a"][s], H, W), dnn.EventCatalog.decode(ref["rows_b"][s], H, W)
        for j in got[s]:                                 # the join names the right decoded events
            ra, rb = ref["rows_a"][s][:, 0].tolist().index(j["a"]["root"]), ref["rows_b"][s][:, 0].tolist().index(j["b"]["root"])
            assert j["a"] == ev_a[ra] and j["b"] == ev_b[rb] and [ra, rb, j["pixels"]] in ref["pairs"][s].tolist()
            assert j["iou"] == j["pixels"] / (j["a"]["pixels"] + j["b"]["pixels"] - j["pixels"]) and (j["class_a"], j["class_b"]) == (j["a"]["class"], j["b"]["class"])
    assert len(m.matches(min_pixels=0)[0]) == len(ref["pairs"][0])
    for bad in (ma.to(torch.float32), ma[:, :-1].contiguous()):
        with pytest.raises(L.DeepcamHipError):
            m(ma, bad)


# ------------------------------------------------------------------------------------------------------------------ 14. full size
def test_full_size_blobs():
    H, W = 768, 1152
    ma, mb = _discs(H, W, 40, 71)[None], _discs(H, W, 36, 72)[None]
    mb[0][ma[0] == 1] = np.where(np.arange(H)[:, None] < H // 2, 1, mb[0])[ma[0] == 1]      # the upper half's class-1 discs are in b as well
    ref = um.match(ma, mb, 1, 8, True, *_tables(H, W), cap_a=CAP)
    assert min(len(ref["rows_a"][0]), len(ref["rows_b"][0])) >= 12 and len(ref["pairs"][0]) >= 12 and 0 < ref["scores"][0, 0, 0]
    got = _run(ma, mb, 8, True, pair_cap=_fit(ref), n_valid=1)
    _assert_equal(got, ref, nv=1)
    print(f"768 x 1152: {len(ref['rows_a'][0])} / {len(ref['rows_b'][0])} events, {len(ref['pairs'][0])} pairs, scores {ref['scores'][0].tolist()}")


# ------------------------------------------------------------------------------------------------------------------ 15. driver
def test_predict_cli_with_verify(tmp_path):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "labelled")
    os.makedirs(root)
    rs = np.random.RandomState(12)
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(3)]
    truth = [_discs(H, W, 7, 300 + i).astype(np.int64) for i in range(3)]
    names = [f"data-{i:02d}.h5" for i in range(3)]
    for name, d, t in zip(names, fields, truth):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
            f.write("climate/labels_0", t)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)

    def run(out, *extra, data=root, ok=True):
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", data, "--stats_file", stats, "--output_dir",
               out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        if not ok:
            return r
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), json.load(open(os.path.join(out, "summary.json")))

    out, min_px = str(tmp_path / "verified"), 2
    line, summary = run(out, "--verify", "--min_event_pixels", str(min_px))               # batch 2 over three files: the last batch is ragged
    total, n_truth = np.zeros((2, 4), np.int64), 0
    for i, name in enumerate(names):
        with h5lite.File(os.path.join(out, name)) as f:
            p, ev, tr, ma, sc = (f.read(k) for k in ("prediction", "events", "truth_events", "matches", "event_scores"))
        assert all(x.dtype == np.int64 for x in (ev, tr, ma, sc)) and sc.shape == (2, 4) and ma.shape[1:] == (3,)
        ref = um.match(p[None], truth[i][None].astype(np.uint8), 1, 8, True, *_tables(H, W), cap_a=CAP, min_pixels=min_px, cover_q=512)
        rows_a, rows_b = ref["rows_a"][0], ref["rows_b"][0]
        keep_a, keep_b = [k for k, r in enumerate(rows_a) if r[2] >= min_px], [k for k, r in enumerate(rows_b) if r[2] >= min_px]
        assert np.array_equal(ev, rows_a[keep_a].reshape(-1, ue.FIELDS)) and np.array_equal(tr, rows_b[keep_b]), name
        want = [[keep_a.index(ra), keep_b.index(rb), n] for ra, rb, n in ref["pairs"][0].tolist() if ra in keep_a and rb in keep_b]
        assert ma.tolist() == want and np.array_equal(sc, ref["scores"][0]), name
        assert summary["files"][i]["event_scores"] == sc.tolist() and summary["files"][i]["matches_overflowed"] is False
        assert summary["files"][i]["events"] == [int((ev[:, 1] == 1).sum()), int((ev[:, 1] == 2).sum())]
        total += sc
        n_truth += len(keep_b)
    assert n_truth > 0 and int(total[:, :2].sum()) == n_truth                               # every labelled event is a hit or a miss
    ver = summary["event_verification"]
    assert ver == line["event_verification"] and ver["samples"] == 3 and ver["truncated"] is False
    for k in (0, 1):
        h, mi, fa, md = (int(v) for v in total[k])
        c = ver[f"class_{k + 1}"]
        assert (c["hits"], c["misses"], c["false_alarms"], c["matched"]) == (h, mi, fa, md)
        assert c["pod"] == (h / (h + mi) if h + mi else None) and c["far"] == (fa / (fa + md) if fa + md else None)
        assert c["csi"] == (h / (h + mi + fa) if h + mi + fa else None)
    # without the flag: the outputs of before, the same prediction bytes
    out2 = str(tmp_path / "plain")
    line2, summary2 = run(out2)
    assert "event_verification" not in summary2 and "event_verification" not in line2 and "events" not in summary2
    for name in names:
        with h5lite.File(os.path.join(out2, name)) as f:
            assert all(k not in f for k in ("events", "truth_events", "matches", "event_scores"))
            p2 = f.read("prediction")
        with h5lite.File(os.path.join(out, name)) as f:
            assert np.array_equal(f.read("prediction"), p2) and p2.dtype == np.uint8
    # a file without labels is an error that names the file
    bare = str(tmp_path / "bare")
    os.makedirs(bare)
    with h5lite.File(os.path.join(bare, "data-00.h5"), "w") as f:
        f.write("climate/data", fields[0])
    r = run(str(tmp_path / "never"), "--verify", data=bare, ok=False)
    assert r.returncode != 0 and "data-00.h5 has no climate/labels_0" in r.stderr
