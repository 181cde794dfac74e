"""The main course on the GPU (csrc/skeleton_course.hip; nn.EventAxis(course=True), nn.EventFilter(axis_measure="course")) against the
checker of util_event_course.py: equality of rows, course map and status, raw calls on poisoned buffers inside guard bands.  The rounds
depend on how the waves interleave (the header says so) and are held to [3, 3 * nodes].  Few rows: link lengths differ strongly by row;
no width is a multiple of 16, and frames of 25 x 71 start at every misalignment of the 16-byte loads."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_event_axis as ua  # noqa: E402
import util_event_course as uc  # noqa: E402
import util_events as ue  # noqa: E402
import util_skeleton_prune as up  # noqa: E402
from test_event_axis_gpu import DEV, GUARD, POISON, _guarded  # noqa: E402
from util_launch import served  # noqa: E402

NODE_CAP = 8192


@functools.lru_cache(maxsize=None)
def _reference(key, shape, conn, wrap, cap, n_valid, prune=0):
    """key: "drawn" (the hand-made skeletons, measured as they are), or a mask kind of util_event_axis (thinned, pruned) -> rows, course, status"""
    H, W = shape
    link, tables = dnn.axis_link_table(H, W), dnn.event_weight_tables(H, W)
    mask = np.stack([uc.drawn(n, H, W) for n in uc.CASES]) if key == "drawn" else ua.make_mask(key, H, W, 3)
    skel = mask if key == "drawn" else ua.thin(mask, n_valid, wrap, max(H, W))[0]
    skel = up.prune(skel, n_valid, wrap, prune)[0] if prune else skel
    labels, table, _, every = ue.catalogue(np.where(mask < 3, mask, 0).astype(np.uint8), n_valid, conn, wrap, *tables, cap)
    out = [uc.course(skel[b], labels[b], every[b][:, 0], cap, wrap, link, NODE_CAP) for b in range(n_valid)]
    return mask, tuple(np.stack([o[i] for o in out]) for i in range(3)) + (table,)


def _assert_course(rows, cmap, status, ref):
    where = np.argwhere((rows != ref[0]).any(axis=2))
    assert len(where) == 0, f"rows differ first at (sample, rank) {where[0].tolist()}: {rows[tuple(where[0])].tolist()} vs {ref[0][tuple(where[0])].tolist()}"
    assert np.array_equal(cmap, ref[1]), f"course pixels differ first at {np.argwhere(cmap != ref[1])[0].tolist()}"
    assert status[:, :, [0, 2]].tolist() == ref[2].tolist()
    swept, rounds = status[:, :, 0] * (1 - status[:, :, 2]), status[:, :, 1]           # a plane over the cap is not swept
    assert ((rounds >= 3 * (swept > 0)) & (rounds <= 3 * swept)).all(), status.tolist()


def _raw(skel, conn, wrap, cap, n_valid):
    """the raw entry point behind a catalogue of the map itself; asserts the guard bands and the padding samples' poison"""
    nb, H, W = skel.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    cat = dnn.EventCatalog(nb, H, W, connectivity=conn, wrap=bool(wrap), cap=cap, device=DEV)
    src, link = d(skel), d(dnn.axis_link_table(H, W))
    cat(src, n_valid=n_valid)
    bufs = {"rows": _guarded(nb * cap * 7, torch.int64), "course": _guarded(nb * H * W, torch.uint8), "status": _guarded(nb * 6, torch.int32),
            "node_ws": _guarded(nb * H * W * 2, torch.uint8)}
    L.call("dc_skeleton_course", nb, n_valid, H, W, L.dptr(src), L.dptr(cat._labels), L.dptr(cat._ws), cap, int(wrap), L.dptr(link),
           *(L.dptr(bufs[k][1]) for k in ("rows", "course", "status", "node_ws")), L.stream_ptr())
    torch.cuda.synchronize()
    got = {}
    for key, (whole, part) in bufs.items():
        p = POISON[whole.dtype]
        assert bool((whole[:GUARD] == p).all()) and bool((whole[-GUARD:] == p).all()), f"{key}: a store outside the buffer"
        got[key] = part.view(nb, -1).cpu().numpy()
        assert (got[key][n_valid:] == (p & 0xFF if whole.dtype == torch.uint8 else p)).all(), f"{key}: a padding sample was written"
    assert np.array_equal(src.cpu().numpy(), skel), "the input was written"
    return got["rows"][:n_valid].reshape(n_valid, cap, 7), got["course"][:n_valid].reshape(n_valid, H, W), got["status"][:n_valid].reshape(-1, 2, 3)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("shape", [(24, 70), (25, 71), (40, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hand_made_skeletons_through_the_raw_entry(shape, wrap, conn):
    skel, ref = _reference("drawn", shape, conn, wrap, 16, len(uc.CASES))
    with served() as names:
        got = _raw(skel, conn, wrap, 16, len(uc.CASES))
    _assert_course(*got, ref)
    assert "skel_course" in names and (ref[0][:, :, 6] > 0).any(axis=1).sum() >= len(uc.CASES) - 1      # every case but the dots has a length


@pytest.mark.parametrize("variant", ["uint8-conn8-wrap", "int64-conn4-nowrap"])
@pytest.mark.parametrize("prune", [0, 4])
@pytest.mark.parametrize("cap", [64, 3])
def test_event_axis_with_course_and_the_filter(cap, prune, variant):
    """random blobs, B = 3 with n_valid = 2, a cap below the event count; the filter on the course keeps what the checker's rows keep"""
    dtype, conn, wrap = (torch.uint8, 8, 1) if variant.startswith("uint8") else (torch.int64, 4, 0)
    H, W = 40, 130
    mask, ref = _reference("blobs", (H, W), conn, wrap, cap, 2, prune)
    cat = dnn.EventCatalog(3, H, W, connectivity=conn, wrap=bool(wrap), cap=cap, device=DEV)
    axis = dnn.EventAxis(cat, prune=prune, course=True)
    m = torch.from_numpy(mask).to(DEV)
    axis._course.fill_(POISON[torch.uint8]), axis._course_rows.fill_(POISON[torch.int64]), axis._course_status.fill_(POISON[torch.int32])
    min_km = (400, 700)
    flt = dnn.EventFilter(cat, min_axis_km=min_km, axis=axis, axis_measure="course")
    if dtype == torch.uint8:
        flt(m, n_valid=2)
    else:
        axis(m.to(dtype), n_valid=cat(m, n_valid=2)._last_valid)
    torch.cuda.synchronize()
    _assert_course(axis.course_table.cpu().numpy(), axis.course_buffer[:2].cpu().numpy(), axis.course_status(), ref)
    assert (axis.course_buffer[2] == POISON[torch.uint8]).all() and (axis._course_rows[2] == POISON[torch.int64]).all()
    assert (ref[0][:, :, 6] > 0).sum() >= 3 and [len(r) for r in axis.course_rows()] == [min(int(n), cap) for n in cat.counts()[:, 0]]
    assert all(e["course_km"] == r[6] / 1000.0 for e, r in zip(axis.axes()[0], ref[0][0]))
    if dtype == torch.uint8:
        want = [[int(ref[3][b, k, 1] in (1, 2) and ref[0][b, k, 6] >= 1000 * min_km[int(ref[3][b, k, 1]) - 1]) for k in range(cap)] for b in range(2)]
        assert flt.keep.cpu().tolist() == want and flt.thresholds()["axis_measure"] == "course"
        assert cap == 3 or 0 < sum(map(sum, want)) < int((ref[3][:, :, 1] > 0).sum())


def test_a_class_plane_over_the_node_cap_and_one_with_several_nodes_per_thread():
    """frame 0, class 1: full rows on every other row, one more than the cap holds -> not measured; class 2 in the same frame: one short
    line.  Frame 1: three full rows (rings under wrap) and a meridian, 3456 nodes: every thread owns several"""
    H, W, cap = 24, 1152, 16
    lines = L.load().dc_course_node_cap() // W + 1
    skel = np.zeros((2, H, W), np.uint8)
    skel[0, 0:2 * lines:2] = 1
    skel[0, 20, 7:30] = 2
    skel[1, 2:8:2] = 1
    skel[1, 10:23, 100] = 2
    rows, cmap, status = _raw(skel, 8, 1, cap, 2)
    link = dnn.axis_link_table(H, W)
    assert status[0, :, [0, 2]].T.tolist() == [[lines * W, 1], [23, 0]] and rows[0, :lines].tolist() == [[W, 0, 0, 0, 0, 0, -1]] * lines
    assert rows[0, lines].tolist() == [23, 20 * W + 7, 22 * link[20, 0], 20 * W + 29, 20 * W + 7, 23, 22 * link[20, 0]] and cmap[0].sum() == 46
    labels, _, _, every = ue.catalogue(skel, 2, 8, 1, *dnn.event_weight_tables(H, W), cap)
    ref = [uc.course(skel[b], labels[b], every[b][:, 0], cap, 1, link, NODE_CAP) for b in range(2)]
    _assert_course(rows, cmap, status, tuple(np.stack([o[i] for o in ref]) for i in range(3)))
    assert rows[1, 0].tolist() == [W, 2 * W, 576 * link[2, 0], 2 * W + 576, 2 * W, W, 576 * link[2, 0]]    # half way round, both ways


def test_launches_without_course_and_refusals():
    H, W = 24, 70
    cat = dnn.EventCatalog(2, H, W, cap=16, device=DEV)
    m = torch.from_numpy(ua.make_mask("blobs", H, W)).to(DEV)
    cat(m)
    for prune, want in ((0, ["skel_thin"] + ["skel_stats"] * 2), (3, ["skel_thin"] + ["skel_stats"] * 2 + ["skel_prune"] + ["skel_stats"] * 2)):
        plain = dnn.EventAxis(cat, prune=prune)
        with served() as names:
            plain(m)
        assert names == want and not hasattr(plain, "_course")
        with served() as names:
            dnn.EventAxis(cat, prune=prune, course=True)(m)
        assert names == want + ["skel_course"] * 2
    with pytest.raises(L.DeepcamHipError, match="only with course=True"):
        plain.course_table
    with pytest.raises(L.DeepcamHipError, match='needs an axis built with course=True'):
        dnn.EventFilter(cat, min_axis_km=(1, 1), axis=plain, axis_measure="course")
    ax = dnn.EventAxis(cat, course=True)
    args = [2, 2, H, W, L.dptr(m), L.dptr(cat._labels), L.dptr(cat._ws), 16, 1, L.dptr(ax._link), L.dptr(ax._course_rows), L.dptr(ax._course),
            L.dptr(ax._course_status), L.dptr(ax._node_ws), L.stream_ptr()]
    for pos, value, message in ((8, 2, "wrap must be 0 or 1"), (11, None, "null pointer"), (11, L.dptr(m), "overlaps an input"),
                                (13, L.dptr(ax._course), "may not overlap"), (2, 5000, "does not fit the LDS")):
        with pytest.raises(L.DeepcamHipError, match=message):
            L.call("dc_skeleton_course", *(args[:pos] + [value] + args[pos + 1:]))
