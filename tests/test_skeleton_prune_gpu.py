"""Spur pruning and the filter's axis criterion on the GPU (csrc/skeleton_prune.hip; nn.EventAxis(prune=), nn.EventFilter(min_axis_km=))
against the checkers of util_skeleton_prune.py: integer equality, no tolerance, every raw call on poisoned buffers inside guard bands.
8 x 64 is one word per row (its own neighbour across the seam), 9 x 65 has one valid bit in the last word."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_event_axis as ua  # noqa: E402
import util_events as ue  # noqa: E402
import util_skeleton_prune as up  # noqa: E402
from test_event_axis_gpu import DEV, GUARD, POISON, _guarded  # noqa: E402
from test_skeleton_prune_cpu import SHAPES, gpu_inputs  # noqa: E402


@functools.lru_cache(maxsize=None)
def _inputs(shape, wrap):
    names, maps = zip(*sorted(gpu_inputs(shape, wrap).items()))
    return names, np.stack(maps)


def _prune(skel, wrap, spur, n_valid=None):
    """the raw entry point; asserts the guard bands and the padding samples' poison -> (pruned [nv, H, W], removed [nv, 2])"""
    nb, H, W = skel.shape
    nv = nb if n_valid is None else n_valid
    src = torch.from_numpy(np.ascontiguousarray(skel)).to(DEV)
    bufs = {"pruned": _guarded(nb * H * W, torch.uint8), "removed": _guarded(nb * 2, torch.int32)}
    L.call("dc_skeleton_prune", nb, nv, H, W, L.dptr(src), int(wrap), spur, L.dptr(bufs["pruned"][1]), L.dptr(bufs["removed"][1]), L.stream_ptr())
    torch.cuda.synchronize()
    got = {}
    for key, (whole, part) in bufs.items():
        p = POISON[whole.dtype]
        assert bool((whole[:GUARD] == p).all()) and bool((whole[-GUARD:] == p).all()), f"{key}: a store outside the buffer"
        got[key] = part.view(nb, -1).cpu().numpy()
        assert (got[key][nv:] == (p & 0xFF if whole.dtype == torch.uint8 else p)).all(), f"{key}: a padding sample was written"
    assert np.array_equal(src.cpu().numpy(), skel), "the input was written"
    return got["pruned"][:nv].reshape(nv, H, W), got["removed"][:nv]


def _assert_pruned(got, ref, names=None):
    bad = np.argwhere(got[0] != ref[0])
    assert len(bad) == 0, f"{len(bad)} pixels differ, first at {bad[0].tolist()}" + (f" ({names[bad[0][0]]})" if names else "")
    assert got[1].tolist() == ref[1].tolist()


@pytest.mark.parametrize("spur", [1, 3, 16])
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pruned_map_matches_the_checker(shape, wrap, spur):
    names, maps = _inputs(shape, wrap)
    _assert_pruned(_prune(maps, wrap, spur), up.prune(maps, len(maps), wrap, spur), names)


@pytest.mark.parametrize("shift", [1, 63, 64])
def test_rolled_input_gives_rolled_output(shift):
    """backward and forward are directions, not indices: no column is special under wrap"""
    maps = _inputs((40, 72), 1)[1]
    plain, rolled = _prune(maps, 1, 3), _prune(np.roll(maps, shift, axis=2), 1, 3)
    assert np.array_equal(np.roll(plain[0], shift, axis=2), rolled[0]) and np.array_equal(plain[1], rolled[1]) and plain[1].any()


def test_padding_samples_and_removed_counts():
    names, maps = _inputs((40, 72), 1)
    maps = maps[[names.index(k) for k in ("spurs", "touching", "vee", "stairs", "ring")]]
    ref = up.prune(maps, 3, 1, 3)
    assert ref[1].any(axis=0).all()                                    # both classes lose pixels
    _assert_pruned(_prune(maps, 1, 3, n_valid=3), ref)


def test_full_size_frame():
    maps = np.stack([up.polylines(768, 1152, 3), up.polylines(768, 1152, 4)])
    ref = up.prune(maps, 2, 1, 16)
    assert (ref[1] > 100).all()
    _assert_pruned(_prune(maps, 1, 16), ref)


def test_refusals():
    z = torch.zeros(2 * 8 * 64, dtype=torch.uint8, device=DEV)
    o, r = torch.zeros_like(z), torch.zeros(4, dtype=torch.int32, device=DEV)
    for spur in (0, 1025):
        with pytest.raises(L.DeepcamHipError, match="spur must lie"):
            L.call("dc_skeleton_prune", 2, 2, 8, 64, L.dptr(z), 1, spur, L.dptr(o), L.dptr(r), L.stream_ptr())
    with pytest.raises(L.DeepcamHipError, match="does not fit the LDS"):
        L.call("dc_skeleton_prune", 1, 1, 1024, 2048, L.dptr(z), 1, 3, L.dptr(o), L.dptr(r), L.stream_ptr())
    with pytest.raises(L.DeepcamHipError, match="may not alias"):
        L.call("dc_skeleton_prune", 2, 2, 8, 64, L.dptr(z), 1, 3, L.dptr(z), L.dptr(r), L.stream_ptr())


def test_select_axis_on_a_small_table():
    """B = 3 with n_valid = 2, cap = 4: sample 0 has 6 events (rows beyond cap), one already dropped, one of class 3; class 2's threshold is off"""
    rs = np.random.RandomState(5)
    table = np.zeros((3, 4, 10), np.int64)
    table[:, :, 1] = [[1, 2, 1, 3], [1, 1, 2, 2], [1, 1, 1, 1]]
    ncomp = np.array([[6, 0, 0], [3, 0, 0], [4, 0, 0]], np.int32)
    axis = rs.randint(0, 3000, (3, 4, 7)).astype(np.int64)
    axis[0, :, 6], axis[1, :, 6] = [999, 10, 1000, 5], [1500, 20, 30, 40]
    keep = np.array([[1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
    counts = rs.randint(5, 50, (3, 2, 4)).astype(np.int64)
    for min_m in ((1000, 0), (0, 0), (25, 35)):
        dev = [torch.from_numpy(a).to(DEV) for a in (table, ncomp, axis, keep, counts)]
        L.call("dc_event_select_axis", 3, 2, 4, *(L.dptr(t) for t in dev[:3]), min_m[0], min_m[1], L.dptr(dev[3]), L.dptr(dev[4]), L.stream_ptr())
        torch.cuda.synchronize()
        rk, rc = up.select_axis(table[:2], ncomp, axis, min_m, keep[:2], counts[:2])
        assert np.array_equal(dev[3].cpu().numpy(), np.concatenate([rk, keep[2:]])), min_m
        assert np.array_equal(dev[4].cpu().numpy(), np.concatenate([rc, counts[2:]])), min_m
    assert rk[0].tolist() == [1, 0, 1, 1] and rk[1].tolist() == [0, 0, 0, 1]      # (25, 35): what the last thresholds drop


def test_event_axis_with_prune_and_the_filter_end_to_end():
    H, W, cap = 40, 72, 512
    mask = ua.make_mask("blobs", H, W)
    cat = dnn.EventCatalog(2, H, W, cap=cap)
    axis = dnn.EventAxis(cat, prune=8)
    m = torch.from_numpy(mask).to(DEV)
    with pytest.raises(L.DeepcamHipError, match="min_axis_km needs axis"):
        dnn.EventFilter(cat, min_axis_km=(300, 300))
    flt = dnn.EventFilter(cat, min_pixels=(3, 0), min_axis_km=(300, 500), axis=axis)
    out = flt(m).cpu().numpy()
    raw = ua.reference(mask, 2, cat.connectivity, cat.wrap, cap, max(H, W), dnn.event_weight_tables(H, W), dnn.axis_link_table(H, W))
    pruned, removed = up.prune(raw["skeleton"], 2, int(cat.wrap), 8)
    assert np.array_equal(axis.raw_skeleton_buffer.cpu().numpy(), raw["skeleton"]) and np.array_equal(axis.raw_table.cpu().numpy(), raw["rows"])
    assert np.array_equal(axis.skeleton_buffer.cpu().numpy(), pruned) and axis.removed().tolist() == removed.tolist() and removed.any()
    labels, _, _, every = ue.catalogue(np.where(mask < 3, mask, 0).astype(np.uint8), 2, cat.connectivity, cat.wrap, *dnn.event_weight_tables(H, W), cap)
    rows = np.stack([ua.stats(pruned[b], labels[b], every[b][:, 0], cap, cat.wrap, axis.link_table) for b in range(2)])
    assert np.array_equal(axis.table.cpu().numpy(), rows)
    # the filter: min_pixels through the catalogue's rows, min_axis_km through the pruned rows; the mask keeps the pixels of kept events
    want, dropped = mask.copy(), 0
    for b in range(2):
        for k, ev in enumerate(every[b][:cap]):
            cls = int(ev[1])
            if ev[2] < (3, 0)[cls - 1] or rows[b, k, 6] < (300000, 500000)[cls - 1]:
                want[b][labels[b] == ev[0] + 1] = 0
                dropped += 1
    assert np.array_equal(out, want) and 0 < dropped == int(flt.counts()[:, :, 1].sum()) < sum(len(e) for e in every)
    assert flt.thresholds()["min_axis_km"] == [300.0, 500.0]
    d = axis.axes()[0][0]
    assert abs(d["spur_km"] - (d["axis_km_unpruned"] - d["axis_km"])) == 0 and d["axis_km"] == rows[0, 0, 6] / 1000.0
