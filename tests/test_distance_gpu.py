"""Distance-map verification on the GPU (dc_distance_score of csrc/distance.hip, nn.DistanceSkill, predict.py --distance_skill) against the
numpy checker of tests/util_distance.py, which is not separable.  Everything is an integer: every comparison is equality.  The shapes come
from the kernels' own workgroup (dc_distance_block: the columns TC of a strip, the rows TR of a segment): one frame narrower than a strip
and shorter than a segment, of odd width, whose window is the whole ring; one of three strips with a ragged last one and three segments with
a ragged last one, with a halo longer than a segment, and the same frame at a cap of 5.  The masks are sparse (util_distance.sparse_masks);
tests/test_distance_cpu.py asserts on the checker alone that they fill the far rings and the beyond cell and reach across the seam.
The standard batch of three removes class 1 from its first prediction and from both sides of its second frame, as the rows of an absent
class must be checked; the rings of class 1 in both directions are compared on the unmodified frames of the plain batch."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_distance as ud  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = ud.B, ud.NV
GUARD, SENTINEL = 64, 0x5A
FAMILY = ["dist_vert", "dist_horz", "dist_total"]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                      # a copy: the shared batches are read-only


def _make(shape, wrap=True, row_range=None, batch=B, keep_maps=False):
    H, W, R = ud.shape(shape)
    return dnn.DistanceSkill(batch, H, W, radius=R, wrap=wrap, row_range=row_range, keep_maps=keep_maps, device=DEV)


def _assert_frame(ds, rows, bad, what=""):
    got_rows, got_bad = (t.cpu().numpy() for t in ds.frame_rows())
    assert got_rows.dtype == np.int64 and got_rows.shape == rows.shape and got_bad.dtype == np.int64 and got_bad.shape == bad.shape, what
    assert np.array_equal(got_rows, rows), (what, np.argwhere(got_rows != rows)[:6].tolist())
    assert np.array_equal(got_bad, bad), (what, got_bad.tolist(), bad.tolist())


# ------------------------------------------------------------------------------------------------------------------ 1. rows, totals, maps
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("shape", ["small", "large", "large-r5"])
def test_rows_baddeley_totals_and_maps_equal_the_checker(shape, wrap):
    H, W, R = ud.shape(shape)
    pred, truth = ud.standard_batch(shape)
    ds = _make(shape, wrap, keep_maps=True)
    with served("DistanceSkill") as names:
        assert ds(_dev(pred), _dev(truth), n_valid=NV) is ds
    assert names == FAMILY
    rows, bad, state = ud.reference(shape, wrap)
    _assert_frame(ds, rows, bad, f"{shape} wrap={wrap}")
    assert not ds._rows[NV:].any() and not ds._baddeley[NV:].any()               # the padding frame: not written
    maps = ds.maps()
    assert maps.dtype == torch.uint16 and tuple(maps.shape) == (NV, 2, 2, H, W)
    got_maps, want_maps = maps.cpu().numpy().astype(np.int64), ud.reference_maps(shape, wrap)
    assert np.array_equal(got_maps, want_maps), np.argwhere(got_maps != want_maps)[:6].tolist()
    assert not ds._maps[NV:].cpu().numpy().any()
    got = ds.state()
    assert got == state and got["frames"] == NV and all(isinstance(v, int) for v in got["total"][1][0] + got["baddeley"])
    assert ds.result() == ud.decode(state["total"], state["baddeley"], NV, R, H, W)
    for b in range(NV):                                                          # ring 0 of both directions is |P and T|
        for k in (1, 2):
            both = int(((pred[b] == k) & (truth[b] == k)).sum())
            assert rows[b, k - 1, 0, 0] == rows[b, k - 1, 1, 0] == both
    assert dnn.distance_from_rows(rows, bad, R, H, W) == [ud.decode(ud.totals_of_rows([(rows[b:b + 1], bad[b:b + 1])], R)["total"], bad[b], 1, R, H, W)
                                                          for b in range(NV)]
    plain = _make(shape, wrap)                                                   # without the maps: the same rows
    plain(_dev(pred), _dev(truth), n_valid=NV)
    _assert_frame(plain, rows, bad, "keep_maps=False")
    assert plain.state() == state
    with pytest.raises(L.DeepcamHipError):
        plain.maps()


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("shape", ["large", "large-r5"])
def test_unmodified_frames_both_classes_in_both_directions(shape, wrap):
    pred, truth = ud.plain_batch(shape)
    rows, bad, state = ud.reference(shape, wrap, None, "plain")
    ds = _make(shape, wrap, batch=len(pred), keep_maps=True)
    ds(_dev(pred), _dev(truth))
    _assert_frame(ds, rows, bad, f"plain {shape} wrap={wrap}")
    assert np.array_equal(ds.maps().cpu().numpy().astype(np.int64), ud.reference_maps(shape, wrap, "plain"))
    assert ds.state() == state


# ------------------------------------------------------------------------------------------------------------------ 2. mask element sizes
@pytest.mark.parametrize("dtypes", [(np.uint8, np.int64), (np.int32, np.uint8), (np.int64, np.int32)], ids=["u8-i64", "i32-u8", "i64-i32"])
def test_mask_element_sizes_mixed_per_side(dtypes):
    pred, truth = ud.standard_batch("large")
    sides = []
    for side, (mask, dtype) in enumerate(zip((pred, truth), dtypes)):
        m = mask.astype(dtype)
        if dtype != np.uint8:                         # background whose low byte or low word is a class
            rs = np.random.RandomState(3 + side)
            m[(mask == 0) & (rs.rand(*mask.shape) < 0.5)] = 256 + 1
            m[mask == 255] = -1
            if dtype == np.int64:
                m[mask == 3] = (1 << 32) + 1
                assert (m == (1 << 32) + 1).any()
            assert (m == 257).any() and (m == -1).any()
        sides.append(m)
    ds = _make("large")
    ds(_dev(sides[0]), _dev(sides[1]), n_valid=NV)
    rows, bad, state = ud.reference("large", True)
    _assert_frame(ds, rows, bad, str(dtypes))
    assert ds.state() == state


# ------------------------------------------------------------------------------------------------------------------ 3. the row range
def _bands():
    H, _, R = ud.shape("large")
    _, TR = ud.block()
    inside = (3, 3 + TR + 9)                          # strictly inside, two segments, targets outside it at both ends
    assert 0 < inside[0] and inside[1] < H and R > inside[0]
    return {"inside": inside, "full": (0, H), "one-row": (4, 5), "last-row": (H - 1, H)}     # row 4 holds class 1's pair across the seam


@pytest.mark.parametrize("band", ["inside", "full", "one-row", "last-row"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
def test_row_range(band, wrap):
    row_range = _bands()[band]
    pred, truth = ud.plain_batch("large")
    pred, truth = pred[:B], truth[:B]
    ds = _make("large", wrap, row_range, keep_maps=(band == "inside"))
    ds(_dev(pred), _dev(truth), n_valid=NV)
    rows, bad = (a[:NV] for a in ud.reference("large", wrap, row_range, "plain")[:2])
    _assert_frame(ds, rows, bad, f"{band} wrap={wrap}")
    assert ds.state() == ud.totals_of_rows([(rows, bad)], ud.shape("large")[2])
    assert bad.any() and rows.any()                   # the band holds sources and Baddeley pixels
    if band != "full":                                # the band selects the sources: the rows differ from the whole frame's
        assert not np.array_equal(rows, ud.reference("large", wrap, None, "plain")[0][:NV])
    if band == "inside":                              # the maps are written for all rows
        assert np.array_equal(ds.maps().cpu().numpy().astype(np.int64), ud.reference_maps("large", wrap, "plain")[:NV])


# ------------------------------------------------------------------------------------------------------------------ 4. the cut into batches
def test_the_cut_into_batches_does_not_matter_and_reset():
    H, W, R = ud.shape("large")
    pred, truth = ud.plain_batch("large")
    n = len(pred)
    assert n == 7
    rows, bad, ref = ud.reference("large", True, None, "plain")
    for batch in (7, 4, 1):
        ds = _make("large", batch=batch)
        for s in range(0, n, batch):
            nv = min(batch, n - s)
            p, t = np.ones((batch, H, W), np.uint8), np.ones((batch, H, W), np.uint8)      # padding: all class 1, wrong if read
            p[:nv], t[:nv] = pred[s:s + nv], truth[s:s + nv]
            ds(_dev(p), _dev(t), n_valid=nv)
        assert ds.state() == ref, f"batch {batch}"
    # two calls on one object: the totals of both batches; the frame rows are the last call's
    ds = _make("large")
    first = ud.standard_batch("large")
    std_rows, std_bad, std_state = ud.reference("large", True)
    ds(_dev(first[0]), _dev(first[1]), n_valid=NV)
    ds(_dev(pred[:B]), _dev(truth[:B]))
    assert ds.state() == ud.totals_of_rows([(std_rows, std_bad), (rows[:B], bad[:B])], R)
    _assert_frame(ds, rows[:B], bad[:B], "second call")
    ds.reset()
    zero = ds.state()
    assert zero["frames"] == 0 and zero["baddeley"] == [0, 0] and not any(v for cls in zero["total"] for d in cls for v in d)
    ds(_dev(first[0]), _dev(first[1]), n_valid=NV)                               # after a reset: the first batch alone
    assert ds.state() == std_state
    before = ds._rows.clone()
    with served("n_valid = 0") as names:
        ds(_dev(first[0]), _dev(first[1]), n_valid=0)                            # nothing valid: nothing read, written or launched
    assert names == [] and ds.state() == std_state and ds.frame_rows()[0].shape[0] == 0 and torch.equal(ds._rows, before)


# ------------------------------------------------------------------------------------------------------------------ 5. the carry
def test_the_carry_into_the_baddeley_high_word():
    pred, truth = ud.standard_batch("large")
    _, _, state = ud.reference("large", True)
    ds = _make("large")
    words = torch.zeros_like(ds._total_baddeley)
    words[1, 0] = -1                                                             # class 2: lo = 2^64 - 1
    words[0, 0], words[0, 1] = -(1 << 63), 5                                     # class 1: lo = 2^63, hi = 5
    ds._total_baddeley.copy_(words)
    ds(_dev(pred), _dev(truth), n_valid=NV)
    want = list(state["baddeley"])
    assert want[0] > 0 and want[1] > 0
    want[1] += (1 << 64) - 1
    want[0] += (5 << 64) + (1 << 63)
    assert ds.state()["baddeley"] == want
    raw = ds._total_baddeley.cpu().numpy()
    assert raw[1, 1] == 1 and raw[1, 0] == state["baddeley"][1] - 1              # (hi, lo) themselves
    assert raw[0, 1] == 5 and raw[0, 0] == state["baddeley"][0] - (1 << 63)


# ------------------------------------------------------------------------------------------------------------------ 6. guard words
@pytest.mark.parametrize("shape", ["small", "large"])
def test_guard_words_survive(shape):
    H, W, R = ud.shape(shape)
    pred, truth = ud.standard_batch(shape)
    ds = _make(shape, keep_maps=True)
    stores = {}
    for name in ("_rows", "_baddeley", "_total", "_total_baddeley", "_frames", "_ws", "_maps"):
        t = getattr(ds, name)
        raw = torch.int16 if t.dtype == torch.uint16 else t.dtype                # the guard is compared in a type every operator knows
        store = torch.zeros(t.numel() + GUARD, dtype=raw, device=DEV)
        store[t.numel():] = SENTINEL
        stores[name] = store
        setattr(ds, name, store[:t.numel()].view(t.dtype).view(t.shape))
    guards_ok = lambda: all(bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())  # noqa: E731
    rows, bad, state = ud.reference(shape, True)
    for _ in range(2):
        ds(_dev(pred), _dev(truth), n_valid=NV)
        _assert_frame(ds, rows, bad, "guarded")
        assert guards_ok()
    assert ds.state() == ud.totals_of_rows([(rows, bad)] * 2, R)
    assert not stores["_maps"][NV * 4 * H * W:-GUARD].any() and not stores["_rows"][NV * 4 * (R + 4):-GUARD].any()   # frames >= n_valid: untouched
    ds.reset()
    assert guards_ok() and ds.state()["frames"] == 0
    ds(_dev(pred), _dev(truth))                                                  # all three frames: the last words of every buffer
    padding = np.zeros((1, 2, 2, R + 4), np.int64)                               # all class 1 on both sides: every pixel a source in ring 0
    padding[0, 0, :, 0] = H * W
    assert guards_ok() and ds.state() == ud.totals_of_rows([(rows, bad), (padding, np.zeros((1, 2), np.int64))], R)
    assert (ds.maps()[B - 1].cpu().numpy()[:, 0] == 0).all()                     # the padding frame is all class 1 on both sides


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors_raise_and_launch_nothing():
    H, W, R = ud.shape("small")
    ds = _make("small")
    pred = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    truth = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    bad_calls = [
        lambda: ds(pred[:, :, :-1].contiguous(), truth),                          # wrong shapes
        lambda: ds(pred, truth[:2]),
        lambda: ds(pred[:, :-1], truth[:, :-1]),
        lambda: ds(pred.permute(0, 2, 1), truth),
        lambda: ds(pred.to(torch.int16), truth),                                  # dtypes
        lambda: ds(pred, truth.float()),
        lambda: ds(pred.bool(), truth),
        lambda: ds(pred.cpu(), truth),                                            # device
        lambda: ds(pred, truth.cpu()),
        lambda: ds(pred, None),
        lambda: ds(pred, truth, n_valid=B + 1),
        lambda: ds(pred, truth, n_valid=-1),
        lambda: ds(torch.zeros((B, W, H), dtype=torch.uint8, device=DEV).permute(0, 2, 1), truth),   # not contiguous
        lambda: ds.maps(),                                                        # without keep_maps
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"radius": 0}, {"radius": 128}, {"radius": R + 1}, {"row_range": (2, 2)}, {"row_range": (0, H + 1)}, {"row_range": (-1, 2)}):
            with pytest.raises(L.DeepcamHipError):
                dnn.DistanceSkill(B, H, W, **{"radius": 3, "device": DEV, **kw})
        with pytest.raises(L.DeepcamHipError):
            dnn.DistanceSkill(0, H, W, radius=3, device=DEV)
    assert names == []
    state = ds.state()
    assert state["frames"] == 0 and state["baddeley"] == [0, 0] and not any(v for cls in state["total"] for d in cls for v in d)
    dnn.DistanceSkill(B, H, W, radius=R + 1, wrap=False, device=DEV)             # wider than the frame is fine without wrap


# ------------------------------------------------------------------------------------------------------------------ 8. driver
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


def test_predict_cli_with_distance_skill(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(31)
    names = [f"data-2003-01-{d:02d}-00-1.h5" for d in (5, 6, 7)]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    truth = [rs.choice(np.asarray([0, 1, 2], np.int64), size=(H // 8, W // 8), p=[0.8, 0.1, 0.1]).repeat(8, 0).repeat(8, 1) for _ in names]
    for name, d, t in zip(names, fields, truth):
        _h5_write(os.path.join(root, name), {"climate/data": d, "climate/labels_0": t})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "fp32", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2"]
    R, band = 12, (8, 56)
    out = str(tmp_path / "out")
    args = predict.build_parser().parse_args([*base, "--output_dir", out, "--batch_size", "2", "--distance_skill", "--distance_radius", str(R),
                                              "--distance_rows", str(band[0]), str(band[1])])
    assert args.verify is True
    with served("predict --distance_skill") as launched:                         # batches of two and one: a padded last batch
        predict.main(args)
    assert set(FAMILY) <= set(launched)
    got = [_h5_read(os.path.join(out, n), ["prediction", "distance", "distance_baddeley", "event_scores"]) for n in names]
    pred = [g["prediction"] for g in got]
    all_rows, all_bad = [], []
    for g, p, t in zip(got, pred, truth):
        rows, bad = ud.frame_rows(p, t, R, True, band)
        assert g["distance"].dtype == np.int64 and g["distance"].shape == (2, 2, R + 4) and np.array_equal(g["distance"], rows)
        assert g["distance_baddeley"].dtype == np.int64 and np.array_equal(g["distance_baddeley"], bad)
        assert g["event_scores"] is not None                                     # the flag implies --verify
        all_rows.append(rows), all_bad.append(bad)
    state = ud.totals_of_rows([(np.stack(all_rows), np.stack(all_bad))], R)
    summary = json.load(open(os.path.join(out, "summary.json")))
    entry = summary["distance_skill"]
    assert entry == predict.distance_summary(R, True, band, H, W, state) and entry["frames"] == 3
    assert entry["radius"] == R and entry["rows"] == list(band) and entry["wrap"] is True and "event_verification" in summary
    assert sum(state["total"][0][0][:R + 2]) > 0 and sum(state["total"][1][0][:R + 2]) > 0
    # without the flag: no datasets, no entry, no launch of the family, and the same predictions byte for byte
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "2", "--distance_radius", "3"])
    with served("predict without --distance_skill") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("dist_")]
    assert "distance_skill" not in json.load(open(os.path.join(plain, "summary.json")))
    for n, p in zip(names, pred):
        g = _h5_read(os.path.join(plain, n), ["prediction", "distance", "distance_baddeley"])
        assert g["distance"] is None and g["distance_baddeley"] is None
        assert g["prediction"].dtype == p.dtype and g["prediction"].tobytes() == p.tobytes()
