"""Displacement verification on the GPU (dc_displacement_score of csrc/displacement.hip, nn.DisplacementSkill, predict.py --displacement)
against the numpy checker of tests/util_displacement.py, which packs no bits.  Everything is an integer: every comparison is equality.  The
shapes come from the kernels' own constants (dc_displacement_block: the pixels of a word, the label rows of a segment): one frame narrower
than a word and shorter than a segment whose window is the whole ring; one of two full words; one of eight words and 37 tail bits, four
segments and a ragged fifth, with two waves of dx; and the same frame with a small window.  The masks are sparse ellipses
(util_displacement.sparse_frames); tests/test_displacement_cpu.py asserts on the checker alone that every class of the plain frames has a
unique non-zero best shift, that hits lie across the seam, that pixels are lost over a pole, and that the standard batch holds the tie and
a class absent on one side."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_displacement as ud  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = ud.B, ud.NV
GUARD, SENTINEL = 64, 0x5A
FAMILY = ["disp_pack", "disp_corr", "disp_best", "disp_total"]
BUFFERS = ("_rows", "_pixels", "_best", "_total", "_total_pixels", "_frames", "_ws")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                      # a copy: the shared batches are read-only


def _make(name, band="full", batch=B):
    H, W, R = ud.shape(name)
    return dnn.DisplacementSkill(batch, H, W, radius=R, row_range=ud.bands(name)[band], device=DEV)


def _assert_frame(ds, rows, pixels, best, what=""):
    got = [t.cpu().numpy() for t in ds.frame_rows()]
    for g, want, part in zip(got, (rows, pixels, best), ("rows", "pixels", "best")):
        assert g.dtype == np.int64 and g.shape == want.shape, (what, part, g.shape, want.shape)
        assert np.array_equal(g, want), (what, part, np.argwhere(g != want)[:6].tolist())


def _zero_state(state):
    return state["frames"] == 0 and state["pixels"] == [[0, 0], [0, 0]] and not any(v for cls in state["total"] for row in cls for v in row)


# ------------------------------------------------------------------------------------------------------------------ 1. tables, best, totals
@pytest.mark.parametrize("band", ["full", "interior", "top", "one-row"])
@pytest.mark.parametrize("name", ud.SHAPES)
def test_rows_pixels_best_and_totals_equal_the_checker(name, band):
    H, W, R = ud.shape(name)
    pred, truth = ud.standard_batch(name)
    ds = _make(name, band)
    with served("DisplacementSkill") as names:
        assert ds(_dev(pred), _dev(truth), n_valid=NV) is ds
    assert names == FAMILY                                                       # exactly the four, in order
    rows, pixels, best, state = ud.reference(name, band)
    _assert_frame(ds, rows, pixels, best, f"{name} {band}")
    assert not ds._rows[NV:].any() and not ds._pixels[NV:].any() and not ds._best[NV:].any()     # the padding frame: not written
    got = ds.state()
    assert got == state and got["frames"] == NV and all(isinstance(v, int) for v in got["total"][1][0] + got["pixels"][0])
    row_range = ud.bands(name)[band]
    assert ds.result() == ud.decode(state["total"], state["pixels"], NV, R, H, W, row_range)
    surface = ds.result(surface=True)["class_2"]["csi_surface"]
    assert np.array_equal(surface, ud.csi_surface(state["total"][1], state["pixels"][1][1], R), equal_nan=True)
    assert dnn.displacement_from_rows(rows, pixels, R, H, W, row_range) == [
        ud.decode(rows[b].tolist(), pixels[b].tolist(), 1, R, H, W, row_range) for b in range(NV)]


@pytest.mark.parametrize("name", ud.SHAPES)
def test_seven_unmodified_frames(name):
    pred, truth, planted = ud.plain_batch(name)
    rows, pixels, best, state = ud.reference(name, "full", "plain")
    ds = _make(name, batch=len(pred))
    ds(_dev(pred), _dev(truth))
    _assert_frame(ds, rows, pixels, best, f"plain {name}")
    assert ds.state() == state
    assert ds.frame_rows()[2][:, :, :2].cpu().tolist() == [[list(s) for s in frame] for frame in planted]    # the planted shifts, found


# ------------------------------------------------------------------------------------------------------------------ 2. mask element sizes
@pytest.mark.parametrize("dtypes", [(np.uint8, np.int64), (np.int32, np.uint8), (np.int64, np.int32)], ids=["u8-i64", "i32-u8", "i64-i32"])
def test_mask_element_sizes_mixed_per_side(dtypes):
    pred, truth = ud.standard_batch("large-r5")
    sides = []
    for side, (mask, dtype) in enumerate(zip((pred, truth), dtypes)):
        m = mask.astype(dtype)
        if dtype != np.uint8:                         # background whose low byte or low word is a class
            rs = np.random.RandomState(3 + side)
            m[(mask == 0) & (rs.rand(*mask.shape) < 0.5)] = 256 + 1
            m[mask == 255] = -1
            if dtype == np.int64:
                m[mask == 3] = (1 << 32) + 2
                assert (m == (1 << 32) + 2).any()
            assert (m == 257).any() and (m == -1).any()
        sides.append(m)
    ds = _make("large-r5")
    ds(_dev(sides[0]), _dev(sides[1]), n_valid=NV)
    rows, pixels, best, state = ud.reference("large-r5")
    _assert_frame(ds, rows, pixels, best, str(dtypes))
    assert ds.state() == state


# ------------------------------------------------------------------------------------------------------------------ 3. dense frames
@pytest.mark.parametrize("name", ["large-r5", "small"])
def test_uniform_random_dense_frames_against_the_shift_algorithm(name):
    H, W, R = ud.shape(name)
    pred, truth = ud.dense_frames(2, H, W, 17)
    band = ud.bands(name)["interior"]
    for row_range in (None, band):
        ds = dnn.DisplacementSkill(2, H, W, radius=R, row_range=row_range, device=DEV)
        ds(_dev(pred), _dev(truth))
        rows, pixels, best = ud.batch_rows(pred, truth, R, row_range, ud.table_by_shifts)
        assert rows[:, :, R - 1:R + 2, :2 * R + 1].min() > 0                     # dense: no label word is skipped, every dx has hits
        _assert_frame(ds, rows, pixels, best, f"dense {name} {row_range}")
        assert ds.state() == ud.totals_of_rows([(rows, pixels)], R)


# ------------------------------------------------------------------------------------------------------------------ 4. the symmetry
@pytest.mark.parametrize("name", ["small", "large"])
def test_swapping_the_sides_mirrors_the_table(name):
    R = ud.shape(name)[2]
    S = 2 * R + 1
    pred, truth, _ = ud.plain_batch(name)
    ds = _make(name, batch=len(pred))
    a, pa, _ = (t.clone() for t in ds(_dev(pred), _dev(truth)).frame_rows())
    b, pb, _ = ds(_dev(truth), _dev(pred)).frame_rows()
    assert a[..., :S].any() and torch.equal(a[..., :S], b[..., :S].flip(2, 3)) and torch.equal(pa, pb.flip(2))


# ------------------------------------------------------------------------------------------------------------------ 5. the cut into batches
def test_the_cut_into_batches_does_not_matter_and_reset():
    H, W, R = ud.shape("large")
    pred, truth, _ = ud.plain_batch("large")
    n = len(pred)
    assert n == 7
    rows, pixels, best, ref = ud.reference("large", "full", "plain")
    for batch in (7, 4, 1):
        ds = _make("large", batch=batch)
        for s in range(0, n, batch):
            nv = min(batch, n - s)
            p, t = np.ones((batch, H, W), np.uint8), np.ones((batch, H, W), np.uint8)      # padding: all class 1, wrong if read
            p[:nv], t[:nv] = pred[s:s + nv], truth[s:s + nv]
            ds(_dev(p), _dev(t), n_valid=nv)
        assert ds.state() == ref, f"batch {batch}"
        _assert_frame(ds, rows[n - nv:], pixels[n - nv:], best[n - nv:], f"the last call of batch {batch}")
    # two calls on one object: the totals of both batches; the frame rows are the last call's
    ds = _make("large")
    first = ud.standard_batch("large")
    std = ud.reference("large")
    ds(_dev(first[0]), _dev(first[1]), n_valid=NV)
    ds(_dev(pred[:B]), _dev(truth[:B]))
    assert ds.state() == ud.totals_of_rows([std, (rows[:B], pixels[:B])], R)
    _assert_frame(ds, rows[:B], pixels[:B], best[:B], "second call")
    ds.reset()
    assert _zero_state(ds.state())
    ds(_dev(first[0]), _dev(first[1]), n_valid=NV)                               # after a reset: the first batch alone
    assert ds.state() == std[3]
    before = [getattr(ds, name).clone() for name in BUFFERS]
    with served("n_valid = 0") as names:
        ds(_dev(first[0]), _dev(first[1]), n_valid=0)                            # nothing valid: nothing read, written or launched
    assert names == [] and ds.state() == std[3] and ds.frame_rows()[0].shape[0] == 0
    assert all(torch.equal(getattr(ds, name), old) for name, old in zip(BUFFERS, before))


# ------------------------------------------------------------------------------------------------------------------ 6. guard words
@pytest.mark.parametrize("name", ["small", "word", "large"])
def test_guard_words_survive(name):
    H, W, R = ud.shape(name)
    S = 2 * R + 1
    pred, truth = ud.standard_batch(name)
    ds = _make(name)
    assert ds._ws.numel() * 8 == L.load().dc_displacement_workspace(B, H, W, R)  # the workspace is exactly what the library asks for
    stores = {}
    for name_ in BUFFERS:
        t = getattr(ds, name_)
        store = torch.zeros(t.numel() + GUARD, dtype=t.dtype, device=DEV)
        store[t.numel():] = SENTINEL
        stores[name_] = store
        setattr(ds, name_, store[:t.numel()].view(t.shape))
    guards_ok = lambda: all(bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())  # noqa: E731
    rows, pixels, best, state = ud.reference(name)
    for _ in range(2):
        ds(_dev(pred), _dev(truth), n_valid=NV)
        _assert_frame(ds, rows, pixels, best, "guarded")
        assert guards_ok()
    assert ds.state() == ud.totals_of_rows([(rows, pixels)] * 2, R)
    for name_, cells in (("_rows", 2 * S * (S + 1)), ("_pixels", 4), ("_best", 8)):                # frames >= n_valid: untouched
        assert not stores[name_][NV * cells:-GUARD].any()
    ds.reset()
    assert guards_ok() and _zero_state(ds.state())
    ds(_dev(pred), _dev(truth))                                                  # all four frames: the last words of every buffer
    padding = np.zeros((1, 2, S, S + 1), np.int64)                               # all class 1 on both sides: every pixel hits under every shift
    for dy in range(-R, R + 1):
        padding[0, 0, dy + R, :] = (H - abs(dy)) * W if abs(dy) < H else 0
    assert guards_ok() and ds.state() == ud.totals_of_rows([(rows, pixels), (padding, np.asarray([[[H * W, H * W], [0, 0]]]))], R)
    assert ds.frame_rows()[2][B - 1].cpu().tolist() == [[0, 0, H * W, H * W], [0, 0, 0, 0]]


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
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"radius": 0}, {"radius": 64}, {"radius": R + 1}, {"row_range": (2, 2)}, {"row_range": (0, H + 1)}, {"row_range": (-1, 2)}):
            with pytest.raises(L.DeepcamHipError):
                dnn.DisplacementSkill(B, H, W, **{"radius": 3, "device": DEV, **kw})
        with pytest.raises(L.DeepcamHipError):
            dnn.DisplacementSkill(0, H, W, radius=3, device=DEV)
        # the C entry point itself, with real buffers: refused before anything is launched
        args = lambda **kw: [kw.get(k, v) for k, v in (  # noqa: E731
            ("B", B), ("n_valid", B), ("H", H), ("W", W), ("pred", L.dptr(pred)), ("pred_bytes", 1), ("truth", L.dptr(truth)), ("truth_bytes", 8),
            ("R", R), ("row0", 0), ("row1", H), ("rows", L.dptr(ds._rows)), ("pixels", L.dptr(ds._pixels)), ("best", L.dptr(ds._best)),
            ("total", L.dptr(ds._total)), ("total_pixels", L.dptr(ds._total_pixels)), ("frames", L.dptr(ds._frames)), ("workspace", L.dptr(ds._ws)),
            ("stream", L.stream_ptr()))]
        for kw in ({"R": R + 1}, {"R": 0}, {"row1": H + 1}, {"row0": 3, "row1": 3}, {"n_valid": B + 1}, {"pred_bytes": 2}, {"workspace": None},
                   {"best": None}, {"truth": truth.data_ptr() + 4}):
            with pytest.raises(L.DeepcamHipError):
                L.call("dc_displacement_score", *args(**kw))
    assert names == []
    assert _zero_state(ds.state())


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


def test_predict_cli_with_displacement(tmp_path):
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
    R, band = 6, (8, 56)
    S = 2 * R + 1
    out = str(tmp_path / "out")
    args = predict.build_parser().parse_args([*base, "--output_dir", out, "--batch_size", "2", "--displacement", "--displacement_radius", str(R),
                                              "--displacement_rows", str(band[0]), str(band[1])])
    assert args.verify is True
    with served("predict --displacement") as launched:                           # batches of two and one: a padded last batch
        predict.main(args)
    assert set(FAMILY) <= set(launched)
    datasets = ["prediction", "displacement", "displacement_pixels", "displacement_best", "event_scores"]
    got = [_h5_read(os.path.join(out, n), datasets) for n in names]
    pred = [g["prediction"] for g in got]
    all_rows, all_pixels, all_best = [], [], []
    for g, p, t in zip(got, pred, truth):
        rows, pixels = ud.table_by_pairs(p, t, R, band)
        best = np.asarray([ud.best_of(rows[k], R) for k in range(2)], np.int64)
        for key, want, dims in (("displacement", rows, (2, S, S + 1)), ("displacement_pixels", pixels, (2, 2)), ("displacement_best", best, (2, 4))):
            assert g[key].dtype == np.int64 and g[key].shape == dims and np.array_equal(g[key], want), key
        assert g["event_scores"] is not None                                     # the flag implies --verify
        all_rows.append(rows), all_pixels.append(pixels), all_best.append(best)
    state = ud.totals_of_rows([(np.stack(all_rows), np.stack(all_pixels))], R)
    summary = json.load(open(os.path.join(out, "summary.json")))
    entry = summary["displacement"]
    assert entry == predict.displacement_summary(R, band, H, W, state, np.stack(all_best)) and entry["frames"] == 3
    assert entry["radius"] == R and entry["rows"] == list(band) and "event_verification" in summary
    for k in (1, 2):
        assert {n: v for n, v in entry[f"class_{k}"].items() if n != "frame_shifts"} == \
            ud.decode(state["total"], state["pixels"], 3, R, H, W, band)[f"class_{k}"]
    assert state["pixels"][0][1] > 0 and state["pixels"][1][1] > 0
    # without the flag: the namespace and the outputs of before -- no datasets, no entry, no launch, the same predictions byte for byte
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "2", "--displacement_radius", "3"])
    assert not hasattr(args, "displacement") and args.verify is False
    with served("predict without --displacement") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("disp_")]
    plain_summary = json.load(open(os.path.join(plain, "summary.json")))
    assert "displacement" not in plain_summary and not [r for r in plain_summary["files"] if "displacement_best" in r]
    for n, p in zip(names, pred):
        g = _h5_read(os.path.join(plain, n), ["prediction", "displacement", "displacement_pixels", "displacement_best"])
        assert g["displacement"] is None and g["displacement_pixels"] is None and g["displacement_best"] is None
        assert g["prediction"].dtype == p.dtype and g["prediction"].tobytes() == p.tobytes()
