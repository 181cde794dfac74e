"""Neighbourhood verification on the GPU (dc_fss_score of csrc/fss.hip, nn.FractionsSkill, predict.py --fss) against the numpy checker of
tests/util_fss.py.  Everything is an integer: every comparison is equality.  The shapes come from the kernels' own workgroup
(dc_fss_block: the columns TC of a strip, the rows TR of a segment): one frame narrower than a strip and shorter than a segment, with an
odd width that the largest window spans as a whole ring; one of three strips with a ragged last one and three segments with a ragged last
one, with a window taller than a segment and the largest admissible one."""
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
import util_fss as uf  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV = 3, 2
GUARD, SENTINEL = 64, 0x5A
FAMILY = {"fss_rows", "fss_cols", "fss_total"}


@functools.lru_cache(maxsize=None)
def _block():
    cols, rows = C.c_int(0), C.c_int(0)
    assert L.load().dc_fss_block(C.byref(cols), C.byref(rows)) == 0 and cols.value > 1 and rows.value > 1
    return cols.value, rows.value


def _odd_at_most(n):
    return n if n % 2 == 1 else n - 1


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(H, W, windows)"""
    TC, TR = _block()
    if name == "small":                              # narrower than a strip, shorter than a segment
        W = _odd_at_most(min(TC - 1, 37))
        H = min(TR - 1, 23)
        assert W % 2 == 1 and 0 < W < TC and 0 < H < TR
        windows = (1, 3, W if W <= 255 else 255)     # under wrap n = W is the whole ring
    else:                                            # three strips and three segments, the last of each ragged
        W = 2 * TC + 37
        H = 2 * TR + 13
        assert W % 2 == 1 and 2 * TC < W < 3 * TC and 2 * TR < H < 3 * TR
        tall = _odd_at_most(TR + 2)                  # 2 r + 1 > TR: the warm-up spans more than a segment
        largest = _odd_at_most(min(255, W))
        windows = tuple(dict.fromkeys((1, 3, 9) + ((tall,) if tall <= 255 else ()) + (largest,)))
    assert len(set(windows)) == len(windows) and all(n % 2 == 1 and n <= min(W, 255) for n in windows)
    return H, W, windows


def _masks(n, H, W, seed):
    """(pred, truth) uint8 [n, H, W]: block-structured random classes with the values 3 and 255 among the background; the prediction is
    a displaced copy of the labels with noise; foreground touches row 0, row H - 1 and both sides of the seam."""
    rs = np.random.RandomState(seed)
    cell = 5
    coarse = rs.choice(np.asarray([0, 1, 2, 3, 255], np.uint8), size=(n, H // cell + 1, W // cell + 1), p=[0.5, 0.2, 0.2, 0.05, 0.05])
    truth = np.ascontiguousarray(coarse.repeat(cell, 1).repeat(cell, 2)[:, :H, :W])
    truth[:, 0, :4], truth[:, H - 1, W - 4:] = 2, 2
    truth[:, H // 2, 0], truth[:, H // 2, W - 1] = 2, 2
    pred = np.roll(truth, (1, 3), axis=(1, 2))
    noise = rs.rand(n, H, W) < 0.03
    pred[noise] = rs.choice(np.asarray([0, 1, 2], np.uint8), size=int(noise.sum()))
    pred[:, 0, 2:6], pred[:, H - 1, :3], pred[:, H // 3, W - 1] = 2, 2, 2
    return np.ascontiguousarray(pred), truth


@functools.lru_cache(maxsize=None)
def _batch(shape):
    """The standard batch of three: random; random with class 1 absent from BOTH masks (the only (frame, class) without a score); and a
    padding frame, all class 1 on both sides, that must not be read.  Shared and never modified."""
    H, W, _ = _shape(shape)
    pred, truth = _masks(B, H, W, 60 + H)
    pred[1][pred[1] == 1] = 0
    truth[1][truth[1] == 1] = 0
    pred[2], truth[2] = 1, 1
    assert (truth == 3).any() and (truth == 255).any() and (pred == 3).any() and (pred == 255).any()
    for m in (pred[0], truth[0]):
        assert (m[0] != 0).any() and (m[H - 1] != 0).any() and ((m[:, 0] == 1) | (m[:, 0] == 2)).any() and ((m[:, W - 1] == 1) | (m[:, W - 1] == 2)).any()
    pred.setflags(write=False), truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def _reference(shape, wrap, row_range=None):
    """(rows [NV, 2, S, 3], pixels [NV, 2, 2], state) of the standard batch.  Shared and never modified."""
    H, W, windows = _shape(shape)
    pred, truth = _batch(shape)
    rows, pixels = uf.batch_rows(pred[:NV], truth[:NV], windows, wrap, row_range)
    scored = rows[..., 1] + rows[..., 2] > 0                                     # [NV, 2, S]
    assert not scored[1, 0].any() and scored[0].all() and scored[1, 1].all()     # the one intended None, and no other
    rows.setflags(write=False), pixels.setflags(write=False)
    return rows, pixels, uf.totals([(pred[:NV], truth[:NV])], windows, wrap, row_range)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                      # a copy: the shared batches are read-only


def _make(shape, wrap=True, row_range=None, batch=B):
    H, W, windows = _shape(shape)
    return dnn.FractionsSkill(batch, H, W, windows=windows, wrap=wrap, row_range=row_range, device=DEV)


def _assert_frame(fs, rows, pixels, what=""):
    got_rows, got_pixels = (t.cpu().numpy() for t in fs.frame_rows())
    assert got_rows.dtype == np.int64 and got_rows.shape == rows.shape and got_pixels.dtype == np.int64 and got_pixels.shape == pixels.shape, what
    assert np.array_equal(got_pixels, pixels), (what, got_pixels.tolist(), pixels.tolist())
    assert np.array_equal(got_rows, rows), (what, np.argwhere(got_rows != rows)[:6].tolist())


# ------------------------------------------------------------------------------------------------------------------ 1. rows, pixels, totals
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_rows_pixels_and_totals_equal_the_checker(shape, wrap):
    H, W, windows = _shape(shape)
    pred, truth = _batch(shape)
    fs = _make(shape, wrap)
    with served("FractionsSkill") as names:
        assert fs(_dev(pred), _dev(truth), n_valid=NV) is fs
    assert names == ["fss_rows", "fss_cols", "fss_total"]
    rows, pixels, state = _reference(shape, wrap)
    _assert_frame(fs, rows, pixels, f"{shape} wrap={wrap}")
    assert not fs._rows[NV:].any() and not fs._pixels[NV:].any()                 # the padding frame: zero rows
    got = fs.state()
    assert got == state and got["frames"] == NV and all(isinstance(v, int) for v in got["total"][1][0])
    assert fs.result() == uf.decode(state["total"], state["pixels"], NV, windows, H, W)
    scores = dnn.fss_from_rows(fs.frame_rows()[0].cpu().numpy())
    assert scores[1][0] == [None] * len(windows) and all(0.0 <= f <= 1.0 for f in scores[0][0] + scores[0][1] + scores[1][1])
    if shape == "small" and wrap:                                                # the whole ring: F and O do not depend on the column
        assert windows[-1] == W


# ------------------------------------------------------------------------------------------------------------------ 2. mask element sizes
@pytest.mark.parametrize("dtypes", [(np.uint8, np.int64), (np.int32, np.uint8), (np.int64, np.int32)], ids=["u8-i64", "i32-u8", "i64-i32"])
def test_mask_element_sizes_mixed_per_side(dtypes):
    pred, truth = _batch("large")
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
    fs = _make("large")
    fs(_dev(sides[0]), _dev(sides[1]), n_valid=NV)
    rows, pixels, state = _reference("large", True)
    _assert_frame(fs, rows, pixels, str(dtypes))
    assert fs.state() == state


# ------------------------------------------------------------------------------------------------------------------ 3. the row range
def _bands():
    H, _, windows = _shape("large")
    _, TR = _block()
    inside = (3, 3 + TR + 9)                          # strictly inside, two segments, windows reaching out of it at both ends
    assert 0 < inside[0] and inside[1] < H and max(windows) // 2 > inside[0]
    return {"inside": inside, "full": (0, H), "one-row": (H // 2, H // 2 + 1), "last-row": (H - 1, H)}


@pytest.mark.parametrize("band", ["inside", "full", "one-row", "last-row"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
def test_row_range(band, wrap):
    row_range = _bands()[band]
    pred, truth = _batch("large")
    fs = _make("large", wrap, row_range)
    fs(_dev(pred), _dev(truth), n_valid=NV)
    rows, pixels, state = _reference("large", wrap, row_range)
    _assert_frame(fs, rows, pixels, f"{band} wrap={wrap}")
    assert fs.state() == state
    if band != "full":                                # the band selects the centres: the sums differ from the whole frame's
        assert not np.array_equal(rows, _reference("large", wrap)[0])


# ------------------------------------------------------------------------------------------------------------------ 4. the cut into batches
def test_the_cut_into_batches_does_not_matter_and_reset():
    H, W, windows = _shape("large")
    n = 7
    pred, truth = _masks(n, H, W, 7)
    ref = uf.totals([(pred, truth)], windows)
    for batch in (7, 4, 1):
        fs = _make("large", batch=batch)
        for s in range(0, n, batch):
            nv = min(batch, n - s)
            p, t = np.ones((batch, H, W), np.uint8), np.ones((batch, H, W), np.uint8)      # padding: all class 1, wrong if read
            p[:nv], t[:nv] = pred[s:s + nv], truth[s:s + nv]
            fs(_dev(p), _dev(t), n_valid=nv)
        assert fs.state() == ref, f"batch {batch}"
    # two calls on one object: one checker pass over both batches; the frame rows are the last call's
    fs = _make("large")
    first, second = _batch("large"), (pred[:B], truth[:B])
    fs(_dev(first[0]), _dev(first[1]), n_valid=NV)
    fs(_dev(second[0]), _dev(second[1]))
    assert fs.state() == uf.totals([(first[0][:NV], first[1][:NV]), second], windows)
    _assert_frame(fs, *uf.batch_rows(*second, windows), "second call")
    fs.reset()
    zero = fs.state()
    assert zero["frames"] == 0 and zero["pixels"] == [[0, 0], [0, 0]] and not any(v for cls in zero["total"] for win in cls for v in win)
    fs(_dev(first[0]), _dev(first[1]), n_valid=NV)                               # after a reset: the first batch alone
    assert fs.state() == _reference("large", True)[2]
    fs(_dev(first[0]), _dev(first[1]), n_valid=0)                                # nothing valid: zero rows, unchanged totals
    assert fs.state() == _reference("large", True)[2] and fs.frame_rows()[0].shape[0] == 0 and not fs._rows.any() and not fs._pixels.any()


# ------------------------------------------------------------------------------------------------------------------ 5. the carry
def test_the_carry_into_the_high_word():
    pred, truth = _batch("large")
    _, _, state = _reference("large", True)
    fs = _make("large")
    words = torch.zeros_like(fs._total)
    words[1, 2, 1, 0] = -1                                                       # lo = 2^64 - 1
    words[0, 1, 0, 0], words[0, 1, 0, 1] = -(1 << 63), 5                         # lo = 2^63, hi = 5
    fs._total.copy_(words)
    fs(_dev(pred), _dev(truth), n_valid=NV)
    want = [[list(win) for win in cls] for cls in state["total"]]
    assert want[1][2][1] > 0 and want[0][1][0] > 0
    want[1][2][1] += (1 << 64) - 1
    want[0][1][0] += (5 << 64) + (1 << 63)
    got = fs.state()["total"]
    assert got == want
    raw = fs._total.cpu().numpy()
    assert raw[1, 2, 1, 1] == 1 and raw[1, 2, 1, 0] == state["total"][1][2][1] - 1       # (hi, lo) themselves
    assert raw[0, 1, 0, 1] == 5 and raw[0, 1, 0, 0] == state["total"][0][1][0] - (1 << 63)


# ------------------------------------------------------------------------------------------------------------------ 6. guard words
@pytest.mark.parametrize("shape", ["small", "large"])
def test_guard_words_survive(shape):
    pred, truth = _batch(shape)
    fs = _make(shape)
    stores = {}
    for name in ("_rows", "_pixels", "_total", "_total_pixels", "_frames", "_ws"):
        t = getattr(fs, name)
        store = torch.zeros(t.numel() + GUARD, dtype=t.dtype, device=DEV)
        store[t.numel():] = SENTINEL
        stores[name] = store
        setattr(fs, name, store[:t.numel()].view(t.shape))
    guards_ok = lambda: all(bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())  # noqa: E731
    rows, pixels, state = _reference(shape, True)
    for _ in range(2):
        fs(_dev(pred), _dev(truth), n_valid=NV)
        _assert_frame(fs, rows, pixels, "guarded")
        assert guards_ok()
    double = uf.totals([(pred[:NV], truth[:NV])] * 2, _shape(shape)[2])
    assert fs.state() == double
    fs.reset()
    assert guards_ok() and fs.state()["frames"] == 0
    fs(_dev(pred), _dev(truth))                                                  # all three frames: the last words of every buffer
    assert guards_ok() and fs.state() == uf.totals([(pred, truth)], _shape(shape)[2])


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors_raise_and_launch_nothing():
    H, W, windows = _shape("small")
    fs = _make("small")
    pred = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    truth = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    bad_calls = [
        lambda: fs(pred[:, :, :-1].contiguous(), truth),                          # wrong shapes
        lambda: fs(pred, truth[:2]),
        lambda: fs(pred[:, :-1], truth[:, :-1]),
        lambda: fs(pred.permute(0, 2, 1), truth),
        lambda: fs(pred.to(torch.int16), truth),                                  # dtypes
        lambda: fs(pred, truth.float()),
        lambda: fs(pred.bool(), truth),
        lambda: fs(pred.cpu(), truth),                                            # device
        lambda: fs(pred, truth.cpu()),
        lambda: fs(pred, None),
        lambda: fs(pred, truth, n_valid=B + 1),
        lambda: fs(pred, truth, n_valid=-1),
        lambda: fs(torch.zeros((B, W, H), dtype=torch.uint8, device=DEV).permute(0, 2, 1), truth),   # not contiguous
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"windows": (1, 4)}, {"windows": (W + 2,)}, {"windows": (257,)}, {"windows": (0,)}, {"windows": (3, 3)}, {"windows": ()},
                   {"windows": tuple(range(1, 35, 2))}, {"row_range": (2, 2)}, {"row_range": (0, H + 1)}, {"row_range": (-1, 2)}):
            with pytest.raises(L.DeepcamHipError):
                dnn.FractionsSkill(B, H, W, **{"windows": (1, 3), "device": DEV, **kw})
        with pytest.raises(L.DeepcamHipError):
            dnn.FractionsSkill(0, H, W, device=DEV, windows=(1,))
    assert names == []
    state = fs.state()
    assert state["frames"] == 0 and not any(v for cls in state["total"] for win in cls for v in win)
    dnn.FractionsSkill(B, H, W, windows=(W + 2,), wrap=False, device=DEV)        # wider than the frame is fine without wrap


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


def test_predict_cli_with_fss(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(29)
    names = [f"data-2003-01-{d:02d}-00-1.h5" for d in (5, 6, 7)]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    truth = [rs.choice(np.asarray([0, 1, 2], np.int64), size=(H // 8, W // 8), p=[0.6, 0.2, 0.2]).repeat(8, 0).repeat(8, 1) for _ in names]
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
    windows, band = [1, 5, 33], (8, 56)
    out = str(tmp_path / "out")
    args = predict.build_parser().parse_args([*base, "--output_dir", out, "--batch_size", "2", "--fss", "--fss_windows", *map(str, windows),
                                              "--fss_rows", str(band[0]), str(band[1])])
    assert args.verify is True
    with served("predict --fss") as launched:                                    # batches of two and one: a padded last batch
        predict.main(args)
    assert FAMILY <= set(launched)
    got = [_h5_read(os.path.join(out, n), ["prediction", "fss", "fss_pixels", "event_scores"]) for n in names]
    pred = [g["prediction"] for g in got]
    for g, p, t in zip(got, pred, truth):
        rows, pixels = uf.frame_rows(p, t, windows, True, band)
        assert g["fss"].dtype == np.int64 and g["fss"].shape == (2, 3, 3) and np.array_equal(g["fss"], rows)
        assert g["fss_pixels"].dtype == np.int64 and np.array_equal(g["fss_pixels"], pixels)
        assert g["event_scores"] is not None                                     # --fss implies --verify
    state = uf.totals([(np.stack(pred), np.stack(truth))], windows, True, band)
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["fss"] == predict.fss_summary(windows, band, W, state) and summary["fss"]["frames"] == 3
    assert summary["fss"]["windows"] == windows and summary["fss"]["rows"] == list(band) and "event_verification" in summary
    assert state["pixels"][0][1] > 0 and state["pixels"][1][1] > 0
    # without the flag: no datasets, no entry, no launch of the family, and the same predictions byte for byte
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "2", "--fss_windows", "3"])
    with served("predict without --fss") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("fss")]
    assert "fss" not in json.load(open(os.path.join(plain, "summary.json")))
    for n, p in zip(names, pred):
        g = _h5_read(os.path.join(plain, n), ["prediction", "fss", "fss_pixels"])
        assert g["fss"] is None and g["fss_pixels"] is None
        assert g["prediction"].dtype == p.dtype and g["prediction"].tobytes() == p.tobytes()
