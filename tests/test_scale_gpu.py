"""Scale-separation verification on the GPU (dc_scale_score of csrc/scale.hip, nn.ScaleSkill, predict.py --scale_skill) against the numpy
checker of tests/util_scale.py.  Everything is an integer: every comparison is equality.  The shapes come from the kernel's own constant
(dc_scale_block: the 64 x 64 workgroup tile): one partial tile; two tiles and 8 columns with a full band and a band of 24 rows; a frame
whose tile T is the workgroup tile; a band that starts at row 37 with T = 128, which takes scale_coarse; and T = 256 with origins on both
sides of a tile's edge, plus frames full of a class, whose 256 x 256 blocks sum to 2^16 and square to 2^32.  The masks are sparse ellipses
(util_scale.standard_batch); tests/test_scale_cpu.py asserts on the checker alone that every class carries error at every level, that the
origins differ, that a block lies across the seam and that the full frames reach both traps."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_scale as us  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = us.B, us.NV
GUARD, SENTINEL = 64, 0x5A
BUFFERS = ("_rows", "_pixels", "_total", "_total_pixels", "_frames", "_ws", "_origins")
DTYPES = [(np.uint8, np.int64), (np.int32, np.uint8), (np.int64, np.int32), (np.uint8, np.uint8), (np.int64, np.int64), (np.int32, np.int32)]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                      # a copy: the shared batches are read-only


def _family(levels):
    return ["scale_sums", "scale_coarse", "scale_total"] if levels > 6 else ["scale_sums", "scale_total"]


def _make(name, band, batch=B):
    H, W, n, origins = us.shape(name)
    return dnn.ScaleSkill(batch, H, W, levels=n, origins=origins, row_range=us.SHAPES[name][4][band], device=DEV)


def _widen(mask, dtype, seed):
    """the mask in another element size, its background partly replaced by values whose low byte or low word is a class"""
    m = mask.astype(dtype)
    if dtype != np.uint8:
        rs = np.random.RandomState(seed)
        m[(mask == 0) & (rs.rand(*mask.shape) < 0.5)] = 256 + 1
        m[(mask == 0) & (rs.rand(*mask.shape) < 0.1)] = -1
        if dtype == np.int64:
            m[mask == 3] = (1 << 32) + 2
        assert (m == 257).any() and (m == -1).any()
    return m


def _assert_frame(ss, rows, pixels, what=""):
    got = [t.cpu().numpy() for t in ss.frame_rows()]
    for g, want, part in zip(got, (rows, pixels), ("rows", "pixels")):
        assert g.dtype == np.int64 and g.shape == want.shape, (what, part, g.shape, want.shape)
        assert np.array_equal(g, want), (what, part, np.argwhere(g != want)[:6].tolist())


def _zero_state(state):
    return state["frames"] == 0 and state["pixels"] == [[0, 0], [0, 0]] and not np.asarray(state["total"], dtype=object).any()


# ------------------------------------------------------------------------------------------------------------------ 1. rows, pixels, totals
@pytest.mark.parametrize("case", range(len(us.CASES)), ids=[f"{n}-{b}" for n, b in us.CASES])
def test_rows_pixels_totals_and_result_equal_the_checker(case):
    name, band = us.CASES[case]
    H, W, n, origins = us.shape(name)
    r0, r1 = us.band_of(name, band)
    pred, truth = us.standard_batch(name)
    dp, dt = DTYPES[case % len(DTYPES)]               # the element sizes mixed per side
    ss = _make(name, band)
    with served("ScaleSkill") as names:
        assert ss(_dev(_widen(pred, dp, 3)), _dev(_widen(truth, dt, 4)), n_valid=NV) is ss
    assert names == _family(n)                                                   # scale_coarse only where L > 6
    rows, pixels, state = us.reference(name, band)
    _assert_frame(ss, rows, pixels, f"{name} {band}")
    assert not ss._rows[NV:].any() and not ss._pixels[NV:].any()                 # the padding frame: not written
    got = ss.state()
    assert got == state and got["frames"] == NV and all(isinstance(v, int) for v in got["total"][1][0][n] + got["pixels"][0])
    assert ss.result() == us.decode(state["total"], state["pixels"], NV, n, r1 - r0, W, origins)
    assert dnn.scale_from_rows(rows, pixels, n, r1 - r0, W, origins) == [
        us.decode(rows[b].tolist(), pixels[b].tolist(), 1, n, r1 - r0, W, origins) for b in range(NV)]


@pytest.mark.parametrize("case", range(len(us.CASES)), ids=[f"{n}-{b}" for n, b in us.CASES])
def test_level_0_equals_the_fractions_skill_of_window_1(case):
    name, band = us.CASES[case]
    H, W, n, origins = us.shape(name)
    pred, truth = us.standard_batch(name)
    p, t = _dev(pred), _dev(truth.astype(np.int32))
    ss = _make(name, band)
    fs = dnn.FractionsSkill(B, H, W, windows=(1,), row_range=us.SHAPES[name][4][band], device=DEV)
    rows, pixels = ss(p, t, n_valid=NV).frame_rows()
    frows, fpixels = fs(p, t, n_valid=NV).frame_rows()                           # the same device tensors
    assert frows.shape == (NV, 2, 1, 3) and frows.any()
    for o in range(len(origins)):
        assert torch.equal(rows[:, :, o, 0, :], frows[:, :, 0, :]), o            # the level-0 triple of every origin
    assert torch.equal(pixels, fpixels)
    a, b = ss.state(), fs.state()
    assert [[a["total"][k][o][0] for o in range(len(origins))] for k in range(2)] == [[b["total"][k][0]] * len(origins) for k in range(2)]
    assert a["pixels"] == b["pixels"] and a["frames"] == b["frames"] == NV


def test_full_frames_reach_2_to_16_and_2_to_32():
    H, W, n, origins = us.shape("deep")
    pred, truth = us.full_batch("deep")
    rows, pixels, state = us.reference("deep", "full", "full")
    ss = _make("deep", "full", batch=2)
    for dtype in (np.uint8, np.int64):
        ss.reset()
        ss(_dev(pred.astype(dtype)), _dev(truth))
        _assert_frame(ss, rows, pixels, "full frames")
        assert ss.state() == state
    assert ss.frame_rows()[0][0, 0, 0, 8].tolist() == [0, 2 << 32, 2 << 32]


# ------------------------------------------------------------------------------------------------------------------ 2. the cut into batches
@pytest.mark.parametrize("name,band", [("two-tiles", "band"), ("coarse", "band")])
def test_the_cut_into_batches_does_not_matter_and_reset(name, band):
    H, W, n, origins = us.shape(name)
    pred, truth = us.plain_batch(name)
    count = len(pred)
    assert count == 7
    rows, pixels, ref = us.reference(name, band, "plain")
    for batch in (7, 4, 1):
        ss = _make(name, band, batch=batch)
        for s in range(0, count, batch):
            nv = min(batch, count - s)
            p, t = np.ones((batch, H, W), np.uint8), np.full((batch, H, W), 2, np.uint8)     # padding: wrong if read
            p[:nv], t[:nv] = pred[s:s + nv], truth[s:s + nv]
            ss(_dev(p), _dev(t), n_valid=nv)
        assert ss.state() == ref, f"batch {batch}"
        _assert_frame(ss, rows[count - nv:], pixels[count - nv:], f"the last call of batch {batch}")
    # two calls on one object: the totals of both batches; the frame rows are the last call's
    ss = _make(name, band)
    first = us.standard_batch(name)
    std = us.reference(name, band)
    ss(_dev(first[0]), _dev(first[1]), n_valid=NV)
    ss(_dev(pred[:B]), _dev(truth[:B]))
    assert ss.state() == us.totals_of_rows([std[:2], (rows[:B], pixels[:B])], n, len(origins))
    _assert_frame(ss, rows[:B], pixels[:B], "second call")
    ss.reset()
    assert _zero_state(ss.state())
    ss(_dev(first[0]), _dev(first[1]), n_valid=NV)                               # after a reset: the first batch alone
    assert ss.state() == std[2]
    before = [getattr(ss, b).clone() for b in BUFFERS]
    with served("n_valid = 0") as names:
        ss(_dev(first[0]), _dev(first[1]), n_valid=0)                            # nothing valid: nothing read, written or launched
    assert names == [] and ss.state() == std[2] and ss.frame_rows()[0].shape[0] == 0
    assert all(torch.equal(getattr(ss, b), old) for b, old in zip(BUFFERS, before))


# ------------------------------------------------------------------------------------------------------------------ 3. guard words
def _guarded(ss):
    stores = {}
    for b in BUFFERS:
        t = getattr(ss, b)
        store = torch.zeros(t.numel() + GUARD, dtype=t.dtype, device=DEV)
        store[:t.numel()] = t.reshape(-1)
        store[t.numel():] = SENTINEL
        stores[b] = store
        setattr(ss, b, store[:t.numel()].view(t.shape))
    return stores, lambda: all(bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values())


@pytest.mark.parametrize("name,band", [("partial", "full"), ("two-tiles", "band"), ("coarse", "band"), ("deep", "full")])
def test_guard_words_survive(name, band):
    H, W, n, origins = us.shape(name)
    O = len(origins)
    r0, r1 = us.band_of(name, band)
    pred, truth = us.standard_batch(name)
    ss = _make(name, band)
    assert ss._ws.numel() * 4 == L.load().dc_scale_workspace(B, H, W, n, O)      # the workspace is exactly what the library asks for
    stores, guards_ok = _guarded(ss)
    rows, pixels, state = us.reference(name, band)
    for _ in range(2):
        ss(_dev(pred), _dev(truth), n_valid=NV)
        _assert_frame(ss, rows, pixels, "guarded")
        assert guards_ok()
    assert ss.state() == us.totals_of_rows([(rows, pixels)] * 2, n, O)
    for b, cells in (("_rows", 2 * O * (n + 1) * 3), ("_pixels", 4)):            # frames >= n_valid: untouched
        assert not stores[b][NV * cells:-GUARD].any()
    ss.reset()
    assert guards_ok() and _zero_state(ss.state())
    ss(_dev(pred), _dev(truth))                                                  # all four frames: the last words of every buffer
    area = (r1 - r0) * W                                                         # the padding frame: all class 1 on both sides
    padding = np.zeros((1, 2, O, n + 1, 3), np.int64)
    padding[0, 0, :, :, 1] = padding[0, 0, :, :, 2] = [area * 4 ** j for j in range(n + 1)]
    assert guards_ok() and ss.state() == us.totals_of_rows([(rows, pixels), (padding, np.asarray([[[area, area], [0, 0]]]))], n, O)


# ------------------------------------------------------------------------------------------------------------------ 4. a bad origin
@pytest.mark.parametrize("name,band", [("two-tiles", "full"), ("coarse", "band")])
def test_an_origin_out_of_range_on_the_device_is_skipped(name, band):
    H, W, n, origins = us.shape(name)
    pred, truth = us.standard_batch(name)
    rows, pixels, state = us.reference(name, band)
    for slot, value in ((1, 1 << n), (0, -1), (1, 1 << 30)):
        ss = _make(name, band)
        stores, guards_ok = _guarded(ss)
        ss._origins[slot] = value                     # only the device can see it
        ss(_dev(pred), _dev(truth), n_valid=NV)
        got_rows, got_pixels = (t.cpu().numpy() for t in ss.frame_rows())
        want = rows.copy()
        want[:, :, slot] = 0                          # that origin's rows stay zero, the others and the pixels are served
        assert np.array_equal(got_rows, want) and np.array_equal(got_pixels, pixels), (slot, value)
        assert guards_ok()
        total = np.asarray(ss.state()["total"], dtype=object)
        assert not total[:, slot].any() and (total[:, 1 - slot] == np.asarray(state["total"], dtype=object)[:, 1 - slot]).all()


# ------------------------------------------------------------------------------------------------------------------ 5. the carry
def test_the_carry_into_the_high_word():
    ss = dnn.ScaleSkill(2, 8, 8, levels=1, origins=(0,), device=DEV)
    words = torch.zeros_like(ss._total)                                          # [2, 1, 2, 3, 2] = (lo, hi)
    words[..., 0] = -1                                                           # every lo = 2^64 - 1, every hi = 0
    ss._total.copy_(words)
    truth = np.zeros((2, 8, 8), np.uint8)
    truth[0, 1:4, 2:5], truth[0, 5:7, 0:3], truth[1, 0:2, 6:8], truth[1, 4:8, 3:4] = 1, 2, 1, 2
    pred = np.zeros((2, 8, 8), np.uint8)                                         # class 1 moved by a pixel, class 2 never predicted
    pred[0, 2:5, 3:6], pred[1, 0:2, 5:7] = 1, 1
    ss(_dev(pred), _dev(truth))
    own = ss.frame_rows()[0].cpu().numpy().astype(object).sum(axis=0)            # [2, 1, 2, 3] Python ints: the call's own rows
    assert (own > 0).any() and (own == 0).any()                                  # class 2 has no sum F^2
    want = (own + ((1 << 64) - 1)).tolist()
    assert ss.state()["total"] == want
    raw = ss._total.cpu().numpy()
    assert np.array_equal(raw[..., 1], (own != 0).astype(np.int64))              # the high words themselves: one carry per non-zero row


# ------------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors_raise_and_launch_nothing():
    H, W, n, origins = us.shape("two-tiles")
    ss = _make("two-tiles", "full")
    pred = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    truth = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    bad_calls = [
        lambda: ss(pred[:, :, :-1].contiguous(), truth),                          # wrong shapes
        lambda: ss(pred, truth[:2]),
        lambda: ss(pred[:, :-1], truth[:, :-1]),
        lambda: ss(pred.permute(0, 2, 1), truth),
        lambda: ss(pred.to(torch.int16), truth),                                  # dtypes
        lambda: ss(pred, truth.float()),
        lambda: ss(pred.bool(), truth),
        lambda: ss(pred.cpu(), truth),                                            # device
        lambda: ss(pred, truth.cpu()),
        lambda: ss(pred, None),
        lambda: ss(pred, truth, n_valid=B + 1),
        lambda: ss(pred, truth, n_valid=-1),
        lambda: ss(torch.zeros((B, W, H), dtype=torch.uint8, device=DEV).permute(0, 2, 1), truth),   # not contiguous
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"levels": 0}, {"levels": 9}, {"levels": 4}, {"row_range": (2, 2)}, {"row_range": (0, H + 1)}, {"row_range": (1, 8)},
                   {"origins": (8,)}, {"origins": ()}, {"origins": (-1,)}):
            with pytest.raises(L.DeepcamHipError):
                dnn.ScaleSkill(B, H, W, **{"levels": 3, "device": DEV, **kw})
        with pytest.raises(L.DeepcamHipError):
            dnn.ScaleSkill(0, H, W, levels=3, device=DEV)
        # the C entry point itself, with real buffers: refused before anything is launched
        args = lambda **kw: [kw.get(k, v) for k, v in (  # noqa: E731
            ("B", B), ("n_valid", B), ("H", H), ("W", W), ("pred", L.dptr(pred)), ("pred_bytes", 1), ("truth", L.dptr(truth)), ("truth_bytes", 8),
            ("L", n), ("O", len(origins)), ("origins", L.dptr(ss._origins)), ("row0", 0), ("row1", H), ("rows", L.dptr(ss._rows)),
            ("pixels", L.dptr(ss._pixels)), ("total", L.dptr(ss._total)), ("total_pixels", L.dptr(ss._total_pixels)),
            ("frames", L.dptr(ss._frames)), ("workspace", L.dptr(ss._ws)), ("stream", L.stream_ptr()))]
        for kw in ({"L": 4}, {"L": 0}, {"O": 0}, {"O": 9}, {"row1": H + 1}, {"row0": 3, "row1": 3}, {"row0": 1}, {"n_valid": B + 1},
                   {"pred_bytes": 2}, {"workspace": None}, {"origins": None}, {"truth": truth.data_ptr() + 4}):
            with pytest.raises(L.DeepcamHipError):
                L.call("dc_scale_score", *args(**kw))
    assert names == []
    assert _zero_state(ss.state())


# ------------------------------------------------------------------------------------------------------------------ 7. driver
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


def test_predict_cli_with_scale_skill(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(37)
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
    band, origins = (8, 56), (0, 5)
    n = dnn.scale_levels(band[1] - band[0], W)        # the flag is not given: 16 divides 48 rows and 96 columns
    assert n == 4
    out = str(tmp_path / "out")
    args = predict.build_parser().parse_args([*base, "--output_dir", out, "--batch_size", "2", "--scale_skill", "--scale_rows", str(band[0]),
                                              str(band[1]), "--scale_origins", *[str(c) for c in origins]])
    assert args.verify is True
    with served("predict --scale_skill") as launched:                            # batches of two and one: a padded last batch
        predict.main(args)
    assert {"scale_sums", "scale_total"} <= set(launched) and "scale_coarse" not in launched
    got = [_h5_read(os.path.join(out, f), ["prediction", "scale", "scale_pixels", "event_scores"]) for f in names]
    pred = [g["prediction"] for g in got]
    all_rows, all_pixels = [], []
    for g, p, t in zip(got, pred, truth):
        rows, pixels = us.rows_by_blocks(p, t, n, origins, band)
        for key, want, dims in (("scale", rows, (2, 2, n + 1, 3)), ("scale_pixels", pixels, (2, 2))):
            assert g[key].dtype == np.int64 and g[key].shape == dims and np.array_equal(g[key], want), key
        assert g["event_scores"] is not None                                     # the flag implies --verify
        all_rows.append(rows), all_pixels.append(pixels)
    state = us.totals_of_rows([(np.stack(all_rows), np.stack(all_pixels))], n, len(origins))
    summary = json.load(open(os.path.join(out, "summary.json")))
    entry = summary["scale_skill"]
    assert entry == predict.scale_summary(n, origins, band, W, state) and entry["frames"] == 3
    assert entry["levels"] == n and entry["origins"] == list(origins) and entry["rows"] == list(band) and "event_verification" in summary
    for k in (1, 2):
        assert entry[f"class_{k}"] == us.decode(state["total"], state["pixels"], 3, n, band[1] - band[0], W, origins)[f"class_{k}"]
    assert state["pixels"][0][1] > 0 and state["pixels"][1][1] > 0
    # without the flag: the namespace and the outputs of before -- no datasets, no entry, no launch, the same predictions byte for byte
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "2", "--scale_levels", "3"])
    assert not hasattr(args, "scale_skill") and args.verify is False
    with served("predict without --scale_skill") as launched:
        predict.main(args)
    assert launched and not [f for f in launched if f.startswith("scale_")]
    assert "scale_skill" not in json.load(open(os.path.join(plain, "summary.json")))
    for f, p in zip(names, pred):
        g = _h5_read(os.path.join(plain, f), ["prediction", "scale", "scale_pixels"])
        assert g["scale"] is None and g["scale_pixels"] is None
        assert g["prediction"].dtype == p.dtype and g["prediction"].tobytes() == p.tobytes()
