"""Event skeletons on the GPU (csrc/skeleton.hip; nn.EventAxis; predict.py --event_axis) against the checkers of util_event_axis.py:
integer equality, no tolerance.  Every raw call runs on poisoned buffers inside guard bands.  8 x 64 is one word per row (its own
neighbour across the seam), 9 x 65 has one valid bit in the last word, 40 x 72 and 64 x 200 ragged last words and several tiles."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_event_axis as ua  # noqa: E402
import util_events as ue  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
CAP, GUARD = 512, 64
POISON = {torch.uint8: 0xA5, torch.int32: -0x01234567, torch.int64: -0x0123456789ABCDEF}
SHAPES = [(8, 64), (9, 65), (33, 128), (40, 72), (64, 200)]
MASKS = ["blobs", "band", "full", "checker", "small", "ring", "rect"]
VARIANTS = {"uint8-conn8": (torch.uint8, 8), "int64-conn4": (torch.int64, 4)}


@functools.lru_cache(maxsize=None)
def _reference(name, shape, conn, wrap, cap=CAP, n_valid=2, max_iters=None, nb=2):
    H, W = shape
    return ua.reference(ua.make_mask(name, H, W, nb), n_valid, conn, wrap, cap, max_iters or max(H, W), dnn.event_weight_tables(H, W),
                        dnn.axis_link_table(H, W))


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), POISON[dtype], dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _run(mask, conn, wrap, cap=CAP, n_valid=None, max_iters=None, dtype=torch.uint8):
    """the raw entry points; asserts the guard bands and the padding samples' poison"""
    nb, H, W = mask.shape
    nv = nb if n_valid is None else n_valid
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    wy, cx, sx = (d(t) for t in dnn.event_weight_tables(H, W))
    link, m8 = d(dnn.axis_link_table(H, W)), d(mask)
    m = m8.to(dtype)
    labels = torch.zeros((nb, H, W), dtype=torch.int32, device=DEV)
    table = torch.zeros((nb, cap, ue.FIELDS), dtype=torch.int64, device=DEV)
    ncomp = torch.zeros((nb, 3), dtype=torch.int32, device=DEV)
    ws = torch.empty(L.load().dc_mask_components_workspace(nb, H, W), dtype=torch.uint8, device=DEV)
    bufs = {"skeleton": _guarded(nb * H * W, torch.uint8), "iters": _guarded(nb * 4, torch.int32),
            "rows": _guarded(nb * cap * ua.FIELDS, torch.int64)}
    st = L.stream_ptr()
    L.call("dc_mask_components", nb, nv, H, W, L.dptr(m8), conn, int(wrap), L.dptr(labels), L.dptr(ws), st)
    L.call("dc_component_stats", nb, nv, H, W, L.dptr(m8), L.dptr(labels), L.dptr(wy), L.dptr(cx), L.dptr(sx), cap, L.dptr(table),
           L.dptr(ncomp), L.dptr(ws), st)
    L.call("dc_mask_thin", nb, nv, H, W, L.dptr(m), m.element_size(), int(wrap), max_iters or max(H, W), L.dptr(bufs["skeleton"][1]),
           L.dptr(bufs["iters"][1]), st)
    L.call("dc_skeleton_stats", nb, nv, H, W, L.dptr(bufs["skeleton"][1]), L.dptr(labels), L.dptr(ws), cap, int(wrap), L.dptr(link),
           L.dptr(bufs["rows"][1]), st)
    torch.cuda.synchronize()
    got = {}
    for key, (whole, part) in bufs.items():
        p = POISON[whole.dtype]
        assert bool((whole[:GUARD] == p).all()) and bool((whole[-GUARD:] == p).all()), f"{key}: a store outside the buffer"
        got[key] = part.view(nb, -1).cpu().numpy()
        assert (got[key][nv:] == (p & 0xFF if whole.dtype == torch.uint8 else p)).all(), f"{key}: a padding sample was written"
    return {"skeleton": got["skeleton"].reshape(nb, H, W), "iters": got["iters"].reshape(nb, 2, 2), "rows": got["rows"].reshape(nb, cap, -1)}


def _assert_equal(got, ref, nv):
    bad = int((got["skeleton"][:nv] != ref["skeleton"]).sum())
    assert bad == 0, f"{bad} skeleton pixels differ, first at {np.argwhere(got['skeleton'][:nv] != ref['skeleton'])[0].tolist()}"
    assert got["iters"][:nv].tolist() == ref["iters"].tolist()
    where = np.argwhere((got["rows"][:nv] != ref["rows"]).any(axis=2))
    assert len(where) == 0, f"rows differ first at (sample, rank) {where[0].tolist()}: " \
        f"{got['rows'][tuple(where[0])].tolist()} vs {ref['rows'][tuple(where[0])].tolist()}"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_skeleton_and_rows_match_the_checker(shape, name, wrap, variant):
    dtype, conn = VARIANTS[variant]
    _assert_equal(_run(ua.make_mask(name, *shape), conn, wrap, dtype=dtype), _reference(name, shape, conn, wrap), 2)


@pytest.mark.parametrize("shift", [1, 63, 64, -1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rolled_mask_gives_rolled_skeleton(shape, shift):
    """under wrap no column is special: this catches the two seam words"""
    mask = np.concatenate([ua.make_mask("band", *shape), ua.make_mask("blobs", *shape)])
    s = shift % shape[1]
    plain, rolled = _run(mask, 8, 1), _run(np.roll(mask, s, axis=2), 8, 1)
    assert np.array_equal(np.roll(plain["skeleton"], s, axis=2), rolled["skeleton"]) and np.array_equal(plain["iters"], rolled["iters"])
    assert plain["skeleton"].any()


def test_one_pass_on_a_thick_blob_stops_unconverged():
    got, ref = _run(ua.make_mask("band", 33, 128), 8, 1, max_iters=1), _reference("band", (33, 128), 8, 1, max_iters=1)
    assert ref["iters"].tolist() == [[[1, 0], [1, 1]], [[1, 1], [1, 0]]]      # the band's class after one pass; the empty class converged
    _assert_equal(got, ref, 2)


@pytest.mark.parametrize("conn", [4, 8])
def test_padding_samples_and_a_small_cap(conn):
    """n_valid < B: _run asserts that the third sample keeps its poison; cap 4: the ranks below it are right, nothing lies behind the table"""
    mask = ua.make_mask("blobs", 40, 72, nb=3)
    ref = _reference("blobs", (40, 72), conn, 1, cap=4, n_valid=2, nb=3)
    assert ref["rows"][:, 3].any()
    _assert_equal(_run(mask, conn, 1, cap=4, n_valid=2), ref, 2)


def test_full_size_frame():
    _assert_equal(_run(ua.make_mask("field", 768, 1152, nb=1), 8, 1, cap=256), _reference("field", (768, 1152), 8, 1, cap=256, n_valid=1, nb=1), 1)


def test_predict_cli_with_event_axis(tmp_path):
    from mlperf_deepcam_amd import h5lite
    import util_val
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "unlabelled")
    os.makedirs(root)
    rs = np.random.RandomState(12)
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(2)]
    names, stats = [f"data-{i:02d}.h5" for i in range(2)], str(tmp_path / "stats.h5")
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt, out = str(tmp_path / "model_step_7.cpt"), str(tmp_path / "out")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
           out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", "--event_axis"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.load(open(os.path.join(out, "summary.json")))
    km = [[], []]
    for name in names:
        with h5lite.File(os.path.join(out, name)) as f:
            p, skel, ev, ax, axv = (f.read(k) for k in ("prediction", "prediction_axis", "events", "event_axis", "event_axis_values"))
        ref = ua.reference(p[None], 1, 8, True, 4096, max(H, W), dnn.event_weight_tables(H, W), dnn.axis_link_table(H, W))
        assert skel.dtype == np.uint8 and np.array_equal(skel, ref["skeleton"][0]) and ref["iters"][0, :, 1].tolist() == [1, 1]
        assert ax.dtype == np.int64 and np.array_equal(ax, ref["rows"][0, :len(ev)]) and not ref["rows"][0, len(ev):].any()
        assert axv.dtype == np.float64 and np.array_equal(axv, dnn.EventAxis.values(ax))
        for k in (0, 1):
            km[k] += (ax[ev[:, 1] == k + 1, 6] / 1000.0).tolist()
    sa = summary["event_axis"]
    assert sa["events"] == [len(v) for v in km] == summary["events"] and sa["frames_at_max_iters"] == 0 and sa["max_iters"] == max(H, W)
    assert sa["max_axis_km"] == [max(v, default=0.0) for v in km]
    assert all(m is None if not v else abs(m - sum(v) / len(v)) <= 1e-9 * m for m, v in zip(sa["mean_axis_km"], km))
