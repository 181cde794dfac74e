"""The event catalogue on the GPU (csrc/components.hip, nn.EventCatalog, Predictor(events=True), predict.py --events) against the flood
fill of tests/util_events.py.  Everything is integer: every comparison is exact.

Shapes come from the kernel's own tile (dc_mask_components_tile): (2 TH + 3, 2 TW + 5) has interior tile borders in both directions,
partial tiles on both edges and a seam between two different tiles; (TH - 1, TW - 3) is one partial tile whose seam lies inside it.
Batch 3 with n_valid = 2: the third sample is padding, pre-filled with sentinels that must come back untouched."""
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
import util_events as ue  # noqa: E402
import util_val  # noqa: E402
from util_launch import assert_served, served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
B, NV, CAP = 3, 2, 4096
LABEL_SENTINEL, COUNT_SENTINEL = -7, -5


def _tile():
    th, tw = C.c_int(), C.c_int()
    assert L.load().dc_mask_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


TH, TW = _tile()
SHAPES = {"tiles": (2 * TH + 3, 2 * TW + 5), "one": (TH - 1, TW - 3)}


# ------------------------------------------------------------------------------------------------------------------ masks
def _spiral(H, W):
    """a one-pixel-wide path from (0, 0) inwards, one empty pixel between its turns"""
    m = np.zeros((H, W), np.uint8)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = 1
    stuck = 0
    while stuck < 2:
        nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if 0 <= nr < H and 0 <= nc < W and not m[nr, nc] and not (0 <= fr < H and 0 <= fc < W and m[fr, fc]):
            r, c, stuck = nr, nc, 0
            m[r, c] = 1
        else:
            dr, dc, stuck = dc, -dr, stuck + 1
    return m


def _mask(name, H, W):
    """uint8 [3, H, W]; sample 2 is padding (all class 1: if it were read, counts and tables would show it)"""
    rs = np.random.RandomState(zlib.crc32(f"{name} {H} {W}".encode()))
    m = np.zeros((B, H, W), np.uint8)
    if name.startswith("random"):
        p = float(name[6:])
        m[:NV] = (rs.rand(NV, H, W) < p) * rs.randint(1, 3, (NV, H, W))
    elif name == "spiral":
        m[0] = _spiral(H, W)
        m[1] = 2 * _spiral(W, H).T
    elif name == "comb":
        m[0, 0, :] = 1
        m[0, :, ::2] = 1
        m[1, :, 0] = 2
        m[1, ::2, :] = 2
    elif name == "checker":
        rr, cc = np.mgrid[0:H, 0:W]
        m[0] = 1 + (rr + cc) % 2
        m[1] = 2 - (rr + cc) % 2
    elif name == "band":
        m[0, 5, :10] = 1                     # both ends on one row: joined under wrap
        m[0, 5, W - 10:] = 1
        m[1, 5, :10] = 1                     # ends on neighbouring rows: joined only under wrap with 8-connectivity
        m[1, 6, W - 10:] = 1
    elif name == "uniform":
        m[1] = 2                             # sample 0: all background
    elif name == "values":
        m[:NV] = rs.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), (NV, H, W))
    elif name == "rows":
        m[0, 0, :] = 1                       # rows do not wrap: the first and the last row stay apart
        m[0, H - 1, :] = 1
        m[1, 0, :] = 2
        m[1, H - 1, :] = 1
    else:
        raise KeyError(name)
    m[NV:] = 1
    return m


MASKS = ["random0.1", "random0.45", "random0.8", "spiral", "comb", "checker", "band", "uniform", "values", "rows"]


@functools.lru_cache(maxsize=None)
def _tables(H, W):
    return dnn.event_weight_tables(H, W)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, conn, wrap, cap=CAP):
    """the checker's answer, computed once per case and shared (callers do not modify it)"""
    H, W = SHAPES[shape]
    return ue.catalogue(_mask(name, H, W), NV, conn, wrap, *_tables(H, W), cap)


def _run(mask, conn, wrap, cap=CAP, n_valid=NV):
    """both calls on buffers pre-filled with sentinels (labels, counts) and with ones (the table, which the call zeroes)"""
    nb, H, W = mask.shape
    wy, cx, sx = (torch.from_numpy(t).to(DEV) for t in _tables(H, W))
    m = torch.from_numpy(mask).to(DEV)
    labels = torch.full((nb, H, W), LABEL_SENTINEL, dtype=torch.int32, device=DEV)
    table = torch.ones((nb, cap, ue.FIELDS), dtype=torch.int64, device=DEV)
    ncomp = torch.full((nb, 3), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.load().dc_mask_components_workspace(nb, H, W), dtype=torch.uint8, device=DEV)
    st = L.stream_ptr()
    L.call("dc_mask_components", nb, n_valid, H, W, L.dptr(m), conn, int(wrap), L.dptr(labels), L.dptr(ws), st)
    L.call("dc_component_stats", nb, n_valid, H, W, L.dptr(m), L.dptr(labels), L.dptr(wy), L.dptr(cx), L.dptr(sx), cap, L.dptr(table),
           L.dptr(ncomp), L.dptr(ws), st)
    torch.cuda.synchronize()
    return labels.cpu(), table.cpu(), ncomp.cpu()


def _assert_equal(got, ref, nv=NV):
    labels, table, ncomp = got
    rl, rt, rn = (torch.from_numpy(a) for a in ref[:3])
    assert torch.equal(ncomp[:nv], rn), f"counts {ncomp[:nv].tolist()} vs {rn.tolist()}"
    assert torch.equal(labels[:nv], rl), f"{int((labels[:nv] != rl).sum())} labels differ"
    assert torch.equal(table[:nv], rt), f"rows differ first at {torch.nonzero((table[:nv] != rt).any(dim=2))[:3].tolist()}"
    # the padding: not read, labels and counts untouched, its part of the table zeroed
    assert bool((labels[nv:] == LABEL_SENTINEL).all()) and bool((ncomp[nv:] == COUNT_SENTINEL).all()) and int(table[nv:].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ 1. kernels vs checker
@pytest.mark.parametrize("wrap", [False, True], ids=["nowrap", "wrap"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", MASKS)
def test_components_vs_flood_fill(name, shape, conn, wrap):
    H, W = SHAPES[shape]
    ref = _reference(name, shape, conn, wrap)
    _assert_equal(_run(_mask(name, H, W), conn, wrap), ref)
    n, rows = ref[2], ref[3]
    if name in ("spiral", "comb"):
        assert n[:, 0].tolist() == [1, 1]                                 # one long component each, through every tile
    elif name == "uniform":
        assert n.tolist() == [[0, 0, 0], [1, 0, 1]] and rows[1][0].tolist()[:3] == [0, 2, H * W]
    elif name == "rows":
        assert n.tolist() == [[2, 2, 0], [2, 1, 1]] and [int(r[9]) for r in rows[0]] == [1, 1]
    elif name == "band":
        joined0, joined1 = wrap, wrap and conn == 8
        assert n[:, 0].tolist() == [1 if joined0 else 2, 1 if joined1 else 2]
        assert [int(r[9]) for r in rows[0]] == ([1] if joined0 else [0, 0]) and [int(r[9]) for r in rows[1]] == ([1] if joined1 else [0, 0])
    elif name == "checker" and not wrap:
        assert n[0].tolist() == ([H * W, (H * W + 1) // 2, H * W // 2] if conn == 4 else [2, 1, 1])


@pytest.mark.parametrize("conn", [4, 8])
def test_more_components_than_the_table_holds(conn):
    """The checkerboard under 4-connectivity is the largest count possible, one component per pixel: the counts stay exact, the table holds
    exactly the first cap roots and nothing behind them."""
    H, W = SHAPES["tiles"]
    cap = 100
    mask = _mask("checker", H, W)
    ref = _reference("checker", "tiles", conn, False, cap)
    got = _run(mask, conn, False, cap=cap)
    _assert_equal(got, ref)
    if conn == 4:
        assert got[2][0].tolist() == [H * W, (H * W + 1) // 2, H * W // 2]
        assert got[1][0, :, 0].tolist() == list(range(cap)) and bool((got[1][0, :, 2] == 1).all())
    else:
        assert got[2][0].tolist() == [2, 1, 1] and int(got[1][0, 2:].abs().sum()) == 0


def test_every_sample_valid_and_a_single_sample():
    H, W = SHAPES["tiles"]
    mask = _mask("random0.45", H, W)
    ref = ue.catalogue(mask, B, 8, True, *_tables(H, W), CAP)
    _assert_equal(_run(mask, 8, True, n_valid=B), ref, nv=B)
    assert ref[2][2].tolist() == [1, 1, 0]                                # the third sample: one class-1 component over the whole field
    _assert_equal(_run(mask[:1], 4, True, n_valid=1), tuple(a[:1] for a in _reference("random0.45", "tiles", 4, True)[:3]), nv=1)


# ------------------------------------------------------------------------------------------------------------------ 2. dispatch, stability
def test_the_four_kernel_families_serve_the_calls():
    H, W = SHAPES["tiles"]
    cat = dnn.EventCatalog(B, H, W)
    m = torch.from_numpy(_mask("random0.45", H, W)).to(DEV)
    with served("EventCatalog") as names:
        cat(m, n_valid=NV)
    torch.cuda.synchronize()
    assert_served(names[:3], ["cc_tile", "cc_merge", "cc_flatten"])
    assert len(names) > 3 and set(names[3:]) == {"cc_stats"}


def test_two_calls_give_identical_outputs():
    H, W = SHAPES["tiles"]
    cat = dnn.EventCatalog(B, H, W, connectivity=8, wrap=True)
    m = torch.from_numpy(_mask("random0.45", H, W)).to(DEV)
    other = torch.from_numpy(_mask("checker", H, W)).to(DEV)
    cat(m, n_valid=NV)
    first = (cat.labels.clone(), cat.table.clone(), cat.counts().clone())
    cat(other, n_valid=NV)                                                # more components: rows the next call has to clear
    assert not torch.equal(cat.counts(), first[2])
    cat(m, n_valid=NV)
    torch.cuda.synchronize()
    assert torch.equal(cat.labels, first[0]) and torch.equal(cat.table, first[1]) and torch.equal(cat.counts(), first[2])
    ref = _reference("random0.45", "tiles", 8, True)
    _assert_equal((torch.cat([cat.labels.cpu(), torch.full((1, H, W), LABEL_SENTINEL, dtype=torch.int32)]),
                   torch.cat([cat.table.cpu(), torch.zeros((1, CAP, ue.FIELDS), dtype=torch.int64)]),
                   torch.cat([cat.counts().cpu(), torch.full((1, 3), COUNT_SENTINEL, dtype=torch.int32)])), ref)
    # the host view: counts first, then only the filled rows; events() decodes them
    ncomp, rows = cat.rows()
    assert ncomp.tolist() == ref[2].tolist() and all(np.array_equal(r, e) for r, e in zip(rows, ref[3]))
    ev = cat.events()
    assert [len(e) for e in ev] == ref[2][:, 0].tolist() and ev[0] == dnn.EventCatalog.decode(ref[3][0], H, W)
    big = cat.events(min_pixels=20)
    assert [[e["root"] for e in s] for s in big] == [[int(r[0]) for r in rows_ if r[2] >= 20] for rows_ in ref[3]]
    with pytest.raises(L.DeepcamHipError):
        cat(m.to(torch.int32))
    with pytest.raises(L.DeepcamHipError):
        cat(m, n_valid=B + 1)


# ------------------------------------------------------------------------------------------------------------------ 3. Predictor
@pytest.fixture(scope="module")
def state():
    return util_val.perturbed_state()


def _net(state):
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.float32, seed=333)
    net.materialize(2, util_val.H, util_val.W)
    net.load_state_dict(state)
    net.eval()
    return net


def test_predictor_with_events(state):
    H, W = util_val.H, util_val.W
    net = _net(state)
    x, _ = util_val.val_inputs(n=2, seed=util_val.INPUT_SEED + 90)
    plain = dnn.Predictor(net, 2, H, W)
    with_events = dnn.Predictor(net, 2, H, W, events=True)
    try:
        assert plain.catalog is None and with_events.catalog is not None
        want = plain(x.to(DEV)).cpu()
        got = with_events(x.to(DEV)).cpu()
        assert torch.equal(got, want) and torch.equal(with_events.class_counts.cpu(), plain.class_counts.cpu())
        cat = with_events.catalog
        assert (cat.connectivity, cat.wrap, cat.cap) == (8, True, 4096)
        labels, table, ncomp, rows = ue.catalogue(got.numpy(), 2, 8, True, *_tables(H, W), cat.cap)
        assert torch.equal(cat.labels.cpu(), torch.from_numpy(labels))
        assert torch.equal(cat.table.cpu(), torch.from_numpy(table)) and torch.equal(cat.counts().cpu(), torch.from_numpy(ncomp))
        assert cat.events() == [dnn.EventCatalog.decode(r, H, W) for r in rows]
        print(f"Predictor(events=True) at {H} x {W}: components per sample {ncomp.tolist()}")
    finally:
        plain.close()
        with_events.close()
    assert with_events.catalog is None


# ------------------------------------------------------------------------------------------------------------------ 4. driver
def test_predict_cli_with_events(tmp_path, state):
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "unlabelled")
    os.makedirs(root)
    rs = np.random.RandomState(12)
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(2)]
    names = [f"data-{i:02d}.h5" for i in range(2)]
    for name, d in zip(names, fields):
        with h5lite.File(os.path.join(root, name), "w") as f:
            f.write("climate/data", d)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": state}, ckpt)

    def run(out, *extra):
        cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir",
               out, "--batch_size", "2", "--dtype", "fp32", "--height", str(H), "--width", str(W), "--max_inter_threads", "2", *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), json.load(open(os.path.join(out, "summary.json")))

    out = str(tmp_path / "with_events")
    line, summary = run(out, "--events", "--event_connectivity", "4")
    total = [0, 0]
    for i, name in enumerate(names):
        with h5lite.File(os.path.join(out, name)) as f:
            p, ev = f.read("prediction"), f.read("events")
        assert ev.dtype == np.int64 and ev.ndim == 2 and ev.shape[1] == ue.FIELDS
        _, rows = ue.label_one(p, 4, True, *_tables(H, W))
        assert np.array_equal(ev, rows), name
        per_class = [int((rows[:, 1] == 1).sum()), int((rows[:, 1] == 2).sum())]
        assert summary["files"][i]["events"] == per_class and summary["files"][i]["events_overflowed"] is False
        total = [total[0] + per_class[0], total[1] + per_class[1]]
    assert summary["events"] == total == line["events"] and summary["events_overflowed_files"] == 0
    # without the flag: the outputs of before
    out2 = str(tmp_path / "plain")
    line2, summary2 = run(out2)
    assert "events" not in summary2 and "events" not in line2 and all("events" not in rec for rec in summary2["files"])
    for name in names:
        with h5lite.File(os.path.join(out2, name)) as f:
            assert "events" not in f and "prediction" in f
            p2 = f.read("prediction")
        with h5lite.File(os.path.join(out, name)) as f:
            assert np.array_equal(f.read("prediction"), p2)
