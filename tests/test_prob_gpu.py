"""Probabilistic verification on the GPU (dc_prob_score of csrc/probskill.hip, nn.ProbabilitySkill, predict.py --prob_skill) against the
numpy checker of tests/util_prob.py.  From q = rint(p * 65536) on everything is an integer: every comparison is equality.  The device
rounds in fp32, the checker in float64, so the data either stand clear of every rounding boundary by construction (asserted on the CPU
first) or the pixels within 1/16 q-unit of one are masked through their label, which the kernel then counts as a bad label.
The shapes come from the kernel's own chunk (dc_prob_block: P pixels per workgroup, G the cap on the workgroups per sample): "tiny" is
less than a wave and odd, so that planes 1 and 2 are not 16-byte aligned; "ragged" is odd, between 2 P and 3 P; "vector" is a multiple of
4 above 2 P whose last workgroup ends inside a pass and inside a wave.  G is 0: a workgroup takes one chunk and ends, so there is no
grid-stride loop to run twice (a kernel with a cap would need a fourth shape beyond G * P pixels; _block() refuses one until it is added)."""
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
import util_prob as up  # noqa: E402
import util_val  # noqa: E402
from util_launch import served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = 3, 2
GUARD, SENTINEL = 64, 0x5A5A5A5A
ONE = 65536
ZERO, TOTAL = "prob_zero", "prob_total"


@functools.lru_cache(maxsize=None)
def _block():
    px, groups = C.c_int(0), C.c_int(-1)
    assert L.load().dc_prob_block(C.byref(px), C.byref(groups)) == 0 and px.value >= 256
    assert groups.value == 0, "the kernel caps its grid: add a shape of more than G * P pixels to SHAPES"
    return px.value


SHAPES = ["tiny", "ragged", "vector"]


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
    else:
        H = 12
        W = (2 * P + P // 3) // H + 1
        assert (H * W) % 4 == 0 and H * W >= 2 * P and (H * W) % P % 256 != 0
    return H, W


def _kernel(shape):
    H, W = _shape(shape)
    return "prob_hist_vec" if (H * W) % 4 == 0 else "prob_hist"


def _labels_for(rs, q, n):
    """labels that follow the probabilities loosely: the class drawn from q in two thirds of the pixels, uniform in the rest"""
    u = rs.randint(0, ONE, size=n)
    drawn = (u >= q[0]).astype(np.int64) + (u >= q[0] + q[1])
    return np.where(rs.rand(n) < 0.67, drawn, rs.randint(0, 3, size=n)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _constructed(shape, seed=0):
    """(logits float32 [B, 3, H, W], labels int64 [B, H, W]) of constructed probabilities, the padding frame all sentinels: NaN logits
    and label 1.  The float64 softmax stands at least 0.25 q-units clear of every rounding boundary.  Shared and never modified."""
    H, W = _shape(shape)
    rs = np.random.RandomState(100 + H + seed)
    logits = np.full((B, 3, H, W), np.nan, np.float32)
    labels = np.ones((B, H, W), np.int64)
    for b in range(NV):
        l, q = up.constructed(rs, H * W)
        assert up.distance_to_boundary(l).min() >= 0.25 and np.array_equal(up.quantise(l), q)
        logits[b] = l.reshape(3, H, W)
        labels[b] = _labels_for(rs, q, H * W).reshape(H, W)
    logits.setflags(write=False), labels.setflags(write=False)
    return logits, labels


@functools.lru_cache(maxsize=None)
def _reference(shape, K):
    """(hist, rows [NV, 3], pixels [NV, 3], state) of the constructed batch.  Shared and never modified."""
    logits, labels = _constructed(shape)
    hist, rows, pixels = up.batch(logits[:NV], labels[:NV], K)
    for a in (hist, rows, pixels):
        a.setflags(write=False)
    return hist, rows, pixels, up.totals([(logits[:NV], labels[:NV])], K)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)         # a copy: the shared batches are read-only


def _make(shape, K, batch=B):
    H, W = _shape(shape)
    return dnn.ProbabilitySkill(batch, H, W, bins=K, device=DEV)


def _assert_call(ps, hist, rows, pixels, what=""):
    got_rows, got_pixels = (t.cpu().numpy() for t in ps.frame_rows())
    got_hist = ps.batch_hist().cpu().numpy()
    assert got_rows.dtype == np.int64 and got_rows.shape == rows.shape and got_pixels.shape == pixels.shape and got_hist.shape == hist.shape, what
    assert np.array_equal(got_pixels, pixels), (what, got_pixels.tolist(), pixels.tolist())
    assert np.array_equal(got_hist, hist), (what, np.argwhere(got_hist != hist)[:6].tolist())
    assert np.array_equal(got_rows, rows), (what, got_rows.tolist(), rows.tolist())


# ------------------------------------------------------------------------------------------------------------------ 1. constructed probabilities
@pytest.mark.parametrize("K", [1, 10, 20, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_constructed_probabilities_equal_the_checker(shape, K):
    logits, labels = _constructed(shape)
    ps = _make(shape, K)
    with served("ProbabilitySkill") as names:
        assert ps(_dev(logits), _dev(labels), n_valid=NV) is ps
    assert names == [ZERO, _kernel(shape), TOTAL]
    hist, rows, pixels, state = _reference(shape, K)
    assert pixels[:, 0].tolist() == [labels[0].size] * NV and not pixels[:, 1:].any()       # no pixel is masked
    _assert_call(ps, hist, rows, pixels, f"{shape} K={K}")
    assert not ps._rows[NV:].any() and not ps._pixels[NV:].any()                 # the padding frame: untouched zeros
    got = ps.state()
    assert up.same_state(got, state) and got["frames"] == NV and all(isinstance(v, int) for v in got["sq"])
    assert ps.result() == up.decode(state["hist"], state["sq"], state["pixels"], K)
    brier = dnn.brier_from_rows(*(t.cpu().numpy() for t in ps.frame_rows()))
    assert all(0.0 < v < 1.0 for frame in brier for v in frame)


# ------------------------------------------------------------------------------------------------------------------ 2. random logits
def _masked_random(rs, n, H, W):
    """3 * randn logits and labels with the ambiguous pixels (within 1/16 q-unit of a rounding boundary) set to 255"""
    logits = (3 * rs.randn(n, 3, H, W)).astype(np.float32)
    labels = rs.randint(0, 3, size=(n, H, W)).astype(np.int64)
    masked = np.stack([up.ambiguous(l, up.EPS) for l in logits])
    assert masked.mean() <= 0.40, masked.mean()      # the reference alone masks about a third of such data
    labels[masked] = 255
    return logits, labels, masked


@pytest.mark.parametrize("shape", ["ragged", "vector"])
def test_random_logits_with_ambiguous_pixels_masked(shape):
    H, W = _shape(shape)
    K = 20
    logits, labels, masked = _masked_random(np.random.RandomState(21 + H), B, H, W)
    logits[NV:], labels[NV:] = np.nan, 1
    ps = _make(shape, K)
    ps(_dev(logits), _dev(labels).to(torch.uint8), n_valid=NV)
    hist, rows, pixels = up.batch(logits[:NV], labels[:NV], K)
    assert pixels[:, 1].tolist() == masked[:NV].sum(axis=(1, 2)).tolist() and (pixels[:, 0] > 0.6 * H * W).all()
    _assert_call(ps, hist, rows, pixels, shape)
    assert up.same_state(ps.state(), up.totals([(logits[:NV], labels[:NV])], K))


# ------------------------------------------------------------------------------------------------------------------ 3. contention patterns
def _pattern(name, shape):
    """(logits [B, 3, H, W], labels [B, H, W]): frames 0 and 1 follow the pattern in pixel order and in order of the 4-pixel groups that
    a lane of the vector form owns; the padding frame is sentinels"""
    H, W = _shape(shape)
    n = H * W
    i = np.arange(n)
    q = np.empty((NV, 3, n), np.int64)
    labels = np.zeros((NV, n), np.int64)
    for b, lane in enumerate((i % 64, (i // 4) % 64)):
        if name == "identical":                      # all background: every lane of every wave on the same three cells
            q[b, 1], q[b, 2] = 60, 40
        elif name == "all-differ":                   # every lane of a wave in another bin, for every class (at K = 256; most at K = 20)
            q[b, 1], q[b, 2] = 500 + 700 * lane, 300 + 290 * ((lane * 7) % 64)
        elif name == "one-differs":                  # one lane against 63: another probability and another outcome
            odd = lane == 37
            q[b, 1], q[b, 2] = np.where(odd, 40000, 60), np.where(odd, 5000, 40)
            labels[b] = np.where(odd, 1, 0)
        else:                                        # "one-label": equal probabilities, one lane with another outcome
            q[b, 1], q[b, 2] = 60, 40
            labels[b] = np.where(lane == 11, 2, 0)
        q[b, 0] = ONE - q[b, 1] - q[b, 2]
    assert (q >= 1).all()
    logits = np.full((B, 3, H, W), np.nan, np.float32)
    logits[:NV] = up.logits_of(q).reshape(NV, 3, H, W)
    for b in range(NV):
        assert up.distance_to_boundary(logits[b]).min() >= 0.25 and np.array_equal(up.quantise(logits[b]).reshape(3, n), q[b])
    full = np.ones((B, H, W), np.int64)
    full[:NV] = labels.reshape(NV, H, W)
    return logits, full


@pytest.mark.parametrize("K", [20, 256])
@pytest.mark.parametrize("shape", SHAPES)                             # each ends in a partially filled wave
@pytest.mark.parametrize("name", ["identical", "all-differ", "one-differs", "one-label"])
def test_contention_patterns(name, shape, K):
    logits, labels = _pattern(name, shape)
    ps = _make(shape, K)
    ps(_dev(logits), _dev(labels), n_valid=NV)
    hist, rows, pixels = up.batch(logits[:NV], labels[:NV], K)
    if name == "identical":
        assert np.count_nonzero(hist[..., 0]) == 3 and hist[0, 1, K - 1, 0] == NV * labels[0].size
    if name == "all-differ" and K == 256 and shape != "tiny":
        assert np.count_nonzero(hist[1, 0, :, 0]) == 64 and np.count_nonzero(hist[2, 0, :, 0]) == 64
    _assert_call(ps, hist, rows, pixels, f"{name} {shape} K={K}")
    assert up.same_state(ps.state(), up.totals([(logits[:NV], labels[:NV])], K))


# ------------------------------------------------------------------------------------------------------------------ 4. label element sizes
@pytest.mark.parametrize("shape", ["ragged", "vector"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64], ids=["u8", "i32", "i64"])
def test_label_element_sizes_bad_labels_and_logits_that_are_not_finite(dtype, shape):
    H, W = _shape(shape)
    K = 20
    base_logits, base_labels = _constructed(shape)
    logits, ref_labels = base_logits.copy(), base_labels.copy()
    rs = np.random.RandomState(41)
    bad = rs.rand(B, H, W) < 0.05
    bad[0, 0, :4] = True
    ref_labels[bad] = 255
    labels = ref_labels.astype(dtype)
    kinds = [3, 255] if dtype == np.uint8 else ([3, 255, -1, 256] if dtype == np.int32 else [3, 255, -1, 256, (1 << 32) + 1, -(1 << 32)])
    labels[bad] = rs.choice(np.asarray(kinds, dtype), size=int(bad.sum()))
    labels[0, 0, :len(kinds)][:4] = kinds[:4]
    for k, v in enumerate((np.nan, np.inf, -np.inf)):                            # one bad value in any one plane
        hit = rs.rand(B, H, W) < 0.02
        hit[0, 1, k] = True
        logits[:, k][hit] = v
    logits[0, :, 0, 0] = np.nan                                                  # with a bad label: counted as a bad label
    assert bad[0, 0, 0]
    logits[NV:], labels[NV:] = np.nan, 1
    ps = _make(shape, K)
    ps(_dev(logits), _dev(labels), n_valid=NV)
    hist, rows, pixels = up.batch(logits[:NV], ref_labels[:NV], K)
    assert pixels[:, 1].tolist() == bad[:NV].sum(axis=(1, 2)).tolist() and (pixels[:, 2] > 0).all() and (pixels.sum(axis=1) == H * W).all()
    _assert_call(ps, hist, rows, pixels, f"{dtype.__name__} {shape}")
    assert up.same_state(ps.state(), up.totals([(logits[:NV], ref_labels[:NV])], K))


# ------------------------------------------------------------------------------------------------------------------ 5. the cut into batches
def test_the_cut_into_batches_does_not_matter_and_reset():
    shape, K, n = "ragged", 20, 3
    H, W = _shape(shape)
    rs = np.random.RandomState(51)
    logits, labels, _ = _masked_random(rs, n, H, W)
    ref = up.totals([(logits, labels)], K)
    states = []
    for batch in (3, 2, 1):
        ps = _make(shape, K, batch=batch)
        for s in range(0, n, batch):
            nv = min(batch, n - s)
            lg, lb = np.full((batch, 3, H, W), np.nan, np.float32), np.ones((batch, H, W), np.int64)   # padding: wrong if read
            lg[:nv], lb[:nv] = logits[s:s + nv], labels[s:s + nv]
            ps(_dev(lg), _dev(lb), n_valid=nv)
        states.append(ps.state())
        assert up.same_state(states[-1], ref), f"batch {batch}"
    assert states[0]["frames"] == n
    # the batch histogram and the frame rows are the last call's; the totals are both calls'
    ps.reset()
    zero = ps.state()
    assert zero["frames"] == 0 and zero["pixels"] == [0, 0, 0] and zero["sq"] == [0, 0, 0] and not zero["hist"].any()
    ps(_dev(logits[:1]), _dev(labels[:1]))
    ps(_dev(logits[1:2]), _dev(labels[1:2]))
    assert up.same_state(ps.state(), up.totals([(logits[:2], labels[:2])], K))
    _assert_call(ps, *up.batch(logits[1:2], labels[1:2], K), "second call")
    ps(_dev(logits[:1]), _dev(labels[:1]), n_valid=0)                            # nothing valid: an empty histogram, unchanged totals
    assert up.same_state(ps.state(), up.totals([(logits[:2], labels[:2])], K))
    assert not ps.batch_hist().any() and ps.frame_rows()[0].shape[0] == 0


# ------------------------------------------------------------------------------------------------------------------ 6. the carry, the guards
def test_the_carry_into_the_high_word():
    shape, K = "vector", 10
    logits, labels = _constructed(shape)
    _, _, _, state = _reference(shape, K)
    ps = _make(shape, K)
    words = torch.zeros_like(ps._total_sq)
    words[0, 0] = -1                                                             # lo = 2^64 - 1
    words[2, 0], words[2, 1] = -(1 << 63), 5                                     # lo = 2^63, hi = 5
    ps._total_sq.copy_(words)
    ps(_dev(logits), _dev(labels), n_valid=NV)
    want = list(state["sq"])
    assert all(v > 0 for v in want)
    want[0] += (1 << 64) - 1
    want[2] += (5 << 64) + (1 << 63)
    assert ps.state()["sq"] == want
    raw = ps._total_sq.cpu().numpy()
    assert raw[0, 1] == 1 and raw[0, 0] == state["sq"][0] - 1                    # (hi, lo) themselves
    assert raw[2, 1] == 5 and raw[2, 0] == state["sq"][2] - (1 << 63) and raw[1].tolist() == [state["sq"][1], 0]


@pytest.mark.parametrize("shape", SHAPES)
def test_guard_words_and_the_padding_sample_survive(shape):
    K = 256
    logits, labels = _constructed(shape)
    ps = _make(shape, K)
    stores = {}
    for name in ("_hist", "_rows", "_pixels", "_total_hist", "_total_sq", "_total_pixels", "_frames"):
        t = getattr(ps, name)
        store = torch.zeros(t.numel() + 2 * GUARD, dtype=t.dtype, device=DEV)
        store[:GUARD], store[GUARD + t.numel():] = SENTINEL, SENTINEL
        stores[name] = store
        setattr(ps, name, store[GUARD:GUARD + t.numel()].view(t.shape))
    ps._rows[NV:], ps._pixels[NV:] = SENTINEL, SENTINEL                          # the padding sample's outputs: not written either
    guards_ok = lambda: all(bool((s[:GUARD] == SENTINEL).all()) and bool((s[-GUARD:] == SENTINEL).all()) for s in stores.values()) \
        and bool((ps._rows[NV:] == SENTINEL).all()) and bool((ps._pixels[NV:] == SENTINEL).all())  # noqa: E731
    hist, rows, pixels, state = _reference(shape, K)
    for _ in range(2):
        ps(_dev(logits), _dev(labels), n_valid=NV)
        _assert_call(ps, hist, rows, pixels, "guarded")
        assert guards_ok()
    assert up.same_state(ps.state(), up.totals([(logits[:NV], labels[:NV])] * 2, K))
    ps.reset()
    assert guards_ok() and ps.state()["frames"] == 0


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors_raise_and_launch_nothing():
    H, W = _shape("tiny")
    ps = _make("tiny", 20)
    logits = torch.zeros((B, 3, H, W), dtype=torch.float32, device=DEV)
    labels = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    bad_calls = [
        lambda: ps(logits[:, :, :, :-1].contiguous(), labels),                    # wrong shapes
        lambda: ps(logits[:2], labels),
        lambda: ps(logits, labels[:2]),
        lambda: ps(logits[:, :2], labels),
        lambda: ps(logits.permute(0, 1, 3, 2), labels),
        lambda: ps(logits.half(), labels),                                        # dtypes
        lambda: ps(logits.double(), labels),
        lambda: ps(logits, labels.float()),
        lambda: ps(logits, labels.to(torch.int16)),
        lambda: ps(logits.cpu(), labels),                                         # device
        lambda: ps(logits, labels.cpu()),
        lambda: ps(logits, None),
        lambda: ps(logits, labels, n_valid=B + 1),
        lambda: ps(logits, labels, n_valid=-1),
        lambda: ps(torch.zeros((B, H, W, 3), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2), labels),   # not contiguous
    ]
    with served("errors") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        for kw in ({"bins": 0}, {"bins": 257}, {"bins": -2}):
            with pytest.raises(L.DeepcamHipError):
                dnn.ProbabilitySkill(B, H, W, device=DEV, **kw)
        with pytest.raises(L.DeepcamHipError):
            dnn.ProbabilitySkill(0, H, W, device=DEV)
        # the C ABI's own checks, behind the Python ones
        args = [B, NV, H, W, L.dptr(logits), L.dptr(labels), 8, 20, L.dptr(ps._hist), L.dptr(ps._rows), L.dptr(ps._pixels),
                L.dptr(ps._total_hist), L.dptr(ps._total_sq), L.dptr(ps._total_pixels), L.dptr(ps._frames), L.stream_ptr()]
        for pos, value in ((1, B + 1), (6, 2), (7, 0), (7, 257), (8, None), (4, logits.data_ptr() + 2), (12, ps._total_sq.data_ptr() + 4)):
            with pytest.raises(L.DeepcamHipError):
                L.call("dc_prob_score", *[value if k == pos else a for k, a in enumerate(args)])
    assert names == []
    state = ps.state()
    assert state["frames"] == 0 and state["sq"] == [0, 0, 0] and not state["hist"].any()
    with served("a good call") as names:
        ps(logits, labels)
    assert names == [ZERO, "prob_hist", TOTAL]                                    # 57 pixels: not a multiple of 4
    with served("a good call, empty") as names:
        ps(logits, labels, n_valid=0)
    assert names == [ZERO]


# ------------------------------------------------------------------------------------------------------------------ 8. Predictor
def _mask_through_labels(logits, labels):
    """labels (int64 numpy, modified in place): 255 where the checker calls the pixel ambiguous; the share must stay below 40 %"""
    masked = np.stack([up.ambiguous(l, up.EPS) for l in logits])
    assert masked.mean() <= 0.40, masked.mean()
    labels[masked] = 255
    return labels


def test_predictor_bf16_with_stored_logits():
    H, W, K = util_val.H, util_val.W, 20
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(2, H, W)
    net.load_state_dict(util_val.perturbed_state())
    net.eval()
    x, y = util_val.val_inputs(n=2)
    pr = dnn.Predictor(net, 2, H, W)
    try:
        pr.store_logits = True
        pr(x.to(DEV))
        assert tuple(pr.logits_buffer.shape) == (2, 3, H, W) and pr.logits_buffer.dtype == torch.float32
        logits = pr.logits.cpu().numpy()
        labels = _mask_through_labels(logits, y.numpy().astype(np.int64))
        ps = dnn.ProbabilitySkill(2, H, W, bins=K, device=DEV)
        with served("ProbabilitySkill behind Predictor") as names:
            ps(pr.logits_buffer, _dev(labels))
        assert names == [ZERO, "prob_hist_vec", TOTAL]
        _assert_call(ps, *up.batch(logits, labels, K), "predictor")
        ref = up.totals([(logits, labels)], K)
        assert up.same_state(ps.state(), ref) and ref["pixels"][2] == 0 and ref["pixels"][0] > 0.6 * 2 * H * W
        assert ps.result() == up.decode(ref["hist"], ref["sq"], ref["pixels"], K)
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------------------------ 9. driver
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


def test_predict_cli_with_prob_skill(tmp_path, monkeypatch):
    from mlperf_deepcam_amd import predict
    H, W, K = util_val.H, util_val.W, 10
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(31)
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
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "bf16", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2"]

    # The driver writes no logits: the test listens where they are scored.  Before every call it copies the stored logits to the host and
    # masks the ambiguous pixels through the labels, as the other tests here do before they launch.
    seen = []
    real_call = dnn.ProbabilitySkill.__call__

    def listening(self, logits, labels, n_valid=None):
        lg = logits[:n_valid].cpu().numpy()
        lb = _mask_through_labels(lg, labels[:n_valid].cpu().numpy().astype(np.int64))
        labels[:n_valid].copy_(torch.from_numpy(lb).to(labels.dtype))
        seen.append((lg, lb))
        return real_call(self, logits, labels, n_valid)

    monkeypatch.setattr(dnn.ProbabilitySkill, "__call__", listening)
    out = str(tmp_path / "out")
    args = predict.build_parser().parse_args([*base, "--output_dir", out, "--batch_size", "2", "--prob_skill", "--prob_bins", str(K)])
    assert args.verify is True
    with served("predict --prob_skill") as launched:                             # batches of two and one: a padded last batch
        predict.main(args)
    assert {ZERO, "prob_hist_vec", TOTAL} <= set(launched) and [len(lg) for lg, _ in seen] == [2, 1]
    state = up.totals(seen, K)
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["prob_skill"] == predict.prob_summary(K, state) and summary["prob_skill"]["frames"] == 3
    ref = up.decode(state["hist"], state["sq"], state["pixels"], K)
    for c in range(3):
        for key in predict.PROB_SUMMARY_KEYS:
            assert abs(summary["prob_skill"][f"class_{c}"][key] - ref[f"class_{c}"][key]) <= 1e-12, (c, key)
    assert "event_verification" in summary                                       # --prob_skill implies --verify
    frames = [(lg[j], lb[j]) for lg, lb in seen for j in range(len(lg))]
    for name, (lg, lb) in zip(names, frames):
        g = _h5_read(os.path.join(out, name), ["prediction", "brier", "prob_pixels", "event_scores"])
        _, rows, pixels = up.frame(lg, lb, K)
        assert g["prob_pixels"].dtype == np.int64 and np.array_equal(g["prob_pixels"], pixels) and g["event_scores"] is not None
        assert g["brier"].dtype == np.float64 and g["brier"].tolist() == [int(r) / (int(pixels[0]) << 32) for r in rows]
    got = _h5_read(os.path.join(out, "prob_skill.h5"), ["hist", "sq_words", "pixels", "frames", "bins", "pod", "curve_n", "scalars"])
    assert np.array_equal(got["hist"], state["hist"]) and got["sq_words"].tolist() == [[v, 0] for v in state["sq"]]
    assert got["pixels"].tolist() == state["pixels"] and got["frames"].tolist() == [3] and got["bins"].tolist() == [K]
    assert got["pod"].shape == (3, K + 1) and got["curve_n"].sum() == 3 * state["pixels"][0] and got["scalars"].shape[0] == 3
    # without the flag: no datasets, no entry, no launch of the family
    monkeypatch.setattr(dnn.ProbabilitySkill, "__call__", real_call)
    plain = str(tmp_path / "plain")
    args = predict.build_parser().parse_args([*base, "--output_dir", plain, "--batch_size", "2", "--prob_bins", "5"])
    with served("predict without --prob_skill") as launched:
        predict.main(args)
    assert launched and not [n for n in launched if n.startswith("prob")]
    assert "prob_skill" not in json.load(open(os.path.join(plain, "summary.json"))) and not os.path.exists(os.path.join(plain, "prob_skill.h5"))
    for n in names:
        g = _h5_read(os.path.join(plain, n), ["brier", "prob_pixels"])
        assert g["brier"] is None and g["prob_pixels"] is None
