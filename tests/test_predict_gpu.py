"""Inference on unlabelled data on the GPU: dc_logits_predict against torch, the fused classifier's prediction variant against the unfused
route bit for bit, nn.Predictor against the reference's fixture (tests/golden/val_small.json) and against itself, the forward-only
engine's contract, the unlabelled input pipeline, and the driver (python -m mlperf_deepcam_amd.predict).

Confidence (the predicted class's softmax probability, fp32 expf and one division) against an fp64 softmax of the same logits, on the
random logits of test_logits_predict_vs_torch: largest absolute error measured on an MI355X 1.302e-07 (CONF_ABS_MEASURED); the test asserts
four times that, rounded up to one significant digit, 6e-07 (CONF_ABS_TOL) -- room for expf / division rounding on other inputs, not for another
algorithm.  The test prints the figure on every run.

bf16 (test_predictor_self_consistency[bf16]): the share of pixels on which Predictor (batch 2) and the existing batch-1 path
(net.engine_for + torch.max) pick different classes may be at most twice the share by which that existing path differs from the fp32 CPU
oracle on the same inputs; the test measures and prints both on every run.  Measured on an MI355X (2 samples of 64 x 96): the existing
path differs from the oracle in 8.7891e-03 of the pixels (BF16_EXISTING_VS_ORACLE_SHARE), Predictor from the existing path in none."""
import ctypes as C
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
from oracle import loss_metric as olm  # noqa: E402  (checker only)
from oracle import model as omodel  # noqa: E402
import util_val  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
CW = olm.class_weights(-0.125)
CONF_ABS_MEASURED = 1.302e-07       # MI355X, the logits of test_logits_predict_vs_torch
CONF_ABS_TOL = 6e-07                # 4 x 1.302e-07 = 5.2e-07, rounded up to one significant digit
BF16_EXISTING_VS_ORACLE_SHARE = 8.7891e-03      # MI355X; on that run Predictor and the existing path differed in no pixel
GAP_PIXELS_CAP = 31                 # val_small.json: pixels of all five samples whose top-two gap is below util_val.MIN_REL_GAP


def _logits_predict(logits, n_valid=None, conf=True):
    """dc_logits_predict into buffers pre-filled with sentinels (mask 255, confidence -1), counts zeroed"""
    B, _, H, W = logits.shape
    mask = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV)
    cf = torch.full((B, H, W), -1.0, dtype=torch.float32, device=DEV) if conf else None
    cnt = torch.zeros((B, 3), dtype=torch.int64, device=DEV)
    L.call("dc_logits_predict", B, B if n_valid is None else n_valid, H, W, L.dptr(logits), L.dptr(mask), L.dptr(cf), L.dptr(cnt), L.stream_ptr())
    torch.cuda.synchronize()
    return mask, cf, cnt


def _bincount(mask):
    """[n,H,W] class map -> int64 [n,3] on the CPU"""
    m = torch.as_tensor(mask).cpu().long()
    return torch.stack([torch.bincount(s.reshape(-1), minlength=3) for s in m])


# ------------------------------------------------------------------------------------------------------------------ 1. dc_logits_predict
def test_logits_predict_vs_torch():
    g = torch.Generator().manual_seed(31)
    B, nv, H, W = 3, 2, 10, 64
    logits = (torch.randn(B, 3, H, W, generator=g) * 3)
    mask, conf, cnt = _logits_predict(logits.to(DEV), n_valid=nv)
    ref = torch.from_numpy(olm.argmax_first(logits))
    assert torch.equal(mask[:nv].cpu().long(), ref[:nv])
    assert torch.equal(cnt[:nv].cpu(), _bincount(ref[:nv]))
    # the padded sample: not read, nothing written
    assert bool((mask[nv:] == 255).all()) and bool((conf[nv:] == -1.0).all()) and int(cnt[nv:].abs().sum()) == 0
    p = torch.softmax(logits[:nv].double(), dim=1).amax(dim=1)
    err = float((conf[:nv].cpu().double() - p).abs().max())
    print(f"confidence vs fp64 softmax: max abs error {err:.3e} (recorded {CONF_ABS_MEASURED}, allowed {CONF_ABS_TOL})")
    assert CONF_ABS_TOL is not None, "the measured confidence error has not been recorded"
    assert err <= CONF_ABS_TOL
    assert float(conf[:nv].min()) >= 1.0 / 3.0 - 1e-6 and float(conf[:nv].max()) <= 1.0
    # without the optional outputs
    m2 = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV)
    L.call("dc_logits_predict", B, B, H, W, L.dptr(logits.to(DEV)), L.dptr(m2), None, None, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(m2.cpu().long(), ref)


def test_logits_predict_ties_kat(golden_dir):
    z = np.load(os.path.join(golden_dir, "loss_kat.npz"))
    logits = torch.from_numpy(z["ties_logit"])
    mask, conf, cnt = _logits_predict(logits.to(DEV))
    assert torch.equal(mask.cpu().long(), torch.from_numpy(z["ties_pred"]))            # the reference's torch.max on exact ties: the first maximum
    assert torch.equal(mask.cpu().long(), torch.from_numpy(olm.argmax_first(logits)))
    assert torch.equal(cnt.cpu(), _bincount(z["ties_pred"]))
    assert len(np.unique(z["ties_pred"])) > 1


def test_predict_from_logits_wrapper():
    g = torch.Generator().manual_seed(32)
    logits = (torch.randn(2, 3, 16, 40, generator=g) * 2).to(DEV)
    mask, conf, cnt = dnn.predict_from_logits(logits, confidence=True)
    rm, rc, rn = _logits_predict(logits)
    torch.cuda.synchronize()
    assert mask.dtype == torch.uint8 and conf.dtype == torch.float32 and cnt.dtype == torch.int64
    assert torch.equal(mask, rm) and torch.equal(conf, rc) and torch.equal(cnt, rn)
    assert dnn.predict_from_logits(logits)[1] is None


# ------------------------------------------------------------------------------------------------------------------ 2. head
@pytest.mark.parametrize("bnin", [False, True], ids=["plain", "bnin"])
@pytest.mark.parametrize("N,nv,Hi,Wi", [(2, 2, 8, 32), (3, 2, 6, 40), (3, 3, 5, 200)])
def test_head_fwd_predict_vs_head_fwd_plus_logits_predict(bnin, N, nv, Hi, Wi):
    """The shapes of test_val_gpu.py::test_head_fwd_score_vs_head_fwd_plus_wce_score: partial tile rows, a partial last tile, more than one
    strip; every pixel belongs to its own sample and none beyond n_valid is written."""
    g = torch.Generator().manual_seed(19)
    ld = 256
    x = (torch.randn(N, Hi, Wi, ld, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    w = (torch.randn(256, 3, 3, 3, generator=g) * 0.05).to(DEV)
    scale = (torch.rand(256, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(256, generator=g) * 0.2).to(DEV)
    ws = torch.empty(L.load().dc_head_workspace(L.DC_BF16, N, 256, Hi, Wi) + 256, dtype=torch.uint8, device=DEV)
    wp = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    logits = torch.zeros(N, 3, 2 * Hi, 2 * Wi, device=DEV)
    st = L.stream_ptr()
    if bnin:
        L.call("dc_head_fwd_bnin", L.DC_BF16, N, 256, Hi, Wi, L.dptr(x), ld, L.dptr(scale), L.dptr(shift), 1, L.dptr(w), L.dptr(logits), wp, st)
    else:
        L.call("dc_head_fwd", L.DC_BF16, N, 256, Hi, Wi, L.dptr(x), ld, L.dptr(w), L.dptr(logits), wp, st)
    rmask, rconf, rcnt = _logits_predict(logits, n_valid=nv)
    assert len(torch.unique(rmask[:nv])) == 3                              # the inputs exercise every class
    for store, with_conf in ((True, True), (False, True), (False, False)):
        mask = torch.full((N, 2 * Hi, 2 * Wi), 255, dtype=torch.uint8, device=DEV)
        conf = torch.full((N, 2 * Hi, 2 * Wi), -1.0, dtype=torch.float32, device=DEV) if with_conf else None
        cnt = torch.zeros((N, 3), dtype=torch.int64, device=DEV)
        lg = torch.zeros_like(logits) if store else None
        tail = (L.dptr(lg), wp, L.dptr(mask), L.dptr(conf), L.dptr(cnt), st)
        if bnin:
            L.call("dc_head_fwd_predict_bnin", L.DC_BF16, N, nv, 256, Hi, Wi, L.dptr(x), ld, L.dptr(scale), L.dptr(shift), 1, L.dptr(w), *tail)
        else:
            L.call("dc_head_fwd_predict", L.DC_BF16, N, nv, 256, Hi, Wi, L.dptr(x), ld, L.dptr(w), *tail)
        torch.cuda.synchronize()
        assert torch.equal(mask, rmask), f"store={store}"                  # (the rows from n_valid on: the sentinel on both sides)
        assert torch.equal(cnt, rcnt), f"store={store}"
        if with_conf:
            assert torch.equal(conf, rconf), f"store={store}"
        if store:
            assert torch.equal(lg[:nv], logits[:nv])                       # dc_head_fwd's logits, bit for bit
            assert int(lg[nv:].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ 3 - 5. Predictor
def _net(dtype, state):
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=dtype, seed=333)
    net.materialize(2, util_val.H, util_val.W)
    net.load_state_dict(state)
    net.eval()
    return net


@pytest.fixture(scope="module")
def state():
    return util_val.perturbed_state()


@pytest.fixture(scope="module")
def net_f32(state):
    return _net(torch.float32, state)


@pytest.fixture(scope="module")
def net_bf16(state):
    return _net(torch.bfloat16, state)


@pytest.fixture(scope="module")
def fixture_inputs(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "val_small.json")))
    x, _ = util_val.val_inputs(seed=g["input_seed"])
    return g, x


@pytest.fixture(scope="module")
def oracle_logits(state, fixture_inputs):
    """fp32 CPU oracle's eval logits of the fixture's five samples, computed once, batch 1 as the reference's validation loop runs"""
    _, x = fixture_inputs
    with torch.no_grad():
        return torch.cat([omodel.forward(state, x[i:i + 1], training=False) for i in range(x.shape[0])])


def _predict_all(net, x, batch, confidence=False):
    """Every sample of x through a Predictor of this batch size, the last batch padded with zeros: masks, counts (CPU)."""
    n = x.shape[0]
    pr = dnn.Predictor(net, batch, x.shape[2], x.shape[3], confidence=confidence)
    masks, counts = [], []
    try:
        for b0 in range(0, n, batch):
            nv = min(batch, n - b0)
            xb = torch.zeros((batch,) + tuple(x.shape[1:]))
            xb[:nv] = x[b0:b0 + nv]
            m = pr(xb.to(DEV), n_valid=nv)
            assert m.dtype == torch.uint8 and tuple(m.shape) == (nv, x.shape[2], x.shape[3]) and pr.class_counts.shape == (nv, 3)
            masks.append(m.cpu())
            counts.append(pr.class_counts.cpu())
    finally:
        pr.close()
    return torch.cat(masks), torch.cat(counts)


@pytest.mark.parametrize("batch", [1, 2, 8], ids=["b1", "b2", "b8_nvalid5"])
def test_predictor_fp32_vs_reference_fixture(fixture_inputs, oracle_logits, net_f32, batch):
    g, x = fixture_inputs
    assert g["pixels_below_gap_all"] == GAP_PIXELS_CAP
    mask, counts = _predict_all(net_f32, x, batch)
    assert torch.equal(counts, _bincount(mask))
    ref_counts = torch.tensor([[s["tp"][j] + s["fp"][j] for j in range(3)] for s in g["samples"]], dtype=torch.int64)
    omask = torch.from_numpy(olm.argmax_first(oracle_logits))
    assert torch.equal(_bincount(omask), ref_counts)                      # the oracle reproduces the reference's predicted pixels per class
    differ = mask.long() != omask
    gap = util_val.rel_gap(oracle_logits)
    ndiff = int(differ.sum())
    cdiff = int((counts - ref_counts).abs().sum())
    print(f"batch {batch}: {ndiff} pixels differ from the oracle (largest gap among them "
          f"{float(gap[differ].max()) if ndiff else 0.0:.3e}); sum |class_counts - (tp + fp)| = {cdiff}")
    assert bool((gap[differ] < util_val.MIN_REL_GAP).all())               # only where the top two logits are closer than 1e-3
    assert ndiff <= GAP_PIXELS_CAP
    assert cdiff <= 2 * ndiff


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_predictor_self_consistency(fixture_inputs, oracle_logits, net_f32, net_bf16, dtype):
    net = net_f32 if dtype == torch.float32 else net_bf16
    _, x5 = fixture_inputs
    x = x5[:2]
    pr = dnn.Predictor(net, 2, util_val.H, util_val.W, confidence=True)
    try:
        pr.store_logits = True
        mask = pr(x.to(DEV))
        got = mask.cpu().long()
        assert torch.equal(got, torch.from_numpy(olm.argmax_first(pr.logits.cpu())))
        assert torch.equal(pr.class_counts.cpu(), _bincount(got))
        rm, rc, rn = _logits_predict(pr.logits.contiguous())
        assert torch.equal(mask, rm) and torch.equal(pr.confidence, rc) and torch.equal(pr.class_counts, rn)
        if dtype == torch.bfloat16:
            pr.store_logits = False                                       # the logits never leave the kernel: the same mask
            assert torch.equal(pr(x.to(DEV)).cpu().long(), got)
    finally:
        pr.close()
    if dtype != torch.bfloat16:
        return
    eng = net.engine_for(shape=(1, 16, util_val.H, util_val.W))
    old = torch.cat([torch.max(eng.forward(x[i:i + 1].to(DEV), train=False), 1)[1].cpu() for i in range(2)])
    omask = torch.from_numpy(olm.argmax_first(oracle_logits[:2]))
    existing_share = float((old != omask).float().mean())
    share = float((got != old).float().mean())
    print(f"bf16: existing batch-1 path vs fp32 oracle: {existing_share:.4e} of the pixels differ (recorded {BF16_EXISTING_VS_ORACLE_SHARE}); "
          f"Predictor batch 2 vs existing path: {share:.4e} (allowed {2 * existing_share:.4e})")
    assert share <= 2 * existing_share


def test_predictor_contract(state):
    x, y = util_val.val_inputs(n=2, seed=util_val.INPUT_SEED + 90)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.float32, seed=333)
    with pytest.raises(L.DeepcamHipError):
        dnn.Predictor(net, 2, util_val.H, util_val.W)                     # nothing to share before materialize
    net.materialize(2, util_val.H, util_val.W)
    net.load_state_dict(state)
    net.eval()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    pr = dnn.Predictor(net, 2, util_val.H, util_val.W)
    eng = pr.eng
    assert torch.cuda.memory_allocated() > m0 and eng.forward_only and eng.bwd == [] and eng.fwd_train == []
    assert pr.confidence is None and pr.store_logits is False
    pr.store_logits = True
    # either labels to score against or a prediction, not both
    eng.score_args = {"labels": y.to(DEV), "weight": dnn._cw_tensor(CW, DEV), "n_valid": 2, "loss_sum": torch.zeros(2, dtype=torch.float64, device=DEV),
                      "counts": torch.zeros((2, 9), dtype=torch.int64, device=DEV), "store_logits": True}
    with pytest.raises(L.DeepcamHipError):
        pr(x.to(DEV))
    eng.score_args = None
    assert eng.predict_args is None                                       # the failed call has put it back
    with pytest.raises(L.DeepcamHipError):
        pr(x.to(DEV), n_valid=3)
    before = pr(x.to(DEV)).clone()
    assert torch.equal(before.cpu().long(), torch.from_numpy(olm.argmax_first(pr.logits.cpu())))
    # n_valid = 1: the second sample's bytes stay as the previous call left them
    pr._mask[0].fill_(255)
    one = pr(x.to(DEV), n_valid=1)
    assert tuple(one.shape) == (1, util_val.H, util_val.W) and torch.equal(one[0], before[0]) and torch.equal(pr._mask[1], before[1])
    assert tuple(pr.class_counts.shape) == (1, 3) and int(pr.class_counts.sum()) == util_val.H * util_val.W
    # one optimizer step on the shared arena (weights AND running statistics move): the next mask is that of the new state
    opt = dnn.make_optimizer("Adam", net, 1e-3, 1e-8, 0.0)
    net.train()
    dnn.TrainStep(net, opt, CW, 2, util_val.H, util_val.W)(x.to(DEV), y.to(DEV))
    net.eval()
    after = pr(x.to(DEV))
    assert int((after != before).sum()) >= 1, "the forward-only engine did not see the optimizer step"
    assert torch.equal(after.cpu().long(), torch.from_numpy(olm.argmax_first(pr.logits.cpu())))
    assert torch.equal(pr.class_counts.cpu(), _bincount(after))
    arena = eng.act_bytes
    torch.cuda.synchronize()
    m2 = torch.cuda.memory_allocated()
    del before, after, one
    pr.close()
    torch.cuda.synchronize()
    # the activation arena, the fp32 logits of two samples and the mask buffer are given back
    assert torch.cuda.memory_allocated() <= m2 - arena - 2 * 3 * util_val.H * util_val.W * 4 - 2 * util_val.H * util_val.W
    with pytest.raises(L.DeepcamHipError):
        eng.forward(x.to(DEV), train=False)


def test_compute_score_accepts_uint8_prediction():
    g = torch.Generator().manual_seed(33)
    pred = torch.randint(0, 3, (2, 24, 40), generator=g).to(DEV)
    labels = torch.randint(0, 3, (2, 24, 40), generator=g).to(DEV)
    a = dnn.compute_score(pred.to(torch.uint8), labels)
    b = dnn.compute_score(pred.long(), labels)
    assert float(a) == float(b) and float(a) == pytest.approx(olm.compute_score(pred.cpu().numpy(), labels.cpu()), rel=1e-6)


# ------------------------------------------------------------------------------------------------------------------ 6. unlabelled input, driver
def _unlabelled_dir(tmp_path, n=5):
    """n CAM5-shaped files without climate/labels_0 at 64 x 96, a stats file, and the normalised NCHW batch they stand for"""
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    root = str(tmp_path / "unlabelled")
    os.makedirs(root)
    rs = np.random.RandomState(11)
    fields = [(rs.rand(util_val.H, util_val.W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in range(n)]
    for i, d in enumerate(fields):
        with h5lite.File(os.path.join(root, f"data-{i:02d}.h5"), "w") as f:
            f.write("climate/data", d)
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", lo)
        f.write("climate/maxval", hi)
    return root, stats


def test_pipeline_over_unlabelled_files_yields_none_labels_and_the_ragged_batch(tmp_path):
    from mlperf_deepcam_amd import data as ddata
    root, stats = _unlabelled_dir(tmp_path)
    ds = ddata.CamDataset(root, stats, list(range(16)), allow_uneven_distribution=True, labels=False)
    pipe = ddata.InputPipeline(ds, 2, dtype=torch.float32, depth=2, workers=2, drop_last=False)
    assert len(pipe) == 3 and all(s.label is None and s.label_host is None for s in pipe.slots)
    seen, fills = [], []
    host = np.empty(tuple(ds.data_shape), np.float32)
    for x, y, names in pipe:
        assert y is None and tuple(x.shape) == (2, util_val.H, util_val.W, 16)
        assert pipe.n_valid == len(names)
        fills.append(pipe.n_valid)
        for j, name in enumerate(names):
            ds.read_into(ds.files.index(name), host, None)
            ref = torch.from_numpy(ds.data_scale * (host - ds.data_shift))
            assert torch.equal(x[j].cpu(), ref)
        seen += names
    assert fills == [2, 2, 1] and seen == ds.files
    assert len(ddata.InputPipeline(ds, 2, dtype=torch.float32, depth=2)) == 2          # the default drops the ragged batch, as before


def test_predict_cli(tmp_path, state):
    from mlperf_deepcam_amd import data as ddata
    from mlperf_deepcam_amd import h5lite
    root, stats = _unlabelled_dir(tmp_path)
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": state}, ckpt)
    out = str(tmp_path / "masks")
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.predict", "--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--output_dir", out,
           "--batch_size", "2", "--confidence", "--dtype", "fp32", "--height", str(util_val.H), "--width", str(util_val.W),
           "--max_inter_threads", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    summary = json.load(open(os.path.join(out, "summary.json")))
    names = [f"data-{i:02d}.h5" for i in range(5)]
    assert sorted(x for x in os.listdir(out) if x.endswith(".h5")) == names
    assert [rec["file"] for rec in summary["files"]] == names and line["samples"] == 5 and line["samples_per_second"] > 0
    # the same files through the Predictor in this process, batched as the driver batches them (2, 2 and the ragged 1)
    net = _net(torch.float32, state)
    ds = ddata.CamDataset(root, stats, list(range(16)), allow_uneven_distribution=True, labels=False)
    assert [os.path.basename(f) for f in ds.files] == names
    pr = dnn.Predictor(net, 2, util_val.H, util_val.W, confidence=True)
    masks, confs = [], []
    try:
        for x, _, fn in ddata.InputPipeline(ds, 2, dtype=torch.float32, depth=2, workers=1, drop_last=False):
            masks.append(pr(x, n_valid=len(fn)).cpu())
            confs.append(pr.confidence.cpu())
    finally:
        pr.close()
    mask, conf = torch.cat(masks), torch.cat(confs)
    assert mask.shape[0] == 5
    tot = np.zeros(3, np.int64)
    for i, name in enumerate(names):
        with h5lite.File(os.path.join(out, name)) as f:
            p, c = f.read("prediction"), f.read("confidence")
        assert p.dtype == np.uint8 and p.shape == (util_val.H, util_val.W) and c.dtype == np.float32 and c.shape == p.shape
        assert torch.equal(torch.from_numpy(p), mask[i]), name
        assert torch.equal(torch.from_numpy(c), conf[i]), name
        rec = summary["files"][i]
        assert rec["class_counts"] == np.bincount(p.reshape(-1), minlength=3).tolist()
        assert rec["mean_confidence"] == pytest.approx(float(c.mean(dtype=np.float64)), rel=1e-12)
        tot += np.bincount(p.reshape(-1), minlength=3)
    assert summary["class_counts"] == tot.tolist() == line["class_counts"] and int(tot.sum()) == 5 * util_val.H * util_val.W
