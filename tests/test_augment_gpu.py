"""Train-time augmentation on the GPU (dc_augment_view_hwc of csrc/augment.hip; data.Augment, data.InputPipeline(augment=...), data.to_source;
train.py --augment_*).  The kernel moves and normalises, so every comparison is equality: sample n of a batch is what dc_input_view_hwc
(nn.view_input) writes for that sample alone in its own view, a batch of identity views is dc_input_normalize_hwc, and the labels are
torch.roll / flip of the 64-bit words.
The shapes are the smallest that reach every path: (5, 12) -- 4-byte gathers with the channel subset, an odd row count -- and (8, 64), both
at batch 3 with 16-byte loads where all 16 file channels are taken; batch 256 at (2, 8) reads every word of the views table.  Outputs sit
inside 64 sentinel elements on both sides."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import data as ddata  # noqa: E402
from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_augment as ua  # noqa: E402
from util_launch import served, assert_served  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
GUARD = 64
CFILE = 16
SUBSET = [1, 2, 4, 7, 8, 11, 13, 15]
NEGATE = [4, 13]                                     # file channels
LABEL_SENTINEL = 0x5A5A5A5A5A5A5A5A


class _Case:
    """a raw batch, its labels and the normalisation constants on the device"""

    def __init__(self, B, H, W, subset, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.H, self.W = B, H, W
        self.raw = (torch.rand(B, H, W, CFILE, generator=g) * torch.linspace(1, 300, CFILE) - 40.0).to(DEV)
        self.file_channels = SUBSET if subset else list(range(CFILE))
        self.C = len(self.file_channels)
        self.channels = torch.tensor(SUBSET, dtype=torch.int32, device=DEV) if subset else None
        self.shift = (torch.rand(self.C, generator=g) * 50 - 40).to(DEV)
        self.scale = (1.0 / (torch.rand(self.C, generator=g) * 300 + 1)).to(DEV)
        self.flip_sign = torch.tensor([-1.0 if c in NEGATE else 1.0 for c in self.file_channels], dtype=torch.float32, device=DEV)
        lab = torch.randint(0, 3, (B, H, W), generator=g, dtype=torch.int64)
        lab.view(-1)[3], lab.view(-1)[H * W + 5] = -1, 7                  # not interpreted: moved like every other word
        self.labels = lab.to(DEV)


def _guarded(n, dtype, fill):
    """(the whole store, its n payload elements): 64 sentinel elements in front and behind; the payload is sentinel-filled too"""
    store = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return store, store[GUARD:GUARD + n]


def _augment(case, dtype, views, flip_sign, with_labels=True, ldo=None):
    """One dc_augment_view_hwc on guarded, sentinel-filled outputs: (out [B, H, W, ldo], labels_out [B, H, W] or None, the launch names,
    (the whole output store, its state before the call, the same two of the labels)).  Asserts that the guards are intact."""
    B, H, W, C_ = case.B, case.H, case.W, case.C
    ldo = C_ if ldo is None else ldo
    ostore, opay = _guarded(B * H * W * ldo, dtype, -777.0)
    lstore, lpay = _guarded(B * H * W, torch.int64, LABEL_SENTINEL)
    obefore, lbefore = ostore.clone(), lstore.clone()
    views = np.ascontiguousarray(np.asarray(views, np.int32).reshape(B, 2))
    with served("dc_augment_view_hwc") as names:
        L.call("dc_augment_view_hwc", L.dtype_code(dtype), B, H, W, CFILE, C_, L.dptr(case.channels), L.dptr(flip_sign), L.dptr(case.raw),
               L.dptr(case.shift), L.dptr(case.scale), C.c_void_p(views.ctypes.data), L.dptr(case.labels if with_labels else None),
               L.dptr(lpay if with_labels else None), L.dptr(opay), ldo, L.stream_ptr())
    torch.cuda.synchronize()
    for store, before, what in ((ostore, obefore, "out"), (lstore, lbefore, "labels_out")):
        assert torch.equal(store[:GUARD], before[:GUARD]) and torch.equal(store[-GUARD:], before[-GUARD:]), f"a guard element of {what} was written"
    return opay.view(B, H, W, ldo), (lpay.view(B, H, W) if with_labels else None), names, (ostore, obefore, lstore, lbefore)


def _normalize(case, dtype):
    out = torch.empty((case.B, case.H, case.W, case.C), dtype=dtype, device=DEV)
    L.call("dc_input_normalize_hwc", L.dtype_code(dtype), case.B * case.H * case.W, CFILE, case.C, L.dptr(case.channels), L.dptr(case.raw),
           L.dptr(case.shift), L.dptr(case.scale), L.dptr(out), case.C, L.stream_ptr())
    return out


def _moved_labels(lab, roll, flip):
    return torch.roll(lab.flip(0) if flip else lab, -roll, 1)


def _check_batch(case, dtype, views, negate, out, labels_out):
    for n, (roll, flip) in enumerate(views):
        want = dnn.view_input(case.raw[n:n + 1], case.channels, case.shift, case.scale, roll, bool(flip), NEGATE if flip and negate else None, dtype=dtype)
        assert torch.equal(out[n], want[0]), (n, roll, flip, negate)
        if labels_out is not None:
            assert torch.equal(labels_out[n], _moved_labels(case.labels[n], roll, flip)), (n, roll, flip)


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("subset", [False, True], ids=["all16", "subset8"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(5, 12), (8, 64)])
def test_every_sample_is_its_own_view_and_the_labels_move_with_it(H, W, dtype, subset):
    case = _Case(3, H, W, subset, 17 + H)
    C_ = case.C
    identity = [(0, 0)] * 3
    for views in ([(0, 0), (W - 1, 1), (W // 2, 0)], [(1, 1), (0, 1), (5, 0)], identity):
        for sign in (case.flip_sign, None):
            out, lab, names, _ = _augment(case, dtype, views, sign)
            assert_served(names, "augment_view")
            assert out.dtype == dtype
            _check_batch(case, dtype, views, sign is not None, out, lab)
            # the label-free form gives the same data and writes no label
            out2, _, names, (_, _, lstore, lbefore) = _augment(case, dtype, views, sign, with_labels=False)
            assert_served(names, "augment_view")
            assert torch.equal(out2, out) and torch.equal(lstore, lbefore)
            if views is identity:                                             # ... whatever the sign: nothing is mirrored
                assert torch.equal(out, _normalize(case, dtype)) and torch.equal(lab, case.labels)
    # a wider leading dimension: the gap stays sentinel
    views = [(1, 1), (0, 1), (5, 0)]
    out, lab, names, (ostore, obefore, _, _) = _augment(case, dtype, views, case.flip_sign, ldo=C_ + 8)
    assert_served(names, "augment_view")
    _check_batch(case, dtype, views, True, out[..., :C_], lab)
    assert torch.equal(out[..., C_:], obefore[GUARD:-GUARD].view(out.shape)[..., C_:])


# ------------------------------------------------------------------------------------------------------------------ 2. the full table
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_batch_of_256_reads_every_word_of_the_views_table(dtype):
    H, W = 2, 8
    case = _Case(256, H, W, False, 29)
    views = [(n % 8, (n // 8) % 2) for n in range(256)]
    out, lab, names, _ = _augment(case, dtype, views, case.flip_sign)
    assert_served(names, "augment_view")
    # dc_input_view_hwc gives one view to a whole batch: sixteen calls, sample n taken from the call with its view
    for roll, flip in sorted(set(views)):
        whole = dnn.view_input(case.raw, None, case.shift, case.scale, roll, bool(flip), NEGATE if flip else None, dtype=dtype)
        mine = [n for n, v in enumerate(views) if v == (roll, flip)]
        assert len(mine) == 16 and torch.equal(out[mine], whole[mine]), (roll, flip)
    for n, (roll, flip) in enumerate(views):
        assert torch.equal(lab[n], _moved_labels(case.labels[n], roll, flip)), n
    ident, lab0, _, _ = _augment(case, dtype, [(0, 0)] * 256, case.flip_sign)
    assert torch.equal(ident, _normalize(case, dtype)) and torch.equal(lab0, case.labels)


# ------------------------------------------------------------------------------------------------------------------ 3. refused calls
def test_refused_calls_launch_nothing_and_leave_the_outputs_untouched():
    """every refusal raises, the launch record of the whole block is empty and every output element is still the sentinel"""
    H, W = 5, 12
    case = _Case(3, H, W, False, 31)
    n = 3 * H * W
    out = torch.full((n * case.C,), -777.0, device=DEV)
    lab = torch.full((n,), LABEL_SENTINEL, dtype=torch.int64, device=DEV)
    good = np.asarray([(1, 1), (0, 0), (5, 0)], np.int32)

    def call(B=3, views=good, dt=L.DC_F32, lin=case.labels, lout=lab, ldo=case.C, vnull=False):
        views = np.ascontiguousarray(views, np.int32)
        L.call("dc_augment_view_hwc", dt, B, H, W, CFILE, case.C, None, L.dptr(case.flip_sign), L.dptr(case.raw), L.dptr(case.shift),
               L.dptr(case.scale), C.c_void_p(0) if vnull else C.c_void_p(views.ctypes.data), L.dptr(lin), L.dptr(lout), L.dptr(out), ldo,
               L.stream_ptr())
    bad_calls = [dict(B=0), dict(B=257, views=np.zeros((257, 2), np.int32)), dict(views=[(1, 1), (W, 0), (5, 0)]), dict(views=[(1, 1), (0, 0), (-1, 0)]),
                 dict(views=[(1, 2), (0, 0), (5, 0)]), dict(lout=None), dict(lin=None), dict(lin=lab), dict(vnull=True), dict(dt=2),
                 dict(ldo=case.C - 1)]
    with served("refused") as names:
        for k, kw in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                call(**kw)
                pytest.fail(f"call {k} ({kw}) was accepted")
    assert names == []
    torch.cuda.synchronize()
    assert bool((out == -777.0).all()) and bool((lab == LABEL_SENTINEL).all())
    call()                                                                    # and the good call is accepted
    torch.cuda.synchronize()
    assert not bool((out == -777.0).any()) and not bool((lab == LABEL_SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------------ 4. the pipeline
SEED = 3
N_SAMPLES, PB, PH, PW = 7, 3, 8, 64
PNEG = (2, 4)


def _host_draws():
    names = [f"data-synthetic-{i:06d}.h5" for i in range(N_SAMPLES)]
    return [ua.draws(SEED, e, names, PW) for e in (0, 1)]


def _check_aug_batch(aug, plain, got, ref, epoch, dtype):
    (xa, la, na), (xp, lp, npl) = got, ref
    assert na == npl and aug.n_valid == plain.n_valid == len(na)
    assert torch.equal(aug.raw, plain.raw)                                    # SOURCE coordinates, as the files store them
    views = aug.views
    assert views.dtype == np.int32 and views.shape == (PB, 2) and (views == ua.slot_views(SEED, epoch, na, PB, PW)).all()
    assert plain.views is None
    for n, (roll, flip) in enumerate(views.tolist()):
        want = dnn.view_input(plain.raw[n:n + 1], plain.channels, plain.shift, plain.scale, roll, bool(flip), list(PNEG) if flip else None, dtype=dtype)
        assert torch.equal(xa[n], want[0]), (epoch, na, n)
        assert torch.equal(la[n], _moved_labels(lp[n], roll, flip))
    assert torch.equal(ddata.to_source(la, views), lp)
    return views


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pipeline_stages_every_sample_in_its_own_view(dtype):
    d0, d1 = _host_draws()
    for d in (d0, d1):                                                        # the seed shows every kind of view, in both epochs
        assert (d[:, 1] == 1).any() and (d[:, 1] == 0).any() and (d[:, 0] != 0).any()
    assert (d0 != d1).any()
    ds = ddata.SyntheticHWC(N_SAMPLES, PH, PW)
    plain = ddata.InputPipeline(ds, PB, dtype=dtype, device=DEV)
    aug = ddata.InputPipeline(ds, PB, dtype=dtype, device=DEV, augment=ddata.Augment(roll=True, flip_lat=True, negate=PNEG, seed=SEED))
    assert aug.views is None and len(aug) == len(plain) == 2
    seen = []
    for epoch in (0, 1):                                                      # without set_epoch: the count of passes started
        with served("an augmented pass") as names:
            it_plain = iter(plain)
            batches = 0
            for got in aug:
                seen.append((epoch, _check_aug_batch(aug, plain, got, next(it_plain), epoch, dtype)))
                batches += 1
            assert next(it_plain, None) is None and batches == 2
        # one launch per batch stages data and labels; the plain pipeline's normalise kernel is a generic launch, and the comparison's
        # own nn.view_input calls are in the record too
        assert names.count("augment_view") == 2 and names.count("aux") == 2 and set(names) == {"augment_view", "aux", "view_normalize"}
    e0 = np.concatenate([v for e, v in seen if e == 0])
    e1 = np.concatenate([v for e, v in seen if e == 1])
    assert (e0 == d0[:6]).all() and (e1 == d1[:6]).all() and (e0 != e1).any()
    with served("a plain pass") as names:
        for _ in plain:
            pass
    assert names == ["aux", "aux"]
    # a ragged last batch: the padding slots repeat the last sample and take its view; set_epoch names the epoch
    plain_r = ddata.InputPipeline(ds, PB, dtype=dtype, device=DEV, drop_last=False)
    aug_r = ddata.InputPipeline(ds, PB, dtype=dtype, device=DEV, drop_last=False,
                                augment=ddata.Augment(roll=True, flip_lat=True, negate=PNEG, seed=SEED))
    aug_r.set_epoch(1)
    it_plain = iter(plain_r)
    last = None
    with served("a ragged pass") as names:
        for got in aug_r:
            views = _check_aug_batch(aug_r, plain_r, got, next(it_plain), 1, dtype)
            last = (got, views)
        assert next(it_plain, None) is None
    assert names.count("augment_view") == 3
    (xa, la, na), views = last
    assert len(na) == 1 and (views == d1[6]).all() and int(d1[6][1]) == 1     # the last sample is a mirrored one
    assert torch.equal(xa[1], xa[0]) and torch.equal(xa[2], xa[0]) and torch.equal(la[1], la[0]) and torch.equal(la[2], la[0])
    torch.cuda.synchronize()


def test_pipeline_refusals():
    ds = ddata.SyntheticHWC(4, 8, 64)
    a = ddata.Augment(roll=True)
    with pytest.raises(ValueError):
        ddata.InputPipeline(ds, 2, dtype=torch.float32, device=DEV, layout="nchw", augment=a)
    with pytest.raises(ValueError):
        ddata.InputPipeline(ddata.SyntheticHWC(4, 8, 64, channels=[0, 1, 2, 3]), 2, dtype=torch.float32, device=DEV,
                            augment=ddata.Augment(flip_lat=True, negate=(5,)))

    class _Unlabelled(ddata.SyntheticHWC):
        labels = False
    with pytest.raises(ValueError):
        ddata.InputPipeline(_Unlabelled(4, 8, 64), 2, dtype=torch.float32, device=DEV, augment=a)


# ------------------------------------------------------------------------------------------------------------------ 5. the driver
def test_driver_trains_on_augmented_batches(tmp_path):
    out = str(tmp_path / "run")
    cmd = [sys.executable, "-m", "mlperf_deepcam_amd.train", "--wireup_method", "single", "--run_tag", "aug", "--output_dir", out,
           "--synthetic_samples", "8", "--local_batch_size", "2", "--height", "64", "--width", "96", "--max_epochs", "2",
           "--logging_frequency", "1", "--validation_frequency", "4", "--augment_roll", "--augment_flip_lat", "--augment_negate", "2", "4",
           "--augment_seed", "5", "--plots", "--training_visualization_frequency", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ev = [json.loads(line[len(":::MLLOG "):]) for line in r.stdout.splitlines() if line.startswith(":::MLLOG ")]
    aug = [e["value"] for e in ev if e["key"] == "data_augmentation"]
    assert aug == [{"roll": True, "flip_lat": True, "negate": [2, 4], "seed": 5}]
    losses = [e["value"] for e in ev if e["key"] == "train_loss"]
    assert len(losses) == 8 and all(np.isfinite(v) for v in losses)
    assert any(e["key"] == "eval_accuracy" for e in ev)
    plots = sorted(f for f in os.listdir(os.path.join(out, "plots")) if f.startswith("training-") and f.endswith(".png"))
    assert plots, "no training picture was written"
