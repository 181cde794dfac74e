"""The batched validation step without a GPU: the fixture from the reference (tests/golden/val_small.json) against the CPU oracle, the
C ABI's new entry points in header and binding table, and the driver's flag."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import loss_metric as olm
from oracle import model as omodel
from util_inputs import sample_index
import util_val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_W = olm.class_weights(-0.125)
NEW_SYMBOLS = ["dc_wce_score", "dc_head_fwd_score", "dc_head_fwd_score_bnin", "dc_val_accumulate", "dc_bn_eval_coeffs_all"]


def test_perturbed_state_moves_every_tensor():
    sd0, sd = omodel.init_state(333), util_val.perturbed_state()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        assert not torch.equal(v, sd0[k]), k
        if k.endswith("running_mean"):
            assert float(v.abs().max()) > 0
        if k.endswith("running_var"):
            assert float(v.min()) >= 0.8 and float(v.max()) <= 1.25 and float((v - 1).abs().max()) > 0


def test_oracle_reproduces_val_small(golden_dir):
    """The tolerances test_oracle_golden.py holds eval_b1 to: logits rtol 1e-4 / atol 1e-5, loss and IoU rel 1e-5."""
    g = json.load(open(os.path.join(golden_dir, "val_small.json")))
    assert (g["H"], g["W"]) == (util_val.H, util_val.W) and len(g["samples"]) == util_val.N_SAMPLES
    assert g["min_rel_gap_sampled"] >= util_val.MIN_REL_GAP
    sd = util_val.perturbed_state(g["state_seed"])
    x, y = util_val.val_inputs(seed=g["input_seed"])
    losses, ious = [], []
    for i, ref in enumerate(g["samples"]):
        with torch.no_grad():
            out = omodel.forward(sd, x[i:i + 1], training=False)
        idx = sample_index(out.numel())
        np.testing.assert_allclose(out.flatten()[idx].numpy(), np.array(ref["logit_samples"]), rtol=1e-4, atol=1e-5)
        loss = float(olm.fp_loss(out, y[i:i + 1], CLASS_W))
        pred = olm.argmax_first(out)
        iou = olm.compute_score(pred, y[i:i + 1])
        assert loss == pytest.approx(ref["loss"], rel=1e-5)
        assert iou == pytest.approx(ref["iou"], rel=1e-5)
        tp, fp, fn = olm.confusion_counts(pred, y[i:i + 1].numpy())
        assert (list(tp), list(fp), list(fn)) == (ref["tp"], ref["fp"], ref["fn"])
        assert olm.iou_from_counts(tp, fp, fn) == pytest.approx(ref["iou"], rel=1e-6)
        losses.append(loss)
        ious.append(iou)
    assert float(np.mean(losses)) == pytest.approx(g["mean_loss"], rel=1e-5)
    assert float(np.mean(ious)) == pytest.approx(g["mean_iou"], rel=1e-5)


def test_new_symbols_are_declared_and_bound():
    from mlperf_deepcam_amd import lib as L
    src = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in deepcam_hip.h"
        assert name in L.EXPORTS and hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(L.BnEvalEntry) == 56


def test_driver_accepts_validation_batch_size():
    from mlperf_deepcam_amd import train
    p = train.build_parser()
    base = ["--run_tag", "t", "--output_dir", "/tmp/x"]
    assert p.parse_args(base).validation_batch_size == 1
    assert p.parse_args(base + ["--validation_batch_size", "4"]).validation_batch_size == 4
