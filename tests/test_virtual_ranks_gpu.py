"""Virtual ranks on the GPU: dc_grad_accumulate, TrainStep(virtual_ranks=K) against hand-summed gradients, a real two-rank run, the
BatchNorm buffer rule, the reference's own accumulation loop, the recorded / captured step and the driver.  64 x 96 inputs, B = 2."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
from util_inputs import make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 2, 64, 96
CW = dnn.class_weights(-0.125)


def _dev():
    return torch.device("cuda", 0)


def _net(dtype, seed=333):
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=dtype, seed=seed)
    net.materialize(B, H, W)
    net.train()
    return net


def _batches(K, step=0):
    """micro-batch v of a step: the batch rank v of the two-rank tests sees (tests/virtual_ranks_worker.py: batch(rank, step))"""
    xs, ys = zip(*[make_inputs(B, H, W, seed=1234 + v + 10 * step) for v in range(K)])
    return torch.cat(xs).to(_dev()), torch.cat(ys).to(_dev())


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4096 * 3 + 1])
def test_grad_accumulate_kernel(n):
    """Every offset of both ranges from a 16-byte boundary (head, body and tail paths): first=1 onto NaN gives g exactly, first=0 is torch's
    fp32 acc + g bit for bit, and the float on either side of acc is untouched."""
    dev = _dev()
    gen = torch.Generator().manual_seed(n)
    for off in range(4):
        gbuf = torch.randn(n + 12, generator=gen).to(dev)
        g = gbuf[4 + off:4 + off + n]
        abuf = torch.full((n + 12,), float("nan"), device=dev)
        abuf[4 + off - 1], abuf[4 + off + n] = 7.0, -9.0           # the guards
        acc = abuf[4 + off:4 + off + n]
        gp, ap = C.c_void_p(gbuf.data_ptr() + 4 * (4 + off)), C.c_void_p(abuf.data_ptr() + 4 * (4 + off))      # (an empty view has no pointer)
        assert gp.value % 16 == 4 * off and ap.value % 16 == 4 * off
        L.call("dc_grad_accumulate", n, gp, ap, 1, L.stream_ptr())
        assert torch.equal(acc, g)
        assert float(abuf[4 + off - 1]) == 7.0 and float(abuf[4 + off + n]) == -9.0
        g2buf = (torch.randn(n + 12, generator=gen) * 1e3).to(dev)
        want = acc + g2buf[4 + off:4 + off + n]
        L.call("dc_grad_accumulate", n, C.c_void_p(g2buf.data_ptr() + 4 * (4 + off)), ap, 0, L.stream_ptr())
        assert torch.equal(acc, want)
        assert float(abuf[4 + off - 1]) == 7.0 and float(abuf[4 + off + n]) == -9.0
        assert torch.isnan(abuf[:4 + off - 1]).all() and torch.isnan(abuf[4 + off + n + 1:]).all()


def test_grad_accumulate_refuses_mismatched_misalignment():
    dev = _dev()
    g, acc = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    lib = L.load()
    for og, oa in ((0, 1), (1, 0), (2, 3), (3, 1)):
        rc = lib.dc_grad_accumulate(8, L.dptr(g[og:]), L.dptr(acc[oa:]), 0, L.stream_ptr())
        assert rc != 0 and "same offset" in L.last_error()
    assert lib.dc_grad_accumulate(-1, L.dptr(g), L.dptr(acc), 0, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert float(acc.sum()) == 64.0


# ------------------------------------------------------------------------------------------ 2. equals hand-summed gradients, and 4.
def _twin_gradients(dtype, K, x, y):
    """K single-micro-batch backward passes of a second, identically seeded net (the step's own forward / loss / backward launches, no
    optimizer in between); returns the net, its step and the K gradient arenas."""
    net = _net(dtype)
    opt = dnn.make_optimizer("Adam", net, 1e-3, 1e-8, 1e-2)
    ts = dnn.TrainStep(net, opt, CW, B, H, W)
    gs = []
    for v in range(K):
        L.call("dc_memset_async", L.dptr(ts._acc), 0, 8, L.stream_ptr())
        ts._micro_batch(x[v * B:(v + 1) * B], y[v * B:(v + 1) * B], None, ts.loss_sum, None)
        torch.cuda.synchronize()
        gs.append(net.engine.grads.clone())
    return net, gs


@pytest.mark.parametrize("optname", ["Adam", "LAMB"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_step_equals_hand_summed_gradients(dtype, K, optname):
    x, y = _batches(K)
    net = _net(dtype)
    opt = dnn.make_optimizer(optname, net, 1e-3, 1e-8, 1e-2)
    step = dnn.TrainStep(net, opt, CW, B, H, W, with_metrics=True, virtual_ranks=K)
    assert opt.grad_scale == 1.0 / K
    step(x, y)
    torch.cuda.synchronize()

    twin, gs = _twin_gradients(dtype, K, x, y)
    total = gs[0].clone()
    for g in gs[1:]:
        total = total + g                                   # ((g0 + g1) + g2): ascending virtual rank
    assert torch.equal(net.engine.grad_acc, total)
    topt = dnn.make_optimizer(optname, twin, 1e-3, 1e-8, 1e-2)
    twin.engine.grads.copy_(total)
    topt.grad_scale = 1.0 / K
    topt.step()
    torch.cuda.synchronize()
    assert torch.equal(net.engine.params, twin.engine.params)
    # the logged loss is the mean of the ranks' own mean losses
    ls = step.rank_losses()
    assert len(ls) == K and step.loss() == pytest.approx(sum(ls) / K, rel=1e-15) and all(0 < l < 20 for l in ls)
    assert 0.0 <= step.iou() <= 1.0


def test_running_buffers_are_virtual_rank_zeros():
    K = 3
    x, y = _batches(K)
    net = _net(torch.float32)
    step = dnn.TrainStep(net, dnn.make_optimizer("Adam", net, 1e-3, 1e-8, 1e-2), CW, B, H, W, virtual_ranks=K)
    step(x, y)
    twin = _net(torch.float32)
    before = twin.engine.buffers.clone()
    ts = dnn.TrainStep(twin, dnn.make_optimizer("Adam", twin, 1e-3, 1e-8, 1e-2), CW, B, H, W)
    ts._micro_batch(x[:B], y[:B], None, ts.loss_sum, None)
    torch.cuda.synchronize()
    assert not torch.equal(before, twin.engine.buffers)
    assert torch.equal(net.engine.buffers, twin.engine.buffers) and torch.equal(net.engine.nbt, twin.engine.nbt)
    assert int(net.engine.nbt.min()) == 1 and int(net.engine.nbt.max()) == 1


# --------------------------------------------------------------------------------------------------- 3. equals a real two-rank run
def _torchrun(args, port, nproc=2, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + args
    return subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, DC_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=timeout)


def test_two_virtual_ranks_equal_two_real_ranks(tmp_path):
    """K = 2 in one process against the two-rank gloo fused step on one GPU, three LAMB steps: weights bit-equal (a + b is commutative in
    fp32), buffers rank 0's, logged loss the mean of the two ranks' losses."""
    out = str(tmp_path / "two_ranks.pt")
    r = _torchrun([os.path.join(ROOT, "tests", "virtual_ranks_worker.py"), out, "fp32"], 29641)
    assert r.returncode == 0 and "VR_WORKER ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    ref = torch.load(out, map_location="cpu", weights_only=False)
    net = _net(torch.float32)
    opt = dnn.make_optimizer("LAMB", net, 1e-3, 1e-8, 1e-2)
    step = dnn.TrainStep(net, opt, CW, B, H, W, with_metrics=True, virtual_ranks=2)
    for s in range(3):
        step(*_batches(2, step=s))
        torch.cuda.synchronize()
        l0, l1 = ref["losses"][s]
        print(f"step {s}: virtual {step.rank_losses()} real {[l0, l1]}")
        assert step.loss() == pytest.approx((l0 + l1) / 2, rel=1e-12)      # (a double-precision atomic sum: 1e-16 jitter)
    assert torch.equal(net.engine.params.cpu(), ref["params"])
    assert torch.equal(net.engine.buffers.cpu(), ref["buffers"]) and torch.equal(net.engine.nbt.cpu(), ref["nbt"])


# ------------------------------------------------------------------------------------------------------- 5. against the reference
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_against_the_reference_accumulation_loop(golden_dir, dtype):
    """tests/golden/virtual_ranks_small.json: the reference net, zero_grad, 2 x (forward, fp_loss / 2, backward), step (Adam), running
    buffers back to micro-batch 0's.  Tolerances are test_model_gpu.py's for model_small.json at the same step index: loss 2e-5 / 2e-3 (fp32,
    steps 0 / 1; test_golden_small_three_adam_steps), running statistics rtol 1e-4, atol 1e-5 behind one forward
    (test_forward_backward_vs_oracle), bf16 loss 5e-3 at step 0 (test_golden_small_bf16_loss_within_north_star; no envelope exists for a
    later bf16 step of that fixture, so none is asserted).  Weights: both sides start from the same weights and an Adam update moves a
    weight by at most lr * |m^ / sqrt(v^)| <= 1.0013 * lr in steps 1 and 2 (Cauchy-Schwarz over the two terms of the moments), so two
    trajectories are at most 2 * 1.0013 * lr * (s + 1) apart after step s -- a bound on sign flips of near-zero gradients, not on drift."""
    g = json.load(open(os.path.join(golden_dir, "virtual_ranks_small.json")))
    f32 = dtype == torch.float32
    K = g["K"]
    x, y = make_inputs(K * g["B"], g["H"], g["W"])
    net = _net(dtype)
    opt = dnn.make_optimizer("Adam", net, 1e-3, 1e-8, 1e-6)
    step = dnn.TrainStep(net, opt, CW, g["B"], g["H"], g["W"], with_metrics=True, virtual_ranks=K)
    idx = torch.tensor(g["sample_index"], device=_dev())
    for s in range(2 if f32 else 1):
        step(x.to(_dev()), y.to(_dev()))
        torch.cuda.synchronize()
        ref = g["steps"][s]
        ltol = (2e-5, 2e-3)[s] if f32 else 5e-3
        got = step.rank_losses()
        print(f"step {s}: losses {got} vs reference {ref['losses']}")
        for a, b in zip(got, ref["losses"]):
            assert a == pytest.approx(b, rel=ltol), f"step {s}"
        w = net.engine.params[idx].cpu().numpy()
        dw = np.abs(w - np.array(ref["weight_samples"]))
        print(f"step {s}: max sampled weight difference {dw.max():.3e}, {int((dw > 1e-5).sum())} of {len(dw)} above 1e-5")
        assert dw.max() <= 2 * 1.0013 * 1e-3 * (s + 1) + 1e-6
        for name, b in ref["buffers"].items():
            assert int(net.engine.buffer_view(name + ".num_batches_tracked")) == b["num_batches_tracked"] == s + 1
            if s == 0 and f32:
                for leaf in ("running_mean", "running_var"):
                    np.testing.assert_allclose(net.engine.buffer_view(name + "." + leaf)[:4].cpu().numpy(), np.array(b[leaf]), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------- 6. recorded and captured step, and 7.
def _run_steps(mode, K=2):
    dev = _dev()
    batches = [_batches(K, step=s) for s in (1, 2, 3)]
    z = (torch.zeros(K * B, 16, H, W, device=dev), torch.zeros(K * B, H, W, dtype=torch.int64, device=dev))
    net = _net(torch.bfloat16)
    opt = dnn.make_optimizer("LAMB", net, 1e-3, 1e-8, 1e-2)
    step = dnn.TrainStep(net, opt, CW, B, H, W, with_metrics=True, virtual_ranks=K)
    # enable_graph is one more launch on the (zero) static buffers with the scalars of the step before, enable_program two real steps
    if mode == "graph":
        step(*z)
        step.enable_graph()
    elif mode == "eager-graph":
        step(*z)
        step.launch(*z)
    elif mode == "program":
        step.enable_program()
    else:
        step(*z)
        step(*z)
    out = []
    for x, y in batches:
        step(x, y)
        torch.cuda.synchronize()
        out.append((step.loss(), step.iou(), net.engine.params.clone(), net.engine.buffers.clone()))
    return out, step, batches


@pytest.mark.parametrize("mode", ["graph", "program"])
def test_recorded_and_captured_step_replay_the_eager_steps(mode):
    a, _, _ = _run_steps("eager-" + mode)
    b, step, batches = _run_steps(mode)
    for (la, ia, pa, ba), (lb, ib, pb, bb) in zip(a, b):
        assert abs(la - lb) <= 1e-12 * abs(la) and ia == ib
        assert torch.equal(pa, pb) and torch.equal(ba, bb)
    if mode == "program":
        names = step._program.names()
        assert names.count("dc_grad_accumulate") == 2 * len(step._reducer.buckets) and names.count("dc_memcpy_async") == 4
        assert names.count("dc_lamb_step") == 1
        with torch.cuda.stream(torch.cuda.Stream()):
            with pytest.raises(L.DeepcamHipError, match="recorded under another stream"):
                step(*batches[0])


def test_one_virtual_rank_is_the_plain_step():
    names = []
    for kw in ({}, {"virtual_ranks": 1}):
        net = _net(torch.bfloat16)
        step = dnn.TrainStep(net, dnn.make_optimizer("LAMB", net, 1e-3, 1e-8, 1e-2), CW, B, H, W, with_metrics=True, **kw)
        step.enable_program()
        names.append(step._program.names())
        assert net.engine.grad_acc is None and net.engine.on_grad_ready is None
    assert names[0] == names[1] and "dc_grad_accumulate" not in names[0] and "dc_memcpy_async" not in names[0]


# ------------------------------------------------------------------------------------------------------------------------ 8. driver
def _train_losses(stdout):
    ev = [json.loads(l[len(":::MLLOG "):]) for l in stdout.splitlines() if l.startswith(":::MLLOG ")]
    return ([e["value"] for e in ev if e["key"] == "train_loss"], [e["value"] for e in ev if e["key"] == "global_batch_size"])


def test_driver_with_two_virtual_ranks_logs_the_two_rank_losses(tmp_path):
    common = ["--synthetic_samples", "16", "--local_batch_size", "2", "--height", "64", "--width", "96", "--logging_frequency", "1",
              "--validation_frequency", "100", "--save_frequency", "0", "--optimizer", "LAMB", "--weight_decay", "1e-2", "--amp_opt_level", "O1",
              "--max_epochs", "1", "--max_steps", "2", "--training_visualization_frequency", "0", "--validation_visualization_frequency", "0"]
    one = subprocess.run([sys.executable, "-m", "mlperf_deepcam_amd.train", "--wireup_method", "single", "--run_tag", "k2",
                          "--output_dir", str(tmp_path / "k2"), "--virtual_ranks", "2"] + common, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-3000:]
    two = _torchrun(["-m", "mlperf_deepcam_amd.train", "--wireup_method", "env", "--run_tag", "w2", "--output_dir", str(tmp_path / "w2")]
                    + common, 29642)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    l1, g1 = _train_losses(one.stdout)
    l2, g2 = _train_losses(two.stdout)
    print("virtual", l1, "two ranks", l2)
    assert g1 == [4] and g2 == [4]
    assert len(l1) == 2 and l1 == l2
