"""Autograd beyond the train step: the gradient w.r.t. the input (dc_stem_dgrad, Engine.input_grad) and the backward of the model in eval
mode, where every BatchNorm is the affine map of its running statistics (dc_bn_bwd_frozen + dc_bn_bwd_finalize, the frozen-BatchNorm
engine).  Kernels against CPU fp64 autograd; the module surface against the CPU oracle (oracle/model.py) with autograd."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from oracle import loss_metric as olm  # noqa: E402  (checker only)
from oracle import model as omodel  # noqa: E402
from util_inputs import make_inputs  # noqa: E402

CW = olm.class_weights(-0.125)
DEV = torch.device("cuda", 0)
EPS = 1e-5


def _rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------ kernels
def _stem_case(B, cin, H, W, dtype, seed=7):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    lddy = 40                                                   # > 32 channels: a padded pixel stride (a multiple of both vectors)
    dybuf = torch.randn(B, Ho, Wo, lddy, generator=g).to(dtype)
    w = torch.randn(32, cin, 3, 3, generator=g) * 0.2
    dx = torch.full((B, cin, H, W), float("nan"), device=DEV)   # every element must be written
    dyd, wd = dybuf.to(DEV), w.to(DEV)
    L.call("dc_stem_dgrad", L.dtype_code(dtype), B, cin, H, W, L.dptr(dyd), lddy, L.dptr(wd), L.dptr(dx), L.stream_ptr())
    torch.cuda.synchronize()
    dy = dybuf[..., :32].double().permute(0, 3, 1, 2)           # the same (bf16-rounded) dy for the reference
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(x, w.double(), stride=2, padding=1), x, dy)
    return dx.cpu(), ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", [(1, 32, 48), (2, 64, 96)])
@pytest.mark.parametrize("cin", [16, 8, 5, 1])
def test_stem_dgrad_vs_autograd(cin, B, H, W, dtype):
    dx, ref = _stem_case(B, cin, H, W, dtype)
    assert torch.isfinite(dx).all()
    err = float((dx.double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, f"max error {err:.2e} of max |dx|"
    assert _rel_l2(dx, ref) <= 1e-5


def test_stem_dgrad_full_size_b1():
    dx, ref = _stem_case(1, 16, 768, 1152, torch.bfloat16, seed=11)
    assert torch.isfinite(dx).all()
    assert float((dx.double() - ref).abs().max() / ref.abs().max()) <= 1e-5


def _bn_frozen_case(dtype, M, C, relu, residual, seed=5):
    """dc_bn_bwd_frozen + dc_bn_bwd_finalize against autograd of F.batch_norm(training=False) [+ residual] [+ ReLU] in fp64."""
    g = torch.Generator().manual_seed(seed)
    ld = C + (16 if dtype == torch.bfloat16 else 8)
    dt = L.dtype_code(dtype)

    def act(scale=1.0):
        return (torch.randn(M, ld, generator=g) * scale).to(dtype)
    y, r, dout = act(2.0), act(), act()
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm = torch.randn(C, generator=g) * 0.5                      # running statistics away from their init
    rv = torch.rand(C, generator=g) * 3.0 + 0.2
    # the reference in fp64 on the very (rounded) values the kernel reads
    y64 = y[:, :C].double().requires_grad_(True)
    r64 = r[:, :C].double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(y64, rm.double(), rv.double(), g64, b64, training=False, eps=EPS)
    if residual:
        z = z + r64
    # a ReLU decision within rounding distance of zero is not a question of this kernel: no gradient arrives there
    do = dout[:, :C].double()
    if relu:
        do = torch.where(z.detach().abs() < 1e-2, torch.zeros_like(do), do)
        dout[:, :C] = do.to(dtype)
        do = dout[:, :C].double()
    o = F.relu(z) if relu else z
    refs = torch.autograd.grad(o, [y64, r64, g64, b64] if residual else [y64, g64, b64], do)
    ref_dy, ref_g = refs[0], (refs[1] if residual else None)
    ref_dgam, ref_dbet = refs[-2], refs[-1]

    dev = lambda t: t.to(DEV)                                   # noqa: E731
    yd, rd, dod = dev(y), dev(r), dev(dout)
    gam, bet, rmd, rvd = dev(gamma), dev(beta), dev(rm), dev(rv)
    scale, shift = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    L.call("dc_bn_eval_coeffs", C, L.dptr(gam), L.dptr(bet), L.dptr(rmd), L.dptr(rvd), EPS, L.dptr(scale), L.dptr(shift), L.stream_ptr())
    out = torch.zeros(M, ld, dtype=dtype, device=DEV)
    L.call("dc_bn_apply", dt, M, C, L.dptr(yd), ld, L.dptr(scale), L.dptr(shift), L.dptr(rd) if residual else None, ld, 1 if relu else 0,
           L.dptr(out), ld, L.stream_ptr())
    rows = L.load().dc_bn_stat_rows(M)
    slab = torch.empty(2 * rows * C, device=DEV)
    dx = torch.zeros(M, ld, dtype=dtype, device=DEV)
    gout = torch.zeros(M, ld, dtype=dtype, device=DEV) if residual else None
    dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    L.call("dc_bn_bwd_frozen", dt, M, C, L.dptr(dod), ld, L.dptr(yd), ld, L.dptr(out), ld, relu, L.dptr(gam), L.dptr(rmd), L.dptr(rvd), EPS,
           L.dptr(dx), ld, L.dptr(gout) if gout is not None else None, ld if gout is not None else 0, L.dptr(slab), L.dptr(scale),
           L.dptr(shift), L.stream_ptr())
    L.call("dc_bn_bwd_finalize", C, L.dptr(slab), rows, L.dptr(dgam), L.dptr(dbet), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)          # read, never written
    return (dx[:, :C].cpu(), ref_dy, None if gout is None else gout[:, :C].cpu(), ref_g, dgam.cpu(), ref_dgam, dbet.cpu(), ref_dbet)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,relu,residual", [(96, 0, False), (96, 2, False), (256, 1, True), (64, 1, False), (256, 0, True)])
def test_bn_bwd_frozen_vs_autograd(dtype, C, relu, residual):
    M = 5003                                                   # not a multiple of the 64-row slab blocks
    dx, ref_dx, g, ref_g, dgam, ref_dgam, dbet, ref_dbet = _bn_frozen_case(dtype, M, C, relu, residual)
    # dx = g * gamma * invstd: one fp32 product (then the activation dtype's rounding)
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    assert _rel_l2(dx, ref_dx) <= tol
    if residual:
        assert torch.equal(g.double(), ref_g)                    # the masked dout itself, exactly
    # fp32 partial sums of 64-row blocks, combined in fp64 by the finalize
    assert _rel_l2(dbet, ref_dbet) <= 1e-5
    assert _rel_l2(dgam, ref_dgam) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ module, train mode
def _oracle(x, y, sd, training):
    keys = omodel.param_keys(sd)
    for k in keys:
        sd[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    out = omodel.forward(sd, xr, training=training)
    olm.fp_loss(out, y, CW).backward()
    return keys, out.detach(), xr.grad


def _net(dtype, B, H, W):
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=dtype, seed=333)
    net.materialize(B, H, W)
    return net


def _backward(net, x, y, requires_grad):
    xd = x.to(DEV).requires_grad_(requires_grad)
    out = net(xd)
    dnn.fp_loss(out, y.to(DEV), CW).backward()
    torch.cuda.synchronize()
    return xd, out


def test_input_grad_train_mode_fp32():
    x, y = make_inputs(2, 64, 96)
    _, _, ref = _oracle(x, y, omodel.init_state(333), training=True)
    net = _net(torch.float32, 2, 64, 96)
    opt = dnn.make_optimizer("Adam", net, 1e-3, 1e-8, 0.0)
    xd, _ = _backward(net, x, y, True)
    assert xd.grad is not None and xd.grad.shape == x.shape and xd.grad.dtype == torch.float32
    g_with = net.engine.grads.clone()
    err = _rel_l2(xd.grad, ref)
    print(f"[fp32 train] input gradient vs oracle: rel L2 {err:.3e}")
    # the same ill-conditioned train-mode backward as the parameter gradients (tests/test_model_gpu.py: per tensor < 8e-2); measured 1.55e-2
    assert err < 3e-2
    # the input gradient is an extra launch after backward: parameter gradients are bit-identical without it
    opt.zero_grad()
    _backward(net, x, y, False)
    assert torch.equal(net.engine.grads, g_with)


def test_input_grad_train_mode_bf16():
    x, y = make_inputs(2, 64, 96)
    _, _, ref = _oracle(x, y, omodel.init_state(333), training=True)
    net = _net(torch.bfloat16, 2, 64, 96)
    xd, _ = _backward(net, x, y, True)
    gx = xd.grad.double().cpu().flatten()
    r = ref.double().flatten()
    cos = float(gx @ r / (gx.norm() * r.norm()))
    ratio = float(gx.norm() / r.norm())
    print(f"[bf16 train] input gradient vs oracle: cosine {cos:.4f}, norm ratio {ratio:.4f}")
    # bf16 activations through 77 train-mode BatchNorms at B=2 (tests/test_model_gpu.py: parameter gradients' cosine 0.18): a descent direction of
    # the right magnitude, no more.  Measured: cosine 0.1702, norm ratio 0.8308 (deterministic; the bounds sit just outside)
    assert cos > 0.15 and 0.78 < ratio < 0.90


# ------------------------------------------------------------------------------------------------------------------ module, eval mode
def _perturbed_state(seed=21):
    """The seed-333 state with running statistics moved away from their init (mean 0, var 1): means ~ N(0, 0.1^2), variances in [0.8, 1.25].
    (The untrained network's eval-mode logits reach 1e5 at this size; wider statistics make the fp32 oracle itself disagree with its fp64
    evaluation by up to 6e-3 per gradient tensor, these by 4e-4.)"""
    sd = omodel.init_state(333)
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.45 + 0.8)
    return sd


@pytest.mark.parametrize("B", [2, 1])
def test_eval_mode_backward_vs_oracle(B):
    x, y = make_inputs(B, 64, 96)
    sd = _perturbed_state()
    net = _net(torch.float32, B, 64, 96)
    net.load_state_dict(sd)
    keys, out_ref, xref = _oracle(x, y, sd, training=False)
    net.eval()
    with torch.no_grad():
        out_ng = net(x.to(DEV)).clone()
    buf0, nbt0 = net.engine.buffers.clone(), net.engine.nbt.clone()
    xd, out = _backward(net, x, y, True)
    assert out.grad_fn is not None
    # the logits of the eval forward with autograd on are those of the no_grad eval forward (tests/test_model_gpu.py's eval tolerance)
    np.testing.assert_allclose(out.detach().cpu().numpy(), out_ng.cpu().numpy(), rtol=2e-3, atol=2e-4)
    lerr = _rel_l2(out.detach(), out_ref)
    assert lerr < 1e-4, lerr             # (logits up to 1e5: element-wise, the near-zero ones are rounding noise of the large ones)
    # the running statistics are read, never updated
    assert torch.equal(net.engine.buffers, buf0) and torch.equal(net.engine.nbt, nbt0)
    worst, g1 = ("", 0.0), {}
    for k in keys:
        g1[k] = net.get_parameter(k).grad.clone()
        e = _rel_l2(g1[k], sd[k].grad)
        if e > worst[1]:
            worst = (k, e)
    allg = torch.cat([g1[k].cpu().flatten() for k in keys])
    allr = torch.cat([sd[k].grad.flatten() for k in keys])
    total = _rel_l2(allg, allr)
    xerr = _rel_l2(xd.grad, xref)
    print(f"[fp32 eval B={B}] logits {lerr:.3e}; worst per-tensor grad err {worst}; whole-arena {total:.3e}; input gradient {xerr:.3e}")
    # frozen BatchNorm is linear: far better conditioned than the train-mode backward (< 8e-2 / < 3e-2 there).  Measured, B=2: worst 1.85e-3
    # (block9.rep.2.bias), whole arena 4.66e-4, input 1.83e-3; B=1: 2.5e-6, 1.4e-6, 2.1e-6 (deterministic; the bounds sit just outside B=2's)
    assert worst[1] < 4e-3 and total < 1e-3 and xerr < 4e-3
    # a second backward without zero_grad adds up (torch semantics), for the parameters and for x.grad alike
    gx1 = xd.grad.clone()
    out = net(xd)
    dnn.fp_loss(out, y.to(DEV), CW).backward()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(net.get_parameter(k).grad, 2 * g1[k]), k
    assert torch.equal(xd.grad, 2 * gx1)
    assert torch.equal(net.engine.buffers, buf0) and torch.equal(net.engine.nbt, nbt0)


def test_eval_mode_without_autograd_stays_on_the_eval_engine():
    x, y = make_inputs(2, 32, 48)
    net = _net(torch.float32, 2, 32, 48)
    net.eval()
    with torch.no_grad():
        out = net(x.to(DEV))
    with torch.inference_mode():
        net(x.to(DEV))
    assert out.grad_fn is None and not net._frozen_engines
    for p in net.parameters():
        p.requires_grad_(False)
    assert net(x.to(DEV)).grad_fn is None and not net._frozen_engines      # nothing asks for a gradient
    for p in net.parameters():
        p.requires_grad_(True)
    assert net(x.to(DEV)).grad_fn is not None and len(net._frozen_engines) == 1


def test_eval_mode_backward_under_a_reducer_raises():
    x, y = make_inputs(2, 32, 48)
    net = _net(torch.float32, 2, 32, 48)
    net.eval()
    net._ddp_reducer = types.SimpleNamespace()      # what dist.DistributedDataParallel attaches (never reached: the backward refuses first)
    loss = dnn.fp_loss(net(x.to(DEV)), y.to(DEV), CW)
    with pytest.raises(NotImplementedError, match="eval mode"):
        loss.backward()
