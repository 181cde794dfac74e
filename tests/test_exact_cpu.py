"""The exact-data kernel tests (test_exact_gpu.py, test_exact_ends_gpu.py) before any kernel is involved:

  - the preconditions of util_exact.py hold for every case the GPU files launch, so a failure there is the kernel's; the extents of the
    stem and the head reach the plans, blocks and caps they are there for;
  - the exact comparison rejects the mistakes hand-written tile kernels make (lost pixels in the statistics or the weight gradient, a lost
    8-channel vector of one tap, a pixel taken from its neighbour), and the statistics check of test_conv_fwd_dgrad_wgrad (rtol = 2e-3 on
    Gaussian data) accepts the first of them at the benchmark's pixel count: the gap the exact tests close;
  - the float64 reference equals an independent int64 evaluation (unfold + integer matmul)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_exact as U

CASES = U.gpu_cases()
CONV_FAMILIES = [f for f in CASES if f not in ("dw", "dwpipe", "sepconv")]
CONV_PARAMS = [pytest.param(f, n, s, e, id=f"{f}-{n}") for f in CONV_FAMILIES for n, s, e in CASES[f]]
DW_PARAMS = [pytest.param(n, s, id=f"{f}-{n}") for f in ("dw", "dwpipe") for n, s, _ in CASES[f]]


@pytest.mark.parametrize("family,name,spec,extra", CONV_PARAMS)
def test_preconditions_hold_for_every_convolution_case(family, name, spec, extra):
    """Every layer of every case, with the seeds the GPU file uses; the margins are wide (the bounds are printed with -s)."""
    for seeds in [U.layer_seeds(l) for l in range(extra["layers"])] if "layers" in extra else [extra.get("seeds", (1, 2, 3, 5))]:
        c = U.conv_case(spec, seeds)
        b = U.preconditions(c, f"{family}-{name}")
        print(family, name, b)
        assert b["y"] <= 64 and b["gx"] <= 64 and b["gw"] <= 2 ** 16 and b["sum_yy"] < 2 ** 23
        assert b["nonzero_y"] > 0.5          # the data exercise the kernel: most outputs are non-zero


@pytest.mark.parametrize("name,spec", DW_PARAMS)
def test_preconditions_hold_for_every_depthwise_case(name, spec):
    b = U.preconditions(U.dw_case(spec), name)
    assert b["y"] <= 9 and b["gx"] <= 10 and b["a0_y"] <= 45 and b["a1_y"] <= 45


@pytest.mark.parametrize("name,spec", [pytest.param(n, s, id=n) for n, s, _ in CASES["sepconv"]])
def test_preconditions_hold_for_the_separable_convolution(name, spec):
    """dc_sepconv_fwd's cases have 65 536 pixels and more; with the thinner pointwise weights and the smaller prologue of sep_case the
    sums of squares stay below 2^24 with a margin of two."""
    b = U.sep_preconditions(U.sep_case(spec), name)
    print(name, b)
    assert b["sum_yy"] < 2 ** 23 and b["y"] <= 64 and b["nonzero_y"] > 0.5


def test_preconditions_hold_at_the_ends_of_the_network():
    U.preconditions(U.stem_case(), "stem")
    b = U.head_preconditions(U.head_case())
    assert b["y"] <= U.HEAD_LOGIT_BOUND and b["gx"] <= 27
    N, Cc, H, W = U.POOL
    x = U.ints((N, Cc, H, W), 1, -4, 4).double()
    U.need_exact(x.sum((2, 3)), torch.float32, "sum_hw", bound=4 * H * W)
    U.need_exact(x.mean((2, 3)), torch.float32, "avgpool")            # 1 / 128: exact
    U.need_exact(x.sum((0, 2, 3)), torch.float32, "colsum", bound=4 * N * H * W)
    U.need_exact(x + 128 * U.ints((N, Cc, 1, 1), 2).double() / (H * W), torch.bfloat16, "avgpool_bwd_add")


@pytest.mark.parametrize("name,shape,budget", [pytest.param(*c, id=c[0]) for c in U.STEM_ENDS])
def test_preconditions_hold_for_the_stem_extents(name, shape, budget):
    """test_exact_ends_gpu.py's stem cases: exact, and the data reach what the case is there for: most outputs non-zero, and where a side
    is odd the ky = 2 / kx = 2 taps of the last output row / column lie on padding while the row / column in front of it is data."""
    N, Cin, H, W = shape
    c = U.stem_case(shape, budget)
    b = U.stem_preconditions(c, name)
    print(name, b)
    assert b["gx"] <= 128 and b["nonzero_y"] > 0.5
    Ho, Wo, P = U.stem_out(shape)
    assert tuple(c.y.shape) == (N, 32, Ho, Wo)
    if H % 2:
        assert 2 * (Ho - 1) - 1 + 2 == H and bool(c.x[:, :, H - 1].abs().sum() > 0)
    if W % 2:
        assert 2 * (Wo - 1) - 1 + 2 == W and bool(c.x[:, :, :, W - 1].abs().sum() > 0)
    assert bool((c.gw.abs().sum((0, 2, 3)) > 0).all()) and bool((c.gx.abs().sum((0, 2, 3)) > 0).all())     # every input channel takes part


def test_stem_extents_reach_every_weight_gradient_plan():
    """stem_wgrad_plan mirrors stem_ppb (the GPU test compares it with dc_stem_wgrad_workspace): among the extents there are one workspace
    row, several rows with a ragged last one, full rows only, a last batch below 64 pixels, and two batches per row."""
    plans = {name: U.stem_wgrad_plan(U.stem_out(shape)[2]) for name, shape, _ in U.STEM_ENDS}
    assert plans["one_row_1x7"] == (64, 1, 4) and plans["two_columns_9x2"] == (64, 1, 15)
    assert plans["odd_31x33"] == (64, 5, 16) and plans["p240"] == (64, 4, 48) and plans["w259"] == (64, 7, 6) and plans["w258"] == (64, 7, 3)
    assert plans["p512"] == (64, 8, 64)
    assert plans["ppb128_513x513"] == (128, 517, 1)
    blocks = {name: (U.stem_out(shape)[2] + 255) // 256 for name, shape, _ in U.STEM_ENDS}       # dc_stem_stat_rows
    assert blocks["odd_31x33"] == 2 and blocks["p512"] == 2 and blocks["p240"] == 1 and blocks["ppb128_513x513"] == 259
    cins = sorted({shape[1] for _, shape, _ in U.STEM_ENDS})
    assert cins == [1, 3, 5, 8, 10, 12, 16]
    assert {(c + 3) // 4 * 4 for c in cins} == {4, 8, 12, 16}          # every CP instantiation of the data gradient, padded and not


@pytest.mark.parametrize("name,shape", [pytest.param(*c, id=c[0]) for c in U.HEAD_ENDS])
def test_preconditions_hold_for_the_head_extents(name, shape):
    """test_exact_ends_gpu.py's head cases: the plain head and the head on an unstored BatchNorm output are exact, the riders' sums too;
    the integer logits tie (the first-index tie-break is exercised) and every class is predicted."""
    N, Cin, H, W = shape
    e = U.head_ends_case(shape)
    b = U.head_ends_preconditions(e, name)
    assert b["y"] <= U.HEAD_LOGIT_BOUND and b["gx"] <= 27
    P = N * H * W
    assert (P >= 256) == (name != "p255")
    for s in [e.score] + [p.score for p in e.bn]:
        assert len(torch.unique(s.pred)) == 3
        assert int(s.counts.sum(0)[:6].sum()) == 4 * P and torch.equal(s.classes.sum(1), torch.full((N,), 4 * H * W))
    top = e.c.y.sort(1).values
    assert int((top[:, 2] == top[:, 1]).sum()) > 0                        # ties for the maximum
    for relu in (0, 1):
        s0, s1 = U.bn_bwd_sums(e.c.gx, e.rin, relu, name)
        assert bool(s1.abs().max() > 0)


def test_head_matrix_reference_equals_autograd():
    """head_matrix_case (how the reference of HEAD_BIG is built: unfold, one matrix product per pixel, float32) against float64
    conv_transpose2d + autograd on the same data, at a small extent with ragged everything."""
    shape = (2, 256, 5, 7)
    N, Cin, H, W = shape
    m = U.head_matrix_case(shape)
    nchw = lambda t: t.reshape(N, H, W, Cin).permute(0, 3, 1, 2).double()  # noqa: E731
    a, w, gl = nchw(m.a).requires_grad_(True), m.w.double().requires_grad_(True), m.gl.double()
    gx, gw = torch.autograd.grad(F.conv_transpose2d(a, w, None, 2, 1, 1), (a, w), gl)
    assert torch.equal(nchw(m.dx), gx) and torch.equal(m.gw.double(), gw)
    r = types.SimpleNamespace(y=nchw(m.y), mean=m.mean.double(), invstd=m.invstd.double(), mscale=m.scale.double(), mshift=m.shift.double())
    s0, s1 = U.bn_bwd_sums(gx, r, 1, "matrix")
    assert torch.equal(m.s0, s0) and torch.equal(m.s1, s1)


def test_head_big_case_binds_both_grid_caps():
    """Shape arithmetic only (the reference itself is built in the GPU test, and checked there by head_matrix_case's own conditions)."""
    N, Cin, H, W = U.HEAD_BIG
    chunks = (N * H * W + 127) // 128
    assert chunks > 2048 and chunks // 2 > 512 and N * H * W * 4 * 3 < 2 ** 31


def test_preconditions_hold_for_the_batchnorm_backward_riders():
    """The sums the data-gradient epilogues take (sum g, sum g * xhat) are exact too: BNSTAT_CASES and every depthwise case."""
    for name, spec, _ in CASES["bnstat"]:
        c = U.conv_case(spec)
        for relu in (0, 1):
            s0, s1 = U.bn_bwd_sums(c.gx, U.bn_rider(tuple(c.x.shape)), relu, name)
            assert U.f32_holds(s0) and U.f32_holds(s1) and bool(s1.abs().max() > 0)
    for name, spec, _ in CASES["dw"] + CASES["dwpipe"]:
        c = U.dw_case(spec)
        r = U.dw_rider(c)
        for g in (c.gx, c.gx + c.add):
            for relu in (0, 1):
                U.bn_bwd_sums(g, r, relu, name)
        if spec[1] == 1 and spec[2] == 1:       # the residual form: mask from the stored input
            xo, gw = U.res_input(c)
            assert 0.2 < float((xo > 0).double().mean()) < 0.8
            for g in (c.gx, c.gx + c.add):
                U.bn_bwd_sums(g, r, 1, name, mask=xo > 0)
    N, Cin, H, W = U.HEAD
    for relu in (0, 1):
        U.bn_bwd_sums(U.head_case().gx, U.bn_rider((N, Cin, H, W)), relu, "head")


def test_preconditions_reject_data_that_are_not_exact():
    """Dense +-1 weights on a 728-channel layer: sums of 728 terms, too large for a bf16 store and for fp32 sums of squares."""
    c = U.conv_case((1, 1, 0, 1, 0, 728, 728, 2, 12, 10), budget=10 ** 9)
    with pytest.raises(U.NotExact):
        U.preconditions(c, "dense weights")
    c = U.conv_case((1, 1, 0, 1, 0, 64, 128, 2, 16, 12))
    U.preconditions(c)
    half = types.SimpleNamespace(**{**vars(c), "x": c.x + 1 / 512})
    with pytest.raises(U.NotExact):
        U.preconditions(half, "x is not a bf16 number")


# ------------------------------------------------------------------------------------------------------------------ teeth
def _nhw(t):
    """NCHW -> [pixel][channel], pixels in the order the kernels walk them (n, h, w)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _rejected(got, ref):
    """The exact comparison of the GPU file, at both compared types."""
    return all(U.first_difference(got.to(dt), ref.to(dt)) is not None for dt in (torch.float32, torch.bfloat16))


TEETH = {"ragged969": dict((n, s) for n, s, _ in CASES["pw384"])["ragged969"], "dense3x3": dict((n, s) for n, s, _ in CASES["conv"])["dense3x3"]}


@pytest.mark.parametrize("name", list(TEETH))
def test_exact_comparison_rejects_kernel_like_mistakes(name):
    spec = TEETH[name]
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    c = U.conv_case(spec)
    U.preconditions(c, name)
    # 1. statistics without the last 8 pixels (a ragged last tile dropped)
    short = _nhw(c.y)[:-8]
    assert not torch.equal(short.sum(0), c.sum_y) and not torch.equal((short * short).sum(0), c.sum_yy)
    assert _rejected((short * short).sum(0), c.sum_yy) and _rejected(short.sum(0), c.sum_y)
    # 2. a weight gradient without the last 8 pixels of dy
    cut = _nhw(c.gy).clone()
    cut[-8:] = 0
    gy_cut = cut.reshape(N, c.gy.shape[2], c.gy.shape[3], cout).permute(0, 3, 1, 2).contiguous()
    wr = c.w.clone().requires_grad_(True)
    (gw_cut,) = torch.autograd.grad(U.conv_ref(c.x, wr, None, k, stride, pad, dil, tr), wr, gy_cut)
    assert _rejected(gw_cut, c.gw)
    # 3. one 8-channel vector of one tap dropped at one border column (the centre tap, input channels 16 .. 23, the last column)
    t = k // 2
    y_drop = c.y.clone()
    y_drop[:, :, :, W - 1] -= torch.einsum("oc,nch->noh", c.w[:, 16:24, t, t], c.x[:, 16:24, :, W - 1])
    assert _rejected(y_drop, c.y)
    # 4. one output pixel taken from its neighbour
    y_shift = c.y.clone()
    y_shift[N - 1, :, H - 1, W - 1] = c.y[N - 1, :, H - 1, W - 2]
    assert _rejected(y_shift, c.y)
    # ... and the comparison accepts the reference itself
    assert not _rejected(c.y.clone(), c.y)


def test_present_statistics_check_accepts_lost_pixels_on_gaussian_data():
    """The gap, written down.  The slab check of test_conv_fwd_dgrad_wgrad compares the kernel's per-channel sums with those of the stored
    output at rtol = 2e-3 (sum of squares) and atol = 2e-3 * max sum |y| (sum).  At the pixel count of the benchmarked middle-flow layer
    (full_pw728_b8 of FULL_CASES: 728 -> 728 over 8 x 48 x 72 = 27 648 pixels, Gaussian data as that test builds them) statistics that lose
    the last 8 pixels pass it: they move the sum of squares by less than 1e-3 relative.  The same mistake on exact data is an inequality
    (test_exact_comparison_rejects_kernel_like_mistakes).  64 of the 728 output channels are evaluated: the check is per channel.

    (ragged969 itself cannot show the gap: 8 of its 969 pixels are 0.8 % of every sum, which rtol = 2e-3 does reject.)"""
    cin, cout, M = 728, 64, 8 * 48 * 72
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, cin, generator=g).bfloat16().float()
    w = (torch.randn(cout, cin, generator=torch.Generator().manual_seed(2)) * cin ** -0.5).bfloat16().float()
    y = (x @ w.t()).bfloat16().float()
    full_s, full_q = y.sum(0), (y * y).sum(0)
    lost_s, lost_q = y[:-8].sum(0), (y[:-8] * y[:-8]).sum(0)
    assert not torch.equal(lost_q, full_q)
    rel = float(((lost_q - full_q) / full_q).abs().max())
    print(f"relative change of the sum of squares when 8 of {M} pixels are lost: {rel:.2e}")
    assert rel < 2e-3
    np.testing.assert_allclose(lost_s.numpy(), full_s.numpy(), rtol=2e-3, atol=2e-3 * float(y.abs().sum(0).max()))
    np.testing.assert_allclose(lost_q.numpy(), full_q.numpy(), rtol=2e-3)


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", ["atrous18", "stem_thin"])
def test_reference_equals_integer_evaluation(name):
    """F.conv2d + autograd in float64 against unfold + int64 matmul: output, statistics and weight gradient, integer for integer."""
    spec = dict((n, s) for n, s, _ in CASES["conv"])[name]
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    assert not tr
    c = U.conv_case(spec)
    cols = F.unfold(c.x, k, dil, pad, stride).round().long()                 # [N][cin * k * k][Ho * Wo]
    wi = c.w.reshape(cout, -1).round().long()
    y = torch.einsum("ok,nkp->nop", wi, cols).reshape(c.y.shape)
    assert torch.equal(y, c.y.long()) and torch.equal(y.double(), c.y)
    assert torch.equal(y.sum((0, 2, 3)), c.sum_y.long()) and torch.equal((y * y).sum((0, 2, 3)), c.sum_yy.long())
    gy = c.gy.reshape(N, cout, -1).round().long()
    gw = torch.einsum("nop,nkp->ok", gy, cols).reshape(c.gw.shape)
    assert torch.equal(gw.double(), c.gw)
    gcols = torch.einsum("ok,nop->nkp", wi, gy).double()
    gx = F.fold(gcols, (H, W), k, dil, pad, stride)                          # sums of integers: exact in float64
    assert torch.equal(gx, c.gx)
