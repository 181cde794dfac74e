"""The riders of the persistent depthwise data gradient (dwpipe.hip: BatchNorm sums, the recomputed forward input with this layer's weight
gradient, the addend, the residual BatchNorm's sums, the masked store) against the tiled path (dwtile.hip, option dw_pipe = 0) on the same
inputs: bf16, two images of 16 x 24 and 8 x 8 pixels on 64 (half a channel block), 128, 200 (a channel block with a tail) and 728 channels,
dilation 1 and 2 -- workgroups with a single tile and nothing but dummy requests behind it --, and 728 channels on 48 x 72 pixels, where a
workgroup walks three tiles (the ring wraps, the steady-state vmcnt counts are reached).

What the two paths share bit for bit (test_depthwise_pipelined_kernel_matches_tiled, test_depthwise_dgrad_takes_the_residual_batchnorm_sums)
is compared with torch.equal: dx.  The sums and the weight gradient are added in another order (a slab row per workgroup instead of one per
tile): they are compared after their finalize / fold with the tolerance of those tests, rtol 3e-5 and 3e-5 of the largest value."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from util_launch import served  # noqa: E402


def dev():
    return torch.device("cuda", 0)


def S():
    return L.stream_ptr()


def vptr(view):
    return C.c_void_p(view.data_ptr())


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def to_nhwc(t_nchw, ld=None):
    """NCHW fp32 on the host -> (buffer, view): a device NHWC view of width C inside an [N, H, W, ld] bf16 buffer poisoned with NaN."""
    n, c, h, w = t_nchw.shape
    buf = torch.full((n, h, w, ld or c), float("nan"), dtype=DTYPE, device=dev())
    buf[..., :c] = t_nchw.permute(0, 2, 3, 1).to(DTYPE).to(dev())
    return buf, buf[..., :c]


def empty_nhwc(n, h, w, c):
    return torch.full((n, h, w, c), float("nan"), dtype=DTYPE, device=dev())


DT, DTYPE, N = L.DC_BF16, torch.bfloat16, 2
CASES = [(Cc, dil, H, W) for Cc in (64, 128, 200, 728) for dil in (1, 2) for (H, W) in ((16, 24), (8, 8))] + [(728, 1, 48, 72), (728, 2, 48, 72)]
IDS = [f"c{Cc}_d{dil}_{H}x{W}" for Cc, dil, H, W in CASES]
RES_CASES = [c for c in CASES if c[1] == 1]             # the residual form is built for dilation 1
RES_IDS = [i for i, c in zip(IDS, CASES) if c[1] == 1]


def close(got, want):
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=3e-5, atol=3e-5 * float(want.abs().max()))


def finalize(Cc, slab, rows):
    dgam, dbet = torch.full((Cc,), float("nan"), device=dev()), torch.full((Cc,), float("nan"), device=dev())
    L.call("dc_bn_bwd_finalize", Cc, vptr(slab), rows, vptr(dgam), vptr(dbet), S())
    return dgam, dbet


def fold(Cc, wslab, rows):
    gw = torch.full((Cc, 1, 3, 3), float("nan"), device=dev())
    L.call("dc_dwconv_wgrad_reduce", Cc, rows, vptr(wslab), vptr(gw), S())
    return gw


@functools.lru_cache(maxsize=None)
def inputs(Cc, H, W):
    """Device tensors of a case, shared by every test and left unchanged (the addend is copied where a call writes over it)."""
    ld = (Cc + 31) // 32 * 32
    wm = rnd(Cc, 1, 3, 3, seed=2, scale=1 / 3).to(dev())
    wd = torch.empty(9 * Cc, device=dev())
    L.call("dc_dwconv_pack_weights", Cc, vptr(wm), vptr(wd), S())
    t = dict(ld=ld, wd=wd,
             x=to_nhwc(rnd(N, Cc, H, W, seed=1), ld=ld),       # BatchNorm input / stored layer input / stored block output
             ybn=to_nhwc(rnd(N, Cc, H, W, seed=7), ld=ld),     # input of the residual BatchNorm
             gy=to_nhwc(rnd(N, Cc, H, W, seed=3), ld=ld),
             add=to_nhwc(rnd(N, Cc, H, W, seed=4)),
             mean=rnd(Cc, seed=8, scale=0.2).to(dev()), invstd=(torch.rand(Cc, generator=torch.Generator().manual_seed(5)) + 0.5).to(dev()),
             sc=(torch.rand(Cc, generator=torch.Generator().manual_seed(6)) + 0.5).to(dev()), sh=rnd(Cc, seed=9, scale=0.3).to(dev()))
    torch.cuda.synchronize()
    return t


def run_stats_wgrad(Cc, dil, H, W, sum_row):
    t, lib = inputs(Cc, H, W), L.load()
    rows = lib.dc_dwconv_dgrad_bnstats_rows(DT, Cc, 1, dil, N, H, W)
    wrows = lib.dc_dwconv_dgrad_wgrad_rows(DT, Cc, 1, dil, N, H, W)
    assert rows > 0 and wrows > 0
    dx = empty_nhwc(N, H, W, Cc)
    wslab = torch.full((wrows, 9, Cc), float("nan"), device=dev())
    slab = torch.zeros(2 * Cc, dtype=torch.float64, device=dev()) if sum_row else torch.full((2, rows, Cc), float("nan"), device=dev())
    with served("dgrad + BatchNorm sums + weight gradient") as names:
        L.call("dc_dwconv_dgrad_bnstats_wgrad_sum" if sum_row else "dc_dwconv_dgrad_bnstats_wgrad", DT, Cc, 1, dil, N, H, W, vptr(t["gy"][1]), t["ld"],
               vptr(t["wd"]), vptr(dx), Cc, vptr(t["x"][1]), t["ld"], vptr(t["mean"]), vptr(t["invstd"]), vptr(t["sc"]), vptr(t["sh"]), 1,
               vptr(slab), vptr(wslab), S())
    dgam, dbet = finalize(Cc, slab, -1 if sum_row else rows)
    gw = fold(Cc, wslab, wrows)
    torch.cuda.synchronize()
    return dict(dx=dx, slab=slab, wslab=wslab, dgam=dgam, dbet=dbet, gw=gw, names=names)


def run_wgrad(Cc, dil, H, W, affine):
    t, lib = inputs(Cc, H, W), L.load()
    wrows = lib.dc_dwconv_dgrad_wgrad_rows(DT, Cc, 1, dil, N, H, W)
    assert wrows > 0
    dx = empty_nhwc(N, H, W, Cc)
    wslab = torch.full((wrows, 9, Cc), float("nan"), device=dev())
    with served("dgrad + addend + weight gradient") as names:
        L.call("dc_dwconv_dgrad_wgrad", DT, Cc, 1, dil, N, H, W, vptr(t["gy"][1]), t["ld"], vptr(t["wd"]), vptr(t["add"][1]), Cc, vptr(dx), Cc, vptr(t["x"][1]),
               t["ld"], vptr(t["sc"]) if affine else None, vptr(t["sh"]) if affine else None, affine, vptr(wslab), S())
    gw = fold(Cc, wslab, wrows)
    torch.cuda.synchronize()
    return dict(dx=dx, gw=gw, names=names)


@functools.lru_cache(maxsize=None)
def tiled(Cc, dil, H, W):
    """The reference of a case, once: every entry point on the tiled kernel, and the residual BatchNorm's sums by dc_bn_bwd_reduce."""
    L.call("dc_set_option", b"dw_pipe", 0)
    try:
        ref = dict(stats=run_stats_wgrad(Cc, dil, H, W, False), wg=[run_wgrad(Cc, dil, H, W, aff) for aff in (0, 1)])
    finally:
        L.call("dc_set_option", b"dw_pipe", 1)
    for r in (ref["stats"], *ref["wg"]):
        assert [n for n in r["names"] if n.startswith("dw")] == ["dw_tile_dgrad"], r["names"]
    t, M = inputs(Cc, H, W), N * H * W
    srows = L.load().dc_bn_stat_rows(M)
    slab = torch.empty((2, srows, Cc), device=dev())
    L.call("dc_bn_bwd_reduce", DT, M, Cc, vptr(ref["wg"][0]["dx"]), Cc, vptr(t["ybn"][1]), t["ld"], vptr(t["x"][1]), t["ld"], 1, vptr(t["mean"]),
           vptr(t["invstd"]), vptr(slab), None, None, S())
    ref["res"] = finalize(Cc, slab, srows)
    torch.cuda.synchronize()
    return ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_with_batchnorm_sums_and_weight_gradient(case):
    """dc_dwconv_dgrad_bnstats_wgrad and its sum-row form: dx bit for bit, the finalized sums and the folded weight gradient to the rounding of
    another summation order; the sum row is the fp64 column sum of the slab rows."""
    ref = tiled(*case)["stats"]
    got = run_stats_wgrad(*case, False)
    got_sum = run_stats_wgrad(*case, True)
    for g in (got, got_sum):
        assert [n for n in g["names"] if n.startswith("dw")] == ["dwpipe_dgrad"], g["names"]
        assert torch.equal(g["dx"], ref["dx"])
        close(g["dgam"], ref["dgam"])
        close(g["dbet"], ref["dbet"])
        close(g["gw"], ref["gw"])
    assert torch.equal(got_sum["wslab"], got["wslab"])
    assert torch.equal(got_sum["slab"], got["slab"].double().sum(1).reshape(-1))


@pytest.mark.parametrize("affine", [0, 1], ids=["stored_input", "affine_relu"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_with_addend_and_weight_gradient(case, affine):
    """dc_dwconv_dgrad_wgrad on a stored layer input and on one formed as relu(x * scale + shift): dx bit for bit, the folded weight gradient to
    the rounding of another summation order."""
    ref = tiled(*case)["wg"][affine]
    got = run_wgrad(*case, affine)
    assert [n for n in got["names"] if n.startswith("dw")] == ["dwpipe_dgrad"], got["names"]
    assert torch.equal(got["dx"], ref["dx"])
    close(got["gw"], ref["gw"])


@pytest.mark.parametrize("sum_row", [False, True], ids=["slab", "sum_row"])
@pytest.mark.parametrize("relu", [1, 2], ids=["relu1", "relu2_masked_store"])
@pytest.mark.parametrize("case", RES_CASES, ids=RES_IDS)
def test_dgrad_with_residual_batchnorm_sums(case, relu, sum_row):
    """dc_dwconv_dgrad_wgrad_bnres[_sum] = the tiled dc_dwconv_dgrad_wgrad (dx bit for bit; with relu = 2 stored masked by the block output's
    sign) + the sums dc_bn_bwd_reduce takes from that dx, the residual BatchNorm's input and the stored block output."""
    Cc, dil, H, W = case
    t, lib, ref = inputs(Cc, H, W), L.load(), tiled(*case)
    rows = lib.dc_dwconv_dgrad_wgrad_bnres_rows(DT, Cc, 1, dil, N, H, W)
    assert rows > 0 and rows == lib.dc_dwconv_dgrad_wgrad_rows(DT, Cc, 1, dil, N, H, W)
    assert lib.dc_dwconv_dgrad_wgrad_bnres_masked(DT, Cc, 1, dil, N, H, W) == 1
    dx = t["add"][1].clone()                              # dx starts as the other consumers' contribution: the addend aliases the output
    wslab = torch.full((rows, 9, Cc), float("nan"), device=dev())
    slab = torch.zeros(2 * Cc, dtype=torch.float64, device=dev()) if sum_row else torch.full((2, rows, Cc), float("nan"), device=dev())
    with served("dgrad + addend + weight gradient + residual BatchNorm sums") as names:
        L.call("dc_dwconv_dgrad_wgrad_bnres_sum" if sum_row else "dc_dwconv_dgrad_wgrad_bnres", DT, Cc, 1, dil, N, H, W, vptr(t["gy"][1]), t["ld"],
               vptr(t["wd"]), vptr(dx), Cc, vptr(dx), Cc, vptr(t["x"][1]), t["ld"], vptr(wslab), vptr(t["ybn"][1]), t["ld"], vptr(t["mean"]),
               vptr(t["invstd"]), relu, vptr(slab), S())
    dgam, dbet = finalize(Cc, slab, -1 if sum_row else rows)
    gw = fold(Cc, wslab, rows)
    torch.cuda.synchronize()
    assert [n for n in names if n.startswith("dw")] == ["dwpipe_dgrad_masked" if relu == 2 else "dwpipe_dgrad"], names
    want = ref["wg"][0]["dx"]
    if relu == 2:
        want = torch.where(t["x"][1] > 0, want, torch.zeros_like(want))
    assert torch.equal(dx, want)
    close(gw, ref["wg"][0]["gw"])
    close(dgam, ref["res"][0])
    close(dbet, ref["res"][1])
