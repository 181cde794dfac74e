"""The stem and the classifier head (stem_head.hip) on exactly representable data, at the extents where their kernels take another path.

The method is test_exact_gpu.py's: small-integer data (util_exact.py), so a correct kernel equals the float64 reference bit for bit in fp32
and in bf16; padded, NaN-poisoned views; a spare slab row and a spare tail behind every flat output that must stay NaN; launch records
(util_launch.served); option overrides restored in `finally`.  test_exact_gpu.py runs these two layers at one shape each (20 x 28 and
6 x 9, both sides even, less than one tile, chunk or block of anything); the multi-tile head tests of test_kernels_gpu.py compare project
kernels with each other.  Here every output meets float64 conv2d / conv_transpose2d and their autograd (util_exact.stem_case,
head_ends_case), and the preconditions of every case are proved without a GPU in test_exact_cpu.py.

Covered
  stem (STEM_ENDS: odd H, odd W, both; one and two full 256-pixel blocks, a partial one, a second block of 16 lanes; W = 258 / 259 with three
  pair chunks per row in the data gradient; one input row; two input columns; 513 x 513 where a weight-gradient workgroup takes two
  64-pixel batches; Cin = 1, 3, 5, 8, 10, 12 at an odd and an even extent), fp32 and bf16: dc_stem_fwd (output, float64 column sums of the
  slab, exactly dc_stem_stat_rows rows written, nothing outside the channel slice), dc_stem_wgrad (every workspace row of the plan
  written, none behind), dc_stem_dgrad.
  head, Cin = 256 (HEAD_ENDS: 2800 pixels = 22 chunks and 5 x 3 tiles; two strips of tiles; exactly one tile = 256 pixels, where the weight
  gradient starts to ride on the statistics pass, and 255, where it does not yet; three samples with nothing aligned), bf16 and, where
  the entry point takes it, fp32: dc_head_fwd (head_fused 1 / 0), dc_head_fwd_loss (with and without a logits buffer), dc_head_bwd,
  dc_head_bwd_bnstats (head_dgrad_fused 1 / 0, relu 1 / 0), dc_head_fwd_bnin, dc_head_fwd_loss_bnin, dc_head_bwd_bnin (parts 3 with a dx;
  1 then 2; 3 without a dx under head_wgrad_fused 1 / 0, and after the riding form parts 2 once more: the gathered gradient image it
  leaves in the workspace is what dc_head_bwd_bnin_apply reads), dc_head_fwd_score and dc_head_fwd_predict with n_valid 0, 1, N.
  Logits, predictions (first index on the many ties of integer logits), confusion and class counts, data and weight gradients and
  BatchNorm-backward sums are equalities.  The only tolerances are the project's own for softmax arithmetic: the loss sum (rel 1e-5) and the
  logit gradient (rtol 2e-4) of test_loss_gpu.py, the per-sample loss sum (rel 2e-6) of test_val_gpu.py, the confidence (CONF_ABS_TOL)
  of test_predict_gpu.py.
  HEAD_BIG (1 x 520 x 512, bf16): 2080 chunks on 2048 workgroups and 1040 candidate weight-gradient rows on 512, so both workgroup-stride
  loops of head_dgrad_kernel run: dc_head_bwd_bnstats and dc_head_bwd_bnin (parts 3, no dx) only, against a matrix-product reference.

Left out
  dc_head_bwd_bnin_apply: its coefficients carry 1 / count, exact only for power-of-two pixel counts; it stays pinned to dc_bn_bwd_apply by
  test_kernels_gpu.test_head_on_unstored_batchnorm_output.  The full 768 x 1152 extent."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from test_kernels_gpu import DTYPES, PLAIN_GEMM, S, dev, empty_nhwc, from_nhwc, to_nhwc, vptr  # noqa: E402
from test_exact_gpu import all_nan, cast, check_rider_slab, column_sums, rider_vectors  # noqa: E402
from test_predict_gpu import CONF_ABS_TOL  # noqa: E402
from util_launch import assert_served, served  # noqa: E402
import util_exact as U  # noqa: E402
from util_exact import exactly  # noqa: E402

NAN = float("nan")
BF16 = torch.bfloat16
# test_loss_gpu.test_loss_kernel_full_size_properties compares the logit gradient at rtol = 2e-4, atol = 1e-12 over n = 2 x 768 x 1152
# pixels.  Every gradient element carries the factor w / n, so the same absolute allowance on a probability is atol * FULL_N / n here
GRAD_RTOL, GRAD_ATOL, FULL_N = 2e-4, 1e-12, 2 * 768 * 1152
LOSS_REL = 1e-5             # test_loss_gpu.py: the loss against olm.fp_loss
SAMPLE_LOSS_REL = 2e-6      # test_val_gpu.test_wce_score_ties_kat: per-sample loss sums against the reference's loss


def flat(shape, dtype=torch.float32, fill=NAN, spare=8):
    """A contiguous output of `shape` with `spare` more elements behind it: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + spare,), fill, dtype=dtype, device=dev())
    return buf, buf[:n].view(shape)


def untouched(buf, spare=8):
    return all_nan(buf[-spare:])


def head_workspace(dt, shape):
    N, Cin, H, W = shape
    ws = torch.empty(L.load().dc_head_workspace(dt, N, Cin, H, W) + 256, dtype=torch.uint8, device=dev())
    return ws, C.c_void_p((ws.data_ptr() + 255) // 256 * 256)


def rider_slab(rows, Cin):
    """[2][rows][Cin] and one spare row behind it."""
    buf = torch.full((2 * rows + 1, Cin), NAN, device=dev())
    return buf, buf[:2 * rows].view(2, rows, Cin)


# ------------------------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape,budget", [pytest.param(*c, id=c[0]) for c in U.STEM_ENDS])
def test_stem(name, shape, budget, dtype):
    """dc_stem_fwd with its slab, dc_stem_wgrad and dc_stem_dgrad (NCHW fp32 input and input gradient) against float64 conv2d(stride 2,
    pad 1) and its autograd."""
    N, Cin, H, W = shape
    c = U.stem_case(shape, budget)
    U.stem_preconditions(c, name)
    dt, lib = L.dtype_code(dtype), L.load()
    Ho, Wo, P = U.stem_out(shape)
    assert (Ho, Wo) == tuple(c.y.shape[2:])
    xd, wd = c.x.float().to(dev()), c.w.float().to(dev())
    ybuf, yv = empty_nhwc(N, Ho, Wo, 32, dtype, ld=56, off=16)
    rows = lib.dc_stem_stat_rows(N, H, W)
    assert rows == (P + 255) // 256
    slab = torch.full((3, rows, 32), NAN, device=dev())                    # [2]: a neighbour's rows
    L.call("dc_stem_fwd", dt, N, Cin, H, W, vptr(xd), vptr(wd), vptr(yv), 56, vptr(slab), S())
    torch.cuda.synchronize()
    exactly(from_nhwc(yv), cast(c.y, dtype), f"{name} fwd")
    assert all_nan(ybuf[..., :16]) and all_nan(ybuf[..., 48:]), f"{name} fwd: wrote outside its channel slice"
    assert all_nan(slab[2]), f"{name} fwd: wrote behind its {rows} slab rows"
    s, ss = column_sums(slab[:2])                                          # (asserts that every one of the rows was written)
    exactly(s, c.sum_y, f"{name}: sum of y")
    exactly(ss, c.sum_yy, f"{name}: sum of y^2")
    # the weight gradient: workspace rows as stem_wgrad_plan says, every one written, none behind
    _, wrows, _ = U.stem_wgrad_plan(P)
    row = 32 * Cin * 9
    wsb = lib.dc_stem_wgrad_workspace(N, Cin, H, W)
    assert wsb == wrows * row * 4
    ws = torch.full((wrows + 1, row), NAN, device=dev())
    _, gyv = to_nhwc(c.gy, dtype, ld=40, off=8)
    gwbuf, gw = flat((32, Cin, 3, 3))
    L.call("dc_stem_wgrad", dt, N, Cin, H, W, vptr(xd), vptr(gyv), 40, vptr(ws), vptr(gw), S())
    dxbuf, dx = flat((N, Cin, H, W))
    L.call("dc_stem_dgrad", dt, N, Cin, H, W, vptr(gyv), 40, vptr(wd), vptr(dx), S())
    torch.cuda.synchronize()
    exactly(gw.cpu(), c.gw.float(), f"{name} wgrad")
    assert untouched(gwbuf) and all_nan(ws[wrows]) and not bool(torch.isnan(ws[:wrows]).any()), f"{name} wgrad: workspace rows / the tail of gw"
    exactly(dx.cpu(), c.gx.float(), f"{name} dgrad")
    assert untouched(dxbuf), f"{name} dgrad: wrote behind dx"


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_PARAMS = [pytest.param(*c, id=c[0]) for c in U.HEAD_ENDS]


def head_operands(name, shape, dtype):
    e = U.head_ends_case(shape)
    U.head_ends_preconditions(e, name)
    Cin = shape[1]
    _, xv = to_nhwc(e.c.x, dtype, ld=Cin + 8)
    ws, wsp = head_workspace(L.dtype_code(dtype), shape)
    return e, xv, e.c.w.float().to(dev()), ws, wsp


def loss_operands(e):
    return e.labels.to(dev()), torch.tensor(e.score.cw, dtype=torch.float32, device=dev()), e.labels.numel()


def check_loss(s, ref_logits, lbuf, logits, store, ls, dlbuf, dl, pred, cnt, n, what):
    """The outputs of a loss call against util_exact.head_score of the float64 logits."""
    if store:
        exactly(logits.cpu(), ref_logits.float(), f"{what}: logits")
    else:
        assert all_nan(logits), f"{what}: logits written without a buffer"
    assert untouched(lbuf) and untouched(dlbuf), f"{what}: wrote behind the logits or their gradient"
    exactly(pred.cpu(), s.pred, f"{what}: predicted class (first maximum)")
    exactly(cnt.cpu(), s.counts.sum(0), f"{what}: tp / fp / fn counts")
    print(f"{what}: loss {float(ls) / n!r}, reference {s.mean_loss!r}")
    assert float(ls) / n == pytest.approx(s.mean_loss, rel=LOSS_REL), f"{what}: loss"
    np.testing.assert_allclose(dl.cpu().numpy(), s.grad.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL * FULL_N / n, err_msg=f"{what}: logit gradient")


def run_loss(fn, head_args, tail_of, s, ref_logits, shape, labels, cw, n, store, what):
    N, _, H, W = shape
    lbuf, logits = flat((N, 3, 2 * H, 2 * W))
    dlbuf, dl = flat((N, 3, 2 * H, 2 * W))
    ls = torch.zeros(1, dtype=torch.float64, device=dev())
    pred = torch.full((N, 2 * H, 2 * W), -1, dtype=torch.int64, device=dev())
    cnt = torch.zeros(9, dtype=torch.int64, device=dev())
    L.call(fn, *head_args, vptr(logits) if store else None, tail_of, vptr(labels), 8, vptr(cw), 1.0 / n, vptr(ls), vptr(dl), vptr(pred), vptr(cnt), S())
    torch.cuda.synchronize()
    check_loss(s, ref_logits, lbuf, logits, store, ls, dlbuf, dl, pred, cnt, n, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape", HEAD_PARAMS)
def test_head_forward(name, shape, dtype):
    """dc_head_fwd on the fused kernel and on GEMM + combine (fp32: the latter under both settings), and dc_head_fwd_loss with and without
    a logits buffer (without: the fused kernel only): logits, predictions and counts equal; loss and logit gradient at the project's
    tolerances."""
    N, Cin, H, W = shape
    e, xv, wd, ws, wsp = head_operands(name, shape, dtype)
    dt, c = L.dtype_code(dtype), e.c
    labels, cw, n = loss_operands(e)
    head_args = (dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(wd))
    try:
        for fused in (1, 0):
            L.call("dc_set_option", b"head_fused", fused)
            what = f"{name} head_fused={fused}"
            buf, out = flat((N, 3, 2 * H, 2 * W))
            with served(what) as names:
                L.call("dc_head_fwd", *head_args, vptr(out), wsp, S())
            if dtype == BF16:
                assert_served(names, ["head_fwd_fused"] if fused else ["igemm128_f32out", "head_combine"], what, ignore=("aux",))
            else:
                assert names[-1] == "head_combine" and "head_fwd_fused" not in names, names
            torch.cuda.synchronize()
            exactly(out.cpu(), c.y.float(), f"{what}: logits")
            assert untouched(buf), f"{what}: wrote behind the logits"
            for store in (True, False) if (dtype == BF16 and fused) else (True,):
                run_loss("dc_head_fwd_loss", head_args, wsp, e.score, c.y, shape, labels, cw, n, store, f"{what} dc_head_fwd_loss store={store}")
    finally:
        L.call("dc_set_option", b"head_fused", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape", HEAD_PARAMS)
def test_head_backward(name, shape, dtype):
    """dc_head_bwd, and dc_head_bwd_bnstats on independent BatchNorm data (bn_rider) with relu 1 / 0, on the streaming and on the tiled
    data-gradient kernel in bf16: dx in the storage type, the fp32 weight gradient and the slab's float64 sums equal the reference."""
    N, Cin, H, W = shape
    e, xv, wd, ws, wsp = head_operands(name, shape, dtype)
    dt, c, P = L.dtype_code(dtype), e.c, N * H * W
    gld = c.gy.float().to(dev())
    dbuf, gxv = empty_nhwc(N, H, W, Cin, dtype, ld=Cin + 8)
    gwbuf, gw = flat((Cin, 3, 3, 3))
    L.call("dc_head_bwd", dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(gld), vptr(wd), vptr(gxv), Cin + 8, vptr(gw), wsp, S())
    torch.cuda.synchronize()
    exactly(from_nhwc(gxv), cast(c.gx, dtype), f"{name} dc_head_bwd: dx")
    exactly(gw.cpu(), c.gw.float(), f"{name} dc_head_bwd: weight gradient")
    assert all_nan(dbuf[..., Cin:]) and untouched(gwbuf)
    r = e.rider
    _, ybv = to_nhwc(r.y, dtype, ld=Cin + 16, off=8)
    mean, invstd, ms, mh = rider_vectors(r)
    rows = (P + 127) // 128
    try:
        for fused in (1, 0) if dtype == BF16 else (1,):
            L.call("dc_set_option", b"head_dgrad_fused", fused)
            for relu in (1, 0):
                what = f"{name} head_dgrad_fused={fused} relu={relu} dc_head_bwd_bnstats"
                sbuf, slab = rider_slab(rows, Cin)
                dbuf, gxv = empty_nhwc(N, H, W, Cin, dtype, ld=Cin + 8)
                gwbuf, gw = flat((Cin, 3, 3, 3))
                with served(what) as names:
                    L.call("dc_head_bwd_bnstats", dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(gld), vptr(wd), vptr(gxv), Cin + 8, vptr(gw), wsp, vptr(ybv),
                           Cin + 16, vptr(mean), vptr(invstd), vptr(ms), vptr(mh), relu, vptr(slab), S())
                if dtype == torch.float32:
                    assert names[-1] == "igemm128_f32", names
                elif fused:
                    assert names[-1] == "head_dgrad_stream", names
                else:
                    assert names[-1] in PLAIN_GEMM and "head_dgrad_stream" not in names, names
                torch.cuda.synchronize()
                exactly(from_nhwc(gxv), cast(c.gx, dtype), f"{what}: dx")
                exactly(gw.cpu(), c.gw.float(), f"{what}: weight gradient")
                assert all_nan(dbuf[..., Cin:]) and untouched(gwbuf) and all_nan(sbuf[-1]), f"{what}: wrote outside an output"
                check_rider_slab(slab, c.gx, r, relu, what)
    finally:
        L.call("dc_set_option", b"head_dgrad_fused", 1)


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "affine"])
@pytest.mark.parametrize("name,shape", HEAD_PARAMS)
def test_head_on_unstored_batchnorm_output(name, shape, relu):
    """dc_head_fwd_bnin, dc_head_fwd_loss_bnin and every call form of dc_head_bwd_bnin (bf16): the head's input act(y * scale + shift) with
    a power-of-two scale and an integer shift is exact, so every output meets float64 and not another kernel."""
    N, Cin, H, W = shape
    e = U.head_ends_case(shape)
    U.head_ends_preconditions(e, name)
    c, p, r, P, dt = e.c, e.bn[relu], e.rin, N * H * W, L.DC_BF16
    _, yv = to_nhwc(c.x, BF16, ld=Cin + 16, off=8)
    wd, gld = c.w.float().to(dev()), c.gy.float().to(dev())
    mean, invstd, sc, sh = rider_vectors(r)
    ws, wsp = head_workspace(dt, shape)
    labels, cw, n = loss_operands(e)
    head_args = (dt, N, Cin, H, W, vptr(yv), Cin + 16, vptr(sc), vptr(sh), relu, vptr(wd))
    buf, out = flat((N, 3, 2 * H, 2 * W))
    L.call("dc_head_fwd_bnin", *head_args, vptr(out), wsp, S())
    torch.cuda.synchronize()
    exactly(out.cpu(), p.y.float(), f"{name} dc_head_fwd_bnin: logits")
    assert untouched(buf)
    for store in (True, False):
        run_loss("dc_head_fwd_loss_bnin", head_args, wsp, p.score, p.y, shape, labels, cw, n, store, f"{name} dc_head_fwd_loss_bnin store={store}")
    rows = (P + 127) // 128
    bwd_args = (dt, N, Cin, H, W, vptr(yv), Cin + 16, vptr(sc), vptr(sh), relu, vptr(gld), vptr(wd))

    def check_slab(sbuf, slab, what):
        assert all_nan(sbuf[-1]), f"{what}: wrote behind its slab rows"
        check_rider_slab(slab, c.gx, r, relu, what)

    # parts = 3 with a stored dx and the sums; then parts = 1 and 2 one after the other, without sums
    for with_sums in (True, False):
        what = f"{name} dc_head_bwd_bnin " + ("parts=3" if with_sums else "parts=1,2")
        sbuf, slab = rider_slab(rows, Cin)
        dbuf, dx = empty_nhwc(N, H, W, Cin, BF16, ld=Cin + 8)
        gwbuf, gw = flat((Cin, 3, 3, 3))
        for parts in (3,) if with_sums else (1, 2):
            L.call("dc_head_bwd_bnin", *bwd_args, vptr(dx), Cin + 8, vptr(gw), wsp, vptr(mean), vptr(invstd), vptr(slab) if with_sums else None, parts, S())
        torch.cuda.synchronize()
        exactly(from_nhwc(dx), cast(c.gx, BF16), f"{what}: dx")
        exactly(gw.cpu(), p.gw.float(), f"{what}: weight gradient")
        assert all_nan(dbuf[..., Cin:]) and untouched(gwbuf)
        if with_sums:
            check_slab(sbuf, slab, what)
        else:
            assert all_nan(sbuf), f"{what}: wrote a slab it was not given"
    # parts = 3 without a dx: the weight gradient rides on the statistics pass from 256 pixels on (head_wgrad_fused = 1), or runs in front of it
    try:
        for switch in (1, 0):
            L.call("dc_set_option", b"head_wgrad_fused", switch)
            what = f"{name} head_wgrad_fused={switch} dc_head_bwd_bnin parts=3, no dx"
            sbuf, slab = rider_slab(rows, Cin)
            gwbuf, gw = flat((Cin, 3, 3, 3))
            with served(what) as names:
                L.call("dc_head_bwd_bnin", *bwd_args, None, 0, vptr(gw), wsp, vptr(mean), vptr(invstd), vptr(slab), 3, S())
            got = [k for k in names if k != "aux"]
            if switch and P >= 256:
                assert got == ["head_dgrad_stream_wgrad"], f"{what}: served by {got}"
            else:
                assert got[-1] == "head_dgrad_stream" and "head_dgrad_stream_wgrad" not in got and len(got) > 1, f"{what}: served by {got}"
            torch.cuda.synchronize()
            exactly(gw.cpu(), p.gw.float(), f"{what}: weight gradient")
            assert untouched(gwbuf)
            check_slab(sbuf, slab, what)
            # the gathered gradient image stays in the workspace for later passes (dc_head_bwd_bnin_apply; a parts = 2 call): it is intact
            gwbuf, gw = flat((Cin, 3, 3, 3))
            L.call("dc_head_bwd_bnin", *bwd_args, None, 0, vptr(gw), wsp, vptr(mean), vptr(invstd), None, 2, S())
            torch.cuda.synchronize()
            exactly(gw.cpu(), p.gw.float(), f"{what}, then parts=2 on the gathered image it left: weight gradient")
    finally:
        L.call("dc_set_option", b"head_wgrad_fused", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape", HEAD_PARAMS)
def test_head_score_and_predict(name, shape, dtype):
    """dc_head_fwd_score and dc_head_fwd_predict over the first n_valid samples: per-sample counts and masks equal, everything of the
    samples from n_valid on untouched (bf16: their logits too; fp32 runs the whole batch's GEMM and stores all logits)."""
    N, Cin, H, W = shape
    e, xv, wd, ws, wsp = head_operands(name, shape, dtype)
    dt, c, s = L.dtype_code(dtype), e.c, e.score
    labels, cw, _ = loss_operands(e)
    oshape = (N, 2 * H, 2 * W)
    for nv in sorted({0, 1, N}):
        for store in (True, False) if dtype == BF16 else (True,):
            what = f"{name} n_valid={nv} store={store}"
            for fn in ("dc_head_fwd_score", "dc_head_fwd_predict"):
                lbuf, lg = flat((N, 3, 2 * H, 2 * W))
                head_args = (dt, N, nv, Cin, H, W, vptr(xv), Cin + 8, vptr(wd), vptr(lg) if store else None, wsp)
                if fn == "dc_head_fwd_score":
                    ls = torch.zeros(N, dtype=torch.float64, device=dev())
                    cnt = torch.zeros((N, 9), dtype=torch.int64, device=dev())
                    ls[nv:], cnt[nv:] = -7.0, 12345
                    L.call(fn, *head_args, vptr(labels), 8, vptr(cw), vptr(ls), vptr(cnt), S())
                    torch.cuda.synchronize()
                    exactly(cnt[:nv].cpu(), s.counts[:nv], f"{what}: per-sample tp / fp / fn counts")
                    assert bool((cnt[nv:] == 12345).all()) and bool((ls[nv:] == -7.0).all()), f"{what}: touched a sample beyond n_valid"
                    print(f"{what}: per-sample loss sums {ls[:nv].tolist()}, reference {s.loss[:nv].tolist()}")
                    np.testing.assert_allclose(ls[:nv].cpu().numpy(), s.loss[:nv].numpy(), rtol=SAMPLE_LOSS_REL, err_msg=f"{what}: per-sample loss")
                else:
                    mask = torch.full(oshape, 255, dtype=torch.uint8, device=dev())
                    cbuf, conf = flat(oshape, fill=-1.0)
                    ccnt = torch.zeros((N, 3), dtype=torch.int64, device=dev())
                    ccnt[nv:] = 12345
                    L.call(fn, *head_args, vptr(mask), vptr(conf), vptr(ccnt), S())
                    torch.cuda.synchronize()
                    exactly(mask[:nv].cpu().long(), s.pred[:nv], f"{what}: class map")
                    exactly(ccnt[:nv].cpu(), s.classes[:nv], f"{what}: per-sample class counts")
                    assert bool((mask[nv:] == 255).all()) and bool((cbuf[conf[:nv].numel():] == -1.0).all()) and bool((ccnt[nv:] == 12345).all()), \
                        f"{what}: touched a sample beyond n_valid"
                    if nv:
                        err = float((conf[:nv].cpu().double() - s.conf[:nv]).abs().max())
                        print(f"{what}: confidence, max abs error {err:.3e} (allowed {CONF_ABS_TOL})")
                        assert err <= CONF_ABS_TOL, f"{what}: confidence"
                assert untouched(lbuf), f"{what} {fn}: wrote behind the logits"
                if not store:
                    assert all_nan(lg), f"{what} {fn}: logits written without a buffer"
                elif dtype == BF16:
                    exactly(lg[:nv].cpu(), c.y[:nv].float(), f"{what} {fn}: logits")
                    assert all_nan(lg[nv:]), f"{what} {fn}: logits of a sample beyond n_valid"
                else:
                    exactly(lg.cpu(), c.y.float(), f"{what} {fn}: logits")


def test_head_backward_where_both_grid_caps_bind():
    """HEAD_BIG, bf16: 2080 chunks of 128 pixels on the 2048 workgroups of the streaming data gradient (HD_STORE, dc_head_bwd_bnstats) and
    on the 512 workgroups of its weight-gradient form (HD_SUMS_WG, dc_head_bwd_bnin parts = 3 without a dx), so a workgroup takes a second
    chunk 2048 (512) chunks on.  dx, the weight gradient and the float64 column sums of the 2080 slab rows equal the matrix-product reference
    (util_exact.head_big_case: 1.5 s on the CPU).  The other calls of the head do not depend on these caps and stay at HEAD_ENDS."""
    m = U.head_big_case()
    N, Cin, H, W = U.HEAD_BIG
    P, dt = N * H * W, L.DC_BF16
    rows = (P + 127) // 128
    assert rows > 2048 and rows // 2 > 512
    yv, av = m.y.to(BF16).to(dev()), m.a.to(BF16).to(dev())           # [P][256]: NHWC, ld = 256
    wd, gld = m.w.to(dev()), m.gl.to(dev())
    mean, invstd, sc, sh = (t.float().to(dev()) for t in (m.mean, m.invstd, m.scale, m.shift))
    ws, wsp = head_workspace(dt, U.HEAD_BIG)

    def check(sbuf, slab, gwbuf, gw, what):
        exactly(gw.cpu(), m.gw, f"{what}: weight gradient")
        assert untouched(gwbuf) and all_nan(sbuf[-1]), f"{what}: wrote outside an output"
        s0, s1 = column_sums(slab)
        exactly(s0, m.s0, f"{what}: sum g")
        exactly(s1, m.s1, f"{what}: sum g * xhat")

    what = "dc_head_bwd_bnstats"
    sbuf, slab = rider_slab(rows, Cin)
    dxbuf, dx = flat((P, Cin), dtype=BF16, spare=Cin)
    gwbuf, gw = flat((Cin, 3, 3, 3))
    with served(what) as names:
        L.call("dc_head_bwd_bnstats", dt, N, Cin, H, W, vptr(av), Cin, vptr(gld), vptr(wd), vptr(dx), Cin, vptr(gw), wsp, vptr(yv), Cin, vptr(mean),
               vptr(invstd), vptr(sc), vptr(sh), 1, vptr(slab), S())
    assert names[-1] == "head_dgrad_stream", names
    torch.cuda.synchronize()
    exactly(dx.float().cpu(), m.dx, f"{what}: dx as [pixel][channel]")
    assert untouched(dxbuf, Cin)
    check(sbuf, slab, gwbuf, gw, what)
    what = "dc_head_bwd_bnin parts=3, no dx"
    sbuf, slab = rider_slab(rows, Cin)
    gwbuf, gw = flat((Cin, 3, 3, 3))
    with served(what) as names:
        L.call("dc_head_bwd_bnin", dt, N, Cin, H, W, vptr(yv), Cin, vptr(sc), vptr(sh), 1, vptr(gld), vptr(wd), None, 0, vptr(gw), wsp, vptr(mean),
               vptr(invstd), vptr(slab), 3, S())
    assert_served(names, ["head_dgrad_stream_wgrad"], what, ignore=("aux",))
    torch.cuda.synchronize()
    check(sbuf, slab, gwbuf, gw, what)
