"""The masked store of the residual-form depthwise data gradient (dc_dwconv_dgrad_wgrad_bnres[_sum] with relu = 2, csrc/dwpipe.hip) and the
block-end BatchNorm backward that lives on it: the data gradient of the next block's first depthwise layer, the last writer of the gradient
of a block output relu(bn(y) + residual), stores it masked by that output's sign; dc_bn_bwd_apply[_fin] then needs no mask, no stored output
and no copy for the shortcut (deeplab_xception.py:99-122 under train_hdf5_ddp.py:363).  Everything here is bit equality."""
import ctypes as C
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from oracle import loss_metric as olm  # noqa: E402
from util_inputs import make_inputs  # noqa: E402
from util_launch import served  # noqa: E402

# (C, N, H, W): a ragged last channel block with several tiles per workgroup; one tile per workgroup; half a channel block
CASES = [(728, 2, 16, 24), (256, 1, 8, 16), (64, 2, 40, 48)]
PAD = 8             # pad channels behind every pixel of dx: no launch may touch them


def dev():
    return torch.device("cuda", 0)


def S():
    return L.stream_ptr()


def vptr(view):
    return C.c_void_p(view.data_ptr())


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def q(t, dtype):
    return t.to(dtype).float()


def empty_nhwc(n, h, w, c, dtype, ld=None, fill=float("nan")):
    buf = torch.full((n, h, w, ld or c), fill, dtype=dtype, device=dev())
    return buf, buf[..., :c]


def to_nhwc(t_nchw, dtype, ld=None):
    """NCHW fp32 CPU -> device NHWC view of width C inside a [N,H,W,ld] buffer poisoned with NaN."""
    n, c, h, w = t_nchw.shape
    buf, view = empty_nhwc(n, h, w, c, dtype, ld)
    view[...] = t_nchw.permute(0, 2, 3, 1).to(dtype).to(dev())
    return buf, view


def _block_output(N, Cc, H, W):
    """The stored block output x (NCHW, bf16 values): random signs, and in every channel block exact +0.0, -0.0, a positive and a negative
    value at known pixels."""
    x = q(rnd(N, Cc, H, W, seed=1), torch.bfloat16)
    x[:, :, 0, 0] = 0.0
    x[:, :, 0, 1] = -0.0
    x[:, :, 0, 2] = 0.5
    x[:, :, 0, 3] = -0.5
    x[:, :, H - 1, W - 1] = -0.0
    x[:, :, H - 1, W - 2] = 0.0
    assert (x > 0).any() and (x < 0).any()
    assert torch.signbit(x[:, :, 0, 1]).all() and not torch.signbit(x[:, :, 0, 0]).any()
    return x


@pytest.mark.parametrize("sum_row", [False, True], ids=["slab", "sum_row"])
@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_masked_store_is_the_masked_gradient(case, with_addend, sum_row):
    Cc, N, H, W = case
    dt, lib, dtype = L.DC_BF16, L.load(), torch.bfloat16
    M = N * H * W
    rows = lib.dc_dwconv_dgrad_wgrad_bnres_rows(dt, Cc, 1, 1, N, H, W)
    assert rows > 0 and lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, 1, N, H, W) == 1
    xo = _block_output(N, Cc, H, W)
    ybn = q(rnd(N, Cc, H, W, seed=7), dtype)
    gy = q(rnd(N, Cc, H, W, seed=3), dtype)
    add = q(rnd(N, Cc, H, W, seed=4), dtype)
    wm = rnd(Cc, 1, 3, 3, seed=2, scale=1 / 3).to(dev())
    wd = torch.empty(9 * Cc, device=dev())
    L.call("dc_dwconv_pack_weights", Cc, vptr(wm), vptr(wd), S())
    mean, invstd = rnd(Cc, seed=8, scale=0.2).to(dev()), (torch.rand(Cc) + 0.5).to(dev())
    gamma = (torch.rand(Cc) + 0.5).to(dev())
    ld = (Cc + 31) // 32 * 32
    _, xv = to_nhwc(xo, dtype, ld=ld)
    _, yv = to_nhwc(ybn, dtype, ld=ld)
    _, gyv = to_nhwc(gy, dtype)
    keep = (xv > 0)
    fn = "dc_dwconv_dgrad_wgrad_bnres_sum" if sum_row else "dc_dwconv_dgrad_wgrad_bnres"

    def run(relu):
        dbuf, dx = to_nhwc(add, dtype, ld=Cc + PAD)              # dx starts as the other consumers' contribution; the addend aliases it
        dbuf[..., Cc:] = 3.0
        ap, al = (vptr(dx), Cc + PAD) if with_addend else (None, 0)
        wslab = torch.full((rows, 9, Cc), float("nan"), device=dev())
        slab = torch.zeros(2 * Cc, dtype=torch.float64, device=dev()) if sum_row else torch.full((2, rows, Cc), float("nan"), device=dev())
        with served(f"{fn} relu={relu}") as names:
            L.call(fn, dt, Cc, 1, 1, N, H, W, vptr(gyv), Cc, vptr(wd), ap, al, vptr(dx), Cc + PAD, vptr(xv), ld, vptr(wslab), vptr(yv), ld,
                   vptr(mean), vptr(invstd), relu, vptr(slab), S())
        torch.cuda.synchronize()
        assert names == ["dwpipe_dgrad_masked" if relu == 2 else "dwpipe_dgrad"], names
        assert (dbuf[..., Cc:] == 3.0).all(), "pad columns of dx written"
        return dx, wslab, slab

    dx1, ws1, slab1 = run(1)
    dx2, ws2, slab2 = run(2)
    assert not torch.isnan(dx1.float()).any()
    assert torch.equal(dx2, torch.where(keep, dx1, torch.zeros_like(dx1)))
    assert not torch.signbit(dx2[~keep]).any()                    # masked means +0.0, as the apply kernel's own mask writes it
    assert torch.equal(ws2, ws1) and torch.equal(slab2, slab1)

    # the consumer: no mask, no stored output, no shortcut copy on the masked dx == mask from x and a copy on the unmasked one
    def apply(dxv, relu, fin):
        _, dyv = empty_nhwc(N, H, W, Cc, dtype)
        gbuf, gv = empty_nhwc(N, H, W, Cc, dtype)
        op, ol, gp, gl = (vptr(xv), ld, vptr(gv), Cc) if relu else (None, 0, None, 0)
        dgam, dbet = torch.full((Cc,), float("nan"), device=dev()), torch.full((Cc,), float("nan"), device=dev())
        srows = -1 if sum_row else rows
        if fin:
            L.call("dc_bn_bwd_apply_fin", dt, M, Cc, M, vptr(dxv), Cc + PAD, vptr(yv), ld, op, ol, relu, vptr(gamma), vptr(mean), vptr(invstd),
                   vptr(slab1), srows, vptr(dgam), vptr(dbet), vptr(dyv), Cc, gp, gl, None, None, S())
        else:
            L.call("dc_bn_bwd_finalize", Cc, vptr(slab1), srows, vptr(dgam), vptr(dbet), S())
            L.call("dc_bn_bwd_apply", dt, M, Cc, M, vptr(dxv), Cc + PAD, vptr(yv), ld, op, ol, relu, vptr(gamma), vptr(mean), vptr(invstd),
                   vptr(dgam), vptr(dbet), vptr(dyv), Cc, gp, gl, None, None, S())
        torch.cuda.synchronize()
        return dyv, gv, dgam, dbet

    forms = [False]
    if sum_row or rows <= lib.dc_bn_bwd_apply_fin_max_rows():
        forms.append(True)
    assert not sum_row or True in forms                          # the sum-row form is always served by the apply that finalizes itself
    for fin in forms:
        dy_ref, g_ref, dg_ref, db_ref = apply(dx1, 1, fin)
        dy_new, _, dg_new, db_new = apply(dx2, 0, fin)
        assert not torch.isnan(dy_ref.float()).any()
        assert torch.equal(dy_new, dy_ref), f"fin={fin}"
        assert torch.equal(g_ref, dx2), f"fin={fin}"
        assert torch.equal(dg_new, dg_ref) and torch.equal(db_new, db_ref)


def test_masked_form_follows_its_switch():
    """Option dw_res_masked = 0: the query says 0 and relu = 2 is an error, not another kernel; relu = 0 / 1 are served as before."""
    Cc, N, H, W = 256, 1, 8, 16
    dt, lib = L.DC_BF16, L.load()
    assert lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, 1, N, H, W) == 1
    assert lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, 2, N, H, W) == 0          # the residual form is built for dilation 1
    assert lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, 1, N, H, W + 4) == 0      # not a multiple of the 8-pixel tile
    L.call("dc_set_option", b"dw_res_masked", 0)
    try:
        assert lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, 1, N, H, W) == 0
        rows = lib.dc_dwconv_dgrad_wgrad_bnres_rows(dt, Cc, 1, 1, N, H, W)
        assert rows > 0
        t = [empty_nhwc(N, H, W, Cc, torch.bfloat16, fill=0.0)[1] for _ in range(4)]
        wd, vec = torch.zeros(9 * Cc, device=dev()), torch.ones(Cc, device=dev())
        wslab, slab = torch.zeros(rows * 9 * Cc, device=dev()), torch.zeros(2 * rows * Cc, device=dev())
        args = lambda relu: (dt, Cc, 1, 1, N, H, W, vptr(t[0]), Cc, vptr(wd), None, 0, vptr(t[1]), Cc, vptr(t[2]), Cc, vptr(wslab), vptr(t[3]), Cc,
                             vptr(vec), vptr(vec), relu, vptr(slab), S())
        with pytest.raises(L.DeepcamHipError, match="dw_res_masked"):
            L.call("dc_dwconv_dgrad_wgrad_bnres", *args(2))
        with served("relu=1, switch off") as names:
            L.call("dc_dwconv_dgrad_wgrad_bnres", *args(1))
        assert names == ["dwpipe_dgrad"]
        torch.cuda.synchronize()
    finally:
        L.call("dc_set_option", b"dw_res_masked", 1)


# ---- the engine: the same step with the switch on and off
def _extent(batch):
    """The smallest input extent whose middle flow (728 channels, 1/16 of the input) the masked form serves."""
    lib = L.load()
    for H, W in ((128, 128), (128, 192), (128, 256), (256, 256)):
        if lib.dc_dwconv_dgrad_wgrad_bnres_masked(L.DC_BF16, 728, 1, 1, batch, H // 16, W // 16) == 1:
            return H, W
    raise AssertionError("no candidate extent is served")


def _run_steps(masked, program, batches, B, H, W):
    """Two LAMB steps; returns (per-step results, the engine's list of masked block ends, launch names of one step, library calls of one step)."""
    d = dev()
    L.call("dc_set_option", b"dw_res_masked", 1 if masked else 0)
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(B, H, W)
    net.train()
    opt = dnn.make_optimizer("LAMB", net, 1e-3, 1e-8, 1e-2)
    step = dnn.TrainStep(net, opt, olm.class_weights(-0.125), B, H, W, with_metrics=True)
    eng = net.engine
    z = (torch.zeros(B, 16, H, W, device=d), torch.zeros(B, H, W, dtype=torch.int64, device=d))
    names, calls = [], []
    if program:
        eng.x_static.zero_()
        step.enable_program()                   # two real steps on the static buffers
    else:
        real = L.call

        def spy(name, *args):
            calls.append((name, args))
            return real(name, *args)
        L.call = spy
        try:
            with served("one eager step") as names:
                step(*z)
        finally:
            L.call = real
        step(*z)
    out = []
    for x, y in batches:
        step(x.to(d), y.to(d))
        torch.cuda.synchronize()
        out.append((step.loss(), eng.dlogits.clone(), eng.grads.clone(), eng.params.clone(), eng.buffers.clone()))
    return out, list(eng.masked_block_ends), names, calls


def _same(a, b):
    """Bit equality of the loss's per-pixel gradient (a function of the logits alone), the gradients, the parameters and the BatchNorm
    buffers.  The reported loss itself is a sum of per-workgroup fp64 partial sums added by atomics in arrival order: two runs of ONE build
    differ in its last bits (1e-16 relative, see test_train_step_is_bit_reproducible), so it is held to 1e-12 and the bits are asked of
    the tensor it is summed from."""
    for (la, da, ga, pa, ba), (lb, db, gb, pb, bb) in zip(a, b):
        assert abs(la - lb) <= 1e-12 * abs(la)
        assert torch.equal(da, db)
        assert torch.equal(ga, gb) and torch.equal(pa, pb) and torch.equal(ba, bb)


@pytest.fixture(scope="module")
def switch_off_steps():
    B = 2
    H, W = _extent(B)
    batches = [make_inputs(B, H, W, seed=s) for s in (1, 2)]
    try:
        out, ends, names, calls = _run_steps(False, False, batches, B, H, W)
    finally:
        L.call("dc_set_option", b"dw_res_masked", 1)
    return {"B": B, "H": H, "W": W, "batches": batches, "out": out, "ends": ends, "names": names, "calls": calls}


def _block_end_applies(calls):
    """(bn_bwd_apply calls that follow a residual-form data gradient directly, all residual-form data gradients) of one step's library calls."""
    res = [(n, a) for n, a in calls if n.startswith("dc_dwconv_dgrad_wgrad_bnres")]
    follow = []
    for i, (n, a) in enumerate(calls):
        if n.startswith("dc_dwconv_dgrad_wgrad_bnres"):
            nxt = next((c for c in calls[i + 1:] if c[0].startswith(("dc_bn_bwd_apply", "dc_bn_bwd_reduce", "dc_bn_bwd_frozen", "dc_dwconv_dgrad"))
                        and c[0] != "dc_bn_bwd_apply_fin_max_rows"), None)
            assert nxt is not None and nxt[0] in ("dc_bn_bwd_apply", "dc_bn_bwd_apply_fin"), (n, nxt and nxt[0])
            follow.append(nxt)
    return follow, res


def _is_null(v):
    return v is None or getattr(v, "value", v) in (None, 0)


def test_engine_step_is_the_same_with_masked_block_ends(switch_off_steps):
    s = switch_off_steps
    B, H, W = s["B"], s["H"], s["W"]
    out, ends, names, calls = _run_steps(True, False, s["batches"], B, H, W)
    # the plan: every middle block (4 .. 19) ends on the masked form; with the switch off none does and no masked launch runs
    blocks = sorted(int(re.match(r"xception_features\.block(\d+)\.", b).group(1)) for b in ends)
    assert set(range(4, 20)) <= set(blocks), blocks
    assert s["ends"] == [] and "dwpipe_dgrad_masked" not in s["names"]
    # the served-kernel record: every residual-form launch of the fused block ends ran masked
    follow, res = _block_end_applies(calls)
    assert len(res) == len(ends) and len(follow) == len(ends)
    assert names.count("dwpipe_dgrad_masked") == len(ends)
    assert all(a[-3] == 2 for _, a in res), [a[-3] for _, a in res]
    # ... and no block-end apply received the stored output or a shortcut buffer: (..., y, ldy, out, ldout, relu, ...), g_out 4th / 5th from the end
    for n, a in follow:
        assert _is_null(a[8]) and a[9] == 0 and a[10] == 0, (n, a[8:11])
        assert _is_null(a[-5]) and a[-4] == 0, (n, a[-5:-3])
    # the switch off is the step as it was: as many launches, the same calls; relu = 1 with the stored output and a shortcut buffer
    follow0, res0 = _block_end_applies(s["calls"])
    assert [n for n, _ in s["calls"]] == [n for n, _ in calls] and len(s["names"]) == len(names)
    assert len(res0) == len(res) and all(a[-3] in (0, 1) for _, a in res0)
    assert all(not _is_null(a[-5]) for _, a in follow0)
    _same(out, s["out"])


def test_engine_launch_list_replay_is_the_same_with_masked_block_ends(switch_off_steps):
    s = switch_off_steps
    out, ends, _, _ = _run_steps(True, True, s["batches"], s["B"], s["H"], s["W"])
    assert len(ends) >= 16
    _same(out, s["out"])
