"""Kernel tests on exactly representable data: equality with the float64 reference, no tolerance.

test_kernels_gpu.py pins the kernels of the training step to PyTorch within a fraction of the output scale (2.5e-2 in bf16, 2e-3 relative on
the BatchNorm slabs) and the fast variants to "the bits of the plain kernel".  That leaves the mistakes of hand-written tile kernels
invisible: a few pixels lost from the statistics or the weight gradient, one 8-channel vector or K step missing at a border (the figures
are in test_exact_cpu.py).  Here the data are small integers (util_exact.py): every product, partial sum and stored value is exactly
representable, so a correct kernel reproduces the float64 reference bit for bit in fp32 and in bf16, whatever its tiling, K order, split
or slab layout, and so do its statistics and weight gradients.  Every assertion is torch.equal (util_exact.exactly names the first
differing element as (n, channel, row, column)) or equality of float64 sums.

Only the data differ from what test_kernels_gpu.py launches: the same entry points through the C ABI, the same shapes (taken from that
file's tables by util_exact.gpu_cases), the same option values, padded views poisoned with NaN, and the same launch-record expectations, so
a variant that silently falls back still fails.  Two extents are not in that file: the pooled image is 8 x 16, so that 1 / HW is a power of
two, and dc_stem_dgrad runs at the shape of test_stem (test_autograd_ext_gpu.py has it at 32 x 48 and 64 x 96).  Every test calls the preconditions first; test_exact_cpu.py proves them for all cases without a GPU.

Covered: dense convolutions under the default planner (CONV_CASES, fp32 and bf16: forward with slab, accumulate, bias, both data gradients,
weight gradient); the forced variants igemm256 = 2, pw384 = 2 .. 5, pw224 = 2 / 3 (dc_conv_fwd_kn / dc_conv_dgrad_kn, compact slab),
igemm256p, thin_tile, dc_conv_fwd_dilated_group; the weight-gradient families (GROUP_CASES, WG384_CASES, TCONV384_CASES, FOLD_CASES);
depthwise (DW_CASES, PIPE_CASES with dw_pipe 0 / 1 / 2); dc_bn_stats, dc_colsum, dc_sum_hw, dc_avgpool_fwd / dc_avgpool_bwd_add; stem and
head at the one shape test_kernels_gpu.py gives each (20 x 28 and 6 x 9: less than one block, tile or chunk of their kernels; odd, ragged and
multi-tile extents, thinner stems, the loss / score / prediction epilogues, the head on an unstored BatchNorm output and the extent at which
the head's grid caps bind are in test_exact_ends_gpu.py).  dc_dwconv_fwd has no statistics slab in its C ABI, so "forward with slab" is
the forward alone for the depthwise layers.

Second tier, built because reading the kernels shows every operation exact on this data (integer mean, power-of-two invstd and scale,
integer shift; the epilogues are gm = mask ? g : 0, a += gm, b = fma(gm, (y - mean) * invstd, b): igemm.hip, igemm256.hip, BnAcc::add in
dwtile_common.h, dwpipe.hip, head_dgrad_kernel in stem_head.hip; a sum row is fp64 atomics of those fp32 sums):
  - dc_conv_dgrad_bnstats on BNSTAT_CASES (128- and 256-tile);
  - dc_dwconv_dgrad_bnstats and dc_dwconv_dgrad_bnstats_wgrad on DW_CASES, and those two plus dc_dwconv_dgrad_bnstats_wgrad_add on
    PIPE_CASES under dw_pipe 0 / 1 / 2;
  - dc_dwconv_dgrad_wgrad_bnres (relu 0, 1, and 2 where dc_dwconv_dgrad_wgrad_bnres_masked serves) with and without an addend on the
    dilation-1 PIPE_CASES, the stored input built as relu(bn(ybn) + residual); dc_dwconv_dgrad_wgrad_bnres_sum and
    dc_dwconv_dgrad_bnstats_wgrad_sum on the shapes test_kernels_gpu.py and test_dw_masked_gradient_gpu.py give them;
  - dc_head_bwd_bnstats at the shape of test_head, on the streaming and on the tiled data-gradient kernel (at more than one chunk, and
    dc_head_bwd_bnin with the weight gradient riding on the statistics pass: test_exact_ends_gpu.py);
  - dc_sepconv_fwd on SEPFWD_CASES, with generators of its own (util_exact.sep_case): at 65 536 pixels and more the sums of squares pass
    2^24 with the budget and the prologue range of the other cases.

Left out:
  - DW_CASES s2_walk: at 264 x 420 the float64 CPU reference of its depthwise gradients is slow; PIPE_CASES 728_b8 and the *_b8 shapes of
    the pointwise tables: they run at the workload's full extent (27 648 pixels of 728 channels);
  - dc_pw_bn_bwd: it applies the BatchNorm backward, its coefficients carry inv_count = 1.0f / count (pwbwd.hip), and the pixel counts of
    its cases (2 x 192 x 192, 257 x 257, ...) are no powers of two: a rounded reciprocal;
  - dc_head_bwd_bnin_apply, for the same reason (1 / count; the head's extents are no powers of two either);
  - BatchNorm finalize / apply (1 / sqrt), the loss and every softmax consumer (test_exact_ends_gpu.py holds the head's fused loss, score
    and prediction to the float64 logits' classes and counts exactly, and to the project's tolerances in loss, gradient and confidence),
    the optimizers, and the workload's full extents.

The tests that override options restore them in `finally` (dc_reset_options where a case brings its own list of overrides)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402
from test_kernels_gpu import DTYPES, PLAIN_GEMM, S, desc, dev, empty_nhwc, from_nhwc, to_nhwc, vptr  # noqa: E402
from util_launch import assert_served, served  # noqa: E402
import util_exact as U  # noqa: E402
from util_exact import exactly  # noqa: E402

CASES = U.gpu_cases()
NAN = float("nan")


def ids(family):
    return [c[0] for c in CASES[family]]


def cast(ref, dtype):
    """The float64 reference cast to the compared type, as the fp32 tensor from_nhwc returns."""
    return ref.to(dtype).float()


def check_served(names, want, what):
    """want: a name or a list of names in launch order (assert_served), or a tuple of alternatives for a single launch."""
    if want is None:
        return
    if isinstance(want, tuple):
        assert len(names) == 1 and names[0] in want, f"{what}: served by {names}, expected one of {want}"
    else:
        assert_served(names, want, what)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def pack(d, w, dtype):
    nwf, nwb = C.c_size_t(), C.c_size_t()
    L.call("dc_conv_packed_elems", C.byref(d), C.byref(nwf), C.byref(nwb))
    wf = torch.empty(nwf.value, dtype=dtype, device=dev())
    wb = torch.empty(nwb.value, dtype=dtype, device=dev())
    L.call("dc_conv_pack_weights", C.byref(d), vptr(w.float().to(dev())), vptr(wf), vptr(wb), S())
    return wf, wb


def column_sums(slab):
    """float64 column sums of a [2][rows][C] slab: (sum, sum of squares) per channel."""
    assert not torch.isnan(slab).any(), "a slab row was not written"
    s = slab.double().sum(1).cpu()
    return s[0], s[1]


FWD_STEPS = {"fwd": (1, 0, 0), "fwd_nostat": (0, 0, 0), "fwd_acc": (0, 0, 1), "fwd_bias": (0, 1, 0), "fwd_bias_acc": (0, 1, 1)}   # slab, bias, accumulate
CONV_STEPS = ("fwd", "fwd_acc", "fwd_bias", "dgrad", "dgrad_acc", "wgrad")         # the six calls of test_conv_fwd_dgrad_wgrad
SAME_BITS_STEPS = ("fwd", "fwd_bias_acc", "dgrad")                                 # the calls of the *_same_bits tests


def run_conv(name, spec, dtype, steps, expect=None, seeds=(1, 2, 3, 5), kn=False):
    """The calls `steps` of one convolution case on exact data, through padded NaN-poisoned views as in test_kernels_gpu.py; every result
    equal to the float64 reference.  expect: step -> who must serve it (check_served).  kn: the dc_conv_fwd_kn / dc_conv_dgrad_kn entry
    points with the compact slab of dc_conv_stat_rows_kn."""
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    c = U.conv_case(spec, seeds)
    U.preconditions(c, name)
    expect = expect or {}
    lib = L.load()
    d = desc(dtype, k, stride, pad, dil, tr, cin, cout)
    Ho, Wo = C.c_int(), C.c_int()
    L.call("dc_conv_out_hw", C.byref(d), H, W, C.byref(Ho), C.byref(Wo))
    Ho, Wo = Ho.value, Wo.value
    assert (Ho, Wo) == tuple(c.y.shape[2:])
    wf, wb = pack(d, c.w, dtype)
    _, xv = to_nhwc(c.x, dtype, ld=cin + 16, off=8)
    _, gyv = to_nhwc(c.gy, dtype)
    ybuf, yv = empty_nhwc(N, Ho, Wo, cout, dtype, ld=cout + 24, off=16)
    gbuf, gxv = empty_nhwc(N, H, W, cin, dtype, ld=cin + 8, off=0)
    bias = c.bias.float().to(dev())
    rows = (lib.dc_conv_stat_rows_kn if kn else lib.dc_conv_stat_rows)(C.byref(d), N, H, W)
    y_state = gx_state = None
    for step in steps:
        what = f"{name} {step}"
        if step in FWD_STEPS:
            with_slab, with_bias, acc = FWD_STEPS[step]
            slab = torch.full((3, rows, cout), NAN, device=dev())          # [2]: a neighbour's rows, must stay NaN
            sl, bi = (vptr(slab) if with_slab else None), (vptr(bias) if with_bias else None)
            with served(what) as names:
                if kn:
                    L.call("dc_conv_fwd_kn", C.byref(d), N, H, W, vptr(xv), cin + 16, vptr(wf), vptr(wb), bi, vptr(yv), cout + 24, sl,
                           rows if with_slab else 0, acc, S())
                else:
                    L.call("dc_conv_fwd", C.byref(d), N, H, W, vptr(xv), cin + 16, vptr(wf), bi, vptr(yv), cout + 24, sl, acc, S())
            check_served(names, expect.get(step), what)
            torch.cuda.synchronize()
            want = c.y + c.bias.view(1, -1, 1, 1) if with_bias else c.y
            y_state = y_state + want if acc else want
            exactly(from_nhwc(yv), cast(y_state, dtype), what)
            assert all_nan(ybuf[..., :16]) and all_nan(ybuf[..., 16 + cout:]), f"{what}: wrote outside its channel slice"
            if with_slab:
                assert all_nan(slab[2]), f"{what}: wrote behind its slab rows"
                s, ss = column_sums(slab[:2])
                exactly(s, c.sum_y, f"{what}: sum of y per channel")
                exactly(ss, c.sum_yy, f"{what}: sum of y^2 per channel")
        elif step in ("dgrad", "dgrad_acc"):
            acc = int(step == "dgrad_acc")
            with served(what) as names:
                if kn:
                    L.call("dc_conv_dgrad_kn", C.byref(d), N, H, W, vptr(gyv), cout, vptr(wb), vptr(wf), vptr(gxv), cin + 8, acc, S())
                else:
                    L.call("dc_conv_dgrad", C.byref(d), N, H, W, vptr(gyv), cout, vptr(wb), vptr(gxv), cin + 8, acc, S())
            check_served(names, expect.get(step), what)
            torch.cuda.synchronize()
            gx_state = gx_state + c.gx if acc else c.gx
            exactly(from_nhwc(gxv), cast(gx_state, dtype), what)
            assert all_nan(gbuf[..., cin:]), f"{what}: wrote outside its channel slice"
        else:
            assert step == "wgrad"
            wsb = lib.dc_conv_wgrad_workspace(C.byref(d), N, H, W)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev())
            gw = torch.full(c.wshape, NAN, device=dev())
            with served(what) as names:
                L.call("dc_conv_wgrad", C.byref(d), N, H, W, vptr(xv), cin + 16, vptr(gyv), cout, vptr(ws), wsb, vptr(gw), S())
            check_served(names, expect.get(step), what)
            torch.cuda.synchronize()
            exactly(gw.cpu(), c.gw.float(), what)
    return rows


# ------------------------------------------------------------------------------------------------------------------ dense convolutions
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES["conv"], ids=ids("conv"))
def test_conv_default_planner(case, dtype):
    name, spec, _ = case
    run_conv(name, spec, dtype, CONV_STEPS)


@pytest.mark.parametrize("case", CASES["conv"], ids=ids("conv"))
def test_conv_256_tile_kernel(case):
    name, spec, _ = case
    L.call("dc_set_option", b"igemm256", 2)
    try:
        run_conv(name, spec, torch.bfloat16, CONV_STEPS, tk.IGEMM256_FORCED[name])
    finally:
        L.call("dc_set_option", b"igemm256", 1)


@pytest.mark.parametrize("case", CASES["pw384"], ids=ids("pw384"))
def test_conv_pointwise_384_tile_kernels(case):
    """Option pw384 = 2 .. 5 (256 x 384, 128 x 384, 256 x 384 with 64-deep stages, 128 x 192).  Fallback on purpose, as in
    test_conv_pointwise_384_tile_kernel_same_bits: a data gradient with fewer than 64 input channels stays on a plain tile kernel."""
    name, spec, _ = case
    cout = spec[6]
    try:
        for mode in (2, 3, 4, 5):
            L.call("dc_set_option", b"pw384", mode)
            fam = tk.PW384_NAME[mode]
            run_conv(f"{name} pw384={mode}", spec, torch.bfloat16, SAME_BITS_STEPS,
                     dict(fwd=fam, fwd_bias_acc=fam, dgrad=fam if cout >= 64 else PLAIN_GEMM))
    finally:
        L.call("dc_set_option", b"pw384", 1)


@pytest.mark.parametrize("case", CASES["pw224"], ids=ids("pw224"))
def test_conv_pointwise_224_tile_kernels(case):
    """Option pw224 = 2 / 3 (224 x 384, 224 x 192) through dc_conv_fwd_kn / dc_conv_dgrad_kn, the slab one row per 224-pixel tile."""
    name, spec, _ = case
    N, H, W = spec[7:]
    try:
        for tile in (2, 3):
            L.call("dc_set_option", b"pw384", 1)
            L.call("dc_set_option", b"pw224", tile)
            fam = "pw224_384" if tile == 2 else "pw224_192"
            rows = run_conv(f"{name} pw224={tile}", spec, torch.bfloat16, SAME_BITS_STEPS, dict(fwd=fam, fwd_bias_acc=fam, dgrad=fam), kn=True)
            assert rows == (N * H * W + 223) // 224
    finally:
        L.call("dc_set_option", b"pw384", 1)
        L.call("dc_set_option", b"pw224", 1)


@pytest.mark.parametrize("case", CASES["persist"], ids=ids("persist"))
def test_conv_persistent_tiles(case):
    """igemm256p.hip forced where it is eligible (the last two columns of PERSIST_CASES), forward with and without statistics and the data
    gradient."""
    name, spec, extra = case
    fwd = "igemm256p" if extra["fwd"] == "p" else "igemm256"
    try:
        L.call("dc_set_option", b"igemm256", 2)
        L.call("dc_set_option", b"igemm256p_min", 1)
        L.call("dc_set_option", b"igemm256p_wgs", extra["wgs"])
        L.call("dc_set_option", b"igemm256p", 1)
        run_conv(name, spec, torch.bfloat16, ("fwd", "fwd_nostat", "dgrad"),
                 dict(fwd=fwd, fwd_nostat=fwd, dgrad="igemm256p" if extra["dgrad"] == "p" else "igemm256"))
    finally:
        L.call("dc_set_option", b"igemm256", 1)
        L.call("dc_set_option", b"igemm256p", 1)
        L.call("dc_set_option", b"igemm256p_min", 257)
        L.call("dc_set_option", b"igemm256p_wgs", 0)


@pytest.mark.parametrize("case", CASES["thin_tile"], ids=ids("thin_tile"))
def test_thin_conv_kernels(case):
    """The LDS-tiled kernel of the stride-1 thin layers (thin_tile = 1) and the gather-form kernel it replaces (thin_tile = 0)."""
    name, spec, _ = case
    try:
        for tiled in (1, 0):
            L.call("dc_set_option", b"thin_tile", tiled)
            fam = "thin_tile" if tiled else "thin_fwd"
            run_conv(f"{name} thin_tile={tiled}", spec, torch.bfloat16, ("fwd", "dgrad"), dict(fwd=fam, dgrad=fam))
    finally:
        L.call("dc_set_option", b"thin_tile", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dilated_group(dtype):
    """dc_conv_fwd_dilated_group at its small shape: three atrous branches over one input in one launch (bf16; fp32 runs the per-branch
    fallback inside the entry point), outputs into channel slices of one buffer, a slab per member."""
    members = CASES["dilated_group"]
    k, stride, _, _, tr, cin, cout, N, H, W = members[0][1]
    cs = [U.conv_case(spec, extra["seeds"]) for _, spec, extra in members]
    for (name, _, _), c in zip(members, cs):
        U.preconditions(c, name)
        assert torch.equal(c.x, cs[0].x)                # one input
    dils = [spec[3] for _, spec, _ in members]
    _, xv = to_nhwc(cs[0].x, dtype, ld=cin + 32, off=16)
    d0 = desc(dtype, 3, 1, 1, 1, 0, cin, cout)
    wfs = [pack(desc(dtype, 3, 1, dil, dil, 0, cin, cout), c.w, dtype)[0] for dil, c in zip(dils, cs)]
    rows = L.load().dc_conv_stat_rows(C.byref(desc(dtype, 3, 1, dils[0], dils[0], 0, cin, cout)), N, H, W)
    cat = torch.full((N, H, W, 3 * cout + 8), NAN, dtype=dtype, device=dev())
    ys = [cat[..., b * cout:(b + 1) * cout] for b in range(3)]
    slabs = [torch.full((2, rows, cout), NAN, device=dev()) for _ in dils]
    with served("dilated group") as names:
        L.call("dc_conv_fwd_dilated_group", C.byref(d0), N, H, W, 3, (C.c_int * 3)(*dils), vptr(xv), cin + 32,
               (C.c_void_p * 3)(*[t.data_ptr() for t in wfs]), (C.c_void_p * 3)(*[t.data_ptr() for t in ys]), 3 * cout + 8,
               (C.c_void_p * 3)(*[t.data_ptr() for t in slabs]), S())
    assert_served(names, ["igemm256"] if dtype == torch.bfloat16 else ["igemm128_f32"] * 3, "dc_conv_fwd_dilated_group")
    torch.cuda.synchronize()
    assert all_nan(cat[..., 3 * cout:])
    for b, c in enumerate(cs):
        exactly(from_nhwc(ys[b]), cast(c.y, dtype), f"member {b} (dilation {dils[b]})")
        s, ss = column_sums(slabs[b])
        exactly(s, c.sum_y, f"member {b}: sum of y")
        exactly(ss, c.sum_yy, f"member {b}: sum of y^2")


BNSTAT_TILES = [pytest.param(torch.float32, 0, id="f32-tile128"), pytest.param(torch.bfloat16, 0, id="bf16-tile128"),
                pytest.param(torch.bfloat16, 2, id="bf16-tile256")]


def rider_vectors(r):
    return tuple(t.float().to(dev()) for t in (r.mean, r.invstd, r.mscale, r.mshift))


def check_rider_slab(slab, g, r, relu, what):
    """[2][rows][C] BatchNorm-backward partial sums: float64 column sums equal to (sum g, sum g * xhat)."""
    s0, s1 = column_sums(slab)
    want0, want1 = U.bn_bwd_sums(g, r, relu, what)
    exactly(s0, want0, f"{what}: sum g")
    exactly(s1, want1, f"{what}: sum g * xhat")


@pytest.mark.parametrize("dtype,tile", BNSTAT_TILES)
@pytest.mark.parametrize("case", CASES["bnstat"], ids=ids("bnstat"))
def test_conv_dgrad_with_bn_backward_statistics(case, dtype, tile):
    """dc_conv_dgrad_bnstats (second tier: the epilogue is mask, add, fma with (y - mean) * invstd; nothing else): dx equal to autograd's,
    the slab's column sums equal to the masked sums of it, on the 128-tile and the 256-tile kernel."""
    name, spec, _ = case
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    c = U.conv_case(spec)
    U.preconditions(c, name)
    r = U.bn_rider((N, cin, H, W))
    d = desc(dtype, k, stride, pad, dil, tr, cin, cout)
    wf, wb = pack(d, c.w, dtype)
    _, gyv = to_nhwc(c.gy, dtype)
    _, ybv = to_nhwc(r.y, dtype, ld=cin + 16, off=8)
    mean, invstd, ms, mh = rider_vectors(r)
    tile_name = "igemm256" if tile == 2 else "igemm128_bf16" if dtype == torch.bfloat16 else "igemm128_f32"
    try:
        L.call("dc_set_option", b"igemm256", tile)
        rows = L.load().dc_conv_dgrad_bnstats_rows(C.byref(d), N, H, W)
        assert rows > 0
        for relu in (1, 0):
            what = f"{name} relu={relu}"
            slab = torch.full((2, rows, cin), NAN, device=dev())
            dbuf, dx = empty_nhwc(N, H, W, cin, dtype, ld=cin + 8, off=0)
            with served(what) as names:
                L.call("dc_conv_dgrad_bnstats", C.byref(d), N, H, W, vptr(gyv), cout, vptr(wb), vptr(dx), cin + 8, vptr(ybv), cin + 16,
                       vptr(mean), vptr(invstd), vptr(ms), vptr(mh), relu, vptr(slab), S())
            assert_served(names, tile_name, what)
            torch.cuda.synchronize()
            exactly(from_nhwc(dx), cast(c.gx, dtype), f"{what}: dx")
            assert all_nan(dbuf[..., cin:])
            check_rider_slab(slab, c.gx, r, relu, what)
    finally:
        L.call("dc_set_option", b"igemm256", 1)


# ------------------------------------------------------------------------------------------------------------------ weight gradients
def layer_views(spec, layers, dtype, ldgy_pad=0):
    """Operand views and float64 references of the `layers` layers of a grouped weight-gradient call."""
    cin, cout = spec[5], spec[6]
    cs, xs, gys, keep = [], [], [], []
    for l in range(layers):
        c = U.conv_case(spec, U.layer_seeds(l))
        U.preconditions(c, f"layer {l}")
        xb, xv = to_nhwc(c.x, dtype, ld=cin + 16, off=8)
        gb, gyv = to_nhwc(c.gy, dtype, ld=cout + ldgy_pad)
        keep += [xb, gb]
        cs.append(c)
        xs.append(xv)
        gys.append(gyv)
    return cs, xs, gys, keep


def pa(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES["wgrad_group"], ids=ids("wgrad_group"))
def test_conv_wgrad_group(case, dtype):
    """dc_conv_wgrad_group: every layer's gradient equal to autograd's; who serves it as in test_kernels_gpu.test_conv_wgrad_group."""
    name, spec, extra = case
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    layers = extra["layers"]
    d = desc(dtype, k, stride, pad, dil, tr, cin, cout)
    cs, xs, gys, keep = layer_views(spec, layers, dtype)
    lib = L.load()
    wsb = lib.dc_conv_wgrad_group_workspace(C.byref(d), N, H, W, layers)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev())
    gws = [torch.full(cs[0].wshape, NAN, device=dev()) for _ in range(layers)]
    with served("wgrad_group") as names:
        L.call("dc_conv_wgrad_group", C.byref(d), N, H, W, layers, pa(xs), cin + 16, pa(gys), cout, vptr(ws), wsb, pa(gws), S())
    if dtype == torch.bfloat16 and name not in ("thin_x2_falls_back", "dense3x3_x2"):
        assert_served(names, ["wgrad384_pw" if k == 1 else "wgrad384_3x3"] + ["wgrad_reduce"] * layers, name)
    else:       # fallbacks on purpose: fp32, a thin layer, rows shorter than a stage
        assert_served(names, ["wgrad128_bf16" if dtype == torch.bfloat16 else "wgrad128_f32", "wgrad_reduce"] * layers, name)
    torch.cuda.synchronize()
    for l in range(layers):
        exactly(gws[l].cpu(), cs[l].gw.float(), f"{name} layer {l}")


@pytest.mark.parametrize("case", CASES["wgrad384"], ids=ids("wgrad384"))
def test_conv_wgrad_384_tile_kernel(case):
    """wgrad384.hip forced (option wgrad384 = 2, with the case's split overrides) and the 128-tile kernel (0): both equal to autograd."""
    name, spec, extra = case
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    layers, dtype = extra["layers"], torch.bfloat16
    d = desc(dtype, k, 1, pad, dil, 0, cin, cout)
    cs, xs, gys, keep = layer_views(spec, layers, dtype, ldgy_pad=8)
    lib = L.load()
    try:
        for mode in (2, 0):
            L.call("dc_set_option", b"wgrad384", mode)
            for kk, v in extra["opts"].items():
                L.call("dc_set_option", kk.encode(), v)
            wsb = lib.dc_conv_wgrad_group_workspace(C.byref(d), N, H, W, layers)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev())
            gws = [torch.full(cs[0].wshape, NAN, device=dev()) for _ in range(layers)]
            with served(f"wgrad384={mode}") as names:
                L.call("dc_conv_wgrad_group", C.byref(d), N, H, W, layers, pa(xs), cin + 16, pa(gys), cout + 8, vptr(ws), wsb, pa(gws), S())
            if mode == 2:
                assert_served(names, ["wgrad384_pw" if k == 1 else "wgrad384_3x3"] + ["wgrad_reduce"] * layers, f"{name} wgrad384=2")
            else:
                assert_served(names, ["wgrad128_bf16", "wgrad_reduce"] * layers, f"{name} wgrad384=0")
            torch.cuda.synchronize()
            for l in range(layers):
                exactly(gws[l].cpu(), cs[l].gw.float(), f"{name} wgrad384={mode} layer {l}")
    finally:
        L.call("dc_reset_options")          # wgrad384 and the case's split overrides, back to the library's table of defaults


@pytest.mark.parametrize("case", CASES["tconv384"], ids=ids("tconv384"))
def test_conv_transpose_wgrad_384_tile_kernel(case):
    name, spec, extra = case
    cin, cout, N, H, W = spec[5:]
    dtype = torch.bfloat16
    d = desc(dtype, 3, 2, 1, 1, 1, cin, cout)
    c = U.conv_case(spec)
    U.preconditions(c, name)
    xb, xv = to_nhwc(c.x, dtype, ld=cin + 16, off=8)
    gb, gyv = to_nhwc(c.gy, dtype, ld=cout + 8)
    lib = L.load()
    try:
        for mode in (2, 0):
            L.call("dc_set_option", b"wgrad384", mode)
            for kk, v in extra["opts"].items():
                L.call("dc_set_option", kk.encode(), v)
            wsb = lib.dc_conv_wgrad_workspace(C.byref(d), N, H, W)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev())
            gw = torch.full(c.wshape, NAN, device=dev())
            with served(f"wgrad384={mode}") as names:
                L.call("dc_conv_wgrad", C.byref(d), N, H, W, vptr(xv), cin + 16, vptr(gyv), cout + 8, vptr(ws), wsb, vptr(gw), S())
            assert_served(names, ["wgrad384_convT" if mode == 2 else "wgrad128_bf16", "wgrad_reduce"], f"{name} wgrad384={mode}")
            torch.cuda.synchronize()
            exactly(gw.cpu(), c.gw.float(), f"{name} wgrad384={mode}")
    finally:
        L.call("dc_reset_options")


FOLD_PARAMS = [pytest.param(c, dt, id=f"{c[0]}-{'f32' if dt == torch.float32 else 'bf16'}") for c in CASES["fold"] for dt in DTYPES
               if not (dt == torch.float32 and c[2]["layers"] > 1)]       # the grouped launch is bf16 only


@pytest.mark.parametrize("case,dtype", FOLD_PARAMS)
def test_conv_wgrad_partial_and_fold(case, dtype):
    """dc_conv_wgrad_partial + dc_fold_slabs, a depthwise layer's (integer) rows riding in the same fold: equal to autograd / to the sum."""
    name, spec, extra = case
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    layers = extra["layers"]
    d = desc(dtype, k, stride, pad, dil, tr, cin, cout)
    cs, xs, gys, keep = layer_views(spec, layers, dtype)
    wshape = cs[0].wshape
    Cd, rows = 72, 37
    wslab = U.ints((rows, 9, Cd), 7, -3, 3)
    dgot = torch.full((Cd, 1, 3, 3), NAN, device=dev())
    wslab_d = wslab.to(dev())
    splits, sbytes = C.c_int(), C.c_size_t()
    L.call("dc_conv_wgrad_plan", C.byref(d), N, H, W, layers, C.byref(splits), C.byref(sbytes))
    assert sbytes.value == splits.value * wshape[0] * wshape[1] * wshape[2] * wshape[3] * 4
    slabs = [torch.full((sbytes.value // 4,), NAN, device=dev()) for _ in range(layers)]
    got = [torch.full(wshape, NAN, device=dev()) for _ in range(layers)]
    L.call("dc_conv_wgrad_partial", C.byref(d), N, H, W, layers, pa(xs), cin + 16, pa(gys), cout, pa(slabs), splits.value, S())
    kind = L.DC_FOLD_CONVT if tr else L.DC_FOLD_CONV
    ents = [L.FoldEntry(wslab_d.data_ptr(), dgot.data_ptr(), L.DC_FOLD_DW, rows, 9, Cd, 1)]
    ents += [L.FoldEntry(slabs[l].data_ptr(), got[l].data_ptr(), kind, splits.value, wshape[2] * wshape[3], cout, cin) for l in range(layers)]
    L.call("dc_fold_slabs", (L.FoldEntry * len(ents))(*ents), len(ents), S())
    torch.cuda.synchronize()
    for l in range(layers):
        exactly(got[l].cpu(), cs[l].gw.float(), f"{name} layer {l}")
    exactly(dgot.cpu().view(Cd, 9), wslab.double().sum(0).t().float().contiguous(), "depthwise rows")


# ------------------------------------------------------------------------------------------------------------------ depthwise
def dw_pack(c, Cc):
    wd = torch.empty(9 * Cc, device=dev())
    L.call("dc_dwconv_pack_weights", Cc, vptr(c.w.float().to(dev())), vptr(wd), S())
    return wd


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES["dw"], ids=ids("dw"))
def test_depthwise(case, dtype):
    """Forward (plain and through the BatchNorm prologue with power-of-two scales, prelu 0 and 1), data gradient (plain and onto an
    addend), weight gradient (plain and through the prologue), and dc_dwconv_dgrad_wgrad + dc_dwconv_wgrad_reduce.  The pipe* cases run
    their bf16 data gradients on dwpipe.hip under the default planner, as test_kernels_gpu.test_depthwise pins."""
    name, spec, _ = case
    Cc, stride, dil, N, H, W = spec
    c = U.dw_case(spec)
    U.preconditions(c, name)
    expect = {}
    if name.startswith("pipe"):
        dg = "dwpipe_dgrad" if dtype == torch.bfloat16 else "dw_tile_dgrad"
        expect = dict(dgrad=dg, dgrad_add=dg, dgrad_wgrad=[dg, "dw_tile_reduce"])
    dt, lib = L.dtype_code(dtype), L.load()
    Ho, Wo = c.y.shape[2:]
    wd = dw_pack(c, Cc)
    sc, sh = c.scale.float().to(dev()), c.shift.float().to(dev())
    _, xv = to_nhwc(c.x, dtype, ld=Cc + 8)
    _, x0 = to_nhwc(c.x, dtype)
    _, gyv = to_nhwc(c.gy, dtype)
    _, addv = to_nhwc(c.add, dtype)
    _, yv = empty_nhwc(N, Ho, Wo, Cc, dtype)
    L.call("dc_dwconv_fwd", dt, Cc, stride, dil, N, H, W, vptr(xv), Cc + 8, vptr(wd), vptr(yv), Cc, None, None, 0, S())
    torch.cuda.synchronize()
    exactly(from_nhwc(yv), cast(c.y, dtype), f"{name} fwd")
    wsb = lib.dc_dwconv_wgrad_workspace(Cc, N, H, W, stride)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev())
    for prelu in (0, 1):
        _, ov = empty_nhwc(N, Ho, Wo, Cc, dtype)
        L.call("dc_dwconv_fwd", dt, Cc, stride, dil, N, H, W, vptr(x0), Cc, vptr(wd), vptr(ov), Cc, vptr(sc), vptr(sh), prelu, S())
        gwp = torch.full((Cc, 1, 3, 3), NAN, device=dev())
        L.call("dc_dwconv_wgrad", dt, Cc, stride, dil, N, H, W, vptr(x0), Cc, vptr(gyv), Cc, vptr(ws), vptr(gwp), vptr(sc), vptr(sh), prelu, S())
        torch.cuda.synchronize()
        exactly(from_nhwc(ov), cast(c.pro[prelu].y, dtype), f"{name} fwd through the prologue, prelu={prelu}")
        exactly(gwp.cpu(), c.pro[prelu].gw.float(), f"{name} wgrad through the prologue, prelu={prelu}")
    _, gxv = empty_nhwc(N, H, W, Cc, dtype)
    with served("dgrad") as names:
        L.call("dc_dwconv_dgrad", dt, Cc, stride, dil, N, H, W, vptr(gyv), Cc, vptr(wd), None, 0, vptr(gxv), Cc, S())
    check_served(names, expect.get("dgrad"), f"{name} dgrad")
    torch.cuda.synchronize()
    exactly(from_nhwc(gxv), cast(c.gx, dtype), f"{name} dgrad")
    with served("dgrad_add") as names:
        L.call("dc_dwconv_dgrad", dt, Cc, stride, dil, N, H, W, vptr(gyv), Cc, vptr(wd), vptr(addv), Cc, vptr(gxv), Cc, S())
    check_served(names, expect.get("dgrad_add"), f"{name} dgrad_add")
    torch.cuda.synchronize()
    exactly(from_nhwc(gxv), cast(c.gx + c.add, dtype), f"{name} dgrad onto an addend")
    gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
    L.call("dc_dwconv_wgrad", dt, Cc, stride, dil, N, H, W, vptr(xv), Cc + 8, vptr(gyv), Cc, vptr(ws), vptr(gw), None, None, 0, S())
    torch.cuda.synchronize()
    exactly(gw.cpu(), c.gw.float(), f"{name} wgrad")
    rows = lib.dc_dwconv_dgrad_wgrad_rows(dt, Cc, stride, dil, N, H, W)
    assert rows > 0
    _, gxv2 = empty_nhwc(N, H, W, Cc, dtype)
    wslab = torch.full((rows, 9, Cc), NAN, device=dev())
    gw2 = torch.full((Cc, 1, 3, 3), NAN, device=dev())
    with served("dgrad_wgrad") as names:
        L.call("dc_dwconv_dgrad_wgrad", dt, Cc, stride, dil, N, H, W, vptr(gyv), Cc, vptr(wd), vptr(addv), Cc, vptr(gxv2), Cc, vptr(xv), Cc + 8,
               None, None, 0, vptr(wslab), S())
        L.call("dc_dwconv_wgrad_reduce", Cc, rows, vptr(wslab), vptr(gw2), S())
    check_served(names, expect.get("dgrad_wgrad"), f"{name} dgrad_wgrad")
    torch.cuda.synchronize()
    exactly(from_nhwc(gxv2), cast(c.gx + c.add, dtype), f"{name} dgrad_wgrad: dx")
    exactly(gw2.cpu(), c.gw.float(), f"{name} dgrad_wgrad: weight gradient after its fold")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES["dw"], ids=ids("dw"))
def test_depthwise_dgrad_riders(case, dtype):
    """dc_dwconv_dgrad_bnstats and dc_dwconv_dgrad_bnstats_wgrad + dc_dwconv_wgrad_reduce (second tier: BnAcc::add is mask, add, fma): dx,
    the BatchNorm-backward sums and the weight gradient through act(y * scale + shift), each equal to the reference."""
    name, spec, _ = case
    Cc, stride, dil, N, H, W = spec
    c = U.dw_case(spec)
    U.preconditions(c, name)
    r = U.dw_rider(c)
    dt, lib = L.dtype_code(dtype), L.load()
    wd = dw_pack(c, Cc)
    mean, invstd, sc, sh = rider_vectors(r)
    _, yv = to_nhwc(c.x, dtype, ld=Cc + 8)
    _, gyv = to_nhwc(c.gy, dtype)
    srows = lib.dc_dwconv_dgrad_bnstats_rows(dt, Cc, stride, dil, N, H, W)
    wrows = lib.dc_dwconv_dgrad_wgrad_rows(dt, Cc, stride, dil, N, H, W)
    assert srows > 0 and wrows > 0
    for relu in (1, 0):
        what = f"{name} relu={relu}"
        _, dx1 = empty_nhwc(N, H, W, Cc, dtype)
        slab1 = torch.full((2, srows, Cc), NAN, device=dev())
        L.call("dc_dwconv_dgrad_bnstats", dt, Cc, stride, dil, N, H, W, vptr(gyv), Cc, vptr(wd), vptr(dx1), Cc, vptr(yv), Cc + 8, vptr(mean),
               vptr(invstd), vptr(sc), vptr(sh), relu, vptr(slab1), S())
        _, dx2 = empty_nhwc(N, H, W, Cc, dtype)
        slab2 = torch.full((2, srows, Cc), NAN, device=dev())
        wslab = torch.full((wrows, 9, Cc), NAN, device=dev())
        gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
        L.call("dc_dwconv_dgrad_bnstats_wgrad", dt, Cc, stride, dil, N, H, W, vptr(gyv), Cc, vptr(wd), vptr(dx2), Cc, vptr(yv), Cc + 8, vptr(mean),
               vptr(invstd), vptr(sc), vptr(sh), relu, vptr(slab2), vptr(wslab), S())
        L.call("dc_dwconv_wgrad_reduce", Cc, wrows, vptr(wslab), vptr(gw), S())
        torch.cuda.synchronize()
        for tag, dx, slab in (("bnstats", dx1, slab1), ("bnstats_wgrad", dx2, slab2)):
            exactly(from_nhwc(dx), cast(c.gx, dtype), f"{what} {tag}: dx")
            check_rider_slab(slab, c.gx, r, relu, f"{what} {tag}")
        exactly(gw.cpu(), c.pro[relu].gw.float(), f"{what}: weight gradient after its fold")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["dw_pipe0", "dw_pipe1", "dw_pipe2"])
@pytest.mark.parametrize("case", CASES["dwpipe"], ids=ids("dwpipe"))
def test_depthwise_pipelined_kernel(case, mode):
    """dwpipe.hip (dw_pipe = 2: forward and data gradients; 1, the default: data gradients) and dwtile.hip (0) on the entry points of
    test_depthwise_pipelined_kernel_matches_tiled that carry no BatchNorm-backward sums: outputs equal to the reference, weight gradients
    equal after their fold, where that test allows the rounding of a different summation order."""
    name, spec, _ = case
    Cc, stride, dil, N, H, W = spec
    c = U.dw_case(spec)
    U.preconditions(c, name)
    dt, dtype = L.DC_BF16, torch.bfloat16
    lib = L.load()
    wd = dw_pack(c, Cc)
    r = U.dw_rider(c)
    mean, invstd, sc, sh = rider_vectors(r)
    ld = (Cc + 31) // 32 * 32
    _, xv = to_nhwc(c.x, dtype, ld=ld)
    _, gyv = to_nhwc(c.gy, dtype, ld=ld)
    _, addv = to_nhwc(c.add, dtype)
    out = {}
    L.call("dc_set_option", b"dw_pipe", mode)
    try:
        with served(f"dw_pipe={mode}") as names:
            for prelu, tag in ((None, "fwd"), (1, "fwd_bn_relu"), (0, "fwd_bn")):
                _, yv = empty_nhwc(N, H, W, Cc, dtype)
                L.call("dc_dwconv_fwd", dt, Cc, 1, dil, N, H, W, vptr(xv), ld, vptr(wd), vptr(yv), Cc, vptr(sc) if prelu is not None else None,
                       vptr(sh) if prelu is not None else None, prelu or 0, S())
                out[tag] = yv
            _, g1 = empty_nhwc(N, H, W, Cc, dtype)
            L.call("dc_dwconv_dgrad", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), None, 0, vptr(g1), Cc, S())
            _, g2 = empty_nhwc(N, H, W, Cc, dtype)
            L.call("dc_dwconv_dgrad", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), vptr(addv), Cc, vptr(g2), Cc, S())
            out["dgrad"], out["dgrad_add"] = g1, g2
            wrows = lib.dc_dwconv_dgrad_wgrad_rows(dt, Cc, 1, dil, N, H, W)
            rows = lib.dc_dwconv_dgrad_bnstats_rows(dt, Cc, 1, dil, N, H, W)
            assert wrows > 0 and rows > 0
            for relu in (1, 0):                      # second tier: the BatchNorm-backward sums ride on the data gradient
                _, g3 = empty_nhwc(N, H, W, Cc, dtype)
                slab = torch.full((2, rows, Cc), NAN, device=dev())
                L.call("dc_dwconv_dgrad_bnstats", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), vptr(g3), Cc, vptr(xv), ld, vptr(mean), vptr(invstd),
                       vptr(sc), vptr(sh), relu, vptr(slab), S())
                _, g4 = empty_nhwc(N, H, W, Cc, dtype)
                slab2 = torch.full((2, rows, Cc), NAN, device=dev())
                wslab = torch.full((wrows, 9, Cc), NAN, device=dev())
                gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
                L.call("dc_dwconv_dgrad_bnstats_wgrad", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), vptr(g4), Cc, vptr(xv), ld, vptr(mean),
                       vptr(invstd), vptr(sc), vptr(sh), relu, vptr(slab2), vptr(wslab), S())
                L.call("dc_dwconv_wgrad_reduce", Cc, wrows, vptr(wslab), vptr(gw), S())
                _, g6 = empty_nhwc(N, H, W, Cc, dtype)
                slab3 = torch.full((2, rows, Cc), NAN, device=dev())
                wslab3 = torch.full((wrows, 9, Cc), NAN, device=dev())
                gw3 = torch.full((Cc, 1, 3, 3), NAN, device=dev())
                L.call("dc_dwconv_dgrad_bnstats_wgrad_add", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), vptr(addv), Cc, vptr(g6), Cc, vptr(xv), ld,
                       vptr(mean), vptr(invstd), vptr(sc), vptr(sh), relu, vptr(slab3), vptr(wslab3), S())
                L.call("dc_dwconv_wgrad_reduce", Cc, wrows, vptr(wslab3), vptr(gw3), S())
                out[f"riders{relu}"] = ((g3, slab, None), (g4, slab2, gw), (g6, slab3, gw3))
            for aff in (0, 1):
                _, g5 = empty_nhwc(N, H, W, Cc, dtype)
                wslab = torch.full((wrows, 9, Cc), NAN, device=dev())
                gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
                L.call("dc_dwconv_dgrad_wgrad", dt, Cc, 1, dil, N, H, W, vptr(gyv), ld, vptr(wd), vptr(addv), Cc, vptr(g5), Cc, vptr(xv), ld,
                       vptr(sc) if aff else None, vptr(sh) if aff else None, aff, vptr(wslab), S())
                L.call("dc_dwconv_wgrad_reduce", Cc, wrows, vptr(wslab), vptr(gw), S())
                out[f"dx{aff}"], out[f"gw{aff}"] = g5, gw
    finally:
        L.call("dc_set_option", b"dw_pipe", 1)
    dw = [n for n in names if n not in ("aux", "dw_tile_reduce")]
    fwd, dgrad = ("dwpipe_fwd" if mode == 2 else "dw_tile_fwd"), ("dwpipe_dgrad" if mode else "dw_tile_dgrad")
    assert dw == [fwd] * 3 + [dgrad] * 10, f"dw_pipe={mode}: served by {dw}"
    torch.cuda.synchronize()
    exactly(from_nhwc(out["fwd"]), cast(c.y, dtype), "fwd")
    exactly(from_nhwc(out["fwd_bn_relu"]), cast(c.pro[1].y, dtype), "fwd through BatchNorm + ReLU")
    exactly(from_nhwc(out["fwd_bn"]), cast(c.pro[0].y, dtype), "fwd through BatchNorm")
    exactly(from_nhwc(out["dgrad"]), cast(c.gx, dtype), "dgrad")
    exactly(from_nhwc(out["dgrad_add"]), cast(c.gx + c.add, dtype), "dgrad onto an addend")
    for relu in (1, 0):
        for i, (dx, slab, gw) in enumerate(out[f"riders{relu}"]):
            g = c.gx + c.add if i == 2 else c.gx             # the _add form: dx is the accumulated gradient, the sums are those of it
            what = f"relu={relu} " + ("bnstats", "bnstats_wgrad", "bnstats_wgrad_add")[i]
            exactly(from_nhwc(dx), cast(g, dtype), f"{what}: dx")
            check_rider_slab(slab, g, r, relu, what)
            if gw is not None:
                exactly(gw.cpu(), c.pro[relu].gw.float(), f"{what}: weight gradient after its fold")
    for aff in (0, 1):
        exactly(from_nhwc(out[f"dx{aff}"]), cast(c.gx + c.add, dtype), f"dgrad_wgrad prologue={aff}: dx")
        exactly(out[f"gw{aff}"].cpu(), (c.pro[1].gw if aff else c.gw).float(), f"dgrad_wgrad prologue={aff}: weight gradient after its fold")


RES_CASES = [c for c in CASES["dwpipe"] if c[1][2] == 1]                 # the residual form is built for dilation 1
SUM_ROW_RELU1 = ("728", "64_half_block")                                  # where test_kernels_gpu.py launches the residual sum row unmasked


def sum_row(Cc):
    """A zeroed double[2][C] sum row with a poisoned tail."""
    row = torch.zeros(2 * Cc + 4, dtype=torch.float64, device=dev())
    row[2 * Cc:] = NAN
    return row


def check_sum_row(row, Cc, g, r, relu, what, mask=None):
    assert bool(torch.isnan(row[2 * Cc:]).all()), f"{what}: wrote behind its sum row"
    got = row[:2 * Cc].view(2, Cc).cpu()
    want0, want1 = U.bn_bwd_sums(g, r, relu, what, mask=mask)
    exactly(got[0], want0, f"{what}: sum g")
    exactly(got[1], want1, f"{what}: sum g * xhat")


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("case", RES_CASES, ids=[c[0] for c in RES_CASES])
def test_depthwise_dgrad_residual_batchnorm_sums(case, with_addend):
    """dc_dwconv_dgrad_wgrad_bnres and dc_dwconv_dgrad_wgrad_bnres_sum (second tier: dwpipe.hip takes gm = masked(x > 0, stored dx),
    a += gm, b = fma(gm, (ybn - mean) * invstd, b); the sum row is fp64 atomics of those fp32 sums).  The stored input is
    x = relu(bn(ybn) + residual) on integer data; relu = 0 and 1, and 2 (dx stored masked, kernel family dwpipe_dgrad_masked) where
    dc_dwconv_dgrad_wgrad_bnres_masked serves.  dx, the sums (row slab after its fold, or the sum row) and the weight gradient after its fold
    equal the reference."""
    name, spec, _ = case
    Cc, stride, dil, N, H, W = spec
    c = U.dw_case(spec)
    U.preconditions(c, name)
    r = U.dw_rider(c)
    xo, gw_ref = U.res_input(c)
    pos = xo > 0
    dt, dtype, lib = L.DC_BF16, torch.bfloat16, L.load()
    rows = lib.dc_dwconv_dgrad_wgrad_bnres_rows(dt, Cc, 1, dil, N, H, W)
    assert rows > 0 and rows == lib.dc_dwconv_dgrad_wgrad_rows(dt, Cc, 1, dil, N, H, W)
    assert lib.dc_dwconv_dgrad_sum_row_ok(dt, Cc, 1, dil, N, H, W) == 1
    masked = lib.dc_dwconv_dgrad_wgrad_bnres_masked(dt, Cc, 1, dil, N, H, W) == 1
    wd = dw_pack(c, Cc)
    mean, invstd, _, _ = rider_vectors(r)
    ld = (Cc + 31) // 32 * 32
    _, xv = to_nhwc(xo, dtype, ld=ld)
    _, yv = to_nhwc(c.x, dtype, ld=ld)
    _, gyv = to_nhwc(c.gy, dtype)
    g_full = c.gx + c.add if with_addend else c.gx
    for relu in (0, 1, 2) if masked else (0, 1):
        for summed in (False, True):
            if summed and not (relu == 2 or (relu == 1 and name in SUM_ROW_RELU1)):
                continue
            what = f"{name} relu={relu} {'sum row' if summed else 'row slab'}"
            _, dx = to_nhwc(c.add, dtype)                        # dx starts as the other consumers' contribution
            ap, al = (vptr(dx), Cc) if with_addend else (None, 0)
            wslab = torch.full((rows, 9, Cc), NAN, device=dev())
            slab = sum_row(Cc) if summed else torch.full((2, rows, Cc), NAN, device=dev())
            with served(what) as names:
                L.call("dc_dwconv_dgrad_wgrad_bnres_sum" if summed else "dc_dwconv_dgrad_wgrad_bnres", dt, Cc, 1, dil, N, H, W, vptr(gyv), Cc, vptr(wd),
                       ap, al, vptr(dx), Cc, vptr(xv), ld, vptr(wslab), vptr(yv), ld, vptr(mean), vptr(invstd), relu, vptr(slab), S())
            assert_served(names, "dwpipe_dgrad_masked" if relu == 2 else "dwpipe_dgrad", what)
            gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
            L.call("dc_dwconv_wgrad_reduce", Cc, rows, vptr(wslab), vptr(gw), S())
            torch.cuda.synchronize()
            exactly(from_nhwc(dx), cast(g_full * pos if relu == 2 else g_full, dtype), f"{what}: dx")
            if summed:
                check_sum_row(slab, Cc, g_full, r, relu, what, mask=pos)
            else:
                s0, s1 = column_sums(slab)
                want0, want1 = U.bn_bwd_sums(g_full, r, relu, what, mask=pos)
                exactly(s0, want0, f"{what}: sum g")
                exactly(s1, want1, f"{what}: sum g * xhat")
            exactly(gw.cpu(), gw_ref.float(), f"{what}: weight gradient after its fold")


SUM_CASES = [c for c in CASES["dwpipe"] if c[0] in ("728", "1024d2", "64_half_block")]


@pytest.mark.parametrize("case", SUM_CASES, ids=[c[0] for c in SUM_CASES])
def test_depthwise_dgrad_batchnorm_sums_into_a_sum_row(case):
    """dc_dwconv_dgrad_bnstats_wgrad_sum: dx, the double[2][C] sum row and the weight gradient after its fold equal the reference."""
    name, spec, _ = case
    Cc, stride, dil, N, H, W = spec
    c = U.dw_case(spec)
    U.preconditions(c, name)
    r = U.dw_rider(c)
    dt, dtype, lib = L.DC_BF16, torch.bfloat16, L.load()
    assert lib.dc_dwconv_dgrad_sum_row_ok(dt, Cc, 1, dil, N, H, W) == 1
    rows = lib.dc_dwconv_dgrad_wgrad_rows(dt, Cc, 1, dil, N, H, W)
    assert rows > 0
    wd = dw_pack(c, Cc)
    mean, invstd, sc, sh = rider_vectors(r)
    ld = (Cc + 31) // 32 * 32
    _, yv = to_nhwc(c.x, dtype, ld=ld)
    _, gyv = to_nhwc(c.gy, dtype)
    _, dx = empty_nhwc(N, H, W, Cc, dtype)
    wslab = torch.full((rows, 9, Cc), NAN, device=dev())
    row = sum_row(Cc)
    with served("bnstats_wgrad_sum") as names:
        L.call("dc_dwconv_dgrad_bnstats_wgrad_sum", dt, Cc, 1, dil, N, H, W, vptr(gyv), Cc, vptr(wd), vptr(dx), Cc, vptr(yv), ld, vptr(mean),
               vptr(invstd), vptr(sc), vptr(sh), 1, vptr(row), vptr(wslab), S())
    assert_served(names, "dwpipe_dgrad", name)
    gw = torch.full((Cc, 1, 3, 3), NAN, device=dev())
    L.call("dc_dwconv_wgrad_reduce", Cc, rows, vptr(wslab), vptr(gw), S())
    torch.cuda.synchronize()
    exactly(from_nhwc(dx), cast(c.gx, dtype), f"{name}: dx")
    check_sum_row(row, Cc, c.gx, r, 1, name)
    exactly(gw.cpu(), c.pro[1].gw.float(), f"{name}: weight gradient after its fold")


@pytest.mark.parametrize("case", CASES["sepconv"], ids=ids("sepconv"))
def test_separable_conv_forward_as_one_operator(case):
    """dc_sepconv_fwd (second tier: a depthwise and a pointwise K loop and the sums of the stored y; no other operation): the depthwise
    output d, the pointwise output y and the slab's column sums equal the reference; rows the kernel does not own are zeros, pad channels
    untouched; without a slab (eval mode) the same y."""
    name, spec, _ = case
    cin, cout, N, H, W, lazy, relu = spec
    c = U.sep_case(spec)
    U.sep_preconditions(c, name)
    dtype, dt, lib = torch.bfloat16, L.DC_BF16, L.load()
    rows = lib.dc_sepconv_fwd_rows(dt, cin, cout, 1, 1, N, H, W)
    assert rows > 0
    _, xv = to_nhwc(c.x, dtype, ld=cin + 8)
    wd = torch.empty(9 * cin, device=dev())
    L.call("dc_dwconv_pack_weights", cin, vptr(c.wdw.float().to(dev())), vptr(wd), S())
    d = L.ConvDesc(dt, 1, 1, 0, 1, 0, cin, cout)
    nwf, nwb = C.c_size_t(), C.c_size_t()
    L.call("dc_conv_packed_elems", C.byref(d), C.byref(nwf), C.byref(nwb))
    wf = torch.zeros(nwf.value, dtype=dtype, device=dev())
    L.call("dc_conv_pack_weights", C.byref(d), vptr(c.w.float().to(dev())), vptr(wf), None, S())
    sc = c.scale.float().to(dev()) if lazy else None
    sh = c.shift.float().to(dev()) if lazy else None
    rows_ref = lib.dc_conv_stat_rows(C.byref(d), N, H, W)
    db, dv = empty_nhwc(N, H, W, cin, dtype, ld=cin + 16)
    yb, yv = empty_nhwc(N, H, W, cout, dtype, ld=cout + 8)
    slab = torch.full((2, rows_ref, cout), NAN, device=dev())
    L.call("dc_sepconv_fwd", dt, cin, cout, N, H, W, vptr(xv), cin + 8, vptr(sc) if lazy else None, vptr(sh) if lazy else None, relu, vptr(wd),
           vptr(dv), cin + 16, vptr(wf), vptr(yv), cout + 8, vptr(slab), rows_ref, S())
    torch.cuda.synchronize()
    exactly(from_nhwc(dv), cast(c.d, dtype), f"{name}: depthwise output")
    exactly(from_nhwc(yv), cast(c.y, dtype), f"{name}: pointwise output")
    assert all_nan(db[..., cin:]) and all_nan(yb[..., cout:])
    assert bool((slab[:, rows:] == 0).all())
    s, ss = column_sums(slab)
    exactly(s, c.sum_y, f"{name}: sum of y")
    exactly(ss, c.sum_yy, f"{name}: sum of y^2")
    yv.fill_(0)
    L.call("dc_sepconv_fwd", dt, cin, cout, N, H, W, vptr(xv), cin + 8, vptr(sc) if lazy else None, vptr(sh) if lazy else None, relu, vptr(wd),
           vptr(dv), cin + 16, vptr(wf), vptr(yv), cout + 8, None, 0, S())
    torch.cuda.synchronize()
    exactly(from_nhwc(yv), cast(c.y, dtype), f"{name}: pointwise output without statistics")


# ------------------------------------------------------------------------------------------------------------------ reductions
BN_SHAPES = U.params_of(tk.test_batchnorm_train_fwd_bwd, "shape")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=U.ids_of(tk.test_batchnorm_train_fwd_bwd, "shape"))
def test_bn_stats(shape, dtype):
    """dc_bn_stats on integers -4 .. 4: the slab's float64 column sums are the tensor's sum and sum of squares."""
    N, Cc, H, W = shape
    M = N * H * W
    y = U.ints((N, Cc, H, W), 1, -4, 4).double()
    U.need_exact(y, torch.bfloat16, "bn_stats", bound=16 * M)
    _, yv = to_nhwc(y, dtype, ld=Cc + 8)
    rows = L.load().dc_bn_stat_rows(M)
    slab = torch.full((2, rows, Cc), NAN, device=dev())
    L.call("dc_bn_stats", L.dtype_code(dtype), M, Cc, vptr(yv), Cc + 8, vptr(slab), S())
    torch.cuda.synchronize()
    s, ss = column_sums(slab)
    exactly(s, y.sum((0, 2, 3)), "sum")
    exactly(ss, (y * y).sum((0, 2, 3)), "sum of squares")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_pool_branch_reductions(dtype):
    """dc_avgpool_fwd, dc_sum_hw, dc_avgpool_bwd_add and dc_colsum over an 8 x 16 image: 1 / HW = 2^-7, so the mean and the spread
    gradient are exact too."""
    N, Cc, H, W = U.POOL
    HW, dt = H * W, L.dtype_code(dtype)
    x = U.ints((N, Cc, H, W), 1, -4, 4).double()
    g = 128 * U.ints((N, Cc), 2).double()
    U.need_exact(x, torch.bfloat16, "pool input", bound=4 * N * HW)
    U.need_exact(x + g[:, :, None, None] / HW, torch.bfloat16, "avgpool_bwd_add")
    _, xv = to_nhwc(x, dtype)
    pooled = torch.full((N, Cc), NAN, device=dev())
    L.call("dc_avgpool_fwd", dt, N, HW, Cc, vptr(xv), Cc, vptr(pooled), S())
    summed = torch.full((N, Cc), NAN, device=dev())
    L.call("dc_sum_hw", dt, N, HW, Cc, vptr(xv), Cc, vptr(summed), S())
    _, av = to_nhwc(x, dtype)
    gd = g.float().to(dev())
    L.call("dc_avgpool_bwd_add", dt, N, HW, Cc, vptr(gd), vptr(av), Cc, S())
    ws = torch.empty(L.load().dc_colsum_workspace(N * HW, Cc), dtype=torch.uint8, device=dev())
    col = torch.full((Cc,), NAN, device=dev())
    L.call("dc_colsum", dt, N * HW, Cc, vptr(xv), Cc, vptr(col), vptr(ws), S())
    torch.cuda.synchronize()
    exactly(pooled.cpu(), x.mean((2, 3)).float(), "avgpool_fwd")
    exactly(summed.cpu(), x.sum((2, 3)).float(), "sum_hw")
    exactly(from_nhwc(av), cast(x + g[:, :, None, None] / HW, dtype), "avgpool_bwd_add")
    exactly(col.cpu(), x.sum((0, 2, 3)).float(), "colsum")


# ------------------------------------------------------------------------------------------------------------------ stem and head
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_stem(dtype):
    """dc_stem_fwd with its slab, dc_stem_wgrad and dc_stem_dgrad at the shape of test_stem (NCHW fp32 input and input gradient)."""
    N, Cin, H, W = U.STEM
    c = U.stem_case()
    U.preconditions(c, "stem")
    dt, lib = L.dtype_code(dtype), L.load()
    Ho, Wo = c.y.shape[2:]
    xd, wd = c.x.float().to(dev()), c.w.float().to(dev())
    _, yv = empty_nhwc(N, Ho, Wo, 32, dtype)
    slab = torch.full((2, lib.dc_stem_stat_rows(N, H, W), 32), NAN, device=dev())
    L.call("dc_stem_fwd", dt, N, Cin, H, W, vptr(xd), vptr(wd), vptr(yv), 32, vptr(slab), S())
    torch.cuda.synchronize()
    exactly(from_nhwc(yv), cast(c.y, dtype), "stem fwd")
    s, ss = column_sums(slab)
    exactly(s, c.sum_y, "stem: sum of y")
    exactly(ss, c.sum_yy, "stem: sum of y^2")
    _, gyv = to_nhwc(c.gy, dtype)
    ws = torch.empty(lib.dc_stem_wgrad_workspace(N, Cin, H, W), dtype=torch.uint8, device=dev())
    gw = torch.full((32, Cin, 3, 3), NAN, device=dev())
    L.call("dc_stem_wgrad", dt, N, Cin, H, W, vptr(xd), vptr(gyv), 32, vptr(ws), vptr(gw), S())
    _, gyp = to_nhwc(c.gy, dtype, ld=40)
    dx = torch.full((N, Cin, H, W), NAN, device=dev())
    L.call("dc_stem_dgrad", dt, N, Cin, H, W, vptr(gyp), 40, vptr(wd), vptr(dx), S())
    torch.cuda.synchronize()
    exactly(gw.cpu(), c.gw.float(), "stem wgrad")
    exactly(dx.cpu(), c.gx.float(), "stem dgrad")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_head(dtype):
    """dc_head_fwd / dc_head_bwd at the shape of test_head with dense +-1 weights: fp32 logits (sums of up to 1 024 terms), the data
    gradient in the storage type, the fp32 weight gradient."""
    N, Cin, H, W = U.HEAD
    c = U.head_case()
    U.head_preconditions(c)
    dt = L.dtype_code(dtype)
    _, xv = to_nhwc(c.x, dtype, ld=Cin + 8)
    wd = c.w.float().to(dev())
    ws = torch.empty(L.load().dc_head_workspace(dt, N, Cin, H, W) + 256, dtype=torch.uint8, device=dev())
    wsp = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    out = torch.full((N, 3, 2 * H, 2 * W), NAN, device=dev())
    L.call("dc_head_fwd", dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(wd), vptr(out), wsp, S())
    torch.cuda.synchronize()
    exactly(out.cpu(), c.y.float(), "head logits")
    gld = c.gy.float().to(dev())
    _, gxv = empty_nhwc(N, H, W, Cin, dtype)
    gw = torch.full((Cin, 3, 3, 3), NAN, device=dev())
    L.call("dc_head_bwd", dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(gld), vptr(wd), vptr(gxv), Cin, vptr(gw), wsp, S())
    torch.cuda.synchronize()
    exactly(from_nhwc(gxv), cast(c.gx, dtype), "head dgrad")
    exactly(gw.cpu(), c.gw.float(), "head wgrad")
    # dc_head_bwd_bnstats (second tier: the streaming kernel and the tiled epilogue take gm = mask ? g : 0, s0 += gm,
    # s1 = fma(gm, (y - mean) * invstd, s1)): the sums of the BatchNorm in front of the head, on both data-gradient kernels in bf16
    r = U.bn_rider((N, Cin, H, W))
    _, ybv = to_nhwc(r.y, dtype)
    mean, invstd, ms, mh = rider_vectors(r)
    rows = (N * H * W + 127) // 128
    try:
        for fused in (1, 0) if dtype == torch.bfloat16 else (1,):
            L.call("dc_set_option", b"head_dgrad_fused", fused)
            what = f"head_dgrad_fused={fused} dc_head_bwd_bnstats"
            slab = torch.full((2, rows, Cin), NAN, device=dev())
            _, gxv2 = empty_nhwc(N, H, W, Cin, dtype)
            gw2 = torch.full((Cin, 3, 3, 3), NAN, device=dev())
            with served(what) as names:
                L.call("dc_head_bwd_bnstats", dt, N, Cin, H, W, vptr(xv), Cin + 8, vptr(gld), vptr(wd), vptr(gxv2), Cin, vptr(gw2), wsp, vptr(ybv), Cin,
                       vptr(mean), vptr(invstd), vptr(ms), vptr(mh), 1, vptr(slab), S())
            if dtype == torch.float32:
                assert names[-1] == "igemm128_f32", names
            elif fused:
                assert names[-1] == "head_dgrad_stream", names
            else:
                assert names[-1] in PLAIN_GEMM and "head_dgrad_stream" not in names, names
            torch.cuda.synchronize()
            exactly(from_nhwc(gxv2), cast(c.gx, dtype), f"{what}: dx")
            exactly(gw2.cpu(), c.gw.float(), f"{what}: weight gradient")
            check_rider_slab(slab, c.gx, r, 1, what)
    finally:
        L.call("dc_set_option", b"head_dgrad_fused", 1)
