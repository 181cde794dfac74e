"""Exactly representable test data for the kernel tests (test_exact_cpu.py, test_exact_gpu.py, test_exact_ends_gpu.py): generators, float64 references and the
preconditions under which a correct kernel must reproduce the reference BIT FOR BIT.

On small-integer data every product, every partial sum in any order or split, and every stored value of a convolution is exactly
representable: fp32 holds every integer below 2^24, bf16 every integer up to 256.  A kernel that accumulates in fp32 and stores fp32 or bf16
therefore has no rounding to hide behind, whatever its tiling, K order, split-K plan or slab layout, and a single lost or doubled element
anywhere shows as an inequality.

preconditions() proves, from the reference alone, that the data of a case are of that kind.  The operator is applied to the ABSOLUTE values
of its operands: by the triangle inequality that bounds every partial sum a kernel can form, in any order and under any grouping.  A raised
NotExact is a mistake in a test's construction, never a kernel failure.

Host-only: nothing here touches a GPU or loads the library (gpu_cases() imports test_kernels_gpu for its tables: see the note there)."""
import functools
import types

import torch
import torch.nn.functional as F

F32_EXACT = 2 ** 24          # every integer of smaller magnitude is an fp32 value; so is every partial sum below it
BF16_EXACT = 256             # ... a bf16 value (8 significant bits)
BUDGET = 24                  # expected number of non-zero weights per output (and per input) of a GEMM convolution


class NotExact(ValueError):
    """The data of a case do not make its comparison exact."""


# ------------------------------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed, lo=-1, hi=1):
    """fp32, uniform on the integers lo .. hi: activations and output gradients ({-1, 0, 1}), biases (-4 .. 4), shifts (-3 .. 3)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


def signs(shape, seed, fan, budget=BUDGET):
    """fp32, +-1 with probability min(1, budget / fan) and 0 otherwise: the weights of a GEMM convolution with fan = k^2 * max(cin, cout), so
    that the forward sums (over k^2 * cin) and the data-gradient sums (over k^2 * cout) both stay small.  fan <= budget: dense +-1."""
    g = _gen(seed)
    s = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    keep = torch.rand(tuple(shape), generator=g) < min(1.0, budget / fan)
    return s * keep


def dw_weights(C, seed):
    """Depthwise 3 x 3 weights [C][1][3][3]: dense +-1."""
    return signs((C, 1, 3, 3), seed, fan=1)


def bias(C, seed):
    return ints((C,), seed, -4, 4)


def bn_prologue(C, seed):
    """BatchNorm prologue coefficients (applied on load as act(x * scale + shift)): scale in {+-1/2, +-1, +-2}, shift an integer in -3 .. 3."""
    table = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
    return table[torch.randint(0, 6, (C,), generator=_gen(seed))], ints((C,), seed + 1000, -3, 3)


def bn_moments(C, seed):
    """For BatchNorm-backward riders: mean an integer in -2 .. 2, invstd a power of two in {1/2, 1, 2}; xhat = (y - mean) * invstd is exact."""
    return ints((C,), seed, -2, 2), 2.0 ** ints((C,), seed + 1000, -1, 1)


# ------------------------------------------------------------------------------------------------------------------ references
def conv_ref(x, w, b, k, stride, pad, dil, transposed):
    """The operators of test_kernels_gpu.py, at whatever dtype the operands have (float64 here)."""
    if transposed:
        return F.conv_transpose2d(x, w, b, 2, 1, 1)
    return F.conv2d(x, w, b, stride, pad, dil)


def dw_ref(x, w, stride, dil):
    C = x.shape[1]
    return F.conv2d(F.pad(x, (dil, dil, dil, dil)), w, None, stride, 0, dil, groups=C)


def _fwd_and_grads(op, x, w, gy):
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = op(xr, wr)
    if gy is None:
        return y.detach(), None, None
    gx, gw = torch.autograd.grad(y, (xr, wr), gy)
    return y.detach(), gx, gw


def stats(y):
    """Per-channel sum and sum of squares of an NCHW float64 tensor."""
    return y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def bf16_holds(t):
    """Every element of t is a bf16 value."""
    return bool(torch.equal(t.to(torch.bfloat16).to(t.dtype), t))


def f32_holds(t):
    return bool(torch.equal(t.float().to(t.dtype), t))


@functools.lru_cache(maxsize=8)
def conv_case(spec, seeds=(1, 2, 3, 5), budget=BUDGET):
    """spec = (k, stride, pad, dil, transposed, cin, cout, N, H, W), the columns of CONV_CASES behind the name.  Returns the float64 data
    (x, w, gy, bias), the float64 reference (y, gx, gw, sum_y, sum_yy) and `bound`, the same operator on absolute values.  Cached: the
    fp32 and the bf16 test of a case share one reference, which nobody may write to."""
    k, stride, pad, dil, tr, cin, cout, N, H, W = spec
    kk = 3 if tr else k
    wshape = (cin, cout, kk, kk) if tr else (cout, cin, kk, kk)
    x = ints((N, cin, H, W), seeds[0]).double()
    w = signs(wshape, seeds[1], fan=kk * kk * max(cin, cout), budget=budget).double()
    op = lambda a, b: conv_ref(a, b, None, k, stride, pad, dil, tr)  # noqa: E731
    with torch.no_grad():
        oshape = op(x[:1, :, :, :], w).shape
    gy = ints((N,) + tuple(oshape[1:]), seeds[2]).double()
    y, gx, gw = _fwd_and_grads(op, x, w, gy)
    ya, gxa, gwa = _fwd_and_grads(op, x.abs(), w.abs(), gy.abs())
    sy, syy = stats(y)
    c = types.SimpleNamespace(spec=spec, wshape=wshape, x=x, w=w, gy=gy, bias=bias(cout, seeds[3]).double(), y=y, gx=gx, gw=gw, sum_y=sy,
                              sum_yy=syy)
    c.bound = dict(y=_maxabs(ya), gx=_maxabs(gxa), gw=_maxabs(gwa), sum_y=_maxabs(stats(ya)[0]), sum_yy=_maxabs(stats(ya)[1]),
                   bias=_maxabs(c.bias), nonzero_y=float((y != 0).double().mean()))
    return c


@functools.lru_cache(maxsize=8)
def dw_case(spec, seeds=(1, 2, 3, 4, 6)):
    """spec = (C, stride, dil, N, H, W).  Depthwise 3 x 3 with implicit zero padding of `dil`: x, dense +-1 weights, gy, an addend for the
    data gradient, and prologue coefficients (scale, shift) with the forward / weight gradient through act(x * scale + shift) for act = identity
    (pro[0]) and ReLU (pro[1])."""
    Cc, stride, dil, N, H, W = spec
    x = ints((N, Cc, H, W), seeds[0]).double()
    w = dw_weights(Cc, seeds[1]).double()
    op = lambda a, b: dw_ref(a, b, stride, dil)  # noqa: E731
    with torch.no_grad():
        oshape = op(x[:1], w).shape
    gy = ints((N,) + tuple(oshape[1:]), seeds[2]).double()
    y, gx, gw = _fwd_and_grads(op, x, w, gy)
    ya, gxa, gwa = _fwd_and_grads(op, x.abs(), w.abs(), gy.abs())
    sy, syy = stats(y)
    scale, shift = (t.double() for t in bn_prologue(Cc, seeds[4]))
    c = types.SimpleNamespace(spec=spec, x=x, w=w, gy=gy, add=ints((N, Cc, H, W), seeds[3]).double(), y=y, gx=gx, gw=gw, sum_y=sy, sum_yy=syy,
                              scale=scale, shift=shift, pro=[])
    c.bound = dict(y=_maxabs(ya), gx=_maxabs(gxa) + 1, gw=_maxabs(gwa), sum_y=_maxabs(stats(ya)[0]), sum_yy=_maxabs(stats(ya)[1]))
    for relu in (0, 1):
        a = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if relu:
            a = a.clamp_min(0)
        ay, _, agw = _fwd_and_grads(op, a, w, gy)
        aya, _, agwa = _fwd_and_grads(op, a.abs(), w.abs(), gy.abs())
        c.pro.append(types.SimpleNamespace(a=a, y=ay, gw=agw))
        c.bound[f"a{relu}"], c.bound[f"a{relu}_y"], c.bound[f"a{relu}_gw"] = _maxabs(a), _maxabs(aya), _maxabs(agwa)
    return c


# ------------------------------------------------------------------------------------------------------------------ preconditions
def _need(ok, what, case):
    if not ok:
        raise NotExact(f"{case}: {what}")


def preconditions(c, name="case"):
    """Bounds of a conv_case / dw_case; raises NotExact unless every comparison of the exact tests is free of rounding for a kernel that
    accumulates in fp32 and stores fp32 or bf16:
      - |partial sum| < 2^24 for everything accumulated in fp32: outputs, both gradients, and the per-channel sums of y and y^2 over the whole
        tensor (hence over any grouping of pixels into slab rows);
      - |value| <= 256, and the value itself a bf16 number, for everything stored as bf16: y, 2 y (accumulate mode), y + bias,
        2 y + bias (bias in accumulate mode), gx, 2 gx, gx + addend; the activation of a BatchNorm prologue and its depthwise output (halves).
    The data themselves must be bf16 numbers (they are stored as bf16 before the kernel sees them)."""
    b = c.bound
    for key in ("y", "gx", "gw", "sum_y", "sum_yy"):
        _need(b[key] < F32_EXACT, f"fp32 partial sums of {key} reach {b[key]:.0f} >= 2^24", name)
    stored = 2 * b["y"] + b.get("bias", 0)
    _need(stored <= BF16_EXACT, f"|2 y + bias| can reach {stored:.0f} > 256 (bf16 store)", name)
    _need(2 * b["gx"] <= BF16_EXACT, f"|2 gx| can reach {2 * b['gx']:.0f} > 256 (bf16 store)", name)
    tensors = [c.x, c.w, c.gy, c.y, c.gx]
    tensors += [c.bias] if hasattr(c, "bias") else [c.add, c.scale, c.shift]
    for t in tensors:
        _need(bf16_holds(t), "an operand or a stored result is not a bf16 number", name)
    _need(f32_holds(c.gw), "the weight gradient is not an fp32 number", name)
    for relu, p in enumerate(getattr(c, "pro", [])):
        # halves: 2 a, 2 y are integers, so the same bounds hold for twice the value
        _need(2 * b[f"a{relu}_y"] <= BF16_EXACT and 2 * b[f"a{relu}_gw"] < F32_EXACT, "prologue sums too large", name)
        _need(bf16_holds(p.a) and bf16_holds(p.y) and f32_holds(p.gw), "a prologue activation or output is not a bf16 number", name)
    return b


def need_exact(t, storage, name, bound=None):
    """One more stored tensor (or vector of fp32 sums) of a test that conv_case / dw_case do not describe: every element a `storage` number,
    and `bound` (the sum of absolute values that reach one accumulator) below 2^24."""
    holds = {torch.bfloat16: bf16_holds, torch.float32: f32_holds}[storage]
    _need(holds(t), f"a stored result is not a {storage} number", name)
    _need(storage != torch.bfloat16 or _maxabs(t) <= BF16_EXACT, "a bf16 store above 256", name)
    _need((_maxabs(t) if bound is None else bound) < F32_EXACT, "an fp32 sum reaches 2^24", name)


def bn_rider(shape, seeds=(7, 8, 9)):
    """The operands of a BatchNorm-backward rider on a data gradient of NCHW `shape`: the BatchNorm input y (integers), integer mean and
    power-of-two invstd (xhat = (y - mean) * invstd is a multiple of 1/2), and the forward scale / shift the ReLU mask is recomputed from."""
    Cc = shape[1]
    mean, invstd = bn_moments(Cc, seeds[1])
    mscale, mshift = bn_prologue(Cc, seeds[2])
    return types.SimpleNamespace(y=ints(shape, seeds[0]).double(), mean=mean.double(), invstd=invstd.double(), mscale=mscale.double(),
                                 mshift=mshift.double())


SEP_BUDGET = 4      # dc_sepconv_fwd serves 65 536 pixels and more: a thinner pointwise weight keeps the sums of squares of that many pixels below 2^24


@functools.lru_cache(maxsize=2)
def sep_case(spec, seeds=(1, 2, 6, 7)):
    """spec = (cin, cout, N, H, W, lazy, relu): SeparableConv2d_same.forward as dc_sepconv_fwd computes it, d = depthwise(act(x)) stored in the
    activation type, y = pointwise(d), with the statistics of y.  act is the identity (a stored input) or, lazy, x * scale + shift (+ ReLU).
    The layer has at least 65 536 pixels and a shift adds up over the nine taps, so the generators are smaller than elsewhere: scale +-1,
    an integer shift in -1 .. 1 on a quarter of the channels, pointwise weights of budget SEP_BUDGET; everything stays an integer, so
    the sums of squares are integers too.  Dense +-1 depthwise weights."""
    cin, cout, N, H, W, lazy, relu = spec
    x = ints((N, cin, H, W), seeds[0]).double()
    g = _gen(seeds[3])
    scale = (torch.randint(0, 2, (cin,), generator=g) * 2 - 1).double()
    shift = (torch.randint(-1, 2, (cin,), generator=g) * (torch.rand(cin, generator=g) < 0.25)).double()
    a = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) if lazy else x
    if relu:
        a = a.clamp_min(0)
    wdw = dw_weights(cin, seeds[1]).double()
    w = signs((cout, cin, 1, 1), seeds[2], fan=max(cin, cout), budget=SEP_BUDGET).double()
    with torch.no_grad():
        d = dw_ref(a, wdw, 1, 1)
        y = F.conv2d(d, w)
        ya = F.conv2d(dw_ref(a.abs(), wdw.abs(), 1, 1), w.abs())
    sy, syy = stats(y)
    c = types.SimpleNamespace(spec=spec, x=x, scale=scale, shift=shift, wdw=wdw, w=w, d=d, y=y, sum_y=sy, sum_yy=syy)
    c.bound = dict(d=_maxabs(d), y=_maxabs(y), partial=_maxabs(ya), sum_y=_maxabs(y.abs().sum((0, 2, 3))), sum_yy=_maxabs(syy),
                   nonzero_y=float((y != 0).double().mean()))
    return c


def sep_preconditions(c, name="sepconv"):
    """Every partial sum of the two K loops is bounded by the operators on absolute values (< 2^24); d and y are stored bf16 integers up
    to 256.  The statistics add the STORED, exact y: every partial sum of them, over any grouping of pixels, is bounded by sum |y| and
    sum y^2 of the reference itself (the terms of the second are non-negative), both below 2^24."""
    b = c.bound
    _need(b["partial"] < F32_EXACT, "fp32 partial sums reach 2^24", name)
    _need(b["d"] <= BF16_EXACT and b["y"] <= BF16_EXACT and bf16_holds(c.d) and bf16_holds(c.y) and bf16_holds(c.x), "a bf16 store is not exact", name)
    _need(bool((c.y == c.y.round()).all()), "y is not an integer (its squares would need more bits)", name)
    _need(b["sum_y"] < F32_EXACT and b["sum_yy"] < F32_EXACT, "the statistics reach 2^24", name)
    return b


def dw_rider(c, seed=8):
    """bn_rider for a depthwise case: the layer input x IS the BatchNorm input, the prologue coefficients are the BatchNorm's scale / shift."""
    mean, invstd = bn_moments(c.x.shape[1], seed)
    return types.SimpleNamespace(y=c.x, mean=mean.double(), invstd=invstd.double(), mscale=c.scale, mshift=c.shift)


def res_input(c, seed=11):
    """For the residual form of the depthwise data gradient: the layer's stored input xo = relu(bn(ybn) + residual) with ybn = c.x, bn the
    case's power-of-two scale and integer shift, and an integer residual; and the weight gradient of the layer on that input.  Halves up to
    6, so a bf16 tensor; raises NotExact otherwise."""
    Cc, stride, dil = c.spec[:3]
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    xo = (c.x * v(c.scale) + v(c.shift) + ints(tuple(c.x.shape), seed).double()).clamp_min(0)
    op = lambda a, b: dw_ref(a, b, stride, dil)  # noqa: E731
    _, _, gw = _fwd_and_grads(op, xo, c.w, c.gy)
    _, _, gwa = _fwd_and_grads(op, xo.abs(), c.w.abs(), c.gy.abs())
    _need(bf16_holds(xo) and f32_holds(gw) and 2 * _maxabs(gwa) < F32_EXACT, "the residual input or its weight gradient is not exact", "res_input")
    return xo, gw


def bn_bwd_sums(g, r, relu, name="bn rider", mask=None):
    """(sum g, sum g * xhat) per channel, g = the gradient masked by y * mscale + mshift > 0 when relu, as the kernels' epilogues take
    them: gm = mask ? g : 0, a += gm, b = fma(gm, (y - mean) * invstd, b).  No reciprocal and no square root on that path (igemm.hip,
    igemm256.hip, dwtile_common.h BnAcc::add, dwpipe.hip), so with these operands every term and every partial sum is a multiple of 1/2 below
    2^23: raises NotExact otherwise."""
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    xhat = (r.y - v(r.mean)) * v(r.invstd)
    if mask is None:            # recomputed from the BatchNorm input; else given (the sign of a stored output)
        mask = r.y * v(r.mscale) + v(r.mshift) > 0
    gm = g * mask if relu else g
    bound = float((g.abs() * xhat.abs()).sum((0, 2, 3)).max())
    _need(2 * bound < F32_EXACT and 2 * float(g.abs().sum((0, 2, 3)).max()) < F32_EXACT, "BatchNorm-backward sums too large", name)
    _need(bf16_holds(r.y) and bf16_holds(xhat) and bf16_holds(g), "a rider operand is not a bf16 number", name)
    return gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------------------------ the cases of the GPU file
def params_of(fn, arg):
    """The values of one @pytest.mark.parametrize argument of a test function."""
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize" and m.args[0] == arg:
            return list(m.args[1])
    raise KeyError(f"{fn.__name__} has no parameter {arg}")


def ids_of(fn, arg):
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize" and m.args[0] == arg:
            return list(m.kwargs["ids"])
    raise KeyError(arg)


def pointwise(shape):
    cin, cout, N, H, W = shape
    return (1, 1, 0, 1, 0, cin, cout, N, H, W)


@functools.lru_cache(maxsize=1)
def gpu_cases():
    """family -> [(name, spec, extra)]: every shape test_exact_gpu.py launches, taken from the case tables and parametrize lists of
    test_kernels_gpu.py (that module imports without a GPU: it loads the library only inside its tests)."""
    # (The one place of this module that is not self-contained.  test_kernels_gpu imports torch and mlperf_deepcam_amd.lib at module level
    # but calls lib.load() only inside its tests, which is what lets this run without a GPU; params_of / ids_of read the Mark objects its
    # @pytest.mark.parametrize decorators leave in `pytestmark`.  Whoever moves a shape list of that file into another decorator form, or
    # loads the library at its import, has to change this function with it: test_exact_cpu.py fails at collection otherwise.)
    import test_kernels_gpu as tk
    t = {}
    t["conv"] = [(c[0], tuple(c[1:11]), {}) for c in tk.CONV_CASES]
    f384 = tk.test_conv_pointwise_384_tile_kernel_same_bits
    t["pw384"] = [(n, pointwise(s), {}) for n, s in zip(ids_of(f384, "shape"), params_of(f384, "shape"))]
    f224 = tk.test_conv_pointwise_224_tile_kernel_same_bits
    t["pw224"] = [(n, pointwise(s), {}) for n, s in zip(ids_of(f224, "shape"), params_of(f224, "shape")) if n != "middle_flow_b8"]
    t["persist"] = [(c[0], tuple(c[1:11]), dict(wgs=c[11], fwd=c[12], dgrad=c[13])) for c in tk.PERSIST_CASES]
    t["thin_tile"] = [("x".join(map(str, c)), (3, 1, 1, 1, 0) + tuple(c), {}) for c in tk.THIN_TILE_CASES]
    fdg = tk.test_dilated_group_is_bit_identical_to_single_launches
    N, H, W, cin, cout = dict(zip(ids_of(fdg, "shape"), params_of(fdg, "shape")))["small"]
    t["dilated_group"] = [(f"small_d{dil}", (3, 1, dil, dil, 0, cin, cout, N, H, W), dict(seeds=(1, 10 + b, 3, 5))) for b, dil in enumerate((6, 12, 18))]
    t["wgrad_group"] = [(c[0], tuple(c[1:11]), dict(layers=c[11])) for c in tk.GROUP_CASES]
    t["wgrad384"] = [(c[0], (c[1], 1, c[2] * (c[1] - 1) // 2, c[2], 0) + tuple(c[3:8]), dict(layers=c[8], opts=c[9])) for c in tk.WG384_CASES]
    t["tconv384"] = [(c[0], (3, 2, 1, 1, 1) + tuple(c[1:6]), dict(opts=c[6])) for c in tk.TCONV384_CASES]
    t["fold"] = [(c[0], tuple(c[1:11]), dict(layers=c[11])) for c in tk.FOLD_CASES]
    t["bnstat"] = [(c[0], tuple(c[1:11]), {}) for c in tk.BNSTAT_CASES]
    t["sepconv"] = [(c[0], (c[1], 128) + tuple(c[2:7]), {}) for c in tk.SEPFWD_CASES]
    t["dw"] = [(c[0], tuple(c[1:7]), {}) for c in tk.DW_CASES if c[0] != "s2_walk"]
    t["dwpipe"] = [(c[0], (c[1], 1, c[2]) + tuple(c[3:6]), {}) for c in tk.PIPE_CASES if c[0] != "728_b8"]
    return t


# the layers of a grouped weight-gradient call take their data from these seeds (x, w, gy, bias), layer l adds l to each
GROUP_SEEDS = (10, 2, 20, 5)


def layer_seeds(l):
    return tuple(s + l for s in GROUP_SEEDS)


# the ends of the network: the shapes of test_stem and test_head, and the pooled extent 8 x 16 (1 / HW a power of two)
STEM = (2, 16, 20, 28)          # N, Cin, H, W
HEAD = (2, 256, 6, 9)           # N, Cin, H, W
POOL = (2, 2048, 8, 16)         # N, C, H, W
HEAD_LOGIT_BOUND = 1024


@functools.lru_cache(maxsize=4)
def stem_case(shape=STEM, budget=BUDGET):
    """Conv2d(Cin -> 32, k 3, s 2, p 1) at shape = (N, Cin, H, W); budget: the expected number of non-zero weights per output is
    budget * Cin / 32 (fan = 9 * 32)."""
    N, Cin, H, W = shape
    return conv_case((3, 2, 1, 1, 0, Cin, 32, N, H, W), budget=budget)


@functools.lru_cache(maxsize=8)
def head_case(shape=HEAD):
    """ConvTranspose2d(256 -> 3, k 3, s 2, p 1, op 1) with dense +-1 weights (budget = fan): logits are fp32 sums of at most 4 * 256 terms."""
    N, Cin, H, W = shape
    c = conv_case((3, 2, 1, 1, 1, Cin, 3, N, H, W), budget=10 ** 9)
    if c.bound["y"] > HEAD_LOGIT_BOUND:
        raise NotExact(f"head: |logit| can reach {c.bound['y']:.0f} > {HEAD_LOGIT_BOUND}")
    return c


def head_preconditions(c):
    """The head stores fp32 logits (bound 1024) and a bf16 data gradient; its weight gradient is fp32."""
    b = c.bound
    _need(b["y"] <= HEAD_LOGIT_BOUND and b["gw"] < F32_EXACT, "head sums too large", "head")
    _need(b["gx"] <= BF16_EXACT and bf16_holds(c.gx) and bf16_holds(c.x) and bf16_holds(c.w) and f32_holds(c.gw), "head stores", "head")
    return b


# ------------------------------------------------------------------------------------------------------------------ the ends, off their one shape
# test_exact_ends_gpu.py: the stem and the head at the extents where their kernels take another path.  Ho = (H - 1) / 2 + 1 and Wo likewise,
# P = N * Ho * Wo output pixels.  The weight-gradient kernel gives a workgroup (= a workspace row) ppb pixels in 64-pixel batches
# (stem_wgrad_plan below mirrors stem_ppb of stem_head.hip): ppb = 64 up to 65 536 pixels, so only the last extent has two batches per row.
STEM_THICK = 96     # budget of the small extents: a third of the weights non-zero (the default 24 leaves a one-channel layer 0.75 weights per output)
STEM_ENDS = [
    # name, (N, Cin, H, W), budget            what it exercises                                                      weight-gradient rows
    ("odd_31x33", (1, 16, 31, 33), STEM_THICK),      # both sides odd; P = 272: the second 256-pixel block holds 16 lanes    5, the last ragged: a 16-pixel batch
    ("odd_h_21x28", (2, 16, 21, 28), STEM_THICK),    # odd H only; P = 308                                                   5, the last ragged: a 52-pixel batch
    ("odd_w_20x27", (2, 16, 20, 27), STEM_THICK),    # odd W only; P = 280                                                   5, the last ragged: a 24-pixel batch
    ("p512", (2, 16, 32, 32), STEM_THICK),           # two full blocks, no ragged lane                                       8 full rows
    ("p240", (1, 16, 32, 30), STEM_THICK),           # a single partial block                                                4, the last ragged: a 48-pixel batch
    ("w259", (1, 16, 5, 259), STEM_THICK),           # odd W above 256: three pair chunks per row, the last of two pairs     7, the last ragged: a 6-pixel batch
    ("w258", (1, 16, 5, 258), STEM_THICK),           # even W above 256: three pair chunks per row, the last of one pair     7, the last ragged: a 3-pixel batch
    ("one_row_1x7", (1, 16, 1, 7), STEM_THICK),      # one input row, Ho = 1; P = 4                                          ONE row, a 4-pixel batch
    ("two_columns_9x2", (3, 16, 9, 2), STEM_THICK),  # two input columns, Wo = 1; P = 15                                     ONE row, a 15-pixel batch
    # added for the weight gradient: P = 66 049 > 65 536, so ppb = 128: 517 rows of two 64-pixel batches, the last row one pixel; five pair
    # chunks per row in the data gradient.  Ranges narrowed: the default budget (a twelfth of the weights non-zero), or the bound on the
    # sums of squares of that many pixels passes 2^24
    ("ppb128_513x513", (1, 16, 513, 513), BUDGET),
]
STEM_ENDS += [(f"cin{cin}_{h}x{w}", (n, cin, h, w), STEM_THICK) for (n, h, w) in ((1, 31, 33), (2, 20, 28)) for cin in (1, 3, 5, 8, 10, 12)]


def stem_out(shape):
    N, Cin, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Ho, Wo, N * Ho * Wo


def stem_wgrad_plan(P):
    """(pixels per workspace row, rows, pixels of the last 64-pixel batch of the last row) of dc_stem_wgrad."""
    ppb = ((P + 1023) // 1024 + 63) // 64 * 64
    rows = (P + ppb - 1) // ppb
    last = P - (rows - 1) * ppb
    return ppb, rows, (last - 1) % 64 + 1


def stem_preconditions(c, name="stem"):
    """preconditions() without the accumulate and bias modes the stem does not have: y and gx are stored once."""
    b = c.bound
    for key in ("y", "gx", "gw", "sum_y", "sum_yy"):
        _need(b[key] < F32_EXACT, f"fp32 partial sums of {key} reach {b[key]:.0f} >= 2^24", name)
    _need(b["y"] <= BF16_EXACT, f"|y| can reach {b['y']:.0f} > 256 (bf16 store)", name)
    for t in (c.x, c.w, c.gy, c.y):
        _need(bf16_holds(t), "an operand or a stored result is not a bf16 number", name)
    _need(f32_holds(c.gw) and f32_holds(c.gx), "a gradient is not an fp32 number", name)      # dx leaves as NCHW fp32 in both modes
    return b


HEAD_ENDS = [
    # name, (N, Cin, H, W)                            what it exercises
    ("chunks22_tiles5x3", (2, 256, 20, 70)),        # 2800 pixels: 21 full 128-pixel chunks and one of 112; 5 x 3 tiles with ragged columns
    ("two_strips", (1, 256, 9, 229)),               # eight tile columns: two strips of HF_TILES = 6; a ragged tile row
    ("one_tile_p256", (1, 256, 8, 32)),             # exactly one tile, P = 256: the first extent at which the weight gradient rides
    ("p255", (1, 256, 5, 51)),                      # P = 255: the last extent at which it does not
    ("three_samples", (3, 256, 7, 37)),             # three samples, nothing aligned
]
# both grid caps of head_bwd_impl bind: 266 240 pixels = 2080 chunks > 2048 workgroups, and 1040 > 512 weight-gradient slab rows.  bf16 only.
# Its reference (head_big_case) took 1.5 s on the CPU this was written on (float32 products of small integers and halves, every partial sum exact)
HEAD_BIG = (1, 256, 520, 512)


def head_weights(seed=2):
    return signs((256, 3, 3, 3), seed, fan=1)


def head_score(logits, labels):
    """What the loss, score and prediction epilogues leave for float64 logits [N][3][H][W]: the first-maximum class, the nine confusion counts
    and the three class counts per sample, the per-sample sums of the weighted cross-entropy, the gradient of its mean, and the
    probability of the predicted class (oracle.loss_metric throughout)."""
    import numpy as np
    from oracle import loss_metric as olm
    cw = olm.class_weights(-0.125)
    N = logits.shape[0]
    pred = torch.from_numpy(olm.argmax_first(logits))
    counts = torch.tensor(np.stack([np.concatenate(olm.confusion_counts(pred[n].numpy(), labels[n].numpy())) for n in range(N)]))
    classes = torch.stack([(pred == k).sum((1, 2)) for k in range(3)], 1)
    return types.SimpleNamespace(pred=pred, counts=counts, classes=classes, loss=olm.weighted_ce_map(logits, labels, cw).sum((1, 2)),
                                 mean_loss=float(olm.fp_loss(logits, labels, cw)), grad=olm.fp_loss_grad(logits, labels, cw),
                                 conf=torch.softmax(logits, 1).amax(1), cw=cw)


@functools.lru_cache(maxsize=8)
def head_ends_case(shape):
    """Everything test_exact_ends_gpu.py compares the head with at one extent, float64 and computed once: head_case (logits, dx, gw on
    x, w, dlogits = gy); labels and head_score of the logits; bn[relu]: the head on a = act(x * scale + shift), x taken as the raw output
    in front of a BatchNorm with bn_prologue coefficients (halves up to 5: logits and weight gradient stay exact; dx does not depend on
    the input); rider: independent bn_rider data for dc_head_bwd_bnstats; rin: the rider of the unstored form (the BatchNorm input is x,
    the mask coefficients are scale / shift)."""
    N, Cin, H, W = shape
    c = head_case(shape)
    labels = torch.randint(0, 3, (N, 2 * H, 2 * W), generator=_gen(7))
    scale, shift = (t.double() for t in bn_prologue(Cin, 6))
    mean, invstd = bn_moments(Cin, 8)
    e = types.SimpleNamespace(c=c, labels=labels, scale=scale, shift=shift, score=head_score(c.y, labels), rider=bn_rider(shape), bn=[],
                              rin=types.SimpleNamespace(y=c.x, mean=mean.double(), invstd=invstd.double(), mscale=scale, mshift=shift))
    op = lambda a, b: conv_ref(a, b, None, 3, 2, 1, 1, True)  # noqa: E731
    for relu in (0, 1):
        a = c.x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if relu:
            a = a.clamp_min(0)
        y, gx, gw = _fwd_and_grads(op, a, c.w, c.gy)
        ya, _, gwa = _fwd_and_grads(op, a.abs(), c.w.abs(), c.gy.abs())
        e.bn.append(types.SimpleNamespace(a=a, y=y, gx=gx, gw=gw, bound=dict(y=_maxabs(ya), gw=_maxabs(gwa)), score=head_score(y, labels)))
    return e


def head_ends_preconditions(e, name="head"):
    """head_preconditions, and for the unstored form: the activation a bf16 number, logits and weight gradient (halves) exact in fp32, the
    data gradient the one of the plain head; every BatchNorm-backward sum exact (bn_bwd_sums raises otherwise)."""
    b = head_preconditions(e.c)
    for relu, p in enumerate(e.bn):
        _need(bf16_holds(p.a) and f32_holds(p.y) and f32_holds(p.gw), "the activation, a logit or the weight gradient is not exact", name)
        _need(2 * p.bound["y"] < F32_EXACT and 2 * p.bound["gw"] < F32_EXACT, "fp32 partial sums (halves) reach 2^24", name)
        _need(torch.equal(p.gx, e.c.gx), "the data gradient depends on the input", name)
        bn_bwd_sums(e.c.gx, e.rider, relu, name)
        bn_bwd_sums(e.c.gx, e.rin, relu, name)
    return b


def head_big_case():
    """The head's backward at HEAD_BIG as a 27 x 256 matrix product per pixel, pixel-major ([P][256], the kernels' layout), in float32: the
    operands are integers and halves, every product and every partial sum of any order is exact, so float32 IS the float64 result here
    (test_exact_cpu.py checks the construction against head_case at a small extent).  y: the BatchNorm input; a = relu(y * scale + shift):
    the head's input; dlogits in {-1, 0, 1}; dP: the gathered gradient image (unfold); dx = dP . W, gw = a^T . dP; s0, s1: the float64
    BatchNorm-backward sums, relu = 1.  Not cached: 1.5 GB."""
    return head_matrix_case(HEAD_BIG)


def head_matrix_case(shape, seeds=(1, 2, 3)):
    N, Cin, H, W = shape
    P = N * H * W
    y = ints((P, Cin), seeds[0])
    scale, shift = bn_prologue(Cin, 6)
    mean, invstd = bn_moments(Cin, 8)
    a = (y * scale + shift).clamp_min(0)
    w = head_weights(seeds[1])
    gl = ints((N, 3, 2 * H, 2 * W), seeds[2])
    dP = F.unfold(gl, 3, 1, 1, 2).permute(0, 2, 1).reshape(P, 27).contiguous()       # [pixel][co * 9 + ky * 3 + kx], zero outside the image
    wm = w.reshape(Cin, 27)
    dx = dP @ wm.t()
    gw = (a.t() @ dP).reshape(Cin, 3, 3, 3)
    gw_bound = float((a.t() @ dP.abs()).max())
    xhat = (y - mean) * invstd
    gm = dx * (a > 0)
    s0, s1 = gm.double().sum(0), (gm * xhat).double().sum(0)
    _need(bf16_holds(a) and bf16_holds(dx) and _maxabs(dx) <= BF16_EXACT and bf16_holds(xhat), "big head: a bf16 operand or store is not exact", "head_big")
    _need(2 * gw_bound < F32_EXACT, "big head: the weight gradient's partial sums (halves) reach 2^24", "head_big")
    # a slab row adds the 128 pixels of one chunk in fp32; the rows are added in float64 by the test
    _need(2 * 128 * _maxabs(dx) * _maxabs(xhat) < F32_EXACT, "big head: a chunk's BatchNorm-backward sums reach 2^24", "head_big")
    return types.SimpleNamespace(shape=shape, y=y, a=a, scale=scale, shift=shift, mean=mean, invstd=invstd, w=w, gl=gl, dP=dP, dx=dx, gw=gw,
                                 s0=s0, s1=s1, gw_bound=gw_bound)


# ------------------------------------------------------------------------------------------------------------------ comparison
def first_difference(got, ref):
    """None where got equals ref element for element; else (index tuple, got value, reference value) of the first differing element."""
    if got.shape != ref.shape:
        return ("shape", tuple(got.shape), tuple(ref.shape))
    ne = (got != ref) | (got != got)
    if not bool(ne.any()):
        return None
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return idx, float(got[idx]), float(ref[idx])


def exactly(got, ref, what=""):
    """The exact comparison: torch.equal, with the first differing element in the message."""
    d = None if torch.equal(got, ref) else first_difference(got, ref)
    assert d is None, f"{what}: first difference at {d[0]}: got {d[1]}, reference {d[2]}"
