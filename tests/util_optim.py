"""float64 references, case tables and error bounds for the optimizer kernels (test_optim_cpu.py, test_optim_gpu.py): dc_adam_step
(adam_kernel) and dc_lamb_step (sumsq_kernel, lamb_plan_kernel, lamb_stage1_kernel, lamb_ratio_kernel, lamb_stage2_kernel) of csrc/misc.hip.

References.  adam_ref64 / lamb_ref64 restate oracle/optim.py in numpy float64 (test_optim_cpu.py pins them to torch.optim and to the oracle
at 1e-12).  LAMB is DESIGN's definition: the global clip acts on the SCALED gradient g * grad_scale, the trust ratio only where
wd != 0 and ||w|| > 0 and ||u|| > 0.  The scalar hyper-parameters are rounded to float32 first, because the ABI takes `float`.

Every step is judged on its own: the reference is applied to the float32 state the code under test started the step from, so errors do not
compound and a bound per step is a bound per expression.

Bounds, per element, with u = 2^-24 (half an fp32 ulp, relative), gr the scaled (and clipped) gradient:

  m = m_prev + (gr - m_prev) * (1 - b1)      the kernel rounds: gr (one product, g * gs), the difference, 1 - b1 (a constant), the product,
                                             the sum: five roundings, each of a quantity of magnitude <= |m_prev| + |gr|, so
                                             |m - m64| <= 5 u (|m_prev| + |gr|) in first order; FMA contraction removes roundings, never adds.
                                             LAMB's gs = grad_scale / clip carries the fp32 clip factor: the norm (fp32 partial sums of at most
                                             a few thousand terms each, totalled in double; relative error well below 1 u after the square
                                             root halves it), its division by max_grad_norm and the division grad_scale / clip: 2.5 u more on gr.
                                             Adam's L2 form adds one fused multiply-add (wd * p + gr): 1 u.
                                             Bound: |m - m64| <= 8 u (|m_prev| + |gr|).                                     (M_UNITS = 8)
  v = v_prev * b2 + (1 - b2) * gr * gr       gr^2 doubles gr's relative error (2 x 3.5 u at the worst), two products and 1 - b2 add 3 u to that
                                             term, v_prev * b2 and the sum 2 u: within 8 u (v_prev + gr^2) only because the terms are
                                             non-negative (no cancellation) and the 7 u belong to the (1 - b2) gr^2 term, a thousandth of the bound's
                                             scale.  Bound: |v - v64| <= 8 u (v_prev + gr^2).                               (V_UNITS = 8)
  A numpy float32 restatement of the kernel's expression sequence (adam_emul32 / lamb_emul32 below) stays within 2 of these units on the
  whole case table (test_optim_cpu.py asserts it): the factor 8 is headroom for the clip factor and for the compiler's contraction choices,
  not for a wrong kernel; the mutants of test_optim_cpu.py are off by thousands of units.

  delta = p_new - p_old (formed in float64 from the two float32 values):
      |delta - delta64| <= k u |p_old| + R * a * U,     k = 1 (2.5 for AdamW with a non-zero decay, below),
      a = lr (Adam, AdamW), lr * trust ratio of the element's tensor (LAMB),
      U = mhat_abs / (sqrt(vhat) + eps) + |wd * p_old|  (the second term for AdamW and LAMB: Adam's L2 decay is inside gr),
      mhat_abs = (b1 |m_prev| + (1 - b1) |gr|) / bc1.
  u |p_old| is the rounding of the stored parameter.  Everything else is an error RELATIVE to the size of the update: the step size and the
  bias corrections (a few u), the trust ratio (two norms), mhat (the m bound above), sqrt(vhat) + eps (half the v bound).  A bound relative
  to delta64 itself fails where the Adam term and the decay term cancel, and where b1 m_prev and (1 - b1) gr cancel inside mhat: the m bound
  is relative to |m_prev| + |gr|, not to |m|.  U is therefore the update evaluated on the ABSOLUTE values of its operands, which is what the
  roundings scale with (on every from-zero case mhat_abs = |mhat| and U is |mhat| / (sqrt(vhat) + eps) + |wd p| to the letter).
  Where a * U = 0 (the all-zero tensor) the parameter may not move beyond u |p_old|.

  R is not derived but measured on references, never on the kernel: the largest R that (a) oracle.optim.OracleOptimizer in float32 on the CPU
  and (b) the numpy float32 restatement of the kernel's expression order need against the float64 reference, over the whole case table
  (measure_R(); test_optim_cpu.py repeats the measurement and asserts it stays below the recorded value).  The bound uses 4 x that: the
  kernel's per-chunk norms are fp32 sums of up to 4096 terms where the oracle's are double, and its contraction choices are the compiler's.
  AdamW with a non-zero decay rounds the stored parameter more than once, which a single u |p_old| cannot cover: the constant 1 - lr * wd
  (u / 2), the decay product p * (1 - lr * wd) (u) and the update (u): 2.5 u |p_old| (p_units()).  With one u the second rounding would
  land in R, and it is not relative to the update: on the elements whose gradient is exactly zero it made the measured R 1.9e-3 instead of
  3e-7, a bound under which no decay-order mistake could be seen.  Adam, LAMB (one fused multiply-add) and AdamW at wd = 0 keep 1 u.

  Adam's L2 form builds gr = g * grad_scale + wd * p, whose terms can cancel while their roundings do not: for that kind the |gr| of the m, v
  and U scales above is |g * grad_scale| + |wd * p| (`gabs`); elsewhere it is |gr| itself.

Input generators: see lamb_inputs / inputs.  The edges carry weight: the last n % 4 elements of the gradient arena hold half of the
global norm, the first and last element of every tensor are as large as the rest of the tensor together (weights and gradients), tensors
differ in scale by up to 8 x, one tensor has zero weights, one has zero weights and zero gradients (and zero moments).

Host-only: nothing here touches a GPU or loads the library."""
import functools
import math
import types

import numpy as np

U24 = 2.0 ** -24
M_UNITS = 8.0
V_UNITS = 8.0
EMUL_UNITS = 2.0             # what the float32 restatement of the kernel needs of the m / v bounds (asserted on the CPU)

# measured (measure_R(): the larger of the fp32 oracle's and the fp32 restatement's need over the whole case table) | chosen = 4 x measured
R_MEASURED = {"LAMB": 3.4e-7, "Adam": 3.3e-7, "AdamW": 3.3e-7}      # chosen: 1.36e-6, 1.32e-6, 1.32e-6
R = {k: 4.0 * x for k, x in R_MEASURED.items()}

LAMB_CHUNK = 4096            # csrc/misc.hip
SUMSQ_BLOCKS = 1024          # csrc/misc.hip: more tensors than this and stage 2 sums the chunk norms itself
B1, B2 = 0.9, 0.999


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ float64 references
def adam_ref64(kind, p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale):
    """torch.optim.Adam ("Adam": L2 penalty folded into the gradient) / AdamW ("AdamW": decoupled decay) single-tensor step in float64.
    Returns p_new, m_new, v_new, gr (the scaled gradient, with Adam's L2 term)."""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gr = g * gs
    if kind == "Adam":
        gr = gr + wd * p
    elif kind == "AdamW":
        p = p * (1.0 - lr * wd)
    else:
        raise ValueError(kind)
    m2 = m + (gr - m) * (1.0 - b1)
    v2 = v * b2 + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p2 = p - (lr / bc1) * (m2 / (np.sqrt(v2) / math.sqrt(bc2) + eps))
    return p2, m2, v2, gr


def adam_U(kind, p, gabs, m, v2, b1, b2, eps, wd, step):
    """The update on absolute values (module docstring); float64 arrays of the step's inputs, gabs = |g * grad_scale| (+ |wd * p| for Adam's
    L2 form), v2 from adam_ref64."""
    b1, b2, eps, wd = (f32(x) for x in (b1, b2, eps, wd))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    mabs = (b1 * np.abs(m) + (1.0 - b1) * gabs) / bc1
    Uu = mabs / (np.sqrt(v2 / bc2) + eps)
    return Uu + np.abs(wd * np.asarray(p, dtype=np.float64)) if kind == "AdamW" else Uu


def tensor_sums(x, offsets):
    return np.add.reduceat(x, np.asarray(offsets[:-1], dtype=np.int64))


def lamb_ref64(offsets, p, g, m, v, lr, b1, b2, eps, wd, step, max_grad_norm, grad_scale):
    """DESIGN's LAMB in float64.  Returns p_new, m_new, v_new, gr (scaled and clipped gradient), a (lr * trust ratio, per tensor) and U
    (the update on absolute values, per element)."""
    lr, b1, b2, eps, wd, mgn, gs = (f32(x) for x in (lr, b1, b2, eps, wd, max_grad_norm, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    sizes = np.diff(np.asarray(offsets, dtype=np.int64))
    assert sizes.min() > 0 and offsets[0] == 0 and offsets[-1] == p.size
    gsc = g * gs
    gnorm = math.sqrt(float(np.dot(gsc, gsc)))
    clip = gnorm / mgn if gnorm > mgn else 1.0
    gr = gsc / clip
    m2 = m + (gr - m) * (1.0 - b1)
    v2 = v * b2 + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    den = np.sqrt(v2 / bc2) + eps
    upd = (m2 / bc1) / den + wd * p
    wn, un = np.sqrt(tensor_sums(p * p, offsets)), np.sqrt(tensor_sums(upd * upd, offsets))
    ok = (wn > 0) & (un > 0) & (wd != 0)
    ratio = np.where(ok, wn / np.where(un > 0, un, 1.0), 1.0)
    a = lr * ratio
    p2 = p - np.repeat(a, sizes) * upd
    Uu = ((b1 * np.abs(m) + (1.0 - b1) * np.abs(gr)) / bc1) / den + np.abs(wd * p)
    return p2, m2, v2, gr, a, Uu


# ------------------------------------------------------------------------------------------------------------------ float32 restatements
F = np.float32


def _fma32(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32) if np.ndim(b) == 0 else \
        (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_emul32(kind, p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, mutant=None):
    """adam_kernel's expression sequence in numpy float32 (every operation rounded; the L2 form's fmaf as one rounding).
    mutant: "decay_after" (AdamW decay applied after the update instead of before the moments), "l2_not_in_v" (Adam's L2 term missing
    from the second moment), "bias_step_minus_1"."""
    lr, b1, b2, eps, wd, gs = (F(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    s = step - 1 if mutant == "bias_step_minus_1" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = 1.0 - float(b1) ** s, 1.0 - float(b2) ** s
        step_size = F(np.float64(lr) / bc1)
        inv = F(1.0 / np.sqrt(np.float64(bc2)))
        gr = g * gs
        grv = gr
        if kind == "Adam":
            gr = _fma32(p, wd, gr)
            grv = gr if mutant != "l2_not_in_v" else grv
        elif mutant != "decay_after":
            p = p * (F(1) - lr * wd)
        m2 = m + (gr - m) * (F(1) - b1)
        v2 = v * b2 + (F(1) - b2) * grv * grv
        p2 = p - step_size * (m2 / (np.sqrt(v2) * inv + eps))
        if kind == "AdamW" and mutant == "decay_after":
            p2 = p2 * (F(1) - lr * wd)
    return p2, m2, v2


def _chunks(offsets):
    """start of every LAMB chunk, and the index of every tensor's first chunk"""
    offs = np.asarray(offsets, dtype=np.int64)
    counts = (np.diff(offs) + LAMB_CHUNK - 1) // LAMB_CHUNK
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    starts = np.repeat(offs[:-1], counts) + LAMB_CHUNK * (np.arange(int(counts.sum())) - np.repeat(first, counts))
    return starts, first


def lamb_emul32(offsets, p, g, m, v, lr, b1, b2, eps, wd, step, max_grad_norm, grad_scale, mutant=None):
    """dc_lamb_step's expression sequence in numpy float32: clip factor from the float32 norm, moments, update direction, per-chunk float32
    norms totalled in double, float32 step size, one fused multiply-add into the parameter.
    mutant: "drop_tail" (clip norm without the last n % 4 elements), "unscaled_norm" (clip norm of g instead of g * grad_scale),
    "neighbour_chunk" (a tensor's norms include the first chunk of the next tensor), "skip_4096" (chunks one element too long: element 4096
    of a tensor is nobody's), "bias_step_minus_1", "ratio_at_wd0" (trust ratio applied whatever the weight decay)."""
    lr, b1, b2, eps, wd, mgn, gs = (F(x) for x in (lr, b1, b2, eps, wd, max_grad_norm, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    offs = np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(offs)
    n = p.size
    x = g if mutant == "unscaled_norm" else g * gs
    if mutant == "drop_tail":
        x = x[:n - n % 4]
    x = x.astype(np.float64)
    gnorm = F(math.sqrt(float(np.dot(x, x))))
    clip = gnorm / mgn if gnorm > mgn else F(1)
    gsf = gs / clip
    s = step - 1 if mutant == "bias_step_minus_1" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = F(1.0 - float(b1) ** s), F(1.0 - float(b2) ** s)
        gr = g * gsf
        m2 = m + (gr - m) * (F(1) - b1)
        v2 = v * b2 + (F(1) - b2) * gr * gr
        upd = (m2 / bc1) / (np.sqrt(v2 / bc2) + eps) + wd * p
        live = np.ones(n, dtype=bool)
        if mutant == "skip_4096":
            idx = offs[:-1][sizes > LAMB_CHUNK] + LAMB_CHUNK
            live[idx] = False
        starts, first = _chunks(offs)
        pw = np.where(live, p * p, F(0)).astype(np.float64)
        uw = np.where(live, upd * upd, F(0)).astype(np.float64)
        cw = np.add.reduceat(pw, starts).astype(np.float32).astype(np.float64)      # per-chunk sums, stored as float32
        cu = np.add.reduceat(uw, starts).astype(np.float32).astype(np.float64)
        tw, tu = np.add.reduceat(cw, first), np.add.reduceat(cu, first)
        if mutant == "neighbour_chunk":
            tw[:-1] += cw[first[1:]]
            tu[:-1] += cu[first[1:]]
        wn, un = np.sqrt(tw).astype(np.float32), np.sqrt(tu).astype(np.float32)
        ok = (wn > 0) & (un > 0) & ((wd != 0) or mutant == "ratio_at_wd0")
        ratio = np.where(ok, wn / np.where(un > 0, un, F(1)), F(1)).astype(np.float32)
        a = (lr * ratio).astype(np.float32)
        p2 = _fma32(-np.repeat(a, sizes), upd, p)
    if mutant == "skip_4096":
        p2, m2, v2 = np.where(live, p2, p), np.where(live, m2, m), np.where(live, v2, v)
    return p2, m2, v2


# ------------------------------------------------------------------------------------------------------------------ input generators
def _edges(x, offs, scale, sizes):
    """first and last element of every tensor as large as the rest of the tensor together (norm scale * sqrt(size)), opposite signs"""
    big = 0.7 * scale * np.sqrt(np.maximum(sizes, 2))
    x[offs[:-1]] = big
    x[offs[1:] - 1] = -big
    return x


def special_tensors(nt):
    """(zero-weight tensor, all-zero tensor): indices, None where the layout is too short.  Never the last tensors: the gradient tail is there."""
    return (1 if nt >= 3 else None), (nt // 2 if nt >= 4 else None)


def lamb_inputs(sizes, seed, gnorm):
    """Weights of scale ~0.05 and a gradient arena of norm `gnorm`, float32.  Per-tensor scales differ by up to 8 x (a chunk credited to
    the wrong tensor moves both norms); edges as in _edges; the last n % 4 gradient elements hold HALF of the squared norm (so a clip norm
    without them is off by a factor 0.71); tensor zw has zero weights, tensor zz zero weights and zero gradients."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n, nt = int(offs[-1]), len(sizes)
    ps = 0.02 * 2.0 ** rs.randint(0, 4, nt)
    gsig = 2.0 ** rs.randint(0, 4, nt)
    p = _edges(rs.standard_normal(n) * np.repeat(ps, sizes), offs, ps, sizes)
    g = _edges(rs.standard_normal(n) * np.repeat(gsig, sizes), offs, gsig, sizes)
    zw, zz = special_tensors(nt)
    if zw is not None:
        p[offs[zw]:offs[zw + 1]] = 0.0
    if zz is not None:
        p[offs[zz]:offs[zz + 1]] = 0.0
        g[offs[zz]:offs[zz + 1]] = 0.0
    k = n % 4
    if k:
        rest = float(np.dot(g[:n - k], g[:n - k]))
        g[n - k:] = math.sqrt(rest / k) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    g *= gnorm / math.sqrt(float(np.dot(g, g)))
    return offs, p.astype(np.float32), g.astype(np.float32)


def moments_like(gr, offs, seed):
    """Non-zero incoming moments of a resumed run: m ~ 0.3 rms(gr) N(0, 1), v = rms(gr)^2 U(0.25, 1.25), rms per tensor (an all-zero
    tensor keeps zero moments)."""
    rs = np.random.RandomState(seed)
    sizes = np.diff(offs)
    rms = np.repeat(np.sqrt(tensor_sums(np.asarray(gr, dtype=np.float64) ** 2, offs) / sizes), sizes)
    m = 0.3 * rms * rs.standard_normal(gr.size)
    v = rms * rms * (0.25 + rs.random_sample(gr.size))
    return m.astype(np.float32), v.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ case tables
ADAM_BIG = 4194304 + 4 * 256 * 3 + 2      # smallest size family at which ew_blocks2 caps the grid: grid-stride loop with a ragged tail
ADAM_SIZES = (1, 2, 3, 4, 5, 1023, 4099, 100003, ADAM_BIG)
WDS = (0.0, 1e-6, 1e-2)
SCALES = (1.0, 0.5, 1.0 / 3.0)
ADAM_LRS = (1e-3, 2e-3, 5e-4)             # changed between steps through the device scalar


def _adam_case(name, kind, n, wd, gs, steps, lrs=ADAM_LRS, resume=False, seed=0):
    return types.SimpleNamespace(family="adam", name=name, kind=kind, n=n, wd=wd, grad_scale=gs, steps=tuple(steps), lrs=tuple(lrs), resume=resume,
                                 eps=1e-8, seed=seed, offsets=np.array([0, n], dtype=np.int64))


def _adam_cases():
    cases = []
    for kind in ("Adam", "AdamW"):
        for i, n in enumerate(ADAM_SIZES):                      # every size, from zero moments, steps 1 .. 3; wd and grad_scale cycle
            cases.append(_adam_case(f"{kind}-n{n}-zero", kind, n, WDS[(i + 1) % 3], SCALES[(i + i // 3) % 3], (1, 2, 3), seed=10 + i))
        for i, (wd, gs) in enumerate((w, s) for w in WDS for s in SCALES):      # wd x grad_scale at two ragged sizes
            n = (4099, 100003)[i % 2]
            cases.append(_adam_case(f"{kind}-n{n}-wd{wd:g}-gs{gs:.2g}", kind, n, wd, gs, (1, 2), seed=40 + i))
        for i, (n, step) in enumerate(((5, 1000), (4099, 1000), (100003, 100000), (ADAM_BIG, 1000), (1023, 100000))):   # resumed runs
            cases.append(_adam_case(f"{kind}-n{n}-step{step}", kind, n, WDS[(i + 2) % 3], SCALES[i % 3], (step, step + 1), resume=True, seed=60 + i))
        # a schedule's warm-up peak: the order of decay and update matters in proportion to lr * wd
        cases.append(_adam_case(f"{kind}-n4099-large_lr", kind, 4099, 1e-2, 0.5, (1, 2, 3), lrs=(5e-2, 1e-1, 2e-2), seed=80))
    return cases


def model_sizes(divisor=64):
    """The 301 parameter tensors of the network, every size divided by `divisor` (rounded up): ~0.9 M elements instead of 56 M."""
    from mlperf_deepcam_amd import spec
    offs = spec.Layout(16, 3).offsets()
    return [max(1, -(-(b - a) // divisor)) for a, b in zip(offs[:-1], offs[1:])]


def _mixed(count, seed, hi):
    rs = np.random.RandomState(seed)
    return [int(x) for x in rs.randint(1, hi + 1, count)]


def lamb_layouts():
    m65 = _mixed(65, 1, 300)
    m65[3], m65[40], m65[64] = 4097, 8192, 4096 + 2        # multi-chunk tensors inside a lane's run, and at its end
    m130 = _mixed(130, 2, 200)
    m130[0], m130[129] = 12289, 4095
    m1024 = _mixed(1024, 3, 9)
    m1024[512] = 4097
    return {
        "eight": [1, 3, 4095, 4096, 4097, 8193, 7, 1000],
        "t65": m65,                                        # more than one tensor per lane of lamb_plan_kernel
        "t130": m130,
        "model301": model_sizes(),
        "t1025": _mixed(1025, 4, 9),                       # step_size == nullptr: stage 2 sums the norms itself
        "t1024": m1024,                                    # the last count served by lamb_ratio_kernel
        "big3": [2150001, 4097, 50001],                    # sumsq_kernel's two-in-flight loop (n / 4 > 2 * 262144); a 525-chunk tensor
    }


LAMB_LRS = (2e-3, 1e-2, 5e-3)
# name: (||g|| / max_grad_norm of the UNSCALED gradient, max_grad_norm, grad_scale, wd, steps, resume)
LAMB_MODES = {
    "clip": (30.0, 1.0, 1.0, 1e-2, (1, 2, 3), False),            # ||g|| >> max_grad_norm
    "noclip": (0.5, 2.0, 1.0, 1e-2, (1, 2, 3), False),           # ||g * grad_scale|| < max_grad_norm
    "gs1": (3.0, 1.0, 1.0, 1e-2, (1, 2), False),                 # the clip decision depends on the scale: 3 and 1.5 clip, 0.75 does not
    "gs.5": (3.0, 1.0, 0.5, 1e-2, (1, 2), False),
    "gs.25": (3.0, 1.0, 0.25, 1e-2, (1, 2), False),
    "wd0": (30.0, 0.5, 0.5, 0.0, (1, 2, 3), False),              # no trust ratio
    "resume": (3.0, 1.0, 0.5, 1e-2, (1000, 1001), True),         # non-zero incoming moments
}
LAMB_BIG_MODES = ("clip", "gs.25", "resume")                      # the two large layouts: a subset


def _lamb_cases():
    cases = []
    for li, (lname, sizes) in enumerate(lamb_layouts().items()):
        big = lname in ("model301", "big3")
        for mi, (mode, (rel, mgn, gs, wd, steps, resume)) in enumerate(LAMB_MODES.items()):
            if big and mode not in LAMB_BIG_MODES:
                continue
            offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            cases.append(types.SimpleNamespace(family="lamb", name=f"{lname}-{mode}", kind="LAMB", layout=lname, mode=mode, sizes=sizes, offsets=offs,
                                               n=int(offs[-1]), gnorm=rel * mgn, max_grad_norm=mgn, grad_scale=gs, wd=wd, steps=tuple(steps),
                                               lrs=LAMB_LRS, resume=resume, eps=1e-6, seed=100 * li + mi))
    return cases


@functools.lru_cache(maxsize=1)
def cases():
    """name -> case, Adam's then LAMB's."""
    return {c.name: c for c in _adam_cases() + _lamb_cases()}


def names(family):
    return [n for n, c in cases().items() if c.family == family]


@functools.lru_cache(maxsize=3)
def inputs(name):
    """The data of a case, generated once and shared (read-only): p0, m0, v0 and one gradient arena per step, all float32."""
    c = cases()[name]
    if c.family == "lamb":
        _, p, g0 = lamb_inputs(c.sizes, c.seed, c.gnorm)
        gs = [g0] + [lamb_inputs(c.sizes, c.seed + 1000 * k, c.gnorm)[2] for k in range(1, len(c.steps))]
        gr = g0.astype(np.float64) * c.grad_scale
        gr /= max(1.0, math.sqrt(float(np.dot(gr, gr))) / c.max_grad_norm)
    else:
        rs = np.random.RandomState(c.seed)
        p = (0.05 * rs.standard_normal(c.n)).astype(np.float32)
        gs = []
        for _ in c.steps:
            g = 0.01 * rs.standard_normal(c.n)
            if not c.resume:
                g[3::5] = 0.0       # exactly zero in every step: v stays 0 there, the denominator is eps alone and the update 0 / eps
            gs.append((g / c.grad_scale).astype(np.float32))
        gr = gs[0].astype(np.float64) * c.grad_scale
    if c.resume:
        m, v = moments_like(gr, c.offsets, c.seed + 7)
    else:
        m, v = np.zeros(c.n, dtype=np.float32), np.zeros(c.n, dtype=np.float32)
    for a in [p, m, v] + gs:
        a.setflags(write=False)
    return types.SimpleNamespace(p=p, m=m, v=v, g=gs)


# ------------------------------------------------------------------------------------------------------------------ judging a step
def p_units(c):
    """roundings of the stored parameter in units of u |p_old| (module docstring): 2.5 for AdamW with a non-zero decay, else 1"""
    return 2.5 if c.kind == "AdamW" and c.wd != 0 else 1.0


def _units(err, scale):
    """max err / scale; 0 / 0 counts as 0, x / 0 and anything non-finite as inf"""
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def reference(c, p, g, m, v, lr, step):
    """The float64 reference of one step of case c from the float32 state (p, m, v): namespace p, m, v, gr, aU (a * U per element)."""
    if c.family == "lamb":
        p2, m2, v2, gr, a, Uu = lamb_ref64(c.offsets, p, g, m, v, lr, B1, B2, c.eps, c.wd, step, c.max_grad_norm, c.grad_scale)
        aU = np.repeat(a, np.diff(c.offsets)) * Uu
    else:
        p2, m2, v2, gr = adam_ref64(c.kind, p, g, m, v, lr, B1, B2, c.eps, c.wd, step, c.grad_scale)
        gabs = np.abs(gr)
        if c.kind == "Adam":        # gr = g * gs + wd * p: the roundings scale with the two terms, not with their (possibly cancelling) sum
            gabs = np.abs(np.asarray(g, dtype=np.float64) * f32(c.grad_scale)) + np.abs(f32(c.wd) * np.asarray(p, dtype=np.float64))
        aU = f32(lr) * adam_U(c.kind, p, gabs, m, v2, B1, B2, c.eps, c.wd, step)
        return types.SimpleNamespace(p=p2, m=m2, v=v2, gr=gr, gabs=gabs, aU=aU, punits=p_units(c))
    return types.SimpleNamespace(p=p2, m=m2, v=v2, gr=gr, gabs=np.abs(gr), aU=aU, punits=1.0)


def judge(ref, p0, m0, v0, p1, m1, v1):
    """Errors of one step in bound units: (m error / (u (|m_prev| + |gr|)), v error / (u (v_prev + gr^2)), the R the step needs)."""
    p0, m0, v0, p1, m1, v1 = (np.asarray(a, dtype=np.float64) for a in (p0, m0, v0, p1, m1, v1))
    em = _units(np.abs(m1 - ref.m), U24 * (np.abs(m0) + ref.gabs))
    ev = _units(np.abs(v1 - ref.v), U24 * (v0 + ref.gabs * ref.gabs))
    ed = np.abs((p1 - p0) - (ref.p - p0))
    ed = np.where(np.isfinite(ed), ed, np.inf)
    r = _units(np.maximum(ed - ref.punits * U24 * np.abs(p0), 0.0), ref.aU)
    return em, ev, r


def stepper_args(c, lr, step):
    """positional hyper-parameters of *_ref64 / *_emul32 behind (p, g, m, v)"""
    if c.family == "lamb":
        return (lr, B1, B2, c.eps, c.wd, step, c.max_grad_norm, c.grad_scale)
    return (lr, B1, B2, c.eps, c.wd, step, c.grad_scale)


def run_case(name, stepper):
    """Walk case `name` with stepper(c, p, g, m, v, lr, step) -> (p, m, v) float32 (numpy), which continues from its OWN state; every step is
    judged against the float64 reference applied to that state.  Returns the worst (m units, v units, R needed) over the steps."""
    c, d = cases()[name], inputs(name)
    p, m, v = d.p, d.m, d.v
    worst = (0.0, 0.0, 0.0)
    for g, lr, step in zip(d.g, c.lrs, c.steps):
        ref = reference(c, p, g, m, v, lr, step)
        p1, m1, v1 = (np.asarray(a, dtype=np.float32) for a in stepper(c, p, g, m, v, lr, step))
        worst = tuple(max(a, b) for a, b in zip(worst, judge(ref, p, m, v, p1, m1, v1)))
        p, m, v = p1, m1, v1
    return worst


def within_bounds(errs, kind):
    em, ev, r = errs
    return em <= M_UNITS and ev <= V_UNITS and r <= R[kind]


def emul_stepper(mutant=None):
    def step(c, p, g, m, v, lr, s):
        if c.family == "lamb":
            return lamb_emul32(c.offsets, p, g, m, v, *stepper_args(c, lr, s), mutant=mutant)
        return adam_emul32(c.kind, p, g, m, v, *stepper_args(c, lr, s), mutant=mutant)
    return step


def oracle_stepper(c, p, g, m, v, lr, step):
    """oracle.optim.OracleOptimizer in float32 on the CPU, started from the given state.  It has no grad_scale: it gets the float32 product
    g * grad_scale (exact for the power-of-two scales)."""
    import torch
    from oracle.optim import OracleOptimizer
    offs = [int(o) for o in c.offsets]
    cut = lambda a: [torch.from_numpy(np.array(a[i:j], dtype=np.float32)) for i, j in zip(offs[:-1], offs[1:])]  # noqa: E731
    ps = cut(p)
    opt = OracleOptimizer(ps, c.kind, lr=f32(lr), eps=f32(c.eps), weight_decay=f32(c.wd), betas=(f32(B1), f32(B2)),
                          max_grad_norm=f32(getattr(c, "max_grad_norm", 1.0)))
    opt.m, opt.v, opt.step_count = cut(m), cut(v), step - 1
    opt.step(cut(np.asarray(g, dtype=np.float32) * np.float32(c.grad_scale)))
    cat = lambda ts: torch.cat(ts).numpy()  # noqa: E731
    return cat(ps), cat(opt.m), cat(opt.v)


def measure_R(verbose=False):
    """family kind -> the largest R the float32 oracle and the float32 restatement need over the case table (R_MEASURED), and the largest
    m / v units of each."""
    need = {"LAMB": 0.0, "Adam": 0.0, "AdamW": 0.0}
    units = {"oracle": 0.0, "emul": 0.0}
    for name, c in cases().items():
        eo, ee = run_case(name, oracle_stepper), run_case(name, emul_stepper())
        need[c.kind] = max(need[c.kind], eo[2], ee[2])
        units["oracle"] = max(units["oracle"], eo[0], eo[1])
        units["emul"] = max(units["emul"], ee[0], ee[1])
        if verbose:
            print(f"{name:32s} oracle m {eo[0]:.2f} v {eo[1]:.2f} R {eo[2]:.3e} | emul m {ee[0]:.2f} v {ee[1]:.2f} R {ee[2]:.3e}", flush=True)
    return need, units
