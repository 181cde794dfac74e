"""The optimizer kernel tests (test_optim_gpu.py) before any kernel is involved:

  - the float64 references of util_optim.py equal torch.optim.Adam / AdamW run in float64 and oracle.optim.OracleOptimizer("LAMB") run on
    float64 tensors, to 1e-12;
  - the float32 oracle and a numpy float32 restatement of the kernels' expression order stay inside the bounds of util_optim.py on EVERY case
    the GPU file launches (the precondition that the reference alone does), the restatement inside 2 of the 8 units of the moment bounds, and
    neither needs more than the recorded R_MEASURED (a quarter of the R the GPU tests allow);
  - eight deliberately wrong restatements (MUTANTS) each violate the bounds on a named case of the table;
  - the reason this file exists: the parameter-only comparison of test_kernels_gpu.py::test_lamb_matches_oracle (rtol 2e-5, atol 2e-6, on
    its own inputs) ACCEPTS a clip norm that drops the last n % 4 gradient elements and cannot express three more of the mistakes at all
    (grad_scale is always 1; at wd == 0 the per-tensor norms are unused), while the bounds of util_optim.py reject every mutant
    (test_what_the_parameter_only_check_accepts: which ones, measured, and why).  A trust ratio that pulls in the neighbouring tensor's
    chunk, which one might expect that check to accept as well, it rejects at wd = 1e-2 on its inputs; it is recorded as such."""
import numpy as np
import pytest
import torch

import util_optim as U
from oracle.optim import OracleOptimizer

HYPER = dict(lr=U.f32(1e-3), b1=U.f32(0.9), b2=U.f32(0.999), eps=U.f32(1e-8))


def _close(a, b, scale, what):
    """|a - b| <= 1e-12 * scale per element, scale the magnitude of the terms the value is made of (a bound relative to the value itself
    fails where they cancel)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = U._units(np.abs(a - b), scale)
    assert err <= 1e-12, f"{what}: difference {err:.3e} of its scale"


@pytest.mark.parametrize("kind,wd,gs", [("Adam", 0.0, 1.0), ("Adam", 1e-2, 0.5), ("AdamW", 1e-2, 1.0), ("AdamW", 1e-6, 0.25)])
def test_adam_ref64_equals_torch_optim_in_float64(kind, wd, gs):
    """Five steps, new gradient and learning rate every step; parameters and both moments."""
    rs = np.random.RandomState(5)
    n, wd = 1000, U.f32(wd)
    p = 0.05 * rs.standard_normal(n)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    cls = torch.optim.Adam if kind == "Adam" else torch.optim.AdamW
    opt = cls([tp], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"], weight_decay=wd)
    m, v = np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = 0.01 * rs.standard_normal(n)
        lr = U.f32(HYPER["lr"] * (1 + 0.5 * step))
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g * gs)            # torch.optim knows no grad_scale; a power of two commutes with the rounding
        opt.step()
        p0, m0, v0 = p, m, v
        p, m, v, _ = U.adam_ref64(kind, p, g, m, v, lr, HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step, gs)
        st = opt.state[tp]
        gabs = np.abs(g * gs) + np.abs(wd * p0)
        _close(p, tp.detach().numpy(), np.abs(p0) + lr * U.adam_U(kind, p0, gabs, m0, v, HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step), f"p, step {step}")
        _close(m, st["exp_avg"].numpy(), np.abs(m0) + gabs, f"m, step {step}")
        _close(v, st["exp_avg_sq"].numpy(), v0 + gabs ** 2, f"v, step {step}")


@pytest.mark.parametrize("mode", ["clip", "noclip", "gs.25", "wd0"])
def test_lamb_ref64_equals_the_oracle_in_float64(mode):
    """OracleOptimizer("LAMB") on float64 tensors, three steps on the eight-tensor layout with its zero tensors; the oracle has no grad_scale
    and gets g * grad_scale (a power of two: exact)."""
    rel, mgn, gs, wd, _, _ = U.LAMB_MODES[mode]
    sizes = U.lamb_layouts()["eight"]
    offs, p32, _ = U.lamb_inputs(sizes, 3, rel * mgn)
    lr, eps, wd, mgn = U.f32(1e-2), U.f32(1e-6), U.f32(wd), U.f32(mgn)
    p = p32.astype(np.float64)
    cut = lambda a: [torch.from_numpy(np.array(a[i:j], dtype=np.float64)) for i, j in zip(offs[:-1], offs[1:])]  # noqa: E731
    ps = cut(p)
    opt = OracleOptimizer(ps, "LAMB", lr=lr, eps=eps, weight_decay=wd, betas=(HYPER["b1"], HYPER["b2"]), max_grad_norm=mgn)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step in range(1, 4):
        g = U.lamb_inputs(sizes, 3 + step, rel * mgn)[2].astype(np.float64)
        opt.step(cut(g * gs))
        p0, m0, v0 = p, m, v
        p, m, v, gr, a, Uu = U.lamb_ref64(offs, p, g, m, v, lr, HYPER["b1"], HYPER["b2"], eps, wd, step, mgn, gs)
        _close(p, torch.cat(ps).numpy(), np.abs(p0) + np.repeat(a, sizes) * Uu, f"p, step {step}")
        _close(m, torch.cat(opt.m).numpy(), np.abs(m0) + np.abs(gr), f"m, step {step}")
        _close(v, torch.cat(opt.v).numpy(), v0 + gr * gr, f"v, step {step}")
    zw, zz = U.special_tensors(len(sizes))
    assert np.all(p[offs[zz]:offs[zz + 1]] == 0) and np.all(p[offs[zw]:offs[zw + 1]] != 0)
    if wd == 0:
        assert np.all(a == lr)                      # no trust ratio without weight decay


def test_the_generators_put_weight_on_the_edges():
    """What the mutants below rely on: the last n % 4 gradient elements hold half of the squared norm; the first and last element of every
    tensor hold a visible share of its weight and gradient norms; the zero tensors are zero; the moments of a resumed case are non-zero, v >= 0."""
    for name in ("t65-clip", "t1024-resume", "t1025-gs.25"):
        c, d = U.cases()[name], U.inputs(name)
        g = d.g[0].astype(np.float64)
        k = c.n % 4
        assert k and float(np.dot(g[-k:], g[-k:])) >= 0.45 * float(np.dot(g, g))
        assert float(np.sqrt(np.dot(g, g))) == pytest.approx(c.gnorm, rel=1e-6)
        offs = c.offsets
        for x in (d.p.astype(np.float64), g[:c.n - k]):
            tot = U.tensor_sums(x * x, offs) if x.size == c.n else None
            if tot is None:
                continue
            edge = x[offs[:-1]] ** 2 + x[offs[1:] - 1] ** 2
            big = np.diff(offs) >= 16
            assert np.all(edge[big & (tot > 0)] >= 0.2 * tot[big & (tot > 0)])
        zw, zz = U.special_tensors(len(c.sizes))
        assert not d.p[offs[zw]:offs[zw + 1]].any() and d.g[0][offs[zw]:offs[zw + 1]].all()
        assert not d.p[offs[zz]:offs[zz + 1]].any() and not any(gg[offs[zz]:offs[zz + 1]].any() for gg in d.g)
        if c.resume:
            live = np.ones(c.n, dtype=bool)
            live[offs[zz]:offs[zz + 1]] = False
            assert np.all(d.v[live] > 0) and np.all(d.m[live] != 0) and not d.m[~live].any() and not d.v[~live].any()
    d = U.inputs("Adam-n4099-zero")
    assert all(not g[3::5].any() and g[0::5].all() for g in d.g)       # exactly-zero gradients while v == 0


def test_case_table_covers_the_paths_the_issue_names():
    cs = U.cases()
    lay = U.lamb_layouts()
    assert len(lay["model301"]) == 301 and sum(lay["model301"]) < 1_000_000 and max(lay["model301"]) > 10 * U.LAMB_CHUNK
    assert len(lay["t1025"]) == U.SUMSQ_BLOCKS + 1 and len(lay["t1024"]) == U.SUMSQ_BLOCKS and max(lay["t1025"]) <= 9
    assert sum(lay["big3"]) // 4 > 2 * U.SUMSQ_BLOCKS * 256 and lay["big3"][0] > 500 * U.LAMB_CHUNK        # two loads in flight in sumsq_kernel
    assert U.ADAM_BIG // 4 + 1 > 256 * 16 * 256 and U.ADAM_BIG % 4 == 2                                   # the grid cap of ew_blocks2
    assert {c.n for c in cs.values() if c.family == "adam"} == set(U.ADAM_SIZES)
    for kind in ("Adam", "AdamW"):
        assert {(c.wd, c.grad_scale) for c in cs.values() if c.kind == kind} >= {(w, s) for w in U.WDS for s in U.SCALES}
        assert {s for c in cs.values() if c.kind == kind for s in c.steps} >= {1, 2, 3, 1000, 100000}


# ------------------------------------------------------------------------------------------------------------------ references inside the bounds
@pytest.mark.parametrize("name", list(U.cases()))
def test_float32_references_stay_inside_the_bounds(name):
    """The float32 oracle and the float32 restatement of the kernel on every GPU case: inside the bounds, the restatement within EMUL_UNITS
    of the moment bounds, and neither needs more than R_MEASURED (so R = 4 x R_MEASURED is what util_optim.py says it is)."""
    kind = U.cases()[name].kind
    eo, ee = U.run_case(name, U.oracle_stepper), U.run_case(name, U.emul_stepper())
    print(f"{name}: oracle m {eo[0]:.2f} v {eo[1]:.2f} R {eo[2]:.3e} | restatement m {ee[0]:.2f} v {ee[1]:.2f} R {ee[2]:.3e}")
    assert U.within_bounds(eo, kind) and U.within_bounds(ee, kind)
    assert max(ee[0], ee[1]) <= U.EMUL_UNITS
    assert max(eo[2], ee[2]) <= U.R_MEASURED[kind]


# ------------------------------------------------------------------------------------------------------------------ mutants
# mutant -> the case of the table that catches it (others do too; one is named and asserted)
MUTANTS = {
    "drop_tail": "t130-clip",                    # clip norm without the last n % 4 elements: gr off by 1 / sqrt(2) -> m, v
    "unscaled_norm": "t65-gs.25",                # clip norm from the unscaled gradient: clips by 3 where the scaled norm is 0.75 -> m, v
    "neighbour_chunk": "eight-noclip",           # tensor t's norms include the first chunk of tensor t + 1 -> trust ratio -> delta
    "skip_4096": "eight-clip",                   # chunk size off by one: element 4096 of a tensor skipped -> m, v, delta of that element
    "bias_step_minus_1": "t1024-resume",         # bias correction with step - 1: 3e-4 of the update at step 1000 -> delta
    "ratio_at_wd0": "t65-wd0",                   # trust ratio applied at wd == 0 -> delta
    "decay_after": "AdamW-n4099-large_lr",       # AdamW decay after instead of before the update: lr * wd of the update -> delta
    "l2_not_in_v": "Adam-n4099-wd1e-06-gs0.5",   # Adam's L2 term not folded into v -> v
}


@pytest.mark.parametrize("mutant,name", list(MUTANTS.items()))
def test_mutants_violate_the_bounds(mutant, name):
    kind = U.cases()[name].kind
    good, bad = U.run_case(name, U.emul_stepper()), U.run_case(name, U.emul_stepper(mutant))
    print(f"{mutant} on {name}: m {bad[0]:.3g} v {bad[1]:.3g} units, R {bad[2]:.3g} (bound {U.R[kind]:.3g}); unmutated {good}")
    assert U.within_bounds(good, kind)
    assert not U.within_bounds(bad, kind)


def test_bias_correction_mutant_is_caught_for_adam_at_a_large_step_too():
    """step - 1 at step 1000 changes the update by 1e-4: invisible to a parameter check at rtol 2e-6, 200 x the R bound."""
    for name in ("Adam-n4099-step1000", "AdamW-n4099-step1000"):
        bad = U.run_case(name, U.emul_stepper("bias_step_minus_1"))
        assert bad[0] <= U.M_UNITS and bad[1] <= U.V_UNITS and 100 * U.R[U.cases()[name].kind] < bad[2] < 1e-3


def _old_lamb_inputs():
    """The data of test_kernels_gpu.py::test_lamb_matches_oracle (wd = 1e-2)."""
    sizes = [1000, 7, 4096, 33, 10001]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    rnd = lambda seed, scale: torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale  # noqa: E731
    p0, g = rnd(1, 1.0), rnd(2, 3.0)
    p0[offs[1]:offs[2]] = 0.0
    return sizes, offs, p0.numpy(), [(g / s).numpy() for s in (1, 2, 3)]


# what test_lamb_matches_oracle's comparison does with each LAMB mutant on that test's own inputs, per weight decay of its two parametrizations
# (measured here, asserted below): "accepts" a wrong result, "rejects" it, or is "blind" (its inputs cannot express the mistake: the
# mutant's result is the correct one there)
OLD_CHECK = {
    "drop_tail": {1e-2: "accepts", 0.0: "accepts"},
    "unscaled_norm": {1e-2: "blind", 0.0: "blind"},          # grad_scale is always 1
    "neighbour_chunk": {1e-2: "rejects", 0.0: "blind"},      # no trust ratio at wd == 0: the norms are not used
    "skip_4096": {1e-2: "rejects", 0.0: "rejects"},
    "bias_step_minus_1": {1e-2: "rejects", 0.0: "rejects"},
    "ratio_at_wd0": {1e-2: "blind", 0.0: "rejects"},
}


@pytest.mark.parametrize("wd", [1e-2, 0.0])
def test_what_the_parameter_only_check_accepts(wd):
    """test_lamb_matches_oracle's comparison (three compounding steps, p only, rtol 2e-5 / atol 2e-6 against the float32 oracle), applied to
    the mutants on that test's own inputs (OLD_CHECK).

    It ACCEPTS the clip norm without the last n % 4 elements: one element of 15 137, the clip factor and both moments are off by 3e-5
    (500 units of the moment bounds), and with a clip that is always active m / sqrt(v) hardly depends on the clip factor at all; the error
    reaches 5 % of its tolerance.  It is BLIND to a clip norm of the unscaled gradient (grad_scale is 1), and at wd == 0 to everything about
    the per-tensor norms; it never looks at m or v.  It REJECTS norms that include the neighbouring tensor's first chunk at wd = 1e-2 (the
    7-element zero-weight tensor gains a trust ratio; 9000 x the tolerance), the skipped element 4096 and the bias correction with step - 1:
    on this table a parameter check is not as weak against a misplaced chunk as one might fear, but only because its tensors are few and tiny.
    The bounds of util_optim.py reject every mutant that is wrong on these inputs, at the first step it is wrong in, and the case table
    leaves none of them blind (test_mutants_violate_the_bounds)."""
    sizes, offs, p0, gs = _old_lamb_inputs()
    c = U.types.SimpleNamespace(family="lamb", kind="LAMB", offsets=offs, wd=wd, eps=1e-6, max_grad_norm=1.0, grad_scale=1.0)
    z = np.zeros_like(p0)

    def chain(stepper):
        p, m, v = p0, z, z
        out = []
        for s in (1, 2, 3):
            p, m, v = stepper(c, p, gs[s - 1], m, v, 1e-2, s)
            out.append(p)
        return out

    def old_check(got, ref):
        with np.errstate(invalid="ignore"):
            return all(bool(np.all(np.abs(p - pr) <= 2e-6 + 2e-5 * np.abs(pr))) for p, pr in zip(got, ref))       # assert_allclose's criterion

    def new_check(stepper):
        p, m, v = p0, z, z
        for s in (1, 2, 3):
            ref = U.reference(c, p, gs[s - 1], m, v, 1e-2, s)
            p1, m1, v1 = stepper(c, p, gs[s - 1], m, v, 1e-2, s)
            if not U.within_bounds(U.judge(ref, p, m, v, p1, m1, v1), "LAMB"):
                return False
            p, m, v = p1, m1, v1
        return True

    oracle, good = chain(U.oracle_stepper), chain(U.emul_stepper())
    assert old_check(good, oracle) and new_check(U.emul_stepper()) and new_check(U.oracle_stepper)
    for mutant, verdicts in OLD_CHECK.items():
        got = chain(U.emul_stepper(mutant))
        same = all(np.array_equal(a, b) for a, b in zip(got, good))
        verdict = "blind" if same else "accepts" if old_check(got, oracle) else "rejects"
        assert verdict == verdicts[wd], f"{mutant} at wd = {wd}: the parameter-only check {verdict}"
        assert new_check(U.emul_stepper(mutant)) == same, f"{mutant} at wd = {wd}: the new bounds and the result disagree"
