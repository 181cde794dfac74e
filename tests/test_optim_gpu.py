"""The optimizer on the device against float64: dc_adam_step and dc_lamb_step through the C ABI on the case table of util_optim.py (every
step judged against the float64 reference applied to the kernel's own previous state: both moments and the parameter change inside
the bounds derived there, guards behind every arena untouched, the gradient arena bit-identical), the argument checks, the two paths of
dc_lamb_step bit for bit, and the ArenaOptimizer wrapper: state-dict layout, resume on the uninterrupted trajectory, interchange with
torch.optim, a step-0 state into a used optimizer.  test_optim_cpu.py holds the preconditions (the float32 references stay inside the same
bounds; eight wrong restatements do not)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import util_optim as U  # noqa: E402
from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
from oracle import loss_metric as olm  # noqa: E402
from util_inputs import make_inputs  # noqa: E402

GUARD = 64                       # words in front of and behind every arena
SENTINEL = 0x7FC0DEAD            # a quiet NaN with a recognisable payload
KIND = {"Adam": L.DC_ADAM, "AdamW": L.DC_ADAMW}


def dev():
    return torch.device("cuda", 0)


def S():
    return L.stream_ptr()


class Arena:
    """n float32 words between two guards of GUARD sentinel words; the arena starts 16-byte aligned and ends wherever n ends."""

    def __init__(self, n, data=None):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
        self.view = self.buf[GUARD:GUARD + n].view(torch.float32)
        assert self.view.data_ptr() % 16 == 0
        if data is not None:
            self.put(data)

    def put(self, data):
        self.view.copy_(torch.from_numpy(np.array(data, dtype=np.float32)))       # a copy: the cases' inputs are read-only

    def get(self):
        return self.view.cpu().numpy()

    def ptr(self, byte_offset=0):
        return C.c_void_p(self.view.data_ptr() + byte_offset)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def bits(self):
        return self.buf.clone()


class KernelStepper:
    """The device side of util_optim.run_case for one case: arenas behind guards, the LAMB workspace at exactly dc_lamb_workspace_words, the
    learning rate and the step count in device scalars that change between the steps."""

    def __init__(self, c):
        self.c = c
        self.arenas = {k: Arena(c.n) for k in "pgmv"}
        self.lr = torch.zeros(1, device=dev())
        self.step = torch.zeros(1, dtype=torch.int32, device=dev())
        self.started = False
        if c.family == "lamb":
            self.offs = torch.from_numpy(np.asarray(c.offsets, dtype=np.int64)).to(dev())
            words = L.load().dc_lamb_workspace_words(len(c.sizes), c.n)
            self.ws = Arena(int(words))
            zw, zz = U.special_tensors(len(c.sizes))
            self.zero = None if zz is None else slice(int(c.offsets[zz]), int(c.offsets[zz + 1]))

    def __call__(self, c, p, g, m, v, lr, step):
        a = self.arenas
        if not self.started:            # later steps continue from what the kernel left on the device
            a["p"].put(p), a["m"].put(m), a["v"].put(v)
            self.started = True
        a["g"].put(g)
        g_before = a["g"].bits()
        self.lr.fill_(lr)
        self.step.fill_(step)
        ptr = [a[k].ptr() for k in "pgmv"]
        if c.family == "lamb":
            L.call("dc_lamb_step", len(c.sizes), C.c_void_p(self.offs.data_ptr()), c.n, *ptr, C.c_void_p(self.lr.data_ptr()), U.B1, U.B2, c.eps,
                   c.wd, C.c_void_p(self.step.data_ptr()), c.max_grad_norm, c.grad_scale, self.ws.ptr(), S())
        else:
            L.call("dc_adam_step", KIND[c.kind], c.n, *ptr, C.c_void_p(self.lr.data_ptr()), U.B1, U.B2, c.eps, c.wd,
                   C.c_void_p(self.step.data_ptr()), c.grad_scale, S())
        torch.cuda.synchronize()
        for k, ar in a.items():
            assert ar.guards_intact(), f"{c.name} step {step}: a store outside the {k} arena"
        assert torch.equal(a["g"].bits(), g_before), f"{c.name} step {step}: the gradient arena was written"
        p1, m1, v1 = a["p"].get(), a["m"].get(), a["v"].get()
        assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all(), f"{c.name} step {step}: not finite"
        if c.family == "lamb":
            assert self.ws.guards_intact(), f"{c.name} step {step}: a store past dc_lamb_workspace_words"
            if self.zero is not None:   # zero weights, zero gradients, zero moments: nothing may move
                assert not p1[self.zero].any() and not m1[self.zero].any() and not v1[self.zero].any(), f"{c.name}: the all-zero tensor moved"
        return p1, m1, v1


def _run(name):
    c = U.cases()[name]
    em, ev, r = U.run_case(name, KernelStepper(c))
    print(f"{name}: m {em:.2f} v {ev:.2f} units (bound {U.M_UNITS:g}), R {r:.3e} (bound {U.R[c.kind]:.3e})")
    assert em <= U.M_UNITS, f"{name}: first moment off by {em:.3g} units of 2^-24 (|m_prev| + |gr|), bound {U.M_UNITS:g}"
    assert ev <= U.V_UNITS, f"{name}: second moment off by {ev:.3g} units of 2^-24 (v_prev + gr^2), bound {U.V_UNITS:g}"
    assert r <= U.R[c.kind], f"{name}: the parameter change needs R = {r:.3e}, bound {U.R[c.kind]:.3e}"
    return c


@pytest.mark.parametrize("name", U.names("adam"))
def test_adam_step_within_bounds_of_float64(name):
    c = _run(name)
    # the project's parameter-level check (test_adam_matches_torch_optim's tolerance) as a second assertion: one step from the case's state
    d = U.inputs(name)
    st = KernelStepper(c)
    p1, _, _ = st(c, d.p, d.g[0], d.m, d.v, c.lrs[0], c.steps[0])
    ref = U.reference(c, d.p, d.g[0], d.m, d.v, c.lrs[0], c.steps[0])
    np.testing.assert_allclose(p1, ref.p, rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("name", U.names("lamb"))
def test_lamb_step_within_bounds_of_float64(name):
    _run(name)


# ------------------------------------------------------------------------------------------------------------------ argument checks
def _refused(name, args, arenas):
    """The entry point returns an error whose text names it, and launches nothing: every arena keeps its bits."""
    before = [a.bits() for a in arenas]
    rc = getattr(L.load(), name)(*args)
    torch.cuda.synchronize()
    assert rc != 0, f"{name} accepted a bad argument"
    assert name in L.last_error(), L.last_error()
    for a, b in zip(arenas, before):
        assert torch.equal(a.bits(), b), f"{name} refused the call but wrote to an arena"


def _variants(good, pointer_slots, arena_slots):
    """argument lists with one pointer null, then with one arena 4 bytes off its 16-byte alignment"""
    for i in pointer_slots:
        yield f"null argument {i}", good[:i] + [C.c_void_p(0)] + good[i + 1:]
    for i in arena_slots:
        yield f"misaligned argument {i}", good[:i] + [C.c_void_p(good[i].value + 4)] + good[i + 1:]


def test_adam_step_refuses_bad_arguments():
    n = 1024
    rs = np.random.RandomState(0)
    ar = [Arena(n, rs.standard_normal(n).astype(np.float32)) for _ in range(4)]
    lr, step = torch.full((1,), 1e-3, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())
    good = [L.DC_ADAMW, n] + [a.ptr() for a in ar] + [C.c_void_p(lr.data_ptr()), 0.9, 0.999, 1e-8, 1e-2, C.c_void_p(step.data_ptr()), 1.0, S()]
    for what, args in _variants(good, (2, 3, 4, 5, 6, 11), (2, 3, 4, 5)):
        _refused("dc_adam_step", args, ar)
    for kind in (L.DC_LAMB, -1, 7):
        _refused("dc_adam_step", [kind] + good[1:], ar)
    for bad_n in (0, -4):
        _refused("dc_adam_step", good[:1] + [bad_n] + good[2:], ar)
    L.call("dc_adam_step", *good)         # and the good call is accepted
    torch.cuda.synchronize()
    assert all(a.guards_intact() for a in ar)


def test_lamb_step_refuses_bad_arguments():
    sizes = [1000, 7, 4097]
    offs_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs_h[-1])
    rs = np.random.RandomState(0)
    ar = [Arena(n, rs.standard_normal(n).astype(np.float32)) for _ in range(4)]
    ws = Arena(int(L.load().dc_lamb_workspace_words(len(sizes), n)))
    offs = torch.from_numpy(offs_h).to(dev())
    lr, step = torch.full((1,), 1e-3, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())
    good = [len(sizes), C.c_void_p(offs.data_ptr()), n] + [a.ptr() for a in ar] + [C.c_void_p(lr.data_ptr()), 0.9, 0.999, 1e-6, 1e-2,
                                                                                 C.c_void_p(step.data_ptr()), 1.0, 1.0, ws.ptr(), S()]
    for what, args in _variants(good, (1, 3, 4, 5, 6, 7, 12, 15), (3, 4, 5, 6, 15)):
        _refused("dc_lamb_step", args, ar + [ws])
    for nt in (0, -1):
        _refused("dc_lamb_step", [nt] + good[1:], ar + [ws])
    _refused("dc_lamb_step", good[:2] + [0] + good[3:], ar + [ws])
    L.call("dc_lamb_step", *good)
    torch.cuda.synchronize()
    assert all(a.guards_intact() for a in ar + [ws])


# ------------------------------------------------------------------------------------------------------------------ the two paths of dc_lamb_step
def test_lamb_ratio_kernel_and_stage2_sum_give_the_same_bits():
    """1024 tensors: lamb_ratio_kernel writes the step sizes; the same arena with one more 1-element tensor (zero weight, zero gradient):
    lamb_stage2_kernel sums the chunk norms itself, "the same bits".  The gradients are multiples of 1/64 up to 1/8, so the sum of their
    squares is exact in fp32 in any order and the clip factor (active: ||g * grad_scale|| ~ 3.7) cannot differ between the two arena
    lengths."""
    sizes = U.lamb_layouts()["t1024"]
    offs, p, _ = U.lamb_inputs(sizes, 11, 1.0)
    n = int(offs[-1])
    rs = np.random.RandomState(12)
    g = (rs.randint(-8, 9, n) / 64.0).astype(np.float32)
    m, v = U.moments_like(g, offs, 13)
    out = []
    for extra in (0, 1):
        z = np.zeros(extra, dtype=np.float32)
        ar = [Arena(n + extra, np.concatenate([x, z])) for x in (p, g, m, v)]
        nt = len(sizes) + extra
        o = torch.from_numpy(np.concatenate([offs, [n + 1]][:1 + extra]).astype(np.int64)).to(dev())
        ws = Arena(int(L.load().dc_lamb_workspace_words(nt, n + extra)))
        lr, step = torch.full((1,), 1e-2, device=dev()), torch.full((1,), 5, dtype=torch.int32, device=dev())
        L.call("dc_lamb_step", nt, C.c_void_p(o.data_ptr()), n + extra, *[a.ptr() for a in ar], C.c_void_p(lr.data_ptr()), 0.9, 0.999, 1e-6, 1e-2,
               C.c_void_p(step.data_ptr()), 1.0, 0.5, ws.ptr(), S())
        torch.cuda.synchronize()
        assert all(a.guards_intact() for a in ar + [ws])
        out.append([a.view[:n].view(torch.int32).clone() for a in (ar[0], ar[2], ar[3])])
        if extra:
            assert float(ar[0].view[n]) == 0.0
    assert not torch.equal(out[0][0], torch.from_numpy(p).view(torch.int32).to(dev()))      # the step did something
    for a, b, what in zip(out[0], out[1], ("p", "m", "v")):
        assert torch.equal(a, b), f"{what} differs between the lamb_ratio_kernel path and the stage-2 sum"


# ------------------------------------------------------------------------------------------------------------------ wrapper and resume
B, H, W = 2, 64, 96
CW = olm.class_weights(-0.125)
LR0, LR1 = 1e-3, 5e-4            # a schedule lowers the rate before step 4


def _model(optname, dtype, seed=333):
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=dtype, seed=seed)
    net.materialize(B, H, W)
    net.train()
    opt = dnn.make_optimizer(optname, net, LR0, 1e-8, 1e-2)
    return net, opt, dnn.TrainStep(net, opt, CW, B, H, W, with_metrics=True)


def _batch(i):
    x, y = make_inputs(B, H, W, seed=100 + i)
    return x.to(dev()), y.to(dev())


def _steps(step, first, last):
    for i in range(first, last + 1):
        step(*_batch(i))
        torch.cuda.synchronize()


def _snapshot(net, opt, step):
    e = net.engine
    return dict(params=e.params.clone(), buffers=e.buffers.clone(), m=opt.m.clone(), v=opt.v.clone(), step_count=opt.step_count,
                lr=opt.param_groups[0]["lr"], loss=step.loss())


def _same(a, b, what):
    for k in ("params", "buffers", "m", "v"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"
    assert a["step_count"] == b["step_count"] and a["lr"] == b["lr"], what
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(a["loss"]), f"{what}: loss {a['loss']!r} vs {b['loss']!r}"     # an fp64 atomic sum


@pytest.mark.parametrize("optname", ["LAMB", "AdamW"])
def test_state_dict_layout(optname):
    net, opt, step = _model(optname, torch.bfloat16)
    sd0 = opt.state_dict()
    assert sd0["state"] == {} and sd0["param_groups"][0]["lr"] == LR0
    _steps(step, 1, 3)
    opt.param_groups[0]["lr"] = LR1
    sd = opt.state_dict()
    lay = net.engine.layout
    assert len(lay.params) == 301 and sorted(sd["state"]) == list(range(301))
    assert sd["param_groups"][0]["lr"] == LR1 and sd["param_groups"][0]["params"] == list(range(301))
    for (i, s), p, info in zip(sorted(sd["state"].items()), net.parameters(), lay.params.values()):
        assert float(s["step"]) == 3.0
        assert tuple(s["exp_avg"].shape) == tuple(s["exp_avg_sq"].shape) == tuple(p.shape) == tuple(info.shape), info.name
        assert p.data_ptr() == net.engine.params.data_ptr() + 4 * info.offset, f"{info.name}: net.parameters() is not in layout order"
    for key, arena in (("exp_avg", opt.m), ("exp_avg_sq", opt.v)):
        cat = torch.cat([sd["state"][i][key].reshape(-1) for i in range(301)])
        assert torch.equal(cat.view(torch.int32), arena.view(torch.int32)), key
    assert bool(opt.m.any()) and bool((opt.v >= 0).all())


@pytest.mark.parametrize("optname,dtype", [("LAMB", torch.bfloat16), ("AdamW", torch.float32)], ids=["LAMB-bf16", "AdamW-f32"])
def test_resume_equals_the_uninterrupted_run(optname, dtype, tmp_path):
    """Five steps in one run against three steps, a checkpoint through torch.save / torch.load, and two steps in a model built with ANOTHER
    seed: parameters, BatchNorm buffers, both moments bit for bit, step count and learning rate equal, after each of steps 4 and 5."""
    net, opt, step = _model(optname, dtype)
    _steps(step, 1, 3)
    opt.param_groups[0]["lr"] = LR1
    want = []
    for i in (4, 5):
        _steps(step, i, i)
        want.append(_snapshot(net, opt, step))

    net, opt, step = _model(optname, dtype)
    _steps(step, 1, 3)
    path = str(tmp_path / "ck.pt")
    torch.save({"model": {"module." + k: v for k, v in net.state_dict().items()}, "optimizer": opt.state_dict()}, path)   # train.py's keys
    ck = torch.load(path, weights_only=False)

    net, opt, step = _model(optname, dtype, seed=7)
    assert not torch.equal(net.engine.params, want[0]["params"])
    net.load_state_dict(ck["model"])
    opt.load_state_dict(ck["optimizer"])
    assert opt.step_count == 3 and opt.param_groups[0]["lr"] == LR0
    opt.param_groups[0]["lr"] = LR1
    for k, i in enumerate((4, 5)):
        _steps(step, i, i)
        _same(_snapshot(net, opt, step), want[k], f"{optname} step {i} after resume")


def test_state_dict_interchanges_with_torch_optim():
    """AdamW, fp32: torch.optim.AdamW over CPU clones of the parameters accepts ArenaOptimizer.state_dict(); its next step on the engine's
    gradient arena matches the engine's own next step; its state_dict() loads into a fresh ArenaOptimizer, with integer or string keys."""
    net, opt, step = _model("AdamW", torch.float32)
    _steps(step, 1, 2)
    eng, lay = net.engine, net.engine.layout
    cpu_p = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
    ref = torch.optim.AdamW(cpu_p, lr=LR0, eps=1e-8, weight_decay=1e-2)
    ref.load_state_dict(opt.state_dict())
    assert ref.param_groups[0]["lr"] == LR0 and len(ref.state) == 301
    grads = eng.grads.cpu()
    for p, info in zip(cpu_p, lay.params.values()):
        p.grad = grads[info.offset:info.offset + p.numel()].view(p.shape).clone()

    # the other direction first (both optimizers hold the state after two steps)
    for keys in (int, str):
        sd = ref.state_dict()
        sd["state"] = {keys(k): v for k, v in sd["state"].items()}
        fresh = dnn.make_optimizer("AdamW", net, 0.5, 1e-8, 0.0)
        fresh.load_state_dict(sd)
        assert fresh.step_count == opt.step_count == 2
        assert torch.equal(fresh.m, opt.m) and torch.equal(fresh.v, opt.v)
        assert fresh.param_groups[0]["lr"] == LR0 and fresh.param_groups[0]["weight_decay"] == 1e-2

    m_prev = opt.m.cpu().numpy().astype(np.float64)
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    got = eng.params.cpu().numpy()
    exp = np.concatenate([p.detach().numpy().reshape(-1) for p in cpu_p])
    np.testing.assert_allclose(got, exp, rtol=2e-6, atol=2e-7)
    st = ref.state_dict()["state"]
    assert float(st[0]["step"]) == 3.0 == float(opt.state_dict()["state"][0]["step"])
    # the first moment too: both are fp32 evaluations within util_optim's 8 units of the exact one, each on the scale |m_prev| + |g|
    m_ref = np.concatenate([st[i]["exp_avg"].numpy().reshape(-1) for i in range(301)]).astype(np.float64)
    err = U._units(np.abs(opt.m.cpu().numpy() - m_ref), U.U24 * (np.abs(m_prev) + np.abs(grads.numpy().astype(np.float64))))
    assert err <= 2 * U.M_UNITS, f"first moment: {err:.3g} units"


@pytest.mark.parametrize("optname", ["LAMB", "AdamW"])
def test_step0_state_into_a_used_optimizer(optname):
    """A step-0 checkpoint ({"state": {}}) loaded into an optimizer that has stepped: torch.optim drops the moments, so the next step must be
    the FIRST step of a fresh optimizer on the same weights and gradient, bit for bit."""
    net, opt, step = _model(optname, torch.bfloat16)
    _steps(step, 1, 2)
    eng = net.engine
    weights, grads = eng.params.clone(), eng.grads.clone()
    assert bool(opt.m.any()) and opt.step_count == 2
    fresh = dnn.make_optimizer(optname, net, LR0, 1e-8, 1e-2)
    opt.load_state_dict({"state": {}, "param_groups": fresh.state_dict()["param_groups"]})
    assert opt.step_count == 0
    opt.step()
    torch.cuda.synchronize()
    got = dict(p=eng.params.clone(), m=opt.m.clone(), v=opt.v.clone())
    eng.params.copy_(weights)
    assert torch.equal(eng.grads, grads)
    fresh.step()
    torch.cuda.synchronize()
    for k, t in (("p", eng.params), ("m", fresh.m), ("v", fresh.v)):
        assert torch.equal(got[k].view(torch.int32), t.view(torch.int32)), f"{optname}: {k} after a step-0 state differs from a fresh optimizer's first step"
    assert opt.step_count == fresh.step_count == 1
