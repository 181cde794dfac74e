"""The view ensemble on the GPU (dc_input_view_hwc, dc_ensemble_add, dc_ensemble_pool of csrc/ensemble.hip; nn.ViewEnsemble,
nn.view_input; predict.py --ensemble_*) against the numpy checker of tests/util_ensemble.py.  From q = rint(p * 65536) on the state is
integers: every comparison of it is equality.  The device rounds in fp32, the checker in float64, so the constructed logits stand clear of
every rounding boundary (asserted on the CPU first, in util_decide.clear_triples / smooth_logits); only the tests whose logits come from a
network treat the pixels near a boundary apart.
The shapes come from the kernels' own constant.  With P from dc_ensemble_block and W = 64 (16-byte accesses) or W = 10 (4-byte accesses):
"one" is a sample of at most P pixels, one workgroup; "two" is exactly 2 P pixels; "ragged" is two workgroups, the second ending inside
a pass, with an odd number of rows.  Batch 3 with 2 valid samples; the padding sample has NaN logits, and its words of the state and the
guard words around the state must stay as they were."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlperf_deepcam_amd import lib as L  # noqa: E402
from mlperf_deepcam_amd import nn as dnn  # noqa: E402
import util_decide as ud  # noqa: E402
import util_ensemble as ue  # noqa: E402
import util_prob as up  # noqa: E402
import util_val  # noqa: E402
from util_launch import served, assert_served  # noqa: E402

DEV = torch.device("cuda", 0)
B, NV = 3, 2
GUARD, SENTINEL = 64, 0x5A5A5A5A
ONE = 65536
MARGIN = 4


@functools.lru_cache(maxsize=None)
def _block():
    px = C.c_int(0)
    assert L.load().dc_ensemble_block(C.byref(px)) == 0 and px.value >= 1024 and px.value % 64 == 0
    return px.value


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(H, W)"""
    P = _block()
    kind, W = name.split("-")
    W = int(W)
    if kind == "one":
        H = P // W
        assert H * W <= P
    elif kind == "two":
        H = 2 * P // W
        assert H * W == 2 * P
    else:
        H = (2 * P // W - 3) | 1
        assert P < H * W < 2 * P and (H * W) % 1024 != 0 and H % 2 == 1
    return H, W


def _views(W, M):
    """M views (roll, flip, weighted): shifts that are multiples of 4 and shifts that are not, flips, seam weights and none"""
    rolls = [0, W // 2, 17 % W, W - 1, 4][:M] if W % 4 == 0 else [0, W // 2, 7 % W, W - 1, 4][:M]
    return [(r, bool(k % 3 == 2 or k == 4), k % 2 == 1) for k, r in enumerate(rolls)]


def _weights(W, roll, weighted):
    return ue.seam_weights(W, roll, MARGIN) if weighted else None


def _scene(rs, H, W):
    """(q1, q2) int64 [H, W] in source coordinates: util_decide.smooth_logits' field with its bumps doubled, so that every class is the
    most probable one somewhere (the original keeps both foreground classes below a half)"""
    q = ud.smooth_logits(rs, H, W, blobs=12)[1]
    q1 = np.minimum(2 * q[1], 60000)
    return q1, np.clip(2 * q[2], 1, 65534 - q1)


def _member_of(rs, scene, roll, flip):
    """logits float32 [3, H, W] in the coordinates of the view: what a member sees of the scene, with noise of its own, as exact integer
    triples clear of every rounding boundary (util_decide.clear_triples asserts it)"""
    q1 = np.clip(scene[0] + rs.randint(-2000, 2001, size=scene[0].shape), 1, 60000)
    q2 = np.clip(scene[1] + rs.randint(-2000, 2001, size=scene[1].shape), 1, 65534 - q1)
    return ud.clear_triples(ue.to_view(q1, roll, flip), ue.to_view(q2, roll, flip))


@functools.lru_cache(maxsize=None)
def _members(shape, M):
    """M members of a batch, each (logits float32 [B, 3, H, W] -- the padding frame NaN --, roll, flip, weights): per frame one scene,
    seen by every member in its own view.  Shared, never modified."""
    H, W = _shape(shape)
    rs = np.random.RandomState(1000 + 7 * H + M)
    scenes = [_scene(rs, H, W) for _ in range(NV)]
    out = []
    for roll, flip, weighted in _views(W, M):
        logits = np.full((B, 3, H, W), np.nan, np.float32)
        for b in range(NV):
            logits[b] = _member_of(rs, scenes[b], roll, flip)
        logits.setflags(write=False)
        out.append((logits, roll, flip, _weights(W, roll, weighted)))
    return out


def _frame_members(members, b):
    return [(lg[b], roll, flip, wt) for lg, roll, flip, wt in members]


@functools.lru_cache(maxsize=None)
def _reference(shape, M):
    """the checker's (state, L, top, rows) of the valid frames of _members(shape, M)"""
    return [ue.frame(_frame_members(_members(shape, M), b)) for b in range(NV)]


def _device_weights(wt):
    return None if wt is None else torch.from_numpy(wt.view(np.int16).copy()).to(DEV)


def _add_all(members, H, W, n_valid=NV):
    """dc_ensemble_add of every member on a guarded, DIRTY state: (state uint32 [B, 4, H, W] on the host, the launch names).  Asserts that
    the guards and the padding samples' words are untouched."""
    n = B * 4 * H * W
    store = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    state = store[GUARD:GUARD + n]
    keep = []
    with served("dc_ensemble_add") as names:
        for m, (logits, roll, flip, wt) in enumerate(members):
            lg, dw = torch.from_numpy(np.array(logits, np.float32, order="C")).to(DEV), _device_weights(wt)
            keep += [lg, dw]
            L.call("dc_ensemble_add", B, n_valid, H, W, L.dptr(lg), roll, int(flip), L.dptr(dw), m, L.dptr(state), L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((store[:GUARD] == SENTINEL).all()) and bool((store[-GUARD:] == SENTINEL).all()), "a guard word was written"
    words = state.cpu().numpy().view(np.uint32).reshape(B, 4, H, W)
    assert (words[n_valid:] == SENTINEL).all(), "a padding sample's state was written"
    return words, names


def _expected_names(members, W):
    return ["ensemble_add_vec" if W % 4 == 0 and roll % 4 == 0 else "ensemble_add" for _, roll, _, _ in members]


# ------------------------------------------------------------------------------------------------------------------ 1. the view of the input
def _normalize(dtype, raw, channels, shift, scale, C_):
    """dc_input_normalize_hwc of a raw batch [N, H, W, Cfile]"""
    N, H, W, cfile = raw.shape
    out = torch.empty((N, H, W, C_), dtype=dtype, device=DEV)
    L.call("dc_input_normalize_hwc", L.dtype_code(dtype), N * H * W, cfile, C_, L.dptr(channels), L.dptr(raw), L.dptr(shift), L.dptr(scale),
           L.dptr(out), C_, L.stream_ptr())
    return out


@pytest.mark.parametrize("subset", [False, True], ids=["all16", "subset8"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(5, 12), (8, 64)])
def test_view_is_the_normalisation_of_the_rolled_mirrored_negated_fields(H, W, dtype, subset):
    g = torch.Generator().manual_seed(11 + H)
    cfile = 16
    raw = ((torch.rand(B, H, W, cfile, generator=g) * torch.linspace(1, 300, cfile) - 40.0)).to(DEV)
    file_channels = [1, 2, 4, 7, 8, 11, 13, 15] if subset else list(range(cfile))
    C_ = len(file_channels)
    channels = torch.tensor(file_channels, dtype=torch.int32, device=DEV) if subset else None
    shift = (torch.rand(C_, generator=g) * 50 - 40).to(DEV)
    scale = (1.0 / (torch.rand(C_, generator=g) * 300 + 1)).to(DEV)
    negate = [4, 13]                                                              # file channels
    sign_file = torch.ones(cfile, device=DEV)
    sign_file[negate] = -1.0
    # the identity view is the existing kernel's bits
    with served("identity view") as names:
        ident = dnn.view_input(raw, channels, shift, scale, 0, False, None, dtype=dtype)
    assert_served(names, "view_normalize")
    assert ident.dtype == dtype and tuple(ident.shape) == (B, H, W, C_) and torch.equal(ident, _normalize(dtype, raw, channels, shift, scale, C_))
    out = torch.empty((B, H, W, C_), dtype=dtype, device=DEV)
    for roll in (0, 1, W - 1, W // 2):
        for flip in (False, True):
            for neg in (None, negate):
                moved = torch.roll(raw.flip(1) if flip else raw, -roll, dims=2)          # moved[n, h, w] = raw[n, src(h, w)]
                if neg is not None:
                    moved = moved * sign_file
                want = _normalize(dtype, moved.contiguous(), channels, shift, scale, C_)
                with served("view") as names:
                    got = dnn.view_input(raw, channels, shift, scale, roll, flip, neg, out)
                assert_served(names, "view_normalize")
                assert got.data_ptr() == out.data_ptr() and torch.equal(got, want), (roll, flip, neg)
                if neg is not None and (roll, flip) == (1, True):                 # the definition itself, in float64
                    ref = ue.view_input(raw.cpu().numpy(), file_channels, sign_file.cpu().numpy()[file_channels], shift.cpu().numpy(),
                                        scale.cpu().numpy(), roll, flip)
                    tol = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22           # relative: bf16's half ulp; fp32's two roundings of 2^-24
                    assert np.allclose(got.float().cpu().numpy(), ref, rtol=tol, atol=1e-12)
    # the sign as a device tensor is the sign as a list of file channels
    sign = sign_file[file_channels].contiguous()
    assert torch.equal(dnn.view_input(raw, channels, shift, scale, 3, True, sign, dtype=dtype), dnn.view_input(raw, channels, shift, scale, 3, True, negate, dtype=dtype))
    bad_calls = [lambda: dnn.view_input(raw, channels, shift, scale, W, False, None, out), lambda: dnn.view_input(raw, channels, shift, scale, -1, False, None, out),
                 lambda: dnn.view_input(raw.cpu(), channels, shift, scale, 0, False, None, out), lambda: dnn.view_input(raw, channels, shift[:-1], scale, 0, False, None, out),
                 lambda: dnn.view_input(raw, channels, shift, scale, 0, False, None, out[:, :, :-1])]
    with served("refused") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
    assert names == []


# ------------------------------------------------------------------------------------------------------------------ 2. members
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("shape", ["one-64", "two-64", "ragged-64", "one-10", "ragged-10"])
def test_state_equals_the_checker(shape, M):
    H, W = _shape(shape)
    members = _members(shape, M)
    words, names = _add_all(members, H, W)
    assert names == _expected_names(members, W)
    if M == 5:                                       # both kernels served the wide shape, the scalar one alone the narrow shape
        assert set(names) == ({"ensemble_add_vec", "ensemble_add"} if W == 64 else {"ensemble_add"})
    ref = _reference(shape, M)
    for b in range(NV):
        assert np.array_equal(words[b], ref[b][0]), (shape, M, b, np.argwhere(words[b] != ref[b][0])[:6].tolist())
    if M == 5:                                       # the fields exercise what they are meant to: disagreement and every class at the top
        S, votes, bad, first = ue.unpack(ref[0][0])
        assert not bad.any() and (votes.max(axis=0) < M).any() and len(np.unique(ref[0][2])) == 3


def test_nothing_valid_launches_nothing_and_bad_arguments_are_refused():
    H, W = 4, 8
    lg = torch.zeros((B, 3, H, W), device=DEV)
    state = torch.full((B, 4, H, W), 7, dtype=torch.int32, device=DEV)
    out = torch.full((B, 3, H, W), 5.0, device=DEV)
    rows, totals, frames = (torch.full(s, 9, dtype=torch.int64, device=DEV) for s in ((B, ue.ROW), (ue.ROW,), (1,)))
    st = L.stream_ptr()
    add = lambda *a: L.call("dc_ensemble_add", *a, st)  # noqa: E731
    pool = lambda *a: L.call("dc_ensemble_pool", *a, st)  # noqa: E731
    bad_calls = [
        lambda: add(B, NV, H, W, L.dptr(lg), W, 0, None, 0, L.dptr(state)), lambda: add(B, NV, H, W, L.dptr(lg), -1, 0, None, 0, L.dptr(state)),
        lambda: add(B, NV, H, W, L.dptr(lg), 0, 2, None, 0, L.dptr(state)), lambda: add(B, NV, H, W, L.dptr(lg), 0, 0, None, 63, L.dptr(state)),
        lambda: add(B, NV, H, W, L.dptr(lg), 0, 0, None, -1, L.dptr(state)), lambda: add(B, B + 1, H, W, L.dptr(lg), 0, 0, None, 0, L.dptr(state)),
        lambda: add(4096, NV, H, W, L.dptr(lg), 0, 0, None, 0, L.dptr(state)), lambda: add(B, NV, H, W, None, 0, 0, None, 0, L.dptr(state)),
        lambda: add(B, NV, 1 << 16, 1 << 15, L.dptr(lg), 0, 0, None, 0, L.dptr(state)),
        lambda: pool(B, NV, H, W, 0, L.dptr(state), L.dptr(out), L.dptr(rows), L.dptr(totals), L.dptr(frames)),
        lambda: pool(B, NV, H, W, 64, L.dptr(state), L.dptr(out), L.dptr(rows), L.dptr(totals), L.dptr(frames)),
        lambda: pool(B, NV, H, W, 1, L.dptr(state), L.dptr(out), None, L.dptr(totals), L.dptr(frames)),
        lambda: pool(B, -1, H, W, 1, L.dptr(state), L.dptr(out), L.dptr(rows), L.dptr(totals), L.dptr(frames)),
    ]
    with served("refused") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
        add(B, 0, H, W, L.dptr(lg), 0, 0, None, 0, L.dptr(state))
        pool(B, 0, H, W, 1, L.dptr(state), L.dptr(out), L.dptr(rows), L.dptr(totals), L.dptr(frames))
    torch.cuda.synchronize()
    assert names == [] and bool((state == 7).all()) and bool((out == 5.0).all())
    assert bool((rows == 9).all()) and bool((totals == 9).all()) and bool((frames == 9).all())


def _spoiled(shape, M):
    """_members with NaN, +inf and -inf in single planes of member 0 and of the last member, at chosen view pixels"""
    H, W = _shape(shape)
    members = [(np.array(lg), roll, flip, wt) for lg, roll, flip, wt in _members(shape, M)]
    spots = []
    for m in (0, M - 1):
        for b in range(NV):
            for k, value in enumerate((np.nan, np.inf, -np.inf)):
                for plane in range(3):
                    r, c = (k + 2 * b + 3 * m) % H, (3 * plane + 11 * k + 7 * b + m) % W
                    members[m][0][b, plane, r, c] = value
                    spots.append((m, b) + ue.source_of(r, c, H, W, members[m][1], members[m][2]))
    return members, spots


@pytest.mark.parametrize("shape", ["ragged-64", "one-10"])
def test_logits_that_are_not_finite_are_counted_and_add_nothing(shape):
    H, W = _shape(shape)
    M = 5
    members, spots = _spoiled(shape, M)
    words, _ = _add_all(members, H, W)
    for b in range(NV):
        ref = ue.frame(_frame_members(members, b))
        assert np.array_equal(words[b], ref[0]), (shape, b)
        S, votes, bad, first = ue.unpack(words[b])
        for m, bb, r, c in spots:
            if bb == b:
                assert bad[r, c] >= 1 and votes[:, r, c].sum() == M - bad[r, c] and (first[r, c] == 3) == any(s == (0, b, r, c) for s in spots)
        assert int(bad.sum()) == 18 and int((bad > 0).sum()) >= 17                # nine pixels of either member, two of them may coincide


def test_sixty_three_members_fill_a_vote_field_without_spilling():
    H, W = 4, 8
    q1 = np.full((H, W), 40000, np.int64)
    frame = ud.clear_triples(q1, np.full((H, W), 5000, np.int64))
    q = up.quantise(frame)
    logits = np.full((B, 3, H, W), np.nan, np.float32)
    logits[:NV] = frame
    members = [(logits, (4 * m) % W, bool(m % 2), None) for m in range(63)]
    words, names = _add_all(members, H, W)
    assert names == ["ensemble_add_vec"] * 63
    for b in range(NV):
        S, votes, bad, first = ue.unpack(words[b])
        assert (votes[1] == 63).all() and not votes[0].any() and not votes[2].any() and not bad.any() and (first == 1).all()
        assert (words[b][3] == (63 << 6 | 1 << 24)).all() and np.array_equal(S, 63 * q)
    ens = dnn.ViewEnsemble(B, H, W, device=DEV)
    lg = torch.from_numpy(logits).to(DEV)
    for m in range(63):
        ens.add(lg, (4 * m) % W, bool(m % 2), n_valid=NV)
    with pytest.raises(L.DeepcamHipError, match="at most 63 members"):
        ens.add(lg, n_valid=NV)
    ens.pool()
    rows = ens.frame_rows().cpu().numpy()
    assert rows.shape == (NV, ue.ROW) and (rows[:, 64 + 63] == H * W).all() and (rows[:, [0, 128]] == H * W).all() and (rows[:, 192 + 5] == H * W).all()
    assert int(rows.sum()) == NV * 4 * H * W and ens.result()["unanimous"] == 1.0 and ens.result()["class_1"]["mean_votes"] == 63.0


# ------------------------------------------------------------------------------------------------------------------ 3. the pool
def _pool(members, H, W, n_valid=NV, ens=None):
    """nn.ViewEnsemble over the members: (pooled logits float32 [n_valid, 3, H, W], rows [n_valid, 208], the object, launch names); the
    padding samples' logits must stay as they were"""
    ens = dnn.ViewEnsemble(B, H, W, device=DEV) if ens is None else ens
    ens.logits_buffer.fill_(-7.0)
    ens.begin()
    with served("ViewEnsemble") as names:
        for logits, roll, flip, wt in members:
            ens.add(torch.from_numpy(np.array(logits, np.float32, order="C")).to(DEV), roll, flip, wt, n_valid=n_valid)
        pooled = ens.pool()
    assert pooled.data_ptr() == ens.logits_buffer.data_ptr() and ens.members == len(members)
    host = pooled.cpu().numpy()
    assert (host[n_valid:] == -7.0).all(), "a padding sample's logits were written"
    return host[:n_valid], ens.frame_rows().cpu().numpy(), ens, names


def _device_q(L_):
    """prob_q of logits float32 [3, n] ON THE DEVICE, through dc_prob_score: every pixel a frame of its own with label 0, whose three
    squared errors are (q_0 - 65536)^2, q_1^2, q_2^2"""
    n = L_.shape[1]
    assert n <= 4095
    skill = dnn.ProbabilitySkill(n, 1, 1, bins=4, device=DEV)
    skill(torch.from_numpy(np.ascontiguousarray(L_.T).reshape(n, 3, 1, 1)).to(DEV), torch.zeros((n, 1, 1), dtype=torch.uint8, device=DEV))
    sq, px = (t.cpu().numpy() for t in skill.frame_rows())
    assert (px[:, 0] == 1).all()
    root = np.rint(np.sqrt(sq.astype(np.float64))).astype(np.int64)
    assert np.array_equal(root * root, sq)
    return np.stack([ONE - root[:, 0], root[:, 1], root[:, 2]])


def _check_pooled(L_, rows, ref, what):
    """one frame's pooled logits and rows against the checker's (state, L, top, rows)"""
    _, want, top, want_rows = ref
    assert rows.dtype == np.int64 and np.array_equal(rows, want_rows), (what, np.flatnonzero(rows != want_rows).tolist())
    finite = top < 3
    assert np.array_equal(np.isnan(L_), np.broadcast_to(~finite[None], L_.shape)), what           # the NaN pattern
    bits = L_.view(np.uint32)
    at_top = np.take_along_axis(bits, np.minimum(top, 2)[None], axis=0)[0]
    assert (at_top[finite] == 0).all(), what                                                      # L_top is +0.0f, bit for bit
    w32 = want.astype(np.float32)
    err = np.abs(L_.astype(np.float64) - w32.astype(np.float64))[:, finite]
    assert (err <= np.spacing(np.abs(w32))[:, finite].astype(np.float64)).all(), (what, float(err.max()))    # within 1 fp32 ulp
    assert np.array_equal(ue.argmax_first(L_[:, finite]), top[finite]), what                       # (P1)


@pytest.mark.parametrize("shape,M", [("one-64", 1), ("two-64", 2), ("ragged-64", 5), ("one-10", 5), ("ragged-10", 2)])
def test_pooled_logits_and_rows_equal_the_checker(shape, M):
    H, W = _shape(shape)
    pooled, rows, ens, names = _pool(_members(shape, M), H, W)
    assert names == _expected_names(_members(shape, M), W) + ["ensemble_pool"]
    ref = _reference(shape, M)
    for b in range(NV):
        _check_pooled(pooled[b], rows[b], ref[b], f"{shape} M={M} frame {b}")
    s = ens.state()
    assert s["frames"] == NV and s["members"] == M and s["totals"] == (ref[0][3] + ref[1][3]).tolist()
    assert ens.result() == ue.decode(s["totals"], NV, M) and ens.result()["pixels"] == NV * H * W
    assert np.array_equal(ens.state_buffer[:NV].cpu().numpy().view(np.uint32), np.stack([r[0] for r in ref]))
    ens.reset()
    assert ens.state()["totals"] == [0] * ue.ROW and ens.state()["frames"] == 0


def test_pool_of_spoiled_members_is_nan_where_a_member_was_not_finite():
    shape, M = "ragged-64", 5
    H, W = _shape(shape)
    members, spots = _spoiled(shape, M)
    pooled, rows, ens, _ = _pool(members, H, W)
    for b in range(NV):
        ref = ue.frame(_frame_members(members, b))
        _check_pooled(pooled[b], rows[b], ref, f"spoiled frame {b}")
        assert int((ref[2] == 3).sum()) >= 17 and rows[b][ue.CHANGED + 15] >= 8 and rows[b][[ue.CHANGED + 3, ue.CHANGED + 7, ue.CHANGED + 11]].sum() >= 8
    assert ens.result()["not_finite"] == int(sum(np.isnan(pooled[b][0]).sum() for b in range(NV)))
    # what takes the classifier's logits counts them as it does today: not finite
    lg = ens.logits_buffer
    rule = dnn.DecisionRule(B, H, W, low=(0.3, 0.3), device=DEV)
    rule(lg, n_valid=NV)
    assert rule.counts()[:, 10].cpu().tolist() == [int(np.isnan(pooled[b][0]).sum()) for b in range(NV)]


def _edge_members():
    """Two members on 4 x 8, one case per pixel of row 0 (the rest generic): exact ties of S and classes with S_c == 0"""
    H, W = 4, 8
    rs = np.random.RandomState(5)
    q1 = [rs.randint(2000, 20000, size=(H, W)).astype(np.int64) for _ in range(2)]
    q2 = [rs.randint(2000, 20000, size=(H, W)).astype(np.int64) for _ in range(2)]
    for m in range(2):
        q1[m][0, 0], q2[m][0, 0] = 30000, 5536                                    # S_0 == S_1 > S_2 in every member
        q1[m][0, 2], q2[m][0, 2] = 27768, 27768                                   # S_1 == S_2 > S_0 in every member
    q1[0][0, 1], q2[0][0, 1], q1[1][0, 1], q2[1][0, 1] = 20000, 5536, 40000, 5536  # S_0 == S_1 through the sum: 40000 + 20000 twice
    q1[0][0, 3], q2[0][0, 3], q1[1][0, 3], q2[1][0, 3] = 5000, 40000, 5000, 20536  # S_0 == S_2 > S_1: 20536 + 40000 twice
    frames = [ud.clear_triples(q1[m], q2[m]) for m in range(2)]
    for f in frames:
        f[:, 0, 5] = (0.0, -40.0, -40.0)                                          # q = (65536, 0, 0): S_1 == S_2 == 0
        f[:, 0, 6] = (-40.0, -40.0, 0.0)
        assert up.distance_to_boundary(f).min() >= 0.25
    members = []
    for f in frames:
        logits = np.full((B, 3, H, W), np.nan, np.float32)
        logits[0], logits[1] = f, f[:, ::-1, ::-1]                                # the second frame: the same cases in other lanes
        members.append((logits, 0, False, None))
    return members, H, W


def test_ties_and_empty_classes_keep_the_integer_first_maximum():
    members, H, W = _edge_members()
    pooled, rows, ens, _ = _pool(members, H, W)
    for b in range(NV):
        ref = ue.frame(_frame_members(members, b))
        _check_pooled(pooled[b], rows[b], ref, f"edge frame {b}")
    S = ue.unpack(ens.state_buffer[0].cpu().numpy().view(np.uint32))[0]
    assert S[0, 0, 0] == S[1, 0, 0] > S[2, 0, 0] and S[0, 0, 1] == S[1, 0, 1] == 60000 and S[1, 0, 2] == S[2, 0, 2] > S[0, 0, 2]
    assert S[0, 0, 3] == S[2, 0, 3] > S[1, 0, 3] and S[:, 0, 5].tolist() == [2 * ONE, 0, 0] and S[:, 0, 6].tolist() == [0, 0, 2 * ONE]
    L0 = pooled[0]
    assert L0[:, 0, 0].view(np.uint32)[:2].tolist() == [0, 0] and L0[2, 0, 0] < 0 and L0[:, 0, 2].view(np.uint32)[1:].tolist() == [0, 0]
    assert L0[1, 0, 5] == L0[2, 0, 5] and abs(float(L0[1, 0, 5]) - np.log(1.0 / (2 * ONE))) <= 2.0 ** -20 and L0[0, 0, 5].view(np.uint32) == 0
    mask = dnn.predict_from_logits(ens.logits_buffer, n_valid=NV)[0].cpu().numpy()
    assert mask[0, 0, :4].tolist() == [0, 0, 1, 0] and mask[0, 0, 5:7].tolist() == [0, 2]          # dc_logits_predict: the first maximum
    assert np.array_equal(mask[0], ue.top_class(S, np.zeros((H, W), np.int64)))


def test_softmax_of_the_pooled_logits_is_the_share_of_the_sums():
    """(P2): | prob_q(L)_c - 65536 * max(S_c, 1) / sum_k max(S_k, 1) | <= 0.75, prob_q taken on the device (dc_prob_score's own chain).
    0.5 is the rounding to an integer.  0.25 is the budget for what stands between the exact share and the fp32 value that is rounded,
    which tests/test_ensemble_cpu.py evaluates in float64 to under 0.15 q-units: L_c = log(r_c), r_c = max(S_c, 1) / S_top, is rounded
    once to fp32 -- |L| <= log(2^32) < 23, so an absolute error of at most 2^-20 (half an ulp below 32) and a relative error of the
    exponential of the same size --, expf adds 2 ulp (2^-22 relative), the sum of three terms 2 roundings and the division and the
    multiplication by 65536 one each (2^-24 relative each): together below 1.6e-6 relative on a value of at most 65536, 0.11 q-units."""
    members, H, W = _edge_members()
    cases = [(members, H, W)] + [(_members(shape, M), *_shape(shape)) for shape, M in (("ragged-64", 5), ("one-10", 2))]
    worst = 0.0
    for mem, H, W in cases:
        pooled, _, ens, _ = _pool(mem, H, W)
        S = ue.unpack(ens.state_buffer[0].cpu().numpy().view(np.uint32))[0].reshape(3, -1)
        pick = np.unique(np.concatenate([np.arange(min(S.shape[1], 2000)), np.linspace(0, S.shape[1] - 1, 2000).astype(np.int64)]))
        q = _device_q(pooled[0].reshape(3, -1)[:, pick])
        err = np.abs(q - ue.shares(S[:, pick]))
        worst = max(worst, float(err.max()))
        assert (err <= 0.75).all(), (H, W, float(err.max()))
    print(f"(P2) largest | prob_q(L) - share | = {worst:.4f} q-units (allowed 0.75)")


def test_totals_do_not_depend_on_how_the_frames_are_cut_into_batches():
    shape, M = "ragged-64", 2
    H, W = _shape(shape)
    rs = np.random.RandomState(77)
    views = _views(W, M)
    frames = [[ud.smooth_logits(rs, H, W, blobs=8)[0] for _ in range(M)] for _ in range(3)]      # [frame][member]

    def batch(picked):
        out = []
        for m, (roll, flip, weighted) in enumerate(views):
            logits = np.full((B, 3, H, W), np.nan, np.float32)
            for slot, f in enumerate(picked):
                logits[slot] = frames[f][m]
            out.append((logits, roll, flip, _weights(W, roll, weighted)))
        return out

    _, rows3, whole, _ = _pool(batch([0, 1, 2]), H, W, n_valid=3)
    cut = dnn.ViewEnsemble(B, H, W, device=DEV)
    _, rows2, _, _ = _pool(batch([0, 1]), H, W, n_valid=2, ens=cut)
    _, rows1, _, _ = _pool(batch([2]), H, W, n_valid=1, ens=cut)
    assert np.array_equal(rows3, np.concatenate([rows2, rows1])) and whole.state() == cut.state() and cut.state()["frames"] == 3
    assert whole.state()["totals"] == rows3.sum(axis=0).tolist()


def test_view_ensemble_object_refusals():
    H, W = 4, 8
    ens = dnn.ViewEnsemble(B, H, W, device=DEV)
    lg = torch.zeros((B, 3, H, W), device=DEV)
    heavy = np.full(W, 40000, np.uint16)
    bad_calls = [lambda: ens.pool(), lambda: ens.add(lg[:2]), lambda: ens.add(lg.half()), lambda: ens.add(lg.cpu()), lambda: ens.add(lg, roll=W),
                 lambda: ens.add(lg, weights=np.zeros(W, np.uint16)), lambda: ens.add(lg, weights=np.ones(W + 1, np.uint16)),
                 lambda: ens.add(lg, weights=np.ones(W, np.int32)), lambda: ens.add(lg, n_valid=B + 1), lambda: ens.add(None)]
    with served("refused") as names:
        for k, bad in enumerate(bad_calls):
            with pytest.raises(L.DeepcamHipError):
                bad()
                pytest.fail(f"call {k} was accepted")
    assert names == [] and ens.members == 0
    ens.add(lg, weights=heavy, n_valid=NV)
    with pytest.raises(L.DeepcamHipError, match="sum to at most 65535"):
        ens.add(lg, weights=torch.from_numpy(heavy.view(np.int16).copy()).to(DEV), n_valid=NV)      # a device tensor is weighed like a host array
    with pytest.raises(L.DeepcamHipError, match="n_valid"):
        ens.add(lg, n_valid=NV + 1)
    ens.add(lg, weights=np.full(W, 25535, np.uint16), n_valid=NV)                                    # 40000 + 25535: the largest sum
    assert ens.members == 2 and tuple(ens.pool().shape) == (B, 3, H, W)
    S = ue.unpack(ens.state_buffer[0].cpu().numpy().view(np.uint32))[0]
    assert (S == 65535 * up.quantise(np.zeros((3, 1, 1), np.float32))).all() and S.max() == 65535 * 21845
    assert ens.begin().members == 0


# ------------------------------------------------------------------------------------------------------------------ 4. behind a network
def test_ensemble_of_views_behind_a_bf16_predictor():
    H, W = util_val.H, util_val.W
    net = dnn.DeepLabv3_plus(16, 3, os=16, _print=False, dtype=torch.bfloat16, seed=333)
    net.materialize(2, H, W)
    net.load_state_dict(util_val.perturbed_state())
    net.eval()
    g = torch.Generator().manual_seed(41)
    raw = (torch.rand(2, H, W, 16, generator=g) * torch.linspace(1, 300, 16) - 40.0).to(DEV)
    lo, hi = raw.amin(dim=(0, 1, 2)), raw.amax(dim=(0, 1, 2))
    shift, scale = lo.contiguous(), (1.0 / (hi - lo)).contiguous()
    views = [(0, False), (48, False), (17, True)]
    pr = dnn.Predictor(net, 2, H, W)
    try:
        pr.store_logits = True
        ens = dnn.ViewEnsemble(2, H, W, device=DEV)
        single = dnn.ViewEnsemble(2, H, W, device=DEV)
        xv = torch.empty((2, H, W, 16), dtype=torch.bfloat16, device=DEV)
        members = []
        for k, (roll, flip) in enumerate(views):
            dnn.view_input(raw, None, shift, scale, roll, flip, [3, 9] if flip else None, xv)
            pr(xv)
            wt = dnn.seam_weights(W, roll, 8)
            ens.add(pr.logits_buffer, roll, flip, wt)
            members.append((pr.logits.cpu().numpy(), roll, flip, wt))
            if k == 0:
                single.add(pr.logits_buffer)
                identity_mask = pr.mask_buffer.clone()
        pooled = ens.pool().cpu().numpy()
        words = ens.state_buffer.cpu().numpy().view(np.uint32)
        lone_mask = dnn.predict_from_logits(single.pool())[0]
        excluded = 0
        for b in range(2):
            mem = _frame_members(members, b)
            S, votes, bad, first = ue.unpack(words[b])
            rS, rvotes, rbad, rfirst = ue.accumulate(mem)
            assert np.array_equal(votes, rvotes) and not bad.any() and np.array_equal(first, rfirst)
            # a member whose p * 65536 stands within util_prob.EPS of a rounding boundary may round either way: one q-unit times its weight
            slack = np.zeros((H, W), np.int64)
            for logits, roll, flip, wt in mem:
                slack += ue.to_source(up.ambiguous(logits), roll, flip) * wt.astype(np.int64)[None, :]
            assert (np.abs(S - rS) <= slack[None]).all() and np.array_equal(S[:, slack == 0], rS[:, slack == 0])
            print(f"frame {b}: {int((slack > 0).sum())} pixels with an ambiguous member, {int((S != rS).any(axis=0).sum())} differ")
            # the single identity member: the pooled mask is the classifier's wherever its two largest q differ -- on the device, so
            # a pixel near a rounding boundary counts as tied when one q-unit either way would close the gap
            q = up.quantise(mem[0][0])
            top2 = np.sort(q, axis=0)
            gap = top2[2] - top2[1]
            tied = (gap == 0) | ((gap <= 2) & up.ambiguous(mem[0][0]))
            excluded += int(tied.sum())
            assert np.array_equal(lone_mask[b].cpu().numpy()[~tied], identity_mask[b].cpu().numpy()[~tied])
        assert excluded < 0.01 * 2 * H * W                                        # a condition on the captured logits, not a measurement
        assert np.isfinite(pooled).all() and ens.result()["members"] == 3
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the driver
def _h5_write(path, datasets):
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with h5.File(path, "w") as f:
        for name, array in datasets.items():
            if backend == "h5py":
                f.create_dataset(name, data=array)
            else:
                f.write(name, array)


def _h5_read(path, names):
    """name -> array, None where the file has no such dataset"""
    from mlperf_deepcam_amd import data as ddata
    backend, h5 = ddata._h5_backend()
    with (h5.File(path, "r") if backend == "h5py" else h5.File(path)) as f:
        return {n: ((f[n][...] if backend == "h5py" else f.read(n)) if n in f else None) for n in names}


def test_predict_cli_with_an_ensemble(tmp_path):
    from mlperf_deepcam_amd import predict
    H, W = util_val.H, util_val.W
    root = str(tmp_path / "files")
    os.makedirs(root)
    rs = np.random.RandomState(31)
    names = [f"data-2003-01-{d:02d}-00-1.h5" for d in (5, 6, 7, 8)]
    fields = [(rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32) for _ in names]
    truth = [rs.choice(np.asarray([0, 1, 2], np.int64), size=(H // 8, W // 8), p=[0.6, 0.2, 0.2]).repeat(8, 0).repeat(8, 1) for _ in names]
    for name, d, t in zip(names, fields, truth):
        _h5_write(os.path.join(root, name), {"climate/data": d, "climate/labels_0": t})
    stats = str(tmp_path / "stats.h5")
    lo = np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    hi = np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32)
    _h5_write(stats, {"climate/minval": lo, "climate/maxval": hi})
    ckpt = str(tmp_path / "model_step_7.cpt")
    torch.save({"step": 7, "epoch": 0, "model": util_val.perturbed_state()}, ckpt)
    base = ["--checkpoint", ckpt, "--data_dir", root, "--stats_file", stats, "--dtype", "bf16", "--height", str(H), "--width", str(W),
            "--max_inter_threads", "2", "--batch_size", "3", "--verify", "--prob_skill"]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    with served("predict without --ensemble_*") as launched:
        predict.main(predict.build_parser().parse_args([*base, "--output_dir", plain]))
    assert launched and not [n for n in launched if n.startswith("ensemble") or n == "view_normalize"]
    with served("predict --ensemble_rolls") as launched:                           # batches of three and one: a padded last batch
        predict.main(predict.build_parser().parse_args([*base, "--output_dir", out, "--ensemble_rolls", "48", "--ensemble_seam_margin", "8",
                                                        "--confidence"]))
    assert launched.count("view_normalize") == 2 and launched.count("ensemble_add_vec") == 4 and launched.count("ensemble_pool") == 2
    s_plain, s_out = (json.load(open(os.path.join(d, "summary.json"))) for d in (plain, out))
    assert "ensemble" not in s_plain
    e = s_out["ensemble"]
    assert e["members"] == 2 and e["views"] == [[0, False], [48, False]] and e["seam_margin"] == 8 and e["frames"] == 4 and e["pixels"] == 4 * H * W
    assert e["not_finite"] == 0 and s_out["prob_skill"]["pixels"] == s_plain["prob_skill"]["pixels"] and s_out["prob_skill"]["pixels"]["scored"] == 4 * H * W
    total = np.zeros(ue.ROW, np.int64)
    for name in names:
        g = _h5_read(os.path.join(out, name), ["prediction", "prediction_ensemble", "ensemble_rows", "confidence", "confidence_ensemble", "events"])
        p = _h5_read(os.path.join(plain, name), ["prediction", "prediction_ensemble", "ensemble_rows"])
        assert p["prediction_ensemble"] is None and p["ensemble_rows"] is None
        assert np.array_equal(g["prediction"], p["prediction"])                    # stays the identity view's mask
        pe, rows = g["prediction_ensemble"], g["ensemble_rows"]
        assert pe.dtype == np.uint8 and pe.shape == (H, W) and rows.dtype == np.int64 and rows.shape == (ue.ROW,)
        assert g["confidence_ensemble"].shape == (H, W) and g["confidence"].shape == (H, W)
        changed = rows[ue.CHANGED:].reshape(4, 4)
        assert changed.sum() == H * W and rows[:64].sum() == H * W
        assert changed.sum(axis=1)[:3].tolist() == np.bincount(g["prediction"].reshape(-1), minlength=3).tolist()      # member 0 IS `prediction`
        assert changed.sum(axis=0)[:3].tolist() == np.bincount(pe.reshape(-1), minlength=3).tolist()                   # ... and the pool is the new mask
        total += rows
    assert e["changed"] == total[ue.CHANGED:].reshape(4, 4).tolist() and e == dict(ue.decode(total, 4, 2), views=e["views"], seam_margin=8, negate=[])
    # mirrored twins with negated channels, without labels
    twins = str(tmp_path / "twins")
    args = predict.build_parser().parse_args([*base[:-2], "--output_dir", twins, "--ensemble_flip_lat", "--ensemble_negate", "4", "10"])
    with served("predict --ensemble_flip_lat") as launched:
        predict.main(args)
    assert launched.count("view_normalize") == 2 and launched.count("ensemble_pool") == 2
    e = json.load(open(os.path.join(twins, "summary.json")))["ensemble"]
    assert e["views"] == [[0, False], [0, True]] and e["negate"] == [4, 10] and e["members"] == 2 and e["frames"] == 4
