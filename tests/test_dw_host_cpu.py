"""The depthwise host code without a device: what the routing queries answer over a grid of shapes and options (tests/golden/dw_plan.json,
recorded from the commit before the host code was rewritten around one route), and what the forward / data-gradient entry points refuse,
with which return code and message.  Every call below is refused before anything is launched: the addresses are made up."""
import itertools
import json
import os
import re

import pytest

from mlperf_deepcam_amd import lib as L
import util_dw_host as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_plan.json")


def test_plan_table_matches_the_recorded_one():
    want = json.load(open(GOLDEN))
    got = U.plan_table(L.load())
    assert sorted(got) == sorted(want) and len(want) == len(U.OPTIONS)
    shapes = list(itertools.product(U.DTYPES, U.CHANNELS, U.STRIDE_DIL, U.EXTENTS))
    for opt in want:
        assert len(want[opt]) == len(shapes) == len(got[opt])
        diff = [(shape, g, w) for shape, g, w in zip(shapes, got[opt], want[opt]) if g != w]
        assert not diff, f"options (dw_tile, dw_pipe, dw_res_masked) = ({opt}): {len(diff)} rows differ, first (dtype, C, (stride, dil), (N, H, W)) = " \
                         f"{diff[0][0]}: {dict(zip(U.QUERIES + ('dc_dwconv_wgrad_workspace',), zip(diff[0][1], diff[0][2])))} (got, recorded)"


A = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced
HEAD = "dtype C stride dil N Hi Wi "
PARAMS = {
    "fwd": "x ldx w y ldy pscale pshift prelu stream",
    "fwd_fin": "x ldx w y ldy prelu count slab rows gamma beta running_mean running_var num_batches_tracked momentum eps scale shift "
               "save_mean save_invstd stream",
    "dgrad": "dy lddy w addend ldadd dx lddx stream",
    "dgrad_bnstats": "dy lddy w dx lddx ybn ldybn save_mean save_invstd mscale mshift relu slab stream",
    "dgrad_bnstats_wgrad": "dy lddy w dx lddx ybn ldybn save_mean save_invstd mscale mshift relu slab wslab stream",
    "dgrad_bnstats_wgrad_sum": "dy lddy w dx lddx ybn ldybn save_mean save_invstd mscale mshift relu slab wslab stream",
    "dgrad_bnstats_wgrad_add": "dy lddy w addend ldadd dx lddx ybn ldybn save_mean save_invstd mscale mshift relu slab wslab stream",
    "dgrad_wgrad": "dy lddy w addend ldadd dx lddx x ldx pscale pshift prelu wslab stream",
    "dgrad_wgrad_bnres": "dy lddy w addend ldadd dx lddx x ldx wslab ybn ldybn save_mean save_invstd relu slab stream",
    "dgrad_wgrad_bnres_sum": "dy lddy w addend ldadd dx lddx x ldx wslab ybn ldybn save_mean save_invstd relu slab stream",
}
# the call every case starts from (bf16, 128 channels, 16 x 16: served by every entry point, so each case has ONE thing wrong): the values below,
# 128 for every other ld*, A for every other pointer
FIXED = dict(dtype=L.DC_BF16, C=128, stride=1, dil=1, N=1, Hi=16, Wi=16, addend=None, ldadd=0, pscale=None, pshift=None, prelu=0, relu=1, count=100,
             rows=4, momentum=0.1, eps=1e-5, stream=None)
BIG = dict(N=2, Hi=32768, Wi=32768)          # 2^31 pixels

ALIGN = ": pointer not 16-byte aligned (ld=128, C=128, dtype=1)"
LD120 = ": pixel stride (ld) smaller than C or not vector aligned (ld=120, C=128, dtype=1)"
CH132 = ": channel count not a positive multiple of the 16-byte vector (ld=128, C=132, dtype=1)"
TILED = "dc_dwconv: tensor too large for the tiled path"
SUM_BNSTATS = "dc_dwconv_dgrad_bnstats_wgrad_sum: shape not served (dc_dwconv_dgrad_sum_row_ok), or the sum row is not double[2][C]"
RELU3 = "dc_dwconv_dgrad_wgrad_bnres: relu is 0, 1 (mask the sums) or 2 (mask the sums and the stored dx)"
RELU2 = "dc_dwconv_dgrad_wgrad_bnres: relu = 2 is switched off (option dw_res_masked)"

# entry point (after dc_dwconv_), case, what differs from the base call, options (dw_tile, dw_pipe, dw_res_masked) or None, return code, message
REFUSALS = [
    ("fwd", "null_w", dict(w=None), None, -2, "dc_dwconv_fwd: null weights"),
    ("fwd", "misaligned", dict(x=A + 2), None, -3, "dc_dwconv_fwd x" + ALIGN),
    ("fwd", "bad_ld", dict(ldy=120), None, -3, "dc_dwconv_fwd y" + LD120),
    ("fwd", "channels", dict(C=132), None, -3, "dc_dwconv_fwd x" + CH132),
    ("fwd", "null_out", dict(y=None), None, -3, "dc_dwconv_fwd y: null pointer (ld=128, C=128, dtype=1)"),
    ("fwd", "stride3", dict(stride=3), None, -2, "dc_dwconv: stride must be 1 or 2"),
    ("fwd", "dil0", dict(dil=0), None, -2, "dc_dwconv: bad shape"),
    ("fwd", "dtype", dict(dtype=7), None, -2, "dc_dwconv: bad dtype"),
    ("fwd", "big_s1", BIG, None, -2, TILED),
    ("fwd", "big_s2", dict(BIG, stride=2), None, -2, "dc_dwconv: tensor too large for the tiled stride-2 path"),
    ("fwd", "big_s1_window", BIG, (0, 1, 1), -2, "dc_dwconv: tensor too large for the stride-1 fast path"),
    ("fwd", "pscale_alone", dict(pscale=A), None, -2, "dc_dwconv_fwd: pscale and pshift go together"),
    ("fwd_fin", "null_w", dict(w=None), None, -2, "dc_dwconv_fwd_fin: null argument"),
    ("fwd_fin", "misaligned", dict(x=A + 2), None, -3, "dc_dwconv_fwd_fin x" + ALIGN),
    ("fwd_fin", "bad_ld", dict(ldy=120), None, -3, "dc_dwconv_fwd_fin y" + LD120),
    ("fwd_fin", "channels", dict(C=132), None, -3, "dc_dwconv_fwd_fin x" + CH132),
    ("fwd_fin", "dil3", dict(dil=3), None, -2, "dc_dwconv_fwd_fin: shape not served (dc_dwconv_fwd_fin_ok)"),
    ("fwd_fin", "stride2", dict(stride=2), None, -2, "dc_dwconv_fwd_fin: shape not served (dc_dwconv_fwd_fin_ok)"),
    ("fwd_fin", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_fwd_fin: shape not served (dc_dwconv_fwd_fin_ok)"),
    ("fwd_fin", "pipe_forward", dict(), (1, 2, 1), -2, "dc_dwconv_fwd_fin: shape not served (dc_dwconv_fwd_fin_ok)"),
    ("fwd_fin", "big", BIG, None, -2, TILED),
    ("fwd_fin", "count1", dict(count=1), None, -2, "Expected more than 1 value per channel when training"),
    ("fwd_fin", "count0", dict(count=0), None, -2, "Expected more than 1 value per channel when training"),
    ("fwd_fin", "slab_misaligned", dict(slab=A + 4), None, -2, "dc_dwconv_fwd_fin: the slab is read with 16-byte loads (16-byte aligned)"),
    ("fwd_fin", "rows0", dict(rows=0), None, -2, "dc_dwconv_fwd_fin: null argument"),
    ("fwd_fin", "null_gamma", dict(gamma=None), None, -2, "dc_dwconv_fwd_fin: null argument"),
    ("fwd_fin", "rows_many", dict(rows=100000), None, -2,
     "dc_dwconv_fwd_fin: a forward pass on the tiled kernel over a slab of at most dc_bn_bwd_apply_fin_max_rows() rows"),
    ("dgrad", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad: null weights"),
    ("dgrad", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad dy" + ALIGN),
    ("dgrad", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad dx" + LD120),
    ("dgrad", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad dy" + CH132),
    ("dgrad", "null_out", dict(dx=None), None, -3, "dc_dwconv_dgrad dx: null pointer (ld=128, C=128, dtype=1)"),
    ("dgrad", "stride3", dict(stride=3), None, -2, "dc_dwconv: stride must be 1 or 2"),
    ("dgrad", "dil0", dict(dil=0), None, -2, "dc_dwconv: bad shape"),
    ("dgrad", "dtype", dict(dtype=7), None, -2, "dc_dwconv: bad dtype"),
    ("dgrad", "big_s1", BIG, None, -2, TILED),
    ("dgrad", "big_s2", dict(BIG, stride=2), None, -2, "dc_dwconv: tensor too large for the tiled stride-2 path"),
    ("dgrad", "big_s1_window", BIG, (0, 1, 1), -2, "dc_dwconv: tensor too large for the stride-1 fast path"),
    ("dgrad", "addend_misaligned", dict(addend=A + 8, ldadd=128), None, -3, "dc_dwconv_dgrad addend" + ALIGN),
    ("dgrad", "addend_ld", dict(addend=A, ldadd=64), None, -3,
     "dc_dwconv_dgrad addend: pixel stride (ld) smaller than C or not vector aligned (ld=64, C=128, dtype=1)"),
    ("dgrad_bnstats", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_bnstats: null argument"),
    ("dgrad_bnstats", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_bnstats dy" + ALIGN),
    ("dgrad_bnstats", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_bnstats dx" + LD120),
    ("dgrad_bnstats", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_bnstats dy" + CH132),
    ("dgrad_bnstats", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_bnstats: shape not served by the tiled kernels"),
    ("dgrad_bnstats", "stride2dil2", dict(stride=2, dil=2), None, -2, "dc_dwconv_dgrad_bnstats: shape not served by the tiled kernels"),
    ("dgrad_bnstats", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_bnstats: shape not served by the tiled kernels"),
    ("dgrad_bnstats", "big", BIG, None, -2, TILED),
    ("dgrad_bnstats", "null_mean", dict(save_mean=None), None, -2, "dc_dwconv_dgrad_bnstats: null argument"),
    ("dgrad_bnstats", "null_mscale", dict(mscale=None), None, -2, "dc_dwconv_dgrad_bnstats: the ReLU mask needs the forward scale / shift vectors"),
    ("dgrad_bnstats", "ybn_misaligned", dict(ybn=A + 2), None, -3, "dc_dwconv_dgrad_bnstats y" + ALIGN),
    ("dgrad_bnstats_wgrad", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: null argument"),
    ("dgrad_bnstats_wgrad", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dy" + ALIGN),
    ("dgrad_bnstats_wgrad", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dx" + LD120),
    ("dgrad_bnstats_wgrad", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dy" + CH132),
    ("dgrad_bnstats_wgrad", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad", "big", BIG, None, -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad", "null_mscale", dict(mscale=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: null argument"),
    ("dgrad_bnstats_wgrad", "ybn_misaligned", dict(ybn=A + 2), None, -3, "dc_dwconv_dgrad_bnstats_wgrad y" + ALIGN),
    # the _sum twins name their base entry point, except in what only they check
    ("dgrad_bnstats_wgrad_sum", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: null argument"),
    ("dgrad_bnstats_wgrad_sum", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dy" + ALIGN),
    ("dgrad_bnstats_wgrad_sum", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dx" + LD120),
    ("dgrad_bnstats_wgrad_sum", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_bnstats_wgrad dy" + CH132),
    ("dgrad_bnstats_wgrad_sum", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad_sum", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad_sum", "big", BIG, None, -2, "dc_dwconv_dgrad_bnstats_wgrad: shape not served"),
    ("dgrad_bnstats_wgrad_sum", "sum_row_misaligned", dict(slab=A + 4), None, -2, SUM_BNSTATS),
    ("dgrad_bnstats_wgrad_sum", "sum_row_shape", dict(Hi=17), None, -2, SUM_BNSTATS),
    ("dgrad_bnstats_wgrad_sum", "sum_row_f32", dict(dtype=L.DC_F32), None, -2, SUM_BNSTATS),
    ("dgrad_bnstats_wgrad_sum", "sum_row_pipe_off", dict(), (1, 0, 1), -2, SUM_BNSTATS),
    ("dgrad_bnstats_wgrad_sum", "sum_row_s2", dict(stride=2), None, -2, SUM_BNSTATS),
    ("dgrad_bnstats_wgrad_sum", "null_mscale", dict(mscale=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad: null argument"),
    ("dgrad_bnstats_wgrad_add", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: null argument"),
    ("dgrad_bnstats_wgrad_add", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_bnstats_wgrad_add dy" + ALIGN),
    ("dgrad_bnstats_wgrad_add", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_bnstats_wgrad_add dx" + LD120),
    ("dgrad_bnstats_wgrad_add", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_bnstats_wgrad_add dy" + CH132),
    ("dgrad_bnstats_wgrad_add", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: shape not served"),
    ("dgrad_bnstats_wgrad_add", "stride2", dict(stride=2), None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: stride 1"),
    ("dgrad_bnstats_wgrad_add", "stride2dil2", dict(stride=2, dil=2), None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: stride 1"),
    ("dgrad_bnstats_wgrad_add", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_bnstats_wgrad_add: shape not served"),
    ("dgrad_bnstats_wgrad_add", "big", BIG, None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: shape not served"),
    ("dgrad_bnstats_wgrad_add", "addend_misaligned", dict(addend=A + 8, ldadd=128), None, -3, "dc_dwconv_dgrad_bnstats_wgrad_add addend" + ALIGN),
    ("dgrad_bnstats_wgrad_add", "null_mscale", dict(mscale=None), None, -2, "dc_dwconv_dgrad_bnstats_wgrad_add: null argument"),
    ("dgrad_bnstats_wgrad_add", "ybn_misaligned", dict(ybn=A + 2), None, -3, "dc_dwconv_dgrad_bnstats_wgrad_add y" + ALIGN),
    ("dgrad_wgrad", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_wgrad: bad argument"),
    ("dgrad_wgrad", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_wgrad dy" + ALIGN),
    ("dgrad_wgrad", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_wgrad dx" + LD120),
    ("dgrad_wgrad", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_wgrad dy" + CH132),
    ("dgrad_wgrad", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_wgrad: shape not served"),
    ("dgrad_wgrad", "stride2dil2", dict(stride=2, dil=2), None, -2, "dc_dwconv_dgrad_wgrad: shape not served"),
    ("dgrad_wgrad", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_wgrad: shape not served"),
    ("dgrad_wgrad", "big", BIG, None, -2, "dc_dwconv_dgrad_wgrad: shape not served"),
    ("dgrad_wgrad", "addend_misaligned", dict(addend=A + 8, ldadd=128), None, -3, "dc_dwconv_dgrad_wgrad addend" + ALIGN),
    ("dgrad_wgrad", "pscale_alone", dict(pscale=A), None, -2, "dc_dwconv_dgrad_wgrad: bad argument"),
    ("dgrad_wgrad", "null_wslab", dict(wslab=None), None, -2, "dc_dwconv_dgrad_wgrad: bad argument"),
    ("dgrad_wgrad", "x_misaligned", dict(x=A + 4), None, -3, "dc_dwconv_dgrad_wgrad x" + ALIGN),
    ("dgrad_wgrad_bnres", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_wgrad_bnres: null argument"),
    ("dgrad_wgrad_bnres", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_wgrad_bnres dy" + ALIGN),
    ("dgrad_wgrad_bnres", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_wgrad_bnres dx" + LD120),
    ("dgrad_wgrad_bnres", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_wgrad_bnres dy" + CH132),
    ("dgrad_wgrad_bnres", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "dil2", dict(dil=2), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "stride2", dict(stride=2), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "pipe_off", dict(), (1, 0, 1), -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "f32", dict(dtype=L.DC_F32), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "odd_extent", dict(Hi=17), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "big", BIG, None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres", "addend_misaligned", dict(addend=A + 8, ldadd=128), None, -3, "dc_dwconv_dgrad_wgrad_bnres addend" + ALIGN),
    ("dgrad_wgrad_bnres", "ybn_misaligned", dict(ybn=A + 2), None, -3, "dc_dwconv_dgrad_wgrad_bnres ybn" + ALIGN),
    ("dgrad_wgrad_bnres", "relu3", dict(relu=3), None, -2, RELU3),
    ("dgrad_wgrad_bnres", "relu2_off", dict(relu=2), (1, 1, 0), -2, RELU2),
    ("dgrad_wgrad_bnres", "null_slab", dict(slab=None), None, -2, "dc_dwconv_dgrad_wgrad_bnres: null argument"),
    ("dgrad_wgrad_bnres_sum", "null_w", dict(w=None), None, -2, "dc_dwconv_dgrad_wgrad_bnres: null argument"),
    ("dgrad_wgrad_bnres_sum", "misaligned", dict(dy=A + 2), None, -3, "dc_dwconv_dgrad_wgrad_bnres dy" + ALIGN),
    ("dgrad_wgrad_bnres_sum", "bad_ld", dict(lddx=120), None, -3, "dc_dwconv_dgrad_wgrad_bnres dx" + LD120),
    ("dgrad_wgrad_bnres_sum", "channels", dict(C=132), None, -3, "dc_dwconv_dgrad_wgrad_bnres dy" + CH132),
    ("dgrad_wgrad_bnres_sum", "dil3", dict(dil=3), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres_sum", "tile_off", dict(), (0, 1, 1), -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres_sum", "odd_extent", dict(Hi=17), None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres_sum", "big", BIG, None, -2, "dc_dwconv_dgrad_wgrad_bnres: shape not served"),
    ("dgrad_wgrad_bnres_sum", "relu3", dict(relu=3), None, -2, RELU3),
    ("dgrad_wgrad_bnres_sum", "relu2_off", dict(relu=2), (1, 1, 0), -2, RELU2),
    ("dgrad_wgrad_bnres_sum", "null_slab", dict(slab=None), None, -2, "dc_dwconv_dgrad_wgrad_bnres: null argument"),
    ("dgrad_wgrad_bnres_sum", "sum_row_misaligned", dict(slab=A + 4), None, -2, "dc_dwconv_dgrad_wgrad_bnres_sum: a sum row is double[2][C]"),
]


def test_every_entry_point_has_refusals():
    assert {r[0] for r in REFUSALS} == set(PARAMS) and len({r[:2] for r in REFUSALS}) == len(REFUSALS)
    for kind in ("null_w", "misaligned", "bad_ld", "channels"):
        assert {r[0] for r in REFUSALS if r[1] == kind} == set(PARAMS), kind


@pytest.mark.parametrize("row", REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in REFUSALS])
def test_refusal_keeps_its_code_and_message(row):
    entry, _, over, opt, rc, msg = row
    names = (HEAD + PARAMS[entry]).split()
    assert over != {} or opt is not None, "the base call would be served"
    assert set(over) <= set(names)
    args = [over[n] if n in over else FIXED[n] if n in FIXED else 128 if n.startswith("ld") else A for n in names]
    lib = L.load()
    U.set_options(lib, opt or U.OPTIONS[0])
    try:
        got = getattr(lib, "dc_dwconv_" + entry)(*args)
    finally:
        U.set_options(lib, U.OPTIONS[0])
    assert got != 0, "the call was not refused"
    assert (got, re.sub(r" \([^()]*:\d+\)$", "", L.last_error())) == (rc, msg)
