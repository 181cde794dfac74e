"""The depthwise host plan as a table: what the six routing queries and the weight-gradient workspace query answer over a grid of shapes
and option settings.  Shared by tests/test_dw_host_cpu.py and tests/golden/make_golden_dw_plan.py; pure host code, no device."""
import itertools

DTYPES = (0, 1)                                   # DC_F32, DC_BF16
CHANNELS = (20, 32, 64, 128, 728)
STRIDE_DIL = ((1, 1), (1, 2), (1, 3), (2, 1), (2, 2))
EXTENTS = ((1, 8, 8), (2, 16, 24), (1, 17, 37), (3, 264, 420), (8, 48, 72), (2, 384, 576))      # N, H, W
OPTIONS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0))                                # dw_tile, dw_pipe, dw_res_masked
OPTION_NAMES = (b"dw_tile", b"dw_pipe", b"dw_res_masked")
QUERIES = ("dc_dwconv_dgrad_bnstats_rows", "dc_dwconv_dgrad_wgrad_rows", "dc_dwconv_dgrad_sum_row_ok", "dc_dwconv_dgrad_wgrad_bnres_rows",
           "dc_dwconv_dgrad_wgrad_bnres_masked", "dc_dwconv_fwd_fin_ok")


def set_options(lib, values):
    for name, v in zip(OPTION_NAMES, values):
        assert lib.dc_set_option(name, v) == 0, lib.dc_last_error().decode()


def plan_table(lib):
    """{"d,t,r": [[the six queries..., workspace] for every (dtype, C, (stride, dil), (N, H, W)) in itertools.product order]}"""
    table = {}
    try:
        for opt in OPTIONS:
            set_options(lib, opt)
            rows = []
            for dt, c, (s, d), (n, h, w) in itertools.product(DTYPES, CHANNELS, STRIDE_DIL, EXTENTS):
                rows.append([getattr(lib, q)(dt, c, s, d, n, h, w) for q in QUERIES] + [lib.dc_dwconv_wgrad_workspace(c, n, h, w, s)])
            table[",".join(map(str, opt))] = rows
    finally:
        set_options(lib, OPTIONS[0])
    return table
