"""CPU side of the input-gradient and frozen-BatchNorm entry points: declared in the header, exported by the library, bound in the ctypes
table with the header's arity, reachable from a recorded launch list, and refusing bad arguments on the host before anything is launched."""
import ctypes as C
import os
import re

from mlperf_deepcam_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dc_stem_dgrad": 10, "dc_bn_bwd_frozen": 22}


def _declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepcam_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/deepcam_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_declared_exported_and_bound():
    lib = L.load()
    for name, nargs in NEW.items():
        assert len(_declaration(name)) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = L._SIGS[name]
        assert res is C.c_int and len(args) == nargs, name
    # the eps of dc_bn_bwd_frozen travels as a float
    assert L._SIGS["dc_bn_bwd_frozen"][1][13] is C.c_float


def test_recorded_launch_lists_reach_them():
    inc = open(os.path.join(ROOT, "mlperf-deepcam_amd", "csrc", "program_thunks.inc")).read()
    for name in NEW:
        assert f'{{"{name}", &t_{name}, {NEW[name]},' in inc, name


def test_bad_arguments_are_refused_on_the_host():
    lib = L.load()
    # Cin above the 16 the stem serves
    assert lib.dc_stem_dgrad(L.DC_BF16, 1, 17, 32, 48, None, 32, None, None, None) != 0
    assert "dc_stem_dgrad" in L.last_error()
    # a dy view whose pixel stride is not a whole number of 16-byte vectors (checked before any launch)
    buf = (C.c_float * 64)()
    assert lib.dc_stem_dgrad(L.DC_BF16, 1, 16, 32, 48, C.cast(buf, C.c_void_p), 36, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), None) != 0
    assert "dc_stem_dgrad dy" in L.last_error()
    # missing tensors
    assert lib.dc_bn_bwd_frozen(L.DC_F32, 64, 32, None, 32, None, 32, None, 0, 0, None, None, None, 1e-5, None, 32, None, 0, None, None, None,
                                None) != 0
    assert "dc_bn_bwd_frozen" in L.last_error()
