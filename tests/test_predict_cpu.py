"""Inference on unlabelled data, the host side: the three C-ABI entry points are declared, exported and bound, the launch-list thunks are
current, the driver's flags parse, and data.CamDataset(labels=False) reads files that have no climate/labels_0.  (InputPipeline needs a
device: its unlabelled / ragged-batch behaviour is in tests/test_predict_gpu.py.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"dc_head_fwd_predict": 15, "dc_head_fwd_predict_bnin": 18, "dc_logits_predict": 9}


def test_predict_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "deepcam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in deepcam_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == nargs, f"{name}: binding table"
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_predict_thunks_are_current():
    inc = open(os.path.join(ROOT, "mlperf-deepcam_amd", "csrc", "program_thunks.inc")).read()
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "mlperf-deepcam_amd", "csrc", "gen_thunks.py")], capture_output=True, text=True,
                         timeout=60)
    assert gen.returncode == 0, gen.stderr[-2000:]
    assert gen.stdout == inc, "program_thunks.inc is stale: python mlperf-deepcam_amd/csrc/gen_thunks.py > program_thunks.inc"
    for name in SYMBOLS:
        assert f'{{"{name}", &t_{name}, {SYMBOLS[name]},' in inc


def test_predict_parser_accepts_the_documented_flags():
    from mlperf_deepcam_amd import predict
    a = predict.build_parser().parse_args(
        ["--checkpoint", "m.cpt", "--data_dir", "d", "--stats_file", "s.h5", "--output_dir", "o", "--batch_size", "4", "--channels", "0", "1", "2",
         "10", "--dtype", "fp32", "--amp_opt_level", "O0", "--confidence", "--height", "64", "--width", "96", "--max_inter_threads", "2"])
    assert (a.checkpoint, a.data_dir, a.stats_file, a.output_dir) == ("m.cpt", "d", "s.h5", "o")
    assert a.batch_size == 4 and a.channels == [0, 1, 2, 10] and a.dtype == "fp32" and a.amp_opt_level == "O0" and a.confidence is True
    assert (a.height, a.width, a.max_inter_threads) == (64, 96, 2)
    d = predict.build_parser().parse_args(["--checkpoint", "m", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"])
    assert d.confidence is False and d.channels == list(range(16)) and (d.height, d.width) == (768, 1152) and d.dtype is None
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(["--data_dir", "d"])                  # no checkpoint, no output directory


# flag -> the attributes it sets to True, and whether the flag leaves no attribute behind unless given (argparse.SUPPRESS)
IMPLYING_FLAGS = {
    "verify": (("verify", "events"), False),
    "event_fields": (("event_fields", "events"), False),
    "tracks": (("tracks", "events"), False),
    "track_fields": (("track_fields", "tracks", "event_fields", "events"), False),
    "event_shape": (("event_shape", "events"), False),
    "composites": (("composites", "event_fields", "events"), True),
    "fss": (("fss", "verify", "events"), True),
    "distance_skill": (("distance_skill", "verify", "events"), True),
    "displacement": (("displacement", "verify", "events"), True),
    "scale_skill": (("scale_skill", "verify", "events"), True),
    "prob_skill": (("prob_skill", "verify", "events"), True),
}


@pytest.mark.parametrize("flag", sorted(IMPLYING_FLAGS))
def test_a_flag_that_implies_others_sets_exactly_those(flag):
    from mlperf_deepcam_amd import predict
    required = ["--checkpoint", "m", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    plain = vars(predict.build_parser().parse_args(required))
    given = vars(predict.build_parser().parse_args([*required, "--" + flag]))
    sets, suppressed = IMPLYING_FLAGS[flag]
    assert (flag not in plain) if suppressed else (plain[flag] is False)
    for other, (_, other_suppressed) in IMPLYING_FLAGS.items():                  # the flag brings in no other flag's attribute
        assert (other in given) == (other in sets or not other_suppressed), other
    changed = {k for k in given if k not in plain or given[k] != plain[k]}
    assert changed == set(sets) and all(given[k] is True for k in sets)
    assert set(plain) - set(given) == set()


def _unlabelled_files(tmp_path, n=3, H=16, W=24):
    from mlperf_deepcam_amd import h5lite
    root = str(tmp_path / "unlabelled")
    os.makedirs(root)
    rs = np.random.RandomState(7)
    fields = []
    for i in range(n):
        d = (rs.rand(H, W, 16) * np.linspace(1, 300, 16) - 40.0).astype(np.float32)
        fields.append(d)
        with h5lite.File(os.path.join(root, f"data-{i:02d}.h5"), "w") as f:
            f.write("climate/data", d)
    stats = str(tmp_path / "stats.h5")
    with h5lite.File(stats, "w") as f:
        f.write("climate/minval", np.min([d.min(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
        f.write("climate/maxval", np.max([d.max(axis=(0, 1)) for d in fields], axis=0).astype(np.float32))
    return root, stats, fields


def test_camdataset_without_labels(tmp_path):
    from mlperf_deepcam_amd import data as ddata
    from mlperf_deepcam_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 C library in this image")
    root, stats, fields = _unlabelled_files(tmp_path)
    ds = ddata.CamDataset(root, stats, list(range(16)), allow_uneven_distribution=True, labels=False)
    assert len(ds) == 3 and ds.labels is False and tuple(ds.data_shape) == (16, 24, 16) and tuple(ds.label_shape) == (16, 24)
    out = np.empty((16, 24, 16), np.float32)
    for i in range(3):
        name = ds.read_into(i, out, None)
        assert os.path.basename(name) == f"data-{i:02d}.h5"
        np.testing.assert_array_equal(out, fields[i])
    with pytest.raises(ValueError):
        ds.read_into(0, out, np.empty((16, 24), np.int64))        # an unlabelled dataset has nothing to put there
    # the default still insists on the labels
    with pytest.raises(Exception):
        ddata.CamDataset(root, stats, list(range(16)), allow_uneven_distribution=True)
