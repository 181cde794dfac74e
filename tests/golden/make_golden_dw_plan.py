#!/usr/bin/env python3
"""Generate tests/golden/dw_plan.json: the depthwise routing queries over the grid of tests/util_dw_host.py, recorded from a build of the
commit BEFORE a change to the depthwise host code (never from the change itself: the file is what the change must reproduce):

    DEEPCAM_HIP_LIB=<that build's libdeepcam_hip.so> python tests/golden/make_golden_dw_plan.py

Host code only: no device is touched."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mlperf_deepcam_amd import lib as L      # noqa: E402
import util_dw_host                          # noqa: E402


def main():
    table = util_dw_host.plan_table(L.load())
    with open(os.path.join(HERE, "dw_plan.json"), "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table.items()) + "\n}\n")
    print(f"dw_plan.json: {len(table)} option sets x {len(next(iter(table.values())))} shapes, from {L.LIB_PATH}")


if __name__ == "__main__":
    main()
