"""Shared by the kernel tests: which kernel family served a library call (the launch record of include/deepcam_hip.h, dc_launch_log_*).

    with served() as names:
        L.call("dc_conv_fwd", ...)
    assert_served(names, ["pw384_256_k64"])

`names` is filled when the block ends: the vocabulary is the header's, one name per launch in launch order.  The record is host state of the
calling thread; nothing is synchronised and nothing changes on the device, so wrapping a call does not change what it computes.

DEEPCAM_LAUNCH_TRACE=<file>: every record is also appended to that file, one line "<pytest test id> | <what> | <names>" (how the per-case
tables of who serves what are made)."""
import contextlib
import ctypes as C
import os

from mlperf_deepcam_amd import lib as L

GENERIC = "aux"        # launch sites no option or planner chooses between (packing, gathers, finalizes, ...)
_CAP = 1 << 16


def end_record():
    """dc_launch_log_end as a list of names; raises DeepcamHipError with the library's message on failure."""
    buf = C.create_string_buffer(_CAP)
    if L.load().dc_launch_log_end(buf, _CAP) != 0:
        raise L.DeepcamHipError(f"dc_launch_log_end: {L.last_error()}")
    text = buf.value.decode()
    return text.split("\n") if text else []


@contextlib.contextmanager
def served(what=""):
    """Records the launches of the block; yields the list that holds their names afterwards (also when the block raises)."""
    names = []
    if L.load().dc_launch_log_begin() != 0:
        raise L.DeepcamHipError(f"dc_launch_log_begin: {L.last_error()}")
    try:
        yield names
    finally:
        names.extend(end_record())
        trace = os.environ.get("DEEPCAM_LAUNCH_TRACE")
        if trace:
            with open(trace, "a") as f:
                f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]} | {what} | {' '.join(names)}\n")


def assert_served(names, expected, what="", ignore=()):
    """The recorded names are exactly `expected` (a name or a list of names, in launch order), not counting the names in `ignore`."""
    if isinstance(expected, str):
        expected = [expected]
    got = [n for n in names if n not in ignore]
    assert got == list(expected), f"{what + ': ' if what else ''}served by {got}, expected {list(expected)}" + \
        (f" (recorded {list(names)}, ignoring {list(ignore)})" if ignore else "")
