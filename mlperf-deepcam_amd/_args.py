"""What the analysis modules (events, render, climate, skills, decide) share: the default device, the number of valid samples, the
frame-group table, the check of a device tensor argument, and a few conversions."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import lib as L

_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}    # the element sizes of a class mask
MASK_KIND = "uint8, int32 or int64"                          # how the messages name _BYTES' dtypes


def _c_int(v: int) -> int:
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _float(v):
    return None if v is None else float(v)


def _ratio(a, b):
    """a / b as a Python float, None where b == 0"""
    return None if b == 0 else a / b


def _two_words(words):
    """Python ints, nested as the leading axes, from int64 words [..., 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned"""
    words = np.asarray(words, np.int64)
    out = np.empty(words.size // 2, dtype=object)
    out[:] = [(int(hi) << 64) | (int(lo) & 0xFFFFFFFFFFFFFFFF) for lo, hi in words.reshape(-1, 2).tolist()]
    return out.reshape(words.shape[:-1]).tolist()


def device_of(device):
    """the current device where none is given, else the argument as it came"""
    return torch.device("cuda", torch.cuda.current_device()) if device is None else device


def _n_valid(who: str, n_valid: Optional[int], batch: int) -> int:
    nv = batch if n_valid is None else int(n_valid)
    if not 0 <= nv <= batch:
        raise L.DeepcamHipError(f"{who}: n_valid must lie in [0, {batch}], got {n_valid}")
    return nv


def group_table(who: str, groups, batch: int, nv: int, n_groups: int) -> tuple:
    """The group of every frame of a batch as a tuple of `batch` ints, from None (every frame to group 0), an int, or `batch` ints; -1 for
    a frame that is skipped: one from nv on, or one given a negative group."""
    if groups is None or isinstance(groups, (int, np.integer)):
        table = [0 if groups is None else int(groups)] * batch
    else:
        table = [int(g) for g in groups]
        if len(table) != batch:
            raise L.DeepcamHipError(f"{who}: {len(table)} groups for a batch of {batch}")
    table = tuple(g if j < nv and g >= 0 else -1 for j, g in enumerate(table))
    if any(g >= n_groups for g in table):
        raise L.DeepcamHipError(f"{who}: group indices must be below {n_groups}, got {list(table)}")
    return table


def check_tensor(who: str, name: str, t, dtypes, shape, device, kind: Optional[str] = None) -> None:
    """Raises unless t is a contiguous tensor of one of `dtypes` and of `shape` on the CUDA device `device`.  kind: how the message names
    the dtypes ("fp32", MASK_KIND); by default their own names."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_cuda or t.device != device \
            or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise L.DeepcamHipError(f"{who}: {name} must be a contiguous {kind or ' / '.join(str(d) for d in dtypes)} tensor "
                                f"{list(shape)} on {device}, got {got}")


def check_range(who: str, name: str, v: int, lo: int, hi: int) -> None:
    """Raises unless the integer v lies in [lo, hi]."""
    if not lo <= v <= hi:
        raise L.DeepcamHipError(f"{who}: {name} must lie in [{lo}, {hi}], got {v}")
