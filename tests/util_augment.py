"""Checker of the train-time augmentation (data.Augment, data.InputPipeline(augment=...), data.to_source; dc_augment_view_hwc): the draw
rule and a viewed batch restated in numpy, on util_ensemble's to_view / view_input, with no knowledge of workgroups or of the packed table.

The DRAW of a file in an epoch is a function of (seed, epoch, basename) alone:
    g = default_rng([seed, epoch, crc32(basename)]); r = g.integers(0, W); f = g.integers(0, 2)      -- both always drawn, in this order
    view = (r if roll else 0, f if flip_lat else 0)
A VIEW is util_ensemble's: view pixel (h, w) of sample n shows source pixel (H - 1 - h if flip_n else h, (w + roll_n) mod W).
A VIEWED BATCH is, per sample, util_ensemble.view_input with the sample's own view and the sign only where the sample is mirrored; its
labels are util_ensemble.to_view of the sample's label map."""
import os
import zlib

import numpy as np

import util_ensemble as ue


def draw(seed, epoch, name, W, roll=True, flip_lat=True):
    """(roll, flip) of one file"""
    g = np.random.default_rng([seed, epoch, zlib.crc32(os.path.basename(name).encode())])
    r = int(g.integers(0, W))
    f = int(g.integers(0, 2))
    return (r if roll else 0, f if flip_lat else 0)


def draws(seed, epoch, names, W, roll=True, flip_lat=True):
    """int32 [len(names), 2]"""
    return np.asarray([draw(seed, epoch, n, W, roll, flip_lat) for n in names], np.int32).reshape(len(names), 2)


def slot_views(seed, epoch, names, B, W, roll=True, flip_lat=True):
    """int32 [B, 2] of a batch whose valid samples are `names`: a padding slot repeats the last sample and takes its view"""
    return draws(seed, epoch, [names[min(j, len(names) - 1)] for j in range(B)], W, roll, flip_lat)


def viewed_labels(labels, views):
    """labels [B, H, W] in source coordinates -> view coordinates, sample n by views[n]"""
    labels = np.asarray(labels)
    return np.stack([ue.to_view(labels[n], int(r), bool(f)) for n, (r, f) in enumerate(np.asarray(views).tolist())])


def viewed_batch(x, channels, flip_sign, shift, scale, views):
    """float64 [B, H, W, C] of x float32 [B, H, W, Cfile]: sample n is util_ensemble.view_input of it alone with views[n], the sign
    flip_sign (per SELECTED channel, None: all +1) only where the sample is mirrored"""
    x = np.asarray(x)
    return np.concatenate([ue.view_input(x[n:n + 1], channels, flip_sign if f else None, shift, scale, int(r), bool(f))
                           for n, (r, f) in enumerate(np.asarray(views).tolist())])
