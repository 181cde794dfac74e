"""Verification skills: neighbourhood (FractionsSkill), distance-map (DistanceSkill), displacement (DisplacementSkill), scale-separation
(ScaleSkill) and probabilistic (ProbabilitySkill) verification of predictions against labels, on the device."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from ._args import _BYTES, MASK_KIND, _float, _n_valid, _ratio, _two_words, check_tensor, device_of


# ---------------------------------------------------------------------------------------------- verification skills: what they share
class _MaskSkill:
    """What the skills that score a predicted class mask against a labelled one share (FractionsSkill, DistanceSkill, DisplacementSkill,
    ScaleSkill): a batch of [B, H, W] frames with fewer than 2^31 pixels each, a band of rows row_range = (row0, row1), the check of
    the two masks (contiguous device uint8, int32 or int64, each side with its own element size), per-frame buffers of the last call
    and running totals since reset().  A subclass names the attributes of its per-frame buffers in `_frame` (the order of FRAME_KEYS, the
    datasets they are stored under) and of its totals in `_totals`, and makes the call in _score()."""

    FRAME_KEYS: tuple = ()
    _frame: tuple = ()
    _totals: tuple = ()

    def _geometry(self, batch: int, height: int, width: int, max_batch: int) -> None:
        if batch < 1 or batch > max_batch or height < 1 or width < 1 or height * width >= 1 << 31:
            raise L.DeepcamHipError(f"{type(self).__name__}: batch must lie in [1, {max_batch}], height and width be positive and "
                                    "height * width below 2^31")
        self.B, self.H, self.W, self._nv = batch, height, width, 0

    def _band(self, row_range) -> tuple:
        row0, row1 = (0, self.H) if row_range is None else (int(row_range[0]), int(row_range[1]))
        if not 0 <= row0 < row1 <= self.H:
            raise L.DeepcamHipError(f"{type(self).__name__}: row_range must satisfy 0 <= row0 < row1 <= {self.H}, got {row_range}")
        self.row_range = (row0, row1)
        return row0, row1

    def __call__(self, pred: torch.Tensor, truth: torch.Tensor, n_valid: Optional[int] = None):
        """pred, truth: contiguous device uint8, int32 or int64 [B, H, W], each side with its own element size; the frames from n_valid on
        are neither read nor written (FractionsSkill: not read, and their rows are zero).  Returns the object."""
        for t, name in ((pred, "pred"), (truth, "truth")):
            check_tensor(type(self).__name__, name, t, _BYTES, (self.B, self.H, self.W), self.device, MASK_KIND)
        nv = _n_valid(type(self).__name__, n_valid, self.B)
        self._score(nv, L.dptr(pred), _BYTES[pred.dtype], L.dptr(truth), _BYTES[truth.dtype])
        self._nv = nv
        return self

    def frame_rows(self) -> tuple:
        """the per-frame buffers of the last call, in the order of FRAME_KEYS, each cut to [n_valid, ...]: views of the object's device
        buffers, not synchronised"""
        return tuple(getattr(self, name)[:self._nv] for name in self._frame)

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        for name in self._totals:
            getattr(self, name).zero_()


# ---------------------------------------------------------------------------------------------- neighbourhood verification
FSS_WINDOWS = (1, 3, 9, 17, 33, 65, 129)
FSS_MAX_WINDOW = 255
FSS_MAX_WINDOWS = 16
FSS_MAX_BATCH = 4095


def _fss(a: int, b: int, c: int):
    """1 - A / (B + C) from Python ints by true division (correctly rounded), None where B + C == 0"""
    return None if b + c == 0 else 1.0 - a / (b + c)


def fss_from_rows(rows):
    """The scores of integer rows [..., 3] = (A, B, C) as nested lists of the leading shape: 1 - A / (B + C) as a Python float from the
    exact integers, None where B + C == 0 (the class is absent from both masks)."""
    rows = np.asarray(rows)
    if rows.shape[-1:] != (3,):
        raise L.DeepcamHipError(f"fss_from_rows: the last axis must hold (A, B, C), got shape {rows.shape}")
    flat = rows.reshape(-1, 3).tolist()
    out = np.empty(len(flat), dtype=object)
    out[:] = [_fss(int(a), int(b), int(c)) for a, b, c in flat]
    return out.reshape(rows.shape[:-1]).tolist()


class FractionsSkill(_MaskSkill):
    """Neighbourhood verification on the device (dc_fss_score, csrc/fss.hip): per frame, class (1, 2) and window of n x n GRID PIXELS the
    integers (A, B, C) = (sum (F - O)^2, sum F^2, sum O^2), F and O the predicted and labelled pixel counts of the class inside the window
    around every pixel of the rows row_range = (row0, row1) -- columns periodic with wrap, rows beyond the poles empty -- and their running
    totals over all frames since reset() as two-word integers.  FSS = 1 - A / (B + C) (Roberts & Lean 2008) is decoded on the host from
    the exact integers; the pooled score of a run is 1 - sum A / (sum B + sum C).  windows: distinct odd sides in [1, 255], at most 16,
    with wrap also <= width.  No latitude weighting and no kilometres: row_range is the tool for a tropics-only score.
    Memory: a workspace of batch * S * height * width * 4 bytes, one packed word per pixel and window (dc_fss_workspace) -- 8 x 768 x 1152
    at the 7 default windows: 198.2 MB --, beside batch * (2 * S * 3 + 4) * 8 bytes of rows and a few hundred bytes of totals.
    A call launches on the current stream and does not synchronise; state() and result() read back."""

    FRAME_KEYS = ("fss", "fss_pixels")                # frame_rows(): int64 [n_valid, 2, S, 3], int64 [n_valid, 2, 2]
    _frame, _totals = ("_rows", "_pixels"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, windows: Sequence[int] = FSS_WINDOWS, wrap: bool = True, row_range=None,
                 device=None):
        self._geometry(batch, height, width, FSS_MAX_BATCH)
        windows = [int(n) for n in windows]
        if not 1 <= len(windows) <= FSS_MAX_WINDOWS:
            raise L.DeepcamHipError(f"FractionsSkill: between 1 and {FSS_MAX_WINDOWS} windows, got {len(windows)}")
        for n in windows:
            if n % 2 == 0 or not 1 <= n <= FSS_MAX_WINDOW:
                raise L.DeepcamHipError(f"FractionsSkill: a window is an odd number of pixels in [1, {FSS_MAX_WINDOW}], got {n}")
            if wrap and n > width:
                raise L.DeepcamHipError(f"FractionsSkill: a periodic window must not be wider than the frame ({width}), got {n}")
        if len(set(windows)) != len(windows):
            raise L.DeepcamHipError(f"FractionsSkill: the windows must be distinct, got {windows}")
        self._band(row_range)
        self.S, self.windows, self.wrap = len(windows), windows, bool(wrap)
        dev = torch.device(device_of(device))
        self._radius = torch.tensor([(n - 1) // 2 for n in windows], dtype=torch.int32, device=dev)
        dev = self.device = self._radius.device
        self._rows = torch.zeros((batch, 2, self.S, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, self.S, 3, 2), dtype=torch.int64, device=dev)          # (lo, hi)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_fss_workspace(batch, height, width, self.S)
        if size == 0:
            raise L.DeepcamHipError("FractionsSkill: dc_fss_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_fss_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.S, L.dptr(self._radius),
               int(self.wrap), self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    @staticmethod
    def combine(total_words) -> list:
        """[2][S][3] Python ints from the int64 words [2, S, 3, 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned"""
        words = np.asarray(total_words, np.int64)
        if words.ndim != 4 or words.shape[0] != 2 or words.shape[2:] != (3, 2):
            raise L.DeepcamHipError(f"FractionsSkill: the totals are int64 [2, S, 3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: total [2][S][3] as Python ints, pixels [2][2] ((pred, truth) per class) and frames as ints"""
        return {"total": self.combine(self._total.cpu().numpy()), "pixels": [[int(v) for v in row] for row in self._total_pixels.cpu().tolist()],
                "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.windows, self.row_range[1] - self.row_range[0], self.W)

    @staticmethod
    def decode(total, pixels, frames, windows, rows: int, width: int) -> dict:
        """Per class ("class_1", "class_2"), from the exact integers: fss, a list over the windows of the pooled 1 - sum A / (sum B + sum
        C), None where sum B + sum C == 0; base_rate = labelled pixels / (frames * rows * width), the share of the scored band the class
        covers; useful = 0.5 + base_rate / 2, the score above which a forecast is taken as skilful at that scale; skilful_window, the
        smallest window whose fss >= useful, else None.  Without a frame base_rate, useful and skilful_window are None."""
        windows = [int(n) for n in windows]
        cells = int(frames) * int(rows) * int(width)
        out = {}
        for k in range(2):
            scores = [_fss(*(int(v) for v in total[k][s])) for s in range(len(windows))]
            base = int(pixels[k][1]) / cells if cells > 0 else None
            useful = None if base is None else 0.5 + base / 2
            good = [n for n, f in zip(windows, scores) if useful is not None and f is not None and f >= useful]
            out[f"class_{k + 1}"] = {"fss": scores, "base_rate": base, "useful": useful, "skilful_window": min(good) if good else None}
        return out


# ---------------------------------------------------------------------------------------------- distance-map verification
DISTANCE_RADIUS = 64
DISTANCE_MAX_RADIUS = 127
DISTANCE_MAX_BATCH = 4095
DISTANCE_Q = 256                                  # dq = rint(sqrt(d^2) * DISTANCE_Q)


def distance_table(radius: int) -> np.ndarray:
    """int32 [R^2 + 2], the table dc_distance_score reads: entry v = ring(v) | dq(v) << 8 with ring(v) the smallest integer j with j^2 >= v
    (math.isqrt) and dq(v) = int(rint(sqrt(float64(v)) * 256)); the last entry (v = R^2 + 1, beyond the cap) has ring R + 1 and dq 0."""
    R = int(radius)
    if not 1 <= R <= DISTANCE_MAX_RADIUS:
        raise L.DeepcamHipError(f"distance_table: the radius must lie in [1, {DISTANCE_MAX_RADIUS}], got {radius}")
    table = np.zeros(R * R + 2, np.int32)
    for v in range(R * R + 1):
        ring = math.isqrt(v)
        ring += ring * ring < v
        table[v] = ring | int(np.rint(np.sqrt(np.float64(v)) * DISTANCE_Q)) << 8
    table[R * R + 1] = R + 1
    return table


class DistanceSkill(_MaskSkill):
    """Distance-map verification on the device (dc_distance_score, csrc/distance.hip): per frame, side (prediction, labels) and class (1, 2)
    the map of the squared Euclidean distance, in GRID PIXELS, to the nearest pixel of that side and class -- columns periodic with wrap,
    rows never --, capped: R^2 + 1 ("beyond") where nothing lies within `radius` = R.  From the maps, per class and direction (0 "miss": from
    every labelled pixel to the nearest predicted one; 1 "false alarm": the reverse) the sources per ring of distance, the sums of the
    distance (in 1/256 pixel) and of its square, and Baddeley's sum of squared map differences, as integers and as running totals over all
    frames since reset(); decode() turns them into the mean error distances, the (partial) Hausdorff distance, Baddeley's Delta and the hit
    rate and success ratio with a displacement of up to r pixels forgiven.  1 <= radius <= 127, with wrap also 2 radius + 1 <= width.
    No latitude weighting and no kilometres: row_range is the tool for a tropics-only score; it selects the sources and the Baddeley
    pixels, targets anywhere in the frame still count.  The single-word totals last 2^26 frames of 768 x 1152.
    Memory: a workspace of batch * height * width * 4 bytes (dc_distance_workspace; 28.3 MB at 8 x 768 x 1152), with keep_maps another
    batch * 4 * height * width * 2 bytes of uint16 maps (56.6 MB), beside batch * (4 * (R + 4) + 2) * 8 bytes of rows and the totals.
    A call launches on the current stream and does not synchronise; state() and result() read back."""

    FRAME_KEYS = ("distance", "distance_baddeley")    # frame_rows(): int64 [n_valid, 2, 2, R + 4], int64 [n_valid, 2]
    _frame, _totals = ("_rows", "_baddeley"), ("_total", "_total_baddeley", "_frames")

    def __init__(self, batch: int, height: int, width: int, radius: int = DISTANCE_RADIUS, wrap: bool = True, row_range=None,
                 keep_maps: bool = False, device=None):
        self._geometry(batch, height, width, DISTANCE_MAX_BATCH)
        R = int(radius)
        if not 1 <= R <= DISTANCE_MAX_RADIUS:
            raise L.DeepcamHipError(f"DistanceSkill: the radius must lie in [1, {DISTANCE_MAX_RADIUS}], got {radius}")
        if wrap and 2 * R + 1 > width:
            raise L.DeepcamHipError(f"DistanceSkill: a periodic window of 2 * {R} + 1 columns must not be wider than the frame ({width})")
        self._band(row_range)
        self.R, self.wrap, self.keep_maps = R, bool(wrap), bool(keep_maps)
        dev = torch.device(device_of(device))
        self._table = torch.from_numpy(distance_table(R)).to(dev)
        dev = self.device = self._table.device
        self._rows = torch.zeros((batch, 2, 2, R + 4), dtype=torch.int64, device=dev)
        self._baddeley = torch.zeros((batch, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, 2, R + 4), dtype=torch.int64, device=dev)
        self._total_baddeley = torch.zeros((2, 2), dtype=torch.int64, device=dev)            # (lo, hi)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._maps = torch.zeros((batch, 2, 2, height, width), dtype=torch.uint16, device=dev) if keep_maps else None
        size = L.load().dc_distance_workspace(batch, height, width, R)
        if size == 0:
            raise L.DeepcamHipError("DistanceSkill: dc_distance_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_distance_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.R, L.dptr(self._table),
               int(self.wrap), self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._baddeley), L.dptr(self._total),
               L.dptr(self._total_baddeley), L.dptr(self._frames), L.dptr(self._maps) if self._maps is not None else None,
               L.dptr(self._ws), L.stream_ptr())

    def maps(self) -> torch.Tensor:
        """uint16 [n_valid, 2 sides, 2 classes, H, W] of the last call (keep_maps): a view of the object's device buffer, not synchronised"""
        if self._maps is None:
            raise L.DeepcamHipError("DistanceSkill: maps() needs keep_maps=True")
        return self._maps[:self._nv]

    def state(self) -> dict:
        """on the host, as Python ints: total [2][2][R + 4], baddeley [2] (the two words combined) and frames"""
        return {"total": [[[int(v) for v in d] for d in cls] for cls in self._total.cpu().tolist()],
                "baddeley": _two_words(self._total_baddeley.cpu().numpy()), "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["baddeley"], s["frames"], self.R, self.H, self.W, self.row_range)

    @staticmethod
    def decode(total, total_baddeley, frames, radius: int, height: int, width: int, row_range=None) -> dict:
        """Per class ("class_1", "class_2"), in float64 from the exact integers; distances in grid pixels; None wherever a denominator is 0:
        pixels {"labelled", "predicted"}; pod_within[r] and success_within[r] for r = 0 .. R, the share of labelled (predicted) pixels with a
        predicted (labelled) pixel within r -- r = 0 is the per-pixel POD and 1 - FAR; med_miss, med_false_alarm, the mean error distances
        sum dq / 256 / n over the sources within the cap, and rms_miss, rms_false_alarm; beyond_miss, beyond_false_alarm, the shares of
        sources beyond the cap; hausdorff, the largest non-empty ring over both directions, None when any source is beyond the cap or there
        is no source; hausdorff_q90, the larger over the directions that have sources of the smallest ring that, with the rings below it,
        holds 90 % of the direction's sources, None when that ring is beyond the cap; baddeley, sqrt(total / (frames * pixels of the band))
        / 256, Baddeley's Delta with p = 2 and cut-off R."""
        R = int(radius)
        row0, row1 = (0, int(height)) if row_range is None else (int(row_range[0]), int(row_range[1]))
        cells = int(frames) * (row1 - row0) * int(width)
        out = {}
        for k in range(2):
            entry, rings, quantiles = {}, [], []
            for d, (name, curve) in enumerate((("miss", "pod_within"), ("false_alarm", "success_within"))):
                cell = [int(v) for v in total[k][d]]
                if len(cell) != R + 4:
                    raise L.DeepcamHipError(f"DistanceSkill.decode: a row holds R + 4 = {R + 4} cells, got {len(cell)}")
                n, beyond = sum(cell[:R + 2]), cell[R + 1]
                within, cum = n - beyond, np.cumsum(np.asarray(cell[:R + 1], np.int64)).tolist()
                entry[curve] = [_ratio(c, n) for c in cum]
                entry[f"med_{name}"] = _ratio(cell[R + 2] / DISTANCE_Q, within)
                entry[f"rms_{name}"] = None if within == 0 else math.sqrt(cell[R + 3] / within)
                entry[f"beyond_{name}"] = _ratio(beyond, n)
                rings.append(cell[:R + 2])
                if n:
                    quantiles.append(next(j for j, c in enumerate(cum + [n]) if 10 * c >= 9 * n))
            entry["pixels"] = {"labelled": sum(rings[0]), "predicted": sum(rings[1])}
            occupied = [j for j in range(R + 2) if rings[0][j] or rings[1][j]]
            entry["hausdorff"] = occupied[-1] if occupied and occupied[-1] <= R else None
            entry["hausdorff_q90"] = max(quantiles) if quantiles and max(quantiles) <= R else None
            entry["baddeley"] = None if cells <= 0 else math.sqrt(int(total_baddeley[k]) / cells) / DISTANCE_Q
            out[f"class_{k + 1}"] = entry
        return out


def distance_from_rows(rows, baddeley, radius: int, height: int, width: int, row_range=None) -> list:
    """DistanceSkill.decode of single frames: rows int64 [n, 2, 2, R + 4] and baddeley int64 [n, 2] (what frame_rows() returns, on the
    host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, baddeley = np.asarray(rows), np.asarray(baddeley)
    if rows.ndim != 4 or rows.shape[1:] != (2, 2, int(radius) + 4) or baddeley.shape != (rows.shape[0], 2):
        raise L.DeepcamHipError(f"distance_from_rows: rows [n, 2, 2, R + 4] and baddeley [n, 2], got shapes {rows.shape} and {baddeley.shape}")
    return [DistanceSkill.decode(r, b, 1, radius, height, width, row_range) for r, b in zip(rows.tolist(), baddeley.tolist())]


# ---------------------------------------------------------------------------------------------- displacement verification
DISPLACEMENT_RADIUS = 16
DISPLACEMENT_MAX_RADIUS = 63
DISPLACEMENT_MAX_BATCH = 4095


def displacement_best(table, radius: int):
    """(dy, dx, hits, kept[dy]) of one class's table [2 R + 1][2 R + 2] in Python ints: the most hits, ties to the smaller dy^2 + dx^2, then
    the smaller dy, then the smaller dx -- the order of dc_displacement_score's key; a table without hits gives (0, 0)."""
    R = int(radius)
    hits, _, dy, dx = max((int(table[dy + R][dx + R]), -(dy * dy + dx * dx), -dy, -dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return -dy, -dx, hits, int(table[R - dy][2 * R + 1])


class DisplacementSkill(_MaskSkill):
    """Displacement verification on the device (dc_displacement_score, csrc/displacement.hip): per frame and class (1, 2) the overlap of the
    labelled mask with the predicted mask moved by every (dy, dx), |dy|, |dx| <= radius -- columns periodic, always; rows never: pixels
    moved over a pole are lost --, the predicted pixels each dy keeps inside the band, and the best shift, the one with the most hits: the
    rigid-shift part of the CRA method.  Integers, per frame and as running totals over all frames since reset(); decode() turns a table
    into the shift, the scores without and with it and the CRA decomposition of the error into displacement, volume and pattern.
    1 <= radius <= 63 and 2 radius + 1 <= width.  row_range is the band of LABEL rows scored (a tropics-only score); predicted pixels from
    anywhere in the frame may move into it.  No latitude weighting, no kilometres, no sub-pixel shifts.
    Memory: a workspace of bit planes (dc_displacement_workspace; 3.8 MB at 8 x 768 x 1152, R = 16) beside batch * 2 * (2 R + 1) * (2 R + 2)
    * 8 bytes of rows and the totals.  A call launches on the current stream and does not synchronise; state() and result() read back."""

    # frame_rows(): rows int64 [n_valid, 2, 2 R + 1, 2 R + 2], pixels int64 [n_valid, 2, 2], best int64 [n_valid, 2, 4]
    FRAME_KEYS = ("displacement", "displacement_pixels", "displacement_best")
    _frame, _totals = ("_rows", "_pixels", "_best"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, radius: int = DISPLACEMENT_RADIUS, row_range=None, device=None):
        self._geometry(batch, height, width, DISPLACEMENT_MAX_BATCH)
        R = int(radius)
        if not 1 <= R <= DISPLACEMENT_MAX_RADIUS:
            raise L.DeepcamHipError(f"DisplacementSkill: the radius must lie in [1, {DISPLACEMENT_MAX_RADIUS}], got {radius}")
        if 2 * R + 1 > width:
            raise L.DeepcamHipError(f"DisplacementSkill: the window of 2 * {R} + 1 columns must not be wider than the frame ({width})")
        self._band(row_range)
        self.R = R
        dev = torch.device(device_of(device))
        S = 2 * R + 1
        self._rows = torch.zeros((batch, 2, S, S + 1), dtype=torch.int64, device=dev)
        dev = self.device = self._rows.device
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._best = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, S, S + 1), dtype=torch.int64, device=dev)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_displacement_workspace(batch, height, width, R)
        if size == 0:
            raise L.DeepcamHipError("DisplacementSkill: dc_displacement_workspace refused the shape")
        self._ws = torch.empty((size + 7) // 8, dtype=torch.int64, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_displacement_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.R, self.row_range[0],
               self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._best), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    def state(self) -> dict:
        """on the host, as Python ints: total [2][2 R + 1][2 R + 2], pixels [2][2] and frames"""
        return {"total": [[[int(v) for v in row] for row in cls] for cls in self._total.cpu().tolist()],
                "pixels": [[int(v) for v in cls] for cls in self._total_pixels.cpu().tolist()], "frames": int(self._frames.cpu()[0])}

    def result(self, surface: bool = False) -> dict:
        """decode() of the object's state: one common shift for all frames since reset(), the systematic displacement"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.R, self.H, self.W, self.row_range, surface)

    @staticmethod
    def decode(total, pixels, frames, radius: int, height: int, width: int, row_range=None, surface: bool = False) -> dict:
        """Per class ("class_1", "class_2"), in float64 from the exact integers; None wherever a denominator is 0:
        pixels {"predicted" (whole frame), "labelled" (in the band)}; best, the raw integers [dy, dx, hits, kept[dy]] of the best shift;
        shift {"rows": dy, "cols": dx, "pixels": sqrt(dy^2 + dx^2), "lat_deg", "lon_deg"} by the steps of linspace(-90, 90, H) and
        linspace(-180, 180, W) -- row 0 is -90 degrees, a positive dy is poleward-north; at_edge, |dy| = R or |dx| = R: the window was too
        small; hits_unshifted, hits_shifted; csi, pod, far, each {"unshifted", "shifted"}, from hits, kept[dy] and labelled (CSI = hits /
        (kept[dy] + labelled - hits)); and the CRA decomposition for binary fields with N = frames * band rows * W: mse_total = (kept[0] +
        labelled - 2 hits[0][0]) / N, mse_shifted likewise at the best shift, mse_displacement = mse_total - mse_shifted, mse_volume =
        ((kept[dy] - labelled) / N)^2, mse_pattern = mse_shifted - mse_volume, and share {"displacement", "volume", "pattern"} of
        mse_total.  surface=True adds csi_surface, float64 [2 R + 1][2 R + 1], the CSI of every shift (NaN where undefined)."""
        R = int(radius)
        S = 2 * R + 1
        row0, row1 = (0, int(height)) if row_range is None else (int(row_range[0]), int(row_range[1]))
        N = int(frames) * (row1 - row0) * int(width)
        out = {}
        for k in range(2):
            table = [[int(v) for v in row] for row in total[k]]
            if len(table) != S or any(len(row) != S + 1 for row in table):
                raise L.DeepcamHipError(f"DisplacementSkill.decode: a table holds [2 R + 1][2 R + 2] = [{S}][{S + 1}] cells")
            predicted, labelled = int(pixels[k][0]), int(pixels[k][1])
            dy, dx, hits, kept = displacement_best(table, R)
            hits0, kept0 = table[R][R], table[R][S]
            entry = {"pixels": {"predicted": predicted, "labelled": labelled}, "best": [dy, dx, hits, kept],
                     "shift": {"rows": dy, "cols": dx, "pixels": math.sqrt(dy * dy + dx * dx),
                               "lat_deg": None if height < 2 else dy * 180.0 / (height - 1),
                               "lon_deg": None if width < 2 else dx * 360.0 / (width - 1)},
                     "at_edge": abs(dy) == R or abs(dx) == R, "hits_unshifted": hits0, "hits_shifted": hits}
            both = ((hits0, kept0), (hits, kept))
            entry["csi"] = {n: _ratio(h, kp + labelled - h) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            entry["pod"] = {n: _ratio(h, labelled) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            entry["far"] = {n: _ratio(kp - h, kp) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            if N > 0:
                mse_total, mse_shifted = (kept0 + labelled - 2 * hits0) / N, (kept + labelled - 2 * hits) / N
                volume = ((kept - labelled) / N) ** 2
                parts = {"displacement": mse_total - mse_shifted, "volume": volume, "pattern": mse_shifted - volume}
                entry.update(mse_total=mse_total, mse_shifted=mse_shifted, mse_displacement=parts["displacement"], mse_volume=volume,
                             mse_pattern=parts["pattern"], share={n: _ratio(v, mse_total) for n, v in parts.items()})
            else:
                entry.update(mse_total=None, mse_shifted=None, mse_displacement=None, mse_volume=None, mse_pattern=None,
                             share={"displacement": None, "volume": None, "pattern": None})
            if surface:
                t = np.asarray(table, np.float64)
                union = t[:, S:] + labelled - t[:, :S]
                entry["csi_surface"] = np.where(union > 0, t[:, :S] / np.where(union > 0, union, 1.0), np.nan)
            out[f"class_{k + 1}"] = entry
        return out


def displacement_from_rows(rows, pixels, radius: int, height: int, width: int, row_range=None, surface: bool = False) -> list:
    """DisplacementSkill.decode of single frames: rows int64 [n, 2, 2 R + 1, 2 R + 2] and pixels int64 [n, 2, 2] (what frame_rows()
    returns, on the host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    S = 2 * int(radius) + 1
    if rows.ndim != 4 or rows.shape[1:] != (2, S, S + 1) or pixels.shape != (rows.shape[0], 2, 2):
        raise L.DeepcamHipError(f"displacement_from_rows: rows [n, 2, 2 R + 1, 2 R + 2] and pixels [n, 2, 2], got shapes {rows.shape} and "
                                f"{pixels.shape}")
    return [DisplacementSkill.decode(r, p, 1, radius, height, width, row_range, surface) for r, p in zip(rows.tolist(), pixels.tolist())]


# ---------------------------------------------------------------------------------------------- scale-separation verification
SCALE_MAX_LEVELS = 8
SCALE_MAX_ORIGINS = 8
SCALE_MAX_BATCH = 4095
SCALE_LISTS = ("mse", "mse_share", "skill", "energy_pred", "energy_truth", "energy_rel_diff")


def scale_levels(rows_in_band: int, width: int) -> int:
    """the largest L <= 8 whose tile T = 2^L divides both the rows of the band and the width (7, T = 128, for 768 x 1152); 0 where one
    of them is odd, which ScaleSkill refuses"""
    L_ = 0
    while L_ < SCALE_MAX_LEVELS and int(rows_in_band) % (2 << L_) == 0 and int(width) % (2 << L_) == 0:
        L_ += 1
    return L_


def _scale_components(q) -> list:
    """the Haar components E_0 .. E_L as Fractions from the block sums Q_0 .. Q_L of one term: E_j = (4 Q_j - Q_{j+1}) / 4^(j+1) for
    j < L, E_L = Q_L / 4^L"""
    n = len(q) - 1
    return [Fraction(4 * q[j] - q[j + 1], 4 ** (j + 1)) for j in range(n)] + [Fraction(q[n], 4 ** n)]


class ScaleSkill(_MaskSkill):
    """Scale-separation verification on the device (dc_scale_score, csrc/scale.hip): the integers behind the intensity-scale skill score
    (Casati, Ross & Stephenson 2004; energies: Casati 2010).  Per frame, class (1, 2), column origin and level j = 0 .. levels the sums
    (A, B, C) = (sum (S_F - S_O)^2, sum S_F^2, sum S_O^2) over the disjoint blocks of side 2^j GRID PIXELS that tile the rows row_range
    from (row0, origin) on, S_F and S_O the predicted and labelled pixels of the class in a block -- columns periodic, always; rows never
    --, and their running totals over all frames since reset() as two-word integers.  decode() turns them, in exact arithmetic, into the
    squared error and the energies of the 2-D Haar components of scale 1, 2, ..., 2^levels pixels.  The tile T = 2^levels must divide
    both the rows of the band and the width; levels=None takes scale_levels(), the largest that does.  origins: 1 to 8 column offsets in
    [0, T) of the dyadic grid, scored in one pass: their spread shows how much a result owes to where the grid falls.  No latitude
    weighting, no kilometres, tiles instead of the whole domain, and "intensity" is the class, not a threshold ladder.
    Memory: batch * 2 * O * (levels + 1) * 3 * 8 bytes of rows and a workspace of 16 bytes per 64 x 64 tile and origin
    (dc_scale_workspace); no per-pixel buffer.  A call launches on the current stream and does not synchronise; state() and result() read
    back."""

    FRAME_KEYS = ("scale", "scale_pixels")            # frame_rows(): int64 [n_valid, 2, O, levels + 1, 3], int64 [n_valid, 2, 2]
    _frame, _totals = ("_rows", "_pixels"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, levels: Optional[int] = None, origins: Sequence[int] = (0,), row_range=None,
                 device=None):
        self._geometry(batch, height, width, SCALE_MAX_BATCH)
        row0, row1 = self._band(row_range)
        lv = scale_levels(row1 - row0, width) if levels is None else int(levels)
        if levels is None and lv < 1:
            raise L.DeepcamHipError(f"ScaleSkill: levels=None needs an even number of rows in the band and an even width, got {row1 - row0} "
                                    f"and {width}")
        if not 1 <= lv <= SCALE_MAX_LEVELS:
            raise L.DeepcamHipError(f"ScaleSkill: levels must lie in [1, {SCALE_MAX_LEVELS}], got {levels}")
        T = 1 << lv
        if (row1 - row0) % T or width % T:
            raise L.DeepcamHipError(f"ScaleSkill: the tile 2^levels = {T} must divide the rows of the band ({row1 - row0}) and the width "
                                    f"({width})")
        try:
            origins = [int(c) for c in origins]
        except TypeError:
            raise L.DeepcamHipError(f"ScaleSkill: origins is a sequence of column offsets, got {origins!r}") from None
        if not 1 <= len(origins) <= SCALE_MAX_ORIGINS:
            raise L.DeepcamHipError(f"ScaleSkill: between 1 and {SCALE_MAX_ORIGINS} origins, got {len(origins)}")
        for c in origins:
            if not 0 <= c < T:
                raise L.DeepcamHipError(f"ScaleSkill: an origin is a column offset in [0, {T}), got {c}")
        self.L, self.O, self.origins = lv, len(origins), origins
        dev = torch.device(device_of(device))
        self._origins = torch.tensor(origins, dtype=torch.int32, device=dev)
        dev = self.device = self._origins.device
        self._rows = torch.zeros((batch, 2, self.O, lv + 1, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, self.O, lv + 1, 3, 2), dtype=torch.int64, device=dev)          # (lo, hi)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_scale_workspace(batch, height, width, lv, self.O)
        if size == 0:
            raise L.DeepcamHipError("ScaleSkill: dc_scale_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_scale_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.L, self.O, L.dptr(self._origins),
               self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    @staticmethod
    def combine(total_words) -> list:
        """[2][O][levels + 1][3] Python ints from the int64 words [2, O, levels + 1, 3, 2] = (lo, hi): (hi << 64) | lo, lo unsigned"""
        words = np.asarray(total_words, np.int64)
        if words.ndim != 5 or words.shape[0] != 2 or words.shape[3:] != (3, 2):
            raise L.DeepcamHipError(f"ScaleSkill: the totals are int64 [2, O, levels + 1, 3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: total [2][O][levels + 1][3] as Python ints, pixels [2][2] ((pred, truth) per class) and frames as ints"""
        return {"total": self.combine(self._total.cpu().numpy()), "pixels": [[int(v) for v in row] for row in self._total_pixels.cpu().tolist()],
                "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.L, self.row_range[1] - self.row_range[0], self.W, self.origins)

    @staticmethod
    def decode(total, pixels, frames, levels: int, rows_in_band: int, width: int, origins=None) -> dict:
        """Per class ("class_1", "class_2"), computed in exact arithmetic (Python ints and fractions.Fraction) from total [2][O][levels +
        1][3] and pixels [2][2]; every reported number is one float() of the exact value, None wherever a denominator is 0.  With N =
        frames * rows_in_band * width and Q_j one of A, B, C at level j, the Haar component of scale 2^j carries E_j = (4 Q_j - Q_{j+1}) /
        4^(j+1) for j < levels (the detail between block means of side 2^j and 2^(j+1)) and E_L = Q_L / 4^L (the father component: the
        TILE means, not the domain mean).  Per origin, lists over j = 0 .. levels: mse = E_j(A) / N, which sum to the per-pixel error
        rate; mse_share = E_j(A) / A_0; skill = 1 - mse (levels + 1) / mse_random with mse_random = p (1 - o) + o (1 - p), p and o the
        pooled predicted and labelled rates -- Casati's equipartition of the random error over the levels + 1 components;
        energy_pred = E_j(B) / N, energy_truth = E_j(C) / N, energy_rel_diff = (pred - truth) / (pred + truth).
        The entry holds pixels {"predicted", "labelled"}, base_rate = labelled / N, bias = predicted / labelled, mse_random, scales =
        [1, 2, ..., 2^levels], the six lists as the exact mean over the origins (energy_rel_diff from the mean energies), by_origin (a
        list of {"origin", the six lists}), origin_spread (max - min of mse[j] over the origins) and skilful_scale: the smallest 2^j from
        which the mean skill of every component up to levels - 1 is positive, else None."""
        n = int(levels)
        N = int(frames) * int(rows_in_band) * int(width)
        out = {}
        for k in range(2):
            table = [[[int(v) for v in level] for level in origin] for origin in total[k]]
            if not table or any(len(origin) != n + 1 or any(len(level) != 3 for level in origin) for origin in table):
                raise L.DeepcamHipError(f"ScaleSkill.decode: a class holds [O][levels + 1][3] = [O][{n + 1}][3] cells")
            O = len(table)
            names = list(range(O)) if origins is None else [int(c) for c in origins]
            if len(names) != O:
                raise L.DeepcamHipError(f"ScaleSkill.decode: {len(names)} origins for a table of {O}")
            predicted, labelled = int(pixels[k][0]), int(pixels[k][1])
            rnd = None if N == 0 else Fraction(predicted * (N - labelled) + labelled * (N - predicted), N * N)
            per = []                                  # per origin: the exact lists
            for origin in table:
                ea, eb, ec = (_scale_components([level[i] for level in origin]) for i in range(3))
                a0 = origin[0][0]
                per.append({"mse": [None if N == 0 else e / N for e in ea], "mse_share": [None if a0 == 0 else e / a0 for e in ea],
                            "energy_pred": [None if N == 0 else e / N for e in eb], "energy_truth": [None if N == 0 else e / N for e in ec]})
            mean = {name: [None if per[0][name][j] is None else sum(p[name][j] for p in per) / O for j in range(n + 1)] for name in per[0]}
            for entry in per + [mean]:
                entry["skill"] = [None if not rnd else 1 - m * (n + 1) / rnd for m in entry["mse"]]
                entry["energy_rel_diff"] = [None if p is None or p + t == 0 else (p - t) / (p + t)
                                            for p, t in zip(entry["energy_pred"], entry["energy_truth"])]
            good = None
            for j in range(n - 1, -1, -1):            # the component n is the father: tile means, not a scale's detail
                if mean["skill"][j] is None or mean["skill"][j] <= 0:
                    break
                good = 1 << j
            entry = {"pixels": {"predicted": predicted, "labelled": labelled}, "base_rate": None if N == 0 else labelled / N,
                     "bias": None if labelled == 0 else predicted / labelled, "mse_random": _float(rnd), "scales": [1 << j for j in range(n + 1)]}
            entry.update({name: [_float(v) for v in mean[name]] for name in SCALE_LISTS})
            entry["by_origin"] = [dict({"origin": c}, **{name: [_float(v) for v in p[name]] for name in SCALE_LISTS}) for c, p in zip(names, per)]
            entry["origin_spread"] = [None if N == 0 else float(max(p["mse"][j] for p in per) - min(p["mse"][j] for p in per))
                                      for j in range(n + 1)]
            entry["skilful_scale"] = good
            out[f"class_{k + 1}"] = entry
        return out


def scale_from_rows(rows, pixels, levels: int, rows_in_band: int, width: int, origins=None) -> list:
    """ScaleSkill.decode of single frames: rows int64 [n, 2, O, levels + 1, 3] and pixels int64 [n, 2, 2] (what frame_rows() returns, on
    the host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    if rows.ndim != 5 or rows.shape[1] != 2 or rows.shape[3:] != (int(levels) + 1, 3) or pixels.shape != (rows.shape[0], 2, 2):
        raise L.DeepcamHipError(f"scale_from_rows: rows [n, 2, O, levels + 1, 3] and pixels [n, 2, 2], got shapes {rows.shape} and "
                                f"{pixels.shape}")
    return [ScaleSkill.decode(r, p, 1, levels, rows_in_band, width, origins) for r, p in zip(rows.tolist(), pixels.tolist())]


# ---------------------------------------------------------------------------------------------- probabilistic verification
PROB_BINS = 20
PROB_MAX_BINS = 256
PROB_MAX_BATCH = 4095
PROB_MAX_PIXELS = 1 << 30
PROB_ONE = 65536                                  # q = rint(p * PROB_ONE)


def brier_from_rows(rows, pixels):
    """The Brier scores of single frames from ProbabilitySkill.frame_rows(): rows [..., 3] = sum (q_c - o_c * 65536)^2 per class, pixels
    [..., 3] = (scored, bad label, logit not finite); rows / (scored * 2^32) as nested lists of Python floats of rows' shape, None where no
    pixel was scored."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    if rows.shape[-1:] != (3,) or pixels.shape != rows.shape:
        raise L.DeepcamHipError(f"brier_from_rows: rows and pixels must both be [..., 3], got {rows.shape} and {pixels.shape}")
    n = pixels.reshape(-1, 3)[:, 0].tolist()
    out = np.empty((len(n), 3), dtype=object)
    for i, (row, scored) in enumerate(zip(rows.reshape(-1, 3).tolist(), n)):
        out[i] = [_ratio(int(v), int(scored) << 32) for v in row]
    return out.reshape(rows.shape).tolist()


class ProbabilitySkill:
    """Probabilistic verification on the device (dc_prob_score, csrc/probskill.hip): from the classifier's fp32 logits and the labels, per
    class c the joint histogram of (probability bin, label == c) with the sum of the probabilities per cell, and the sum of the squared
    errors -- one streaming pass --, as integers: q_c = rint(softmax_c * 65536), bin = min(bins - 1, (q_c * bins) >> 16).  Running totals
    over all frames since reset(); the squared errors as two-word integers.  decode() turns the integers into the reliability diagram,
    the Brier score with Murphy's (1973) decomposition, ECE / MCE, and POD / POFD / CSI / bias per threshold k / bins with the ROC area
    (Mason 1982).  Pixels whose label is outside [0, 3) or whose logits are not finite are counted and left out.  No latitude weighting.
    Memory: (2 * 3 * 2 * bins * 2 + 2 * batch * 3 + 10) * 8 bytes.  A call launches on the current stream and does not synchronise; state()
    and result() read back."""

    FRAME_KEYS = ("prob", "prob_pixels")              # frame_rows(); the driver stores `brier` (brier_from_rows) in place of the raw rows

    def __init__(self, batch: int, height: int, width: int, bins: int = PROB_BINS, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"ProbabilitySkill: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        bins = int(bins)
        if not 1 <= bins <= PROB_MAX_BINS:
            raise L.DeepcamHipError(f"ProbabilitySkill: bins must lie in [1, {PROB_MAX_BINS}], got {bins}")
        self.B, self.H, self.W, self.K = batch, height, width, bins
        dev = torch.device(device_of(device))
        self._hist = torch.zeros((3, 2, bins, 2), dtype=torch.int64, device=dev)
        dev = self.device = self._hist.device
        self._rows = torch.zeros((batch, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 3), dtype=torch.int64, device=dev)
        self._total_hist = torch.zeros((3, 2, bins, 2), dtype=torch.int64, device=dev)
        self._total_sq = torch.zeros((3, 2), dtype=torch.int64, device=dev)                  # (lo, hi)
        self._total_pixels = torch.zeros((3,), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._nv = 0

    def __call__(self, logits: torch.Tensor, labels: torch.Tensor, n_valid: Optional[int] = None) -> "ProbabilitySkill":
        """logits: contiguous device fp32 [B, 3, H, W]; labels: contiguous device uint8, int32 or int64 [B, H, W]; the frames from n_valid
        on are not read."""
        check_tensor("ProbabilitySkill", "logits", logits, (torch.float32,), (self.B, 3, self.H, self.W), self.device)
        check_tensor("ProbabilitySkill", "labels", labels, tuple(_BYTES), (self.B, self.H, self.W), self.device)
        nv = _n_valid("ProbabilitySkill", n_valid, self.B)
        L.call("dc_prob_score", self.B, nv, self.H, self.W, L.dptr(logits), L.dptr(labels), _BYTES[labels.dtype], self.K,
               L.dptr(self._hist), L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total_hist), L.dptr(self._total_sq),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.stream_ptr())
        self._nv = nv
        return self

    def frame_rows(self):
        """(int64 [n_valid, 3], int64 [n_valid, 3]) of the last call: per frame and class the sum of squared errors, and the pixel
        counters (scored, bad label, not finite); views of the object's device buffers, not synchronised"""
        return self._rows[:self._nv], self._pixels[:self._nv]

    def batch_hist(self) -> torch.Tensor:
        """int64 [3, 2, bins, 2] of the last call: class, outcome, bin, (n, sum q); the object's device buffer, not synchronised"""
        return self._hist

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        for t in (self._total_hist, self._total_sq, self._total_pixels, self._frames):
            t.zero_()

    @staticmethod
    def combine(words) -> list:
        """[3] Python ints from the int64 words [3, 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned (FractionsSkill's convention)"""
        words = np.asarray(words, np.int64)
        if words.shape != (3, 2):
            raise L.DeepcamHipError(f"ProbabilitySkill: the squared-error totals are int64 [3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: hist int64 [3, 2, bins, 2], sq [3] as Python ints, pixels [3] and frames as ints"""
        return {"hist": self._total_hist.cpu().numpy(), "sq": self.combine(self._total_sq.cpu().numpy()),
                "pixels": [int(v) for v in self._total_pixels.cpu().tolist()], "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["hist"], s["sq"], s["pixels"], self.K)

    @staticmethod
    def decode(hist, sq, pixels, bins: int) -> dict:
        """Per class ("class_0", "class_1", "class_2"), in float64 from the exact integers hist [3][2][bins][2] = (n, sum q) per (outcome,
        bin), sq [3] and pixels [3]:
          n, base_rate (o = labelled share), mean_probability, brier = sq / (n * 2^32), brier_skill = 1 - brier / (o (1 - o)),
          reliability = sum_k n_k (f_k - o_k)^2 / n, resolution = sum_k n_k (o_k - o)^2 / n, uncertainty = o (1 - o) (Murphy 1973; f_k =
          sum q / n_k / 65536 the bin's mean forecast, o_k its observed frequency), ece = sum_k n_k |f_k - o_k| / n, mce = max_k |f_k - o_k|,
          curve {mean_probability, observed_frequency, n} per bin, sharpness n_k / n per bin,
          pod, pofd, csi, bias at the thresholds k / bins, k = 0 .. bins (the forecast is "bin >= k": k = 0 says yes everywhere, k = bins
          nowhere), auc by trapezoids over the (pofd, pod) points, best_csi and best_csi_threshold (the smallest among equals).
        A value is None where its denominator is zero.  "pixels" holds the three counters."""
        K = int(bins)
        h = np.asarray(hist, np.int64)
        if h.shape != (3, 2, K, 2):
            raise L.DeepcamHipError(f"ProbabilitySkill.decode: hist must be [3, 2, {K}, 2], got {h.shape}")
        h = h.tolist()
        out = {"bins": K, "pixels": {"scored": int(pixels[0]), "bad_label": int(pixels[1]), "not_finite": int(pixels[2])}}
        for c in range(3):
            n0, n1 = [cell[0] for cell in h[c][0]], [cell[0] for cell in h[c][1]]
            qk = [a[1] + b[1] for a, b in zip(h[c][0], h[c][1])]
            nk = [a + b for a, b in zip(n0, n1)]
            N0, N1 = sum(n0), sum(n1)
            N = N0 + N1
            base = _ratio(N1, N)
            unc = None if base is None else base * (1.0 - base)
            brier = _ratio(int(sq[c]), N << 32)
            fk = [_ratio(q, n * PROB_ONE) for q, n in zip(qk, nk)]
            ok = [_ratio(o, n) for o, n in zip(n1, nk)]
            full = [k for k in range(K) if nk[k]]
            rel = res = ece = mce = None
            if N:
                rel = sum(nk[k] * (fk[k] - ok[k]) ** 2 for k in full) / N
                res = sum(nk[k] * (ok[k] - base) ** 2 for k in full) / N
                ece = sum(nk[k] * abs(fk[k] - ok[k]) for k in full) / N
                mce = max(abs(fk[k] - ok[k]) for k in full)
            hits, alarms = [0] * (K + 1), [0] * (K + 1)     # labelled / unlabelled pixels in the bins >= k
            for k in range(K - 1, -1, -1):
                hits[k], alarms[k] = hits[k + 1] + n1[k], alarms[k + 1] + n0[k]
            pod = [_ratio(a, N1) for a in hits]
            pofd = [_ratio(b, N0) for b in alarms]
            csi = [_ratio(a, N1 + b) for a, b in zip(hits, alarms)]          # hits / (hits + misses + false alarms)
            bias = [_ratio(a + b, N1) for a, b in zip(hits, alarms)]
            auc = None
            if N0 and N1:
                auc = sum((pofd[k] - pofd[k + 1]) * (pod[k] + pod[k + 1]) / 2 for k in range(K))
            best = None
            for k in range(K + 1):
                if csi[k] is not None and (best is None or csi[k] > csi[best]):
                    best = k
            out[f"class_{c}"] = {
                "n": N, "base_rate": base, "mean_probability": _ratio(sum(qk), N * PROB_ONE), "brier": brier,
                "brier_skill": None if brier is None or not unc else 1.0 - brier / unc, "reliability": rel, "resolution": res,
                "uncertainty": unc, "ece": ece, "mce": mce, "curve": {"mean_probability": fk, "observed_frequency": ok, "n": nk},
                "sharpness": [_ratio(n, N) for n in nk], "pod": pod, "pofd": pofd, "csi": csi, "bias": bias, "auc": auc,
                "best_csi": None if best is None else csi[best], "best_csi_threshold": None if best is None else best / K}
        return out
