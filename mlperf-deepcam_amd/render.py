"""Frame renderer (utils/visualizer.py: CamVisualizer.plot, called from train_hdf5_ddp.py:374-394,463-476)."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import lib as L
from ._args import _BYTES, MASK_KIND, _c_int, check_tensor, device_of


def gall_rows(height: int, width: int) -> np.ndarray:
    """int32 [Ho]: the source row of every output row of a Gall stereographic picture `width` pixels wide, whose height over width is
    (1 + sqrt(2) / 2) * 2 / (sqrt(2) * pi): Ho = round(width * (2 + sqrt(2)) / (sqrt(2) * pi)), 885 for 1152.  Output row y shows the
    latitude 2 * atan(1 - 2 * (y + 1/2) / Ho); its source row is the nearest one of linspace(-90, 90, height).  North is at the top: the
    table runs from height - 1 down to 0.  The lower half mirrors the upper one (t[y] + t[Ho - 1 - y] = height - 1); with Ho odd the
    middle row shows the equator, which lies between two source rows when height is even."""
    ho = int(round(width * (2.0 + math.sqrt(2.0)) / (math.sqrt(2.0) * math.pi)))
    y = np.arange(ho, dtype=np.float64)
    lat = np.rad2deg(2.0 * np.arctan(1.0 - 2.0 * (y + 0.5) / ho))
    t = np.rint((lat + 90.0) / 180.0 * (height - 1)).astype(np.int64)
    half = ho // 2
    t[ho - half:] = (height - 1 - t[:half])[::-1]
    return np.clip(t, 0, height - 1).astype(np.int32)


def plate_rows(height: int) -> np.ndarray:
    """int32 [height]: every source row once, north (the last row) at the top"""
    return np.arange(height - 1, -1, -1, dtype=np.int32)


RENDER_BACKGROUND = (12, 20, 44)
_RAMP = ((0.0, (20, 40, 90)), (0.35, (30, 120, 160)), (0.7, (130, 200, 190)), (1.0, (250, 250, 235)))


def render_palette(n: int = 64) -> np.ndarray:
    """uint8 [n, 3]: the renderer's colour table for the normalised field, entry i for u = i / (n - 1).  A piecewise-linear ramp (_RAMP:
    deep blue, teal, pale green, near white) whose opacity u^0.75 grows with the value, composited over RENDER_BACKGROUND: dry air
    fades into the background, moist air stands out.  This project's own table; the reference's colour formula is not reproduced."""
    if not 1 <= int(n) <= 256:
        raise L.DeepcamHipError(f"render_palette: n must lie in [1, 256], got {n}")
    u = np.linspace(0.0, 1.0, int(n)) if n > 1 else np.asarray([1.0])
    stops = np.asarray([s[0] for s in _RAMP])
    ramp = np.stack([np.interp(u, stops, [s[1][k] for s in _RAMP]) for k in range(3)], axis=1)
    alpha = (u ** 0.75)[:, None]
    return np.rint(alpha * ramp + (1.0 - alpha) * np.asarray(RENDER_BACKGROUND, np.float64)).astype(np.uint8)


def graticule(rows, width: int, shift: int, parallels: float = 30, meridians: float = 60, height: Optional[int] = None):
    """(row_line uint8 [Ho], col_line uint8 [width]) for a table of source rows: 1 where a graticule line runs.  A parallel every
    `parallels` degrees strictly between the poles, on the output row whose source row is nearest to the parallel's (source rows are
    linspace(-90, 90, height); height defaults to the table's largest entry + 1).  A meridian every `meridians` degrees from longitude 0 =
    source column 0 (columns are longitudes 360 * c / width), on output column (c - shift) mod width.  0 switches either family off."""
    t = np.asarray(rows, np.int64).reshape(-1)
    if height is None:
        height = int(max(t.max(), 0)) + 1
    t = np.clip(t, 0, height - 1)
    row_line, col_line = np.zeros(len(t), np.uint8), np.zeros(width, np.uint8)
    if parallels and parallels > 0 and height > 1:
        k = 1
        while k * parallels < 90.0:
            for lat in (k * parallels, -k * parallels):
                row_line[int(np.argmin(np.abs(t - (lat + 90.0) / 180.0 * (height - 1))))] = 1
            k += 1
        row_line[int(np.argmin(np.abs(t - 0.5 * (height - 1))))] = 1
    if meridians and meridians > 0:
        k = 0
        while k * meridians < 360.0:
            col_line[(int(round(k * meridians / 360.0 * width)) - shift) % width] = 1
            k += 1
    return row_line, col_line


RENDER_COLOURS = {"missing": 0x404040, "line": 0x50FFFFFF, "class1": 0xFFFF4030, "class2": 0xFFFFE040}


class FrameRenderer:
    """The visualiser's picture on the device (dc_render_frames, csrc/render.hip): per sample `panels` panels stacked, the first with
    mask_a's classes outlined (the prediction), the second with mask_b's (the labels), over channel `channel` of the raw fields drawn
    through `palette` across [lo, hi].  projection: "gall" (gall_rows), "plate" (every row once) or an int32 array of source rows, north
    first; shift: the column roll, width // 2 by default (longitude 0 in the middle); outline: the outlines' width in source pixels, 1,
    3, 5 or 7; colours: RENDER_COLOURS with any of its entries replaced (missing 0xRRGGBB, the others 0xAARRGGBB).  The object owns the
    colour table, the row table, the graticule tables, the workspace and the output buffer.  A call launches on the current stream and
    does not synchronise; what it returns is a view of the output buffer, which the next call overwrites."""

    def __init__(self, batch: int, height: int, width: int, channel: int = 0, ldc: int = 16, lo: float = 0.0, hi: float = 1.0,
                 palette=None, projection="gall", outline: int = 3, panels: int = 2, colours: Optional[dict] = None, device=None,
                 shift: Optional[int] = None, parallels: float = 30, meridians: float = 60):
        if batch < 1 or height < 1 or width < 8 or height * width >= 1 << 31:
            raise L.DeepcamHipError("FrameRenderer: batch and height must be positive, width at least 8 and height * width below 2^31")
        if panels not in (1, 2) or outline not in (1, 3, 5, 7) or not 0 <= channel < ldc:
            raise L.DeepcamHipError(f"FrameRenderer: panels must be 1 or 2, outline 1, 3, 5 or 7 and channel in [0, ldc), got {panels}, "
                                    f"{outline}, {channel} of {ldc}")
        self.B, self.H, self.W, self.P, self.channel, self.ldc, self.outline = batch, height, width, panels, channel, ldc, outline
        span = np.float32(hi) - np.float32(lo)
        if not (np.isfinite(np.float32(lo)) and np.isfinite(span) and span > 0):
            raise L.DeepcamHipError(f"FrameRenderer: lo and hi must be finite with hi > lo in fp32, got {lo}, {hi}")
        self.lo = float(np.float32(lo))
        self.scale = float(np.float32(1.0) / span)
        self.palette = np.ascontiguousarray(render_palette() if palette is None else palette)
        if self.palette.dtype != np.uint8 or self.palette.ndim != 2 or self.palette.shape[1] != 3 or not 1 <= len(self.palette) <= 256:
            raise L.DeepcamHipError("FrameRenderer: palette must be uint8 [n, 3] with 1 <= n <= 256")
        if isinstance(projection, str):
            if projection not in ("gall", "plate"):
                raise L.DeepcamHipError(f"FrameRenderer: projection must be 'gall', 'plate' or a table of rows, got {projection!r}")
            self.rows = gall_rows(height, width) if projection == "gall" else plate_rows(height)
        else:
            self.rows = np.ascontiguousarray(np.asarray(projection, np.int32).reshape(-1))
        self.Ho = len(self.rows)
        if self.Ho < 1 or self.Ho * width >= 1 << 31:
            raise L.DeepcamHipError("FrameRenderer: the row table must hold at least one row and Ho * width stay below 2^31")
        self.shift = width // 2 if shift is None else int(shift)
        if not 0 <= self.shift < width:
            raise L.DeepcamHipError(f"FrameRenderer: shift must lie in [0, {width}), got {shift}")
        self.colours = dict(RENDER_COLOURS, **(colours or {}))
        if set(self.colours) != set(RENDER_COLOURS):
            raise L.DeepcamHipError(f"FrameRenderer: colours has the entries {sorted(RENDER_COLOURS)}")
        self.lines = graticule(self.rows, width, self.shift, parallels, meridians, height=height)
        dev = torch.device(device_of(device))
        self._lut = torch.from_numpy(self.palette).to(dev)
        dev = self.device = self._lut.device       # with its index, whatever form `device` came in
        self._rows = torch.from_numpy(self.rows).to(dev)
        self._row_line, self._col_line = (torch.from_numpy(t).to(dev) for t in self.lines)
        self._ws = torch.empty(max(L.load().dc_render_workspace(batch, panels, height, width), 256), dtype=torch.uint8, device=dev)
        self._out = torch.zeros((batch, panels, self.Ho, width, 3), dtype=torch.uint8, device=dev)

    def _mask(self, m: torch.Tensor, name: str) -> int:
        check_tensor("FrameRenderer", name, m, _BYTES, (self.B, self.H, self.W), self.device, MASK_KIND)
        return _BYTES[m.dtype]

    def __call__(self, fields: torch.Tensor, mask_a: torch.Tensor, mask_b: Optional[torch.Tensor] = None,
                 n_valid: Optional[int] = None) -> torch.Tensor:
        """fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw); mask_a (and, with two panels, mask_b): device
        uint8, int32 or int64 [B, H, W].  Returns uint8 [n_valid, panels * Ho, W, 3]: per sample the panels stacked."""
        check_tensor("FrameRenderer", "fields", fields, (torch.float32,), (self.B, self.H, self.W, self.ldc), self.device, "fp32")
        if (mask_b is None) != (self.P == 1):
            raise L.DeepcamHipError(f"FrameRenderer: built for {self.P} panel(s): mask_b is given exactly when there are two")
        a_bytes = self._mask(mask_a, "mask_a")
        b_bytes = self._mask(mask_b, "mask_b") if mask_b is not None else 0
        nv = self.B if n_valid is None else int(n_valid)
        if not 0 < nv <= self.B:
            raise L.DeepcamHipError(f"FrameRenderer: n_valid must lie in [1, {self.B}], got {n_valid}")
        c = self.colours
        L.call("dc_render_frames", self.B, nv, self.H, self.W, L.dptr(fields), self.channel, self.ldc, self.lo, self.scale,
               L.dptr(self._lut), len(self.palette), L.dptr(mask_a), a_bytes, L.dptr(mask_b), b_bytes, L.dptr(self._rows), self.Ho,
               self.shift, L.dptr(self._row_line), L.dptr(self._col_line), _c_int(c["missing"]), _c_int(c["line"]), _c_int(c["class1"]),
               _c_int(c["class2"]), self.outline, L.dptr(self._out), L.dptr(self._ws), L.stream_ptr())
        return self._out[:nv].view(nv, self.P * self.Ho, self.W, 3)
