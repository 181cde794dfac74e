"""Climatology: the maps over time (Climatology), and storm-centred composites (StormComposite)."""
from __future__ import annotations

import os
import re
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from ._args import _BYTES, MASK_KIND, _c_int, _n_valid, check_tensor, device_of, group_table
from .events import EARTH_RADIUS_KM, event_weight_tables

CLIMATOLOGY_ROWS = ("all", "class1", "class2")
CLIMATOLOGY_PRODUCTS = {"frequency": 0, "mean": 1, "share": 2}
CLIMATOLOGY_MAX_FRAMES = (1 << 31) - 1
CLIMATOLOGY_GROUPS = {"all": ("all",), "month": tuple(f"{m:02d}" for m in range(1, 13)), "season": ("DJF", "MAM", "JJA", "SON")}
_SEASON_OF_MONTH = (0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0)                      # DJF, MAM, JJA, SON
_DATE = re.compile(r"(\d{4})-(\d{2})-(\d{2})")


def climatology_group(name: str, by: str = "all") -> int:
    """The group of a file from its base name: by = "all": 0; "month": 0 .. 11; "season": DJF, MAM, JJA, SON -> 0 .. 3 (December is season
    0).  The date is the first YYYY-MM-DD in the name; a name without one (or with a month outside 1 .. 12) is an error unless by is
    "all"."""
    if by not in CLIMATOLOGY_GROUPS:
        raise L.DeepcamHipError(f"climatology_group: by must be 'all', 'month' or 'season', got {by!r}")
    if by == "all":
        return 0
    m = _DATE.search(os.path.basename(str(name)))
    month = int(m.group(2)) if m else 0
    if not 1 <= month <= 12:
        raise L.DeepcamHipError(f"climatology_group: no YYYY-MM-DD date in {name!r}")
    return month - 1 if by == "month" else _SEASON_OF_MONTH[month - 1]


class Climatology:
    """Occurrence and class-conditional field maps over time, accumulated on the device (dc_climatology_accumulate, dc_climatology_maps,
    csrc/climatology.hip): per group (1, 4 seasons, 12 months) how many frames a pixel spent inside class 1 / class 2, and per selected
    channel of the raw fields the sum and number of its values over all frames, over the class-1 frames and over the class-2 frames of the
    pixel -- the frequency of cyclones and rivers, the mean field inside them, the share of a field's total they account for.
    channels: indices into the ldc channels of a pixel (ldc defaults to the largest index + 1); bits: the sums' binary scale per SELECTED
    channel (event_field_bits).  The object owns frames (int64 [G]), count (int32 [G, 2, H, W]), sum (int64 [G, 3, H, W, C]) and n (int32
    [G, 3, H, W, C]); everything is an integer sum, so the state does not depend on how a sequence was cut into batches or ordered.
    Memory: G * H * W * (8 + 36 * C) bytes -- 8 for the two counts, 3 * (8 + 4) per selected channel.  768 x 1152 with 16 channels and
    one group: 884736 * 584 = 516.7 MB (12 months: 6.2 GB; without channels 7.1 MB per group).
    A call launches on the current stream and does not synchronise; state() and maps() read back."""

    def __init__(self, batch: int, height: int, width: int, channels: Sequence[int] = (), bits=None, ldc: Optional[int] = None,
                 groups: int = 1, device=None):
        channels = [int(c) for c in channels]
        C = len(channels)
        if batch < 1 or batch > 65535 or height < 1 or width < 1 or height * width >= 1 << 31:
            raise L.DeepcamHipError("Climatology: batch must lie in [1, 65535], height and width be positive and height * width below 2^31")
        if not 1 <= int(groups) <= 65536:
            raise L.DeepcamHipError(f"Climatology: groups must lie in [1, 65536], got {groups}")
        if C > 32:
            raise L.DeepcamHipError(f"Climatology: at most 32 channels, got {C}")
        ldc = int((max(channels) + 1 if C else 0) if ldc is None else ldc)
        if C and (min(channels) < 0 or max(channels) >= ldc):
            raise L.DeepcamHipError(f"Climatology: channels must lie in [0, {ldc}), got {channels}")
        bits = [] if bits is None else [int(v) for v in np.asarray(bits).reshape(-1)]
        if len(bits) != C:
            raise L.DeepcamHipError(f"Climatology: {len(bits)} scale bits for {C} channels")
        self.B, self.H, self.W, self.C, self.ldc, self.G = batch, height, width, C, ldc, int(groups)
        self.channels, self.bits = channels, bits
        dev = torch.device(device_of(device))
        self._frames = torch.zeros((self.G,), dtype=torch.int64, device=dev)
        dev = self.device = self._frames.device
        self._count = torch.zeros((self.G, 2, height, width), dtype=torch.int32, device=dev)
        self._sum = torch.zeros((self.G, 3, height, width, C), dtype=torch.int64, device=dev) if C else None
        self._n = torch.zeros((self.G, 3, height, width, C), dtype=torch.int32, device=dev) if C else None
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev) if C else None
        # the identity over all ldc channels travels as a null table: the library then knows it on the host and may take its 16-byte loads
        self._chan = None if channels == list(range(ldc)) else torch.tensor(channels, dtype=torch.int32, device=dev)
        self._tables = {}                            # group tuple -> device int32 [B]: a time-sorted sequence produces few distinct ones
        self._products = {}                          # product tuple -> (device int32 [K, 3], out fp32 [G, H, W, K], contour uint8 [G, H, W])
        self.host_frames = [0] * self.G              # the device's `frames`, counted here too: the overflow bound needs no read-back

    def __call__(self, mask: torch.Tensor, fields: Optional[torch.Tensor] = None, groups=None, n_valid: Optional[int] = None) -> "Climatology":
        """mask: contiguous device uint8, int32 or int64 [B, H, W]; fields: contiguous device fp32 [B, H, W, ldc] in physical units
        (InputPipeline.raw), given exactly when channels were selected; groups: None (every frame to group 0), an int, or B ints, a
        negative one skipping its frame; frames from n_valid on are skipped."""
        check_tensor("Climatology", "mask", mask, _BYTES, (self.B, self.H, self.W), self.device, MASK_KIND)
        if (fields is None) != (self.C == 0):
            raise L.DeepcamHipError(f"Climatology: built for {self.C} channel(s): fields are given exactly when there are some")
        if fields is not None:
            check_tensor("Climatology", "fields", fields, (torch.float32,), (self.B, self.H, self.W, self.ldc), self.device, "fp32")
        table = group_table("Climatology", groups, self.B, _n_valid("Climatology", n_valid, self.B), self.G)
        added = [0] * self.G
        for g in table:
            if g >= 0:
                added[g] += 1
        if any(h + a > CLIMATOLOGY_MAX_FRAMES for h, a in zip(self.host_frames, added)):
            raise L.DeepcamHipError(f"Climatology: a group would pass {CLIMATOLOGY_MAX_FRAMES} frames, the bound of the int32 counts")
        if not any(added):
            return self
        dev_table = self._tables.get(table)
        if dev_table is None:
            dev_table = self._tables[table] = torch.tensor(table, dtype=torch.int32, device=self.device)
        L.call("dc_climatology_accumulate", self.B, self.H, self.W, self.G, L.dptr(mask), _BYTES[mask.dtype], L.dptr(fields), self.C,
               max(self.ldc, 1), L.dptr(self._chan), L.dptr(self._bits), L.dptr(dev_table), L.dptr(self._frames), L.dptr(self._count),
               L.dptr(self._sum), L.dptr(self._n), L.stream_ptr())
        self.host_frames = [h + a for h, a in zip(self.host_frames, added)]
        return self

    def reset(self) -> None:
        """zeroes the accumulators (in stream order)"""
        for t in (self._frames, self._count, self._sum, self._n):
            if t is not None:
                t.zero_()
        self.host_frames = [0] * self.G

    def state(self) -> dict:
        """the four accumulators on the host: frames int64 [G], count int32 [G, 2, H, W], sum int64 / n int32 [G, 3, H, W, C]"""
        empty = (self.G, 3, self.H, self.W, 0)
        return {"frames": self._frames.cpu().numpy(), "count": self._count.cpu().numpy(),
                "sum": self._sum.cpu().numpy() if self.C else np.zeros(empty, np.int64),
                "n": self._n.cpu().numpy() if self.C else np.zeros(empty, np.int32)}

    def product_table(self, products) -> np.ndarray:
        """int32 [K, 3] of products given as ("frequency", k), ("mean", c, row) or ("share", c, k): k the class 1 or 2, c the POSITION of
        a selected channel, row 0 / 1 / 2 or a name of CLIMATOLOGY_ROWS"""
        out = []
        for prod in products:
            kind, args = prod[0], list(prod[1:])
            if kind not in CLIMATOLOGY_PRODUCTS or len(args) != (1 if kind == "frequency" else 2):
                raise L.DeepcamHipError(f"Climatology: a product is ('frequency', k), ('mean', c, row) or ('share', c, k), got {prod!r}")
            if kind == "mean" and args[1] in CLIMATOLOGY_ROWS:
                args[1] = CLIMATOLOGY_ROWS.index(args[1])
            args = [int(a) for a in args] + [0] * (2 - len(args))
            ok = args[0] in (1, 2) if kind == "frequency" else 0 <= args[0] < self.C and (0 <= args[1] < 3 if kind == "mean" else args[1] in (1, 2))
            if not ok:
                raise L.DeepcamHipError(f"Climatology: product {prod!r} names a class, channel position or row that does not exist")
            out.append([CLIMATOLOGY_PRODUCTS[kind]] + args)
        if not 1 <= len(out) <= 256:
            raise L.DeepcamHipError(f"Climatology: between 1 and 256 products, got {len(out)}")
        return np.asarray(out, np.int32)

    def fields(self, products, t1: float = 0.1, t2: float = 0.1):
        """(fp32 [G, H, W, K], uint8 [G, H, W]) on the device, from dc_climatology_maps on the current stream, not synchronised: the
        products as the channels of a FrameRenderer(batch=G, ldc=K) input, and the contour mask (1 where the class-1 frequency >= t1, else
        2 where the class-2 frequency >= t2).  Both are buffers of the object, overwritten by the next call with the same products."""
        key = tuple(tuple(p) for p in products)
        if key not in self._products:
            table = self.product_table(products)
            self._products[key] = (torch.from_numpy(table).to(self.device),
                                   torch.empty((self.G, self.H, self.W, len(table)), dtype=torch.float32, device=self.device),
                                   torch.empty((self.G, self.H, self.W), dtype=torch.uint8, device=self.device))
        table, out, contour = self._products[key]
        L.call("dc_climatology_maps", self.G, self.H, self.W, self.C, L.dptr(self._frames), L.dptr(self._count), L.dptr(self._sum),
               L.dptr(self._n), L.dptr(self._bits), len(table), L.dptr(table), float(np.float32(t1)), float(np.float32(t2)), L.dptr(out),
               L.dptr(contour), L.stream_ptr())
        return out, contour

    def maps(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["frames"], s["count"], s["sum"], s["n"], self.bits, self.H, self.W)

    @staticmethod
    def occurrence(frames, count, height: int, width: int) -> dict:
        """decode()'s frequency, zonal_frequency and area_frequency, which need the counts alone"""
        frames = np.asarray(frames, np.int64).reshape(-1)
        count = np.asarray(count, np.int64).reshape(len(frames), 2, height, width)
        fr = frames.astype(np.float64)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        rows = count.sum(axis=3)                                                # int64 [G, 2, H]
        wy = event_weight_tables(height, width)[0].astype(np.int64)
        return {"frequency": div(count.astype(np.float64), fr[:, None, None, None]),
                "zonal_frequency": div(rows.astype(np.float64), fr[:, None, None] * width),
                "area_frequency": div((rows * wy).sum(axis=2).astype(np.float64), fr[:, None] * (float(width) * float(wy.sum())))}

    @staticmethod
    def decode(frames, count, sum, n, bits, height: int, width: int) -> dict:
        """float64 maps from the raw integers, NaN where a divisor is zero: frequency [G, 2, H, W] = count / frames; mean [G, 3, H, W, C]
        = sum * 2^-bits / n; share [G, 2, H, W, C] = sum of class k / sum of all; zonal_frequency [G, 2, H], the mean frequency of a row;
        area_frequency [G, 2], the cos(lat)-weighted mean frequency with event_weight_tables' integer wy: sum_r wy[r] * (count summed
        along the row) / (frames * W * sum_r wy[r]) -- the share of the globe's area and time spent inside the class."""
        out = Climatology.occurrence(frames, count, height, width)
        G, C = len(out["area_frequency"]), len(np.asarray(bits).reshape(-1))
        total = np.asarray(sum, np.int64).reshape(G, 3, height, width, C).astype(np.float64)
        n = np.asarray(n, np.int64).reshape(G, 3, height, width, C)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        scaled = np.ldexp(total, -np.asarray(bits, np.int32).reshape(-1)) if C else total
        out.update(mean=div(scaled, n.astype(np.float64)), share=div(total[:, 1:], total[:, :1]))
        return out


# ---------------------------------------------------------------------------------------------- storm-centred composites
COMPOSITE_COUNTS = ("composited", "no_center", "below_min_pixels", "other_class", "uncatalogued")
COMPOSITE_MAX_EVENTS = 1 << 21
COMPOSITE_MAX_RADIUS = 40
COMPOSITE_KEYS = ("events", "sum", "n", "inside", "rsum", "rn")


def composite_bits(minval, maxval) -> np.ndarray:
    """int32 [C]: the binary scale of dc_composite_accumulate's sums per channel, from the dataset's recorded range.  With m =
    max(|minval|, |maxval|): 27 - frexp(m)[1], and 0 where m is zero or not finite.  A value inside the range is summed as
    rint(v * 2^bits) with |q| < 2^27; values up to twice outside the range still fit below the kernel's limit of 2^28."""
    lo = np.atleast_1d(np.asarray(minval, np.float64))
    hi = np.atleast_1d(np.asarray(maxval, np.float64))
    m = np.maximum(np.abs(lo), np.abs(hi))
    ok = np.isfinite(m) & (m > 0)
    return np.where(ok, 27 - np.frexp(np.where(ok, m, 1.0))[1], 0).astype(np.int32)


def composite_radius_table(height: int, width: int, radius: int, bin_km: float, bins: int) -> np.ndarray:
    """uint8 [H][S][R + 1], S = 2 R + 1: entry (r0, d + R, a) is the distance bin floor(distance / bin_km) between the pixel centres
    (r0, c0) and (r0 + d, c0 + a) -- the great-circle distance by the haversine formula in float64, latitudes from linspace(-90, 90, H),
    a longitude step of 360 / W (the periodic grid of event_shape_tables), Earth radius EARTH_RADIUS_KM.  255 where the bin is >= bins or
    row r0 + d is off the grid.  bins <= 255."""
    height, width, radius, bins = int(height), int(width), int(radius), int(bins)
    if height < 1 or width < 1 or not 1 <= radius <= COMPOSITE_MAX_RADIUS or not 0 <= bins <= 255 or not float(bin_km) > 0:
        raise L.DeepcamHipError(f"composite_radius_table: height and width must be positive, radius in [1, {COMPOSITE_MAX_RADIUS}], bins in "
                                f"[0, 255] and bin_km positive, got {height}, {width}, {radius}, {bins}, {bin_km}")
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    d = np.arange(-radius, radius + 1)
    rows = np.arange(height)[:, None] + d[None, :]                              # [H, S]
    on = (rows >= 0) & (rows < height)
    lat1 = lat[:, None, None]
    lat2 = lat[np.clip(rows, 0, height - 1)][:, :, None]
    dlon = np.deg2rad(360.0 / width * np.arange(radius + 1))[None, None, :]
    hav = np.sin((lat2 - lat1) / 2.0) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin(dlon / 2.0) ** 2
    dist = 2.0 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.clip(hav, 0.0, 1.0)))
    k = np.floor(dist / float(bin_km))
    return np.where(on[:, :, None] & (k < bins), np.minimum(k, 255), 255).astype(np.uint8)


class StormComposite:
    """The fields in storm coordinates, accumulated on the device (dc_composite_centers, dc_composite_accumulate, csrc/composite.hip):
    around the centre of every selected event of an EventFields catalogue -- the pixel of the minimum (or maximum) of center_channel, a
    cyclone's pressure minimum -- a window of S x S grid pixels, S = 2 radius + 1, summed cell by cell over the events of a group, with
    the events' mean footprint and the sums per great-circle distance bin (bins of bin_km; bins = 0: no radial profile).
    channels: indices into the ldc channels of a pixel (None: all of them); bits: the binary scale per SELECTED channel (composite_bits;
    None: EventFields' bits less 12, which is the same number for a channel with a recorded range); classes: the event classes that are
    composited; groups: the frame groups G (climatology_group); intensity_edges: ascending finite values that cut the centre value into
    len + 1 bins (an event on an edge goes to the bin above), so that GT = G * (len + 1) composites are kept, index group * (len + 1) + bin;
    flip_south: southern events are reflected about their centre row, so that "up" is poleward and the rotation is northern; negate:
    selected-channel POSITIONS whose sign the reflection reverses (the meridional wind components).
    The object owns events (int64 [GT]), sum (int64 [GT, S, S, C]), n (int32 [GT, S, S, C]), inside (int32 [GT, S, S]), rsum / rn (int64
    [GT, NB, C]) and counts (int64 [5], COMPOSITE_COUNTS); everything is an integer sum, so the state does not depend on how a sequence was
    cut into batches or ordered.  A call must follow the catalogue's and the EventFields call of the same batch on the same stream; it
    launches and does not synchronise; state() and composites() read back."""

    def __init__(self, fields: "EventFields", center_channel: int, center_stat: str = "min", radius: int = 32, channels=None, bits=None,
                 classes=(1,), min_pixels: int = 0, groups: int = 1, intensity_edges=(), flip_south: bool = True, negate=(),
                 bin_km: float = 25.0, bins: int = 40):
        cat = fields.catalog
        if center_stat not in ("min", "max"):
            raise L.DeepcamHipError(f"StormComposite: center_stat must be 'min' or 'max', got {center_stat!r}")
        if not 0 <= int(center_channel) < fields.C:
            raise L.DeepcamHipError(f"StormComposite: center_channel must lie in [0, {fields.C}), got {center_channel}")
        radius = int(radius)
        if not 1 <= radius <= COMPOSITE_MAX_RADIUS or 2 * radius + 1 > cat.W:
            raise L.DeepcamHipError(f"StormComposite: radius must lie in [1, {COMPOSITE_MAX_RADIUS}] and 2 * radius + 1 may not exceed the "
                                    f"width {cat.W}, got {radius}")
        channels = list(range(fields.ldc)) if channels is None else [int(c) for c in channels]
        C_ = len(channels)
        if not 1 <= C_ <= 32 or min(channels) < 0 or max(channels) >= fields.ldc:
            raise L.DeepcamHipError(f"StormComposite: between 1 and 32 channels out of [0, {fields.ldc}), got {channels}")
        if bits is None:
            if max(channels) >= fields.C:
                raise L.DeepcamHipError("StormComposite: bits are needed for channels the EventFields object does not cover")
            bits = [fields.bits[c] - 12 for c in channels]
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        if len(bits) != C_:
            raise L.DeepcamHipError(f"StormComposite: {len(bits)} scale bits for {C_} channels")
        classes = sorted({int(k) for k in classes})
        if not classes or any(k not in (1, 2) for k in classes):
            raise L.DeepcamHipError(f"StormComposite: classes must be a non-empty subset of (1, 2), got {classes}")
        if int(min_pixels) < 0:
            raise L.DeepcamHipError(f"StormComposite: min_pixels must not be negative, got {min_pixels}")
        edges = np.asarray(list(intensity_edges), np.float32).reshape(-1)
        if len(edges) > 255 or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) < 0):
            raise L.DeepcamHipError(f"StormComposite: intensity_edges must be at most 255 finite ascending values, got {list(intensity_edges)}")
        if not 1 <= int(groups) or int(groups) * (len(edges) + 1) > 65536:
            raise L.DeepcamHipError(f"StormComposite: groups must be positive and groups * (edges + 1) at most 65536, got {groups}")
        negate = sorted({int(c) for c in negate})
        if any(not 0 <= c < C_ for c in negate):
            raise L.DeepcamHipError(f"StormComposite: negate holds positions of selected channels, [0, {C_}), got {negate}")
        if not 0 <= int(bins) <= 255 or not float(bin_km) > 0:
            raise L.DeepcamHipError(f"StormComposite: bins must lie in [0, 255] and bin_km be positive, got {bins}, {bin_km}")
        self.fields, self.catalog = fields, cat
        self.center_channel, self.center_stat, self.R, self.S = int(center_channel), center_stat, radius, 2 * radius + 1
        self.channels, self.bits, self.C, self.classes, self.min_pixels = channels, bits, C_, classes, int(min_pixels)
        self.G, self.edges, self.NE = int(groups), edges, len(edges)
        self.GT = self.G * (self.NE + 1)
        self.flip_south, self.negate, self.bin_km, self.NB = bool(flip_south), negate, float(bin_km), int(bins)
        self.class_mask = sum(1 << k for k in classes)
        self.negate_mask = sum(1 << c for c in negate)
        dev = self.device = cat._labels.device
        S, GT = self.S, self.GT
        self._events = torch.zeros((GT,), dtype=torch.int64, device=dev)
        self._sum = torch.zeros((GT, S, S, C_), dtype=torch.int64, device=dev)
        self._n = torch.zeros((GT, S, S, C_), dtype=torch.int32, device=dev)
        self._inside = torch.zeros((GT, S, S), dtype=torch.int32, device=dev)
        self._rsum = torch.zeros((GT, self.NB, C_), dtype=torch.int64, device=dev)
        self._rn = torch.zeros((GT, self.NB, C_), dtype=torch.int64, device=dev)
        self._counts = torch.zeros((len(COMPOSITE_COUNTS),), dtype=torch.int64, device=dev)
        self._centers = torch.full((cat.B, cat.cap), -1, dtype=torch.int32, device=dev)
        self._egroup = torch.full((cat.B, cat.cap), -1, dtype=torch.int32, device=dev)
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev)
        self._edges = torch.from_numpy(edges).to(dev) if self.NE else None
        # the identity over all ldc channels travels as a null table: the library then knows it on the host and may take its 16-byte loads
        self._chan = None if channels == list(range(fields.ldc)) else torch.tensor(channels, dtype=torch.int32, device=dev)
        self.radius_table = composite_radius_table(cat.H, cat.W, radius, bin_km, bins) if self.NB else None
        self._rbin = torch.from_numpy(self.radius_table).to(dev) if self.NB else None
        self._tables = {}                            # group tuple -> device int32 [B]
        self._last_valid = 0

    def __call__(self, raw_fields: torch.Tensor, groups=None, n_valid: Optional[int] = None) -> "StormComposite":
        """raw_fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw) -- the tensor the EventFields call of this
        batch was given; groups: None (every frame to group 0), an int, or B ints, a negative one skipping its frame; n_valid defaults to
        the EventFields call's, frames from it on are skipped."""
        cat, ef = self.catalog, self.fields
        check_tensor("StormComposite", "fields", raw_fields, (torch.float32,), (cat.B, cat.H, cat.W, ef.ldc), self.device, "fp32")
        nv = _n_valid("StormComposite", ef._last_valid if n_valid is None else n_valid, cat.B)
        table = group_table("StormComposite", groups, cat.B, nv, self.G)
        self._last_valid = nv
        if nv == 0 or all(g < 0 for g in table):
            return self
        dev_table = self._tables.get(table)
        if dev_table is None:
            dev_table = self._tables[table] = torch.tensor(table, dtype=torch.int32, device=self.device)
        st = L.stream_ptr()
        L.call("dc_composite_centers", cat.B, nv, cat.H, cat.W, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(ef._ftable), ef.C,
               self.center_channel, 0 if self.center_stat == "min" else 1, self.class_mask, self.min_pixels, L.dptr(dev_table), self.G,
               L.dptr(self._edges), self.NE, L.dptr(self._centers), L.dptr(self._egroup), L.dptr(self._counts), st)
        L.call("dc_composite_accumulate", cat.B, nv, cat.H, cat.W, cat.cap, self.R, self.GT, L.dptr(self._centers), L.dptr(self._egroup),
               L.dptr(cat._table), L.dptr(cat._labels), L.dptr(raw_fields), self.C, ef.ldc, L.dptr(self._chan), L.dptr(self._bits),
               _c_int(self.negate_mask), int(self.flip_south), L.dptr(self._rbin), self.NB, L.dptr(self._events), L.dptr(self._sum),
               L.dptr(self._n), L.dptr(self._inside), L.dptr(self._rsum) if self.NB else None, L.dptr(self._rn) if self.NB else None, st)
        return self

    @property
    def centers(self) -> torch.Tensor:
        """int32 [n_valid, cap] of the last call (a view): the centre pixel r0 * W + c0 of every composited event, -1 elsewhere"""
        return self._centers[:self._last_valid]

    @property
    def event_groups(self) -> torch.Tensor:
        """int32 [n_valid, cap] of the last call (a view): group * (edges + 1) + intensity bin of every composited event, -1 elsewhere"""
        return self._egroup[:self._last_valid]

    def reset(self) -> None:
        """zeroes the accumulators and the counts (in stream order)"""
        for t in (self._events, self._sum, self._n, self._inside, self._rsum, self._rn, self._counts):
            t.zero_()

    def state(self) -> dict:
        """the raw integers on the host (COMPOSITE_KEYS) and counts (a dict over COMPOSITE_COUNTS).  Raises when a group has reached
        COMPOSITE_MAX_EVENTS events: from there on the sums are no longer known to fit their words."""
        out = {"events": self._events.cpu().numpy(), "sum": self._sum.cpu().numpy(), "n": self._n.cpu().numpy(),
               "inside": self._inside.cpu().numpy(), "rsum": self._rsum.cpu().numpy(), "rn": self._rn.cpu().numpy()}
        if int(out["events"].max()) >= COMPOSITE_MAX_EVENTS:
            raise L.DeepcamHipError(f"StormComposite: a group has reached {COMPOSITE_MAX_EVENTS} events, the bound of the integer sums")
        out["counts"] = dict(zip(COMPOSITE_COUNTS, (int(v) for v in self._counts.cpu().tolist())))
        return out

    def composites(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(*(s[k] for k in COMPOSITE_KEYS), self.bits, self.bin_km)

    @staticmethod
    def decode(events, sum, n, inside, rsum, rn, bits, bin_km: float = 25.0) -> dict:
        """float64 from the raw integers: mean [GT, S, S, C] = sum * 2^-bits / n, NaN where n == 0; footprint [GT, S, S] = inside /
        events, NaN where events == 0; radial_mean [GT, NB, C] = rsum * 2^-bits / rn, NaN where rn == 0; radius_km [NB], the bin
        centres (k + 1/2) * bin_km; radius_of_max_km [GT, C], the centre of the bin with the largest finite radial mean -- the smallest
        such bin on ties --, NaN where no bin has a value."""
        bits = np.asarray(bits, np.int32).reshape(-1)
        events = np.asarray(events, np.int64).reshape(-1)
        total, n = np.asarray(sum, np.int64).astype(np.float64), np.asarray(n, np.int64).astype(np.float64)
        rsum, rn = np.asarray(rsum, np.int64).astype(np.float64), np.asarray(rn, np.int64).astype(np.float64)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        radial = div(np.ldexp(rsum, -bits), rn)
        radius = (np.arange(radial.shape[1]) + 0.5) * float(bin_km)
        rmax = np.full((radial.shape[0], radial.shape[2]), np.nan)
        if radial.shape[1]:
            some = np.isfinite(radial).any(axis=1)
            first = np.argmax(np.where(np.isfinite(radial), radial, -np.inf), axis=1)    # argmax takes the first among equals
            rmax = np.where(some, radius[first], np.nan)
        return {"mean": div(np.ldexp(total, -bits), n), "footprint": div(np.asarray(inside, np.int64).astype(np.float64), events[:, None, None].astype(np.float64)),
                "radial_mean": radial, "radius_km": radius, "radius_of_max_km": rmax}
