"""The events of class masks, on the device: the catalogue of connected components (EventCatalog), two catalogues matched (EventMatcher),
per-event statistics of the input fields (EventFields), shapes and a shape filter (EventShape, EventFilter), events linked across time
steps (EventTracker), the tracks' life cycles (TrackFields) and two sides' tracks matched (TrackMatcher)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from ._args import _ratio, check_range, check_tensor, device_of

EVENT_FIELDS = ("root", "class", "pixels", "area", "sum_row", "sum_cx", "sum_sx", "row_min", "row_max", "seam")
EVENT_SCALE = 1 << 20


def event_weight_tables(height: int, width: int):
    """(wy [H], cx [W], sx [W]) int32 numpy arrays: cos(lat_r), cos(lon_c), sin(lon_c) times 2^20, rounded to nearest (ties to even), with
    lat = linspace(-90, 90, H) and lon = linspace(-180, 180, W) degrees, evaluated in float64.  Integer weights make every sum of the
    catalogue exact and independent of the order in which pixels arrive."""
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    lon = np.deg2rad(np.linspace(-180.0, 180.0, width))
    q = lambda v: np.rint(v * EVENT_SCALE).astype(np.int32)  # noqa: E731
    return q(np.cos(lat)), q(np.cos(lon)), q(np.sin(lon))


def _filled_rows(table: torch.Tensor, fill):
    """Per valid sample only the filled rows of a device table [B, cap, ...]: a list of numpy arrays table[b, :fill[b]], b < len(fill) (at
    least one sample).  One copy to the host, cut at the fullest sample's rows."""
    host = table[:len(fill), :max(max(fill), 1)].cpu().numpy()
    return [host[b, :fill[b]].copy() for b in range(len(fill))]


class EventCatalog:
    """Connected components of class masks on the device (dc_mask_components + dc_component_stats, csrc/components.hip): what a user of a
    tropical-cyclone / atmospheric-river detector works with -- how many events a snapshot holds, where they are and how large.
    Classes 1 and 2 are foreground; a component is a maximal set of pixels of one class under 4- or 8-connectivity, with periodic columns
    when wrap is set (the fields are global longitude bands).  The object owns the label map (int32, 0 = background, else 1 + the smallest
    r * W + c of the component), the workspace, the weight tables, the table (int64 [B, cap, 10], EVENT_FIELDS) and the counts (int32
    [B, 3]: all, class 1, class 2 -- not capped).  A call launches on the current stream and does not synchronise; events() reads back."""

    def __init__(self, batch: int, height: int, width: int, connectivity: int = 8, wrap: bool = True, cap: int = 4096, device=None):
        if connectivity not in (4, 8):
            raise L.DeepcamHipError(f"EventCatalog: connectivity must be 4 or 8, got {connectivity}")
        if batch < 1 or height < 1 or width < 1 or cap < 1:
            raise L.DeepcamHipError("EventCatalog: batch, height, width and cap must be positive")
        self.B, self.H, self.W, self.connectivity, self.wrap, self.cap = batch, height, width, connectivity, bool(wrap), cap
        dev = device_of(device)
        self.tables = event_weight_tables(height, width)
        self._wy, self._cx, self._sx = (torch.from_numpy(t).to(dev) for t in self.tables)
        self._labels = torch.zeros((batch, height, width), dtype=torch.int32, device=dev)
        self._table = torch.zeros((batch, cap, len(EVENT_FIELDS)), dtype=torch.int64, device=dev)
        self._ncomp = torch.zeros((batch, 3), dtype=torch.int32, device=dev)
        self._ws = torch.empty(max(L.load().dc_mask_components_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> "EventCatalog":
        """mask: device uint8 [B, H, W].  Samples from n_valid on are padding: not read, their labels and counts stay as they were."""
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (self.B, self.H, self.W) or not mask.is_cuda or not mask.is_contiguous():
            raise L.DeepcamHipError(f"EventCatalog: mask must be a contiguous device uint8 tensor [{self.B}, {self.H}, {self.W}], got "
                                    f"{mask.dtype} {tuple(mask.shape)} on {mask.device}")
        nv = self.B if n_valid is None else int(n_valid)
        st = L.stream_ptr()
        L.call("dc_mask_components", self.B, nv, self.H, self.W, L.dptr(mask), self.connectivity, int(self.wrap), L.dptr(self._labels),
               L.dptr(self._ws), st)
        L.call("dc_component_stats", self.B, nv, self.H, self.W, L.dptr(mask), L.dptr(self._labels), L.dptr(self._wy), L.dptr(self._cx),
               L.dptr(self._sx), self.cap, L.dptr(self._table), L.dptr(self._ncomp), L.dptr(self._ws), st)
        self._last_valid = nv
        return self

    @property
    def labels(self) -> torch.Tensor:
        """int32 [n_valid, H, W] of the last call (a view)"""
        return self._labels[:self._last_valid]

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, 10] of the last call (a view): the raw rows, zero beyond min(count, cap)"""
        return self._table[:self._last_valid]

    def counts(self) -> torch.Tensor:
        """int32 [n_valid, 3] of the last call (a view): components of any class, of class 1, of class 2"""
        return self._ncomp[:self._last_valid]

    @property
    def rank_map(self) -> torch.Tensor:
        """int32 [n_valid, H, W] of the last call (a view of the workspace's first segment, valid until the next call): at every root pixel
        (labels == r * W + c + 1) the row index of that component, undefined elsewhere.  What dc_component_overlap reads."""
        n = self.B * self.H * self.W
        return self._ws[:4 * n].view(torch.int32).view(self.B, self.H, self.W)[:self._last_valid]

    def rows(self):
        """(counts, rows) on the host: the counts first, then only the rows that are filled -- one list entry per valid sample, each an
        int64 numpy array [min(total, cap), 10]."""
        nv = self._last_valid
        if nv == 0:
            return [], []
        ncomp = self._ncomp[:nv].cpu().numpy()
        return ncomp, _filled_rows(self._table, [min(int(t), self.cap) for t in ncomp[:, 0]])

    def _fill(self, nv: int):
        """The rows the table holds for each of the first nv samples: min(total, cap) (EventFields and EventShape cut their tables by it)"""
        return [min(int(t), self.cap) for t in self._ncomp[:nv, 0].cpu().tolist()]

    def events(self, min_pixels: int = 0):
        """Per valid sample of the last call a list of dicts (decode), components below min_pixels left out on the host."""
        _, rows = self.rows()
        return [self.decode(r, self.H, self.W, min_pixels=min_pixels) for r in rows]

    @staticmethod
    def decode(rows, height: int, width: int, min_pixels: int = 0):
        """Raw rows [n, 10] (EVENT_FIELDS) -> dicts: class, pixels, area_fraction (area / sum_r W * wy[r]: the share of the sphere), lat (the
        mean row through linspace(-90, 90, H)), lon (atan2(sum sx, sum cx) in degrees: the circular mean, right across the seam), row_min,
        row_max, crosses_seam, root."""
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        out = []
        for r in rows:
            root, cls, n, area, sr, scx, ssx, rmin, rmax, seam = (int(v) for v in r)
            if n < max(min_pixels, 1):
                continue
            lat = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 else -90.0
            out.append({"class": cls, "pixels": n, "area_fraction": area / whole if whole > 0 else 0.0, "lat": lat,
                        "lon": math.degrees(math.atan2(ssx, scx)), "row_min": rmin, "row_max": rmax, "crosses_seam": bool(seam), "root": root})
        return out


class EventMatcher:
    """Two event catalogues of the same frames matched on the device (dc_component_overlap + dc_event_scores, csrc/event_match.hip): which
    event of mask a overlaps which event of mask b and by how many pixels, how much of every event the other mask covers with the same
    class, and from that the detection scores per class -- hits and misses among b's events, false alarms and matched detections among
    a's.  With a = a prediction and b = its labels these are the counts behind POD, FAR and CSI; the same pairs link the events of two
    time steps.  An event is SCORED when it has at least max(min_pixels, 1) pixels and a row in its table; it is MATCHED when the other
    mask covers at least min_cover of it with its class (integer: cover * 1024 >= round(min_cover * 1024) * pixels, and cover >= 1).
    Coverage, not pairwise IoU, decides: a labelled river predicted as two fragments is still found.  The object owns the two catalogues
    `.a` and `.b`, the pair table (int64 [B, pair_cap, 3]), the coverage counts (int64 [B, cap] per side), the per-sample scores (int64
    [B, 2, 4]) and the running sums.  A call launches on the current stream and does not synchronise."""

    SCORE_FIELDS = ("hits", "misses", "false_alarms", "matched")

    def __init__(self, batch: int, height: int, width: int, connectivity: int = 8, wrap: bool = True, cap: int = 4096, pair_cap: int = 8192,
                 min_pixels: int = 0, min_cover: float = 0.5, device=None):
        if not 0.0 < float(min_cover) <= 1.0:
            raise L.DeepcamHipError(f"EventMatcher: min_cover must lie in (0, 1], got {min_cover}")
        if pair_cap < 1 or min_pixels < 0:
            raise L.DeepcamHipError("EventMatcher: pair_cap must be positive and min_pixels not negative")
        dev = device_of(device)
        self.a = EventCatalog(batch, height, width, connectivity=connectivity, wrap=wrap, cap=cap, device=dev)
        self.b = EventCatalog(batch, height, width, connectivity=connectivity, wrap=wrap, cap=cap, device=dev)
        self.B, self.H, self.W, self.cap, self.pair_cap, self.min_pixels = batch, height, width, cap, pair_cap, int(min_pixels)
        self.cover_q = min(max(int(round(float(min_cover) * 1024)), 1), 1024)
        self._pairs = torch.zeros((batch, pair_cap, 3), dtype=torch.int64, device=dev)
        self._npairs = torch.zeros((batch, 2), dtype=torch.int32, device=dev)
        self._cover_a = torch.zeros((batch, cap), dtype=torch.int64, device=dev)
        self._cover_b = torch.zeros((batch, cap), dtype=torch.int64, device=dev)
        self._scores = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
        self.acc = torch.zeros(10, dtype=torch.int64, device=dev)
        nbytes = L.load().dc_component_overlap_workspace(batch, pair_cap)
        if nbytes == 0:
            raise L.DeepcamHipError(f"EventMatcher: pair_cap {pair_cap} is out of range")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._mask_b = None
        self._last_valid = 0

    def __call__(self, mask_a: torch.Tensor, mask_b: torch.Tensor, n_valid: Optional[int] = None) -> "EventMatcher":
        """mask_a: device uint8 [B, H, W]; mask_b: the same, or a label tensor (int64, int32) whose classes become bytes here.  Samples from
        n_valid on are padding: not read."""
        if mask_b.dtype in (torch.int64, torch.int32):
            mask_b = mask_b.to(torch.uint8)
        nv = self.B if n_valid is None else int(n_valid)
        a, b, st = self.a, self.b, L.stream_ptr()
        a(mask_a, n_valid=nv)
        b(mask_b, n_valid=nv)
        self._mask_b = mask_b                      # the converted bytes stay alive while the launches below may still read them
        L.call("dc_component_overlap", self.B, nv, self.H, self.W, L.dptr(mask_a), L.dptr(a._labels), L.dptr(a._ws), a.cap, L.dptr(mask_b),
               L.dptr(b._labels), L.dptr(b._ws), b.cap, self.pair_cap, L.dptr(self._pairs), L.dptr(self._npairs), L.dptr(self._cover_a),
               L.dptr(self._cover_b), L.dptr(self._ws), st)
        L.call("dc_event_scores", self.B, nv, a.cap, L.dptr(a._table), L.dptr(a._ncomp), L.dptr(self._cover_a), b.cap, L.dptr(b._table),
               L.dptr(b._ncomp), L.dptr(self._cover_b), L.dptr(self._npairs), self.min_pixels, self.cover_q, L.dptr(self._scores),
               L.dptr(self.acc), st)
        self._last_valid = nv
        return self

    @property
    def mask_b(self) -> Optional[torch.Tensor]:
        """uint8 [B, H, W]: side b's mask of the last call as the catalogue took it -- the converted bytes of a label tensor (read-only;
        what an EventTracker on `.b` is called with).  None before the first call."""
        return self._mask_b

    @property
    def pair_table(self) -> torch.Tensor:
        """int64 [n_valid, pair_cap, 3] of the last call (a view): (rank a, rank b, pixels), device order, zero beyond the stored count"""
        return self._pairs[:self._last_valid]

    @property
    def pair_counts(self) -> torch.Tensor:
        """int32 [n_valid, 2] of the last call (a view): rows stored, overflow flag"""
        return self._npairs[:self._last_valid]

    @property
    def score_table(self) -> torch.Tensor:
        """int64 [n_valid, 2, 4] of the last call (a view): per class 1, 2 the SCORE_FIELDS"""
        return self._scores[:self._last_valid]

    @staticmethod
    def sort_pairs(rows: np.ndarray) -> np.ndarray:
        """the stored rows [n, 3] ordered by (rank a, rank b)"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        return np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0]))])

    def pairs(self):
        """(rows, flags) on the host: per valid sample an int64 numpy array [n, 3] sorted by (rank a, rank b), and the overflow flags"""
        nv = self._last_valid
        if nv == 0:
            return [], []
        npairs = self._npairs[:nv].cpu().numpy()
        return [self.sort_pairs(p) for p in _filled_rows(self._pairs, [int(n) for n in npairs[:, 0]])], [int(f) for f in npairs[:, 1]]

    def cover(self):
        """(cover_a, cover_b) on the host: int64 numpy arrays [n_valid, cap], per component the pixels the other mask covers with its class"""
        nv = self._last_valid
        return self._cover_a[:nv].cpu().numpy(), self._cover_b[:nv].cpu().numpy()

    def scores(self) -> np.ndarray:
        """int64 numpy array [n_valid, 2, 4]: per sample and class the SCORE_FIELDS"""
        return self._scores[:self._last_valid].cpu().numpy()

    @staticmethod
    def join(pairs, rows_a, rows_b, height: int, width: int, min_pixels: int = 0):
        """Sorted pairs [n, 3] and the two catalogues' raw rows -> a list of dicts: `a`, `b` (EventCatalog.decode of the two rows),
        `class_a`, `class_b`, `pixels` (shared), `iou` (shared / union).  Pairs with an event below min_pixels are left out."""
        out = []
        for ra, rb, n in np.asarray(pairs, dtype=np.int64).reshape(-1, 3).tolist():
            if min(int(rows_a[ra][2]), int(rows_b[rb][2])) < max(min_pixels, 1):
                continue
            ea = EventCatalog.decode(rows_a[ra:ra + 1], height, width)[0]
            eb = EventCatalog.decode(rows_b[rb:rb + 1], height, width)[0]
            out.append({"a": ea, "b": eb, "class_a": ea["class"], "class_b": eb["class"], "pixels": n,
                        "iou": n / (ea["pixels"] + eb["pixels"] - n)})
        return out

    def matches(self, min_pixels: Optional[int] = None):
        """Per valid sample of the last call the joined pairs (join); min_pixels defaults to the matcher's."""
        mp = self.min_pixels if min_pixels is None else int(min_pixels)
        pairs, _ = self.pairs()
        _, rows_a = self.a.rows()
        _, rows_b = self.b.rows()
        return [self.join(p, ra, rb, self.H, self.W, mp) for p, ra, rb in zip(pairs, rows_a, rows_b)]

    def reset(self) -> None:
        L.call("dc_memset_async", L.dptr(self.acc), 0, 80, L.stream_ptr())

    @staticmethod
    def rates(hits: int, misses: int, false_alarms: int, matched: int) -> dict:
        """pod = hits / (hits + misses): the share of b's events found; far = false_alarms / (false_alarms + matched): the share of a's
        events that answer to nothing; csi = hits / (hits + misses + false_alarms).  None where the denominator is zero."""
        div = lambda n, d: n / d if d > 0 else None  # noqa: E731
        return {"pod": div(hits, hits + misses), "far": div(false_alarms, false_alarms + matched),
                "csi": div(hits, hits + misses + false_alarms)}

    @staticmethod
    def summarize(acc) -> dict:
        """the ten running sums -> {"samples", "truncated", "class_1": {...}, "class_2": {...}}: per class the SCORE_FIELDS and rates();
        truncated: some sample held more events than a table or more pairs than the pair table, so counts may be short"""
        acc = [int(v) for v in acc]
        out = {"samples": acc[8], "truncated": acc[9] != 0}
        for k in (0, 1):
            h, m, f, d = acc[4 * k:4 * k + 4]
            out[f"class_{k + 1}"] = {"hits": h, "misses": m, "false_alarms": f, "matched": d, **EventMatcher.rates(h, m, f, d),
                                     "truncated": acc[9] != 0}
        return out

    def result(self) -> dict:
        """summarize() of the sums since reset(): one device-to-host read"""
        return self.summarize(self.acc.cpu().tolist())


EVENT_FIELD_STATS = ("min", "max", "sum", "wsum", "nonfinite", "saturated")


def event_field_bits(minval, maxval) -> np.ndarray:
    """int32 [C]: the binary scale of dc_component_fields' sums per channel, from the dataset's recorded range (stats.h5: climate/minval,
    climate/maxval).  With m = max(|minval|, |maxval|): 39 - frexp(m)[1], and 0 where m is zero or not finite.  A value v inside the range
    is summed as rint(v * 2^bits) with |v * 2^bits| < 2^39; values up to twice outside the range still fit below the kernel's limit of
    2^40, larger ones are counted as saturated.  The quantum of the sums is 2^-bits: a sum of n values is within n * 2^-(bits + 1) of the
    real one (m = 1e5: bits 22, 1.2e-7 per value)."""
    lo = np.atleast_1d(np.asarray(minval, np.float64))
    hi = np.atleast_1d(np.asarray(maxval, np.float64))
    m = np.maximum(np.abs(lo), np.abs(hi))
    ok = np.isfinite(m) & (m > 0)
    return np.where(ok, 39 - np.frexp(np.where(ok, m, 1.0))[1], 0).astype(np.int32)


def event_field_key(values) -> np.ndarray:
    """uint32 keys of float32 values whose unsigned order is the values' order (-0.0 below +0.0, denormals in their places): the bits with
    the sign bit set for non-negative values, all bits flipped for negative ones.  The upper half of the min / max words."""
    u = np.asarray(values, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000)).astype(np.uint32)


def event_field_value(keys) -> np.ndarray:
    """float32 values of event_field_key's keys"""
    k = np.asarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


class EventFields:
    """Per-event statistics of the raw input fields on the device (dc_component_fields, csrc/event_fields.hip): for every event of a
    catalogue and every channel the minimum and where it sits (a cyclone's pressure minimum is its centre), the maximum and where it sits
    (its strongest wind), the sum and the area-weighted sum (a river's mean water vapour).  The object owns the device scale_bits (int32
    [C], see event_field_bits) and the table (int64 [B, cap, C, 6], EVENT_FIELD_STATS; row k belongs to row k of the catalogue's table).
    Everything is exact and independent of the order in which pixels arrive.  A call must follow the catalogue's call on the same stream
    (it reads the catalogue's labels and rank map); it launches and does not synchronise."""

    def __init__(self, catalog: EventCatalog, channels: int, bits: Sequence[int], ldc: Optional[int] = None):
        ldc = int(channels if ldc is None else ldc)
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        if not 1 <= int(channels) <= 32 or ldc < channels:
            raise L.DeepcamHipError(f"EventFields: channels must lie in [1, 32] and ldc must be at least channels, got {channels}, {ldc}")
        if len(bits) != channels:
            raise L.DeepcamHipError(f"EventFields: {len(bits)} scale bits for {channels} channels")
        if catalog.H * catalog.W > 1 << 22:
            raise L.DeepcamHipError("EventFields: H * W must be at most 2^22")
        self.catalog, self.C, self.ldc, self.bits = catalog, int(channels), ldc, bits
        dev = catalog._labels.device
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev)
        self._ftable = torch.zeros((catalog.B, catalog.cap, self.C, len(EVENT_FIELD_STATS)), dtype=torch.int64, device=dev)
        self._last_valid = 0

    def __call__(self, fields: torch.Tensor, n_valid: Optional[int] = None) -> "EventFields":
        """fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw).  n_valid defaults to the catalogue's."""
        cat = self.catalog
        check_tensor("EventFields", "fields", fields, (torch.float32,), (cat.B, cat.H, cat.W, self.ldc), cat._labels.device, "fp32")
        nv = cat._last_valid if n_valid is None else int(n_valid)
        L.call("dc_component_fields", cat.B, nv, cat.H, cat.W, L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(fields), self.C, self.ldc,
               L.dptr(self._bits), L.dptr(cat._wy), L.dptr(self._ftable), L.stream_ptr())
        self._last_valid = nv
        return self

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, C, 6] of the last call (a view): rows from min(count, cap) on are empty (-1, 0, 0, 0, 0, 0)"""
        return self._ftable[:self._last_valid]

    def rows(self):
        """On the host, per valid sample only the filled rows: int64 numpy arrays [min(total, cap), C, 6] (the catalogue's counts decide)"""
        nv = self._last_valid
        if nv == 0:
            return []
        return _filled_rows(self._ftable, self.catalog._fill(nv))

    def stats(self, min_pixels: int = 0):
        """Per valid sample a list aligned with catalog.events(min_pixels): per event a list over channels of dicts (decode)."""
        _, rows = self.catalog.rows()
        out = []
        for fr, r in zip(self.rows(), rows):
            keep = r[:, 2] >= max(min_pixels, 1)
            out.append(self.decode(fr[keep], r[keep], self.catalog.H, self.catalog.W, self.bits))
        return out

    FIELD_VALUES = ("min", "min_lat", "min_lon", "max", "max_lat", "max_lon", "mean", "area_mean")

    @staticmethod
    def values(frows, rows, height: int, width: int, bits) -> np.ndarray:
        """float64 [n, C, 8] (FIELD_VALUES): decode's numbers for whole arrays at once, NaN where decode gives None -- the same
        operations on the same operands, so the two agree to the bit (what predict.py stores as event_field_values)."""
        bits = np.asarray(bits, np.int64).reshape(-1)
        fr = np.asarray(frows, np.int64).reshape(-1, len(bits), len(EVENT_FIELD_STATS))
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        out = np.full(fr.shape[:2] + (8,), np.nan, np.float64)
        lo, hi = fr[..., 0].view(np.uint64), fr[..., 1].view(np.uint64)
        for k, (word, some) in enumerate(((lo, fr[..., 0] != -1), (hi, fr[..., 1] != 0))):
            p = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
            p = np.where(some, p if k == 0 else 0xFFFFFFFF - p, 0)
            val = event_field_value((word >> np.uint64(32)).astype(np.uint32)).astype(np.float64)
            out[..., 3 * k] = np.where(some, val, np.nan)
            out[..., 3 * k + 1] = np.where(some, lat[np.minimum(p // width, height - 1)], np.nan)
            out[..., 3 * k + 2] = np.where(some, lon[p % width], np.nan)
        n = rows[:, 2, None] - fr[..., 4] - fr[..., 5]
        area = rows[:, 3, None].astype(np.float64) * 2.0 ** -20
        with np.errstate(divide="ignore", invalid="ignore"):
            out[..., 6] = np.where(n > 0, np.ldexp(fr[..., 2].astype(np.float64), -bits) / n, np.nan)
            out[..., 7] = np.where(area > 0, fr[..., 3].astype(np.float64) / (np.ldexp(1.0, bits) * area), np.nan)
        return out

    @staticmethod
    def decode(frows, rows, height: int, width: int, bits):
        """Raw rows [n, C, 6] (EVENT_FIELD_STATS) and the events' own rows [n, 10] (EVENT_FIELDS) -> per event a list over channels of
        dicts: min, min_row, min_col, min_lat, min_lon, max, max_row, max_col, max_lat, max_lon (lat / lon through the linspaces of
        event_weight_tables), mean = sum * 2^-bits / (pixels - nonfinite - saturated), area_mean = wsum / (2^bits * area * 2^-20),
        nonfinite, saturated.  None where the row is empty (no finite value) or a divisor is zero."""
        frows = np.asarray(frows, np.int64)
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        out = []
        for fr, r in zip(frows.tolist(), np.asarray(rows, np.int64).tolist()):
            pixels, area = r[2], r[3]
            per = []
            for ch, (lo, hi, s, ws, nonfinite, saturated) in enumerate(fr):
                d = {"nonfinite": nonfinite, "saturated": saturated}
                for name, word, empty in (("min", lo, -1), ("max", hi, 0)):
                    if word == empty:
                        d.update({name: None, name + "_row": None, name + "_col": None, name + "_lat": None, name + "_lon": None})
                        continue
                    word &= 0xFFFFFFFFFFFFFFFF
                    p = word & 0xFFFFFFFF if name == "min" else 0xFFFFFFFF - (word & 0xFFFFFFFF)
                    d.update({name: float(event_field_value(np.uint32(word >> 32))), name + "_row": p // width, name + "_col": p % width,
                              name + "_lat": float(lat[p // width]), name + "_lon": float(lon[p % width])})
                n = pixels - nonfinite - saturated
                d["mean"] = math.ldexp(float(s), -int(bits[ch])) / n if n > 0 else None
                d["area_mean"] = float(ws) / (math.ldexp(1.0, int(bits[ch])) * (area * 2.0 ** -20)) if area > 0 else None
                per.append(d)
            out.append(per)
        return out


EVENT_SHAPE_FIELDS = ("boundary_pixels", "faces_v", "faces_h", "s_x", "s_y", "s_z", "s_xx", "s_xy", "s_yy", "s_xz", "s_yz", "s_zz")
EVENT_SHAPE_VALUES = ("lat", "lon", "length_km", "width_km", "aspect", "orientation_deg", "perimeter_km", "area_km2", "compactness",
                      "boundary_pixels")
EVENT_FILTER_COUNTS = ("events_kept", "events_dropped", "pixels_kept", "pixels_dropped")
EARTH_RADIUS_KM = 6371.0


def event_shape_tables(height: int, width: int):
    """(rows int32 [6, H]: wy, rc2, rcs, rc3, rc2s, rcs2; cols int32 [5, W]: cx, sx, cxx, cxy, cyy) -- the tables of dc_component_shape.
    With cl / sl the cosine / sine of a row's latitude and co / so of a column's longitude: cl, cl^2, cl sl, cl^3, cl^2 sl, cl sl^2 and
    co, so, co^2, co so, so^2, each evaluated in float64, scaled by 2^20 and rounded to nearest (ties to even).  The latitudes are those
    of event_weight_tables (rows[0] is its wy).  The longitudes are the W columns of a PERIODIC grid, lon_c = -180 + 360 c / W: column
    W - 1 is one step west of column 0, as `wrap` has it, so a shape rolled across the seam keeps its moments.  event_weight_tables'
    linspace(-180, 180, W) holds the seam meridian twice (columns 0 and W - 1) and is left as it is for the catalogue."""
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    lon = np.deg2rad(-180.0 + 360.0 * np.arange(width) / width)
    cl, sl, co, so = np.cos(lat), np.sin(lat), np.cos(lon), np.sin(lon)
    q = lambda v: np.rint(v * EVENT_SCALE).astype(np.int32)  # noqa: E731
    rows = np.stack([q(cl), q(cl * cl), q(cl * sl), q(cl * cl * cl), q(cl * cl * sl), q(cl * sl * sl)])
    cols = np.stack([q(co), q(so), q(co * co), q(co * so), q(so * so)])
    return np.ascontiguousarray(rows), np.ascontiguousarray(cols)


class EventShape:
    """Geometry per event on the device (dc_component_shape, csrc/event_shape.hip): boundary pixels, perimeter faces, and the first and
    second moments of the event's pixels as area-weighted unit vectors on the sphere, all exact integer sums (EVENT_SHAPE_FIELDS; the
    header has the definition).  decode turns them into a spherical centroid, the length and width of the uniform strip with the same
    second moments, aspect, orientation, perimeter and compactness.  Built on an existing EventCatalog, as EventFields is; a call must
    follow the catalogue's call on the same stream, launches and does not synchronise.  The object owns the tables and the shape rows
    (int64 [B, cap, 12]: 96 bytes per event slot; row k belongs to row k of the catalogue's table)."""

    def __init__(self, catalog: EventCatalog):
        if catalog.H * catalog.W > 1 << 22:
            raise L.DeepcamHipError("EventShape: H * W must be at most 2^22")
        self.catalog = catalog
        dev = catalog._labels.device
        self.tables = event_shape_tables(catalog.H, catalog.W)
        self._rowt, self._colt = (torch.from_numpy(t).to(dev) for t in self.tables)
        self._shape = torch.zeros((catalog.B, catalog.cap, len(EVENT_SHAPE_FIELDS)), dtype=torch.int64, device=dev)
        self._last_valid = 0

    def __call__(self, n_valid: Optional[int] = None) -> "EventShape":
        """n_valid defaults to the catalogue's."""
        cat = self.catalog
        nv = cat._last_valid if n_valid is None else int(n_valid)
        L.call("dc_component_shape", cat.B, nv, cat.H, cat.W, L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, int(cat.wrap), L.dptr(self._rowt),
               L.dptr(self._colt), L.dptr(self._shape), L.stream_ptr())
        self._last_valid = nv
        return self

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, 12] of the last call (a view): zero from min(count, cap) on"""
        return self._shape[:self._last_valid]

    def rows(self):
        """On the host, per valid sample only the filled rows: int64 numpy arrays [min(total, cap), 12] (the catalogue's counts decide)"""
        nv = self._last_valid
        if nv == 0:
            return []
        return _filled_rows(self._shape, self.catalog._fill(nv))

    def shapes(self):
        """Per valid sample of the last call a list of dicts (decode), one per row of the catalogue."""
        _, rows = self.catalog.rows()
        return [self.decode(s, r, self.catalog.H, self.catalog.W) for s, r in zip(self.rows(), rows)]

    @staticmethod
    def steps(height: int, width: int):
        """(dlat, dlon) in radians: the spacing of the rows and columns of event_shape_tables (rows pole to pole, columns periodic)"""
        return math.pi / max(height - 1, 1), 2.0 * math.pi / width

    ARC_MAX = 4.4934                               # radians: 1 - sin(t) / t grows up to here (tan t = t), well beyond half the globe

    @staticmethod
    def chord_moment(theta):
        """12 lambda+ of a uniform great-circle arc of angle theta (radians, numpy): 6 (1 - sin(theta) / theta) -- points on the unit
        sphere, second moment along the chord.  theta^2 (1 - theta^2 / 20 + ...) for short arcs (the series below 0.3, where the closed
        form cancels)."""
        t = np.asarray(theta, np.float64)
        t2 = t * t
        series = t2 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            closed = 6.0 * (1.0 - np.sin(t) / t)
        return np.where(t < 0.3, series, closed)

    @staticmethod
    def arc_angle(q):
        """the inverse of chord_moment on [0, ARC_MAX], by bisection (numpy): the angle of the great-circle arc whose 12 lambda+ is q"""
        q = np.asarray(q, np.float64)
        lo, hi = np.zeros_like(q), np.full_like(q, EventShape.ARC_MAX)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            below = EventShape.chord_moment(mid) < q
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return 0.5 * (lo + hi)

    @staticmethod
    def moments(shape_rows, rows):
        """float64 numpy on the integers: (s0 [n], m [n, 3], C [n, 3, 3], lat [n], lon [n] in radians, lam_plus [n], lam_minus [n],
        theta [n]: the major axis' angle counter-clockwise from east, in radians) -- the header's decode formula.  Events whose zeroth
        moment is 0 (pixels on the pole rows only) give NaN moments and zero eigenvalues."""
        s = np.asarray(shape_rows, np.int64).reshape(-1, len(EVENT_SHAPE_FIELDS)).astype(np.float64)
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        s0 = rows[:, 3].astype(np.float64) * float(EVENT_SCALE)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = s[:, 3:6] / s0[:, None]
            second = np.empty((len(s), 3, 3), np.float64)
            for (i, j), f in zip(((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)), range(6, 12)):
                second[:, i, j] = second[:, j, i] = s[:, f] / s0
            cov = second - m[:, :, None] * m[:, None, :]
            norm = np.sqrt((m * m).sum(axis=1))
            c = np.where((norm > 0)[:, None], m / norm[:, None], np.array([1.0, 0.0, 0.0]))
            lat, lon = np.arcsin(np.clip(c[:, 2], -1.0, 1.0)), np.arctan2(c[:, 1], c[:, 0])
            zero = np.zeros_like(lat)
            e = np.stack([-np.sin(lon), np.cos(lon), zero], axis=1)
            n = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=1)
            cn = np.einsum("kij,kj->ki", cov, n)
            a, b, d = np.einsum("ki,kij,kj->k", e, cov, e), (e * cn).sum(axis=1), (n * cn).sum(axis=1)
            rad = np.sqrt(((a - d) / 2) ** 2 + b * b)
            lp, lm = np.maximum((a + d) / 2 + rad, 0.0), np.maximum((a + d) / 2 - rad, 0.0)
            theta = 0.5 * np.arctan2(2 * b, a - d)
        ok = s0 > 0
        return s0, m, cov, np.where(ok, lat, np.nan), np.where(ok, lon, np.nan), np.where(ok, lp, 0.0), np.where(ok, lm, 0.0), \
            np.where(ok, theta, np.nan)

    @staticmethod
    def values(shape_rows, rows, height: int, width: int) -> np.ndarray:
        """float64 [n, 10] (EVENT_SHAPE_VALUES): decode's numbers for whole arrays at once (what predict.py stores as
        event_shape_values).  NaN where the zeroth moment is 0 (lat, lon, orientation) or the perimeter is (compactness)."""
        s = np.asarray(shape_rows, np.int64).reshape(-1, len(EVENT_SHAPE_FIELDS))
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        _, _, _, lat, lon, lp, lm, theta = EventShape.moments(s, rows)
        dlat, dlon = EventShape.steps(height, width)
        out = np.empty((len(s), len(EVENT_SHAPE_VALUES)), np.float64)
        length, wid = EARTH_RADIUS_KM * EventShape.arc_angle(12.0 * lp), EARTH_RADIUS_KM * np.sqrt(12.0 * lm)
        perimeter = EARTH_RADIUS_KM * (dlat * s[:, 1].astype(np.float64) + dlon * s[:, 2].astype(np.float64) / EVENT_SCALE)
        area = EventFilter.area_km2(rows[:, 3].astype(np.float64), height, width)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 0], out[:, 1] = np.degrees(lat), np.degrees(lon)
            out[:, 2], out[:, 3] = length, wid
            out[:, 4] = np.where(lm > 0, np.sqrt(lp / lm), np.inf)
            out[:, 5] = np.degrees(theta)                     # atan2 lies in (-pi, pi]: half of it in (-90, 90]
            out[:, 6], out[:, 7] = perimeter, area
            out[:, 8] = np.where(perimeter > 0, 4.0 * math.pi * area / (perimeter * perimeter), np.nan)
            out[:, 9] = s[:, 0]
        return out

    @staticmethod
    def decode(shape_rows, rows, height: int, width: int):
        """Shape rows [n, 12] (EVENT_SHAPE_FIELDS) and the events' own rows [n, 10] (EVENT_FIELDS) -> one dict per event with the keys of
        EVENT_SHAPE_VALUES, R = 6371 km: lat / lon of the spherical centroid in degrees; sqrt(12 lambda+) and sqrt(12 lambda-) are the
        sides of the uniform strip with the same second moments in chord space (not a skeleton length).  width_km = R sqrt(12 lambda-).
        length_km = R theta with 6 (1 - sin(theta) / theta) = 12 lambda+: the great-circle arc with that second moment (arc_angle) --
        R sqrt(12 lambda+) itself is the chord-space figure and falls short of a long thin event by theta^2 / 40, 2.7 % at 6700 km.
        aspect = sqrt(lambda+ / lambda-), the ratio of the strip's sides and the number the filter compares (inf at width 0);
        orientation_deg of the major axis, counter-clockwise from east, in (-90, 90]; perimeter_km =
        R (dlat faces_v + dlon faces_h / 2^20); area_km2 from the catalogue's area; compactness = 4 pi area / perimeter^2;
        boundary_pixels."""
        vals = EventShape.values(shape_rows, rows, height, width)
        out = []
        for v in vals:
            d = {k: float(x) for k, x in zip(EVENT_SHAPE_VALUES, v)}
            d["boundary_pixels"] = int(v[9])
            out.append(d)
        return out


class EventFilter:
    """A size and shape filter for the events of a mask, on the device (dc_event_select + dc_mask_select behind an EventCatalog and an
    EventShape): an event of class k is kept iff it has at least min_pixels[k] pixels, min_area_km2[k] of area, min_length_km[k] of length
    and min_aspect[k] of aspect (EventShape.decode's numbers; 0: the criterion is off), and the filtered mask keeps the pixels of kept
    events -- and of events beyond the catalogue's cap, for which nothing was evaluated.  Each threshold is a pair (class 1, class 2).
    `catalog` is the filter's own catalogue of the RAW mask; whatever consumes the filtered mask (another EventCatalog, a matcher, a
    tracker, ...) does so unchanged.  Nothing is copied to the host and nothing synchronises."""

    def __init__(self, catalog: EventCatalog, min_pixels=(0, 0), min_area_km2=(0, 0), min_length_km=(0, 0), min_aspect=(0, 0)):
        self.min_pixels, self.min_area_km2 = self._pair(min_pixels, "min_pixels"), self._pair(min_area_km2, "min_area_km2")
        self.min_length_km, self.min_aspect = self._pair(min_length_km, "min_length_km"), self._pair(min_aspect, "min_aspect")
        self.catalog = catalog
        self.shape = EventShape(catalog)
        dev = catalog._labels.device
        self.criteria = self.criteria_rows(catalog.H, catalog.W, self.min_pixels, self.min_area_km2, self.min_length_km, self.min_aspect)
        self._criteria = torch.from_numpy(self.criteria.view(np.int64).copy()).to(dev)
        self._keep = torch.zeros((catalog.B, catalog.cap), dtype=torch.uint8, device=dev)
        self._counts = torch.zeros((catalog.B, 2, len(EVENT_FILTER_COUNTS)), dtype=torch.int64, device=dev)
        self._out = torch.zeros((catalog.B, catalog.H, catalog.W), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    @staticmethod
    def _pair(v, name):
        v = tuple(float(x) for x in (v if isinstance(v, (tuple, list, np.ndarray)) else (v, v)))
        if len(v) != 2 or any(not (x >= 0) or math.isinf(x) for x in v):
            raise L.DeepcamHipError(f"EventFilter: {name} takes two finite values >= 0 (class 1, class 2), got {v}")
        return v

    # -- the thresholds in the kernel's units, and back (the checker and the tests use the same ones)
    @staticmethod
    def pixel_area_km2(height: int, width: int) -> float:
        """km^2 of one pixel on the equator: R^2 dlat dlon"""
        dlat, dlon = EventShape.steps(height, width)
        return EARTH_RADIUS_KM * EARTH_RADIUS_KM * dlat * dlon

    @staticmethod
    def area_units(km2: float, height: int, width: int) -> int:
        """min_area: the smallest catalogue area (field 3: sum of 2^20 cos lat) that is at least km2"""
        return int(math.ceil(float(km2) / EventFilter.pixel_area_km2(height, width) * EVENT_SCALE))

    @staticmethod
    def area_km2(units, height: int, width: int):
        return units / float(EVENT_SCALE) * EventFilter.pixel_area_km2(height, width)

    @staticmethod
    def length_units(km: float) -> float:
        """min_len2 = chord_moment(km / R): length_km >= km  iff  12 lambda+ >= min_len2 (both sides of decode's arc_angle)"""
        theta = float(km) / EARTH_RADIUS_KM
        if not 0.0 <= theta <= EventShape.ARC_MAX:
            raise L.DeepcamHipError(f"EventFilter: a length threshold must lie in [0, {EARTH_RADIUS_KM * EventShape.ARC_MAX:.0f}] km, got {km}")
        return float(EventShape.chord_moment(theta))

    @staticmethod
    def length_km(len2: float) -> float:
        return EARTH_RADIUS_KM * float(EventShape.arc_angle(len2))

    @staticmethod
    def aspect_units(aspect: float) -> float:
        """min_aspect2 = aspect^2: decode's aspect >= aspect  iff  lambda+ >= min_aspect2 lambda-"""
        return float(aspect) ** 2

    @staticmethod
    def aspect(aspect2: float) -> float:
        return math.sqrt(aspect2)

    CRITERIA = np.dtype([("min_pixels", np.int64), ("min_area", np.int64), ("min_len2", np.float64), ("min_aspect2", np.float64)])

    @staticmethod
    def criteria_rows(height: int, width: int, min_pixels=(0, 0), min_area_km2=(0, 0), min_length_km=(0, 0), min_aspect=(0, 0)) -> np.ndarray:
        """the two rows dc_event_select takes (class 1, class 2), a numpy record array of dtype CRITERIA"""
        out = np.zeros(2, EventFilter.CRITERIA)
        for k in range(2):
            out[k] = (int(math.ceil(min_pixels[k])), EventFilter.area_units(min_area_km2[k], height, width),
                      EventFilter.length_units(min_length_km[k]), EventFilter.aspect_units(min_aspect[k]))
        return out

    def thresholds(self) -> dict:
        return {"min_pixels": list(self.min_pixels), "min_area_km2": list(self.min_area_km2), "min_length_km": list(self.min_length_km),
                "min_aspect": list(self.min_aspect)}

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> torch.Tensor:
        """mask: device uint8 [B, H, W].  Returns the filtered mask [n_valid, H, W], a view of a buffer this object owns (mask_buffer is
        the whole of it; the next call overwrites it).  Samples from n_valid on are padding: neither read nor written."""
        cat = self.catalog
        cat(mask, n_valid=n_valid)
        nv = cat._last_valid
        self.shape(nv)
        st = L.stream_ptr()
        L.call("dc_event_select", cat.B, nv, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(self.shape._shape), L.dptr(self._criteria),
               L.dptr(self._keep), L.dptr(self._counts), st)
        L.call("dc_mask_select", cat.B, nv, cat.H, cat.W, L.dptr(mask), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(self._keep),
               L.dptr(self._out), L.dptr(self._counts), st)
        self._last_valid = nv
        return self._out[:nv]

    @property
    def mask_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the whole buffer the filtered masks are written to, padding samples included"""
        return self._out

    @property
    def keep(self) -> torch.Tensor:
        """uint8 [n_valid, cap] of the last call (a view): 1 for a kept event, 0 for a dropped one and for rows without an event"""
        return self._keep[:self._last_valid]

    def counts(self) -> torch.Tensor:
        """int64 [n_valid, 2, 4] of the last call (a view): per class EVENT_FILTER_COUNTS (events among the ranks below cap)"""
        return self._counts[:self._last_valid]


TRACK_STORE_FIELDS = ("frame", "rank") + EVENT_FIELDS
TRACK_FIELDS = ("id", "class", "events", "first_frame", "last_frame", "pixels", "peak", "area")


class EventTracker:
    """Events linked across time steps on the device (dc_track_append, dc_track_link, dc_track_resolve, csrc/tracks.hip): the frames
    given since reset() are one time series, frame numbers 0, 1, 2, ...; two events of consecutive frames are linked when they have the
    same class, share at least one pixel and each has at least max(min_pixels, 1) pixels; a track is a connected component of the events
    under these links (merges and splits stay in one track), its id the smallest event number it holds (include/deepcam_hip.h has the
    definitions).  Built on an existing EventCatalog, as EventFields is.  The object owns the state that survives from call to call --
    the four counters, the forest over event numbers, the store (int64 [event_cap, 12], TRACK_STORE_FIELDS) -- and one-frame copies of
    the last frame's mask, labels, rank map and first event number, because the caller's mask buffer and the catalogue's workspace are
    overwritten by the next call.  A call must follow the catalogue's call for that mask on the same stream; it launches and neither
    synchronises nor reads anything back.  tracks() / rows() resolve and read back only the filled parts."""

    def __init__(self, catalog: EventCatalog, event_cap: int = 1 << 19, track_cap: Optional[int] = None, min_pixels: int = 0):
        event_cap = int(event_cap)
        track_cap = event_cap if track_cap is None else int(track_cap)
        if not 1 <= event_cap <= 1 << 30:
            raise L.DeepcamHipError(f"EventTracker: event_cap must lie in [1, 2^30], got {event_cap}")
        if not 1 <= track_cap <= event_cap:
            raise L.DeepcamHipError(f"EventTracker: track_cap must lie in [1, event_cap], got {track_cap}")
        if int(min_pixels) < 0:
            raise L.DeepcamHipError("EventTracker: min_pixels must not be negative")
        if event_cap > ((1 << 43) - 1) // (catalog.H * catalog.W):
            raise L.DeepcamHipError(f"EventTracker: event_cap * H * W * 2^20 must stay below 2^63, got event_cap {event_cap} at "
                                    f"{catalog.H} x {catalog.W}")
        self.catalog, self.event_cap, self.track_cap, self.min_pixels = catalog, event_cap, track_cap, int(min_pixels)
        dev = catalog._labels.device
        H, W = catalog.H, catalog.W
        self._state = torch.zeros(4, dtype=torch.int64, device=dev)
        self._first = torch.zeros(catalog.B, dtype=torch.int64, device=dev)
        self._parent = torch.empty(event_cap, dtype=torch.int32, device=dev)
        self._store = torch.empty((event_cap, len(TRACK_STORE_FIELDS)), dtype=torch.int64, device=dev)
        self._track_of = torch.empty(event_cap, dtype=torch.int32, device=dev)
        self._tracks = torch.zeros((track_cap, len(TRACK_FIELDS)), dtype=torch.int64, device=dev)
        self._ntracks = torch.zeros(4, dtype=torch.int64, device=dev)
        self._ws = torch.empty(L.load().dc_track_workspace(event_cap), dtype=torch.uint8, device=dev)
        # the carry: the last valid frame of the call before
        self._c_mask = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
        self._c_labels = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
        self._c_rank = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
        self._c_first = torch.zeros(1, dtype=torch.int64, device=dev)
        self._carry = False
        self._frames = 0                           # frames given since reset(), counted on the host: the next call's frame0
        self._last_valid = 0                       # the valid frames of the last call (TrackMatcher compares the two sides)

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> "EventTracker":
        """mask: the device uint8 [B, H, W] the catalogue was just called with.  n_valid defaults to the catalogue's and must equal it."""
        cat = self.catalog
        check_tensor("EventTracker", "mask", mask, (torch.uint8,), (cat.B, cat.H, cat.W), cat._labels.device, "uint8")
        nv = cat._last_valid if n_valid is None else int(n_valid)
        if nv < 1 or nv != cat._last_valid:
            raise L.DeepcamHipError(f"EventTracker: call the catalogue on this mask first, with the same n_valid (its last call had "
                                    f"{cat._last_valid}, this one has {nv})")
        HW, st = cat.H * cat.W, L.stream_ptr()
        at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())  # noqa: E731
        L.call("dc_track_append", cat.B, nv, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), self._frames, self.event_cap, L.dptr(self._state),
               L.dptr(self._first), L.dptr(self._parent), L.dptr(self._store), st)
        link = lambda n, a, b: L.call("dc_track_link", n, cat.H, cat.W, *a, *b, cat.cap, self.event_cap, self.min_pixels,  # noqa: E731
                                      L.dptr(self._store), L.dptr(self._parent), st)
        side = lambda k: (at(mask, k * HW), at(cat._labels, k * HW), at(cat._ws, 4 * k * HW), at(self._first, k))  # noqa: E731
        if nv > 1:
            link(nv - 1, side(0), side(1))
        if self._carry:
            link(1, (L.dptr(self._c_mask), L.dptr(self._c_labels), L.dptr(self._c_rank), L.dptr(self._c_first)), side(0))
        for dst, src in zip((self._c_mask, self._c_labels, self._c_rank, self._c_first), side(nv - 1)):
            L.call("dc_memcpy_async", L.dptr(dst), src, dst.numel() * dst.element_size(), st)
        self._carry = True
        self._frames += nv
        self._last_valid = nv
        return self

    def cut(self) -> None:
        """A break in the sequence: the next frame is not linked to the one before it.  Frame numbering goes on."""
        self._carry = False

    def reset(self) -> None:
        """Forget every frame: the next one is frame 0."""
        L.call("dc_memset_async", L.dptr(self._state), 0, 32, L.stream_ptr())
        self._carry = False
        self._frames = 0

    def state(self) -> dict:
        """the four counters (one device-to-host read)"""
        s = [int(v) for v in self._state.cpu().tolist()]
        return {"events": s[0], "frames": s[1], "events_dropped": s[2], "frames_truncated": s[3]}

    def resolve(self) -> "EventTracker":
        """dc_track_resolve on the current stream: track_of, the track rows and the counts for the frames given so far.  Does not
        synchronise; may be called in the middle of a series."""
        L.call("dc_track_resolve", self.event_cap, self.track_cap, L.dptr(self._state), L.dptr(self._parent), L.dptr(self._store),
               L.dptr(self._track_of), L.dptr(self._tracks), L.dptr(self._ntracks), L.dptr(self._ws), L.stream_ptr())
        return self

    def track_counts(self) -> np.ndarray:
        """int64 [4] of the last resolve: tracks of any class, of class 1, of class 2 (not capped), rows stored"""
        return self._ntracks.cpu().numpy()

    def rows(self):
        """(state int64 [4], store rows int64 [n, 12], track_of int32 [n], track rows int64 [m, 8]) as numpy arrays: resolves, reads the
        counters, then only the filled parts."""
        self.resolve()
        state = self._state.cpu().numpy()
        n, m = int(state[0]), int(self._ntracks[3].item())
        return state, self._store[:n].cpu().numpy(), self._track_of[:n].cpu().numpy(), self._tracks[:m].cpu().numpy()

    def tracks(self, min_frames: int = 1):
        """The tracks of the frames given so far as a list of dicts (decode), those of fewer than min_frames frames left out."""
        _, store, track_of, tracks = self.rows()
        return self.decode(store, track_of, tracks, self.catalog.H, self.catalog.W, min_frames=min_frames)

    @staticmethod
    def decode(store, track_of, tracks, height: int, width: int, min_frames: int = 1):
        """Store rows [n, 12] (TRACK_STORE_FIELDS), track_of [n] and track rows [m, 8] (TRACK_FIELDS) -> one dict per track with at least
        min_frames frames, in row order: id, class, first_frame, last_frame, frames (last - first + 1), events, pixels, peak_pixels and
        peak_frame (the largest single event and its frame, the earliest among equals), area_fraction_sum (the events' area fractions
        summed) and path: per frame of the track its events' count, their pixels and the centroid lat / lon by EventCatalog.decode's
        formulas over the SUMMED columns, so two fragments of one frame give their joint centroid.  Needs no GPU."""
        store = np.asarray(store, np.int64).reshape(-1, len(TRACK_STORE_FIELDS))
        track_of = np.asarray(track_of, np.int64).reshape(-1)
        tracks = np.asarray(tracks, np.int64).reshape(-1, len(TRACK_FIELDS))
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        order = np.argsort(track_of, kind="stable")
        lo = np.searchsorted(track_of[order], np.arange(len(tracks)), side="left")
        hi = np.searchsorted(track_of[order], np.arange(len(tracks)), side="right")
        out = []
        for t, row in enumerate(tracks.tolist()):
            tid, cls, nev, f0, f1, px, peak, area = row
            if f1 - f0 + 1 < min_frames:
                continue
            peak &= 0xFFFFFFFFFFFFFFFF
            ev = store[order[lo[t]:hi[t]]]
            path = []
            for f in np.unique(ev[:, 0]).tolist():
                n, sr, scx, ssx = (int(v) for v in ev[ev[:, 0] == f][:, [4, 6, 7, 8]].sum(axis=0))
                lat = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 and n > 0 else -90.0
                path.append({"frame": f, "events": int((ev[:, 0] == f).sum()), "pixels": n, "lat": lat, "lon": math.degrees(math.atan2(ssx, scx))})
            out.append({"id": tid, "class": cls, "first_frame": f0, "last_frame": f1, "frames": f1 - f0 + 1, "events": nev, "pixels": px,
                        "peak_pixels": peak >> 32, "peak_frame": 0xFFFFFFFF - (peak & 0xFFFFFFFF),
                        "area_fraction_sum": area / whole if whole > 0 else 0.0, "path": path})
        return out


TRACK_STEP_FIELDS = ("track", "frame", "events", "pixels", "area", "sum_row", "sum_cx", "sum_sx")
TRACK_FIELD_STATS = ("min", "min_pixel", "max", "max_pixel")


class TrackFields:
    """Storm life cycles on the device (dc_track_fields_append, dc_track_cycles, csrc/tracks.hip): the join of an EventTracker (which
    events of which frames form one storm) and an EventFields of the same catalogue (every event's extremes and sums of the raw fields).
    Per track and frame -- a STEP -- the field rows of the track's events in that frame merged into one (for a cyclone and sea-level
    pressure the minimum's place is the conventional track position, its value the intensity), per track the lifetime extremes with the
    frame and place where they occurred (include/deepcam_hip.h has the definitions).  The object owns the field store (int64 [event_cap,
    C, 6]: 48 * C bytes per event slot next to the tracker's store, 403 MB at the tracker's default event_cap = 2^19 with 16 channels) and
    the output tables: offsets int64 [track_cap], steps int64 [step_cap, 8] (TRACK_STEP_FIELDS), step_fields int64 [step_cap, C, 6]
    (EVENT_FIELD_STATS), track_fields int64 [track_cap, C, 4] (TRACK_FIELD_STATS) and the four counters.  A call launches and neither
    synchronises nor reads anything back; reset() and cut() are the tracker's -- the state follows its counters.  rows() / cycles() resolve
    and read back only the filled parts."""

    def __init__(self, tracker: "EventTracker", fields: EventFields, step_cap: Optional[int] = None):
        if not isinstance(tracker, EventTracker) or not isinstance(fields, EventFields):
            raise L.DeepcamHipError("TrackFields: needs an EventTracker and an EventFields")
        if tracker.catalog is not fields.catalog:
            raise L.DeepcamHipError("TrackFields: the tracker and the fields must be built on the same EventCatalog")
        step_cap = tracker.event_cap if step_cap is None else int(step_cap)
        if not 1 <= step_cap <= (1 << 31) - 1:
            raise L.DeepcamHipError(f"TrackFields: step_cap must lie in [1, 2^31 - 1], got {step_cap}")
        self.tracker, self.fields, self.C, self.step_cap = tracker, fields, fields.C, step_cap
        dev = tracker._store.device
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
        self._fstore = torch.empty((tracker.event_cap, self.C, len(EVENT_FIELD_STATS)), dtype=torch.int64, device=dev)
        self._offsets = i64(tracker.track_cap)
        self._steps = i64(step_cap, len(TRACK_STEP_FIELDS))
        self._step_fields = i64(step_cap, self.C, len(EVENT_FIELD_STATS))
        self._track_fields = i64(tracker.track_cap, self.C, len(TRACK_FIELD_STATS))
        self._ncycles = i64(4)
        self._ws = torch.empty(max(L.load().dc_track_cycles_workspace(tracker.event_cap, tracker.track_cap), 256), dtype=torch.uint8, device=dev)

    def __call__(self) -> "TrackFields":
        """Files the field rows of the batch the tracker and the fields were just called with (both, on this stream, before this)."""
        trk, fld, cat = self.tracker, self.fields, self.tracker.catalog
        nv = cat._last_valid
        if nv < 1 or fld._last_valid != nv:
            raise L.DeepcamHipError(f"TrackFields: call the tracker and the fields on the same batch first (the catalogue's last call had "
                                    f"{nv} valid samples, the fields' {fld._last_valid})")
        L.call("dc_track_fields_append", cat.B, nv, cat.cap, L.dptr(cat._ncomp), L.dptr(trk._first), L.dptr(fld._ftable), self.C, trk.event_cap,
               L.dptr(self._fstore), L.stream_ptr())
        return self

    @staticmethod
    def class_mask(classes) -> int:
        mask = 0
        for c in classes:
            if int(c) not in (1, 2):
                raise L.DeepcamHipError(f"TrackFields: classes are 1 and 2, got {c}")
            mask |= 1 << int(c)
        if mask == 0:
            raise L.DeepcamHipError("TrackFields: no class selected")
        return mask

    def launch(self, min_frames: int = 1, classes=(1, 2)) -> "TrackFields":
        """dc_track_resolve and dc_track_cycles on the current stream, for the frames given so far.  Does not synchronise."""
        trk = self.tracker
        trk.resolve()
        L.call("dc_track_cycles", trk.event_cap, trk.track_cap, self.step_cap, self.C, max(int(min_frames), 0), self.class_mask(classes),
               L.dptr(trk._state), L.dptr(trk._store), L.dptr(trk._track_of), L.dptr(trk._tracks), L.dptr(trk._ntracks), L.dptr(self._fstore),
               L.dptr(self._offsets), L.dptr(self._steps), L.dptr(self._step_fields), L.dptr(self._track_fields), L.dptr(self._ncycles),
               L.dptr(self._ws), L.stream_ptr())
        return self

    def rows(self, min_frames: int = 1, classes=(1, 2)) -> dict:
        """launch(), then the counters and only the filled parts as numpy arrays: "counts" int64 [4] (tracks selected, step rows needed, step
        rows stored, tracks selected but not stored), "tracks" int64 [m, 8], "offsets" int64 [m], "steps" int64 [n, 8], "step_fields" int64
        [n, C, 6], "track_fields" int64 [m, C, 4], with m the tracker's stored track rows and n the stored step rows."""
        self.launch(min_frames, classes)
        counts = self._ncycles.cpu().numpy()
        m, n = int(self.tracker._ntracks[3].item()), int(counts[2])
        return {"counts": counts, "tracks": self.tracker._tracks[:m].cpu().numpy(), "offsets": self._offsets[:m].cpu().numpy(),
                "steps": self._steps[:n].cpu().numpy(), "step_fields": self._step_fields[:n].cpu().numpy(),
                "track_fields": self._track_fields[:m].cpu().numpy()}

    def cycles(self, min_frames: int = 1, classes=(1, 2), center_channel: Optional[int] = None):
        """The life cycles of the frames given so far as a list of dicts (decode)."""
        r = self.rows(min_frames, classes)
        cat = self.tracker.catalog
        return self.decode(r["tracks"], r["offsets"], r["steps"], r["step_fields"], r["track_fields"], cat.H, cat.W, self.fields.bits,
                           center_channel=center_channel)

    @staticmethod
    def decode(tracks, offsets, steps, step_fields, track_fields, height: int, width: int, bits, center_channel: Optional[int] = None):
        """Track rows [m, 8] (TRACK_FIELDS), offsets [m], step rows [n, 8] (TRACK_STEP_FIELDS), their field rows [n, C, 6]
        (EVENT_FIELD_STATS) and the lifetime rows [m, C, 4] (TRACK_FIELD_STATS) -> one dict per STORED track (offsets >= 0), in row order:
        id, class, first_frame, last_frame, frames, events, pixels, peak_pixels, peak_frame, area_fraction_sum as EventTracker.decode gives
        them; fields: per channel min, min_frame, min_row, min_col, min_lat, min_lon, the same for max (None where the track has no finite
        value), mean = the step sums added in Python integers * 2^-bits / the pixels that took part (None without any) and nonfinite,
        saturated; series: per frame of the track frame, events, pixels, the centroid lat / lon by EventCatalog.decode's formulas over the
        summed columns, and fields: the EventFields.decode entries of the merged row.  With center_channel = c every series entry also
        has center_lat / center_lon, the place of channel c's minimum (None where the step has no finite value).  Needs no GPU."""
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        nch = len(bits)
        tracks = np.asarray(tracks, np.int64).reshape(-1, len(TRACK_FIELDS))
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        steps = np.asarray(steps, np.int64).reshape(-1, len(TRACK_STEP_FIELDS))
        step_fields = np.asarray(step_fields, np.int64).reshape(-1, nch, len(EVENT_FIELD_STATS))
        track_fields = np.asarray(track_fields, np.int64).reshape(-1, nch, len(TRACK_FIELD_STATS))
        if center_channel is not None and not 0 <= int(center_channel) < nch:
            raise L.DeepcamHipError(f"TrackFields: center_channel must lie in [0, {nch}), got {center_channel}")
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        out = []
        for t, row in enumerate(tracks.tolist()):
            off = int(offsets[t])
            if off < 0:
                continue
            tid, cls, nev, f0, f1, px, peak, area = row
            peak &= 0xFFFFFFFFFFFFFFFF
            st = steps[off:off + f1 - f0 + 1]
            sf = step_fields[off:off + f1 - f0 + 1]
            if len(st) != f1 - f0 + 1 or (st[:, 0] != t).any() or (st[:, 1] != np.arange(f0, f1 + 1)).any():
                raise L.DeepcamHipError(f"TrackFields.decode: the step rows of track row {t} are not its frames {f0} .. {f1}")
            # a step as one event row (EVENT_FIELDS): pixels, area and the centroid sums are the columns the decoders read
            pseudo = np.zeros((len(st), len(EVENT_FIELDS)), np.int64)
            pseudo[:, 1], pseudo[:, 2:7] = cls, st[:, 3:8]
            per_step = EventFields.decode(sf, pseudo, height, width, bits)
            series = []
            for (_, f, n_ev, n, _a, sr, scx, ssx), per in zip(st.tolist(), per_step):
                la = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 and n > 0 else -90.0
                entry = {"frame": f, "events": n_ev, "pixels": n, "lat": la, "lon": math.degrees(math.atan2(ssx, scx)), "fields": per}
                if center_channel is not None:
                    entry["center_lat"], entry["center_lon"] = per[int(center_channel)]["min_lat"], per[int(center_channel)]["min_lon"]
                series.append(entry)
            life = []
            for ch, (wlo, plo, whi, phi) in enumerate(track_fields[t].tolist()):
                total = sum(int(v) for v in sf[:, ch, 2])
                nonfinite, saturated = int(sf[:, ch, 4].sum()), int(sf[:, ch, 5].sum())
                n = px - nonfinite - saturated
                d = {"nonfinite": nonfinite, "saturated": saturated, "mean": math.ldexp(float(total), -bits[ch]) / n if n > 0 else None}
                for name, word, p, empty in (("min", wlo, plo, -1), ("max", whi, phi, 0)):
                    if word == empty:
                        d.update({name: None, name + "_frame": None, name + "_row": None, name + "_col": None, name + "_lat": None,
                                  name + "_lon": None})
                        continue
                    word &= 0xFFFFFFFFFFFFFFFF
                    frame = word & 0xFFFFFFFF if name == "min" else 0xFFFFFFFF - (word & 0xFFFFFFFF)
                    d.update({name: float(event_field_value(np.uint32(word >> 32))), name + "_frame": frame, name + "_row": p // width,
                              name + "_col": p % width, name + "_lat": float(lat[p // width]), name + "_lon": float(lon[p % width])})
                life.append(d)
            out.append({"id": tid, "class": cls, "first_frame": f0, "last_frame": f1, "frames": f1 - f0 + 1, "events": nev, "pixels": px,
                        "peak_pixels": peak >> 32, "peak_frame": 0xFFFFFFFF - (peak & 0xFFFFFFFF),
                        "area_fraction_sum": area / whole if whole > 0 else 0.0, "fields": life, "series": series})
        return out


TRACK_PAIR_FIELDS = ("row_a", "row_b", "class", "overlaps", "common_frames", "shared_pixels", "first_common_frame", "last_common_frame")
TRACK_COVER_FIELDS = ("matched_frames", "shared_pixels")


def great_circle_km(lat_a: float, lon_a: float, lat_b: float, lon_b: float) -> float:
    """the great-circle distance of two points given in degrees, in km on the sphere of EARTH_RADIUS_KM (haversine, float64)"""
    pa, pb = math.radians(lat_a), math.radians(lat_b)
    h = math.sin((pb - pa) / 2) ** 2 + math.cos(pa) * math.cos(pb) * math.sin(math.radians(lon_b - lon_a) / 2) ** 2
    return 2.0 * EARTH_RADIUS_KM * math.asin(min(1.0, math.sqrt(h)))


class TrackMatcher:
    """Predicted against labelled storm tracks on the device (dc_track_match_append, dc_track_match_resolve, csrc/track_match.hip): the
    join of an EventMatcher (side a: the prediction, side b: the labels) and one EventTracker on each of its two catalogues.  Every
    overlap of two stored events of the same class is filed as a link (event a, event b, shared pixels); at resolve time the links are
    grouped by (track row a, track row b) -- overlaps, DISTINCT common frames, shared pixels, first and last common frame per pair --
    and every track gets its matched frames (the distinct frames in which one of its events overlaps any track of the other side) and
    its shared pixels.  A track is SCORED when it has a row and at least max(min_frames, 1) frames; it is MATCHED when matched >= 1 and
    matched * 1024 >= round(min_cover * 1024) * frames.  Coverage, not pairwise overlap, decides: a labelled storm predicted as two tracks
    with a missed frame in between is still found, and the pairs show the fragmentation (include/deepcam_hip.h has the definitions).
    The object owns the link store (int64 [link_cap, 3]: 24 bytes per link), the four counters, the outputs (pairs int64 [pair_cap, 8],
    TRACK_PAIR_FIELDS; cover int64 [track_cap, 2] per side, TRACK_COVER_FIELDS; scores int64 [2, 4]; counts int64 [4]) and the resolve's
    workspace.  A call follows the matcher's call and both trackers' calls of the same batch on the same stream; it launches once and
    neither synchronises nor reads anything back.  rows() / pairs() / result() resolve and read back only the filled parts."""

    SCORE_FIELDS = EventMatcher.SCORE_FIELDS

    def __init__(self, matcher: EventMatcher, tracker_a: "EventTracker", tracker_b: "EventTracker", link_cap: int = 1 << 20,
                 pair_cap: int = 1 << 16, min_frames: int = 1, min_cover: float = 0.5):
        link_cap, pair_cap, min_frames = int(link_cap), int(pair_cap), int(min_frames)
        check_range("TrackMatcher", "link_cap", link_cap, 1, 1 << 26)
        check_range("TrackMatcher", "pair_cap", pair_cap, 1, 1 << 24)
        check_range("TrackMatcher", "min_frames", min_frames, 0, (1 << 31) - 1)
        if not 0.0 < float(min_cover) <= 1.0:
            raise L.DeepcamHipError(f"TrackMatcher: min_cover must lie in (0, 1], got {min_cover}")
        if not isinstance(matcher, EventMatcher) or not isinstance(tracker_a, EventTracker) or not isinstance(tracker_b, EventTracker):
            raise L.DeepcamHipError("TrackMatcher: needs an EventMatcher and two EventTrackers")
        if tracker_a.catalog is not matcher.a or tracker_b.catalog is not matcher.b:
            raise L.DeepcamHipError("TrackMatcher: tracker_a must be built on matcher.a and tracker_b on matcher.b")
        self.matcher, self.tracker_a, self.tracker_b = matcher, tracker_a, tracker_b
        self.link_cap, self.pair_cap, self.min_frames = link_cap, pair_cap, min_frames
        self.cover_q = min(max(int(round(float(min_cover) * 1024)), 1), 1024)
        dev = tracker_a._store.device
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
        self._state = i64(4)
        self._links = torch.empty((link_cap, 3), dtype=torch.int64, device=dev)
        self._tpairs = i64(pair_cap, len(TRACK_PAIR_FIELDS))
        self._cover_a = i64(tracker_a.track_cap, len(TRACK_COVER_FIELDS))
        self._cover_b = i64(tracker_b.track_cap, len(TRACK_COVER_FIELDS))
        self._scores = i64(2, 4)
        self._counts = i64(4)
        nbytes = L.load().dc_track_match_workspace(tracker_a.event_cap, tracker_b.event_cap, tracker_a.track_cap, tracker_b.track_cap, link_cap,
                                                   pair_cap)
        if nbytes == 0:
            raise L.DeepcamHipError("TrackMatcher: a capacity is out of range")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._frames = 0                           # frames filed since reset(), counted on the host

    def __call__(self) -> "TrackMatcher":
        """Files the overlaps of the batch the matcher and both trackers were just called with (all three, on this stream, before this)."""
        m, ta, tb = self.matcher, self.tracker_a, self.tracker_b
        nv = m._last_valid
        if nv < 1 or ta._last_valid != nv or tb._last_valid != nv:
            raise L.DeepcamHipError(f"TrackMatcher: call the matcher and both trackers on the same batch first, with the same n_valid (the "
                                    f"matcher's last call had {nv}, the trackers' {ta._last_valid} and {tb._last_valid})")
        if ta._frames != tb._frames or ta._frames != self._frames + nv:
            raise L.DeepcamHipError(f"TrackMatcher: both trackers must have seen the frames filed so far and this batch ({self._frames} + {nv}); "
                                    f"they have seen {ta._frames} and {tb._frames}")
        L.call("dc_track_match_append", m.B, nv, m.a.cap, m.b.cap, m.pair_cap, L.dptr(m._pairs), L.dptr(m._npairs), L.dptr(m.a._ncomp),
               L.dptr(ta._first), ta.event_cap, L.dptr(ta._store), L.dptr(m.b._ncomp), L.dptr(tb._first), tb.event_cap, L.dptr(tb._store),
               self.link_cap, L.dptr(self._links), L.dptr(self._state), L.stream_ptr())
        self._frames += nv
        return self

    def reset(self) -> None:
        """Forget every link.  The caller resets the two trackers."""
        L.call("dc_memset_async", L.dptr(self._state), 0, 32, L.stream_ptr())
        self._frames = 0

    def state(self) -> dict:
        """the four counters (one device-to-host read)"""
        s = [int(v) for v in self._state.cpu().tolist()]
        return {"links": s[0], "links_dropped": s[1], "frames": s[2], "frames_truncated": s[3]}

    def resolve(self) -> "TrackMatcher":
        """dc_track_resolve of both trackers, then dc_track_match_resolve, on the current stream, for the frames filed so far.  Does not
        synchronise; may be called in the middle of a series."""
        ta, tb = self.tracker_a.resolve(), self.tracker_b.resolve()
        L.call("dc_track_match_resolve", ta.event_cap, tb.event_cap, ta.track_cap, tb.track_cap, self.link_cap, self.pair_cap, self.min_frames,
               self.cover_q, L.dptr(self._state), L.dptr(self._links), L.dptr(ta._store), L.dptr(ta._track_of), L.dptr(ta._tracks),
               L.dptr(ta._ntracks), L.dptr(tb._track_of), L.dptr(tb._tracks), L.dptr(tb._ntracks), L.dptr(self._tpairs), L.dptr(self._cover_a),
               L.dptr(self._cover_b), L.dptr(self._scores), L.dptr(self._counts), L.dptr(self._ws), L.stream_ptr())
        return self

    @staticmethod
    def sort_pairs(rows) -> np.ndarray:
        """the stored rows [n, 8] ordered by (row a, row b)"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(TRACK_PAIR_FIELDS))
        return np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0]))])

    def rows(self) -> dict:
        """resolve(), then the counters and only the filled parts as numpy arrays: "state" int64 [4], "counts" int64 [4] (pair rows stored,
        the pair overflow flag, links skipped for a missing track row, 0), "scores" int64 [2, 4], "pairs" int64 [n, 8] sorted by (row a,
        row b), "cover_a" int64 [ma, 2], "cover_b" int64 [mb, 2], "tracks_a" int64 [ma, 8], "tracks_b" int64 [mb, 8] (TRACK_FIELDS), with
        ma / mb the stored track rows of the two trackers."""
        self.resolve()
        ta, tb = self.tracker_a, self.tracker_b
        counts = self._counts.cpu().numpy()
        ma, mb = int(ta._ntracks[3].item()), int(tb._ntracks[3].item())
        return {"state": self._state.cpu().numpy(), "counts": counts, "scores": self._scores.cpu().numpy(),
                "pairs": self.sort_pairs(self._tpairs[:int(counts[0])].cpu().numpy()), "cover_a": self._cover_a[:ma].cpu().numpy(),
                "cover_b": self._cover_b[:mb].cpu().numpy(), "tracks_a": ta._tracks[:ma].cpu().numpy(), "tracks_b": tb._tracks[:mb].cpu().numpy()}

    def pairs(self) -> np.ndarray:
        """the track-pair rows int64 [n, 8] (TRACK_PAIR_FIELDS) sorted by (row a, row b)"""
        return self.rows()["pairs"]

    def cover(self):
        """(cover_a [ma, 2], cover_b [mb, 2]) (TRACK_COVER_FIELDS) of the stored track rows"""
        r = self.rows()
        return r["cover_a"], r["cover_b"]

    def scores(self) -> np.ndarray:
        """int64 [2, 4]: per class 1, 2 the SCORE_FIELDS of tracks"""
        return self.rows()["scores"]

    @staticmethod
    def decode(pairs, tracks_a, tracks_b, min_frames: int = 1):
        """Track-pair rows [n, 8] (TRACK_PAIR_FIELDS) and the two sides' tracks as EventTracker.decode gives them with min_frames = 1 (one
        dict per track row, in row order) -> one dict per pair whose two tracks have at least min_frames frames, in the rows' order: row_a,
        row_b, id_a, id_b, class, overlaps, common_frames, shared_pixels, first_common_frame, last_common_frame, frames_a, frames_b,
        genesis_error = first_frame_a - first_frame_b (positive: the prediction is late), lysis_error = last_frame_a - last_frame_b,
        duration_error = frames_a - frames_b, and mean_separation_km: the great-circle distance (float64, R = 6371 km) between the two
        paths' joint centroids, averaged over the frames from the first to the last common frame -- both tracks live in every one of
        them; a frame in between without an overlap counts with its distance.  Needs no GPU."""
        out = []
        for ra, rb, cls, links, common, shared, f0, f1 in np.asarray(pairs, np.int64).reshape(-1, len(TRACK_PAIR_FIELDS)).tolist():
            a, b = tracks_a[ra], tracks_b[rb]
            if min(a["frames"], b["frames"]) < max(int(min_frames), 1):
                continue
            pa = {p["frame"]: p for p in a["path"]}
            pb = {p["frame"]: p for p in b["path"]}
            dist = [great_circle_km(pa[f]["lat"], pa[f]["lon"], pb[f]["lat"], pb[f]["lon"]) for f in range(f0, f1 + 1) if f in pa and f in pb]
            out.append({"row_a": ra, "row_b": rb, "id_a": a["id"], "id_b": b["id"], "class": cls, "overlaps": links, "common_frames": common,
                        "shared_pixels": shared, "first_common_frame": f0, "last_common_frame": f1, "frames_a": a["frames"],
                        "frames_b": b["frames"], "genesis_error": a["first_frame"] - b["first_frame"],
                        "lysis_error": a["last_frame"] - b["last_frame"], "duration_error": a["frames"] - b["frames"],
                        "mean_separation_km": _ratio(math.fsum(dist), len(dist))})
        return out

    def _decoded_tracks(self):
        cat = self.tracker_a.catalog
        return [EventTracker.decode(*t.rows()[1:], cat.H, cat.W) for t in (self.tracker_a, self.tracker_b)]

    def matches(self, min_frames: Optional[int] = None):
        """The joined track pairs of the frames filed so far (decode); min_frames defaults to the matcher's."""
        mf = self.min_frames if min_frames is None else int(min_frames)
        return self.decode(self.pairs(), *self._decoded_tracks(), min_frames=mf)

    @staticmethod
    def is_matched(matched: int, frames: int, cover_q: int) -> bool:
        return matched >= 1 and matched * 1024 >= cover_q * frames

    @staticmethod
    def summarize(rows: dict, matches, min_frames: int, cover_q: int) -> dict:
        """rows() and decode(rows["pairs"], ..., min_frames=1) -> the summary: the counters ("frames", "links", "links_dropped",
        "frames_truncated", "pairs", "pairs_overflowed", "links_without_track", "truncated": any of the four non-zero -- counts may be
        short), "min_frames", "min_cover" (cover_q / 1024) and per class "class_1", "class_2": the SCORE_FIELDS of tracks with
        EventMatcher.rates (pod, far, csi), and over the matched scored b tracks that have a stored pair -- each with its BEST partner: most
        common frames, then most shared pixels, then smallest row a -- "partnered" (their number), "mean_abs_genesis_error",
        "mean_abs_lysis_error", "mean_separation_km" and "mean_partners" (the pairs per such b track: 1 means no fragmentation).  None where
        a denominator is zero.  Needs no GPU."""
        state, counts = [int(v) for v in rows["state"]], [int(v) for v in rows["counts"]]
        scores = np.asarray(rows["scores"], np.int64).reshape(2, 4)
        out = {"frames": state[2], "links": state[0], "links_dropped": state[1], "frames_truncated": state[3], "pairs": counts[0],
               "pairs_overflowed": counts[1] != 0, "links_without_track": counts[2],
               "truncated": bool(state[1] or state[3] or counts[1] or counts[2]), "min_frames": int(min_frames), "min_cover": cover_q / 1024}
        by_b: dict = {}
        for m in matches:
            by_b.setdefault(m["row_b"], []).append(m)
        need = max(int(min_frames), 1)
        for k in (1, 2):
            h, mi, fa, md = (int(v) for v in scores[k - 1])
            best, partners = [], 0
            for t, (row, cov) in enumerate(zip(np.asarray(rows["tracks_b"], np.int64).tolist(), np.asarray(rows["cover_b"], np.int64).tolist())):
                frames = row[4] - row[3] + 1
                if row[1] != k or frames < need or not TrackMatcher.is_matched(cov[0], frames, cover_q) or t not in by_b:
                    continue
                partners += len(by_b[t])
                best.append(min(by_b[t], key=lambda m: (-m["common_frames"], -m["shared_pixels"], m["row_a"])))
            sep = [m["mean_separation_km"] for m in best if m["mean_separation_km"] is not None]
            out[f"class_{k}"] = {"hits": h, "misses": mi, "false_alarms": fa, "matched": md, **EventMatcher.rates(h, mi, fa, md),
                                 "partnered": len(best),
                                 "mean_abs_genesis_error": _ratio(sum(abs(m["genesis_error"]) for m in best), len(best)),
                                 "mean_abs_lysis_error": _ratio(sum(abs(m["lysis_error"]) for m in best), len(best)),
                                 "mean_separation_km": _ratio(math.fsum(sep), len(sep)), "mean_partners": _ratio(partners, len(best))}
        return out

    def result(self) -> dict:
        """summarize() of the frames filed so far"""
        rows = self.rows()
        return self.summarize(rows, self.decode(rows["pairs"], *self._decoded_tracks(), min_frames=1), self.min_frames, self.cover_q)
