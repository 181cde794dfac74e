"""Checker of the storm life cycles (nn.TrackFields, dc_track_fields_append / dc_track_cycles): the definition of include/deepcam_hip.h in
plain loops on Python integers, and the frame sequences the CPU and the GPU tests share.

cycles() takes host copies of what the tracker left (store [n, 12], track_of [n], tracks [m, 8]) and the per-event field rows [n, C, 6]:
  selected   track row t with last - first + 1 >= max(min_frames, 1) and bit `class` of class_mask set; need[t] = the frames of the selected
             rows before it; stored iff need[t] + frames[t] <= step_cap
  offsets    [m]: need[t] for stored rows, -1 not selected, -2 selected but not stored
  ncycles    [4]: tracks selected, step rows needed, step rows stored, tracks selected but not stored
  steps      [stored rows, 8]: row offsets[t] + f - first[t] = track row, frame, events, and the sums of the store columns pixels, area,
             sum_row, sum_cx, sum_sx over the track's events of frame f
  step_fields [stored rows, C, 6]: unsigned minimum of the min words, unsigned maximum of the max words, sums of the other four
  track_fields [m, C, 4]: (key << 32) | frame and pixel of the lexicographic minimum of (key, frame, pixel) over the track's steps with a
             finite value, empty (-1, -1); (key << 32) | (0xFFFFFFFF - frame) and pixel of the largest key, then the earliest frame, then
             the smallest pixel, empty (0, -1)
Every input is also held against the interval property the device layout rests on: the frames of a track are exactly first .. last."""
import functools
import zlib

import numpy as np

import util_event_fields as uef
import util_tracks as ut

STEP, LIFE = 8, 4
M64 = (1 << 64) - 1
I63 = 1 << 63


def _i64(v: int) -> int:
    """the int64 that holds the low 64 bits of v"""
    v &= M64
    return v - (1 << 64) if v >= I63 else v


def assert_intervals(store, track_of, tracks):
    """every frame from a track's first to its last holds at least one of its events, and no event lies outside"""
    seen = [set() for _ in range(len(tracks))]
    for e in range(len(store)):
        if track_of[e] >= 0:
            seen[int(track_of[e])].add(int(store[e, 0]))
    for t, row in enumerate(np.asarray(tracks).tolist()):
        assert seen[t] == set(range(row[3], row[4] + 1)), f"track row {t}: frames {sorted(seen[t])} are not the interval {row[3]} .. {row[4]}"


def cycles(store, track_of, tracks, frows, step_cap, min_frames=1, class_mask=6):
    store, track_of, tracks = np.asarray(store, np.int64), np.asarray(track_of, np.int64), np.asarray(tracks, np.int64).reshape(-1, ut.TRACK)
    frows = np.asarray(frows, np.int64)
    n, m, C = len(store), len(tracks), frows.shape[1]
    assert frows.shape == (n, C, uef.STATS) and len(track_of) == n
    assert_intervals(store, track_of, tracks)
    offsets = np.full(m, -1, np.int64)
    selected = need = stored = left = 0
    for t in range(m):
        frames, cls = int(tracks[t, 4] - tracks[t, 3] + 1), int(tracks[t, 1])
        if frames < max(int(min_frames), 1) or not (class_mask >> cls) & 1:
            continue
        selected += 1
        if need + frames <= step_cap:
            offsets[t] = need
            stored += frames
        else:
            offsets[t] = -2
            left += 1
        need += frames
    steps = [[0] * STEP for _ in range(stored)]
    sf = [[[M64, 0, 0, 0, 0, 0] for _ in range(C)] for _ in range(stored)]
    fr = frows.tolist()
    for e in range(n):
        t = int(track_of[e])
        if t < 0 or offsets[t] < 0:
            continue
        f = int(store[e, 0])
        row = int(offsets[t]) + f - int(tracks[t, 3])
        s = steps[row]
        s[0], s[1] = t, f
        s[2] += 1
        for k, col in enumerate((4, 5, 6, 7, 8)):
            s[3 + k] += int(store[e, col])
        for ch in range(C):
            a, b = sf[row][ch], fr[e][ch]
            a[0], a[1] = min(a[0], b[0] & M64), max(a[1], b[1] & M64)
            for k in range(2, 6):
                a[k] += b[k]
    life = [[[M64, M64, 0, M64] for _ in range(C)] for _ in range(m)]
    for t in range(m):
        if offsets[t] < 0:
            continue
        for ch in range(C):
            lo = hi = None
            for f in range(int(tracks[t, 3]), int(tracks[t, 4]) + 1):
                a = sf[int(offsets[t]) + f - int(tracks[t, 3])][ch]
                if a[0] == M64:
                    assert a[1] == 0
                    continue
                cand = (a[0] >> 32, f, a[0] & 0xFFFFFFFF)
                lo = cand if lo is None or cand < lo else lo
                cand = (a[1] >> 32, -f, -(0xFFFFFFFF - (a[1] & 0xFFFFFFFF)))
                hi = cand if hi is None or cand > hi else hi
            if lo is not None:
                life[t][ch] = [(lo[0] << 32) | lo[1], lo[2], (hi[0] << 32) | (0xFFFFFFFF - -hi[1]), -hi[2]]
    to64 = lambda rows, shape: np.array([_i64(v) for v in np.array(rows, object).reshape(-1).tolist()], np.int64).reshape(shape)  # noqa: E731
    for row in sf:
        for a in row:
            assert all(-I63 <= v < I63 for v in a[2:]), "a step's sums leave int64: the bound of dc_component_fields does not hold"
    return {"offsets": offsets, "ncycles": np.array([selected, need, stored, left], np.int64), "steps": to64(steps, (stored, STEP)),
            "step_fields": to64(sf, (stored, C, uef.STATS)), "track_fields": to64(life, (m, C, LIFE))}


def event_rows(masks, fields, connectivity, wrap, tables, cap, C, bits, store):
    """the field rows [n, C, 6] of the stored events (store [n, 12]: frame, rank, ...) by the loop of util_event_fields, frame by frame"""
    masks = np.asarray(masks, np.uint8)
    ftable, _ = uef.field_table(masks, len(masks), connectivity, wrap, *tables, cap, np.asarray(fields, np.float32), C, bits)
    out = np.empty((len(store), C, uef.STATS), np.int64)
    for e in range(len(store)):
        out[e] = ftable[int(store[e, 0]), int(store[e, 1])]
    return out


def reference(masks, fields, connectivity, wrap, tables, C, bits, cap=512, event_cap=8192, track_cap=None, min_pixels=0, cuts=(), step_cap=None,
              min_frames=1, class_mask=6):
    """the tracker's checker, the field rows and cycles() in one: the dict of util_tracks.track plus "frows" and the five tables"""
    trk = ut.track(masks, connectivity, wrap, *tables, cap=cap, event_cap=event_cap, track_cap=track_cap, min_pixels=min_pixels, cuts=cuts)
    trk["frows"] = event_rows(masks, fields, connectivity, wrap, tables, cap, C, bits, trk["store"])
    trk.update(cycles(trk["store"], trk["track_of"], trk["tracks"], trk["frows"], event_cap if step_cap is None else step_cap, min_frames,
                      class_mask))
    return trk


# ------------------------------------------------------------------------------------------------------------------ sequences
DRAWN = ("hold", "split_merge", "seam", "two_classes")
DRAWN_SHAPE, DRAWN_FRAMES = (16, 24), 6
RANDOM_CASES = {"small": (12, 16, 4, 11), "wide": (20, 27, 8, 12), "large": (32, 48, 12, 13)}     # H, W, frames, seed
MIN_FRAMES = 3                                     # what the selection tests filter with


def scale_bits(C):
    return [20 - (c % 4) for c in range(C)]


def _background(rs, T, H, W, C):
    """distinct values in (1, 2) + channel: nothing here ties with anything, and nothing is below 1"""
    f = 1.0 + rs.permutation(T * H * W * C).reshape(T, H, W, C).astype(np.float64) / (T * H * W * C) + np.arange(C)
    return f.astype(np.float32)


@functools.lru_cache(maxsize=None)
def drawn(name, C, ldc=None):
    """(masks uint8 [T, H, W], fields float32 [T, H, W, ldc]) of a drawn sequence; callers do not modify them.  Channels beyond C hold NaN."""
    (H, W), T = DRAWN_SHAPE, DRAWN_FRAMES
    ldc = C if ldc is None else ldc
    rs = np.random.RandomState(zlib.crc32(f"track fields {name} {C}".encode()))
    m = np.zeros((T, H, W), np.uint8)
    f = np.full((T, H, W, ldc), np.nan, np.float32)
    f[..., :C] = _background(rs, T, H, W, C)
    if name == "hold":                                   # a 4 x 5 blob, 2 columns per frame; its minimum -5 in frames 1 AND 2, its maximum 9 in 3 AND 4
        for t in range(T):
            m[t, 5:9, 2 + 2 * t:7 + 2 * t] = 1
        f[1, 7, 6, 0] = f[2, 6, 8, 0] = -5.0             # the later frame holds it at the SMALLER pixel: the frame decides first
        f[3, 8, 10, 0] = f[4, 5, 11, 0] = 9.0
        f[0, 0, 0, 0], f[5, 15, 23, 0] = -50.0, 50.0     # background pixels take no part
    elif name == "split_merge":                          # two blobs of class 2: apart, one for two frames, apart again
        gap = [4, 2, 0, 0, 2, 4]
        for t in range(T):
            m[t, 6:12, 3:9] = 2
            m[t, 6:12, 9 + gap[t]:15 + gap[t]] = 2
        for t in (0, 5):                                 # both fragments hold the extremes; the smaller pixel lies in the RIGHT one
            f[t, 9, 4, 0] = f[t, 7, 16, 0] = -7.0
            f[t, 10, 5, 0] = f[t, 8, 17, 0] = 11.0
    elif name == "seam":                                 # a blob across the periodic seam, one column per frame
        for t in range(T):
            for c in range(6):
                m[t, 4:9, (W - 4 + t + c) % W] = 1
        f[2, 6, W - 1, 0], f[3, 6, 0, 0] = -3.0, -4.0
    elif name == "two_classes":                          # a cyclone in frames 0 .. 3, a river in 2 .. 5 that then covers the cyclone's pixels
        for t in range(0, 4):
            m[t, 3:8, 3:9] = 1
        for t in range(2, 6):
            m[t, 3:8, 9:15] = 2
        m[4, 3:8, 3:9] = 2
    else:
        raise KeyError(name)
    m.setflags(write=False)
    f.setflags(write=False)
    return m, f


@functools.lru_cache(maxsize=None)
def random_sequence(case, C, ldc=None, special=False):
    """Masks that persist from frame to frame (long tracks, splits and merges), fields of few distinct values in channels 0, 3, 6, ... (ties
    inside a step, across fragments and across frames), continuous ones in 1, 4, ..., small integers in 2, 5, ...  special: NaN, +-Inf,
    values at and beyond the saturation limit of channel 0's scale, and a channel of -0.0 / +0.0."""
    H, W, T, seed = RANDOM_CASES[case]
    ldc = C if ldc is None else ldc
    rs = np.random.RandomState(seed)
    m = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        fresh = ((rs.rand(H, W) < 0.3) * rs.randint(1, 3, (H, W))).astype(np.uint8)
        m[t] = fresh if t == 0 else np.where(rs.rand(H, W) < 0.75, m[t - 1], fresh)
    f = np.full((T, H, W, ldc), np.nan, np.float32)
    for c in range(C):
        if c % 3 == 0:
            f[..., c] = rs.randint(-2, 3, (T, H, W)) * 0.25
        elif c % 3 == 1:
            f[..., c] = rs.randn(T, H, W) * 100.0
        else:
            f[..., c] = rs.randint(0, 3, (T, H, W))
    if special:
        pick = rs.rand(T, H, W)
        odd = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 20, 2.0 ** 21, -2.0 ** 20 - 1.0], np.float32)   # bits 20: 2^20 fits, 2^21 does not
        f[..., 0] = np.where(pick < 0.3, odd[rs.randint(0, len(odd), (T, H, W))], f[..., 0])
        if C > 1:
            f[..., C - 1] = np.where(rs.rand(T, H, W) < 0.5, np.float32(-0.0), np.float32(0.0))
        if C > 2:
            f[..., 1] = np.where(pick > 0.5, np.nan, f[..., 1])
            f[m == 2, 1] = np.nan                        # channel 1 of every river: empty rows, empty lifetime extremes
    m.setflags(write=False)
    f.setflags(write=False)
    return m, f
