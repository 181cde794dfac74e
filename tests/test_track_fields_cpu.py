"""The storm life cycles' host side (no GPU): the checker of tests/util_track_fields.py against a brute force that works from the frame
stack itself -- pixel by pixel into dictionaries keyed by (track, frame) --, the cases the GPU tests' sequences must contain,
nn.TrackFields.decode on hand-made rows, the host-only entry point and the argument checks of the C ABI, and the driver's flags and summary."""
import ctypes as C
import math

import numpy as np
import pytest

from mlperf_deepcam_amd import lib as L
from mlperf_deepcam_amd import nn as dnn
import util_event_fields as uef
import util_events as ue
import util_track_fields as uf
import util_tracks as ut

CAP, EVENT_CAP = 512, 8192


def _brute(masks, fields, conn, wrap, C_, bits, min_frames=1, class_mask=6, step_cap=EVENT_CAP):
    """Flood-fill every frame, link with util_tracks, then every foreground pixel on its own into its (track, frame): extremes as
    (key, pixel) tuples, sums of per-pixel quantised values.  Lifetime extremes come from the PIXELS, not from the steps.  Returns the five
    tables in the checker's form and what the sequence contains."""
    T, H, W = masks.shape
    tables = dnn.event_weight_tables(H, W)
    wy, cx, sx = (t.astype(np.int64).tolist() for t in tables)
    trk = ut.track(masks, conn, wrap, *tables, cap=CAP, event_cap=EVENT_CAP)
    n, first, track_of, tracks = len(trk["store"]), trk["first"], trk["track_of"], trk["tracks"]
    steps, sfield, life, ev_min = {}, {}, {}, {}
    for f in range(T):
        labels, rows = ue.label_one(masks[f], conn, wrap, *tables)
        rank = {int(r[0]): k for k, r in enumerate(rows)}
        v = np.asarray(fields[f], np.float32)[:, :, :C_]
        with np.errstate(over="ignore", invalid="ignore"):
            s = np.ldexp(v.astype(np.float64), np.asarray(bits, np.int32))
            q = np.rint(s)
            wq = np.rint(s * (np.asarray(wy, np.float64) * 2.0 ** -20)[:, None, None])
            fits = np.abs(q) <= uef.LIMIT
        for r in range(H):
            for c in range(W):
                if labels[r, c] <= 0:
                    continue
                k = rank[int(labels[r, c]) - 1]
                e = int(first[f]) + k
                if k >= CAP or e >= n or track_of[e] < 0:
                    continue
                t, p = int(track_of[e]), r * W + c
                st = steps.setdefault((t, f), {"events": set(), "sums": [0, 0, 0, 0, 0]})
                st["events"].add(e)
                for i, add in enumerate((1, wy[r], r, cx[c], sx[c])):
                    st["sums"][i] += add
                for ch in range(C_):
                    a = sfield.setdefault((t, f, ch), {"lo": None, "hi": None, "acc": [0, 0, 0, 0]})
                    if not np.isfinite(v[r, c, ch]):
                        a["acc"][2] += 1
                        continue
                    key = uef.key(v[r, c, ch])
                    a["lo"] = min(a["lo"], (key, p)) if a["lo"] else (key, p)
                    a["hi"] = max(a["hi"], (key, -p)) if a["hi"] else (key, -p)
                    ev_min[(e, ch)] = min(ev_min.get((e, ch), key), key)
                    b = life.setdefault((t, ch), {"lo": (key, f, p), "hi": (key, -f, -p)})
                    b["lo"], b["hi"] = min(b["lo"], (key, f, p)), max(b["hi"], (key, -f, -p))
                    if not fits[r, c, ch]:
                        a["acc"][3] += 1
                        continue
                    a["acc"][0] += int(q[r, c, ch])
                    a["acc"][1] += int(wq[r, c, ch])
    # the layout, by the issue's words: selected rows in row order, stored while they end inside step_cap
    m = len(tracks)
    offsets, need, sel, left = np.full(m, -1, np.int64), 0, 0, 0
    for t in range(m):
        frames = int(tracks[t, 4] - tracks[t, 3]) + 1
        if frames >= max(min_frames, 1) and (class_mask >> int(tracks[t, 1])) & 1:
            sel += 1
            if need + frames <= step_cap:
                offsets[t] = need
            else:
                offsets[t], left = -2, left + 1
            need += frames
    stored = int(sum(tracks[t, 4] - tracks[t, 3] + 1 for t in range(m) if offsets[t] >= 0))
    out_steps = np.zeros((stored, 8), np.int64)
    out_sf = np.zeros((stored, C_, 6), np.int64)
    out_sf[:] = uef.EMPTY_ROW
    out_life = np.zeros((m, C_, 4), np.int64)
    out_life[:] = (-1, -1, 0, -1)
    for (t, f), st in steps.items():
        if offsets[t] < 0:
            continue
        row = int(offsets[t]) + f - int(tracks[t, 3])
        out_steps[row] = [t, f, len(st["events"])] + st["sums"]
        for ch in range(C_):
            a = sfield[(t, f, ch)]
            if a["lo"]:
                out_sf[row, ch, 0] = uef.signed((a["lo"][0] << 32) | a["lo"][1])
                out_sf[row, ch, 1] = uef.signed((a["hi"][0] << 32) | (0xFFFFFFFF + a["hi"][1]))
            out_sf[row, ch, 2:] = a["acc"]
    for (t, ch), b in life.items():
        if offsets[t] >= 0:
            out_life[t, ch] = [uef.signed((b["lo"][0] << 32) | b["lo"][1]), b["lo"][2], uef.signed((b["hi"][0] << 32) | (0xFFFFFFFF + b["hi"][1])),
                               -b["hi"][2]]
    # what the sequence contains
    has = {"multi_event_step": any(len(st["events"]) >= 2 for st in steps.values()), "extreme_in_two_frames": False,
           "extreme_in_two_fragments": False, "filtered": False, "tracks": m}
    for (t, ch), b in life.items():
        frames = [f for f in range(int(tracks[t, 3]), int(tracks[t, 4]) + 1) if sfield[(t, f, ch)]["lo"] and sfield[(t, f, ch)]["lo"][0] == b["lo"][0]]
        has["extreme_in_two_frames"] |= len(frames) >= 2
    for (t, f), st in steps.items():
        for ch in range(C_):
            a = sfield[(t, f, ch)]
            if a["lo"] and sum(1 for e in st["events"] if ev_min.get((e, ch)) == a["lo"][0]) >= 2:
                has["extreme_in_two_fragments"] = True
    frames = tracks[:, 4] - tracks[:, 3] + 1
    has["filtered"] = bool((frames < uf.MIN_FRAMES).any() and (frames >= uf.MIN_FRAMES).any())
    return {"offsets": offsets, "ncycles": np.array([sel, need, stored, left], np.int64), "steps": out_steps, "step_fields": out_sf,
            "track_fields": out_life}, has


def _check(masks, fields, conn, wrap, C_, **kw):
    H, W = masks.shape[1:]
    bits = uf.scale_bits(C_)
    ref = uf.reference(masks, fields, conn, wrap, dnn.event_weight_tables(H, W), C_, bits, cap=CAP, event_cap=EVENT_CAP,
                       step_cap=kw.get("step_cap", EVENT_CAP), min_frames=kw.get("min_frames", 1), class_mask=kw.get("class_mask", 6))
    brute, has = _brute(masks, fields, conn, wrap, C_, bits, **kw)
    for key in ("ncycles", "offsets", "steps", "step_fields", "track_fields"):
        assert ref[key].shape == brute[key].shape and np.array_equal(ref[key], brute[key]), key
    return ref, has


@pytest.mark.parametrize("name", uf.DRAWN)
def test_checker_agrees_with_the_brute_force_on_the_drawn_sequences(name):
    masks, fields = uf.drawn(name, 3)
    ref, has = _check(masks, fields, 8, True, 3)
    tr, life, W = ref["tracks"], ref["track_fields"], masks.shape[2]
    word = lambda v, f: uef.signed((uef.key(v) << 32) | f)  # noqa: E731
    if name == "hold":                                   # one track; the earliest of two frames wins although the later pixel is smaller
        assert len(tr) == 1 and has["extreme_in_two_frames"]
        assert life[0, 0].tolist() == [word(-5.0, 1), 7 * W + 6, word(9.0, 0xFFFFFFFF - 3), 8 * W + 10]
    elif name == "split_merge":                          # frame 0 is a step of two fragments, both with the extremes: the smaller pixel
        assert len(tr) == 1 and has["multi_event_step"] and has["extreme_in_two_fragments"]
        assert ref["steps"][0, :3].tolist() == [0, 0, 2] and ref["steps"][2, :3].tolist() == [0, 2, 1]
        assert ref["step_fields"][0, 0, :2].tolist() == [uef.signed((uef.key(-7.0) << 32) | (7 * W + 16)),
                                                         uef.signed((uef.key(11.0) << 32) | (0xFFFFFFFF - (8 * W + 17)))]
        assert life[0, 0].tolist() == [word(-7.0, 0), 7 * W + 16, word(11.0, 0xFFFFFFFF), 8 * W + 17]
    elif name == "seam":
        assert len(tr) == 1 and (ref["store"][:, 11] == 1).any() and life[0, 0, :2].tolist() == [word(-4.0, 3), 6 * W]
    else:                                                # a cyclone and a river: overlapping in time, the same pixels later, never joined
        assert tr[:, [1, 3, 4]].tolist() == [[1, 0, 3], [2, 2, 5]] and ref["offsets"].tolist() == [0, 4]
        only, _ = _check(masks, fields, 8, True, 3, class_mask=2)
        assert only["offsets"].tolist() == [0, -1] and only["ncycles"].tolist() == [1, 4, 4, 0]


@pytest.mark.parametrize("case", list(uf.RANDOM_CASES))
def test_checker_agrees_with_the_brute_force_on_the_random_sequences(case):
    C_ = {"small": 1, "wide": 3, "large": 3}[case]
    masks, fields = uf.random_sequence(case, C_)
    ref, has = _check(masks, fields, 4, True, C_)
    if case != "small":                                  # what a GPU test on these frames must meet
        assert has["multi_event_step"] and has["extreme_in_two_frames"] and has["extreme_in_two_fragments"] and has["filtered"], has
    if case == "large":
        assert has["tracks"] > 256 and len(ref["store"]) * 16 > 4096, "one workgroup ranks all track rows: the chunked scan is not exercised"
    sel, _ = _check(masks, fields, 4, True, C_, min_frames=uf.MIN_FRAMES, class_mask=4)
    assert 0 < sel["ncycles"][0] < ref["ncycles"][0] and (sel["offsets"] == -1).any()
    cut = int(ref["ncycles"][1]) // 2
    part, _ = _check(masks, fields, 4, True, C_, step_cap=cut)
    assert part["ncycles"][2] <= cut < part["ncycles"][1] and part["ncycles"][3] > 0 and (part["offsets"] == -2).any()
    stored = part["offsets"] >= 0
    assert np.array_equal(part["offsets"][stored], ref["offsets"][stored]) and np.array_equal(part["steps"], ref["steps"][:len(part["steps"])])


def test_special_values_reach_the_checker():
    masks, fields = uf.random_sequence("wide", 3, special=True)
    ref, _ = _check(masks, fields, 8, True, 3)
    sf = ref["step_fields"]
    assert (sf[:, 0, 4] > 0).any() and (sf[:, 0, 5] > 0).any()                      # non-finite and saturated values were met
    river = ref["tracks"][ref["steps"][:, 0], 1] == 2
    assert river.any() and (sf[river, 1, 0] == -1).all() and (sf[river, 1, 1] == 0).all()
    assert (ref["track_fields"][ref["tracks"][:, 1] == 2, 1] == [-1, -1, 0, -1]).all()
    zero = ref["track_fields"][:, 2]                     # the channel of signed zeros: -0.0 is the minimum, +0.0 the maximum
    both = (zero[:, 0] >> 32 == uef.key(-0.0)) & (zero[:, 2] >> 32 == uef.key(0.0) - (1 << 32))   # int64 words: the second is negative
    assert both.any()


def _hand_made():
    """One cyclone on an 8 x 16 grid: two fragments in frame 2, one event in frame 3; channel 1 holds no finite value at all."""
    H, W, bits = 8, 16, [10, 12]
    wy, cx, sx = (t.astype(np.int64) for t in dnn.event_weight_tables(H, W))

    def event(frame, rank, pix, vals):
        r, c = np.array([p // W for p in pix]), np.array([p % W for p in pix])
        row = [frame, rank, min(pix), 1, len(pix), int(wy[r].sum()), int(r.sum()), int(cx[c].sum()), int(sx[c].sum()), int(r.min()), int(r.max()), 0]
        lo = min((uef.key(v) << 32) | p for p, v in zip(pix, vals))
        hi = max((uef.key(v) << 32) | (0xFFFFFFFF - p) for p, v in zip(pix, vals))
        q = [int(np.rint(np.ldexp(np.float64(np.float32(v)), bits[0]))) for v in vals]
        wq = [int(np.rint(np.ldexp(np.float64(np.float32(v)), bits[0]) * (float(wy[p // W]) * 2.0 ** -20))) for p, v in zip(pix, vals)]
        return row, [[uef.signed(lo), uef.signed(hi), sum(q), sum(wq), 0, 0], [-1, 0, 0, 0, len(pix), 0]]

    ev = [event(2, 0, [2 * W + 3, 2 * W + 4], [-2.5, 1.0]), event(2, 1, [5 * W + 9, 5 * W + 10, 6 * W + 9], [3.0, -2.5, 0.5]),
          event(3, 0, [3 * W + 4, 3 * W + 5, 4 * W + 5, 4 * W + 6], [-1.0, 3.0, 0.25, 2.0])]
    store = np.array([e[0] for e in ev], np.int64)
    frows = np.array([e[1] for e in ev], np.int64)
    tracks = np.array([[0, 1, 3, 2, 3, 9, (4 << 32) | (0xFFFFFFFF - 3), int(store[:, 5].sum())]], np.int64)
    return H, W, bits, store, frows, tracks


def test_decode_on_hand_made_rows():
    H, W, bits, store, frows, tracks = _hand_made()
    lat, lon = np.linspace(-90.0, 90.0, H), np.linspace(-180.0, 180.0, W)
    c = uf.cycles(store, np.zeros(3, np.int32), tracks, frows, step_cap=8)
    assert c["ncycles"].tolist() == [1, 2, 2, 0] and c["steps"][:, :4].tolist() == [[0, 2, 2, 5], [0, 3, 1, 4]]
    args = (tracks, c["offsets"], c["steps"], c["step_fields"], c["track_fields"], H, W, bits)
    (cyc,) = dnn.TrackFields.decode(*args, center_channel=0)
    plain = dnn.EventTracker.decode(store, np.zeros(3, np.int32), tracks, H, W)[0]
    for key in ("id", "class", "first_frame", "last_frame", "frames", "events", "pixels", "peak_pixels", "peak_frame", "area_fraction_sum"):
        assert cyc[key] == plain[key], key
    # the two-fragment step: the joint centroid (the tracker's path), the extremes of both fragments, the smallest pixel among equals
    s0, s1 = cyc["series"]
    assert {k: s0[k] for k in plain["path"][0]} == plain["path"][0] and {k: s1[k] for k in plain["path"][1]} == plain["path"][1]
    assert s0["events"] == 2 and s0["pixels"] == 5 and s0["lat"] == -90.0 + 180.0 * ((2 + 2 + 5 + 5 + 6) / 5) / (H - 1)
    f0 = s0["fields"][0]
    assert (f0["min"], f0["min_row"], f0["min_col"], f0["max"], f0["max_row"], f0["max_col"]) == (-2.5, 2, 3, 3.0, 5, 9)
    assert f0["mean"] == (-2.5 + 1.0 + 3.0 - 2.5 + 0.5) / 5 and (s0["center_lat"], s0["center_lon"]) == (float(lat[2]), float(lon[3]))
    assert (s1["center_lat"], s1["center_lon"]) == (float(lat[3]), float(lon[4])) and s1["fields"][0]["max"] == 3.0
    # a merged row decodes as an event's row does: to the bit what EventFields.values gives for it
    pseudo = np.zeros((2, 10), np.int64)
    pseudo[:, 2:7] = c["steps"][:, 3:8]
    vals = dnn.EventFields.values(c["step_fields"], pseudo, H, W, bits)
    assert np.array_equal(uef.values_from_decode([s0["fields"], s1["fields"]], 2), vals, equal_nan=True)
    # the empty channel: no extremes, no means, and the centre of a step without a finite value is None
    assert all(s["fields"][1][k] is None for s in (s0, s1) for k in ("min", "min_lat", "max", "max_lon", "mean"))
    assert s0["fields"][1]["nonfinite"] == 5
    (other,) = dnn.TrackFields.decode(*args, center_channel=1)
    assert other["series"][0]["center_lat"] is None and other["series"][1]["center_lon"] is None
    assert "center_lat" not in dnn.TrackFields.decode(*args)[0]["series"][0]
    # lifetime: -2.5 and 3.0 both occur in frame 2 first; the mean over all nine pixels from the summed step sums
    life = cyc["fields"][0]
    assert (life["min"], life["min_frame"], life["min_row"], life["min_col"]) == (-2.5, 2, 2, 3)
    assert (life["max"], life["max_frame"], life["max_row"], life["max_col"]) == (3.0, 2, 5, 9)
    assert (life["min_lat"], life["min_lon"], life["max_lat"], life["max_lon"]) == (float(lat[2]), float(lon[3]), float(lat[5]), float(lon[9]))
    total = int(c["step_fields"][:, 0, 2].sum())
    assert life["mean"] == math.ldexp(float(total), -bits[0]) / 9 == (-2.5 + 1.0 + 3.0 - 2.5 + 0.5 - 1.0 + 3.0 + 0.25 + 2.0) / 9
    assert cyc["fields"][1] == {"nonfinite": 9, "saturated": 0, "mean": None, **{f"{n}{k}": None for n in ("min", "max")
                                                                                for k in ("", "_frame", "_row", "_col", "_lat", "_lon")}}
    # tracks that are not stored are left out; a bad centre channel raises
    none = uf.cycles(store, np.zeros(3, np.int32), tracks, frows, step_cap=1)
    assert none["offsets"].tolist() == [-2] and none["ncycles"].tolist() == [1, 2, 0, 1] and (none["track_fields"] == [-1, -1, 0, -1]).all()
    assert dnn.TrackFields.decode(tracks, none["offsets"], none["steps"], none["step_fields"], none["track_fields"], H, W, bits) == []
    with pytest.raises(L.DeepcamHipError, match="center_channel"):
        dnn.TrackFields.decode(*args, center_channel=2)


def test_the_checker_refuses_a_track_with_a_gap():
    H, W, bits, store, frows, tracks = _hand_made()
    store = store.copy()
    store[2, 0] = 4
    gap = tracks.copy()
    gap[0, 4] = 4
    with pytest.raises(AssertionError, match="interval"):
        uf.cycles(store, np.zeros(3, np.int32), gap, frows, step_cap=8)


def test_host_entry_point_and_argument_checks_without_a_device():
    lib = L.load()
    assert lib.dc_track_cycles_workspace(1 << 19, 1 << 19) == 2048 * 16 + 2048 * 8
    assert lib.dc_track_cycles_workspace(16, 1) == 512 and lib.dc_track_cycles_workspace(1024, 257) == 2 * 256
    for bad in ((0, 1), ((1 << 30) + 1, 1), (16, 0), (16, 17)):
        assert lib.dc_track_cycles_workspace(*bad) == 0
    fake = C.c_void_p(4096)                                                        # never dereferenced: the checks come before any launch
    ap = lambda **kw: lib.dc_track_fields_append(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("B", 2), ("nv", 2), ("cap", 4), ("ncomp", fake), ("first", fake), ("ftable", fake), ("C", 3), ("event_cap", 16), ("fstore", fake),
        ("st", None))])
    assert ap(nv=0) != 0 and "n_valid" in L.last_error()
    assert ap(nv=3) != 0
    assert ap(cap=0) != 0 and "cap" in L.last_error()
    assert ap(C=0) != 0 and "C must" in L.last_error()
    assert ap(C=33) != 0 and "C must" in L.last_error()
    assert ap(event_cap=0) != 0 and "event_cap" in L.last_error()
    assert ap(first=None) != 0 and "null" in L.last_error()
    assert ap(fstore=C.c_void_p(4104)) != 0 and "aligned" in L.last_error()
    cy = lambda **kw: lib.dc_track_cycles(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("event_cap", 16), ("track_cap", 16), ("step_cap", 16), ("C", 3), ("min_frames", 1), ("class_mask", 6), ("state", fake), ("store", fake),
        ("track_of", fake), ("tracks", fake), ("ntracks", fake), ("fstore", fake), ("offsets", fake), ("steps", fake), ("step_fields", fake),
        ("track_fields", fake), ("ncycles", fake), ("ws", fake), ("st", None))])
    assert cy(event_cap=0) != 0 and "event_cap" in L.last_error()
    assert cy(track_cap=17) != 0 and "track_cap" in L.last_error()
    assert cy(step_cap=0) != 0 and "step_cap" in L.last_error()
    assert cy(C=0) != 0 and cy(C=33) != 0 and "C must" in L.last_error()
    assert cy(min_frames=-1) != 0 and "min_frames" in L.last_error()
    assert cy(class_mask=0) != 0 and cy(class_mask=7) != 0 and "class_mask" in L.last_error()
    assert cy(ncycles=None) != 0 and "null" in L.last_error()
    assert cy(steps=C.c_void_p(4104)) != 0 and "aligned" in L.last_error()
    assert cy(ws=C.c_void_p(4112)) != 0 and "aligned" in L.last_error()


def test_the_new_calls_are_bound():
    for name in ("dc_track_fields_append", "dc_track_cycles", "dc_track_cycles_workspace"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert len(L._SIGS["dc_track_fields_append"][1]) == 10 and len(L._SIGS["dc_track_cycles"][1]) == 19
    assert len(dnn.TRACK_STEP_FIELDS) == uf.STEP and len(dnn.TRACK_FIELD_STATS) == uf.LIFE
    assert dnn.TRACK_STEP_FIELDS[3:] == dnn.EVENT_FIELDS[2:7]


def test_driver_track_fields_implies_tracks_and_event_fields():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "c", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.track_fields is False and a.tracks is False and a.event_fields is False and a.track_center_channel is None
    a = predict.build_parser().parse_args(base + ["--track_fields"])
    assert a.track_fields is True and a.tracks is True and a.event_fields is True and a.events is True and a.track_center_channel is None
    a = predict.build_parser().parse_args(base + ["--track_fields", "--track_center_channel", "5", "--min_track_frames", "2"])
    assert a.track_center_channel == 5 and a.min_track_frames == 2
    a = predict.build_parser().parse_args(base + ["--tracks", "--event_fields"])
    assert a.track_fields is False
    assert "life cycles" in predict.build_parser().format_help()


def test_driver_summary_of_track_fields():
    from mlperf_deepcam_amd import predict
    H, W = 8, 16
    tracks = np.array([[0, 1, 4, 0, 2, 7, 0, 0], [1, 2, 1, 0, 0, 1, 0, 0], [5, 1, 3, 1, 3, 9, 0, 0], [9, 1, 1, 4, 4, 2, 0, 0]], np.int64)
    word = lambda v, f: uef.signed((uef.key(v) << 32) | f)  # noqa: E731
    life = np.zeros((4, 2, 4), np.int64)
    life[:] = (-1, -1, 0, -1)
    life[0, 1, :2] = [word(990.5, 1), 3 * W + 2]
    life[1, 1, :2] = [word(900.0, 0), 5]                 # a river: deeper, but not class 1
    life[2, 1, :2] = [word(951.25, 3), 6 * W + 15]
    life[3, 1, :2] = [word(940.0, 4), 7]                 # deeper still, but its track is not stored
    rows = {"counts": np.array([4, 9, 8, 1], np.int64), "tracks": tracks, "offsets": np.array([0, 3, 4, -2], np.int64), "track_fields": life}
    s = predict.track_fields_summary(rows, H, W, center_channel=1)
    assert s == {"tracks_selected": 4, "steps_needed": 9, "steps_stored": 8, "tracks_not_stored": 1, "class_1": 2, "class_2": 1,
                 "center_channel": 1, "deepest_class_1": {"id": 5, "value": 951.25, "frame": 3, "lat": float(np.linspace(-90, 90, H)[6]),
                                                          "lon": float(np.linspace(-180, 180, W)[15])}}
    s = predict.track_fields_summary(rows, H, W)
    assert "deepest_class_1" not in s and s["class_1"] == 2
    assert predict.track_fields_summary(rows, H, W, center_channel=0)["deepest_class_1"] is None
