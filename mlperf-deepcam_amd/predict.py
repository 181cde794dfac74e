"""Inference driver: a checkpoint and a directory of unlabelled CAM5 files in, one mask file per input file out.

    python -m mlperf_deepcam_amd.predict --checkpoint model_step_1000.cpt --data_dir /data/unlabelled --stats_file /data/stats.h5 \
        --output_dir /data/masks --batch_size 8 --dtype bf16 --confidence

What the reference offers for this is its validation loop's ``net.eval(); torch.max(net(x), 1)[1]`` (train_hdf5_ddp.py:452-458), which
needs labelled files.  Here the files need no ``climate/labels_0`` (data.CamDataset(labels=False)); the batches run through nn.Predictor
(forward-only engine, the class map written by the classifier's kernel as one byte per pixel); the masks leave the device through two
pinned host buffers, and a writer thread stores them while the device works on the next batch.  Every output file carries the base name
of its input file and holds ``prediction`` (uint8 [H, W]: 0 background, 1 tropical cyclone, 2 atmospheric river) and, with --confidence,
``confidence`` (float32 [H, W]: the predicted class's softmax probability).  ``summary.json`` lists the class pixel counts and the mean
confidence per file.  With --events every output file also carries ``events`` (int64 [n, 10], the raw rows of nn.EventCatalog: root,
class, pixels, area, sum of rows, sum of cx, sum of sx, first row, last row, seam flag -- connected components of the mask, found on the
device; the table, not a label map, is what crosses to the host), and ``summary.json`` the number of class-1 and class-2 events per file
and in total and the number of files whose table overflowed.  With --verify (which implies --events) the files must be labelled: the
masks and the labels go through nn.EventMatcher (a = prediction, b = labels), every output file also carries ``truth_events`` (int64
[m, 10], the label side's rows), ``matches`` (int64 [p, 3]: row of ``events``, row of ``truth_events``, shared pixels; sorted) and
``event_scores`` (int64 [2, 4], per class: hits, misses, false alarms, matched detections), and ``summary.json`` and the final line
gain ``event_verification`` (hits, misses, false alarms, POD, FAR and CSI per class over all files).  With --event_fields (which
implies --events) nn.EventFields reduces the raw fields of every batch per event on the device, behind the catalogue: every output file
also carries ``event_fields`` (int64 [n, C, 6] over all C file channels: min, max, sum, wsum, nonfinite, saturated -- the rows of
``events``, in their order), ``event_field_values`` (float64 [n, C, 8]: min, its lat and lon, max, its lat and lon, mean, area-weighted
mean; NaN where there is none) and ``event_field_bits`` (int32 [C], the sums' binary scale from the stats file's range), and
``summary.json`` gains ``event_fields`` (channels, scale_bits, and the non-finite and saturated values met over all stored events).
With --plots nn.FrameRenderer draws, on the device, what the reference's visualiser draws on the host: channel --plot_channel of the raw
fields through a colour table, the predicted cyclones and rivers outlined, and with --verify a second panel below it with the labelled
ones; ``<output_dir>/plots/<base>.png`` is written for every --plot_every-th input file (in the order of the file names) and
``summary.json`` gains ``plots`` (their number).  Only the RGB bytes cross to the host; the writer thread encodes them (png.py).
With --tracks (which implies --events) nn.EventTracker links the events of consecutive files on the device, behind the catalogue of every
batch: the sorted files are taken as ONE gap-free time sequence, file index = frame number (gaps in the dates or interleaved runs are
not detected from the names).  At the end of the run ``<output_dir>/tracks.h5`` holds ``tracks`` (int64 [n, 8]: id, class, events, first
frame, last frame, pixels, peak, area), ``track_events`` (int64 [m, 13]: frame, rank, the ten columns of ``events``, the row of
``tracks`` or -1 -- with --min_event_pixels 0, (frame, rank) is row `rank` of the ``events`` and ``event_fields`` of file `frame`) and
``track_state`` (int64 [4]: events stored, frames, events dropped, frames with a truncated catalogue); ``summary.json`` gains ``tracks``.
With --verify_tracks (which implies --verify and --tracks) a second nn.EventTracker runs on the labels' events and nn.TrackMatcher files,
behind every batch and on the device, every overlap of a predicted and a labelled event under the two events' tracks.  ``tracks.h5``
additionally holds ``truth_tracks``, ``truth_track_events``, ``truth_track_state`` (the labels' side of the three datasets above),
``track_pairs`` (int64 [p, 8]: row of ``tracks``, row of ``truth_tracks``, class, overlaps, distinct common frames, shared pixels, first
and last common frame), ``track_cover`` and ``truth_track_cover`` (int64 [n, 2] per side: matched frames, shared pixels),
``track_scores`` (int64 [2, 4]: per class hits, misses, false alarms, matched detections of tracks) and ``track_match_state`` (int64
[4]: links stored, links dropped, frames filed, frames truncated); ``summary.json`` gains ``track_verification`` (the counters, POD,
FAR and CSI of tracks per class, the mean
genesis and lysis errors and the mean separation of the paths over each found storm's best partner, the partners per found storm).
With --track_fields (which implies --tracks and --event_fields) nn.TrackFields files the field rows of every batch next to the tracker's
store and joins the two on the device at the end of the run -- the storm life cycles: ``tracks.h5`` additionally holds
``track_step_offsets`` (int64 [n]: per row of ``tracks`` the first of its step rows, -1 not selected by --min_track_frames, -2 beyond the
step table), ``track_steps`` (int64 [s, 8]: row of ``tracks``, frame, events, and the summed pixels, area, sum of rows, sum of cx, sum of sx
of the track's events in that frame), ``track_step_fields`` (int64 [s, C, 6]: their ``event_fields`` rows merged), ``track_fields`` (int64
[n, C, 4]: per channel the lifetime minimum as (key << 32) | frame and its pixel, the maximum as (key << 32) | (0xFFFFFFFF - frame) and its
pixel) and ``track_cycle_counts`` (int64 [4]: tracks selected, step rows needed, step rows stored, tracks left out); ``summary.json`` gains
``track_fields`` (the counters, the cycles per class and, with --track_center_channel C, the deepest minimum of channel C over the
class-1 tracks with its track id, frame, lat and lon -- for sea-level pressure the strongest cyclone of the run).
With --climatology nn.Climatology accumulates, behind every batch and on the device, the maps over time: per group (--climatology_by all,
month or season, from the first YYYY-MM-DD in a file's name) how often every pixel was predicted class 1 / class 2 and, per file channel
of --climatology_channels, the sum and number of its values over all frames, the class-1 frames and the class-2 frames of the pixel.  At
the end of the run ``<output_dir>/climatology.h5`` holds the raw integers ``frames`` (int64 [G]), ``count`` (int32 [G, 2, H, W]), ``sum``
(int64 [G, 3, H, W, C]), ``n`` (int32 [G, 3, H, W, C]), ``bits`` and ``channels`` (int32 [C]) -- the datasets of two runs add exactly, and
nn.Climatology.decode turns them into frequencies, means and shares --, with --verify also ``truth_count``, ``truth_sum``, ``truth_n`` of
the files' labels; ``summary.json`` gains ``climatology`` (the groups, their frames, the area-weighted frequency per class and group).
With --plots ``plots/climatology-<group>-class<k>.png`` shows, for every group that received a frame, the frequency of class k across
[0, 1] with the region of frequency >= --climatology_contour outlined (with --verify above the same picture of the labels).
With --event_shape (which implies --events) nn.EventShape adds the geometry of every event, behind the catalogue: every output file also
carries ``event_shape`` (int64 [n, 12]: boundary pixels, the two face counts and the nine moment sums -- the rows of ``events``, in their
order), ``event_shape_values`` (float64 [n, 10]: lat, lon, length_km, width_km, aspect, orientation_deg, perimeter_km, area_km2,
compactness, boundary_pixels) and ``event_shape_value_names`` (uint8: that column order, comma-separated ASCII).
With --event_filter nn.EventFilter drops, on the device, the events of the classifier's mask that miss the --filter_min_pixels,
--filter_min_area_km2, --filter_min_length_km or --filter_min_aspect of their class (two values each: class 1, class 2; 0: off).
``prediction`` stays the classifier's mask, ``prediction_filtered`` is added, and EVERYTHING downstream takes the filtered mask: the
catalogue behind ``events`` (a second one: the filter's own runs on the raw mask), --verify's prediction side, --event_fields, --tracks,
--track_fields, --climatology and --plots.  The labels under --verify are not filtered.  ``summary.json`` gains ``event_filter`` (the
thresholds and per class the events and pixels kept and dropped).
With --composites (which implies --event_fields) nn.StormComposite accumulates, behind every batch and on the device, the fields in storm
coordinates: around the --composite_center_stat (min or max) pixel of file channel --composite_center_channel of every event of the
--composite_classes with at least --composite_min_pixels pixels, a window of 2 * --composite_radius + 1 grid pixels a side of the
--composite_channels (all file channels by default), southern storms reflected so that "up" is poleward (--composite_no_flip: as they
lie; --composite_negate: the channels whose sign the reflection reverses, the meridional winds), per group (--composite_by) and per bin
of the centre value between the --composite_intensity_edges, with the sums per distance bin (--composite_bins bins of
--composite_bin_km).  At the end ``<output_dir>/composites.h5`` holds the raw integers ``events``, ``sum``, ``n``, ``inside``, ``rsum``,
``rn``, ``counts`` (int64 [5]: composited, no_center, below_min_pixels, other_class, uncatalogued), ``bits``, ``channels``, ``edges``,
``group_names`` (uint8: comma-separated ASCII) and the decoded ``mean``, ``footprint``, ``radial_mean``, ``radius_km``,
``radius_of_max_km``; ``summary.json`` gains ``composites``.  The catalogue is the one the other event products use: under --event_filter
the filtered one.
With --fss (which implies --verify) nn.FractionsSkill scores, behind every batch and on the device, the prediction side of --verify (the
filtered mask under --event_filter) against the unfiltered labels by neighbourhood: per class and window of --fss_windows grid pixels a
side (odd; columns periodic unless --fss_no_wrap; centres in the rows --fss_rows I0 I1, the whole frame by default) the integers sum (F -
O)^2, sum F^2, sum O^2 of the window counts F and O.  Every output file also carries ``fss`` (int64 [2, S, 3]) and ``fss_pixels`` (int64
[2, 2]: predicted and labelled pixels per class in those rows); ``summary.json`` gains ``fss`` (windows, rows, frames and per class the
pooled Fractions Skill Score 1 - sum A / (sum B + sum C) per window, the labels' base rate, the useful score 0.5 + base_rate / 2, the
smallest window that reaches it, and the raw totals as integers).
With --distance_skill (which implies --verify) nn.DistanceSkill scores, behind every batch and on the device, the same prediction side
against the unfiltered labels by distance: capped squared Euclidean distance maps in grid pixels (cap --distance_radius; columns periodic
unless --distance_no_wrap; sources in the rows --distance_rows I0 I1, the whole frame by default; no latitude weighting) and from them, per
class and direction (miss, false alarm), the sources per ring of distance with the sums of the distance and of its square, and Baddeley's
sum.  Every output file also carries ``distance`` (int64 [2, 2, R + 4]) and ``distance_baddeley`` (int64 [2]); ``summary.json`` gains
``distance_skill`` (radius, wrap, rows, frames and per class the mean error distances, the Hausdorff and partial Hausdorff distance,
Baddeley's Delta, the hit rate and success ratio within r pixels, and the raw totals as integers).
With --displacement (which implies --verify) nn.DisplacementSkill scores, behind every batch and on the device, the same prediction side
against the unfiltered labels by displacement: per class the overlap with the prediction moved by every (dy, dx) within
--displacement_radius rows and columns (columns periodic, rows never; label rows --displacement_rows I0 I1, the whole frame by default) and
the shift with the most hits.  Every output file also carries ``displacement`` (int64 [2, 2 R + 1, 2 R + 2]: the hits per shift, the last
cell of a row the predicted pixels that dy keeps in the band), ``displacement_pixels`` (int64 [2, 2]) and ``displacement_best`` (int64
[2, 4]: dy, dx, hits, kept); ``summary.json`` gains ``displacement`` (radius, rows, frames, per class the pooled decode -- one common
shift for all frames, the scores without and with it, the CRA decomposition -- and the means of the per-frame best shifts).
With --scale_skill (which implies --verify) nn.ScaleSkill scores, behind every batch and on the device, the same prediction side against
the unfiltered labels by spatial scale: per class, column origin of the dyadic grid (--scale_origins, 0 by default) and level j = 0 ..
--scale_levels (by default the largest whose tile 2^L divides the scored rows and the width) the sums (A, B, C) over the blocks of side
2^j grid pixels of the rows --scale_rows I0 I1 (the whole frame by default).  Every output file also carries ``scale`` (int64 [2, O,
L + 1, 3]) and ``scale_pixels`` (int64 [2, 2]); ``summary.json`` gains ``scale_skill`` (levels, origins, rows, frames and per class the
pooled decode: squared error, skill and energies per Haar component of scale 1, 2, ..., 2^L pixels).
With --prob_skill (which implies --verify) nn.ProbabilitySkill scores, behind every batch and on the device, the classifier's softmax
probabilities -- the stored fp32 logits, never the mask, so --event_filter does not change them -- against the unfiltered labels: per
class the joint histogram of (probability bin of --prob_bins bins, label is the class) with the sum of the probabilities per cell, and the
sum of squared errors, as integers (q = rint(p * 65536)).  Every output file also carries ``brier`` (float64 [3], NaN where no pixel was
scored) and ``prob_pixels`` (int64 [3]: scored, label outside [0, 3), a logit not finite); ``<output_dir>/prob_skill.h5`` holds the raw
integers ``hist``, ``sq_words``, ``pixels``, ``frames``, ``bins`` and the decoded curves per class (reliability diagram, sharpness, POD /
POFD / CSI / bias per threshold, and ``scalars`` named by ``scalar_names``); ``summary.json`` gains ``prob_skill`` (per class brier,
brier_skill, reliability, resolution, ece, auc, best_csi_threshold, base_rate).
With --decision_low TC AR (probabilities of class 1 and class 2), or --decision_from FILE (the prob_skill.h5 of an earlier run, typically
of the validation split: the best-CSI threshold per class), nn.DecisionRule turns the stored fp32 logits into a second mask on the device:
class c where its softmax probability reaches the threshold, of two the more probable one -- instead of the argmax, which the training's
class weights bias on purpose.  --decision_high TC AR adds hysteresis: a connected region above the low threshold (--event_connectivity,
periodic columns) is kept only if it holds a pixel above the high one.  ``prediction`` stays the argmax mask, every output file gains
``prediction_decided`` (uint8 [H, W]) and ``decision`` (int64 [12], nn.DECISION_COUNTS), and EVERYTHING downstream takes the decided mask:
--event_filter (which then filters it), --events, --verify, --fss and the rest; --prob_skill keeps scoring the probabilities.
``summary.json`` gains ``decision`` (the thresholds as q and as probabilities, the connectivity, the counters' totals).
With --ensemble_rolls S [S ...] and / or --ensemble_flip_lat, nn.ViewEnsemble pools the forecasts of several views of every batch on the
device (test-time augmentation): the network pads the first and the last column with zeros while the grid is periodic, so a storm on
longitude 0 is seen cut in two; a view rolled by S columns sees it whole.  Shift 0 is always member 0, the plain forward pass;
--ensemble_flip_lat adds the north-south mirrored twin of every member, the file channels of --ensemble_negate (the meridional winds)
with their sign reversed; --ensemble_seam_margin N fades every member out over the N columns next to its own seam (1: the plain mean).
Every further view is made from the raw fields by nn.view_input, costs one more forward pass, and is pooled in q.  ``prediction`` stays
the classifier's mask of the identity view; every output file gains ``prediction_ensemble`` (uint8 [H, W], the first maximum of the
pooled logits), with --confidence ``confidence_ensemble``, and ``ensemble_rows`` (int64 [208]: the pixels with exactly k votes for class
c at 64 c + k, the (identity class, pooled class) matrix at 192 + 4 i + j, 3 = not finite).  EVERYTHING downstream takes the pooled mask,
and --decision_* and --prob_skill take the pooled logits in place of the classifier's.  ``summary.json`` gains ``ensemble`` (the views,
the margin and nn.ViewEnsemble.decode's result).  The flags need the NHWC input pipeline (a channel count the MFMA stem takes).
Single process, single device."""
from __future__ import annotations

import argparse
import json
import os
import queue
import threading
import time

import numpy as np
import torch

from . import data as ddata
from . import nn as dnn
from . import png


def _implies(*flags, default=False):
    """The Action class of a flag that implies others: given, it sets every attribute named in `flags` -- its own first -- to True.
    default: False, or argparse.SUPPRESS for a flag that leaves no attribute behind unless given."""

    class Implies(argparse.Action):
        def __init__(self, option_strings, dest, **kw):
            super().__init__(option_strings, dest, nargs=0, default=default, **kw)

        def __call__(self, parser, namespace, values, option_string=None):
            for name in flags:
                setattr(namespace, name, True)

    return Implies


def _prob_bins(text: str) -> int:
    """--prob_bins: an integer in [1, 256]"""
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--prob_bins takes an integer, got {text!r}")
    if not 1 <= k <= dnn.PROB_MAX_BINS:
        raise argparse.ArgumentTypeError(f"--prob_bins must lie in [1, {dnn.PROB_MAX_BINS}], got {k}")
    return k


class _Parser(argparse.ArgumentParser):
    """the checks that span two flags"""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if hasattr(ns, "decision_high") and not (hasattr(ns, "decision_low") or hasattr(ns, "decision_from")):
            self.error("--decision_high needs --decision_low or --decision_from")
        if hasattr(ns, "ensemble_negate") and not hasattr(ns, "ensemble_flip_lat"):
            self.error("--ensemble_negate needs --ensemble_flip_lat")
        if hasattr(ns, "ensemble_seam_margin") and not (hasattr(ns, "ensemble_rolls") or hasattr(ns, "ensemble_flip_lat")):
            self.error("--ensemble_seam_margin needs --ensemble_rolls or --ensemble_flip_lat")
        return ns


def build_parser():
    AP = _Parser(description="DeepCAM inference: masks for unlabelled CAM5 files")
    AP.add_argument("--checkpoint", type=str, required=True, help="a checkpoint written by train.py or by the reference (its 'model' entry), "
                    "or a bare state dict")
    AP.add_argument("--data_dir", type=str, required=True, help="directory with the input .h5 files (climate/data, no labels needed)")
    AP.add_argument("--stats_file", type=str, required=True, help="the stats.h5 of the dataset (climate/minval, climate/maxval)")
    AP.add_argument("--output_dir", type=str, required=True, help="where the mask files and summary.json go")
    AP.add_argument("--batch_size", type=int, default=8, help="samples per forward pass")
    AP.add_argument("--channels", type=int, nargs="+", default=list(range(16)), help="Channels used in input")
    AP.add_argument("--amp_opt_level", type=str, default="O1", help="O0 = fp32 activations, O1/O2 = bf16 activations")
    AP.add_argument("--dtype", type=str, default=None, choices=["fp32", "bf16"], help="overrides --amp_opt_level")
    AP.add_argument("--confidence", action="store_true", help="also store the predicted class's softmax probability")
    AP.add_argument("--events", action="store_true", help="also catalogue the connected components of every mask (dataset 'events')")
    AP.add_argument("--min_event_pixels", type=int, default=0, help="with --events: leave out components of fewer pixels")
    AP.add_argument("--event_connectivity", type=int, default=8, choices=[4, 8], help="with --events: pixel connectivity")
    AP.add_argument("--verify", action=_implies("verify", "events"),
                    help="match the events of every mask to the events of the file's labels (implies --events; "
                    "the files need climate/labels_0): datasets 'truth_events', 'matches', 'event_scores'; 'event_verification' in the summary")
    AP.add_argument("--min_event_cover", type=float, default=0.5, help="with --verify: an event is found when the other mask covers at "
                    "least this share of it with its class, in (0, 1]")
    AP.add_argument("--event_fields", action=_implies("event_fields", "events"),
                    help="per event and file channel the extremes with their positions and the means "
                    "of the raw fields (implies --events): datasets 'event_fields', 'event_field_values', 'event_field_bits'")
    AP.add_argument("--event_shape", action=_implies("event_shape", "events"),
                    help="per event its geometry (implies --events): spherical centroid, length, width, "
                    "aspect, orientation, perimeter, compactness; datasets 'event_shape', 'event_shape_values', 'event_shape_value_names'")
    AP.add_argument("--event_filter", action="store_true", help="filter the classifier's mask by event size and shape on the device (the "
                    "--filter_* thresholds): dataset 'prediction_filtered', 'event_filter' in the summary; --events, --verify's prediction "
                    "side, --event_fields, --tracks, --track_fields, --climatology and --plots all take the FILTERED mask.  The labels "
                    "under --verify are NOT filtered")
    AP.add_argument("--filter_min_pixels", type=int, nargs=2, default=[0, 0], metavar=("TC", "AR"), help="with --event_filter: drop events "
                    "of fewer pixels (class 1, class 2; 0: off)")
    AP.add_argument("--filter_min_area_km2", type=float, nargs=2, default=[0.0, 0.0], metavar=("TC", "AR"), help="with --event_filter: drop "
                    "events of less area")
    AP.add_argument("--filter_min_length_km", type=float, nargs=2, default=[0.0, 0.0], metavar=("TC", "AR"), help="with --event_filter: drop "
                    "events shorter than this (an atmospheric river is roughly 2000 km or longer)")
    AP.add_argument("--filter_min_aspect", type=float, nargs=2, default=[0.0, 0.0], metavar=("TC", "AR"), help="with --event_filter: drop "
                    "events whose length / width is below this (an atmospheric river is at least twice as long as wide)")
    AP.add_argument("--plots", action="store_true", help="also write <output_dir>/plots/<base>.png: the field with the predicted classes "
                    "outlined (with --verify: above the same field with the labelled ones).  Encoding one two-panel 768 x 1152 frame takes tens "
                    "to hundreds of milliseconds of the writer thread, so with --plot_every 1 the writer bounds the rate, not the device: raise --plot_every")
    AP.add_argument("--plot_every", type=int, default=1, help="with --plots: draw every N-th input file")
    AP.add_argument("--plot_channel", type=int, default=0, help="with --plots: the file channel that is drawn (0: integrated water vapour)")
    AP.add_argument("--tracks", action=_implies("tracks", "events"),
                    help="link the events of consecutive files into tracks (implies --events): the files, in the "
                    "order of their sorted names, are taken as one gap-free time sequence (file index = frame number; date gaps or interleaved "
                    "runs are not detected).  Writes <output_dir>/tracks.h5 ('tracks', 'track_events', 'track_state'); 'tracks' in the summary")
    AP.add_argument("--min_track_frames", type=int, default=1, help="with --tracks: the summary also counts the tracks of at least N frames")
    AP.add_argument("--min_track_pixels", type=int, default=0, help="with --tracks: events of fewer pixels link nothing")
    AP.add_argument("--track_fields", action=_implies("track_fields", "tracks", "event_fields", "events"),
                    help="the storm life cycles: per track and frame the merged field rows of its events, "
                    "per track the lifetime extremes with frame and place (implies --tracks and --event_fields; --min_track_frames selects the "
                    "cycles).  tracks.h5 gains 'track_step_offsets', 'track_steps', 'track_step_fields', 'track_fields', 'track_cycle_counts'; "
                    "'track_fields' in the summary")
    AP.add_argument("--verify_tracks", action=_implies("verify_tracks", "verify", "tracks", "events", default=argparse.SUPPRESS),
                    help="match the predicted tracks to the tracks of the files' labels on the device (implies --verify and --tracks): a "
                    "second tracker runs on the labels' events, and every overlap of a predicted and a labelled event is filed under the "
                    "two events' tracks.  tracks.h5 gains 'truth_tracks', 'truth_track_events', 'truth_track_state', 'track_pairs', "
                    "'track_cover', 'truth_track_cover', 'track_scores', 'track_match_state'; 'track_verification' in the summary "
                    "(--min_track_frames: the tracks that are scored)")
    AP.add_argument("--min_track_cover", type=float, default=argparse.SUPPRESS, help="with --verify_tracks: a track is found when tracks of the "
                    "other side overlap it in at least this share of its frames, in (0, 1] (default 0.5)")
    AP.add_argument("--track_center_channel", type=int, default=None, help="with --track_fields: the file channel whose minimum is a track's "
                    "centre (sea-level pressure for cyclones); the summary names the deepest minimum over the class-1 tracks")
    AP.add_argument("--climatology", action="store_true", help="accumulate the maps over time on the device: how often every pixel is class 1 / "
                    "class 2, and the sums of the --climatology_channels over all, class-1 and class-2 frames.  Writes <output_dir>/climatology.h5 "
                    "('frames', 'count', 'sum', 'n', 'bits', 'channels'; with --verify also the labels' 'truth_count', 'truth_sum', 'truth_n'); "
                    "'climatology' in the summary; with --plots one frequency map per group and class")
    AP.add_argument("--climatology_by", type=str, default="all", choices=list(dnn.CLIMATOLOGY_GROUPS), help="with --climatology: one set of "
                    "maps for the whole run, per month or per season (DJF, MAM, JJA, SON), from the first YYYY-MM-DD in every file name")
    AP.add_argument("--climatology_channels", type=int, nargs="*", default=[], help="with --climatology: the file channels whose sums are "
                    "kept (36 bytes per pixel, group and channel); none by default: occurrence only")
    AP.add_argument("--climatology_contour", type=float, default=0.1, help="with --climatology and --plots: the frequency whose region is outlined")
    # the --composite_* flags leave no attribute behind unless given (COMPOSITE_DEFAULTS has their defaults): a namespace without
    # them is the namespace of before
    AP.add_argument("--composites", action=_implies("composites", "event_fields", "events", default=argparse.SUPPRESS),
                    help="accumulate storm-centred composites on the device (implies --event_fields; "
                    "needs --composite_center_channel): windows of the raw fields around every event's centre and their radial profiles.  "
                    "Writes <output_dir>/composites.h5; 'composites' in the summary")
    S = argparse.SUPPRESS
    AP.add_argument("--composite_center_channel", type=int, default=S, help="with --composites: the file channel whose extreme is an "
                    "event's centre (sea-level pressure for cyclones)")
    AP.add_argument("--composite_center_stat", type=str, default=S, choices=["min", "max"], help="with --composites: which extreme (min)")
    AP.add_argument("--composite_radius", type=int, default=S, help="with --composites: the window reaches this many grid pixels from the "
                    "centre (32)")
    AP.add_argument("--composite_channels", type=int, nargs="+", default=S, help="with --composites: the file channels that are composited "
                    "(all)")
    AP.add_argument("--composite_negate", type=int, nargs="*", default=S, help="with --composites: file channels (among --composite_channels) "
                    "whose sign changes in a reflected southern storm: the meridional wind components (none)")
    AP.add_argument("--composite_classes", type=int, nargs="+", default=S, choices=[1, 2], help="with --composites: the event classes (1)")
    AP.add_argument("--composite_min_pixels", type=int, default=S, help="with --composites: leave out events of fewer pixels (0)")
    AP.add_argument("--composite_by", type=str, default=S, choices=list(dnn.CLIMATOLOGY_GROUPS), help="with --composites: one composite "
                    "for the whole run, per month or per season, from the first YYYY-MM-DD in every file name (all)")
    AP.add_argument("--composite_intensity_edges", type=float, nargs="*", default=S, help="with --composites: ascending values of the centre "
                    "channel that cut the events into intensity bins; an event on an edge goes to the bin above (none)")
    AP.add_argument("--composite_no_flip", action="store_true", default=S, help="with --composites: do not reflect southern storms")
    AP.add_argument("--composite_bin_km", type=float, default=S, help="with --composites: the width of a distance bin of the radial profile (25)")
    AP.add_argument("--composite_bins", type=int, default=S, help="with --composites: the number of distance bins; 0: no radial profile (40)")
    # like the --composite_* flags, the --fss* flags leave no attribute behind unless given (FSS_DEFAULTS has their defaults)
    AP.add_argument("--fss", action=_implies("fss", "verify", "events", default=argparse.SUPPRESS),
                    help="neighbourhood verification on the device (implies --verify; the files need climate/labels_0): "
                    "the Fractions Skill Score of --verify's prediction side against the labels per class and window.  Datasets 'fss', "
                    "'fss_pixels'; 'fss' in the summary")
    AP.add_argument("--fss_windows", type=int, nargs="+", default=S, help="with --fss: the windows' sides in grid pixels, distinct odd "
                    "numbers in [1, 255], at most 16 (1 3 9 17 33 65 129)")
    AP.add_argument("--fss_rows", type=int, nargs=2, default=S, metavar=("I0", "I1"), help="with --fss: score the window centres in the "
                    "rows I0 <= i < I1 only (a latitude band; the whole frame by default)")
    AP.add_argument("--fss_no_wrap", action="store_true", default=S, help="with --fss: do not take the columns as periodic")
    # likewise the --distance_* flags (DISTANCE_DEFAULTS)
    AP.add_argument("--distance_skill", action=_implies("distance_skill", "verify", "events", default=argparse.SUPPRESS),
                    help="distance-map verification on the device (implies --verify; the files "
                    "need climate/labels_0): mean error distance, Hausdorff distance, Baddeley's Delta and hit rate / success ratio within "
                    "r grid pixels of --verify's prediction side against the labels, per class.  Datasets 'distance', 'distance_baddeley'; "
                    "'distance_skill' in the summary")
    AP.add_argument("--distance_radius", type=int, default=S, help="with --distance_skill: the cap R on the distances in grid pixels, "
                    "1 .. 127, with periodic columns 2 R + 1 <= --width (64)")
    AP.add_argument("--distance_rows", type=int, nargs=2, default=S, metavar=("I0", "I1"), help="with --distance_skill: count the sources "
                    "in the rows I0 <= i < I1 only (a latitude band; the whole frame by default)")
    AP.add_argument("--distance_no_wrap", action="store_true", default=S, help="with --distance_skill: do not take the columns as periodic")
    # likewise the --displacement* flags (DISPLACEMENT_DEFAULTS)
    AP.add_argument("--displacement", action=_implies("displacement", "verify", "events", default=argparse.SUPPRESS),
                    help="displacement verification on the device (implies --verify; the files "
                    "need climate/labels_0): the shift of --verify's prediction side that overlaps the labels most, the scores without "
                    "and with it and the CRA decomposition of the error, per class.  Datasets 'displacement', 'displacement_pixels', "
                    "'displacement_best'; 'displacement' in the summary")
    AP.add_argument("--displacement_radius", type=int, default=S, help="with --displacement: the largest shift in rows and in columns, "
                    "1 .. 63, with 2 R + 1 <= --width (16)")
    AP.add_argument("--displacement_rows", type=int, nargs=2, default=S, metavar=("I0", "I1"), help="with --displacement: score the label "
                    "rows I0 <= i < I1 only (a latitude band; the whole frame by default)")
    # likewise the --scale_* flags (SCALE_DEFAULTS)
    AP.add_argument("--scale_skill", action=_implies("scale_skill", "verify", "events", default=argparse.SUPPRESS),
                    help="scale-separation verification on the device (implies --verify; the files "
                    "need climate/labels_0): the squared error of --verify's prediction side and the energies of both sides per 2-D Haar "
                    "component of scale 1, 2, 4, ... grid pixels, per class (the intensity-scale skill score).  Datasets 'scale', "
                    "'scale_pixels'; 'scale_skill' in the summary")
    AP.add_argument("--scale_levels", type=int, default=S, help="with --scale_skill: the levels L, 1 .. 8; the tile 2^L must divide the "
                    "scored rows and --width (the largest that does)")
    AP.add_argument("--scale_rows", type=int, nargs=2, default=S, metavar=("I0", "I1"), help="with --scale_skill: score the rows "
                    "I0 <= i < I1 only (a latitude band; the whole frame by default)")
    AP.add_argument("--scale_origins", type=int, nargs="+", default=S, metavar="C", help="with --scale_skill: up to 8 column offsets in "
                    "[0, 2^L) of the dyadic grid, scored in one pass (0)")
    # likewise the --prob_* flags (PROB_DEFAULTS)
    AP.add_argument("--prob_skill", action=_implies("prob_skill", "verify", "events", default=argparse.SUPPRESS),
                    help="probabilistic verification on the device (implies --verify; the files need "
                    "climate/labels_0): reliability diagram, Brier score with its decomposition, POD / POFD / CSI per probability threshold "
                    "and ROC area per class, from the classifier's softmax probabilities against the labels.  It always scores the "
                    "classifier's probabilities: --event_filter does not change them.  Datasets 'brier', 'prob_pixels'; prob_skill.h5; "
                    "'prob_skill' in the summary")
    AP.add_argument("--prob_bins", type=_prob_bins, default=S, help="with --prob_skill: the probability bins, 1 .. 256; the thresholds are "
                    "k / bins (20)")
    # likewise the --decision_* flags
    low = AP.add_mutually_exclusive_group()
    low.add_argument("--decision_low", type=float, nargs=2, default=S, metavar=("TC", "AR"), help="decide the mask by probability thresholds "
                     "on the device, not by the argmax: class 1 / class 2 where its softmax probability is at least this.  Dataset "
                     "'prediction_decided' and the counters 'decision'; everything downstream (--event_filter, --events, --verify, --fss, "
                     "...) takes the decided mask; 'prediction' stays the argmax")
    low.add_argument("--decision_from", type=str, default=S, metavar="FILE", help="like --decision_low, the thresholds being the best-CSI "
                     "thresholds of the prob_skill.h5 an earlier --prob_skill run wrote (typically on the validation split)")
    AP.add_argument("--decision_high", type=float, nargs=2, default=S, metavar=("TC", "AR"), help="with --decision_low or --decision_from: "
                    "hysteresis -- a connected region above the low threshold is kept only if it holds a pixel at or above this one")
    # likewise the --ensemble_* flags (ENSEMBLE_DEFAULTS)
    AP.add_argument("--ensemble_rolls", type=int, nargs="+", default=S, metavar="S", help="test-time augmentation on the device: also predict "
                    "on the frame rolled by S columns (periodic longitudes; only the network's zero padding breaks that symmetry) and pool "
                    "the views' probabilities.  Shift 0 is always member 0, the plain forward pass; every other view costs one more.  "
                    "Datasets 'prediction_ensemble', 'ensemble_rows'; 'ensemble' in the summary; everything downstream takes the pooled "
                    "mask, --decision_* and --prob_skill the pooled logits; 'prediction' stays the identity view's mask")
    AP.add_argument("--ensemble_flip_lat", action="store_true", default=S, help="add the north-south mirrored twin of every ensemble member")
    AP.add_argument("--ensemble_negate", type=int, nargs="+", default=S, metavar="C", help="with --ensemble_flip_lat: the file channels "
                    "(among --channels) whose sign reverses in a mirrored view: the meridional wind components (none)")
    AP.add_argument("--ensemble_seam_margin", type=int, default=S, metavar="N", help="with --ensemble_rolls or --ensemble_flip_lat: a member "
                    "weighs min(d + 1, N) at a pixel d columns from the nearer edge of its own view, so that near a view's seam the other "
                    "views decide (1: the plain mean)")
    AP.add_argument("--height", type=int, default=768)
    AP.add_argument("--width", type=int, default=1152)
    AP.add_argument("--max_inter_threads", type=int, default=4, help="Maximum number of concurrent readers")
    return AP


def track_fields_summary(rows: dict, height: int, width: int, center_channel=None) -> dict:
    """the `track_fields` entry of summary.json from nn.TrackFields.rows(): the four counters, the cycles per class and, with a centre
    channel, the deepest lifetime minimum of that channel over the stored class-1 tracks (the smallest track row among equals)"""
    counts = [int(v) for v in rows["counts"]]
    tracks, stored = rows["tracks"], rows["offsets"] >= 0
    out = {"tracks_selected": counts[0], "steps_needed": counts[1], "steps_stored": counts[2], "tracks_not_stored": counts[3],
           "class_1": int((stored & (tracks[:, 1] == 1)).sum()), "class_2": int((stored & (tracks[:, 1] == 2)).sum())}
    if center_channel is not None:
        c = int(center_channel)
        out["center_channel"], out["deepest_class_1"] = c, None
        life = rows["track_fields"][:, c]
        pick = np.flatnonzero(stored & (tracks[:, 1] == 1) & (life[:, 0] != -1))
        if len(pick):
            t = int(pick[int(np.argmin(life[pick, 0].view(np.uint64)))])
            word, p = int(life[t, 0]) & 0xFFFFFFFFFFFFFFFF, int(life[t, 1])
            out["deepest_class_1"] = {"id": int(tracks[t, 0]), "value": float(dnn.event_field_value(np.uint32(word >> 32))),
                                      "frame": word & 0xFFFFFFFF, "lat": float(np.linspace(-90.0, 90.0, height)[p // width]),
                                      "lon": float(np.linspace(-180.0, 180.0, width)[p % width])}
    return out


COMPOSITE_DEFAULTS = {"composite_center_channel": None, "composite_center_stat": "min", "composite_radius": 32, "composite_channels": None,
                      "composite_negate": [], "composite_classes": [1], "composite_min_pixels": 0, "composite_by": "all",
                      "composite_intensity_edges": [], "composite_no_flip": False, "composite_bin_km": 25.0, "composite_bins": 40}


def composite_options(pargs, cfile: int, width: int) -> dict:
    """the keyword arguments of nn.StormComposite from the --composite_* flags (COMPOSITE_DEFAULTS where one was not given), validated
    against the files' channel count and the width; --composite_negate names FILE channels and is turned into positions among the
    selected ones"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in COMPOSITE_DEFAULTS.items()})
    cc = a.composite_center_channel
    if cc is None:
        raise ValueError("--composites needs --composite_center_channel")
    if not 0 <= int(cc) < cfile:
        raise ValueError(f"--composite_center_channel must lie in [0, {cfile}), got {cc}")
    channels = list(range(cfile)) if a.composite_channels is None else [int(c) for c in a.composite_channels]
    if not 1 <= len(channels) <= 32 or any(not 0 <= c < cfile for c in channels) or len(set(channels)) != len(channels):
        raise ValueError(f"--composite_channels: between 1 and 32 distinct file channels in [0, {cfile}), got {channels}")
    negate = [int(c) for c in a.composite_negate]
    if any(c not in channels for c in negate):
        raise ValueError(f"--composite_negate: every channel must be one of --composite_channels {channels}, got {negate}")
    radius = int(a.composite_radius)
    if not 1 <= radius <= dnn.COMPOSITE_MAX_RADIUS or 2 * radius + 1 > width:
        raise ValueError(f"--composite_radius must lie in [1, {dnn.COMPOSITE_MAX_RADIUS}] with 2 * radius + 1 <= --width, got {radius}")
    edges = [float(e) for e in a.composite_intensity_edges]
    if len(edges) > 255 or not all(np.isfinite(edges)) or any(hi < lo for lo, hi in zip(edges, edges[1:])):
        raise ValueError(f"--composite_intensity_edges: at most 255 finite ascending values, got {edges}")
    if a.composite_min_pixels < 0:
        raise ValueError("--composite_min_pixels must not be negative")
    if not 0 <= a.composite_bins <= 255 or not a.composite_bin_km > 0:
        raise ValueError("--composite_bins must lie in [0, 255] and --composite_bin_km be positive")
    return {"center_channel": int(cc), "center_stat": a.composite_center_stat, "radius": radius, "channels": channels,
            "classes": tuple(sorted(set(a.composite_classes))), "min_pixels": int(a.composite_min_pixels),
            "groups": len(dnn.CLIMATOLOGY_GROUPS[a.composite_by]), "intensity_edges": tuple(edges),
            "flip_south": not a.composite_no_flip, "negate": tuple(channels.index(c) for c in negate),
            "bin_km": float(a.composite_bin_km), "bins": int(a.composite_bins)}


def composite_group_names(by: str, edges) -> list:
    """the names of the GT composites in their order: the group, then ".bin<k>" when there are intensity edges"""
    names = dnn.CLIMATOLOGY_GROUPS[by]
    return [g if not len(edges) else f"{g}.bin{k}" for g in names for k in range(len(edges) + 1)]


def composite_summary(by: str, comp_kwargs: dict, state: dict, decoded: dict) -> dict:
    """the `composites` entry of summary.json: the definition, the counters, the events per composite and, per composite and selected
    channel, the radius of the largest radial mean (None where there is none)"""
    clean = lambda a: [None if np.isnan(v) else float(v) for v in a]  # noqa: E731
    return {"by": by, "group_names": composite_group_names(by, comp_kwargs["intensity_edges"]), "center_channel": comp_kwargs["center_channel"],
            "center_stat": comp_kwargs["center_stat"], "radius": comp_kwargs["radius"], "channels": list(comp_kwargs["channels"]),
            "classes": list(comp_kwargs["classes"]), "min_pixels": comp_kwargs["min_pixels"], "intensity_edges": list(comp_kwargs["intensity_edges"]),
            "flip_south": comp_kwargs["flip_south"], "counts": dict(state["counts"]), "events": [int(v) for v in state["events"]],
            "radius_of_max_km": [clean(row) for row in decoded["radius_of_max_km"]]}


FSS_DEFAULTS = {"fss": False, "fss_windows": list(dnn.FSS_WINDOWS), "fss_rows": None, "fss_no_wrap": False}


def fss_options(pargs) -> dict:
    """the keyword arguments of nn.FractionsSkill from the --fss_* flags (FSS_DEFAULTS where one was not given)"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in FSS_DEFAULTS.items()})
    return {"windows": tuple(int(n) for n in a.fss_windows), "wrap": not a.fss_no_wrap,
            "row_range": None if a.fss_rows is None else (int(a.fss_rows[0]), int(a.fss_rows[1]))}


def fss_summary(windows, row_range, width: int, state: dict) -> dict:
    """the `fss` entry of summary.json from nn.FractionsSkill.state(): the windows, the scored rows, the frames and, per class, the
    decoded result (pooled scores, base rate, useful score, skilful window) with the raw totals [S][3] as integers"""
    decoded = dnn.FractionsSkill.decode(state["total"], state["pixels"], state["frames"], windows, row_range[1] - row_range[0], width)
    out = {"windows": [int(n) for n in windows], "rows": [int(row_range[0]), int(row_range[1])], "frames": int(state["frames"])}
    for k in range(2):
        out[f"class_{k + 1}"] = dict(decoded[f"class_{k + 1}"], total=[[int(v) for v in term] for term in state["total"][k]],
                                     pixels=[int(v) for v in state["pixels"][k]])
    return out


DISTANCE_DEFAULTS = {"distance_skill": False, "distance_radius": dnn.DISTANCE_RADIUS, "distance_rows": None, "distance_no_wrap": False}


def distance_options(pargs) -> dict:
    """the keyword arguments of nn.DistanceSkill from the --distance_* flags (DISTANCE_DEFAULTS where one was not given)"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in DISTANCE_DEFAULTS.items()})
    return {"radius": int(a.distance_radius), "wrap": not a.distance_no_wrap,
            "row_range": None if a.distance_rows is None else (int(a.distance_rows[0]), int(a.distance_rows[1]))}


def distance_summary(radius: int, wrap: bool, row_range, height: int, width: int, state: dict) -> dict:
    """the `distance_skill` entry of summary.json from nn.DistanceSkill.state(): the cap, the scored rows, the frames and, per class, the
    decoded result with the raw totals [2][R + 4] and the Baddeley sum as integers"""
    decoded = dnn.DistanceSkill.decode(state["total"], state["baddeley"], state["frames"], radius, height, width, row_range)
    out = {"radius": int(radius), "wrap": bool(wrap), "rows": [int(row_range[0]), int(row_range[1])], "frames": int(state["frames"])}
    for k in range(2):
        out[f"class_{k + 1}"] = dict(decoded[f"class_{k + 1}"], total=[[int(v) for v in d] for d in state["total"][k]],
                                     total_baddeley=int(state["baddeley"][k]))
    return out


DISPLACEMENT_DEFAULTS = {"displacement": False, "displacement_radius": dnn.DISPLACEMENT_RADIUS, "displacement_rows": None}


def displacement_options(pargs) -> dict:
    """the keyword arguments of nn.DisplacementSkill from the --displacement* flags (DISPLACEMENT_DEFAULTS where one was not given)"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in DISPLACEMENT_DEFAULTS.items()})
    return {"radius": int(a.displacement_radius),
            "row_range": None if a.displacement_rows is None else (int(a.displacement_rows[0]), int(a.displacement_rows[1]))}


def displacement_summary(radius: int, row_range, height: int, width: int, state: dict, frame_best) -> dict:
    """the `displacement` entry of summary.json from nn.DisplacementSkill.state() and the per-frame best shifts (int64 [n, 2, 4], the
    files' displacement_best): the radius, the scored rows, the frames and, per class, the pooled decode (its "best" the raw integers of
    the common shift) with frame_shifts: over the frames that have hits, their number and the mean dy, mean dx and mean length of the
    per-frame best shifts (None without such a frame)"""
    decoded = dnn.DisplacementSkill.decode(state["total"], state["pixels"], state["frames"], radius, height, width, row_range)
    best = np.asarray(frame_best, np.int64).reshape(-1, 2, 4)
    out = {"radius": int(radius), "rows": [int(row_range[0]), int(row_range[1])], "frames": int(state["frames"])}
    for k in range(2):
        shifts = best[best[:, k, 2] > 0, k, :2].astype(np.float64)
        n = len(shifts)
        out[f"class_{k + 1}"] = dict(decoded[f"class_{k + 1}"], frame_shifts={
            "frames": n, "mean_rows": float(shifts[:, 0].mean()) if n else None, "mean_cols": float(shifts[:, 1].mean()) if n else None,
            "mean_pixels": float(np.sqrt((shifts ** 2).sum(axis=1)).mean()) if n else None})
    return out


SCALE_DEFAULTS = {"scale_skill": False, "scale_levels": None, "scale_rows": None, "scale_origins": (0,)}


def scale_options(pargs) -> dict:
    """the keyword arguments of nn.ScaleSkill from the --scale_* flags (SCALE_DEFAULTS where one was not given)"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in SCALE_DEFAULTS.items()})
    return {"levels": None if a.scale_levels is None else int(a.scale_levels),
            "row_range": None if a.scale_rows is None else (int(a.scale_rows[0]), int(a.scale_rows[1])),
            "origins": tuple(int(c) for c in a.scale_origins)}


def scale_summary(levels: int, origins, row_range, width: int, state: dict) -> dict:
    """the `scale_skill` entry of summary.json from nn.ScaleSkill.state(): the levels, the origins, the scored rows, the frames and, per
    class, the pooled decode"""
    out = {"levels": int(levels), "origins": [int(c) for c in origins], "rows": [int(row_range[0]), int(row_range[1])],
           "frames": int(state["frames"])}
    out.update(dnn.ScaleSkill.decode(state["total"], state["pixels"], state["frames"], levels, row_range[1] - row_range[0], width, origins))
    return out


PROB_DEFAULTS = {"prob_skill": False, "prob_bins": dnn.PROB_BINS}
PROB_SUMMARY_KEYS = ("brier", "brier_skill", "reliability", "resolution", "ece", "auc", "best_csi_threshold", "base_rate")
PROB_SCALARS = ("n", "base_rate", "mean_probability", "brier", "brier_skill", "reliability", "resolution", "uncertainty", "ece", "mce", "auc",
                "best_csi", "best_csi_threshold")


def prob_options(pargs) -> dict:
    """the keyword arguments of nn.ProbabilitySkill from the --prob_* flags (PROB_DEFAULTS where one was not given)"""
    return {"bins": int(getattr(pargs, "prob_bins", PROB_DEFAULTS["prob_bins"]))}


def prob_summary(bins: int, state: dict) -> dict:
    """the `prob_skill` entry of summary.json from nn.ProbabilitySkill.state(): bins, frames, the pixel counters and, per class, the
    scalar scores of decode() named in PROB_SUMMARY_KEYS"""
    decoded = dnn.ProbabilitySkill.decode(state["hist"], state["sq"], state["pixels"], bins)
    out = {"bins": int(bins), "frames": int(state["frames"]), "pixels": decoded["pixels"]}
    for c in range(3):
        out[f"class_{c}"] = {k: decoded[f"class_{c}"][k] for k in PROB_SUMMARY_KEYS}
    return out


def prob_arrays(bins: int, state: dict) -> dict:
    """the datasets of prob_skill.h5: the raw integers (the squared errors as (lo, hi) words) and decode()'s curves, None as NaN"""
    decoded = dnn.ProbabilitySkill.decode(state["hist"], state["sq"], state["pixels"], bins)
    per_class = [decoded[f"class_{c}"] for c in range(3)]
    real = lambda rows: np.asarray([[np.nan if v is None else float(v) for v in row] for row in rows], np.float64)  # noqa: E731
    words = [[(v & 0xFFFFFFFFFFFFFFFF) - ((v & (1 << 63)) << 1), v >> 64] for v in (int(v) for v in state["sq"])]
    return {"hist": np.asarray(state["hist"], np.int64), "sq_words": np.asarray(words, np.int64),
            "pixels": np.asarray(state["pixels"], np.int64), "frames": np.asarray([state["frames"]], np.int64),
            "bins": np.asarray([bins], np.int32),
            "curve_mean_probability": real(d["curve"]["mean_probability"] for d in per_class),
            "curve_observed_frequency": real(d["curve"]["observed_frequency"] for d in per_class),
            "curve_n": np.asarray([d["curve"]["n"] for d in per_class], np.int64), "sharpness": real(d["sharpness"] for d in per_class),
            "pod": real(d["pod"] for d in per_class), "pofd": real(d["pofd"] for d in per_class), "csi": real(d["csi"] for d in per_class),
            "bias": real(d["bias"] for d in per_class), "scalars": real([d[k] for k in PROB_SCALARS] for d in per_class),
            "scalar_names": np.frombuffer(",".join(PROB_SCALARS).encode(), np.uint8).copy()}


DECISION_FLAGS = ("decision_low", "decision_high", "decision_from")


def read_datasets(path: str, names) -> dict:
    """name -> array of the named datasets of one HDF5 file, through the backend data.CamDataset reads with"""
    backend, h5 = ddata._h5_backend()
    with (h5.File(path, "r") if backend == "h5py" else h5.File(path)) as f:
        return {n: np.asarray(f[n][...] if backend == "h5py" else f.read(n)) for n in names}


def decision_options(pargs):
    """the `low` and `high` of nn.DecisionRule from the --decision_* flags, None where none of them was given: --decision_low's
    probabilities, or the q thresholds of --decision_from's prob_skill.h5; --decision_high's probabilities or None"""
    if not any(hasattr(pargs, k) for k in DECISION_FLAGS):
        return None
    low, source = getattr(pargs, "decision_low", None), getattr(pargs, "decision_from", None)
    if (low is None) == (source is None):
        raise ValueError("give exactly one of --decision_low and --decision_from" if low is not None else
                         "--decision_high needs --decision_low or --decision_from")
    if source is not None:
        low = dnn.DecisionRule.low_from_prob_skill(read_datasets(source, ("scalars", "scalar_names", "bins")))
    else:
        low = tuple(float(v) for v in low)
    high = getattr(pargs, "decision_high", None)
    return {"low": low, "high": None if high is None else tuple(float(v) for v in high)}


def decision_summary(rule, records) -> dict:
    """the `decision` entry of summary.json: the thresholds as q and as probabilities, whether hysteresis ran, the connectivity, and the
    counters summed over the files"""
    totals = [sum(r["decision"][k] for r in records) for k in range(len(dnn.DECISION_COUNTS))]
    return dict(rule.thresholds(), hysteresis=rule.hysteresis, connectivity=rule.connectivity, wrap=rule.wrap,
                counts=dict(zip(dnn.DECISION_COUNTS, totals)))


ENSEMBLE_DEFAULTS = {"ensemble_rolls": None, "ensemble_flip_lat": False, "ensemble_negate": [], "ensemble_seam_margin": 1}


def ensemble_options(pargs, width: int, channels):
    """From the --ensemble_* flags (ENSEMBLE_DEFAULTS where one was not given), None where neither --ensemble_rolls nor
    --ensemble_flip_lat was: {"views": the (roll, flip) pairs in member order -- (0, False) first, then the other shifts as given, then
    the mirrored twin of each --, "margin", "negate": the file channels whose sign a mirrored view reverses}, validated against the width
    and the selected file channels"""
    a = argparse.Namespace(**{k: getattr(pargs, k, v) for k, v in ENSEMBLE_DEFAULTS.items()})
    if a.ensemble_rolls is None and not a.ensemble_flip_lat:
        if a.ensemble_negate or a.ensemble_seam_margin != 1:
            raise ValueError("--ensemble_negate and --ensemble_seam_margin need --ensemble_rolls or --ensemble_flip_lat")
        return None
    rolls = [0]
    for s in a.ensemble_rolls or []:
        s = int(s)
        if not 0 <= s < width:
            raise ValueError(f"--ensemble_rolls: a shift must lie in [0, {width}), got {s}")
        if s not in rolls:
            rolls.append(s)
    negate = [int(c) for c in a.ensemble_negate]
    if negate and not a.ensemble_flip_lat:
        raise ValueError("--ensemble_negate needs --ensemble_flip_lat")
    if any(c not in list(channels) for c in negate):
        raise ValueError(f"--ensemble_negate: every channel must be one of --channels {list(channels)}, got {negate}")
    margin = int(a.ensemble_seam_margin)
    views = [(s, False) for s in rolls] + ([(s, True) for s in rolls] if a.ensemble_flip_lat else [])
    if len(views) > dnn.ENSEMBLE_MAX_MEMBERS or margin < 1 or margin * len(views) > dnn.ENSEMBLE_MAX_WEIGHT_SUM:
        raise ValueError(f"--ensemble_*: at most {dnn.ENSEMBLE_MAX_MEMBERS} views, and --ensemble_seam_margin at least 1 with margin * views "
                         f"at most {dnn.ENSEMBLE_MAX_WEIGHT_SUM}, got {len(views)} views and margin {margin}")
    return {"views": views, "margin": margin, "negate": negate}


def ensemble_summary(options: dict, state: dict) -> dict:
    """the `ensemble` entry of summary.json: the views as [roll, flip] in member order, the margin, the negated channels and
    nn.ViewEnsemble.decode of the running totals"""
    return dict(dnn.ViewEnsemble.decode(state["totals"], state["frames"], len(options["views"])),
                views=[[int(s), bool(f)] for s, f in options["views"]], seam_margin=options["margin"], negate=list(options["negate"]))


def climatology_summary(by: str, frames, maps: dict, truth_maps=None, channels=()) -> dict:
    """the `climatology` entry of summary.json: the groups' names and frames and, per class, the area-weighted frequency of every group
    (None for a group without a frame); with --verify the same of the labels"""
    clean = lambda a: [None if np.isnan(v) else float(v) for v in a]  # noqa: E731
    out = {"by": by, "groups": list(dnn.CLIMATOLOGY_GROUPS[by]), "frames": [int(v) for v in frames], "channels": [int(c) for c in channels],
           "area_frequency": {f"class_{k + 1}": clean(maps["area_frequency"][:, k]) for k in range(2)}}
    if truth_maps is not None:
        out["truth_area_frequency"] = {f"class_{k + 1}": clean(truth_maps["area_frequency"][:, k]) for k in range(2)}
    return out


def climatology_plot_name(group: str, cls: int) -> str:
    return f"climatology-{group}-class{cls}.png"


def climatology_pictures(clim, truth, contour: float, by: str) -> dict:
    """file name -> uint8 [rows, W, 3]: per group with a frame and per class the frequency map across [0, 1] through nn.FrameRenderer, the
    region of frequency >= contour outlined; with `truth` (the labels' climatology) the labels' picture below it"""
    renderer = dnn.FrameRenderer(clim.G, clim.H, clim.W, channel=0, ldc=1, lo=0.0, hi=1.0, panels=1, device=clim.device)
    names = dnn.CLIMATOLOGY_GROUPS[by]
    never = float("inf")
    out = {}
    for cls in (1, 2):
        t = (contour, never) if cls == 1 else (never, contour)
        panels = [renderer(*c.fields([("frequency", cls)], *t)).cpu().numpy() for c in ([clim] if truth is None else [clim, truth])]
        for g, name in enumerate(names):
            if clim.host_frames[g]:
                out[climatology_plot_name(name, cls)] = np.concatenate([p[g] for p in panels], axis=0)
    return out


def write_mask_file(path: str, prediction: np.ndarray, confidence, events=None, extra=None) -> None:
    """`prediction` (and `confidence`, `events`, the datasets of `extra`) as datasets of one HDF5 file, through the backend
    data.CamDataset reads with."""
    backend, h5 = ddata._h5_backend()
    if backend == "h5py":
        with h5.File(path, "w") as f:
            f.create_dataset("prediction", data=prediction)
            if confidence is not None:
                f.create_dataset("confidence", data=confidence)
            if events is not None:
                f.create_dataset("events", data=events)
            for name, array in (extra or {}).items():
                f.create_dataset(name, data=array)
        return
    with h5.File(path, "w") as f:
        f.write("prediction", prediction)
        if confidence is not None:
            f.write("confidence", confidence)
        if events is not None:
            f.write("events", events)
        for name, array in (extra or {}).items():
            f.write(name, array)


def write_datasets(path: str, arrays: dict) -> None:
    """the arrays as datasets of one HDF5 file, through the backend data.CamDataset reads with"""
    backend, h5 = ddata._h5_backend()
    with h5.File(path, "w") as f:
        for name, array in arrays.items():
            if backend == "h5py":
                f.create_dataset(name, data=array)
            else:
                f.write(name, array)


def track_summary(state, tracks, min_frames: int = 1) -> dict:
    """the `tracks` entry of summary.json from the four counters and the track rows [n, 8]: per class the number of tracks, of those with
    at least min_frames frames, and the longest one (the smallest id among equals)"""
    tracks = np.asarray(tracks, np.int64).reshape(-1, len(dnn.TRACK_FIELDS))
    out = {"min_frames": int(min_frames), "tracks": len(tracks)}
    frames = tracks[:, 4] - tracks[:, 3] + 1
    for cls in (1, 2):
        sel = tracks[:, 1] == cls
        longest = None
        if sel.any():
            t = tracks[sel][int(np.argmax(frames[sel]))]
            longest = {"id": int(t[0]), "frames": int(t[4] - t[3] + 1), "first_frame": int(t[3]), "last_frame": int(t[4]), "events": int(t[2]),
                       "pixels": int(t[5])}
        out[f"class_{cls}"] = {"tracks": int(sel.sum()), "tracks_min_frames": int((sel & (frames >= min_frames)).sum()), "longest": longest}
    s = [int(v) for v in state]
    out["state"] = {"events": s[0], "frames": s[1], "events_dropped": s[2], "frames_truncated": s[3]}
    return out


def require_labels(data_dir: str) -> None:
    """--verify: every input file must hold climate/labels_0; the first one that does not is named."""
    backend, h5 = ddata._h5_backend()
    for name in sorted(x for x in os.listdir(data_dir) if x.endswith(".h5")):
        path = os.path.join(data_dir, name)
        with (h5.File(path, "r") if backend == "h5py" else h5.File(path)) as f:
            if "climate/labels_0" not in f:
                raise ValueError(f"--verify needs labelled files: {path} has no climate/labels_0")


def filter_matches(rows_a: np.ndarray, rows_b: np.ndarray, pairs: np.ndarray, min_pixels: int):
    """The rows of both tables with at least min_pixels pixels, and the pairs between them with their ranks renumbered to the rows that
    are left (so `matches` indexes `events` and `truth_events` as they are stored)."""
    keep_a, keep_b = rows_a[:, 2] >= min_pixels, rows_b[:, 2] >= min_pixels
    new_a, new_b = np.cumsum(keep_a) - 1, np.cumsum(keep_b) - 1
    pairs = pairs.reshape(-1, 3)
    pairs = pairs[keep_a[pairs[:, 0]] & keep_b[pairs[:, 1]]]
    out = np.stack([new_a[pairs[:, 0]], new_b[pairs[:, 1]], pairs[:, 2]], axis=1).astype(np.int64).reshape(-1, 3)
    return np.ascontiguousarray(rows_a[keep_a]), np.ascontiguousarray(rows_b[keep_b]), np.ascontiguousarray(out)


def plot_name(base: str) -> str:
    """the picture's file name for an input file's base name"""
    return (base[:-3] if base.endswith(".h5") else base) + ".png"


class _HostSlot:
    def __init__(self, B: int, H: int, W: int, confidence: bool, event_cap: int = 0, pair_cap: int = 0, field_channels: int = 0,
                 plot_rows: int = 0, event_shape: bool = False, event_filter: bool = False, decision: bool = False, frame_skills=(),
                 ensemble: bool = False):
        # --ensemble_*: the pooled mask, its confidence and the counters of nn.ViewEnsemble
        self.emask = torch.empty((B, H, W), dtype=torch.uint8).pin_memory() if ensemble else None
        self.econf = torch.empty((B, H, W), dtype=torch.float32).pin_memory() if ensemble and confidence else None
        self.erows = torch.empty((B, dnn.ENSEMBLE_ROW), dtype=torch.int64).pin_memory() if ensemble else None
        # --fss, --distance_skill, --displacement, --scale_skill, --prob_skill: per skill the buffers of its frame_rows(), under the
        # names of its FRAME_KEYS and in the skills' order, which is the order of their datasets in a mask file
        self.frames = {key: torch.empty((B, *t.shape[1:]), dtype=t.dtype).pin_memory()
                       for skill in frame_skills for key, t in zip(skill.FRAME_KEYS, skill.frame_rows())}
        # --decision_*: the decided mask and the rule's counters
        self.dmask = torch.empty((B, H, W), dtype=torch.uint8).pin_memory() if decision else None
        self.dcounts = torch.empty((B, len(dnn.DECISION_COUNTS)), dtype=torch.int64).pin_memory() if decision else None
        # --event_shape: the rows of nn.EventShape (cap rows of 96 bytes per sample)
        self.shape = torch.empty((B, event_cap, len(dnn.EVENT_SHAPE_FIELDS)), dtype=torch.int64).pin_memory() if event_shape else None
        # --event_filter: the filtered mask and the filter's counts
        self.fmask = torch.empty((B, H, W), dtype=torch.uint8).pin_memory() if event_filter else None
        self.fcounts = torch.empty((B, 2, len(dnn.EVENT_FILTER_COUNTS)), dtype=torch.int64).pin_memory() if event_filter else None
        # --plots: the RGB bytes of nn.FrameRenderer, per sample the panels stacked
        self.rgb = torch.empty((B, plot_rows, W, 3), dtype=torch.uint8).pin_memory() if plot_rows else None
        # --event_fields: the rows of nn.EventFields (cap * C rows of 48 bytes per sample)
        self.fields = torch.empty((B, event_cap, field_channels, len(dnn.EVENT_FIELD_STATS)), dtype=torch.int64).pin_memory() \
            if field_channels else None
        # --verify: the label side's table and counts, the pair table with its counts, the scores
        self.truth = torch.empty((B, event_cap, len(dnn.EVENT_FIELDS)), dtype=torch.int64).pin_memory() if pair_cap else None
        self.ntruth = torch.empty((B, 3), dtype=torch.int32).pin_memory() if pair_cap else None
        self.pairs = torch.empty((B, pair_cap, 3), dtype=torch.int64).pin_memory() if pair_cap else None
        self.npairs = torch.empty((B, 2), dtype=torch.int32).pin_memory() if pair_cap else None
        self.scores = torch.empty((B, 2, 4), dtype=torch.int64).pin_memory() if pair_cap else None
        # --events: the whole table of a batch (cap rows of 80 bytes per sample) and the counts that say how many rows are filled
        self.events = torch.empty((B, event_cap, len(dnn.EVENT_FIELDS)), dtype=torch.int64).pin_memory() if event_cap else None
        self.ncomp = torch.empty((B, 3), dtype=torch.int32).pin_memory() if event_cap else None
        self.mask = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
        self.conf = torch.empty((B, H, W), dtype=torch.float32).pin_memory() if confidence else None
        self.counts = torch.empty((B, 3), dtype=torch.int64).pin_memory()
        self.done = torch.cuda.Event()


def _writer(work_q: "queue.Queue", free_q: "queue.Queue", out_dir: str, records: list, errors: list, min_event_pixels: int = 0,
            field_bits=None) -> None:
    while True:
        item = work_q.get()
        if item is None:
            return
        slot, names, plot = item
        try:
            if not errors:
                slot.done.synchronize()                      # host wait of THIS thread: the copies of the batch have landed
                for j, name in enumerate(names):
                    conf = slot.conf[j].numpy() if slot.conf is not None else None
                    base = os.path.basename(name)
                    rows = extra = None
                    if slot.events is not None:
                        total = int(slot.ncomp[j, 0])
                        rows = slot.events[j, :min(total, slot.events.shape[1])].numpy()
                        frows = srows = None
                        if slot.fields is not None:          # the filter of `events`, whichever branch below applies it
                            frows = np.ascontiguousarray(slot.fields[j, :len(rows)].numpy()[rows[:, 2] >= min_event_pixels])
                        if slot.shape is not None:
                            srows = np.ascontiguousarray(slot.shape[j, :len(rows)].numpy()[rows[:, 2] >= min_event_pixels])
                        if slot.pairs is not None:
                            truth = slot.truth[j, :min(int(slot.ntruth[j, 0]), slot.truth.shape[1])].numpy()
                            pairs = dnn.EventMatcher.sort_pairs(slot.pairs[j, :int(slot.npairs[j, 0])].numpy())
                            rows, truth, pairs = filter_matches(rows, truth, pairs, min_event_pixels)
                            extra = {"truth_events": truth, "matches": pairs, "event_scores": slot.scores[j].numpy()}
                        else:
                            rows = np.ascontiguousarray(rows[rows[:, 2] >= min_event_pixels])
                        if frows is not None:
                            H, W = slot.mask.shape[1:]
                            extra = dict(extra or {}, event_fields=frows, event_field_values=dnn.EventFields.values(frows, rows, H, W, field_bits),
                                         event_field_bits=np.asarray(field_bits, np.int32))
                        if srows is not None:
                            H, W = slot.mask.shape[1:]
                            extra = dict(extra or {}, event_shape=srows, event_shape_values=dnn.EventShape.values(srows, rows, H, W),
                                         event_shape_value_names=np.frombuffer(",".join(dnn.EVENT_SHAPE_VALUES).encode(), np.uint8).copy())
                    if slot.emask is not None:
                        extra = dict(extra or {}, prediction_ensemble=slot.emask[j].numpy(), ensemble_rows=slot.erows[j].numpy())
                        if slot.econf is not None:
                            extra["confidence_ensemble"] = slot.econf[j].numpy()
                    if slot.dmask is not None:
                        extra = dict(extra or {}, prediction_decided=slot.dmask[j].numpy(), decision=slot.dcounts[j].numpy())
                    if slot.fmask is not None:
                        extra = dict(extra or {}, prediction_filtered=slot.fmask[j].numpy())
                    frames = {key: t[j].numpy() for key, t in slot.frames.items()}
                    if "prob" in frames:                     # the last skill's two: `brier` is stored in the raw rows' place
                        prob_rows, prob_pixels = frames.pop("prob"), frames.pop("prob_pixels")
                        brier = dnn.brier_from_rows(prob_rows, prob_pixels)
                        frames.update(brier=np.asarray([np.nan if v is None else v for v in brier], np.float64), prob_pixels=prob_pixels)
                    if frames:
                        extra = dict(extra or {}, **frames)
                    write_mask_file(os.path.join(out_dir, base), slot.mask[j].numpy(), conf, rows, extra)
                    if plot[j]:
                        png.write_png(os.path.join(out_dir, "plots", plot_name(base)), slot.rgb[j].numpy())
                    rec = {"file": base, "class_counts": [int(v) for v in slot.counts[j].tolist()],
                           "mean_confidence": float(conf.mean(dtype=np.float64)) if conf is not None else None}
                    if plot[j]:
                        rec["plot"] = plot_name(base)
                    if "displacement_best" in frames:
                        rec["displacement_best"] = [[int(v) for v in row] for row in frames["displacement_best"].tolist()]
                    if slot.dcounts is not None:
                        rec["decision"] = [int(v) for v in slot.dcounts[j].tolist()]
                    if slot.fcounts is not None:
                        rec["event_filter"] = [dict(zip(dnn.EVENT_FILTER_COUNTS, (int(v) for v in row))) for row in slot.fcounts[j].tolist()]
                    if rows is not None:
                        rec["events"] = [int((rows[:, 1] == 1).sum()), int((rows[:, 1] == 2).sum())]
                        rec["events_overflowed"] = total > slot.events.shape[1]
                    if extra is not None and "event_fields" in extra:
                        rec["event_field_counts"] = [int(extra["event_fields"][..., 4].sum()), int(extra["event_fields"][..., 5].sum())]
                    if extra is not None and "event_scores" in extra:
                        rec["event_scores"] = extra["event_scores"].tolist()
                        rec["matches_overflowed"] = bool(slot.npairs[j, 1])
                    records.append(rec)
        except BaseException as e:      # surfaces in the main thread; the slots keep circulating so that it cannot block
            errors.append(e)
        finally:
            free_q.put(slot)


def main(pargs) -> dict:
    if not torch.cuda.is_available():
        raise RuntimeError("mlperf_deepcam_amd.predict needs an MI355X: there is no CPU path")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = pargs.batch_size, pargs.height, pargs.width
    if B < 1:
        raise ValueError("--batch_size must be at least 1")
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[pargs.dtype] if pargs.dtype else \
        (torch.float32 if pargs.amp_opt_level == "O0" else torch.bfloat16)
    os.makedirs(pargs.output_dir, exist_ok=True)

    verify = bool(getattr(pargs, "verify", False))
    if verify:
        require_labels(pargs.data_dir)
    dataset = ddata.CamDataset(pargs.data_dir, pargs.stats_file, pargs.channels, allow_uneven_distribution=True, shuffle=False,
                               preprocess=True, labels=verify)
    assert tuple(dataset.data_shape[:2]) == (H, W), "pass --height/--width matching the files"

    net = dnn.DeepLabv3_plus(n_input=len(pargs.channels), n_classes=3, os=16, pretrained=False, rank=0, dtype=dtype, _print=False)
    net.materialize(1, H, W)                      # the arena's owner; the batches run on the Predictor's forward-only engine
    checkpoint = torch.load(pargs.checkpoint, map_location=device, weights_only=False)
    net.load_state_dict(checkpoint["model"] if "model" in checkpoint else checkpoint)
    net.eval()
    layout = "nhwc" if net.engine.x0 is not None else "nchw"
    loader = ddata.InputPipeline(dataset, B, dtype=dtype, device=device, layout=layout, drop_last=False, workers=pargs.max_inter_threads)
    events = bool(pargs.events) or verify or bool(getattr(pargs, "tracks", False))
    # --decision_*: the rule takes the stored logits; everything below, the filter included, takes the decided mask
    decision = decision_options(pargs)
    decide = None
    if decision is not None:
        decide = dnn.DecisionRule(B, H, W, connectivity=pargs.event_connectivity, device=device, **decision)
    # --event_filter: the filter's own catalogue takes the mask as it arrives; everything below takes the filtered one
    efilter = None
    if getattr(pargs, "event_filter", False):
        efilter = dnn.EventFilter(dnn.EventCatalog(B, H, W, connectivity=pargs.event_connectivity, device=device),
                                  min_pixels=pargs.filter_min_pixels, min_area_km2=pargs.filter_min_area_km2,
                                  min_length_km=pargs.filter_min_length_km, min_aspect=pargs.filter_min_aspect)
    # --ensemble_*: the views of every batch pooled into one logits tensor, which then stands where the classifier's stood
    ens_options = ensemble_options(pargs, W, pargs.channels)
    ens = ens_view = ens_sign = None
    if ens_options is not None:
        if layout != "nhwc":
            raise ValueError("--ensemble_* needs the NHWC input pipeline: a --channels count the MFMA stem takes (a multiple of 8 in bf16, of 4 in fp32)")
        ens = dnn.ViewEnsemble(B, H, W, device=device)
        ens_view = torch.empty((B, H, W, len(pargs.channels)), dtype=dtype, device=device)       # every further view, one after the other
        if ens_options["negate"]:
            ens_sign = torch.tensor([-1.0 if c in ens_options["negate"] else 1.0 for c in pargs.channels], dtype=torch.float32, device=device)
        ens_weights = [None if ens_options["margin"] == 1 else dnn.seam_weights(W, s, ens_options["margin"]) for s, _ in ens_options["views"]]
    predictor = dnn.Predictor(net, B, H, W, confidence=pargs.confidence,
                              events=events and not verify and efilter is None and decide is None and ens is None,
                              event_connectivity=pargs.event_connectivity)
    # --verify: the matcher's catalogue of the masks (its side a) is the source of `events`, so that no mask is catalogued twice
    matcher = dnn.EventMatcher(B, H, W, connectivity=pargs.event_connectivity, min_pixels=pargs.min_event_pixels,
                               min_cover=pargs.min_event_cover, device=device) if verify else None
    catalog = matcher.a if verify else predictor.catalog
    predictor.store_logits = predictor.store_logits or decide is not None or ens is not None   # bf16 keeps the logits in registers unless asked
    if events and catalog is None:                # a pooled, decided or filtered mask without --verify: a catalogue of its own for it
        catalog = dnn.EventCatalog(B, H, W, connectivity=pargs.event_connectivity, device=device)
    own_catalog = events and not verify and (efilter is not None or decide is not None or ens is not None)
    event_cap = catalog.cap if events else 0
    eshape = dnn.EventShape(catalog) if getattr(pargs, "event_shape", False) else None
    # --event_fields: every file channel, in physical units, as the input pipeline holds the batch on the device before normalisation
    efields = field_bits = None
    if getattr(pargs, "event_fields", False):
        field_bits = dnn.event_field_bits(dataset.minval, dataset.maxval)
        efields = dnn.EventFields(catalog, loader.cfile, field_bits)

    # --tracks: behind the catalogue of every batch; the batches arrive in the order of the sorted names, one frame per file
    tracker = dnn.EventTracker(catalog, min_pixels=pargs.min_track_pixels) if getattr(pargs, "tracks", False) else None
    # --verify_tracks: a second tracker on the labels' catalogue (the matcher's side b), and the join of the two behind every batch
    truth_tracker = tmatch = None
    if getattr(pargs, "verify_tracks", False):
        truth_tracker = dnn.EventTracker(matcher.b, min_pixels=pargs.min_track_pixels)
        tmatch = dnn.TrackMatcher(matcher, tracker, truth_tracker, min_frames=pargs.min_track_frames, min_cover=getattr(pargs, "min_track_cover", 0.5))
    # --track_fields: the field rows of every batch filed next to the tracker's store, joined with the tracks at the end of the run
    tfields = center = None
    if getattr(pargs, "track_fields", False):
        center = getattr(pargs, "track_center_channel", None)
        if center is not None and not 0 <= int(center) < efields.C:
            raise ValueError(f"--track_center_channel must lie in [0, {efields.C}), got {center}")
        tfields = dnn.TrackFields(tracker, efields)

    # --plots: one panel (the prediction), with --verify two (the prediction above the labels); the range is the stats file's
    renderer = None
    plot_every = max(int(getattr(pargs, "plot_every", 1)), 1)
    if getattr(pargs, "plots", False):
        pc = int(pargs.plot_channel)
        if not 0 <= pc < loader.cfile:
            raise ValueError(f"--plot_channel must lie in [0, {loader.cfile}), got {pc}")
        os.makedirs(os.path.join(pargs.output_dir, "plots"), exist_ok=True)
        renderer = dnn.FrameRenderer(B, H, W, channel=pc, ldc=loader.cfile, lo=float(dataset.minval[pc]), hi=float(dataset.maxval[pc]),
                                     panels=2 if verify else 1, device=device)
    # --climatology: behind every batch; the groups come from the files' names
    clim = clim_truth = None
    if getattr(pargs, "climatology", False):
        clim_by = pargs.climatology_by
        clim_channels = [int(c) for c in pargs.climatology_channels]
        if any(not 0 <= c < loader.cfile for c in clim_channels) or len(clim_channels) > 32:
            raise ValueError(f"--climatology_channels: at most 32 file channels in [0, {loader.cfile}), got {clim_channels}")
        all_bits = dnn.event_field_bits(dataset.minval, dataset.maxval)
        clim_bits = [int(all_bits[c]) for c in clim_channels]
        make = lambda: dnn.Climatology(B, H, W, channels=clim_channels, bits=clim_bits, ldc=loader.cfile,  # noqa: E731
                                       groups=len(dnn.CLIMATOLOGY_GROUPS[clim_by]), device=device)
        clim, clim_truth = make(), make() if verify else None
    # --fss: behind every batch, the prediction side of --verify against the labels
    fss = dnn.FractionsSkill(B, H, W, device=device, **fss_options(pargs)) if getattr(pargs, "fss", False) else None
    # --distance_skill: likewise
    dist = dnn.DistanceSkill(B, H, W, device=device, **distance_options(pargs)) if getattr(pargs, "distance_skill", False) else None
    # --displacement: likewise
    disp = dnn.DisplacementSkill(B, H, W, device=device, **displacement_options(pargs)) if getattr(pargs, "displacement", False) else None
    # --scale_skill: likewise
    scale = dnn.ScaleSkill(B, H, W, device=device, **scale_options(pargs)) if getattr(pargs, "scale_skill", False) else None
    # --prob_skill: behind every batch, the classifier's stored logits against the labels
    prob = None
    if getattr(pargs, "prob_skill", False):
        prob = dnn.ProbabilitySkill(B, H, W, device=device, **prob_options(pargs))
        predictor.store_logits = True              # bf16 keeps the logits in registers unless asked
    frame_skills = [skill for skill in (fss, dist, disp, scale, prob) if skill is not None]
    # --composites: behind every batch, on the catalogue and the field rows of --event_fields
    comp = None
    if getattr(pargs, "composites", False):
        comp_kwargs = composite_options(pargs, loader.cfile, W)
        comp_by = getattr(pargs, "composite_by", COMPOSITE_DEFAULTS["composite_by"])
        comp_bits = [int(v) for v in dnn.composite_bits(dataset.minval, dataset.maxval)[comp_kwargs["channels"]]]
        comp = dnn.StormComposite(efields, bits=comp_bits, **comp_kwargs)
    seen = 0                                       # input files so far, in the order the batches arrive (sorted names)

    free_q: "queue.Queue" = queue.Queue()
    work_q: "queue.Queue" = queue.Queue()
    for _ in range(2):
        free_q.put(_HostSlot(B, H, W, pargs.confidence, event_cap, matcher.pair_cap if verify else 0, efields.C if efields else 0,
                             renderer.P * renderer.Ho if renderer else 0, eshape is not None, efilter is not None, decide is not None,
                             frame_skills, ens is not None))
    records: list = []
    errors: list = []
    writer = threading.Thread(target=_writer, args=(work_q, free_q, pargs.output_dir, records, errors, pargs.min_event_pixels, field_bits),
                              daemon=True)
    writer.start()
    t0 = time.perf_counter()
    try:
        for x, y, names in loader:
            nv = len(names)
            slot = free_q.get()                    # blocks only while the writer still holds BOTH host buffers
            if errors:
                free_q.put(slot)
                break
            mask = predictor(x, n_valid=nv)
            dmask = predictor.mask_buffer          # what everything downstream takes
            logits = predictor.logits_buffer       # ... and what --decision_* and --prob_skill take
            if ens is not None:
                # the identity view's outputs leave first: the further views run through the same predictor and overwrite its buffers
                slot.mask[:nv].copy_(mask, non_blocking=True)
                if slot.conf is not None:
                    slot.conf[:nv].copy_(predictor.confidence, non_blocking=True)
                slot.counts[:nv].copy_(predictor.class_counts, non_blocking=True)
                ens.begin()
                for (shift, flip), weights in zip(ens_options["views"], ens_weights):
                    if shift or flip:
                        dnn.view_input(loader.raw, loader.channels, loader.shift, loader.scale, shift, flip, ens_sign if flip else None, ens_view)
                        predictor(ens_view, n_valid=nv)
                    ens.add(predictor.logits_buffer, shift, flip, weights, n_valid=nv)
                logits = ens.pool()
                dmask, econf, _ = dnn.predict_from_logits(logits, confidence=slot.econf is not None, n_valid=nv)
                slot.emask[:nv].copy_(dmask[:nv], non_blocking=True)
                if econf is not None:
                    slot.econf[:nv].copy_(econf[:nv], non_blocking=True)
                slot.erows[:nv].copy_(ens.frame_rows(), non_blocking=True)
            if decide is not None:
                slot.dmask[:nv].copy_(decide(logits, n_valid=nv), non_blocking=True)
                slot.dcounts[:nv].copy_(decide.counts(), non_blocking=True)
                dmask = decide.mask_buffer
            if efilter is not None:
                slot.fmask[:nv].copy_(efilter(dmask, n_valid=nv), non_blocking=True)
                slot.fcounts[:nv].copy_(efilter.counts(), non_blocking=True)
                dmask = efilter.mask_buffer
            if own_catalog:
                catalog(dmask, n_valid=nv)
            if verify:
                matcher(dmask, y, n_valid=nv)
            for skill in frame_skills:             # the mask skills take the mask, the probabilities' skill the stored logits
                skill(logits if skill is prob else dmask, y, n_valid=nv)
                for key, rows in zip(skill.FRAME_KEYS, skill.frame_rows()):
                    slot.frames[key][:nv].copy_(rows, non_blocking=True)
            if eshape is not None:
                slot.shape[:nv].copy_(eshape(nv).table, non_blocking=True)
            if tracker is not None:
                tracker(dmask, n_valid=nv)
            if tmatch is not None:
                truth_tracker(matcher.mask_b, n_valid=nv)
                tmatch()
            if efields is not None:
                efields(loader.raw, n_valid=nv)     # behind the catalogue's launches, on their stream
                slot.fields[:nv].copy_(efields.table, non_blocking=True)
            if tfields is not None:
                tfields()
            if comp is not None:
                comp(loader.raw, groups=[dnn.climatology_group(name, comp_by) for name in names] + [-1] * (B - nv), n_valid=nv)
            if clim is not None:
                groups = [dnn.climatology_group(name, clim_by) for name in names] + [-1] * (B - nv)
                raw = loader.raw if clim.C else None
                clim(dmask, raw, groups=groups, n_valid=nv)
                if clim_truth is not None:
                    clim_truth(y, raw, groups=groups, n_valid=nv)
            if ens is None:
                slot.mask[:nv].copy_(mask, non_blocking=True)
                if slot.conf is not None:
                    slot.conf[:nv].copy_(predictor.confidence, non_blocking=True)
                slot.counts[:nv].copy_(predictor.class_counts, non_blocking=True)
            if slot.events is not None:
                slot.events[:nv].copy_(catalog.table, non_blocking=True)
                slot.ncomp[:nv].copy_(catalog.counts(), non_blocking=True)
            if slot.pairs is not None:
                slot.truth[:nv].copy_(matcher.b.table, non_blocking=True)
                slot.ntruth[:nv].copy_(matcher.b.counts(), non_blocking=True)
                slot.pairs[:nv].copy_(matcher.pair_table, non_blocking=True)
                slot.npairs[:nv].copy_(matcher.pair_counts, non_blocking=True)
                slot.scores[:nv].copy_(matcher.score_table, non_blocking=True)
            plot = [renderer is not None and (seen + j) % plot_every == 0 for j in range(nv)]
            seen += nv
            if any(plot):
                slot.rgb[:nv].copy_(renderer(loader.raw, dmask, y if verify else None, n_valid=nv), non_blocking=True)
            slot.done.record(torch.cuda.current_stream())
            work_q.put((slot, names, plot))
    finally:
        work_q.put(None)
        writer.join()
        predictor.close()
    if errors:
        raise errors[0]
    verification = matcher.result() if verify else None
    track_rows = tracker.rows() if tracker is not None else None
    truth_track_rows = truth_tracker.rows() if truth_tracker is not None else None
    match_rows = tmatch.rows() if tmatch is not None else None
    cycle_rows = tfields.rows(min_frames=pargs.min_track_frames) if tfields is not None else None
    clim_state = clim.state() if clim is not None else None
    comp_state = comp.state() if comp is not None else None
    fss_state = fss.state() if fss is not None else None
    dist_state = dist.state() if dist is not None else None
    disp_state = disp.state() if disp is not None else None
    scale_state = scale.state() if scale is not None else None
    prob_state = prob.state() if prob is not None else None
    ens_state = ens.state() if ens is not None else None
    elapsed = time.perf_counter() - t0

    records.sort(key=lambda r: r["file"])
    totals = [sum(r["class_counts"][j] for r in records) for j in range(3)]
    summary = {"files": records, "class_counts": totals}
    if events:
        summary["events"] = [sum(r["events"][j] for r in records) for j in range(2)]
        summary["events_overflowed_files"] = sum(1 for r in records if r["events_overflowed"])
    if ens is not None:
        summary["ensemble"] = ensemble_summary(ens_options, ens_state)
    if decide is not None:
        summary["decision"] = decision_summary(decide, records)
    if efilter is not None:
        summary["event_filter"] = dict(efilter.thresholds(), classes=[
            {k: sum(r["event_filter"][j][k] for r in records) for k in dnn.EVENT_FILTER_COUNTS} for j in range(2)])
    if efields is not None:
        summary["event_fields"] = {"channels": efields.C, "scale_bits": [int(v) for v in field_bits],
                                   "nonfinite": sum(r["event_field_counts"][0] for r in records),
                                   "saturated": sum(r["event_field_counts"][1] for r in records)}
    if verify:
        summary["event_verification"] = verification
    if fss is not None:
        summary["fss"] = fss_summary(fss.windows, fss.row_range, W, fss_state)
    if dist is not None:
        summary["distance_skill"] = distance_summary(dist.R, dist.wrap, dist.row_range, H, W, dist_state)
    if disp is not None:
        summary["displacement"] = displacement_summary(disp.R, disp.row_range, H, W, disp_state, [r["displacement_best"] for r in records])
    if scale is not None:
        summary["scale_skill"] = scale_summary(scale.L, scale.origins, scale.row_range, W, scale_state)
    if prob is not None:
        write_datasets(os.path.join(pargs.output_dir, "prob_skill.h5"), prob_arrays(prob.K, prob_state))
        summary["prob_skill"] = prob_summary(prob.K, prob_state)
    if track_rows is not None:
        t_state, t_store, t_of, t_tracks = track_rows
        arrays = {"tracks": t_tracks, "track_events": np.concatenate([t_store, t_of.astype(np.int64)[:, None]], axis=1), "track_state": t_state}
        if cycle_rows is not None:
            arrays.update({"track_step_offsets": cycle_rows["offsets"], "track_steps": cycle_rows["steps"],
                           "track_step_fields": cycle_rows["step_fields"], "track_fields": cycle_rows["track_fields"],
                           "track_cycle_counts": cycle_rows["counts"]})
        if match_rows is not None:
            b_state, b_store, b_of, b_tracks = truth_track_rows
            arrays.update({"truth_tracks": b_tracks, "truth_track_events": np.concatenate([b_store, b_of.astype(np.int64)[:, None]], axis=1),
                           "truth_track_state": b_state, "track_pairs": match_rows["pairs"], "track_cover": match_rows["cover_a"],
                           "truth_track_cover": match_rows["cover_b"], "track_scores": match_rows["scores"],
                           "track_match_state": match_rows["state"]})
            track_dicts = [dnn.EventTracker.decode(st, of, tr, H, W) for st, of, tr in ((t_store, t_of, t_tracks), (b_store, b_of, b_tracks))]
            summary["track_verification"] = dnn.TrackMatcher.summarize(
                match_rows, dnn.TrackMatcher.decode(match_rows["pairs"], *track_dicts, min_frames=1), tmatch.min_frames, tmatch.cover_q)
        write_datasets(os.path.join(pargs.output_dir, "tracks.h5"), arrays)
        summary["tracks"] = track_summary(t_state, t_tracks, pargs.min_track_frames)
        if cycle_rows is not None:
            summary["track_fields"] = track_fields_summary(cycle_rows, H, W, center)
    if renderer is not None:
        summary["plots"] = sum(1 for r in records if "plot" in r)
    if clim is not None:
        arrays = dict(clim_state, bits=np.asarray(clim.bits, np.int32), channels=np.asarray(clim.channels, np.int32))
        truth_maps = None
        if clim_truth is not None:
            truth_state = clim_truth.state()
            arrays.update({"truth_" + k: truth_state[k] for k in ("count", "sum", "n")})
            truth_maps = dnn.Climatology.occurrence(truth_state["frames"], truth_state["count"], H, W)
        write_datasets(os.path.join(pargs.output_dir, "climatology.h5"), arrays)
        maps = dnn.Climatology.occurrence(clim_state["frames"], clim_state["count"], H, W)
        summary["climatology"] = climatology_summary(clim_by, clim_state["frames"], maps, truth_maps, clim.channels)
        if getattr(pargs, "plots", False):
            pictures = climatology_pictures(clim, clim_truth, float(pargs.climatology_contour), clim_by)
            for name, rgb in pictures.items():
                png.write_png(os.path.join(pargs.output_dir, "plots", name), rgb)
            summary["climatology"]["plots"] = sorted(pictures)
    if comp is not None:
        decoded = dnn.StormComposite.decode(*(comp_state[k] for k in dnn.COMPOSITE_KEYS), comp.bits, comp.bin_km)
        arrays = {k: comp_state[k] for k in dnn.COMPOSITE_KEYS}
        arrays.update(decoded, counts=np.asarray([comp_state["counts"][k] for k in dnn.COMPOSITE_COUNTS], np.int64),
                      bits=np.asarray(comp.bits, np.int32), channels=np.asarray(comp.channels, np.int32), edges=comp.edges,
                      group_names=np.frombuffer(",".join(composite_group_names(comp_by, comp.edges)).encode(), np.uint8))
        write_datasets(os.path.join(pargs.output_dir, "composites.h5"), arrays)
        summary["composites"] = composite_summary(comp_by, comp_kwargs, comp_state, decoded)
    with open(os.path.join(pargs.output_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    line = {"samples": len(records), "class_counts": totals, "seconds": round(elapsed, 4),
            "samples_per_second": round(len(records) / elapsed, 3) if elapsed > 0 else None}
    if events:
        line["events"] = summary["events"]
    if verify:
        line["event_verification"] = verification
    if pargs.confidence and records:
        line["mean_confidence"] = float(np.mean([r["mean_confidence"] for r in records]))
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    main(build_parser().parse_args())
