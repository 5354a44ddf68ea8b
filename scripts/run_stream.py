#!/usr/bin/env python
"""Play one event sequence through a ``dagr.streaming.EventStream``: a detection every ``--step_us`` microseconds on the
events of the last ``--window_us``.  Every step uploads only the events that arrived since the step before; the window
slides on the device.  The detections are written as ``detections_<sequence>.npy`` with the rows
``run_test_interframe.py`` writes, sorted by timestamp, so ``visualize_detections.py`` draws them.

The sequence is the synthetic stand-in stream the other scripts fall back to (``--stream``, ``--events_per_window`` events
per 50 ms, ``--width`` x ``--height``); ``main(argv, source=...)`` takes any object with ``t_range()`` and
``events(t0, t1)`` (a dict of ``x``, ``y``, ``t``, ``p`` with ``t0 <= t < t1``) -- and, for ``--use_image`` models,
``image_timestamps`` and ``image(i)`` (BGR uint8) -- in its place, as ``visualize_detections.main`` does.  Reading DSEC
files is not part of this script.

``--downsample F``: the source delivers RAW sensor events, in the pixels of a ``--sensor_width`` x ``--sensor_height``
sensor (default ``F * width`` x ``F * height``), and the stream downsamples them ``F`` x ``F`` on the device, as
``scripts/downsample_events.py`` does for the ``events_2x`` files the models read.

``--raw_frames`` (``--use_image`` models): the source's ``image(i)`` is a sensor-size BGR uint8 frame and goes to the stream
as it is (``frame=``); the stream crops, shrinks and scales it on the device (``dagr.streaming.frame_definition``) with the
``--downsample`` factor, or 1 without.  A frame is handed over when the source's frame index changes; every step between
two frames samples the maps the image branch left for the last one.

``--max_lane_events N``: the window holds the newest ``N`` events of the last ``--window_us`` at most, and the stream's
buffers have the constant size ``N``; ``--window_us 0`` then means the model's whole time window, a pure count window.  The
number of events the cap removed is printed with the summary.

``--denoise_us D`` / ``--refractory_us R``: the stream's noise filter, on the device and in front of everything else
(``dagr.streaming``): an event is kept if one of its 8 neighbours saw an event in the last ``D`` microseconds and its own
pixel saw none in the last ``R``.  The number of events the filter removed is printed with the summary.

``--flicker_hz LO HI`` / ``--trail_us T``: the stream's anti-flicker and trail filters, on the device, behind the decoder and
in front of the noise filter (``dagr.streaming``: ``EventStream(flicker=, trail_us=)``): the events of pixels that flicker
at a steady rate between ``LO`` and ``HI`` Hz are removed, and so is an event that follows one of its own polarity on its
pixel by less than ``T`` microseconds.  The rule is this project's statement of two well-known filters, not a vendor's
algorithm.  ``--flicker_pixels N`` lights ``N`` pixels of the synthetic sequence at ``--flicker_pixel_hz`` (default 100) Hz
(``dagr.utils.synthetic.flicker_events``).  The numbers of events either stage removed are printed with the summary.

``--track``: the stream gives every detection a track id on the device (``dagr.streaming``: greedy IoU matching inside a
label against the tracks of the step before), tuned by ``--track_iou``, ``--track_max_age_us``, ``--track_min_score`` and
``--max_tracks``.  ``detections_<sequence>.npy`` stays what it is; a second file ``tracks_<sequence>.npy`` holds the same
rows in the same order with ``track_id`` (``<u8``, 0: no track) and ``hits`` (``<u4``) appended.  The number of distinct ids
and of untracked detections is printed with the summary.

``--track_motion`` (needs ``--track``): the tracker carries a constant-velocity motion model (``dagr.streaming``:
``EventStream(motion=)``), tuned by ``--track_alpha`` (position gain, default 1.0) and ``--track_beta`` (velocity gain,
default 0.25) -- conventions, not measured optima.  Tracks then survive steps in which the detector misses them.
``tracks_<sequence>.npy`` also carries, per row, the track's filtered box (``tx1, ty1, tx2, ty2``) and its velocity in pixels
per microsecond (``vx1, vy1, vx2, vy2``); a third file ``coasting_<sequence>.npy`` holds, per step, the tracks the step did
not see with the boxes they are predicted to have (``step, lane, t, id, x1, y1, x2, y2, label, age_us``).  The number of
coasted track-steps is printed with the summary.

``--track_low_score L`` (needs ``--track`` with a ``--track_min_score`` above ``L``): a second association round
(``dagr.streaming``: ``EventStream(rescue=)``): the detections with a confidence in ``[L, --track_min_score)`` may continue a
track that no confident detection matched, and never start one, so a score that dips for a few steps does not cost the track
its id.  ``--track_low_iou I`` (needs ``--track_low_score``) gives that round an IoU threshold of its own (default:
``--track_iou``).  0.1 for ``L`` and 0.5 for ``--track_min_score`` are ByteTrack's conventions, not measured optima.  The
number of rescued matches is printed with the summary.

``--track_assign optimal`` (needs ``--track``; ``greedy`` is the default rule): the match of every association round is an
optimal one-to-one assignment instead of the greedy walk in score order (``dagr.streaming``: ``EventStream(assign=)``): the
most matches, then the largest sum of IoUs.  It pays where boxes crowd and changes next to nothing elsewhere.  The rule is
named in the summary's tracker line.

``--track_score`` (needs ``--track``): the track ids are scored against labelled boxes on the device (``dagr.streaming``:
``EventStream(score=)``, this project's statement of the CLEAR-MOT counts with a greedy matcher; agreement with another MOT
tool is not claimed).  The source must have ``labels(t_step)``, which returns ``None`` (no labels at this instant) or
``(boxes fp32 [G, 4], labels [G], ids [G])`` for lane 0; the steps with labels are scored.  ``--track_score_iou V`` (needs
``--track_score``) sets the overlap a match needs (default 0.5).  The built-in synthetic sequence has no labels and is
refused.  Id switches, fragmentations, MOTA and MOTP are printed with the summary; the detections written do not change.

``--track_identity`` (needs ``--track_score``): every scored step also counts which object identities overlap which track
ids (``EventStream(identity=)``), and at the end the maximum-weight pairing of identities with track ids gives IDF1, IDP and
IDR (Ristani et al., 2016), printed beside the MOTA summary; agreement with another MOT tool is not claimed.
``--track_identity_max_tracks N`` (needs ``--track_identity``) sizes the table of track ids (default 256, at most 1024): a
track id that finds it full can only count as identity false positives.  The detections written do not change.

``--track_hota`` (implies ``--track_score`` and ``--track_identity``): every scored step is also appended to a log of the
labelled instants on the device (``EventStream(hota=)``), and at the end the log is replayed -- one optimal assignment per
instant, 19 localisation thresholds -- for HOTA, DetA, AssA and LocA (Luiten et al., 2021; this project's integer
statement of it, agreement with TrackEval is not claimed), printed beside MOTA and IDF1.  ``--track_hota_max_instants N``
(needs ``--track_hota``) sizes the log (default 1200, at most 65535); the instants behind it are left out and counted.
The detections written do not change.

``--track_score_every_step`` (needs ``--track_score``): labels arrive far more rarely than steps, so EVERY step is scored,
against the source's labelled keyframes interpolated to the step's own instant on the device (``dagr.streaming``:
``EventStream(labels=)``: linear in x, y, w, h between the two keyframes that bracket the step, the identities both hold --
the reference's inter-frame evaluation; wrong wherever an object's motion is not linear).  The source must also have
``label_instants()``, its labelled instants as sorted int64; the script keeps the store one keyframe ahead of the step --
it pushes ``labels(t_k)`` for every instant up to the first one behind the step -- and the summary says how many steps
were labelled, outside the keyframes, or in a gap.  ``--label_max_gap_us N`` leaves the steps between two keyframes more
than ``N`` microseconds apart unscored; ``--label_min_height V`` / ``--label_min_diag V`` drop interpolated boxes that are
not larger (``filter_small_bboxes``).  HOTA's log holds at most 65535 instants a lane -- about a minute at 1 kHz --, the
rest is counted as left out.  The detections written do not change.

``--decode evt2|evt3``: the step's events are encoded as camera words (``dagr.data.evt.encode_events``, an encoder for
synthetic sources, not a model of any camera) and pushed through ``step_words``; the stream decodes them on the device
(``dagr.streaming``: ``EventStream(decode=)``) in front of the filter, the front and the window.  ``--max_decoded N`` sizes
the decoded events' buffers (default: the worst case of every push).  The decoder's counters are printed with the
summary.  Composes with ``--downsample``, ``--denoise_us``, ``--max_lane_events`` and ``--track``.

``--render DIR``: every ``--render_every``-th step is drawn on the device from the stream's own arrays (``dagr.streaming``:
``EventStream(render=)``, ``render_step()``) -- the window's events (``--render_event_window_us N``: of the last ``N``
microseconds), the step's box outlines and, with ``--track``, the track ids on plates and the trails of the last
``--render_trail`` centres (``--render_id_scale`` sizes the digits) -- on a black base at the model's resolution, and
written as ``DIR/%06d_lane0.png`` through PIL.  The look is this project's own; there is no window display.  The
detections written do not change."""
import os
import time
import types

import numpy as np
import torch

import _common as C
from dagr.data.evt import encode_events
from dagr.streaming import (EventStream, _assign_options, _flicker_options, _identity_options, _motion_options, _rescue_options,
                            _hota_options, _label_options, _map_options, _render_options, _score_options, _track_options, hota_summary,
                            identity_summary,
                            score_summary)
from dagr.utils.buffers import DETECTION_DTYPE, detections_to_records
from dagr.utils.logging import set_up_logging_directory
from dagr.utils import synthetic as syn


def stream_options(p):
    g = p.add_argument_group("event stream")
    g.add_argument("--step_us", type=int, default=1000, help="microseconds between two detections")
    g.add_argument("--window_us", type=int, default=50000, help="length of the sliding event window (0 with "
                   "--max_lane_events: the model's time window)")
    g.add_argument("--max_lane_events", type=int, default=None, help="keep the newest N events of the window at most")
    g.add_argument("--steps", type=int, default=100, help="number of steps to play (synthetic sequence)")
    g.add_argument("--sequence", type=str, default="synthetic_stream", help="name the detections are written under")
    g.add_argument("--downsample", type=int, default=None, help="the source delivers raw sensor events: downsample them "
                   "by this factor on the device")
    g.add_argument("--sensor_width", type=int, default=None, help="sensor width with --downsample (default F * width)")
    g.add_argument("--sensor_height", type=int, default=None, help="sensor height with --downsample (default F * height)")
    g.add_argument("--denoise_us", type=int, default=None, help="noise filter: keep an event only if one of its 8 "
                   "neighbours saw an event in the last D microseconds")
    g.add_argument("--refractory_us", type=int, default=None, help="noise filter: drop an event whose own pixel saw an "
                   "event less than R microseconds ago")
    g.add_argument("--flicker_hz", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="anti-flicker filter: remove "
                   "the events of pixels that flicker at LO..HI Hz")
    g.add_argument("--trail_us", type=int, default=None, help="trail filter: drop an event that follows one of its own "
                   "polarity on its pixel by less than T microseconds")
    g.add_argument("--flicker_pixels", type=int, default=0, help="synthetic sequence: this many pixels flicker")
    g.add_argument("--flicker_pixel_hz", type=int, default=100, help="synthetic sequence: the frequency of --flicker_pixels")
    g.add_argument("--decode", type=str, default=None, choices=("evt2", "evt3"), help="encode the step's events as camera "
                   "words of this format and let the stream decode them on the device")
    g.add_argument("--max_decoded", type=int, default=None, help="with --decode: rows of the decoded events' buffers "
                   "(default: the worst case of every push)")
    g.add_argument("--track", action="store_true", help="give every detection a track id, on the device")
    g.add_argument("--track_iou", type=float, default=None, help="with --track: smallest IoU that continues a track "
                   "(default 0.3)")
    g.add_argument("--track_max_age_us", type=int, default=None, help="with --track: a track unseen for longer is dropped "
                   "(default 20000)")
    g.add_argument("--track_min_score", type=float, default=None, help="with --track: detections below this confidence get "
                   "no id (default 0.0)")
    g.add_argument("--max_tracks", type=int, default=None, help="with --track: tracks held at a time (default 64, at most 256)")
    g.add_argument("--track_motion", action="store_true", help="with --track: a constant-velocity motion model; tracks "
                   "survive a gap and coast")
    g.add_argument("--track_alpha", type=float, default=None, help="with --track_motion: position gain in (0, 1] (default 1.0)")
    g.add_argument("--track_beta", type=float, default=None, help="with --track_motion: velocity gain in [0, 1] (default 0.25)")
    g.add_argument("--track_low_score", type=float, default=None, help="with --track: a second association round lets "
                   "detections with a confidence in [L, --track_min_score) continue a track (never start one)")
    g.add_argument("--track_low_iou", type=float, default=None, help="with --track_low_score: that round's own smallest IoU "
                   "in (0, 1] (default: --track_iou)")
    g.add_argument("--track_assign", default=None, help="with --track: 'optimal' matches every association round by an "
                   "optimal one-to-one assignment, 'greedy' (the default) in score order")
    g.add_argument("--track_score", action="store_true", help="with --track: score the track ids against the source's "
                   "labelled boxes (source.labels), on the device")
    g.add_argument("--track_score_iou", type=float, default=None, help="with --track_score: the IoU a match needs, in "
                   "(0, 1] (default 0.5)")
    g.add_argument("--track_identity", action="store_true", help="with --track_score: IDF1 / IDP / IDR from the maximum-weight "
                   "pairing of object identities with track ids, on the device")
    g.add_argument("--track_identity_max_tracks", type=int, default=None, help="with --track_identity: the size of the table "
                   "of track ids, 1..1024 (default 256)")
    g.add_argument("--track_hota", action="store_true", help="HOTA / DetA / AssA / LocA from a log of the labelled instants "
                   "kept and replayed on the device; implies --track_score and --track_identity")
    g.add_argument("--track_hota_max_instants", type=int, default=None, help="with --track_hota: the labelled instants the "
                   "log holds, 1..65535 (default 1200); those behind it are left out and counted")
    g.add_argument("--track_score_every_step", action="store_true", help="with --track_score: score EVERY step against the "
                   "source's labelled keyframes (source.label_instants), interpolated to the step's instant on the device")
    g.add_argument("--label_max_gap_us", type=int, default=None, help="with --track_score_every_step: no labels between two "
                   "keyframes further apart than this (default: no limit)")
    g.add_argument("--label_min_height", type=float, default=None, help="with --track_score_every_step: drop interpolated "
                   "boxes whose width or height is not above this")
    g.add_argument("--label_min_diag", type=float, default=None, help="with --track_score_every_step: drop interpolated boxes "
                   "whose diagonal is not above this")
    g.add_argument("--map", action="store_true", help="detection mAP over EVERY step: log every step's detections and the "
                   "source's interpolated labels on the device and run the COCO protocol on the log at the end")
    g.add_argument("--map_max_images", type=int, default=None, help="with --map: images the log holds a lane (default 1200)")
    g.add_argument("--raw_frames", action="store_true", help="the source's frames are sensor-size BGR uint8 frames: prepare "
                   "them on the device (crop, shrink by the --downsample factor, / 255)")
    g.add_argument("--render", type=str, default=None, metavar="DIR", help="draw every step on the device -- events, box "
                   "outlines and, with --track, track ids and trails -- and write DIR/%%06d_lane<b>.png")
    g.add_argument("--render_every", type=int, default=1, help="with --render: draw every N-th step")
    g.add_argument("--render_event_window_us", type=int, default=None, help="with --render: draw the events of the last N "
                   "microseconds (default: the whole window)")
    g.add_argument("--render_trail", type=int, default=None, help="with --render --track: centres a trail holds (default "
                   "32, at most 64; 0: no trails)")
    g.add_argument("--render_id_scale", type=int, default=None, help="with --render --track: size of the id digits, 1..4")


TRACK_FLAGS = (("track_iou", "iou"), ("track_max_age_us", "max_age_us"), ("track_min_score", "min_score"),
               ("max_tracks", "max_tracks"))
TRACK_RECORD_DTYPE = DETECTION_DTYPE + [("track_id", "<u8"), ("hits", "<u4")]


def track_options(a):
    """``track=`` of the stream the flags describe: None without ``--track``, else the options that were given."""
    given = {key: getattr(a, flag) for flag, key in TRACK_FLAGS if getattr(a, flag, None) is not None}
    if not getattr(a, "track", False):
        if given:
            raise SystemExit(f"run_stream.py: --{[f for f, k in TRACK_FLAGS if k in given][0]} needs --track")
        return None
    try:
        _track_options(given, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


RENDER_FLAGS = (("render_event_window_us", "event_window_us"), ("render_trail", "trail"), ("render_id_scale", "id_scale"))


def render_options(a):
    """``render=`` of the stream the flags describe: None without ``--render``, else the options that were given."""
    given = {key: getattr(a, flag) for flag, key in RENDER_FLAGS if getattr(a, flag, None) is not None}
    if getattr(a, "render", None) is None:
        if given:
            raise SystemExit(f"run_stream.py: --{[f for f, k in RENDER_FLAGS if k in given][0]} needs --render")
        return None
    if getattr(a, "render_every", 1) < 1:
        raise SystemExit("run_stream.py: --render_every must be positive")
    try:
        _render_options(given or True, track_options(a), "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given or True


def write_frames(directory, step, frames):
    """``DIR/%06d_lane<b>.png`` of a step's BGR frames (RGB on disk), through PIL as visualize_detections.py writes its."""
    from PIL import Image
    for b, frame in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(os.path.join(directory, "%06d_lane%d.png" % (step, b)))


MOTION_FLAGS = (("track_alpha", "alpha"), ("track_beta", "beta"))
MOTION_RECORD_DTYPE = TRACK_RECORD_DTYPE + [(n, "<f4") for n in ("tx1", "ty1", "tx2", "ty2", "vx1", "vy1", "vx2", "vy2")]
COAST_RECORD_DTYPE = [("step", "<u4"), ("lane", "<u4"), ("t", "<u8"), ("id", "<u8"), ("x1", "<f4"), ("y1", "<f4"),
                      ("x2", "<f4"), ("y2", "<f4"), ("label", "<i4"), ("age_us", "<i8")]


def motion_options(a):
    """``motion=`` of the stream the flags describe: None without ``--track_motion``, else the options that were given."""
    given = {key: getattr(a, flag) for flag, key in MOTION_FLAGS if getattr(a, flag, None) is not None}
    if not getattr(a, "track_motion", False):
        if given:
            raise SystemExit(f"run_stream.py: --{[f for f, k in MOTION_FLAGS if k in given][0]} needs --track_motion")
        return None
    if not getattr(a, "track", False):
        raise SystemExit("run_stream.py: --track_motion needs --track")
    try:
        _motion_options(given, _track_options(track_options(a), "run_stream.py"), "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


RESCUE_FLAGS = (("track_low_score", "low_score"), ("track_low_iou", "iou"))


def rescue_options(a):
    """``rescue=`` of the stream the flags describe: None without ``--track_low_score``, else the options that were given."""
    given = {key: getattr(a, flag) for flag, key in RESCUE_FLAGS if getattr(a, flag, None) is not None}
    if "low_score" not in given:
        if given:
            raise SystemExit("run_stream.py: --track_low_iou needs --track_low_score")
        return None
    if not getattr(a, "track", False):
        raise SystemExit("run_stream.py: --track_low_score needs --track")
    try:
        _rescue_options(given, _track_options(track_options(a), "run_stream.py"), "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


def assign_option(a):
    """``assign=`` of the stream the flags describe: None without ``--track_assign``, else what was given."""
    given = getattr(a, "track_assign", None)
    if given is None:
        return None
    if not getattr(a, "track", False):
        raise SystemExit("run_stream.py: --track_assign needs --track")
    try:
        _assign_options(given, _track_options(track_options(a), "run_stream.py"), "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


def score_options(a, source=None):
    """``score=`` of the stream the flags describe: None without ``--track_score``, else the options that were given.  With
    ``source`` the refusal of a source without labels."""
    given = {} if getattr(a, "track_score_iou", None) is None else dict(iou=a.track_score_iou)
    if not getattr(a, "track_score", False):
        if given:
            raise SystemExit("run_stream.py: --track_score_iou needs --track_score")
        return None
    if not getattr(a, "track", False):
        raise SystemExit("run_stream.py: --track_score needs --track")
    try:
        _score_options(given, _track_options(track_options(a), "run_stream.py"), None, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if source is not None and not callable(getattr(source, "labels", None)):
        raise SystemExit(f"run_stream.py: --track_score needs a source with labels(t_step); {type(source).__name__} has none "
                         "(the built-in synthetic sequence carries no labelled boxes)")
    return given


LABEL_FLAGS = (("label_max_gap_us", "max_gap_us"), ("label_min_height", "min_height"), ("label_min_diag", "min_diag"))


def label_options(a, source=None):
    """``labels=`` of the stream the flags describe: None without ``--track_score_every_step``, else the options that were
    given.  With ``source`` the refusal of a source that cannot list its labelled instants."""
    given = {key: getattr(a, flag) for flag, key in LABEL_FLAGS if getattr(a, flag, None) is not None}
    if not getattr(a, "track_score_every_step", False):
        if given:
            raise SystemExit(f"run_stream.py: --{next(f for f, k in LABEL_FLAGS if k in given)} needs --track_score_every_step")
        return None
    if not getattr(a, "track_score", False):
        raise SystemExit("run_stream.py: --track_score_every_step needs --track_score")
    try:
        _label_options(given, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if source is not None and not callable(getattr(source, "label_instants", None)):
        raise SystemExit("run_stream.py: --track_score_every_step needs a source with label_instants() (its labelled "
                         f"instants, sorted int64) besides labels(t); {type(source).__name__} has none")
    return given


def map_options(a, source=None):
    """``map=`` of the stream the flags describe: None without ``--map``, else the options that were given.  With ``source``
    the refusal of a source without labelled keyframes."""
    given = {} if getattr(a, "map_max_images", None) is None else dict(max_images=a.map_max_images)
    if not getattr(a, "map", False):
        if given:
            raise SystemExit("run_stream.py: --map_max_images needs --map")
        return None
    try:
        _map_options(given, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if source is not None and not (callable(getattr(source, "labels", None)) and callable(getattr(source, "label_instants", None))):
        raise SystemExit("run_stream.py: --map needs a source with labels(t) and label_instants() (its labelled instants, "
                         f"sorted int64); {type(source).__name__} lacks one (the built-in synthetic sequence carries no "
                         "labelled boxes)")
    return given


def push_keyframe(stream, source, t):
    """``source.labels(t)`` (x1, y1, x2, y2 boxes of lane 0, or None: a labelled instant with no box) into the stream's
    label store as the keyframe of the instant ``t``."""
    labelled = source.labels(int(t))
    boxes, labels, ids = labelled if labelled is not None else (np.zeros((0, 4)), np.zeros(0), np.zeros(0))
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    xywh = np.concatenate([boxes[:, :2], boxes[:, 2:] - boxes[:, :2]], axis=1)
    stream.push_labels(np.array([int(t)], np.int64), xywh[None], np.asarray(labels, np.int32).reshape(1, -1),
                       np.asarray(ids, np.int64).reshape(1, -1))


def identity_options(a):
    """``identity=`` of the stream the flags describe: None without ``--track_identity``, else the options that were given."""
    given = {} if getattr(a, "track_identity_max_tracks", None) is None else dict(max_tracks=a.track_identity_max_tracks)
    if not getattr(a, "track_identity", False):
        if given:
            raise SystemExit("run_stream.py: --track_identity_max_tracks needs --track_identity")
        return None
    if not getattr(a, "track_score", False):
        raise SystemExit("run_stream.py: --track_identity needs --track_score")
    try:
        _identity_options(given, True, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


def hota_options(a):
    """``hota=`` of the stream the flags describe: None without ``--track_hota``, else the options that were given.
    ``--track_hota`` implies ``--track_score`` and ``--track_identity``: it sets both, so it comes in front of their checks."""
    given = {} if getattr(a, "track_hota_max_instants", None) is None else dict(max_instants=a.track_hota_max_instants)
    if not getattr(a, "track_hota", False):
        if given:
            raise SystemExit("run_stream.py: --track_hota_max_instants needs --track_hota")
        return None
    a.track_score = a.track_identity = True
    try:
        _hota_options(given, True, "run_stream.py")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return given


def motion_records(rec, det):
    """``track_records`` with the step's ``track_boxes`` / ``track_vel`` appended."""
    out = np.zeros(len(rec), MOTION_RECORD_DTYPE)
    for name in rec.dtype.names:
        out[name] = rec[name]
    box, vel = det["track_boxes"].cpu().numpy(), det["track_vel"].cpu().numpy()
    for k, c in enumerate(("x1", "y1", "x2", "y2")):
        out["t" + c], out["v" + c] = box[:, k], vel[:, k]
    return out


def coast_records(step, t, coasting):
    """The coast lists of one step (``EventStream.coasting()``) as ``COAST_RECORD_DTYPE`` rows."""
    out = []
    for lane, c in enumerate(coasting):
        rec = np.zeros(len(c), COAST_RECORD_DTYPE)
        rec["step"], rec["lane"], rec["t"] = step, lane, t
        for name in c.dtype.names:
            rec[name] = c[name]
        out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, COAST_RECORD_DTYPE)


def track_records(rec, det):
    """``rec`` (``detections_to_records`` of ``det``) with the step's ``track_ids`` / ``track_hits`` appended."""
    out = np.zeros(len(rec), TRACK_RECORD_DTYPE)
    for name in rec.dtype.names:
        out[name] = rec[name]
    out["track_id"], out["hits"] = det["track_ids"].cpu().numpy(), det["track_hits"].cpu().numpy()
    return out


def flicker_options(a):
    """``flicker=`` of the stream the flags describe: None without ``--flicker_hz``."""
    hz = getattr(a, "flicker_hz", None)
    return None if hz is None else dict(min_hz=int(hz[0]), max_hz=int(hz[1]))


def sensor_size(a):
    """``(W_in, H_in)`` the flags describe, or None without ``--downsample``."""
    if a.downsample is None:
        if a.sensor_width is not None or a.sensor_height is not None:
            raise SystemExit("run_stream.py: --sensor_width / --sensor_height need --downsample")
        return None
    return (a.sensor_width or a.downsample * a.width, a.sensor_height or a.downsample * a.height)


class SyntheticStream:
    """``--steps`` x ``--step_us`` microseconds of the synthetic stand-in stream, ``events_per_window`` events per 50 ms,
    with absolute timestamps (and one synthetic frame every 50 ms for ``--use_image`` models).  With ``--downsample`` the
    events are drawn over the sensor, ``width`` / ``height`` stay the model's."""

    def __init__(self, a, t0=1 << 33):
        self.duration = max(1, a.steps * a.step_us)
        n = max(1, int(a.events_per_window * self.duration / 50000))
        gen = syn.edges_window if a.stream == "edges" else syn.uniform_window
        self.sensor_width, self.sensor_height = sensor_size(a) or (a.width, a.height)
        x, y, t, p = gen(n, self.sensor_width, self.sensor_height, seed=7, window_us=self.duration, time_window=self.duration)
        t = t.astype(np.int64)
        lights = int(getattr(a, "flicker_pixels", 0) or 0)
        if lights > 0:        # pixels lit by a flickering light, merged into the sequence stably by time
            rng = np.random.Generator(np.random.PCG64(11))
            flat = rng.choice(self.sensor_width * self.sensor_height, lights, replace=False)
            lit = syn.flicker_events(np.stack([flat % self.sensor_width, flat // self.sensor_width], -1),
                                     int(getattr(a, "flicker_pixel_hz", 100)), self.duration, seed=11,
                                     t0=int(t[0]) if len(t) else 0)
            x, y, t, p = (np.concatenate([u, v]) for u, v in zip((x, y, t, p), lit))
            order = np.argsort(t, kind="stable")
            x, y, t, p = x[order], y[order], t[order], p[order]
        self.x, self.y, self.p = x, y, p
        self.t = t + np.int64(t0)
        self.t0, self.width, self.height = int(t0), a.width, a.height
        self.image_timestamps = np.arange(self.t0, self.t0 + self.duration + 1, 50000, dtype=np.int64)
        raw = getattr(a, "raw_frames", False)         # frames as the sensor delivers them
        self.frame_width, self.frame_height = (self.sensor_width, self.sensor_height) if raw else (a.width, a.height)

    def t_range(self):
        return self.t0, self.t0 + self.duration

    def events(self, t0, t1):
        i0, i1 = np.searchsorted(self.t, [t0, t1], side="left")
        return dict(x=self.x[i0:i1], y=self.y[i0:i1], t=self.t[i0:i1], p=self.p[i0:i1])

    def image(self, i):
        rng = np.random.Generator(np.random.PCG64(1000 + int(i)))
        return rng.integers(0, 256, (self.frame_height, self.frame_width, 3), dtype=np.uint8)


def _frame_index(source, t):
    """The index of the newest frame at or before ``t``."""
    ts = np.asarray(source.image_timestamps)
    return int(np.clip(np.searchsorted(ts, t, side="right") - 1, 0, len(ts) - 1))


def _frame(source, t, dev):
    """The newest frame at or before ``t`` as the model's image batch (fp32 [1,3,H,W] in [0,1], RGB)."""
    i = _frame_index(source, t)
    img = np.ascontiguousarray(np.asarray(source.image(i), dtype=np.uint8)[..., ::-1])
    return i, torch.from_numpy(img).to(dev).permute(2, 0, 1).unsqueeze(0).float() / 255.0


def play(a, model, source, dev):
    """One detections list per step: ``[(t_step, detections of lane 0), ...]``."""
    use_image = bool(model.backbone.use_image)
    raw_size = None
    if getattr(a, "raw_frames", False) and use_image:
        h_f, w_f = np.asarray(source.image(0)).shape[:2]
        raw_size = (int(w_f), int(h_f))
    cap = getattr(a, "max_lane_events", None)
    decode = getattr(a, "decode", None)
    hota = hota_options(a)                 # (first: it implies the two flags behind it)
    mapped, labels = map_options(a), label_options(a)
    if mapped is not None and labels is None:
        labels = {}                        # --map alone: the label store with its defaults
    stream = EventStream(model, window_us=a.window_us or None, downsample=a.downsample, sensor_size=sensor_size(a),
                         frame_size=raw_size, frame_bgr=True, max_lane_events=cap,
                         denoise_us=getattr(a, "denoise_us", None), refractory_us=getattr(a, "refractory_us", None),
                         flicker=flicker_options(a), trail_us=getattr(a, "trail_us", None),
                         track=track_options(a), motion=motion_options(a), rescue=rescue_options(a), assign=assign_option(a),
                         score=score_options(a),
                         identity=identity_options(a), hota=hota, labels=labels, map=mapped,
                         decode=decode, max_decoded=getattr(a, "max_decoded", None),
                         t_base=int(source.t_range()[0]) if decode else None,      # (the words' times start at the sequence's)
                         render=render_options(a))
    if stream.render is not None:
        os.makedirs(a.render, exist_ok=True)
    a.stream_rendered = 0 if stream.render is not None else None
    t0, t1 = source.t_range()
    out, last_frame = [], None
    instants, pushed = (np.asarray(source.label_instants(), np.int64), 0) if stream.labels is not None else (None, 0)
    t_encoded = None                       # where the encoder of --decode stands (times relative to the sequence's start)
    a.stream_coasting = [] if stream.motion is not None else None      # per step the tracks it did not see
    for t_step in range(int(t0) + a.step_us, int(t1) + 1, a.step_us):
        ev = source.events(t_step - a.step_us, t_step)
        xy = np.stack([np.asarray(ev["x"], np.int16), np.asarray(ev["y"], np.int16)], -1)
        image = raw = None
        if raw_size is not None:
            i = _frame_index(source, t_step)
            if i != last_frame:
                raw, last_frame = np.asarray(source.image(i), dtype=np.uint8), i
        elif use_image:
            i, frame = _frame(source, t_step, dev)
            if i != last_frame:
                image, last_frame = frame, i
        # every event of the step is older than t_step, the instant the detections are for
        if stream.decode is not None:
            t_rel = np.asarray(ev["t"], np.int64) - int(t0)
            words = encode_events(ev["x"], ev["y"], t_rel, ev["p"], stream.decode, t_prev=t_encoded)
            if len(t_rel):
                t_encoded = int(t_rel[-1])
            det = stream.step_words(words, t_now=t_step, image=image, frame=raw)
        else:
            det = stream.step(xy, np.asarray(ev["t"], np.int64), np.asarray(ev["p"], np.int8), t_now=t_step, image=image,
                              frame=raw)
        out.append((t_step, det[0]))
        if stream.render is not None and (len(out) - 1) % a.render_every == 0:
            write_frames(a.render, len(out) - 1, stream.render_step().cpu().numpy())   # the step's own arrays, on the device
            a.stream_rendered += 1
        if stream.labels is not None:
            # the store stays one keyframe ahead of the step: every labelled instant up to the first one behind t_step
            while pushed < len(instants) and (pushed == 0 or instants[pushed - 1] <= t_step):
                push_keyframe(stream, source, instants[pushed])
                pushed += 1
            if stream.score is not None:
                stream.score_step()             # two launches: the labels at the step's own instant, then the scorer
            if stream.map_options is not None:
                stream.map_step()               # one launch more (two without a scorer): the step goes into the log
        labelled = source.labels(t_step) if stream.score is not None and stream.labels is None else None
        if labelled is not None:                # one more launch, on the step's own device arrays
            boxes, labels, ids = labelled
            stream.score_step(np.asarray(boxes, np.float32).reshape(1, -1, 4), np.asarray(labels, np.int32).reshape(1, -1),
                              np.asarray(ids, np.int64).reshape(1, -1))
        if stream.motion is not None:
            a.stream_coasting.append(coast_records(len(out) - 1, t_step, stream.coasting()))
    a.stream_steps = (stream.frame_steps, stream.held_steps)      # (frame bodies, held bodies) of the run
    a.stream_dropped = int(stream.dropped().sum()) if cap is not None else None
    a.stream_filtered = int(stream.filtered().sum()) if stream.state.noise is not None else None
    a.stream_suppressed = tuple(int(v.sum()) for v in stream.suppressed()) if stream.state.flick is not None else None
    a.stream_decoded = {k: int(v.sum()) for k, v in stream.decode_counts().items()} if stream.decode is not None else None
    a.stream_untracked = int(stream.untracked().sum()) if stream.track is not None else None
    a.stream_rescued = int(stream.rescued().sum()) if stream.rescue is not None else None
    a.stream_assign = stream.assign
    a.stream_score = None
    if stream.score is not None:
        counters = stream.track_score()
        a.stream_score = dict(score_summary(counters, stream.scored_objects())["total"], steps=int(counters["steps"].sum()))
    a.stream_labels = {k: int(v.sum()) for k, v in stream.label_counts().items()} if stream.labels is not None else None
    a.stream_map = stream.map() if stream.map_options is not None else None
    a.stream_identity = identity_summary(stream.identity())["total"] if stream.identity_options is not None else None
    a.stream_hota = hota_summary(stream.hota())["total"] if stream.hota_options is not None else None
    return out


def main(argv=None, model_factory=None, source=None):
    a = C.flags(__doc__, argv, extra=stream_options)
    capped = getattr(a, "max_lane_events", None) is not None
    if capped and a.max_lane_events < 1:
        raise SystemExit("run_stream.py: --max_lane_events must be positive")
    for name in ("denoise_us", "refractory_us"):
        if getattr(a, name, None) is not None and getattr(a, name) < 1:
            raise SystemExit(f"run_stream.py: --{name} must be positive")
    if getattr(a, "trail_us", None) is not None and a.trail_us < 1:
        raise SystemExit("run_stream.py: --trail_us must be positive")
    try:
        _flicker_options(flicker_options(a), None, 1, 1, 1, "run_stream.py --flicker_hz")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if a.step_us <= 0 or a.window_us < 0 or (a.window_us == 0 and not capped):
        raise SystemExit("run_stream.py: --step_us and --window_us must be positive (--window_us 0: the model's time "
                         "window, with --max_lane_events only)")
    if getattr(a, "max_decoded", None) is not None and (getattr(a, "decode", None) is None or a.max_decoded < 1):
        raise SystemExit("run_stream.py: --max_decoded needs --decode and must be positive")
    tracking = track_options(a) is not None
    moving = motion_options(a) is not None
    rescue_options(a)                      # (refusals in front of the model)
    assign_option(a)
    hota_options(a)                        # (in front of the two it implies)
    score_options(a)
    identity_options(a)
    label_options(a)
    map_options(a)
    render_options(a)
    a.batch_size = 1                     # one sequence: one lane
    world, rank, dev = C.distributed()
    torch.manual_seed(42)
    np.random.seed(42)
    if source is None:
        if a.dataset_directory is not None and rank == 0:
            print(f"NOTICE: --dataset_directory {a.dataset_directory}: run_stream.py does not read DSEC files; playing the "
                  "SYNTHETIC stand-in stream instead.", flush=True)
        source = SyntheticStream(a)
    score_options(a, source)               # (a source without labels is refused in front of the model too)
    label_options(a, source)
    map_options(a, source)
    geometry = types.SimpleNamespace(width=int(getattr(source, "width", a.width)), height=int(getattr(source, "height", a.height)))
    args, net = (model_factory or C.build_model)(a, geometry, dev)
    net = net.eval()
    out_dir = set_up_logging_directory("synthetic", a.task, a.output_directory,
                                       exp_name=getattr(a, "exp_name", "run_stream"))
    t_start = time.perf_counter()
    steps = play(a, net, source, dev)
    seconds = time.perf_counter() - t_start
    per_step = [detections_to_records({k: v.cpu() for k, v in det.items()}, np.uint64(t)) for t, det in steps]
    rec = np.concatenate(per_step) if per_step else \
        detections_to_records(dict(boxes=np.zeros((0, 4)), labels=np.zeros(0), scores=np.zeros(0)), 0)
    order = np.argsort(rec["t"], kind="stable")
    rec = rec[order]
    if tracking:        # the same rows in the same order, with the two fields appended
        trk = [track_records(r, det) for r, (_, det) in zip(per_step, steps)]
        if moving:      # ... and the filtered box and the velocity
            trk = [motion_records(r, det) for r, (_, det) in zip(trk, steps)]
        trk = (np.concatenate(trk) if trk else np.zeros(0, MOTION_RECORD_DTYPE if moving else TRACK_RECORD_DTYPE))[order]
    path = None
    if rank == 0:
        out_dir.mkdir(parents=True, exist_ok=True)
        path = out_dir / f"detections_{a.sequence}.npy"
        np.save(path, rec)
        window = f"a {a.window_us} us window" if a.window_us else "the model's time window"
        if capped:
            window += f" capped at {a.max_lane_events} events ({a.stream_dropped} dropped by the cap)"
        if a.stream_filtered is not None:
            window += f" behind the noise filter ({a.stream_filtered} events filtered)"
        if a.stream_suppressed is not None:
            window += (f" behind the flicker / trail filters ({a.stream_suppressed[0]} flicker events, "
                       f"{a.stream_suppressed[1]} trail events suppressed)")
        if a.stream_decoded is not None:
            c = a.stream_decoded
            window += (f" decoded from {a.decode} words ({c['decoded']} events decoded, {c['unsynced']} unsynced, "
                       f"{c['outside']} outside, {c['skipped']} words skipped)")
        tracked = ""
        if tracking:
            np.save(out_dir / f"tracks_{a.sequence}.npy", trk)
            ids = np.unique(trk["track_id"])
            tracked = (f"; {len(ids[ids != 0])} distinct track ids, {a.stream_untracked} detections untracked -> "
                       f"{out_dir / f'tracks_{a.sequence}.npy'}")
        if moving:
            coast = np.concatenate(a.stream_coasting) if a.stream_coasting else np.zeros(0, COAST_RECORD_DTYPE)
            np.save(out_dir / f"coasting_{a.sequence}.npy", coast)
            tracked += f"; {len(coast)} coasted track-steps -> {out_dir / f'coasting_{a.sequence}.npy'}"
        if a.stream_rescued is not None:
            tracked += f"; {a.stream_rescued} low-score detections rescued by the second round"
        if a.stream_assign is not None:
            tracked += f"; every round matched by an {a.stream_assign} assignment"
        if a.stream_score is not None:
            c = a.stream_score
            tracked += (f"; scored {c['steps']} labelled steps: {c['objects']} objects, {c['switch']} id switches, "
                        f"{c['frag']} fragmentations, {c['miss']} misses, {c['false_pos']} false positives, MOTA "
                        f"{c['mota']:.3f}, MOTP {c['motp']:.3f}, {c['mostly_tracked']} mostly tracked, {c['mostly_lost']} "
                        "mostly lost")
        if getattr(a, "stream_labels", None) is not None:
            c = a.stream_labels
            what = "scored" if a.stream_score is not None else "logged"
            tracked += (f"; every step {what} against {c['keyframes']} resident keyframes, interpolated: {c['labelled']} steps "
                        f"labelled, {c['outside']} outside the keyframes, {c['gap']} in a gap")
        if getattr(a, "stream_identity", None) is not None:
            c = a.stream_identity
            tracked += (f"; IDF1 {c['idf1']:.3f}, IDP {c['idp']:.3f}, IDR {c['idr']:.3f} (IDTP {c['idtp']} of {c['gt_frames']} "
                        f"labelled and {c['hyp_frames']} tracked frames, {c['objects']} objects, {c['tracks']} tracks)")
        if getattr(a, "stream_rendered", None) is not None:
            tracked += f"; {a.stream_rendered} frames drawn on the device -> {a.render}"
        if getattr(a, "stream_hota", None) is not None:
            c = a.stream_hota
            tracked += (f"; HOTA {c['hota']:.3f}, DetA {c['deta']:.3f}, AssA {c['assa']:.3f}, LocA {c['loca']:.3f} "
                        f"({c['instants']} logged instants, {c['dropped_instants']} left out)")
        print(f"{len(steps)} steps of {a.step_us} us on {window} in {seconds:.2f} s "
              f"({1e3 * seconds / max(1, len(steps)):.2f} ms per step; {a.stream_steps[0]} with the full window, "
              f"{a.stream_steps[1]} on held image maps) -> {path}: {len(rec)} detections{tracked}")
        if getattr(a, "stream_map", None) is not None:
            c = a.stream_map
            print(", ".join(f"{k} {float(c[k]):.4f}" for k in ("AP", "AP_50", "AP_75", "AP_S", "AP_M", "AP_L"))
                  + f" over {int(c['images'].sum())} logged steps ({int(c['dropped_images'].sum())} dropped, "
                  f"{int(c['unlabelled'].sum())} without labels, {int(c['empty'].sum())} without a box, "
                  f"{int(c['cut_dets'].sum())} detections cut)")
    C.finish(world)
    return path


if __name__ == "__main__":
    main()
