"""The event stream's tracker without a GPU: TrackDefinition (dagr_amd/streaming.py) against the written-out expectations
of tests/stream_track_cases.py, the refusals of track=, the constants against the header, and run_stream.py's flags."""
import os
import re
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from tests import stream_track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_the_definition_gives_every_cases_expected_ids_hits_and_untracked(name):
    case = next(c for c in tc.cases() if c["name"] == name)
    assert len(case["steps"]) == len(case["expect"])
    steps, d = tc.run_definition(case)
    for k, (ids, hits, untracked, _) in enumerate(steps):
        assert ids.dtype == np.int64 and hits.dtype == np.int32 and ids.shape == (case["B"], case["A"])
        tc.check_expectation(case, k, ids, hits, untracked)
    for b, trk in enumerate(d.tracks()):               # the live tracks, sorted by id, say what the slots say
        assert trk.dtype == np.dtype(S.TRACK_DTYPE) and np.all(np.diff(trk["id"]) > 0)
        assert sorted(trk["id"].tolist()) == sorted(d.id[b][d.id[b] != 0].tolist())
        assert np.all(trk["id"] < d.next_id[b])


def test_the_cases_cover_what_they_are_meant_to():
    seen = {}
    for case in tc.cases():
        seen[case["name"]] = tc.run_definition(case)[1].events
    assert seen["spawn-then-match"]["matched"] == 2 and seen["spawn-then-match"]["spawned"] == 2
    assert seen["identical-tracks-lowest-id-and-slot-reuse"]["reused"] == 1
    assert seen["identical-tracks-lowest-id-and-slot-reuse"]["retired"] == 1
    assert seen["age-at-the-limit-survives-one-more-retires"]["retired"] == 1
    assert seen["max-tracks-full-rows-go-untracked"]["untracked"] == 3
    assert seen["more-than-256-eligible-rows"] == dict(matched=256, spawned=256, retired=0, reused=0, untracked=28)
    assert seen["a-zero-area-box-spawns-every-time"]["matched"] == 0
    # the tie inside one thread: slots 0 and 64 hold one box, the lower id in the higher slot; the tail slots 128, 129 live
    two = next(c for c in tc.cases() if c["name"] == "equal-ious-in-one-threads-two-slots-at-130-tracks")
    d = tc.run_definition(two)[1]
    assert (int(d.id[0, 0]), int(d.id[0, 64])) == (131, 65) and np.array_equal(d.box[0, 0], d.box[0, 64])
    assert d.id.shape == (1, 130) and d.id[0, 128:].tolist() == [129, 130] and d.events["reused"] == 1
    many = next(c for c in tc.cases() if c["name"] == "more-than-256-eligible-rows")
    assert many["track"]["max_tracks"] == S.DAGR_TRACK_MAX_TRACKS and many["A"] > S.DAGR_TRACK_MAX_DETS


@pytest.mark.parametrize("max_tracks", [8, 64])
def test_the_random_walk_exercises_every_rule(max_tracks):
    """What the GPU test compares against is not vacuous: matches, retirements, slots taken again and -- with 8 slots --
    untracked rows; some rows fall below min_score, and the lanes differ."""
    case = tc.random_walk(max_tracks)
    assert case["B"] == 3 and case["A"] == 64 and len(case["steps"]) == 40
    assert max(int(s["n_keep"].max()) for s in case["steps"]) <= 40
    steps, d = tc.run_definition(case)
    e = d.events
    assert e["matched"] > 100 and e["retired"] > 10 and e["reused"] > 10 and e["spawned"] > e["reused"]
    assert (e["untracked"] > 100) if max_tracks == 8 else (e["untracked"] == 0)
    assert any(np.any(s["det"][b, :s["n_keep"][b], 4] < 0.1) for s in case["steps"] for b in range(3))
    assert len(set(d.next_id.tolist())) > 1


def test_the_iou_is_fp32_and_exact_on_the_threshold_case():
    iou = S.TrackDefinition.iou
    half = iou((0, 0, 4, 2), (0, 0, 4, 4))
    assert half.dtype == np.float32 and half == np.float32(0.5)
    assert half < np.nextafter(np.float32(0.5), np.float32(1))
    assert np.isnan(iou((5, 5, 5, 5), (5, 5, 5, 5)))
    assert iou((0, 0, 10, 10), (20, 20, 30, 30)) == 0
    # a third is not representable: the result is the fp32 quotient of the fp32 operands
    assert iou((0, 0, 1, 1), (0, 0, 3, 1)) == np.float32(1) / np.float32(3)


def test_track_options_defaults_and_refusals_by_name():
    assert S._track_options(None, "t") is None
    assert S._track_options(True, "t") == dict(iou=float(np.float32(0.3)), max_age_us=20000, min_score=0.0, max_tracks=64)
    got = S._track_options(dict(iou=1, max_age_us=np.int64(0), max_tracks=np.int32(256), min_score=-1), "t")
    assert got == dict(iou=1.0, max_age_us=0, min_score=-1.0, max_tracks=256)
    for bad, name in ((dict(iou=0), "iou"), (dict(iou=1.5), "iou"), (dict(iou=float("nan")), "iou"), (dict(iou="0.3"), "iou"),
                      (dict(iou=True), "iou"), (dict(max_age_us=-1), "max_age_us"), (dict(max_age_us=2.0), "max_age_us"),
                      (dict(min_score=float("nan")), "min_score"), (dict(min_score=None), "min_score"),
                      (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=257), "max_tracks"),
                      (dict(max_tracks=8.0), "max_tracks"), (dict(max_track=8), "max_track"), (False, "track"),
                      ([("iou", 0.3)], "track"), (64, "track")):
        with pytest.raises(ValueError, match=name):
            S._track_options(bad, "EventStream")
    with pytest.raises(ValueError, match="does not track"):
        S.TrackDefinition(2, None)


def test_the_constants_and_the_entry_points_are_the_headers():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for name in ("DAGR_TRACK_MAX_TRACKS", "DAGR_TRACK_MAX_DETS"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(S, name)
    import ctypes
    sig = _lib.SIGNATURES
    assert sig["dagr_stream_track_bytes"] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32])
    assert sig["dagr_stream_t_ref"] == (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64])
    res, args = sig["dagr_stream_track"]
    assert res is ctypes.c_int and len(args) == 15 and args[4] is ctypes.c_float and args[5] is ctypes.c_int64
    assert sig["dagr_stream_track_reset"][1] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_void_p]


def test_run_stream_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    base = ["--steps", "3"]
    a = C.flags("", base, extra=R.stream_options)
    assert a.track is False and R.track_options(a) is None
    a = C.flags("", base + ["--track"], extra=R.stream_options)
    assert R.track_options(a) == {}
    a = C.flags("", base + ["--track", "--track_iou", "0.5", "--track_max_age_us", "3000", "--track_min_score", "0.25",
                            "--max_tracks", "16"], extra=R.stream_options)
    assert R.track_options(a) == dict(iou=0.5, max_age_us=3000, min_score=0.25, max_tracks=16)
    assert S._track_options(R.track_options(a), "t")["max_tracks"] == 16
    with pytest.raises(SystemExit, match="--track_iou needs --track"):
        R.track_options(C.flags("", base + ["--track_iou", "0.5"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="max_tracks"):
        R.track_options(C.flags("", base + ["--track", "--max_tracks", "300"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="iou"):
        R.track_options(C.flags("", base + ["--track", "--track_iou", "0"], extra=R.stream_options))
    names = [n for n, _ in R.TRACK_RECORD_DTYPE]
    from dagr_amd.utils.buffers import DETECTION_DTYPE
    assert R.TRACK_RECORD_DTYPE[:len(DETECTION_DTYPE)] == DETECTION_DTYPE
    assert R.TRACK_RECORD_DTYPE[-2:] == [("track_id", "<u8"), ("hits", "<u4")] and len(set(names)) == len(names)
