"""The event stream's motion model without a GPU: TrackDefinition(motion=) (dagr_amd/streaming.py) on the gap case that
the plain tracker loses, on a hand case for every rule, against the plain definition where the two must agree, and on a
seeded walk that has to exercise every rule; the refusals of motion=; run_stream.py's flags; and what must not change."""
import ctypes
import os
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from tests import stream_motion_cases as mc
from tests import stream_track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
T = mc.T


def _case(name):
    return next(c for c in mc.cases() if c["name"] == name)


def _coast(step, b=0):
    n = int(step["n_coast"][b])
    ids, box, label, age = step["coast"]
    return ids[b, :n].tolist(), box[b, :n], label[b, :n].tolist(), age[b, :n].tolist()


# ------------------------------------------------------------------------------------------------ the gap
def test_a_track_survives_the_gap_with_motion_and_not_without():
    case = _case("the-gap")
    steps, d = mc.run_definition(case)
    seen = [(int(s["ids"][0, 0]), int(s["hits"][0, 0])) for s, c in zip(steps, case["steps"]) if c["n_keep"][0]]
    assert seen == [(1, 1), (1, 2), (1, 3), (1, 4)]
    assert [int(s["n_coast"][0]) for s in steps] == [0, 0, 1, 1, 1, 1, 0, 0]
    for k, x1, age in ((2, 14, 1000), (3, 16, 2000), (4, 18, 3000), (5, 20, 4000)):
        ids, box, label, ages = _coast(steps[k])
        assert ids == [1] and label == [0] and ages == [age]
        assert box[0].tolist() == [x1, 50, x1 + 8, 58], (k, box)
    q = f32(2) / f32(1000)
    assert steps[1]["vel"][0, 0].tolist() == [q, 0, q, 0]                       # 0.002 px / us in x after the first continuation
    assert steps[6]["box"][0, 0].tolist() == [22, 50, 30, 58] and d.events["motion_only"] == 1
    # the same steps through the plain definition: the track is lost and a second id appears
    plain, _ = mc.run_plain(case)
    seen = [(int(ids[0, 0]), int(hits[0, 0])) for (ids, hits, _, _), c in zip(plain, case["steps"]) if c["n_keep"][0]]
    assert seen == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert S.TrackDefinition.iou((22, 50, 30, 58), (12, 50, 20, 58)) == 0


# ------------------------------------------------------------------------------------------------ every hand case
@pytest.mark.parametrize("name", [c["name"] for c in mc.cases() if c["expect"] is not None])
def test_the_definition_gives_every_cases_expected_ids_hits_and_untracked(name):
    case = _case(name)
    assert len(case["steps"]) == len(case["expect"])
    steps, d = mc.run_definition(case)
    for k, s in enumerate(steps):
        assert s["ids"].dtype == np.int64 and s["hits"].dtype == np.int32 and s["box"].dtype == np.float32
        assert s["box"].shape == (case["B"], case["A"], 4) == s["vel"].shape
        tc.check_expectation(case, k, s["ids"], s["hits"], s["untracked"])
        for b in range(case["B"]):                       # a row without a track keeps its own box and has no velocity
            n = min(max(int(case["steps"][k]["n_keep"][b]), 0), case["A"])
            lone = np.flatnonzero(s["hits"][b, :n] <= 1)
            assert np.array_equal(mc.bits(s["box"][b, lone]), mc.bits(case["steps"][k]["det"][b, lone, :4])), (name, k, b)
            assert not s["vel"][b, lone].any(), (name, k, b)
    for b, trk in enumerate(d.tracks()):
        assert trk.dtype == np.dtype(S.TRACK_MOTION_DTYPE) and np.all(np.diff(trk["id"]) > 0)
        assert not d.vel[b][d.id[b] == 0].any()          # a free slot is at rest


def test_the_first_continuation_sets_the_velocity_and_later_ones_blend():
    steps, _ = mc.run_definition(_case("first-continuation-sets-vel-later-ones-blend"))
    q = f32(2) / f32(1000)
    assert not steps[0]["vel"][0, 0].any()                                      # spawned at rest
    assert steps[1]["vel"][0, 0].tolist() == [q, 0, q, 0]                       # vel = q, whatever beta
    # 16 against the prediction 12 + q * 1000 = 14: r = 2, q = 0.002 again, blended in by beta = 0.25
    v2 = f32(q + f32(f32(0.25) * (f32(2) / f32(1000))))
    assert steps[2]["vel"][0, 0].tolist() == [v2, 0, v2, 0] and v2 > q
    pred = f32(f32(16) + f32(v2 * f32(1000)))
    v3 = f32(v2 + f32(f32(0.25) * f32(f32(f32(19) - pred) / f32(1000))))
    assert steps[3]["vel"][0, 0, 0] == v3 and steps[3]["box"][0, 0].tolist() == [19, 50, 27, 58]


def test_beta_zero_freezes_the_velocity_after_the_first_continuation():
    steps, d = mc.run_definition(_case("beta-zero-freezes-the-velocity"))
    q = f32(2) / f32(1000)
    assert [s["vel"][0, 0, 0] for s in steps] == [0, q, q, q] and d.motion == dict(alpha=1.0, beta=0.0)


def test_alpha_one_stores_the_rows_box_bit_for_bit_and_alpha_half_goes_half_way():
    case = _case("alpha-one-stores-the-rows-box")
    steps, _ = mc.run_definition(case)
    for k, s in enumerate(steps):
        assert np.array_equal(mc.bits(s["box"][0, 0]), mc.bits(case["steps"][k]["det"][0, 0, :4])), k
        assert np.array_equal(mc.bits(s["slots"][2][0, 0]), mc.bits(case["steps"][k]["det"][0, 0, :4])), k
    case = _case("alpha-half-stores-between-prediction-and-row")
    steps, _ = mc.run_definition(case)
    for k in (1, 2, 3):
        before, z = steps[k - 1]["slots"], case["steps"][k]["det"][0, 0, :4]
        dt = f32(int(case["steps"][k]["t_ref"][0]) - int(before[1][0, 0]))
        pred = np.array([f32(before[2][0, 0, c] + f32(before[3][0, 0, c] * dt)) for c in range(4)], f32)
        want = np.array([f32(pred[c] + f32(f32(0.5) * f32(z[c] - pred[c]))) for c in range(4)], f32)
        assert np.array_equal(mc.bits(steps[k]["box"][0, 0]), mc.bits(want)), k
        assert not np.array_equal(mc.bits(want), mc.bits(z)), k                 # ... which is not the row's box
        assert np.array_equal(mc.bits(steps[k]["slots"][2][0, 0]), mc.bits(want)), k


def test_two_steps_at_one_instant_leave_the_velocity_and_predict_the_box():
    steps, _ = mc.run_definition(_case("two-steps-at-one-instant"))
    q = f32(2) / f32(1000)
    assert [s["vel"][0, 0, 0] for s in steps] == [0, q, q, q]                   # dt = 0 at the third step: vel stays
    assert steps[2]["box"][0, 0].tolist() == [13, 50, 21, 58] and int(steps[2]["hits"][0, 0]) == 3
    assert steps[3]["box"][0, 0].tolist() == [15, 50, 23, 58]                   # 13 + q * 1000 was the prediction: r = 0


def test_the_coast_list_holds_the_unseen_tracks_only_in_slot_order():
    steps, d = mc.run_definition(_case("coast-list-matched-spawned-retired-and-slot-order"))
    got = [(_coast(s)[0], _coast(s)[3]) for s in steps]
    assert got[0] == ([], [])                                                   # spawned in the step: not coasting
    assert got[1] == ([1, 3], [1000, 1000])                                     # B, D matched, E spawned: A and C coast
    assert got[2] == ([4, 5], [2000, 2000])                                     # A, C retired in the step: D and E coast
    assert got[3] == ([], [])
    assert got[4] == ([6, 2, 7], [1000, 1000, 1000])                            # slot order, not id order
    assert d.id[0].tolist() == [6, 2, 7, 0, 0, 0] and d.events["coasted"] == 7 and d.events["retired"] == 4
    assert _coast(steps[4])[1][:, 0].tolist() == [100, 20, 120]                 # at rest: predicted where they are
    assert [c.dtype for c in d.coasting()] == [np.dtype(S.COAST_DTYPE)] and d.coasting()[0]["id"].tolist() == [6, 2, 7]


def test_a_nan_box_never_matches_and_coasts_as_nan():
    steps, d = mc.run_definition(_case("a-nan-box-never-matches-and-spawns"))
    assert d.events["spawned"] == 3 and _coast(steps[1])[0] == [1] and _coast(steps[2])[0] == [1, 3]
    assert np.isnan(_coast(steps[2])[1][:, 0]).all() and _coast(steps[2])[1][:, 2].tolist() == [8, 8]


def test_lanes_are_independent():
    case = _case("lanes-are-independent")
    steps, d = mc.run_definition(case)
    assert steps[4]["box"][0, 0].tolist() == [26, 50, 34, 58] and int(steps[4]["hits"][0, 0]) == 3
    assert [int(s["n_coast"][1]) for s in steps] == [0] * 5                     # never, then a spawn
    assert [int(s["n_coast"][0]) for s in steps] == [0, 0, 1, 1, 0] and [int(s["n_coast"][2]) for s in steps] == [0, 0, 0, 1, 2]
    # lane 0 alone gives what lane 0 gives here
    alone = S.TrackDefinition(1, case["track"], motion=case["motion"])
    for k, s in enumerate(case["steps"]):
        ids, hits = alone.step(s["det"][:1], s["n_keep"][:1], s["t_ref"][:1])
        assert np.array_equal(ids[0], steps[k]["ids"][0]) and np.array_equal(mc.bits(alone.track_vel[0]), mc.bits(steps[k]["vel"][0]))


def test_a_difference_beyond_2_to_the_24_is_converted_to_the_nearest_even():
    case = _case("a-backwards-clock-beyond-2**24")
    steps, d = mc.run_definition(case)
    want = [-float((1 << 24)), -float((1 << 24) + 4), -float((1 << 25) + 4)]
    vel = f32(2) / f32(1000)
    for b, (gone, dt) in enumerate(zip(mc.BACKWARDS, want)):
        assert np.int64(-gone).astype(f32) == f32(dt) and float(dt) != -gone
        ids, box, _, age = _coast(steps[2], b)
        assert ids == [1] and age == [-gone]
        assert box[0, 0] == f32(f32(12) + f32(vel * f32(dt)))
        assert box[0, 0] != f32(f32(12) + f32(vel * f32(dt + 2 if b < 2 else dt + 4)))        # the next fp32 is another box
        assert steps[3]["vel"][b, 0].tolist() == [vel, 0, vel, 0]               # dt <= 0: the velocity stays


# ------------------------------------------------------------------------------------------------ against the plain definition
@pytest.mark.parametrize("max_tracks", [8, 64])
def test_at_one_shared_instant_the_motion_tracker_is_the_plain_one(max_tracks):
    case = mc.shared_instant(max_tracks)
    assert all(np.all(s["t_ref"] == T) for s in case["steps"]) and case["motion"]["alpha"] == 1.0
    steps, d = mc.run_definition(case)
    plain, p = mc.run_plain(case)
    for k, (s, (ids, hits, untracked, slots)) in enumerate(zip(steps, plain)):
        assert np.array_equal(s["ids"], ids) and np.array_equal(s["hits"], hits), k
        assert np.array_equal(s["untracked"], untracked), k
        m = s["slots"]
        assert np.array_equal(m[0], slots[0]) and np.array_equal(m[6], slots[5]), k
        live = slots[0] != 0
        for a, b in ((m[1], slots[1]), (mc.bits(m[2]), mc.bits(slots[2])), (m[4], slots[3]), (m[5], slots[4])):
            assert np.array_equal(a[live], b[live]), k
        assert not m[3].any(), k                         # no velocity ever
    assert {k: d.events[k] for k in p.events} == p.events and d.events["matched"] > 50 and d.events["motion_only"] == 0
    assert (d.events["untracked"] > 0) == (max_tracks == 8)


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("max_tracks", [8, 64, 130])
def test_the_walk_exercises_every_rule(max_tracks):
    """What the GPU test compares against is not vacuous: matches, spawns, retirements, slots taken again, coasting
    tracks, matches that the unpredicted boxes would not have given, and -- with 8 slots -- untracked rows."""
    case = mc.random_walk(max_tracks)
    assert case["B"] == 3 and case["A"] == 64 and len(case["steps"]) == (24 if max_tracks == 130 else 40)
    assert max(int(s["n_keep"].max()) for s in case["steps"]) <= 64
    steps, d = mc.run_definition(case)
    e = d.events
    print(max_tracks, e)
    for name in ("matched", "spawned", "retired", "reused", "coasted", "motion_only"):
        assert e[name] > 0, (name, e)
    assert (e["untracked"] > 0) if max_tracks == 8 else (e["untracked"] == 0), e
    assert any(np.any(s["det"][b, :s["n_keep"][b], 4] < 0.1) for s in case["steps"] for b in range(3))
    assert len(set(d.next_id.tolist())) > 1
    assert d._used[:, 64:].any() == (max_tracks == 130)          # the crowded walk reaches a thread's second slot register
    if max_tracks != 8:     # with slots to spare the motion model keeps more tracks alive than the plain tracker does
        _, p = mc.run_plain(case)
        assert e["matched"] > p.events["matched"] and e["spawned"] < p.events["spawned"], (e, p.events)
        assert any(np.any(s["vel"] != 0) for s in steps)


# ------------------------------------------------------------------------------------------------ refusals, flags, constants
def test_motion_options_defaults_and_refusals_by_name():
    trk = S._track_options(True, "t")
    assert S._motion_options(None, trk, "t") is None and S._motion_options(None, None, "t") is None
    assert S._motion_options(True, trk, "t") == dict(alpha=1.0, beta=0.25)
    assert S._motion_options(dict(alpha=0.5, beta=np.float32(1)), trk, "t") == dict(alpha=0.5, beta=1.0)
    assert S._motion_options(dict(beta=0), trk, "t") == dict(alpha=1.0, beta=0.0)
    for bad, name in ((dict(alpha=0), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
                      (dict(alpha="1"), "alpha"), (dict(beta=-0.1), "beta"), (dict(beta=float("nan")), "beta"),
                      (dict(beta=1.01), "beta"), (dict(beta=True), "beta"), (dict(gamma=0.1), "gamma"), (False, "motion"),
                      (0.5, "motion")):
        with pytest.raises(ValueError, match=name):
            S._motion_options(bad, trk, "EventStream")
    with pytest.raises(ValueError, match="motion= needs track="):
        S._motion_options(True, None, "EventStream")
    with pytest.raises(ValueError, match="motion= needs track="):
        S.TrackDefinition(2, None, motion=True)
    with pytest.raises(ValueError, match="max_age_us"):
        S._motion_options(True, S._track_options(dict(max_age_us=1 << 24), "t"), "EventStream")
    assert S._motion_options(True, S._track_options(dict(max_age_us=(1 << 24) - 1), "t"), "t") is not None
    assert S._track_options(dict(max_age_us=1 << 24), "t")["max_age_us"] == 1 << 24        # fine without motion
    with pytest.raises(RuntimeError, match="no motion model"):
        S.TrackDefinition(1, True).coasting()


def test_what_must_not_change_has_not():
    assert S._track_options(True, "t") == dict(iou=float(np.float32(0.3)), max_age_us=20000, min_score=0.0, max_tracks=64)
    assert S.TRACK_DTYPE == [("id", "<i8"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("label", "<i4"),
                             ("t_last", "<i8"), ("hits", "<i4")]
    assert S.TRACK_MOTION_DTYPE[:len(S.TRACK_DTYPE)] == S.TRACK_DTYPE
    assert [n for n, _ in S.TRACK_MOTION_DTYPE[len(S.TRACK_DTYPE):]] == ["vx1", "vy1", "vx2", "vy2"]
    assert [n for n, _ in S.COAST_DTYPE] == ["id", "x1", "y1", "x2", "y2", "label", "age_us"]
    d = S.TrackDefinition(1, True)
    assert d.motion is None and not hasattr(d, "vel") and sorted(d.events) == ["matched", "retired", "reused", "spawned", "untracked"]
    assert d.tracks()[0].dtype == np.dtype(S.TRACK_DTYPE)


def test_the_entry_points_and_the_age_bound_are_the_headers():
    assert S.MOTION_MAX_AGE_US == (1 << 24) - 1 == _lib.DEFINES["DAGR_TRACK_CV_MAX_AGE_US"]
    sig = _lib.SIGNATURES
    assert sig["dagr_stream_track_cv_bytes"] == sig["dagr_stream_track_bytes"]
    assert sig["dagr_stream_track_cv_reset"] == sig["dagr_stream_track_reset"]
    res, args = sig["dagr_stream_track_cv"]
    plain = sig["dagr_stream_track"][1]
    assert res is ctypes.c_int and len(args) == 24
    assert args[:7] == plain[:7] and args[7:9] == [ctypes.c_float] * 2 and args[9:15] == plain[7:13]
    assert args[15:22] == [ctypes.c_void_p] * 7 and args[22:] == plain[13:]


def test_run_stream_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    base = ["--steps", "3"]
    a = C.flags("", base + ["--track"], extra=R.stream_options)
    assert a.track_motion is False and R.motion_options(a) is None and R.track_options(a) == {}
    a = C.flags("", base + ["--track", "--track_motion"], extra=R.stream_options)
    assert R.motion_options(a) == {} and R.track_options(a) == {}
    a = C.flags("", base + ["--track", "--max_tracks", "16", "--track_motion", "--track_alpha", "0.5", "--track_beta", "0.1"],
                extra=R.stream_options)
    assert R.motion_options(a) == dict(alpha=0.5, beta=0.1) and R.track_options(a) == dict(max_tracks=16)
    with pytest.raises(SystemExit, match="--track_motion needs --track"):
        R.motion_options(C.flags("", base + ["--track_motion"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="--track_alpha needs --track_motion"):
        R.motion_options(C.flags("", base + ["--track", "--track_alpha", "0.5"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="--track_beta needs --track_motion"):
        R.motion_options(C.flags("", base + ["--track_beta", "0.5"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="alpha"):
        R.motion_options(C.flags("", base + ["--track", "--track_motion", "--track_alpha", "0"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="beta"):
        R.motion_options(C.flags("", base + ["--track", "--track_motion", "--track_beta", "-1"], extra=R.stream_options))
    with pytest.raises(SystemExit, match="max_age_us"):
        R.motion_options(C.flags("", base + ["--track", "--track_motion", "--track_max_age_us", str(1 << 24)],
                                 extra=R.stream_options))
    names = [n for n, _ in R.MOTION_RECORD_DTYPE]
    assert R.MOTION_RECORD_DTYPE[:len(R.TRACK_RECORD_DTYPE)] == R.TRACK_RECORD_DTYPE and len(set(names)) == len(names)
    assert names[len(R.TRACK_RECORD_DTYPE):] == ["tx1", "ty1", "tx2", "ty2", "vx1", "vy1", "vx2", "vy2"]
    assert [n for n, _ in R.COAST_RECORD_DTYPE] == ["step", "lane", "t", "id", "x1", "y1", "x2", "y2", "label", "age_us"]
