"""The stream tracker's second association round without a GPU: TrackDefinition(rescue=) (dagr_amd/streaming.py) on the
flicker that the plain tracker loses, on a hand case for every rule (tests/stream_rescue_cases.py), on the seeded walks, which
have to rescue hundreds of matches and spawn less, and against the definition without the round where no score lies in the
band; the refusals of rescue=; the new entries' signatures; run_stream.py's flags."""
import ctypes
import os
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from tests import stream_rescue_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = rc.T


def _case(name):
    return next(c for c in rc.cases() if c["name"] == name)


def _rows(steps, key, b=0, n=1):
    return [s[key][b, :n].tolist() for s in steps]


# ------------------------------------------------------------------------------------------------ the flicker
@pytest.mark.parametrize("motion", [None, True], ids=["plain", "motion"])
def test_one_id_lives_through_the_flicker_with_rescue_and_two_without(motion):
    case = _case("the-flicker" + ("-with-motion" if motion else ""))
    assert [float(s["det"][0, 0, 4]) for s in case["steps"]] == [float(np.float32(v)) for v in rc.FLICKER_SCORES]
    steps, d = rc.run_definition(case)
    assert _rows(steps, "ids") == [[1]] * 7 and _rows(steps, "hits") == [[k] for k in range(1, 8)]
    assert [int(s["rescued"][0]) for s in steps] == [0, 0, 1, 2, 3, 3, 3]
    assert d.events["retired"] == 0 and d.events["spawned"] == 1 and d.events["rescued"] == 3 and not d.untracked.any()
    # the same steps without the round: the track retires and id 2 spawns in the freed slot
    plain, p = rc.run_definition(case, rescue=None)
    assert _rows(plain, "ids") == [[1], [1], [0], [0], [0], [2], [2]]
    assert _rows(plain, "hits") == [[1], [2], [0], [0], [0], [1], [2]]
    assert p.events["retired"] == 1 and p.rescue is None and "rescued" not in p.events and not hasattr(p, "rescued")
    assert p.id[0].tolist()[:2] == [2, 0]


# ------------------------------------------------------------------------------------------------ every hand case
@pytest.mark.parametrize("name", [c["name"] for c in rc.cases()])
def test_the_definition_gives_every_cases_expected_ids_hits_untracked_and_rescued(name):
    case = _case(name)
    assert len(case["steps"]) == len(case["expect"])
    steps, d = rc.run_definition(case)
    for k, s in enumerate(steps):
        assert s["ids"].dtype == np.int64 and s["hits"].dtype == np.int32 and s["rescued"].dtype == np.int64
        rc.check_expectation(case, k, s["ids"], s["hits"], s["untracked"], s["rescued"])
        if case["motion"]:                              # a row without a track, or with a new one: its own box, at rest
            for b in range(case["B"]):
                n = min(max(int(case["steps"][k]["n_keep"][b]), 0), case["A"])
                lone = np.flatnonzero(s["hits"][b, :n] <= 1)
                assert rc.same(s["box"][b, lone], case["steps"][k]["det"][b, lone, :4]), (name, k, b)
                assert not s["vel"][b, lone].any(), (name, k, b)
    assert d.events["rescued"] == int(d.rescued.sum()) == sum(case["expect"][-1]["rescued"])


def test_the_band_and_the_cap_are_what_the_cases_say_they_are():
    f = np.float32
    edges = _case("the-band-edges")["steps"][1]["det"][0, :, 4]
    assert edges[0] == f(0.5) and edges[1] == f(0.25) and edges[2] < f(0.25) and np.isnan(edges[3])
    assert np.nextafter(edges[2], f(1)) == f(0.25)
    cap = _case("more-than-256-low-rows")
    s = cap["steps"][1]
    assert cap["A"] == 600 and int(s["n_keep"][0]) == 560 and S.DAGR_TRACK_MAX_DETS == 256
    low = np.flatnonzero((s["det"][0, :560, 4] >= f(0.1)) & ~(s["det"][0, :560, 4] >= f(0.5)))
    assert len(low) == 560 and s["det"][0, low[255], :4].tolist() == [940, 900, 948, 908]
    assert s["det"][0, low[256], :4].tolist() == [900, 900, 908, 908]
    steps, d = rc.run_definition(cap)                   # track 1 is live, of the row's label, unmatched and equal to row 257
    assert d.id[0].tolist()[:2] == [1, 2] and d.box[0, 0].tolist() == [900, 900, 908, 908]
    assert d.t_last[0].tolist()[:2] == [T, T + 1000]
    for name, iou in (("the-rounds-own-threshold-refuses", 0.5), ("without-a-threshold-of-its-own-the-trackers-holds", 0.3)):
        c = _case(name)
        v = S.TrackDefinition.iou(c["steps"][1]["det"][0, 0, :4], c["steps"][0]["det"][0, 0, :4])
        assert f(0.3) < v < f(0.5) and rc.run_definition(c)[1].rescue["iou"] == float(f(iou))


# ------------------------------------------------------------------------------------------------ with the motion model
def _all_high(case):
    """The same boxes with every score 0.9, and no second round."""
    steps = [dict(s, det=np.concatenate([s["det"][..., :4], np.full_like(s["det"][..., 4:5], 0.9), s["det"][..., 5:]], -1))
             for s in case["steps"]]
    return dict(case, name=case["name"] + "-all-high", rescue=None, steps=steps)


def test_a_rescued_match_filters_exactly_as_a_round_one_match_does():
    """A box at x = 10, 12, 16, 19 (tests/stream_motion_cases.py: the first continuation sets the velocity, later ones blend
    it) whose first two continuations are RESCUED, and the flicker: against the same boxes with every score high and no
    rescue, everything the steps leave except the counter is the same, bit for bit -- velocities, filtered boxes, slots,
    coast lists -- and the rescued track does not coast."""
    f = np.float32
    moving = rc._case("rescued-continuations-set-and-blend-the-velocity", rc.TRACK, True,
                      [([[rc._box(x, 50, score=s)]], T + 1000 * k) for k, (x, s) in
                       enumerate(((10, 0.9), (12, 0.3), (16, 0.2), (19, 0.9)))],
                      [([[1]], [[k + 1]], [0], [r]) for k, r in enumerate((0, 1, 2, 2))])
    moving["motion"] = True
    for case in (moving, _case("the-flicker-with-motion")):
        steps, d = rc.run_definition(case)
        want, _ = rc.run_definition(_all_high(case), rescue=None)
        for k, (got, ref) in enumerate(zip(steps, want)):
            rc.check_expectation(case, k, got["ids"], got["hits"], got["untracked"], got["rescued"])
            assert rc.same_step({n: v for n, v in got.items() if n != "rescued"}, ref) is None, (case["name"], k)
            assert int(got["n_coast"][0]) == 0, k           # a rescued track does not coast
    steps, _ = rc.run_definition(moving)
    q = f(2) / f(1000)
    v2 = f(q + f(f(0.25) * (f(2) / f(1000))))               # 16 against the prediction 14: r = 2, blended in by beta
    assert steps[1]["vel"][0, 0].tolist() == [q, 0, q, 0] and steps[2]["vel"][0, 0].tolist() == [v2, 0, v2, 0] and v2 > q
    assert steps[2]["box"][0, 0].tolist() == [16, 50, 24, 58] and steps[2]["slots"][3][0, 0, 0] == v2
    # without the round the flicker's track coasts into the dip instead, and retires in it
    assert [int(s["n_coast"][0]) for s in rc.run_definition(_case("the-flicker-with-motion"), rescue=None)[0]][:3] == [0, 0, 1]


def test_an_unmatched_low_row_has_its_own_box_and_no_velocity():
    case = _case("high-rows-pick-first-with-motion")
    s = rc.run_definition(case)[0][1]
    assert s["ids"][0, :2].tolist() == [1, 0]
    assert rc.same(s["box"][0, 1], case["steps"][1]["det"][0, 1, :4]) and not s["vel"][0, 1].any()
    assert s["box"][0, 0].tolist() == [0, 4, 10, 14] and s["vel"][0, 0, 1] == np.float32(4) / np.float32(1000)


# ------------------------------------------------------------------------------------------------ the walks
@pytest.mark.parametrize("max_tracks,motion,iou", rc.WALKS)
def test_the_walks_rescue_hundreds_of_matches_and_spawn_less(max_tracks, motion, iou):
    case = rc.walk(max_tracks, motion, iou)
    assert case["track"]["min_score"] == 0.5 and case["rescue"]["low_score"] == 0.1 and case["rescue"].get("iou") == iou
    _, d = rc.run_definition(case)
    _, p = rc.run_definition(case, rescue=None)
    print(max_tracks, motion, iou, d.events, "plain", p.events)
    assert d.events["rescued"] >= 200, d.events
    assert d.events["spawned"] < p.events["spawned"], (d.events, p.events)
    assert d.events["rescued"] == int(d.rescued.sum()) and (d.rescued > 0).all()


# ------------------------------------------------------------------------------------------------ neutrality
@pytest.mark.parametrize("name", [c["name"] for c in rc.neutral_cases()])
def test_an_empty_band_leaves_every_byte_of_every_step(name):
    case = next(c for c in rc.neutral_cases() if c["name"] == name)
    assert rc.scores_in_band(case, case["rescue"]["low_score"]) == 0
    assert case["rescue"]["low_score"] == -1.0 or rc.scores_in_band(case, -1.0) > 0
    got, d = rc.run_definition(case)
    want, p = rc.run_definition(case, rescue=None)
    for k, (g, w) in enumerate(zip(got, want)):
        assert not g["rescued"].any(), k
        assert rc.same_step({n: v for n, v in g.items() if n != "rescued"}, w) is None, (name, k)
    assert {n: v for n, v in d.events.items() if n != "rescued"} == p.events and d.events["rescued"] == 0


# ------------------------------------------------------------------------------------------------ options, entries, flags
def test_rescue_options_defaults_and_refusals_by_name():
    trk = S._track_options(dict(min_score=0.5), "t")
    f = np.float32
    assert S.RESCUE_DEFAULTS == dict(low_score=0.1, iou=None)
    assert S._rescue_options(None, trk, "t") is None and S._rescue_options(None, None, "t") is None
    assert S._rescue_options(True, trk, "t") == dict(low_score=float(f(0.1)), iou=float(f(0.3)))
    assert S._rescue_options(dict(low_score=0.25, iou=f(0.5)), trk, "t") == dict(low_score=0.25, iou=0.5)
    assert S._rescue_options(dict(iou=1), S._track_options(dict(min_score=0.5, iou=0.7), "t"), "t")["iou"] == 1.0
    assert S._rescue_options(True, S._track_options(dict(min_score=0.5, iou=0.7), "t"), "t")["iou"] == float(f(0.7))
    assert S._rescue_options(dict(low_score=-1), S._track_options(True, "t"), "t")["low_score"] == -1.0
    nan = float("nan")
    for bad, name in ((dict(low=0.1), "'low'"), (dict(low_score=nan), "low_score"), (dict(low_score="0.1"), "low_score"),
                      (dict(low_score=True), "low_score"), (dict(iou=0), "rescue iou"), (dict(iou=1.5), "rescue iou"),
                      (dict(iou=nan), "rescue iou"), (dict(iou="x"), "rescue iou"), (dict(low_score=0.5), "raise track's min_score"),
                      (dict(low_score=0.7), "raise track's min_score"), (False, "rescue"), (0.1, "rescue")):
        with pytest.raises(ValueError, match=name):
            S._rescue_options(bad, trk, "EventStream")
    # as fp32: 0.1 is not below fp32(0.1), though the doubles differ
    with pytest.raises(ValueError, match="low_score"):
        S._rescue_options(dict(low_score=float(f(0.1))), S._track_options(dict(min_score=0.1), "t"), "t")
    with pytest.raises(ValueError, match="raise track's min_score"):          # the default min_score = 0.0: intended
        S._rescue_options(True, S._track_options(True, "t"), "EventStream")
    with pytest.raises(ValueError, match="rescue= needs track="):
        S._rescue_options(True, None, "EventStream")
    with pytest.raises(ValueError, match="rescue= needs track="):
        S.TrackDefinition(2, None, rescue=True)
    d = S.TrackDefinition(2, dict(min_score=0.5), rescue=True)
    assert d.rescue == dict(low_score=float(f(0.1)), iou=float(f(0.3))) and d.rescued.tolist() == [0, 0]
    assert d.rescued.dtype == np.int64 and d.events["rescued"] == 0
    d.rescued[:] = 5
    d.reset()
    assert d.rescued.tolist() == [0, 0]


def test_what_must_not_change_has_not():
    assert S._track_options(True, "t") == dict(iou=float(np.float32(0.3)), max_age_us=20000, min_score=0.0, max_tracks=64)
    assert S.MOTION_DEFAULTS == dict(alpha=1.0, beta=0.25)
    d = S.TrackDefinition(1, True, motion=True)
    assert d.rescue is None and not hasattr(d, "rescued")
    assert sorted(d.events) == ["coasted", "matched", "motion_only", "retired", "reused", "spawned", "untracked"]


def test_the_new_entries_are_their_base_entries_with_three_more_arguments():
    sig = _lib.SIGNATURES
    for base in ("dagr_stream_track", "dagr_stream_track_cv"):
        res, args = sig[base + "_rescue"]
        assert res is ctypes.c_int and args[:-1] == sig[base][1][:-1] + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
        assert args[-1] == sig[base][1][-1]
    assert "dagr_stream_track_rescue_bytes" not in sig and "dagr_stream_track_rescue_reset" not in sig      # the same state


def test_run_stream_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    base = ["--steps", "3"]
    flags = lambda *more: C.flags("", base + list(more), extra=R.stream_options)           # noqa: E731
    a = flags("--track")
    assert a.track_low_score is None and a.track_low_iou is None and R.rescue_options(a) is None
    assert R.rescue_options(flags()) is None
    a = flags("--track", "--track_min_score", "0.5", "--track_low_score", "0.1")
    assert R.rescue_options(a) == dict(low_score=0.1) and R.track_options(a) == dict(min_score=0.5) and R.motion_options(a) is None
    a = flags("--track", "--track_min_score", "0.5", "--track_low_score", "0.2", "--track_low_iou", "0.5", "--track_motion")
    assert R.rescue_options(a) == dict(low_score=0.2, iou=0.5) and R.motion_options(a) == {}
    for argv, why in ((["--track_low_score", "0.1"], "--track_low_score needs --track"),
                      (["--track", "--track_low_iou", "0.5"], "--track_low_iou needs --track_low_score"),
                      (["--track_low_iou", "0.5"], "--track_low_iou needs --track_low_score"),
                      (["--track", "--track_low_score", "0.1"], "raise track's min_score"),
                      (["--track", "--track_min_score", "0.5", "--track_low_score", "0.5"], "raise track's min_score"),
                      (["--track", "--track_min_score", "0.5", "--track_low_score", "nan"], "low_score"),
                      (["--track", "--track_min_score", "0.5", "--track_low_score", "0.1", "--track_low_iou", "0"], "rescue iou"),
                      (["--track", "--track_min_score", "0.5", "--track_low_score", "0.1", "--track_low_iou", "1.5"], "rescue iou")):
        with pytest.raises(SystemExit, match=why):
            R.rescue_options(flags(*argv))
    for flag in ("--track_low_score", "--track_low_iou"):
        assert flag in R.__doc__
