"""The event stream's scorer without a GPU: the numpy definition (dagr_amd/streaming.py: ScoreDefinition) against the
written-out expectations of tests/stream_score_cases.py after every step, the caps, the lanes' independence, the labelled
scene (dagr_amd/utils/synthetic.py: track_scene) under the four trackers, the options and their refusals, score_summary,
the entry points' signatures and scripts/run_stream.py's flags."""
import ctypes
import os
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.utils.synthetic import track_scene
from tests import stream_score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _objects(step, B):
    return [S.objects_from_arrays(int(step["n_objects"][b]), *step["table"][:, b]) for b in range(B)]


@pytest.mark.parametrize("name", [c["name"] for c in sc.cases()])
def test_the_definition_gives_every_cases_expected_matches_flags_counters_and_objects(name):
    case = next(c for c in sc.cases() if c["name"] == name)
    assert len(case["steps"]) == len(case["expect"])
    steps, d = sc.run_definition(case)
    for k, got in enumerate(steps):
        sc.check_expectation(case, k, got["match"], got["flags"], got["counters"], _objects(got, case["B"]))
        for b in range(case["B"]):                  # behind n_gt, and in a skipped lane, the sentinel is still there
            n = min(int(case["steps"][k]["n_gt"][b]), case["G"])
            assert np.all(got["match"][b, max(n, 0):] == sc.SENTINEL) and np.all(got["flags"][b, max(n, 0):] == sc.SENTINEL)
        c = got["counters"]                         # what the counters must satisfy whatever happened
        assert np.array_equal(c["gt"], c["match"] + c["miss"]) and np.array_equal(c["hyp"], c["match"] + c["false_pos"])
        assert np.all(c["kept"] <= c["match"]) and np.all(c["iou_q"] <= c["match"] * S.SCORE_IOU_ONE)


def test_the_hand_cases_exercise_every_rule():
    total = {}
    for case in sc.cases():
        for k, v in sc.run_definition(case)[1].events.items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    caps = sc.run_definition(next(c for c in sc.cases() if c["name"].startswith("300-rows")))[1]
    assert caps.counters["unscored_hyp"].tolist() == [88] and caps.counters["hyp"].tolist() == [2 * S.DAGR_TRACK_MAX_DETS]
    full = sc.run_definition(next(c for c in sc.cases() if c["name"].startswith("1024-objects")))[1]
    assert full.n_objects.tolist() == [S.DAGR_SCORE_MAX_OBJECTS] and full.id[0].tolist() == list(range(1, 1025))


def test_a_skipped_lane_keeps_every_byte():
    case = next(c for c in sc.cases() if c["name"].startswith("a-skipped-lane"))
    steps, _ = sc.run_definition(case)
    assert np.array_equal(steps[1]["table"][:, 1], steps[0]["table"][:, 1])
    assert all(steps[1]["counters"][k][1] == steps[0]["counters"][k][1] for k in S.SCORE_COUNTERS)
    assert not np.array_equal(steps[1]["table"][:, 0], steps[0]["table"][:, 0])


def test_iou_q_counts_exact_units():
    """An IoU of 1 is 2**20 units, 56 / 72 is rint(fp32(56 / 72) * 2**20)."""
    d = S.ScoreDefinition(1, True)
    s = sc.step([[sc.hyp(0, 0, 5), sc.hyp(51, 0, 6)]], [[sc.gt(0, 0, 1), sc.gt(50, 0, 2)]], 4, 4)
    d.step(s["det"], s["n_keep"], s["track_id"], s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"])
    want = (1 << 20) + int(np.rint(np.float32(np.float32(56) / np.float32(72)) * np.float32(1 << 20)))
    assert d.counters["iou_q"].tolist() == [want]
    m = S.score_summary(d.counters, d.objects())["total"]
    assert m["motp"] == want / (1 << 20) / 2 and m["mota"] == 1.0


@pytest.mark.parametrize("max_objects,boxes,iou", [(40, "det", 0.5), (130, "track", 0.3)])
def test_scoring_a_lane_alone_equals_its_part_of_a_joint_run(max_objects, boxes, iou):
    case = sc.walk(max_objects, boxes, iou)
    steps, joint = sc.run_definition(case)
    for b in range(case["B"]):
        alone = S.ScoreDefinition(1, case["score"])
        for k, s in enumerate(case["steps"]):
            m, f = alone.step(s["det"][b:b + 1], s["n_keep"][b:b + 1], s["track_id"][b:b + 1], s["gt_box"][b:b + 1],
                              s["gt_label"][b:b + 1], s["gt_id"][b:b + 1], s["n_gt"][b:b + 1], track_box=s["track_box"][b:b + 1])
            n = int(s["n_gt"][b])
            assert np.array_equal(m[0, :n], steps[k]["match"][b, :n]) and np.array_equal(f[0, :n], steps[k]["flags"][b, :n]), (b, k)
        assert all(alone.counters[name][0] == joint.counters[name][b] for name in S.SCORE_COUNTERS), b
        assert np.array_equal(sc.table(alone)[:, 0], sc.table(joint)[:, b]), b


def test_the_walks_fill_the_table_and_the_two_box_sources_differ():
    """max_objects = 40 is full and leaves identities unscored, 130 has room for all; the motion model's boxes (alpha 0.5)
    give other IoUs than the detections' boxes."""
    small, large = (sc.run_definition(sc.walk(m, "det", 0.5))[1] for m in (40, 130))
    assert small.n_objects.tolist() == [40] * 3 and np.all(small.counters["unscored_gt"] > 0)
    assert np.all(large.n_objects > 64) and np.all(large.n_objects < 130) and not large.counters["unscored_gt"].any()
    other = sc.run_definition(sc.walk(130, "track", 0.5))[1]
    assert not np.array_equal(other.counters["iou_q"], large.counters["iou_q"])
    assert all(v > 0 for v in small.events.values()), small.events
    for d in (large, other):            # (every row of the walk shows an object: with room for all, nothing is a false positive)
        assert all(v > 0 for k, v in d.events.items() if k not in ("unscored_gt", "false_pos")), d.events


def test_the_scene_shows_what_motion_and_rescue_are_for():
    """The committed scene (2 lanes x 12 places x 120 steps; dagr_amd/utils/synthetic.py: track_scene) through the four
    trackers, definitions alone.  `unscored_hyp` is the one counter that cannot be positive here: it needs more than
    DAGR_TRACK_MAX_DETS = 256 rows with an id in one step of one lane, and the plain tracker gives ids to 256 rows a step at
    the most (its own cap); tests/stream_score_cases.py's 300-row case covers it.  The figures themselves go to
    profiles/stream_score.md and are not asserted."""
    scene = sc.scene()
    assert len(scene) == sc.SCENE["steps"] and scene[0]["det"].shape == (sc.SCENE["B"], sc.SCENE["A"], 6)
    for s in scene:                                 # sorted by descending score, as dagr_postprocess leaves the rows
        for b in range(sc.SCENE["B"]):
            assert np.all(np.diff(s["det"][b, :s["n_keep"][b], 4]) <= 0)
    again = track_scene(**sc.SCENE)
    assert all(np.array_equal(u[k], v[k]) for u, v in zip(scene, again) for k in u)             # seeded
    runs = {name: sc.scene_chain(name)[0] for name, _, _ in sc.VARIANTS}
    total = {name: {k: int(v.sum()) for k, v in d.counters.items()} for name, d in runs.items()}
    print(total)
    plain = total["plain"]
    assert all(v > 0 for k, v in plain.items() if k != "unscored_hyp"), plain
    assert plain["unscored_hyp"] == 0
    assert all(v > 0 for v in runs["plain"].events.values()), runs["plain"].events
    assert plain["switch"] >= 10
    assert total["both"]["switch"] * 2 < plain["switch"]
    assert total["rescue"]["miss"] < plain["miss"]


def test_score_options_defaults_and_refusals_by_name():
    trk, mot = S._track_options(True, "t"), S._motion_options(True, S._track_options(True, "t"), "t")
    assert S.SCORE_DEFAULTS == dict(iou=0.5, max_objects=256, boxes="det")
    assert S._score_options(None, trk, None, "t") is None and S._score_options(None, None, None, "t") is None
    assert S._score_options(True, trk, None, "t") == dict(iou=0.5, max_objects=256, boxes="det")
    assert S._score_options(dict(iou=0.3, boxes="track", max_objects=1024), trk, mot, "t") == \
        dict(iou=float(np.float32(0.3)), max_objects=1024, boxes="track")
    for score, track, motion, why in ((True, None, None, "score= needs track="), (dict(iou=0.0), trk, None, "score iou"),
                                      (dict(iou=1.5), trk, None, "score iou"), (dict(iou=float("nan")), trk, None, "score iou"),
                                      (dict(max_objects=0), trk, None, "max_objects"), (dict(max_objects=1025), trk, None, "DAGR_SCORE_MAX_OBJECTS"),
                                      (dict(max_objects=2.5), trk, None, "max_objects"), (dict(boxes="pred"), trk, mot, "score boxes"),
                                      (dict(boxes="track"), trk, None, "needs motion="), (dict(threshold=0.5), trk, None, "no option 'threshold'"),
                                      ("yes", trk, None, "score = 'yes'")):
        with pytest.raises(ValueError, match=why):
            S._score_options(score, track, motion, "who")
    with pytest.raises(ValueError, match="does not score"):
        S.ScoreDefinition(1, None)
    d = S.ScoreDefinition(2, dict(boxes="track"))
    s = sc.step([[sc.hyp(0, 0, 5)]] * 2, [[sc.gt(0, 0, 1)]] * 2, 4, 4)
    with pytest.raises(ValueError, match="track_box"):
        d.step(s["det"], s["n_keep"], s["track_id"], s["gt_box"], s["gt_label"], s["gt_id"])
    with pytest.raises(ValueError, match="DAGR_SCORE_MAX_GT"):
        d.step(s["det"], s["n_keep"], s["track_id"], np.zeros((2, 257, 4), np.float32), np.zeros((2, 257), np.int32),
               np.zeros((2, 257), np.int64), track_box=s["det"][..., :4])
    assert S.DAGR_SCORE_MAX_OBJECTS == 1024 and S.DAGR_SCORE_MAX_GT == 256
    for word in ("CLEAR-MOT", "Bernardin", "greedy", "not a minimum-cost assignment", "py-motmetrics", "IDF1 and HOTA"):
        assert word in S.__doc__, word


def test_score_summary_on_hand_counters():
    c = {k: np.zeros(2, np.int64) for k in S.SCORE_COUNTERS}
    c["gt"][:], c["match"][:], c["miss"][:], c["false_pos"][:], c["switch"][:], c["frag"][:] = [10, 0], [8, 0], [2, 0], [1, 0], [1, 0], [3, 0]
    c["iou_q"][0] = 6 << 20
    table = np.zeros(5, S.SCORE_OBJECT_DTYPE)
    table["present"], table["tracked"] = [10, 10, 10, 5, 5], [8, 7, 2, 1, 5]          # 0.8: mostly tracked; 0.2: mostly lost
    out = S.score_summary(c, [table, np.zeros(0, S.SCORE_OBJECT_DTYPE)])
    a, b, t = out["lanes"][0], out["lanes"][1], out["total"]
    assert a["mota"] == 1 - 4 / 10 and a["motp"] == 6 / 8 and a["precision"] == 8 / 9 and a["recall"] == 8 / 10
    assert (a["mostly_tracked"], a["mostly_lost"], a["objects"], a["switch"], a["frag"]) == (2, 2, 5, 1, 3)
    assert all(np.isnan(b[k]) for k in ("mota", "motp", "precision", "recall")) and b["objects"] == 0
    assert t["mota"] == a["mota"] and t["objects"] == 5 and t["gt"] == 10


def test_the_entry_points_are_declared_as_the_header_states_them():
    sig, V = _lib.SIGNATURES, ctypes.c_void_p
    i32, f32 = ctypes.c_int32, ctypes.c_float
    assert sig["dagr_stream_score_bytes"] == (ctypes.c_size_t, [i32, i32])
    assert sig["dagr_stream_score_reset"] == (ctypes.c_int, [V, ctypes.c_size_t, i32, i32, V])
    assert sig["dagr_stream_score"] == (ctypes.c_int, [V, ctypes.c_size_t, i32, i32, f32, V, V, i32, V, V, V, V, V, V, i32, V, V, V])
    # the tracker's entries are what they were
    assert len(sig["dagr_stream_track"][1]) == 15 and len(sig["dagr_stream_track_cv_rescue"][1]) == 27


def test_run_stream_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    flags = lambda *more: C.flags("", ["--steps", "3"] + list(more), extra=R.stream_options)           # noqa: E731
    assert R.score_options(flags("--track")) is None and R.score_options(flags()) is None
    assert R.score_options(flags("--track", "--track_score")) == {}
    assert R.score_options(flags("--track", "--track_score", "--track_score_iou", "0.3")) == dict(iou=0.3)
    for argv, why in ((["--track_score"], "--track_score needs --track"),
                      (["--track", "--track_score_iou", "0.3"], "--track_score_iou needs --track_score"),
                      (["--track", "--track_score", "--track_score_iou", "0"], "score iou"),
                      (["--track", "--track_score", "--track_score_iou", "1.5"], "score iou")):
        with pytest.raises(SystemExit, match=why):
            R.score_options(flags(*argv))
    a = flags("--track", "--track_score")
    with pytest.raises(SystemExit, match=r"needs a source with labels\(t_step\); SyntheticStream has none"):
        R.score_options(a, R.SyntheticStream(a))

    class Labelled:
        def labels(self, t):
            return None
    assert R.score_options(a, Labelled()) == {}
    for flag in ("--track_score", "--track_score_iou"):
        assert flag in R.__doc__
