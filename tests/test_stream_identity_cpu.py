"""The identity state's definition (dagr_amd/streaming.py: IdentityDefinition, identity_summary) without a GPU: the
hand-built cases of tests/stream_identity_cases.py against their written-out tables, the rules the cases exercise, the two
scenes of the GPU tests, and the options' refusals."""
import numpy as np
import pytest

from dagr_amd import streaming as S
from dagr_amd.streaming import IdentityDefinition, check_identity, identity_summary
from tests import stream_identity_cases as ic


@pytest.mark.parametrize("name", [c["name"] for c in ic.cases()])
def test_the_definition_gives_the_written_out_tables(name):
    case = next(c for c in ic.cases() if c["name"] == name)
    _, d, result = ic.run_definition(case)
    ic.check_expectation(case, ic.tables(d), result)
    for b in range(case["B"]):
        assert check_identity(d.overlap[b], d.track_id[b], result, b) is None, (name, b)
        assert result["idfn"][b] == result["gt_frames"][b] - result["idtp"][b]
        assert result["idfp"][b] == result["hyp_frames"][b] - result["idtp"][b]
        # a table word is a sum of its pairs: no object and no track shares more frames than it has
        assert (d.overlap[b].sum(1) >= 0).all() and (d.overlap[b].max(1) <= d.obj_len[b]).all()
        assert (d.overlap[b].max(0) <= d.track_len[b]).all()


def test_the_cases_exercise_every_rule():
    events = {}
    for case in ic.cases():
        for k, v in ic.run_definition(case)[1].events.items():
            events[k] = events.get(k, 0) + v
    assert set(events) == {"pairs", "duplicates", "unlisted", "new_columns", "rows_skipped", "lanes_skipped", "label_mismatch",
                           "nan_iou", "shared_hyp"}
    assert all(v > 0 for v in events.values()), events


def test_the_summary():
    result = {k: np.array(v, np.int64) for k, v in dict(idtp=[6, 0], idfn=[4, 0], idfp=[2, 3], gt_frames=[10, 0],
                                                        hyp_frames=[8, 3], n_objects=[2, 0], n_tracks=[3, 1], dup_hyp=[0, 0],
                                                        unlisted_hyp=[0, 0]).items()}
    m = identity_summary(result)
    assert m["lanes"][0]["idf1"] == 12 / 18 and m["lanes"][0]["idp"] == 6 / 8 and m["lanes"][0]["idr"] == 0.6
    assert m["lanes"][1]["idf1"] == 0.0 and m["lanes"][1]["idp"] == 0.0 and np.isnan(m["lanes"][1]["idr"])
    assert m["total"]["idf1"] == 12 / 21 and m["total"]["idtp"] == 6 and m["total"]["objects"] == 2 and m["total"]["tracks"] == 4
    empty = identity_summary({k: np.zeros(1, np.int64) for k in S.IDENTITY_RESULT})
    assert all(np.isnan(empty["total"][k]) for k in ("idf1", "idp", "idr"))


@pytest.mark.parametrize("variant", [v[0] for v in ic.sc.VARIANTS])
def test_the_scene_has_a_right_solve(variant):
    d, shots, result = ic.scene_chain(variant)
    assert [k for k, _ in shots] == [24, 49, 74, 99, 124, 149]
    for b in range(ic.SCENE["B"]):
        assert check_identity(d.overlap[b], d.track_id[b], result, b) is None
        assert 0 < result["idtp"][b] <= min(result["gt_frames"][b], result["hyp_frames"][b])
    m = identity_summary(result)["total"]
    print(variant, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in m.items()}, d.events)
    assert 0 < m["idf1"] <= 1


def test_the_crossing_scene_crosses_the_boundaries():
    steps, s, d, shots, result = ic.crossing()
    c = ic.CROSSING
    assert d.words["n_tracks"].tolist() == [8, 8] and d.words["n_objects"].tolist() == [16, 16]
    assert d.words["steps"].tolist() == [c["steps"], c["steps"] - 1]
    assert all(d.events[k] > 0 for k in ("pairs", "duplicates", "unlisted", "new_columns", "rows_skipped", "lanes_skipped",
                                         "label_mismatch")), d.events
    assert (s.counters["unscored_gt"] > 0).all() and (s.id[:, 15] > 100 * np.arange(2) + 64).all()      # a slot for a row >= 64
    assert d.overlap.sum() == d.words["pairs"].sum() > 20
    for b in range(c["B"]):
        assert check_identity(d.overlap[b], d.track_id[b], result, b) is None
        assert result["idtp"][b] > 0


def test_the_options_are_refused_by_name():
    for kw, text in ((dict(identity=dict(max_tracks=0)), "max_tracks"), (dict(identity=dict(max_tracks=1025)), "DAGR_ASSIGN_MAX"),
                     (dict(identity=dict(max_tracks=2.0)), "max_tracks"), (dict(identity=dict(tracks=3)), "tracks"),
                     (dict(identity="yes"), "identity"), (dict(identity=None), "identity = None"),
                     (dict(score=None), "score = None"), (dict(score=dict(iou=2.0)), "score iou")):
        with pytest.raises(ValueError, match=text):
            IdentityDefinition(1, **kw)
    with pytest.raises(ValueError, match="identity= needs score="):
        S._identity_options(True, None, "test")
    assert S._identity_options(None, None, "test") is None
    assert S._identity_options(True, S._score_options(True, True, None, "test"), "test") == dict(max_tracks=256)
    d = IdentityDefinition(1, dict(max_tracks=3), dict(max_objects=2))
    assert d.overlap.shape == (1, 2, 3) and d.overlap.dtype == np.int32 and d.track_id.shape == (1, 3)
    with pytest.raises(ValueError, match="score_ids"):
        d.step(np.zeros((1, 4, 6), np.float32), [0], np.zeros((1, 4), np.int64), np.zeros((1, 2, 4), np.float32),
               np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int64), [2], np.zeros((1, 2), np.int64), np.zeros((1, 5), np.int64))
