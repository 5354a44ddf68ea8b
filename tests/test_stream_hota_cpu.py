"""HOTA's definition without a GPU (dagr_amd/streaming.py: HotaDefinition, hota_summary, _hota_options): the hand-built
cases against numbers worked out on paper; the definition against the float restatement of the paper's algorithm
(tests/stream_hota_cases.hota_float, scipy's assignment) on the labelled scenes -- the counts and the mc tables integer for
integer, DetA / AssA to a sum's rounding, LocA to the quantisation --; the scene that crosses the boundaries; the refusals."""
import numpy as np
import pytest

from dagr_amd import streaming as S
from dagr_amd.streaming import HotaDefinition, hota_summary
from tests import stream_hota_cases as hc


@pytest.mark.parametrize("name", [c["name"] for c in hc.cases()])
def test_the_hand_built_cases_give_the_numbers_worked_out_on_paper(name):
    case = next(c for c in hc.cases() if c["name"] == name)
    h, result = hc.run_definition(case)
    hc.check_expectation(case, h.words, result)


def test_the_hand_built_cases_exercise_every_rule():
    events = {}
    for case in hc.cases():
        for k, v in hc.run_definition(case)[0].events.items():
            events[k] = events.get(k, 0) + v
    for name in ("logged", "dropped", "lanes_skipped", "no_rows", "no_columns", "label_mismatch", "nan_iou", "matched"):
        assert events[name] > 0, (name, events)


def test_an_iou_of_exactly_one_half_has_its_last_tp_at_k_10():
    case = next(c for c in hc.cases() if c["name"].startswith("an-iou-of-exactly"))
    h, result = hc.run_definition(case)
    q, w = h.weights(0, h.log[0][0])
    assert q.tolist() == [[1 << 19]] and w.tolist() == [[1 << 29]]          # gq = 2**20: the pair is all there is
    total = hota_summary(result)["total"]
    assert total["alphas"]["deta"] == [1.0] * 10 + [0.0] * 9 and total["alphas"]["loca"][:10] == [0.5] * 10
    assert all(np.isnan(v) for v in total["alphas"]["loca"][10:]) and total["loca"] == 0.5
    assert abs(total["hota"] - 10 / 19) < 1e-15


def test_the_summary_sums_the_lanes_before_it_divides():
    case = next(c for c in hc.cases() if c["name"].startswith("a-skipped-lane"))
    _, result = hc.run_definition(case)
    s = hota_summary(result)
    assert [lane["tp"][0] for lane in s["lanes"]] == [2, 1] and s["total"]["tp"] == [3] * 19
    assert s["total"]["instants"] == 3 and s["total"]["dropped_instants"] == 0
    assert s["total"]["hota"] == 1.0 and all(lane["hota"] == 1.0 for lane in s["lanes"])


@pytest.mark.parametrize("variant", sorted(hc.SCENES))
def test_the_definition_equals_the_float_restatement_on_the_labelled_scenes(variant):
    """Seed 4 (tests/stream_hota_cases.SCENES), plain and motion= + rescue=.  On the float side alone: no similarity within
    2**-19 of a threshold, and scipy's pairing is the definition's at EVERY instant.  Then tp, fn, fp and the mc tables are
    equal integer for integer, DetA and AssA to (pairs + 2) * 2**-52 relative, LocA to 2**-21."""
    h, _, result, pairings = hc.scene_chain(variant)
    M, T = h.score["max_objects"], h.identity["max_tracks"]
    ref = hc.hota_float(h.log, M, T)
    assert ref["near"] >= 2.0 ** -19, ref["near"]
    instants = 0
    for b in range(h.B):
        assert len(ref["pairing"][b]) == len(pairings[b]) == h.words["instants"][b]
        for t, (want, got) in enumerate(zip(ref["pairing"][b], pairings[b])):
            assert np.array_equal(want, got), (variant, b, t, want, got)
            instants += 1
    assert instants == 2 * hc.SCENES[variant]["steps"] and h.events["dropped"] == 0 and h.events["matched"] > 0
    for name in ("tp", "fn", "fp"):
        assert np.array_equal(result[name], ref[name]), (variant, name)
    assert np.array_equal(result["mc"], ref["mc"]), variant
    lanes = hota_summary(result)["lanes"]
    for b in range(h.B):
        tol = (ref["pairs"][b] + 2) * 2.0 ** -52
        got = {name: np.asarray(lanes[b]["alphas"][name]) for name in ("deta", "assa", "loca")}
        assert np.all(np.abs(got["deta"] - ref["deta"][b]) <= tol * ref["deta"][b]), (variant, b)
        assert np.all(np.abs(got["assa"] - ref["assa"][b]) <= tol * ref["assa"][b]), (variant, b)
        has_tp = result["tp"][b] > 0
        assert np.array_equal(np.isnan(got["loca"]), ~has_tp) and np.array_equal(np.isnan(ref["loca"][b]), ~has_tp)
        assert np.all(np.abs(got["loca"][has_tp] - ref["loca"][b][has_tp]) <= 2.0 ** -21), (variant, b)
    print(variant, {k: round(v, 4) for k, v in hota_summary(result)["total"].items() if isinstance(v, float)}, h.events)


def test_the_alignment_score_decides_a_pairing_somewhere():
    """The matching is on alignment x similarity: at some instant of the scenes the pairing on the similarity alone is
    another one."""
    assert sum(hc.scene_chain(v)[0].events["alignment_decides"] for v in hc.SCENES) > 0


def test_the_scene_that_crosses_the_boundaries_fills_its_log_and_runs_both_orientations():
    c = hc.CROSSING
    _, h, shots, solves = hc.crossing()
    assert len(shots) == c["steps"] and sorted(solves) == list(c["solve_at"])
    assert h.words["instants"].tolist() == [4, 4] and h.words["dropped_instants"].tolist() == [8, 7]
    assert h.events["lanes_skipped"] == 1 and h.events["tall"] > 0 and h.events["matched"] > 0
    first, last = solves[c["solve_at"][0]], solves[c["solve_at"][-1]]
    assert first["instants"].tolist() == [3, 3] and last["instants"].tolist() == [4, 4]
    assert (last["tp"] + last["fn"] == h.words["rows"][:, None]).all() and (last["tp"] + last["fp"] == h.words["columns"][:, None]).all()
    assert (np.diff(last["tp"], axis=1) <= 0).all() and last["tp"][:, 0].min() > 0
    _, hw, _, solved = hc.wide()
    assert hw.events["wide"] > 0 and hw.events["tall"] > 0 and hw.events["alignment_decides"] >= 0
    assert max(len(e["slot"]) for e in hw.log[0]) > 64 and max(len(e["col"]) for e in hw.log[0]) > 64
    assert solved["tp"][0, 0] > 64


def test_a_solve_changes_no_table_and_can_be_repeated():
    case = next(c for c in hc.cases() if c["name"].startswith("an-id-switch"))
    _, _, h, _, _ = hc.chain(case["B"], case["steps"])
    before = hc.tables(h)
    a, b = h.solve(), h.solve()
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    after = hc.tables(h)
    assert all(np.array_equal(before[k], after[k]) for k in ("pmc", "gc", "tc"))
    h.reset()
    assert not h.pmc.any() and not h.solve()["tp"].any() and h.log == [[]]


def test_the_options_are_refused_by_name():
    for kw, text in ((dict(hota=True, identity=None), "hota= needs identity="),
                     (dict(hota=dict(max_instants=0)), "hota max_instants"),
                     (dict(hota=dict(max_instants=65536)), "DAGR_HOTA_MAX_INSTANTS"),
                     (dict(hota=dict(max_instants=2.5)), "hota max_instants"),
                     (dict(hota=dict(instants=4)), "instants"), (dict(hota="yes"), "hota"),
                     (dict(hota=None), "hota = None")):
        with pytest.raises(ValueError, match=text):
            HotaDefinition(1, **kw)
    assert S._hota_options(None, None, "t") is None
    assert S._hota_options(True, dict(max_tracks=4), "t") == dict(max_instants=1200)
    assert S._hota_options(dict(max_instants=65535), dict(max_tracks=4), "t") == dict(max_instants=65535)
    assert S.HOTA_THRESHOLDS == 19 and S.DAGR_HOTA_MAX_INSTANTS == 65535
