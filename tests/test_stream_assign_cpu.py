"""The stream tracker's optimal assignment on the CPU: TrackDefinition(assign="optimal") (dagr_amd/streaming.py) against
the hand cases of tests/stream_assign_cases.py, against a brute force over every partial matching of small rounds, against
the greedy definition where nothing is contested, and on the crowded scene; the two counters; the refusals by name."""
import itertools

import numpy as np
import pytest

from dagr_amd.streaming import (ASSIGN_IOU_ONE, ASSIGN_ONE, TrackDefinition, _assign_options, _track_options,
                                assign_max_weight_definition)
from tests import stream_assign_cases as ac
from tests import stream_rescue_cases as rc


@pytest.mark.parametrize("name", [c["name"] for c in ac.cases() if c["expect"] is not None])
def test_the_hand_cases_leave_what_is_written_out(name):
    """ids, hits, untracked and rescued after every step are the case's expectation; where the case is about the difference,
    the greedy definition leaves the ids the case says IT leaves."""
    case = next(c for c in ac.cases() if c["name"] == name)
    steps, d = ac.run_definition(case)
    for k, o in enumerate(steps):
        ac.check_expectation(case, k, o["ids"], o["hits"], o["untracked"], o.get("rescued"))
    if case["greedy"] is not None:
        greedy, g = ac.run_definition(case, assign=None)
        for k, o in enumerate(greedy):
            for b, want in enumerate(case["greedy"][k]):
                assert o["ids"][b, :len(want)].tolist() == want, (name, k, b)
        assert d.events["reassigned"] > 0 and d.events["conflicts"] >= d.events["reassigned"], d.events
        assert "conflicts" not in g.events and "reassigned" not in g.events and not hasattr(g, "rounds")


def test_the_two_box_example_keeps_both_ids_where_greedy_spawns_one():
    case = next(c for c in ac.cases() if c["name"] == "the-two-box-example")
    optimal, d = ac.run_definition(case)
    greedy, g = ac.run_definition(case, assign=None)
    assert optimal[1]["ids"][0, :2].tolist() == [1, 2] and d.events["spawned"] == 2 and int(d.next_id[0]) == 3
    assert greedy[1]["ids"][0, :2].tolist() == [2, 3] and g.events["spawned"] == 3 and int(g.next_id[0]) == 4
    (r,) = optimal[1]["rounds"]
    q = lambda v: ASSIGN_ONE + int(np.float32(v) * np.float32(ASSIGN_IOU_ONE))                  # noqa: E731
    assert r["w"].dtype == np.int32 and r["w"].shape == (2, 4) and not r["second"] and r["lane"] == 0
    assert r["w"].tolist() == [[q(np.float32(70) / np.float32(130)), q(np.float32(80) / np.float32(120)), 0, 0],
                               [0, q(np.float32(60) / np.float32(140)), 0, 0]]
    assert r["row_col"].tolist() == [0, 1] and r["greedy"].tolist() == [1, -1]


def test_the_tie_is_what_the_assignment_definition_gives():
    """Two identical rows over two identical tracks: w is constant over the 2 x 2 block, and the pairing the tracker uses
    is assign_max_weight_definition's on that w, the lowest column first."""
    case = next(c for c in ac.cases() if c["name"] == "a-tie-goes-to-the-lowest-column")
    steps, _ = ac.run_definition(case)
    (r,) = steps[1]["rounds"]
    assert len(set(r["w"][:, :2].reshape(-1).tolist())) == 1 and r["w"][0, 0] == ASSIGN_ONE + ASSIGN_IOU_ONE and not r["w"][:, 2:].any()
    assert r["row_col"].tolist() == assign_max_weight_definition(r["w"])[1].tolist() == [0, 1]


def _best_by_brute_force(w):
    """(most pairs, the largest sum of q among those) over every partial matching of the admissible pairs of w."""
    n, m = w.shape
    best = (0, 0)
    for cols in itertools.product(range(-1, m), repeat=n):
        used = [c for c in cols if c >= 0]
        if len(set(used)) != len(used) or any(c >= 0 and w[r, c] == 0 for r, c in enumerate(cols)):
            continue
        best = max(best, (len(used), sum(int(w[r, c]) - ASSIGN_ONE for r, c in enumerate(cols) if c >= 0)))
    return best


def test_a_round_has_the_most_pairs_and_among_those_the_largest_sum():
    """200 seeded single steps of at most 5 rows over at most 5 tracks, one label, overlapping boxes: the definition's round
    has the maximum number of pairs over every partial matching of the admissible pairs, and among those the maximum sum
    of q."""
    rng = np.random.Generator(np.random.PCG64(2))
    contested = 0
    for seed in range(200):
        n_tracks, n_rows = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        def boxes(n):
            at = rng.uniform(0, 14, (n, 2))
            return [(x, y, x + 10, y + 10, 0.9, 0) for x, y in at]
        d = TrackDefinition(1, dict(max_tracks=5), assign="optimal")
        d.step(ac._step([boxes(n_tracks)], ac.T, 5)["det"], [n_tracks], ac.T)
        assert int((d.id[0] != 0).sum()) == n_tracks
        s = ac._step([boxes(n_rows)], ac.T + 1000, 5)
        d.step(s["det"], s["n_keep"], s["t_ref"])
        (r,) = d.rounds
        w, row_col = r["w"], r["row_col"]
        assert w.shape == (n_rows, 5) and ((w == 0) | (w > ASSIGN_ONE)).all()
        pairs = [(i, c) for i, c in enumerate(row_col) if c >= 0]
        assert len({c for _, c in pairs}) == len(pairs) and all(w[i, c] > 0 for i, c in pairs), seed
        got = (len(pairs), sum(int(w[i, c]) - ASSIGN_ONE for i, c in pairs))
        assert got == _best_by_brute_force(w), (seed, got)
        contested += int(((w > 0).sum(0) > 1).any() or ((w > 0).sum(1) > 1).any())
    assert contested >= 100, contested


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
def test_where_nothing_is_contested_the_result_is_the_greedy_definitions(motion, rescue):
    """The well-separated scene: no round has a row or a track with two admissible partners (asserted), and ids, hits,
    untracked, rescued, the slots, with motion the boxes, velocities and coast lists are byte for byte the greedy
    TrackDefinition's after every step."""
    case = ac.separated(motion, rescue)
    optimal, d = ac.run_definition(case)
    greedy, g = ac.run_definition(case, assign=None)
    assert d.events["conflicts"] == 0 and d.events["reassigned"] == 0, d.events
    assert d.events["matched"] > 100 and d.events["retired"] > 0 and d.events["spawned"] > 12, d.events
    assert not rescue or d.events["rescued"] > 0, d.events
    for k, (a, b) in enumerate(zip(optimal, greedy)):
        a = {name: v for name, v in a.items() if name != "rounds"}
        assert rc.same_step(a, b) is None, (case["name"], k, rc.same_step(a, b))
    assert {k: v for k, v in d.events.items() if k not in ("conflicts", "reassigned")} == g.events


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
def test_the_crowded_scene_is_reassigned_and_never_matches_fewer(motion, rescue):
    """The first 40 steps of the crowded scene: some rounds pair otherwise than greedy does on the same state, and no round
    has fewer matches than greedy has on the same state."""
    steps, d = ac.run_definition(ac.crowd(motion, rescue))
    rounds = [r for o in steps for r in o["rounds"]]
    assert d.events["reassigned"] > 0 and d.events["conflicts"] >= d.events["reassigned"], d.events
    assert d.events["reassigned"] == sum(not np.array_equal(r["row_col"], r["greedy"]) for r in rounds)
    assert len(rounds) == 40 * 2 * (2 if rescue else 1)
    for r in rounds:
        assert int((r["row_col"] >= 0).sum()) >= int((r["greedy"] >= 0).sum()), (r["lane"], r["second"])
    if not motion:                                  # what the issue's prototype saw
        assert d.events["reassigned"] == (29 if rescue else 23), d.events


@pytest.mark.parametrize("max_tracks", [8, 64, 130])
def test_the_walks_exercise_the_rule(max_tracks):
    _, d = ac.run_definition(ac.walk(max_tracks, False, True))
    assert d.events["conflicts"] > 0 and d.events["rescued"] > 0 and d.events["retired"] > 0, d.events


def test_greedy_and_none_are_the_definition_as_it_was():
    case = ac.crowd(True, True, steps=10)
    runs = []
    for kw in (dict(), dict(assign=None), dict(assign="greedy")):
        d = TrackDefinition(case["B"], case["track"], motion=case["motion"], rescue=case["rescue"], **kw)
        assert d.assign is None and "conflicts" not in d.events
        runs.append([d.step(s["det"], s["n_keep"], s["t_ref"])[0].tobytes() for s in case["steps"]] + [d.box.tobytes()])
    assert runs[0] == runs[1] == runs[2]


def test_assign_is_refused_by_name():
    track = _track_options(True, "t")
    assert _assign_options(None, None, "t") is None and _assign_options(None, track, "t") is None
    assert _assign_options("greedy", track, "t") is None and _assign_options("optimal", track, "t") == "optimal"
    for bad in ("hungarian", True, 1, "Optimal", dict()):
        with pytest.raises(ValueError, match="assign = .* must be None or 'greedy'"):
            _assign_options(bad, track, "who")
    for given in ("optimal", "greedy"):
        with pytest.raises(ValueError, match="who: assign= needs track="):
            _assign_options(given, None, "who")
    with pytest.raises(ValueError, match="TrackDefinition: assign = 'best'"):
        TrackDefinition(1, True, assign="best")
