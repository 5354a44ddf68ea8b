"""Hand-written cases of the event stream's tracker (dagr_amd/streaming.py: TrackDefinition, dagr_stream_track), shared by
the CPU and the GPU tests.  Every box is a small integer, so every IoU is an exact ratio of small integers and the one
threshold that matters (0.5) is met exactly.  A case is

    name, B, A, track (the options), steps: [dict(det fp32 [B, A, 6], n_keep int32 [B], t_ref int64 [B])],
    expect: per step dict(ids, hits: per lane the rows below the clamped n_keep; untracked: per lane, cumulative).

Rows at and behind n_keep are filled with a box that would match everything, label 0 and score 1: nothing may read them."""
import numpy as np

NEVER = np.iinfo(np.int64).min
T = (1 << 33) + 5000          # absolute microseconds: int64 matters
PAD = (0.0, 0.0, 1000.0, 1000.0, 1.0, 0.0)


def _step(lanes, t_ref, A, n_keep=None):
    """lanes: per lane a list of rows (x1, y1, x2, y2, score, label)."""
    B = len(lanes)
    det = np.tile(np.asarray(PAD, np.float32), (B, A, 1))
    for b, rows in enumerate(lanes):
        for i, r in enumerate(rows):
            det[b, i] = r
    counts = [len(rows) for rows in lanes] if n_keep is None else n_keep
    t_ref = np.broadcast_to(np.asarray(t_ref, np.int64).reshape(-1), (B,)).copy()
    return dict(det=det, n_keep=np.asarray(counts, np.int32), t_ref=t_ref)


def _box(x, y, w=8, h=8, score=0.9, label=0):
    return (x, y, x + w, y + h, score, label)


def _case(name, track, steps, expect, A=4):
    B = len(steps[0][0])
    return dict(name=name, B=B, A=A, track=track, steps=[_step(lanes, t, A, n_keep=(s[2] if len(s) > 2 else None))
                                                         for s in steps for lanes, t in [s[:2]]],
                expect=[dict(ids=e[0], hits=e[1], untracked=e[2]) for e in expect])


def _many():
    """300 rows on a grid of disjoint boxes, every tenth below min_score: 270 eligible, the first 256 take part."""
    rows = [_box(20 * (i % 20), 20 * (i // 20), 10, 10, score=0.1 if i % 10 == 3 else 0.9, label=i % 3) for i in range(300)]
    eligible = [i for i in range(300) if i % 10 != 3]
    rank = {i: k for k, i in enumerate(eligible)}
    ids = [rank[i] + 1 if i in rank and rank[i] < 256 else 0 for i in range(300)]
    return dict(name="more-than-256-eligible-rows", B=1, A=300, track=dict(max_tracks=256, min_score=0.5),
                steps=[_step([rows], T, 300), _step([rows], T + 1000, 300)],
                expect=[dict(ids=[ids], hits=[[1 if v else 0 for v in ids]], untracked=[14]),
                        dict(ids=[ids], hits=[[2 if v else 0 for v in ids]], untracked=[28])])


def _two_register_slots():
    """max_tracks = 130: three register slots a thread, the last with a tail of two.  130 disjoint boxes fill every slot
    (ids 1 .. 130 in slots 0 .. 129) and a 131st row finds none.  The box of slot 0 then stays away and is retired, the box X
    of slot 64 (id 65) comes twice in one step, and its second row spawns id 131 into slot 0: slots 0 and 64, both in
    thread 0's registers, hold the same box, the LOWER id in the HIGHER slot.  A single X then has to go to id 65."""
    grid = [_box(20 * (i % 20), 20 * (i // 20), 10, 10, score=0.9 - 0.001 * i) for i in range(131)]
    first = [_box(900, 900, 10, 10)] + grid[1:131]                  # row 0 is far from the grid
    rest = grid[1:130]
    ids_rest = list(range(2, 131))
    return dict(name="equal-ious-in-one-threads-two-slots-at-130-tracks", B=1, A=140,
                track=dict(max_tracks=130, max_age_us=15),
                steps=[_step([first], T, 140), _step([rest], T + 10, 140), _step([rest + [grid[64]]], T + 20, 140),
                       _step([[grid[64]]], T + 25, 140)],
                expect=[dict(ids=[list(range(1, 131)) + [0]], hits=[[1] * 130 + [0]], untracked=[1]),
                        dict(ids=[ids_rest], hits=[[2] * 129], untracked=[1]),
                        dict(ids=[ids_rest + [131]], hits=[[3] * 129 + [1]], untracked=[1]),
                        dict(ids=[[65]], hits=[[4]], untracked=[1])])


def cases():
    just_above_half = float(np.nextafter(np.float32(0.5), np.float32(1)))
    out = [
        # (0,0,8,8) against (0,1,8,9): 56 / 72; the rows change places between the steps
        _case("spawn-then-match", dict(max_tracks=4),
              [([[_box(0, 0), _box(20, 20, score=0.8, label=1)]], T),
               ([[_box(21, 20, label=1), _box(0, 1, score=0.8)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0]), ([[2, 1]], [[2, 2]], [0])]),
        _case("label-mismatch-spawns", dict(max_tracks=4),
              [([[_box(0, 0, label=0)]], T), ([[_box(0, 0, label=1)]], T + 1), ([[_box(0, 0, label=1), _box(0, 0, label=0)]], T + 2)],
              [([[1]], [[1]], [0]), ([[2]], [[1]], [0]), ([[2, 1]], [[2, 2]], [0])]),
        # (0,0,4,4) against (0,0,4,2): inter 8, union (8 + 16) - 8 = 16: exactly 0.5
        _case("iou-exactly-at-the-threshold-matches", dict(iou=0.5, max_tracks=4),
              [([[_box(0, 0, 4, 4)]], T), ([[_box(0, 0, 4, 2)]], T + 1)],
              [([[1]], [[1]], [0]), ([[1]], [[2]], [0])]),
        _case("iou-one-ulp-below-the-threshold-spawns", dict(iou=just_above_half, max_tracks=4),
              [([[_box(0, 0, 4, 4)]], T), ([[_box(0, 0, 4, 2)]], T + 1)],
              [([[1]], [[1]], [0]), ([[2]], [[1]], [0])]),
        # slot 0 is retired and taken again by id 3, slot 1 holds id 2 with the same box: the lowest id wins, not the lowest
        # slot; the ids keep counting
        _case("identical-tracks-lowest-id-and-slot-reuse", dict(max_tracks=2, max_age_us=15),
              [([[_box(100, 100)]], T), ([[_box(0, 0)]], T + 10), ([[_box(0, 0), _box(0, 0, score=0.8)]], T + 20),
               ([[_box(0, 0)]], T + 25)],
              [([[1]], [[1]], [0]), ([[2]], [[1]], [0]), ([[2, 3]], [[2, 1]], [0]), ([[2]], [[3]], [0])]),
        # tracks (0,0,10,10) and (0,4,10,14).  Row (0,3,10,13): 70 / 130 with the first, 90 / 110 with the second -> the second
        _case("the-largest-iou-wins", dict(max_tracks=4),
              [([[_box(0, 0, 10, 10), _box(0, 4, 10, 10, score=0.8)]], T),
               ([[_box(0, 3, 10, 10), _box(0, 0, 10, 10, score=0.8)]], T + 1)],
              [([[1, 2]], [[1, 1]], [0]), ([[2, 1]], [[2, 2]], [0])]),
        # (0,2,10,12) scores higher than (0,0,10,10) and takes the contested track at 80 / 120, although the later row equals it
        _case("greedy-order-the-higher-score-takes-the-track", dict(max_tracks=4),
              [([[_box(0, 0, 10, 10)]], T), ([[_box(0, 2, 10, 10), _box(0, 0, 10, 10, score=0.8)]], T + 1)],
              [([[1]], [[1]], [0]), ([[1, 2]], [[2, 1]], [0])]),
        # an empty step ages only; age == max_age_us survives, one more retires
        _case("age-at-the-limit-survives-one-more-retires", dict(max_tracks=4, max_age_us=1000),
              [([[_box(0, 0)]], T), ([[]], T + 1000), ([[_box(0, 0)]], T + 1000), ([[_box(0, 0)]], T + 2001)],
              [([[1]], [[1]], [0]), ([[]], [[]], [0]), ([[1]], [[2]], [0]), ([[2]], [[1]], [0])]),
        _case("an-empty-lane-only-ages", dict(max_tracks=4, max_age_us=1000),
              [([[_box(0, 0), _box(20, 20)]], T), ([[]], T + 1001), ([[_box(20, 20)]], T + 1002)],
              [([[1, 2]], [[1, 1]], [0]), ([[]], [[]], [0]), ([[3]], [[1]], [0])]),
        _case("max-tracks-full-rows-go-untracked", dict(max_tracks=2),
              [([[_box(0, 0), _box(20, 0), _box(40, 0)]], T), ([[_box(0, 0), _box(20, 0), _box(40, 0)]], T + 1),
               ([[_box(40, 0), _box(20, 0)]], T + 2)],
              [([[1, 2, 0]], [[1, 1, 0]], [1]), ([[1, 2, 0]], [[2, 2, 0]], [2]), ([[0, 2]], [[0, 3]], [3])]),
        _many(),
        _two_register_slots(),
        _case("min-score-cut-and-a-nan-score", dict(max_tracks=4, min_score=0.5),
              [([[_box(0, 0), _box(20, 0, score=0.5), _box(40, 0, score=0.49), _box(60, 0, score=float("nan"))]], T),
               ([[_box(40, 0, score=0.6), _box(0, 0, score=0.2)]], T + 1)],
              [([[1, 2, 0, 0]], [[1, 1, 0, 0]], [0]), ([[3, 0]], [[1, 0]], [0])]),
        # 0 / 0: the box never matches its own track and spawns again
        _case("a-zero-area-box-spawns-every-time", dict(max_tracks=4),
              [([[_box(5, 5, 0, 0)]], T), ([[_box(5, 5, 0, 0)]], T + 1)],
              [([[1]], [[1]], [0]), ([[2]], [[1]], [0])]),
        _case("a-lane-without-a-reference-instant", dict(max_tracks=4),
              [([[_box(0, 0), _box(20, 0)]], NEVER), ([[_box(0, 0)]], T)],
              [([[0, 0]], [[0, 0]], [0]), ([[1]], [[1]], [0])]),
        # lane 0 spawns and matches, lane 1 has no instant until the last step, lane 2 fills up, ages and starts again
        _case("three-lanes-doing-different-things", dict(max_tracks=2, max_age_us=100),
              [([[_box(0, 0)], [_box(0, 0)], [_box(0, 0), _box(20, 0, label=1), _box(40, 0)]], [T, NEVER, T + 7]),
               ([[_box(1, 0), _box(30, 30)], [_box(0, 0)], []], [T + 50, NEVER, T + 107]),
               ([[_box(30, 30), _box(2, 0)], [_box(0, 0), _box(0, 0, label=1)], [_box(20, 0, label=1)]], [T + 60, T, T + 108])],
              [([[1], [0], [1, 2, 0]], [[1], [0], [1, 1, 0]], [0, 0, 1]),
               ([[1, 2], [0], []], [[2, 1], [0], []], [0, 0, 1]),
               ([[2, 1], [1, 2], [3]], [[2, 3], [1, 1], [1]], [0, 0, 1])]),
        _case("n-keep-beyond-A-is-clamped-and-negative-is-zero", dict(max_tracks=4),
              [([[_box(0, 0), _box(20, 0)], [_box(0, 0), _box(20, 0)]], T, [5, -3])],
              [([[1, 2], []], [[1, 1], []], [0, 0])], A=2),
    ]
    return out


def random_walk(max_tracks, seed=11, B=3, A=64, steps=40, objects=40):
    """A seeded walk as a case without written-out expectations: per lane ``objects`` boxes of two labels that drift by a
    fraction of a pixel to a few pixels a step, vanish for 1 to 9 steps (a step is 1000 us and max_age_us 3000: within
    and beyond the age) and come back where they are then; the visible ones are the step's rows, by descending score.
    Nothing is dyadic here: every IoU is a rounded fp32 quotient."""
    rng = np.random.Generator(np.random.PCG64(seed))
    centre = rng.uniform(20, 280, (B, objects, 2))
    size = rng.uniform(12, 40, (B, objects, 2))
    label = rng.integers(0, 2, (B, objects))
    hidden_until = np.zeros((B, objects), np.int64)
    out = []
    for k in range(steps):
        centre += rng.normal(0, 1.5, centre.shape)
        size *= rng.uniform(0.97, 1.03, size.shape)
        vanish = (rng.random((B, objects)) < 0.08) & (hidden_until <= k)
        hidden_until[vanish] = k + 1 + rng.integers(1, 10, int(vanish.sum()))
        lanes = []
        for b in range(B):
            seen = np.flatnonzero(hidden_until[b] <= k)
            score = rng.uniform(0.05, 1.0, len(seen)).astype(np.float32)
            order = np.argsort(-score, kind="stable")
            lanes.append([(centre[b, o, 0] - size[b, o, 0] / 2, centre[b, o, 1] - size[b, o, 1] / 2,
                           centre[b, o, 0] + size[b, o, 0] / 2, centre[b, o, 1] + size[b, o, 1] / 2, score[j], label[b, o])
                          for j, o in ((j, seen[j]) for j in order)])
        out.append(_step(lanes, T + 1000 * k, A))
    return dict(name=f"random-walk-{max_tracks}", B=B, A=A, steps=out, expect=None,
                track=dict(max_tracks=max_tracks, max_age_us=3000, iou=0.3, min_score=0.1))


def run_definition(case):
    """The definition's ``(ids, hits, untracked, tracks)`` after every step of a case; the definition itself last."""
    from dagr_amd.streaming import TrackDefinition
    d = TrackDefinition(case["B"], case["track"])
    out = []
    for s in case["steps"]:
        ids, hits = d.step(s["det"], s["n_keep"], s["t_ref"])
        out.append((ids, hits, d.untracked.copy(), (d.id.copy(), d.t_last.copy(), d.box.copy(), d.label.copy(), d.hits.copy(),
                                                    d.next_id.copy())))
    return out, d


def check_expectation(case, step, ids, hits, untracked):
    """The written-out expectation of one step against ``ids`` / ``hits`` [B, A] and ``untracked`` [B]."""
    e, s = case["expect"][step], case["steps"][step]
    where = (case["name"], step)
    for b in range(case["B"]):
        n = min(max(int(s["n_keep"][b]), 0), case["A"])
        assert len(e["ids"][b]) == n and len(e["hits"][b]) == n, where
        assert np.asarray(ids)[b, :n].tolist() == e["ids"][b], (where, b, "ids")
        assert np.asarray(hits)[b, :n].tolist() == e["hits"][b], (where, b, "hits")
    assert np.asarray(untracked).tolist() == e["untracked"], (where, "untracked")
