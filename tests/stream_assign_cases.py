"""Cases of the stream tracker's optimal assignment (dagr_amd/streaming.py: TrackDefinition(assign="optimal"),
dagr_stream_track_optimal), shared by the CPU and the GPU tests.  The format is tests/stream_rescue_cases.py's with one more
expectation:

    name, B, A, track, motion, rescue, steps: [dict(det fp32 [B, A, 6], n_keep int32 [B], t_ref int64 [B])],
    expect: None, or per step dict(ids, hits: per lane the rows below the clamped n_keep; untracked, rescued: per lane,
    cumulative), greedy: None, or the ids the GREEDY rule leaves per step where the case is about the difference.

The hand cases slide boxes of 10 x 10 along x: a shift of d pixels is an IoU of (10 - d) / (10 + d) -- 1: 0.82, 2: 0.67,
3: 0.54, 4: 0.43, 5: 0.33, 6: 0.25 -- against the tracker's threshold of 0.3.  Every case runs under all of its flag
combinations in the tests: its own motion / rescue, with assign="optimal"."""
import functools

import numpy as np

from dagr_amd.utils import synthetic as syn
from tests import stream_motion_cases as mc
from tests import stream_rescue_cases as rc
from tests import stream_track_cases as tc

NEVER, T = tc.NEVER, tc.T
_step = tc._step
LOW = 0.3
TRACK = dict(max_tracks=4, min_score=0.5)
CROWD_TRACK = dict(min_score=0.5, max_age_us=6000)


def _box(x, y=0, w=10, h=10, score=0.9, label=0):
    return tc._box(x, y, w, h, score, label)


def _case(name, track, motion, rescue, steps, expect, greedy=None, A=4):
    c = rc._case(name, track, rescue, steps, expect, A=A)
    c.update(motion=motion, greedy=greedy)
    return c


def _hand_cases(motion):
    m = "-with-motion" if motion else ""
    return [
        # tracks A (id 1) at 0 and B (id 2) at 5.  Box 1 at 3: 0.54 with A, 0.67 with B.  Box 2 at 9: 0.43 with B, 0.05 with A.
        # Greedy gives B to box 1 and box 2 spawns id 3; the assignment keeps both ids
        _case("the-two-box-example" + m, TRACK, motion, None,
              [([[_box(0), _box(5, score=0.8)]], T), ([[_box(3), _box(9, score=0.8)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0], None), ([[1, 2]], [[2, 2]], [0], None)], greedy=[[[1, 2]], [[2, 3]]]),
        # two identical rows over two identical tracks (slots 0 and 1): every pairing is optimal, the lowest column wins
        _case("a-tie-goes-to-the-lowest-column" + m, TRACK, motion, None,
              [([[_box(0), _box(0, score=0.8)]], T), ([[_box(0), _box(0, score=0.8)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0], None), ([[1, 2]], [[2, 2]], [0], None)]),
        # the track has label 0: the row of label 1 on top of it spawns, the row of label 0 one pixel off takes it
        _case("a-cross-label-pair-is-never-matched" + m, TRACK, motion, None,
              [([[_box(0)]], T), ([[_box(0, label=1), _box(1, score=0.8)]], T + 1000)],
              [([[1]], [[1]], [0], None), ([[2, 1]], [[1, 2]], [0], None)]),
        # 0 / 0: the zero-area box has a NaN IoU with its own track, and spawns again; the other row keeps its track
        _case("a-nan-iou-is-no-pair" + m, TRACK, motion, None,
              [([[_box(50, 50, 0, 0), _box(0, score=0.8)]], T), ([[_box(50, 50, 0, 0), _box(1, score=0.8)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0], None), ([[3, 2]], [[1, 2]], [0], None)]),
        # a shift of 6 is 0.25: under the threshold, the row spawns; the row shifted by 5 (0.33) of the other track matches
        _case("a-row-under-the-threshold-spawns" + m, TRACK, motion, None,
              [([[_box(0), _box(100, score=0.8)]], T), ([[_box(6), _box(105, score=0.8)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0], None), ([[3, 2]], [[1, 2]], [0], None)]),
        # round one pairs the high row (0.43) with the track; the low row (0.82) may not take what round one took
        _case("a-low-row-may-not-take-round-ones-slot" + m, TRACK, motion, True,
              [([[_box(0)]], T), ([[_box(4), _box(1, score=LOW)]], T + 1000)],
              [([[1]], [[1]], [0], [0]), ([[1, 0]], [[2, 0]], [0], [0])]),
        # round two is an assignment too: tracks at 0 and 5, no high row; low box 1 at 3 (0.54, 0.67), low box 2 at 9 (B only)
        _case("round-two-keeps-both-ids" + m, TRACK, motion, True,
              [([[_box(0), _box(5, score=0.8)]], T), ([[_box(3, score=LOW), _box(9, score=0.2)]], T + 1000)],
              [([[1, 2]], [[1, 1]], [0], [0]), ([[1, 2]], [[2, 2]], [0], [2])], greedy=[[[1, 2]], [[2, 0]]]),
        # lane 1 has no instant at first and then plays the two-box example; lane 0 stays alone
        _case("a-lane-without-an-instant" + m, TRACK, motion, None,
              [([[_box(0)], [_box(0), _box(5, score=0.8)]], [T, NEVER]),
               ([[_box(1)], [_box(0), _box(5, score=0.8)]], [T + 1000, T]),
               ([[_box(2)], [_box(3), _box(9, score=0.8)]], [T + 2000, T + 1000])],
              [([[1], [0, 0]], [[1], [0, 0]], [0, 0], None), ([[1], [1, 2]], [[2], [1, 1]], [0, 0], None),
               ([[1], [1, 2]], [[3], [2, 2]], [0, 0], None)]),
    ]


def _motion_only():
    """A box of 8 x 8 moves 4 px per 1000 us and is not seen for one step: at T + 3000 it stands at 12, where the track is
    predicted to be, and has no overlap with where the track was last seen (4).  Admissible only against pred."""
    return _case("a-pair-admissible-only-against-pred", TRACK, True, None,
                 [([[tc._box(0, 0)]], T), ([[tc._box(4, 0)]], T + 1000), ([[tc._box(12, 0)]], T + 3000)],
                 [([[1]], [[1]], [0], None), ([[1]], [[2]], [0], None), ([[1]], [[3]], [0], None)])


def _transposed():
    """max_tracks = 4 and 9 eligible rows on top of each other: more rows than slots, the transposed path; five rows find
    no slot, neither to match nor to spawn."""
    first = [_box(3 * i, score=0.9 - 0.01 * i) for i in range(4)]
    crowd = [_box(i, score=0.9 - 0.01 * i) for i in range(9)]
    return dict(name="more-rows-than-slots", B=1, A=12, track=dict(max_tracks=4), motion=None, rescue=None, expect=None,
                greedy=None, steps=[_step([first], T, 12), _step([crowd], T + 1000, 12), _step([crowd[::-1]], T + 2000, 12)])


def _cut():
    """300 rows against max_tracks = 256: 270 are eligible, 256 take part and fill every slot.  In the second step every box
    is 26 wide and reaches the next one of its grid row (0.2, above this case's threshold of 0.1; its own track: 0.38):
    a 256 x 256 round with conflicts along every grid row."""
    def rows(w):
        return [_box(20 * (i % 20), 20 * (i // 20), w, 10, score=0.1 if i % 10 == 3 else 0.9) for i in range(300)]
    return dict(name="the-256-row-cut", B=1, A=300, track=dict(max_tracks=256, min_score=0.5, iou=0.1), motion=None,
                rescue=None, expect=None, greedy=None, steps=[_step([rows(10)], T, 300), _step([rows(26)], T + 1000, 300)])


@functools.lru_cache(maxsize=None)
def cases():
    """The hand cases without and with the motion model, the motion-only pair, the transposed round and the cut (built
    once; nobody changes what comes back)."""
    return _hand_cases(None) + _hand_cases(True) + [_motion_only(), _transposed(), _cut()]


COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (motion, rescue): the four flag combinations


def _named(c, name, motion, rescue):
    return dict(c, name=f"{name}-{'motion' if motion else 'plain'}-{'rescue' if rescue else 'one-round'}", expect=None,
                greedy=None, motion=True if motion else None, rescue=dict(low_score=0.1) if rescue else None)


@functools.lru_cache(maxsize=None)
def walk(max_tracks, motion, rescue):
    """The committed seeded walk (tests/stream_motion_cases.py: random_walk: B = 3, A = 64, 40 steps) with min_score 0.5:
    40 boxes a lane in 260 x 260, so rounds with conflicts are common."""
    c = mc.random_walk(max_tracks, motion=True if motion else None)
    return dict(_named(c, f"assign-walk-{max_tracks}", motion, rescue), track=dict(c["track"], min_score=0.5))


@functools.lru_cache(maxsize=None)
def crowd(motion, rescue, steps=40):
    """The first ``steps`` steps of the crowded scene: 24 places in 160 x 120, one label, B = 2."""
    scene = syn.track_scene(seed=4, B=2, objects=24, steps=120, A=48, width=160, height=120, labels=1)[:steps]
    c = dict(B=2, A=48, track=CROWD_TRACK, steps=[dict(det=s["det"], n_keep=s["n_keep"], t_ref=s["t_ref"]) for s in scene])
    return _named(c, "crowd" if steps == 40 else f"crowd-{steps}-steps", motion, rescue)


@functools.lru_cache(maxsize=None)
def separated(motion, rescue, seed=3, B=2, steps=30):
    """A well-separated scene: 12 cells of 80 x 80, one box of 20 x 20 in each, which drifts by a pixel a step and jitters by
    at most 1.5 -- every IoU with its own live track stays above 0.4, every other IoU is 0 --, is absent now and then for
    up to eight steps (max_age_us is 3000: some tracks retire) and has a score between 0.2 and 1.  No row and no track ever
    has two admissible partners."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cells, A = 12, 16
    origin = np.array([[80 * (c % 4) + 20, 80 * (c // 4) + 30] for c in range(cells)], np.float64)
    hidden_until = np.zeros((B, cells), np.int64)
    out = []
    for k in range(steps):
        vanish = (rng.random((B, cells)) < 0.1) & (hidden_until <= k)
        hidden_until[vanish] = k + 1 + rng.integers(1, 9, int(vanish.sum()))
        lanes = []
        for b in range(B):
            seen = np.flatnonzero(hidden_until[b] <= k)
            score = rng.uniform(0.2, 1.0, len(seen)).astype(np.float32)
            at = origin[seen] + [k, 0] + np.clip(rng.normal(0, 0.7, (len(seen), 2)), -1.5, 1.5)
            order = np.argsort(-score, kind="stable")
            lanes.append([(at[j, 0], at[j, 1], at[j, 0] + 20, at[j, 1] + 20, score[j], seen[j] % 2) for j in order])
        out.append(_step(lanes, T + 1000 * k, A))
    c = dict(B=B, A=A, track=dict(max_tracks=16, max_age_us=3000, iou=0.3, min_score=0.5), steps=out)
    return _named(c, "separated", motion, rescue)


_RESULTS = {}


def run_definition(case, assign="optimal"):
    """``tests/stream_rescue_cases.py: run_definition`` with ``assign``: after every step what the definition leaves, and
    the definition itself last; with ``assign`` every step also has ``rounds``.  Computed once per case name and shared."""
    key = (case["name"], assign)
    if key in _RESULTS:
        return _RESULTS[key]
    from dagr_amd.streaming import TrackDefinition
    d = TrackDefinition(case["B"], case["track"], motion=case["motion"], rescue=case["rescue"], assign=assign)
    out = []
    for s in case["steps"]:
        ids, hits = d.step(s["det"], s["n_keep"], s["t_ref"])
        vel = (d.vel.copy(),) if d.motion is not None else ()
        o = dict(ids=ids, hits=hits, untracked=d.untracked.copy(),
                 slots=(d.id.copy(), d.t_last.copy(), d.box.copy(), *vel, d.label.copy(), d.hits.copy(), d.next_id.copy()))
        if d.rescue is not None:
            o["rescued"] = d.rescued.copy()
        if d.motion is not None:
            o.update(box=d.track_box.copy(), vel=d.track_vel.copy(), n_coast=d.n_coast.copy(),
                     coast=(d.coast_id.copy(), d.coast_box.copy(), d.coast_label.copy(), d.coast_age_us.copy()))
        if d.assign is not None:
            o["rounds"] = d.rounds
        out.append(o)
    _RESULTS[key] = (out, d)
    return out, d


def check_expectation(case, step, ids, hits, untracked, rescued=None):
    tc.check_expectation(case, step, ids, hits, untracked)
    if case["rescue"] is not None:
        assert np.asarray(rescued).tolist() == case["expect"][step]["rescued"], (case["name"], step, "rescued")
