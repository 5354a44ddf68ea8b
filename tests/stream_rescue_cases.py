"""Cases of the stream tracker's second association round (dagr_amd/streaming.py: TrackDefinition(rescue=),
dagr_stream_track_rescue, dagr_stream_track_cv_rescue), shared by the CPU and the GPU tests.  The format is
tests/stream_motion_cases.py's with one more option and one more expectation:

    name, B, A, track, motion, rescue, steps: [dict(det fp32 [B, A, 6], n_keep int32 [B], t_ref int64 [B])],
    expect: None, or per step dict(ids, hits: per lane the rows below the clamped n_keep; untracked, rescued: per lane,
    cumulative).

Every hand case exists twice, without and with ``motion=True``, under one expectation: its boxes stand still or move by whole
pixels per 1000 us, and wherever an expectation hangs on an IoU the track is at rest, so the prediction is the box.
``min_score`` is 0.5 and ``low_score`` 0.1 unless a case says otherwise: a score of 0.9 is high, one of 0.3 is low."""
import functools

import numpy as np

from tests import stream_motion_cases as mc
from tests import stream_track_cases as tc

NEVER, T = tc.NEVER, tc.T
_box, _step = tc._box, tc._step
LOW = 0.3
TRACK = dict(max_tracks=4, min_score=0.5)
FLICKER_SCORES = (0.9, 0.9, 0.3, 0.2, 0.3, 0.9, 0.9)


def _case(name, track, rescue, steps, expect, A=4):
    c = mc._case(name, track, None, steps, [e[:3] for e in expect], A=A)
    c["rescue"] = rescue
    for e, full in zip(c["expect"], expect):
        e["rescued"] = full[3]
    return c


def flicker_steps():
    """One box that moves 2 px per 1000 us and whose score dips under min_score for three steps."""
    return [([[_box(10 + 2 * k, 50, score=s)]], T + 1000 * k) for k, s in enumerate(FLICKER_SCORES)]


def _cap():
    """Tracks 1 at (900, 900) and 2 at (940, 900).  Then 560 low rows: the 256th of the band lies on track 2 and is the last
    to take part; the 257th lies on track 1, which no row has taken, and must not get it.  The rest are far from both."""
    grid = [_box(20 * (i % 20), 20 * (i // 20), 10, 10, score=LOW) for i in range(558)]
    rows = grid[:255] + [_box(940, 900, score=LOW), _box(900, 900, score=LOW)] + grid[255:]
    ids = [0] * 560
    ids[255] = 2
    return dict(name="more-than-256-low-rows", B=1, A=600, track=TRACK, rescue=True, motion=None,
                steps=[_step([[_box(900, 900), _box(940, 900, score=0.8)]], T, 600), _step([rows], T + 1000, 600)],
                expect=[dict(ids=[[1, 2]], hits=[[1, 1]], untracked=[0], rescued=[0]),
                        dict(ids=[ids], hits=[[2 * int(v > 0) for v in ids]], untracked=[0], rescued=[1])])


def _hand_cases():
    nan = float("nan")
    below_quarter = float(np.nextafter(np.float32(0.25), np.float32(0)))
    four = [_box(0, 0), _box(20, 0, score=0.8), _box(40, 0, score=0.7), _box(60, 0, score=0.6)]
    return [
        _case("the-flicker", dict(min_score=0.5, max_age_us=1500), True, flicker_steps(),
              [([[1]], [[k + 1]], [0], [r]) for k, r in enumerate((0, 0, 1, 2, 3, 3, 3))]),
        # three free slots, and the low row still gets none -- twice; the high row next to it spawns and continues
        _case("a-low-row-never-spawns-and-is-not-untracked", TRACK, True,
              [([[_box(0, 0, score=LOW), _box(20, 0)]], T), ([[_box(20, 0), _box(0, 0, score=LOW)]], T + 1000)],
              [([[0, 1]], [[0, 1]], [0], [0]), ([[1, 0]], [[2, 0]], [0], [0])]),
        # track (0,0,10,10).  The high row (0,4,10,14) has 60 / 140 with it, the low row (0,1,10,11) has 90 / 110
        _case("high-rows-pick-first", TRACK, True,
              [([[_box(0, 0, 10, 10)]], T), ([[_box(0, 4, 10, 10), _box(0, 1, 10, 10, score=LOW)]], T + 1000)],
              [([[1]], [[1]], [0], [0]), ([[1, 0]], [[2, 0]], [0], [0])]),
        # the same with the low row in FRONT of the high row: where a row stands in det does not decide its round
        _case("a-low-row-in-front-of-a-high-row-waits", TRACK, True,
              [([[_box(0, 0, 10, 10)]], T), ([[_box(0, 1, 10, 10, score=LOW), _box(0, 4, 10, 10)]], T + 1000)],
              [([[1]], [[1]], [0], [0]), ([[0, 1]], [[0, 2]], [0], [0])]),
        # as tests/stream_track_cases.py builds it: slot 0 holds id 3, slot 1 id 2, both the box (0,0,8,8).  Then three low
        # rows there: label 1 finds no track of its label; the first of label 0 takes the LOWEST id, the second what is left
        _case("round-two-keeps-the-label-rule-and-the-lowest-id", dict(max_tracks=2, max_age_us=15, min_score=0.5), True,
              [([[_box(100, 100)]], T), ([[_box(0, 0)]], T + 10), ([[_box(0, 0), _box(0, 0, score=0.8)]], T + 20),
               ([[_box(0, 0, score=LOW, label=1), _box(0, 0, score=LOW), _box(0, 0, score=0.2)]], T + 25)],
              [([[1]], [[1]], [0], [0]), ([[2]], [[1]], [0], [0]), ([[2, 3]], [[2, 1]], [0], [0]),
               ([[0, 2, 3]], [[0, 3, 2]], [0], [2])]),
        # (0,0,10,10) against (0,4,10,14): 60 / 140 = 0.43, between the tracker's 0.3 and the round's own 0.5
        _case("the-rounds-own-threshold-refuses", dict(max_tracks=4, min_score=0.5, iou=0.3), dict(iou=0.5),
              [([[_box(0, 0, 10, 10)]], T), ([[_box(0, 4, 10, 10, score=LOW)]], T + 1000)],
              [([[1]], [[1]], [0], [0]), ([[0]], [[0]], [0], [0])]),
        _case("without-a-threshold-of-its-own-the-trackers-holds", dict(max_tracks=4, min_score=0.5, iou=0.3), dict(iou=None),
              [([[_box(0, 0, 10, 10)]], T), ([[_box(0, 4, 10, 10, score=LOW)]], T + 1000)],
              [([[1]], [[1]], [0], [0]), ([[1]], [[2]], [0], [1])]),
        # exactly min_score is high, exactly low_score is low, one ulp under low_score and NaN are in neither band
        _case("the-band-edges", dict(max_tracks=4, min_score=0.5), dict(low_score=0.25),
              [([four], T), ([[_box(20, 0, score=0.5), _box(0, 0, score=0.25), _box(40, 0, score=below_quarter),
                               _box(60, 0, score=nan)]], T + 1000)],
              [([[1, 2, 3, 4]], [[1, 1, 1, 1]], [0], [0]), ([[2, 1, 0, 0]], [[2, 2, 0, 0]], [0], [1])]),
        _case("a-low-row-cannot-match-a-track-spawned-in-its-step", TRACK, True,
              [([[_box(0, 0), _box(0, 0, score=LOW)]], T), ([[_box(0, 0, score=LOW)]], T + 1000)],
              [([[1, 0]], [[1, 0]], [0], [0]), ([[1]], [[2]], [0], [1])]),
        _case("a-track-retired-in-this-step-is-not-rescued", dict(max_tracks=4, min_score=0.5, max_age_us=1000), True,
              [([[_box(0, 0)]], T), ([[_box(0, 0, score=LOW)]], T + 1001), ([[_box(0, 0)]], T + 1002)],
              [([[1]], [[1]], [0], [0]), ([[0]], [[0]], [0], [0]), ([[2]], [[1]], [0], [0])]),
        _cap(),
        # lane 0 has no instant for two steps, lane 1 never sees a low row, lane 2 is rescued three times
        _case("three-lanes-count-on-their-own", TRACK, True,
              [([[_box(0, 0)], [_box(0, 0)], [_box(0, 0), _box(20, 0, score=0.8)]], [NEVER, T, T]),
               ([[_box(0, 0, score=LOW)], [_box(0, 0)], [_box(0, 0, score=LOW), _box(20, 0, score=0.2)]],
                [NEVER, T + 1000, T + 1000]),
               ([[_box(0, 0)], [_box(0, 0)], [_box(0, 0), _box(20, 0, score=LOW)]], T + 2000),
               ([[_box(0, 0, score=LOW)], [], []], T + 3000)],
              [([[0], [1], [1, 2]], [[0], [1], [1, 1]], [0, 0, 0], [0, 0, 0]),
               ([[0], [1], [1, 2]], [[0], [2], [2, 2]], [0, 0, 0], [0, 0, 2]),
               ([[1], [1], [1, 2]], [[1], [3], [3, 3]], [0, 0, 0], [0, 0, 3]),
               ([[1], [], []], [[2], [], []], [0, 0, 0], [1, 0, 3])]),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    """Every hand case without and with the motion model (built once; nobody changes what comes back)."""
    out = []
    for c in _hand_cases():
        out.append(c)
        out.append(dict(c, name=c["name"] + "-with-motion", motion=True))
    return out


@functools.lru_cache(maxsize=None)
def walk(max_tracks, motion, iou=None):
    """The committed seeded walk (tests/stream_motion_cases.py: random_walk; scores uniform in 0.05 .. 1.0) with min_score
    raised to 0.5, so that half of its rows fall under the cut, and low_score 0.1."""
    c = mc.random_walk(max_tracks, motion=True if motion else None)
    rescue = dict(low_score=0.1) if iou is None else dict(low_score=0.1, iou=iou)
    return dict(c, name=f"rescue-walk-{max_tracks}-{'motion' if motion else 'plain'}-{iou}", rescue=rescue,
                track=dict(c["track"], min_score=0.5))


WALKS = [(m, motion, iou) for m in (8, 64, 130) for motion in (False, True) for iou in (None, 0.5)]


def scores_in_band(case, low_score):
    """How many rows of a case have a score in [low_score, the case's min_score), as fp32."""
    from dagr_amd.streaming import _track_options
    cut = np.float32(_track_options(case["track"], "t")["min_score"])
    scores = np.concatenate([s["det"][b, :min(max(int(s["n_keep"][b]), 0), case["A"]), 4]
                             for s in case["steps"] for b in range(case["B"])])
    return int(np.sum((scores >= np.float32(low_score)) & ~(scores >= cut)))


@functools.lru_cache(maxsize=None)
def neutral_cases():
    """Every existing case of the tracker and of its motion model, and the walks, with the case's own min_score and a rescue
    band that no score of the case falls in: [-1, min_score) wherever that band is empty.  It is not in the walks (min_score
    0.1, scores from 0.05) nor in the two hand cases that have rows under their min_score of 0.5; those run with the band
    of one fp32 value under min_score, which no row has.  The tests assert the band empty before they rely on it."""
    from dagr_amd.streaming import _track_options
    out = [dict(c, motion=None) for c in tc.cases()] + list(mc.cases())
    out += [dict(tc.random_walk(m), motion=None) for m in (8, 64)]
    out += [mc.random_walk(m, motion=True if motion else None) for m in (8, 64, 130) for motion in (False, True)]
    done = []
    for c in out:
        low = -1.0
        if scores_in_band(c, low):
            cut = np.float32(_track_options(c["track"], "t")["min_score"])
            low = float(np.nextafter(cut, np.float32(-np.inf)))
        done.append(dict(c, name=f"neutral-{c['name']}-{'motion' if c['motion'] else 'plain'}", rescue=dict(low_score=low),
                         expect=None))
    return done


_RESULTS = {}


def run_definition(case, rescue="the case's"):
    """After every step of a case what the definition leaves: ``dict(ids, hits, untracked, slots: (id, t_last, box, [vel,]
    label, hits, next_id))``, with ``rescue`` also ``rescued``, with ``motion`` also ``box, vel, n_coast, coast: (id, box,
    label, age_us)``; and the definition itself last.  ``rescue=None`` runs the same steps without the second round.
    Computed once per case name and shared: nobody changes what comes back."""
    key = (case["name"], rescue is None)
    if key in _RESULTS:
        return _RESULTS[key]
    from dagr_amd.streaming import TrackDefinition
    d = TrackDefinition(case["B"], case["track"], motion=case["motion"], rescue=case["rescue"] if rescue is not None else None)
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
        out.append(o)
    _RESULTS[key] = (out, d)
    return out, d


def same(a, b):
    """Equal arrays; floats as bits (tests/stream_motion_cases.py: bits), so a NaN equals itself and -0.0 is not 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = mc.bits(a), mc.bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def same_step(got, want):
    """Everything a step leaves, by name (what ``run_definition`` returns per step), bit for bit; the coast entries up to
    ``n_coast``.  The name of the first difference, or None."""
    for name in sorted(set(got) | set(want)):
        if name not in got or name not in want:
            return name
        if name == "slots":
            if len(got[name]) != len(want[name]) or not all(same(a, b) for a, b in zip(got[name], want[name])):
                return name
        elif name == "coast":
            for b, n in enumerate(want["n_coast"]):
                if not all(same(x[b, :n], y[b, :n]) for x, y in zip(got[name], want[name])):
                    return name
        elif not same(got[name], want[name]):
            return name
    return None


def check_expectation(case, step, ids, hits, untracked, rescued):
    tc.check_expectation(case, step, ids, hits, untracked)
    assert np.asarray(rescued).tolist() == case["expect"][step]["rescued"], (case["name"], step, "rescued")
