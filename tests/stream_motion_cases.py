"""Cases of the event stream's tracker with its motion model (dagr_amd/streaming.py: TrackDefinition(motion=),
dagr_stream_track_cv), shared by the CPU and the GPU tests.  The format is tests/stream_track_cases.py's with one more key:

    name, B, A, track, motion, steps: [dict(det fp32 [B, A, 6], n_keep int32 [B], t_ref int64 [B])],
    expect: None, or per step dict(ids, hits: per lane the rows below the clamped n_keep; untracked: per lane, cumulative).

The hand cases move 8x8 boxes by whole pixels in steps of 1000 us, so the predictions are whole pixels too wherever a case's
expectation depends on them; what each rule leaves in the state is asserted in tests/test_stream_motion_cpu.py, and the GPU
test holds the kernel to the definition bit for bit after every step of every case."""
import numpy as np

from tests import stream_track_cases as tc

NEVER, T = tc.NEVER, tc.T
_box, _step = tc._box, tc._step


def _case(name, track, motion, steps, expect=None, A=4):
    c = tc._case(name, track, steps, expect or [], A=A)
    c["motion"] = motion
    if expect is None:
        c["expect"] = None
    return c


def gap_steps():
    """The smallest case: one box that moves 2 px a step, is missed for four steps and comes back where it then is."""
    x = {0: 10, 1000: 12, 6000: 22, 7000: 24}
    return [([[_box(x[t], 50)] if t in x else []], T + t) for t in range(0, 8000, 1000)]


def _coast_list():
    """Stationary boxes A .. G at x = 0, 20, .. 120.  max_age_us 2500, six slots.
    t+0:    A B C D spawn (ids 1..4, slots 0..3)
    t+1000: B D E     -> B, D match, E spawns (id 5, slot 4); A (slot 0) and C (slot 2) coast
    t+3000: B         -> A, C retire (age 3000); D, E coast (age 2000)
    t+4000: B F G     -> D, E retire; F, G spawn into slots 0 and 2 (ids 6, 7); nothing coasts
    t+5000: (no rows) -> F, B, G coast: ids 6, 2, 7 in slot order, not in id order"""
    at = {n: _box(20 * k, 0) for k, n in enumerate("ABCDEFG")}
    rows = lambda names: [[at[n] for n in names]]                                     # noqa: E731
    return _case("coast-list-matched-spawned-retired-and-slot-order", dict(max_tracks=6, max_age_us=2500), True,
                 [(rows("ABCD"), T), (rows("BDE"), T + 1000), (rows("B"), T + 3000), (rows("BFG"), T + 4000),
                  (rows(""), T + 5000)],
                 [([[1, 2, 3, 4]], [[1, 1, 1, 1]], [0]), ([[2, 4, 5]], [[2, 2, 1]], [0]), ([[2]], [[3]], [0]),
                  ([[2, 6, 7]], [[4, 1, 1]], [0]), ([[]], [[]], [0])], A=4)


BACKWARDS = ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 5)          # a tie to the even below, a tie to the even above, no tie


def _backwards_clock():
    """Three lanes, each with one box that moves 2 px in the first 1000 us (vel 0.002) and a clock that then jumps BACK by
    more than 2**24 us: t_ref - t_last is negative (the track is not retired) and not representable in fp32, so the
    prediction shows how the difference was converted -- an ulp of the predicted x1 is 0.004 px, the velocity times 2 us.
    The step after the jump has no rows (the track coasts at the prediction), the one after it has the row there."""
    f = np.float32
    vel = f(2) / f(1000)
    steps = [([[_box(10, 50)]] * 3, T), ([[_box(12, 50)]] * 3, T + 1000)]
    back = [T + 1000 - d for d in BACKWARDS]
    dts = [np.int64(-d).astype(f) for d in BACKWARDS]
    there = [[(float(f(12 + f(vel * dt))), 50, float(f(20 + f(vel * dt))), 58, 0.9, 0)] for dt in dts]
    steps += [([[], [], []], back), (there, back)]
    return _case("a-backwards-clock-beyond-2**24", dict(max_tracks=4), True, steps,
                 [([[1]] * 3, [[1]] * 3, [0] * 3), ([[1]] * 3, [[2]] * 3, [0] * 3), ([[]] * 3, [[]] * 3, [0] * 3),
                  ([[1]] * 3, [[3]] * 3, [0] * 3)])


def _reused(case, name, motion=True):
    c = dict(case, name=name, motion=motion)
    return c


def cases():
    nan = float("nan")
    moving = [([[_box(10, 50)]], T), ([[_box(12, 50)]], T + 1000), ([[_box(16, 50)]], T + 2000), ([[_box(19, 50)]], T + 3000)]
    moving_ids = [([[1]], [[k]], [0]) for k in (1, 2, 3, 4)]
    odd = lambda dx: (10.1 + dx, 50.3 + dx, 18.7 + dx, 58.9 + dx, 0.9, 0)               # noqa: E731
    out = [
        _case("the-gap", True, True, gap_steps(),
              [([[1]], [[1]], [0]), ([[1]], [[2]], [0])] + [([[]], [[]], [0])] * 4 + [([[1]], [[3]], [0]), ([[1]], [[4]], [0])]),
        # 10, 12 (vel = q = 0.002), 16 (pred 14, r 2: vel += beta * 0.002), 19
        _case("first-continuation-sets-vel-later-ones-blend", dict(max_tracks=4), True, moving, moving_ids),
        _case("beta-zero-freezes-the-velocity", dict(max_tracks=4), dict(beta=0.0), moving, moving_ids),
        _case("alpha-one-stores-the-rows-box", dict(max_tracks=4), dict(alpha=1.0, beta=0.5),
              [([[odd(0)]], T), ([[odd(0.37)]], T + 700), ([[odd(1.01)]], T + 1900)], moving_ids[:3]),
        _case("alpha-half-stores-between-prediction-and-row", dict(max_tracks=4), dict(alpha=0.5, beta=0.5),
              [([[odd(0)]], T), ([[odd(0.37)]], T + 700), ([[odd(1.01)]], T + 1900), ([[odd(1.4)]], T + 2300)], moving_ids),
        # two steps at one instant: dt = 0 leaves vel and predicts box + vel * 0
        _case("two-steps-at-one-instant", dict(max_tracks=4), True,
              [([[_box(10, 50)]], T), ([[_box(12, 50)]], T + 1000), ([[_box(13, 50)]], T + 1000), ([[_box(15, 50)]], T + 2000)],
              moving_ids),
        _coast_list(),
        # min(a2, b2) - max(NaN, b1) is NaN: the box never matches, not even the track it spawned, which coasts as NaN
        _case("a-nan-box-never-matches-and-spawns", dict(max_tracks=4), True,
              [([[(nan, 0, 8, 8, 0.9, 0), _box(20, 0, score=0.8)]], T), ([[(nan, 0, 8, 8, 0.9, 0), _box(21, 0, score=0.8)]], T + 1000),
               ([[_box(22, 0, score=0.8)]], T + 2000)],
              [([[1, 2]], [[1, 1]], [0]), ([[3, 2]], [[1, 2]], [0]), ([[2]], [[3]], [0])]),
        # lane 0 loses its box for two steps and finds it again, lane 1 has no instant until the last step, lane 2 stands still
        _case("lanes-are-independent", dict(max_tracks=4, max_age_us=5000), True,
              [([[_box(10, 50)], [_box(10, 50)], [_box(100, 100)]], [T, NEVER, T + 7]),
               ([[_box(14, 50)], [_box(14, 50)], [_box(100, 100)]], [T + 1000, NEVER, T + 1007]),
               ([[], [_box(18, 50), _box(60, 60)], [_box(100, 100), _box(50, 50, label=1)]], [T + 2000, NEVER, T + 2007]),
               ([[], [], [_box(100, 100)]], [T + 3000, NEVER, T + 3007]),
               ([[_box(26, 50)], [_box(26, 50)], []], [T + 4000, T + 4000, T + 4007])],
              [([[1], [0], [1]], [[1], [0], [1]], [0, 0, 0]), ([[1], [0], [1]], [[2], [0], [2]], [0, 0, 0]),
               ([[], [0, 0], [1, 2]], [[], [0, 0], [3, 1]], [0, 0, 0]), ([[], [], [1]], [[], [], [4]], [0, 0, 0]),
               ([[1], [1], []], [[3], [1], []], [0, 0, 0])]),
        _backwards_clock(),
        _reused(tc._many(), "more-than-256-eligible-rows-with-motion"),
        _reused(tc._two_register_slots(), "three-register-slots-at-130-tracks-with-motion"),
    ]
    return out


def random_walk(max_tracks, seed=5, B=3, A=64, motion=True):
    """A seeded walk as a case without written-out expectations: per lane 36 boxes of two labels on constant-velocity paths
    (up to 5 px a step of 1000 us) with a jitter of a third of a pixel, which vanish for 2 to 9 steps (max_age_us is 6000:
    within and beyond the age) and come back where their path has taken them; the visible ones are the step's rows, by
    descending score, 40 steps.  Nothing is dyadic here.  With more than 64 slots the walk is crowded instead, so that
    the slots of a thread's second register fill: 100 boxes a lane of which a quarter vanishes every step -- about 40 rows
    a step and as many tracks again that coast --, 24 steps."""
    crowded = max_tracks > 64
    objects, steps, p_vanish = (100, 24, 0.25) if crowded else (36, 40, 0.08)
    rng = np.random.Generator(np.random.PCG64(seed))
    centre = rng.uniform(40, 280, (B, objects, 2))
    speed = rng.uniform(-5, 5, (B, objects, 2))
    size = rng.uniform(12, 40, (B, objects, 2))
    label = rng.integers(0, 2, (B, objects))
    hidden_until = np.zeros((B, objects), np.int64)
    out = []
    for k in range(steps):
        centre += speed
        seen_at = centre + rng.normal(0, 0.3, centre.shape)
        size *= rng.uniform(0.99, 1.01, size.shape)
        vanish = (rng.random((B, objects)) < p_vanish) & (hidden_until <= k)
        hidden_until[vanish] = k + rng.integers(2, 10, int(vanish.sum()))
        lanes = []
        for b in range(B):
            seen = np.flatnonzero(hidden_until[b] <= k)
            score = rng.uniform(0.05, 1.0, len(seen)).astype(np.float32)
            order = np.argsort(-score, kind="stable")[:A]
            lanes.append([(seen_at[b, o, 0] - size[b, o, 0] / 2, seen_at[b, o, 1] - size[b, o, 1] / 2,
                           seen_at[b, o, 0] + size[b, o, 0] / 2, seen_at[b, o, 1] + size[b, o, 1] / 2, score[j], label[b, o])
                          for j, o in ((j, seen[j]) for j in order)])
        out.append(_step(lanes, T + 1000 * k, A))
    return dict(name=f"motion-walk-{max_tracks}", B=B, A=A, steps=out, expect=None, motion=motion,
                track=dict(max_tracks=max_tracks, max_age_us=6000, iou=0.3, min_score=0.1))


def shared_instant(max_tracks=64):
    """The first 12 steps of the walk with every ``t_ref`` the same instant, ``alpha = 1``: ``dt`` is 0 throughout, every
    prediction is the box and no velocity ever changes, so the motion tracker has to give what the plain one gives."""
    case = random_walk(max_tracks, motion=dict(alpha=1.0, beta=0.25))
    steps = [dict(s, t_ref=np.full_like(s["t_ref"], T)) for s in case["steps"][:12]]
    return dict(case, name=f"shared-instant-{max_tracks}", steps=steps)


_RESULTS = {}


def run_definition(case):
    """After every step of a case the definition's ``dict(ids, hits, untracked, box, vel, n_coast, coast: (id, box, label,
    age_us), slots: (id, t_last, box, vel, label, hits, next_id))``, and the definition itself last.  Computed once per
    case name and shared: nobody changes what comes back."""
    if case["name"] in _RESULTS:
        return _RESULTS[case["name"]]
    from dagr_amd.streaming import TrackDefinition
    d = TrackDefinition(case["B"], case["track"], motion=case["motion"])
    out = []
    for s in case["steps"]:
        ids, hits = d.step(s["det"], s["n_keep"], s["t_ref"])
        out.append(dict(ids=ids, hits=hits, untracked=d.untracked.copy(), box=d.track_box.copy(), vel=d.track_vel.copy(),
                        n_coast=d.n_coast.copy(),
                        coast=(d.coast_id.copy(), d.coast_box.copy(), d.coast_label.copy(), d.coast_age_us.copy()),
                        slots=(d.id.copy(), d.t_last.copy(), d.box.copy(), d.vel.copy(), d.label.copy(), d.hits.copy(),
                               d.next_id.copy())))
    _RESULTS[case["name"]] = (out, d)
    return out, d


def run_plain(case):
    """The same steps through the plain definition: ``(ids, hits, untracked, slots)`` per step, and the definition."""
    return tc.run_definition(dict(case))


def bits(a):
    """Floats as their bits, so that NaNs compare and -0.0 differs from 0.0."""
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
