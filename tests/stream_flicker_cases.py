"""Pushes for the event stream's anti-flicker and trail filters (tests/test_stream_flicker_cpu.py and _gpu.py).

A case is ``dict(name, B, W, H, flicker, trail_us, pushes, expect)``: a ``W x H`` sensor, ``B`` lanes, the options as
``EventStream`` takes them (``flicker``: None, True or a dict; ``trail_us``: None or an int), a list of pushes
``dict(x, y, t, p, batch)`` in lane order with absolute int64 timestamps from ``T0 = 2^33 + 777`` on, and -- for the
hand-computed cases -- the expected outcome (0 kept, 1 flicker, 2 trail, -1 not of this sensor) of every event of every
push.  With the defaults ``min_period = 2000`` and ``max_period = 20000`` microseconds, ``start = 4``, ``stop = 1``,
``max_count = 7``.

The random cases come from ``dagr_amd.utils.synthetic.flicker_events`` plus same-polarity bursts and uniform noise, at
seeds 0 to 3, each once as ONE push and once cut into 1 ms pushes; ``outcome_shares`` is what the CPU test holds against
the 10 % floor, so that no case degenerates into all-kept."""
import numpy as np

from dagr_amd.utils import synthetic as syn
from tests.stream_denoise_cases import T0, push

ON, OFF = 1, -1
LONG_RUNS = (15, 16, 17, 63, 64, 65, 128, 129)      # around the walk's per-thread / per-wave threshold and its 64-event rounds


def _one_pixel(x, y, rows):
    """rows: [(t, p)] on one pixel -> (x, y, t, p)."""
    a = np.asarray(rows, np.int64).reshape(-1, 2)
    return np.full(len(a), x), np.full(len(a), y), a[:, 0], a[:, 1]


def _merge(*parts):
    """Events of several sources in one lane, stably by time."""
    x, y, t, p = (np.concatenate([np.asarray(q[k], np.int64) for q in parts]) for k in range(4))
    o = np.argsort(t, kind="stable")
    return x[o], y[o], t[o], p[o]


def _square(period, t_end, t0=0):
    """ON at t0, OFF half a period later, ... : [(t, p)] below t_end."""
    return [(t, ON if k % 2 == 0 else OFF) for k, t in enumerate(range(t0, t_end, period // 2))]


def _case(name, B, W, H, flicker, trail_us, pushes, expect=None):
    return dict(name=name, B=B, W=W, H=H, flicker=flicker, trail_us=trail_us, pushes=pushes,
                expect=None if expect is None else [np.asarray(e, np.int8) for e in expect])


# ------------------------------------------------------------------------------------------------ hand-computed
def hand_100hz():
    """100 Hz on one pixel.  ON@0 has no predecessor: not an edge.  ON@10000 is the first edge: it sets t_edge and counts
    nothing.  ON@20000, 30000, 40000, 50000 count 1, 2, 3, 4 = start: blocked from ON@50000 on."""
    rows = _square(10000, 100000)
    return _case("hand-100hz", 1, 8, 6, True, None, [push({0: _one_pixel(3, 2, rows)})],
                 [[0 if t < 50000 else 1 for t, _ in rows]])


def hand_out_of_band():
    """10 Hz (period 100000 > max_period: every edge is stale) and 5 kHz (period 200 < min_period: every edge counts
    down from 0) are never blocked."""
    slow, fast = _square(100000, 1000000), _square(200, 8000)
    ev = _merge(_one_pixel(1, 1, slow), _one_pixel(6, 4, fast))
    return _case("hand-out-of-band", 1, 8, 6, True, None, [push({0: ev})], [[0] * (len(slow) + len(fast))])


def hand_stops():
    """A flicker that stops: the last edge is ON@80000 (count 7).  OFF@100000 is exactly max_period after it: not stale,
    still blocked.  OFF@100001 is stale: count 0, released.  ON@100002 is an edge 20002 after the last: counts nothing."""
    rows = _square(10000, 90000) + [(100000, OFF), (100001, OFF), (100002, ON)]
    expect = [0 if t < 50000 else 1 for t, _ in rows[:-2]] + [0, 0]
    return _case("hand-stops", 1, 8, 6, True, None, [push({0: _one_pixel(0, 0, rows)})], [expect])


def hand_hysteresis():
    """count reaches 4 at ON@50000 (blocked).  Edges 200 us apart count down: 3 at ON@50200 and 2 at ON@50400 stay
    blocked (between stop and start), 1 at ON@50600 releases.  Counting up again, 2 at ON@60600 and 3 at ON@70600 stay
    released, 4 at ON@80600 blocks."""
    rows = _square(10000, 50001)                                        # ..., OFF@45000, ON@50000
    expect = [0] * (len(rows) - 1) + [1]
    tail = [(50100, OFF, 1), (50200, ON, 1), (50300, OFF, 1), (50400, ON, 1), (50500, OFF, 1), (50600, ON, 0), (50700, OFF, 0),
            (60600, ON, 0), (65600, OFF, 0), (70600, ON, 0), (75600, OFF, 0), (80600, ON, 1), (85600, OFF, 1)]
    rows += [(t, p) for t, p, _ in tail]
    expect += [o for _, _, o in tail]
    return _case("hand-hysteresis", 1, 8, 6, True, None, [push({0: _one_pixel(7, 5, rows)})], [expect])


def hand_no_predecessor():
    """ON events only: never an edge, t_edge stays never, nothing is blocked, at a 100 Hz rate."""
    rows = [(t, ON) for t in range(0, 100000, 10000)]
    return _case("hand-no-predecessor", 1, 8, 6, True, None, [push({0: _one_pixel(2, 3, rows)})], [[0] * len(rows)])


def hand_trail_gaps():
    """trail_us = 1000: gaps of 999 trail, also behind an event that trailed itself; a gap of exactly 1000 does not; a
    change of polarity does not."""
    rows = [(0, ON, 0), (999, ON, 2), (1998, ON, 2), (2998, ON, 0), (3000, ON, 2), (3001, OFF, 0), (4000, OFF, 2), (5000, OFF, 0)]
    return _case("hand-trail-gaps", 1, 8, 6, None, 1000, [push({0: _one_pixel(4, 1, [r[:2] for r in rows])})],
                 [[r[2] for r in rows]])


def hand_alternating():
    """Alternating polarity 10 us apart never trails."""
    rows = [(10 * k, ON if k % 2 == 0 else OFF) for k in range(40)]
    return _case("hand-alternating", 1, 8, 6, None, 1000, [push({0: _one_pixel(5, 5, rows)})], [[0] * len(rows)])


def hand_chained():
    """Both stages, trail_us = 40000.  The last event through the flicker stage before it blocks is OFF@45000.  ON@50000,
    OFF@55000 and ON@60000 are blocked and update neither t_pass nor p_pass: OFF@80001 -- stale, released -- meets
    p_pass = -1 and t_pass = 45000, 35001 us old, and trails.  Had ON@60000 reached the trail stage it would have been
    kept.  ON@80002 changes polarity: kept."""
    rows = _square(10000, 60001) + [(80001, OFF), (80002, ON)]
    expect = [0 if t < 50000 else 1 for t, _ in rows[:-2]] + [2, 0]
    return _case("hand-chained", 1, 8, 6, True, 40000, [push({0: _one_pixel(3, 3, rows)})], [expect])


def hand_equal_timestamps():
    """Six events with one timestamp on one pixel, both stages, trail_us = 1: the second ON sees the first (0 us old:
    trails); the later ONs are edges 0 us apart, which count down from 0."""
    rows = [(100, ON, 0), (100, ON, 2), (100, OFF, 0), (100, ON, 0), (100, OFF, 0), (100, ON, 0)]
    return _case("hand-equal-timestamps", 1, 8, 6, True, 1, [push({0: _one_pixel(0, 5, [r[:2] for r in rows])})],
                 [[r[2] for r in rows]])


# ------------------------------------------------------------------------------------------------ structural
def three_lanes():
    """The same pixel in three lanes: 100 Hz in lane 0, a trail burst in lane 1, single events far apart in lane 2; a second
    push continues all three."""
    sq = _square(10000, 120000)
    burst = [(1000 + 300 * k, ON) for k in range(8)]
    first = {0: _one_pixel(3, 2, sq[:14]), 1: _one_pixel(3, 2, burst[:5]), 2: _one_pixel(3, 2, [(5, OFF), (90000, OFF)])}
    second = {0: _one_pixel(3, 2, sq[14:]), 1: _one_pixel(3, 2, burst[5:]), 2: _one_pixel(3, 2, [(95000, OFF)])}
    return _case("three-lanes", 3, 8, 6, True, 1000, [push(first), push(second)])


def not_of_this_sensor(batch_tail):
    """Events outside the sensor on every side (status value 16, no state, not counted), a lane >= B and lane -1 rows
    behind a count (no status from the filter); then an empty push and a push of one event."""
    rng = np.random.Generator(np.random.PCG64(31))
    n = 90
    x, y = rng.integers(0, 8, n), rng.integers(0, 6, n)
    t, p = np.cumsum(rng.integers(0, 400, n)), rng.choice(np.array([-1, 1]), n)
    bad = np.array([3, 20, 41, 77])
    x[bad], y[bad] = [-1, 8, x[41], x[77]], [y[3], y[20], -1, 6]
    first = push({0: (x[:50], y[:50], t[:50], p[:50]), 1: (x[50:], y[50:], t[50:], p[50:])})
    k = len(batch_tail)
    tail = dict(x=np.zeros(k, np.int16), y=np.zeros(k, np.int16), t=np.full(k, T0 + 5, np.int64), p=np.ones(k, np.int8),
                batch=np.asarray(batch_tail, np.int64))
    first = {key: np.concatenate([first[key], tail[key]]) for key in first}
    clean = push({1: ([2, 2], [2, 2], [int(t[-1]) + 10, int(t[-1]) + 20], [1, 1])})        # no event outside: status 0
    one = push({0: ([7], [5], [int(t[-1]) + 30], [-1])})
    return _case("not-of-this-sensor", 2, 8, 6, True, 500, [first, push({}), clean, push({}), one])


def long_runs(flicker, trail_us, tag):
    """One push: runs of 15 .. 129 events on pixels of their own (the walk's threshold between one thread and one wave, and
    its rounds of 64), a run of 300 events on one pixel -- a mix of 100 Hz flicker and bursts, so that every outcome occurs
    inside it --, and a row of neighbouring pixels with single events.  A second push meets the carried state."""
    rng = np.random.Generator(np.random.PCG64(57))
    parts = []
    for k, n in enumerate(LONG_RUNS):
        t = np.cumsum(rng.integers(100, 900, n))
        parts.append((np.full(n, 2 * k), np.full(n, 3), t, rng.choice(np.array([-1, 1]), n)))
    sq = _square(10000, 400000, t0=200000)                              # 40 events of a light switched on at 200 ms
    burst_t = (rng.integers(0, 399000, 65)[:, None] + 100 * np.arange(4)).reshape(-1)       # 65 bursts of 4, 100 us apart
    burst_p = np.repeat(rng.choice(np.array([-1, 1]), 65), 4)
    parts.append(_merge(_one_pixel(9, 7, sq), (np.full(260, 9), np.full(260, 7), burst_t, burst_p)))
    parts.append((np.arange(16), np.full(16, 8), rng.integers(0, 400000, 16), np.ones(16, np.int64)))
    ev = _merge(*parts)
    assert int(((ev[0] == 9) & (ev[1] == 7)).sum()) == 300 and len(ev[2]) % 64 != 0
    later = (ev[0][::3], ev[1][::3], ev[2][::3] + 400000, ev[3][::3])
    return _case("long-runs-" + tag, 1, 16, 12, flicker, trail_us, [push({0: ev}), push({0: later})])


# ------------------------------------------------------------------------------------------------ random
RANDOM_SHAPES = ((8, 6, 3), (33, 21, 1), (32, 24, 2), (64, 48, 3))       # (W, H, B) of seeds 0 .. 3
DURATION_US = 100000


def _random_lane(W, H, seed):
    """100 ms of one lane: flickering pixels at 100 / 120 Hz (3 ON and 3 OFF events per half period), 4-event
    same-polarity bursts 200 us apart, uniform noise."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    n_flicker = min(12, W * H // 4)
    flat = rng.choice(W * H, n_flicker, replace=False)
    pixels = np.stack([flat % W, flat // W], -1)
    fx, fy, ft, fp = syn.flicker_events(pixels, np.where(np.arange(n_flicker) % 2 == 0, 100, 120), DURATION_US, seed)
    n_burst = 150
    bx, by = rng.integers(0, W, n_burst), rng.integers(0, H, n_burst)
    bt, bp = rng.integers(0, DURATION_US - 800, n_burst), rng.choice(np.array([-1, 1]), n_burst)
    burst = (np.repeat(bx, 4), np.repeat(by, 4), (bt[:, None] + 200 * np.arange(4)).reshape(-1), np.repeat(bp, 4))
    n_noise = 500
    noise = (rng.integers(0, W, n_noise), rng.integers(0, H, n_noise), rng.integers(0, DURATION_US, n_noise),
             rng.choice(np.array([-1, 1]), n_noise))
    return _merge((fx, fy, ft, fp), burst, noise)


def random_case(seed, sliced):
    """Seed ``seed`` as one push, or (``sliced``) as one push per millisecond."""
    W, H, B = RANDOM_SHAPES[seed]
    lanes = {b: _random_lane(W, H, 10 * seed + b) for b in range(B)}
    if not sliced:
        pushes = [push(lanes)]
    else:
        pushes = []
        for lo in range(0, DURATION_US, 1000):
            part = {}
            for b, ev in lanes.items():
                m = (ev[2] >= lo) & (ev[2] < lo + 1000)
                if m.any():
                    part[b] = tuple(v[m] for v in ev)
            pushes.append(push(part))
    return _case(f"random-seed{seed}-" + ("1ms" if sliced else "whole"), B, W, H, True, 1000, pushes)


_CASES = None


def cases():
    """Every case, built once."""
    global _CASES
    if _CASES is None:
        out = [hand_100hz(), hand_out_of_band(), hand_stops(), hand_hysteresis(), hand_no_predecessor(), hand_trail_gaps(),
               hand_alternating(), hand_chained(), hand_equal_timestamps(), three_lanes(),
               not_of_this_sensor([5, -1, -1, -1]), long_runs(True, None, "flicker"), long_runs(None, 300, "trail"),
               long_runs(True, 300, "both")]
        for seed in range(len(RANDOM_SHAPES)):
            out += [random_case(seed, False), random_case(seed, True)]
        _CASES = out
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def reference(case):
    """Per push of a case, from ``flicker_definition`` alone: ``(outcomes, state after the push, cumulative (flicker [B],
    trail [B]), status word)``; computed once per case and left unchanged."""
    if "_ref" not in case:
        from dagr_amd.streaming import flicker_definition, flicker_state
        B, W, H = case["B"], case["W"], case["H"]
        state = flicker_state(B, W, H)
        removed = [np.zeros(B, np.int64), np.zeros(B, np.int64)]
        ref = []
        for s in case["pushes"]:
            out = flicker_definition(state, s["x"], s["y"], s["t"], s["p"], s["batch"], case["flicker"], case["trail_us"])
            lane_ok = (s["batch"] >= 0) & (s["batch"] < B)
            outside = (s["x"] < 0) | (s["x"] >= W) | (s["y"] < 0) | (s["y"] >= H)
            removed = [r + np.bincount(s["batch"][out == k], minlength=B) for k, r in enumerate(removed, 1)]
            ref.append((out, {k: v.copy() for k, v in state.items()}, tuple(removed), 16 if (outside & lane_ok).any() else 0))
        case["_ref"] = ref
    return case["_ref"]


def outcome_shares(case):
    """The shares of the outcomes 0, 1 and 2 among the case's events of the sensor."""
    out = np.concatenate([r[0] for r in reference(case)])
    out = out[out >= 0]
    return [float((out == k).mean()) for k in (0, 1, 2)]


def lane_outcomes(case):
    """Per lane the outcomes of its events in arrival order, over all pushes: what two chunkings of one sequence share."""
    per = [[] for _ in range(case["B"])]
    for s, r in zip(case["pushes"], reference(case)):
        for b in range(case["B"]):
            per[b].append(r[0][s["batch"] == b])
    return [np.concatenate(v) for v in per]
