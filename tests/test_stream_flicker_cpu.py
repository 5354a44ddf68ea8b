"""The event stream's anti-flicker and trail filters without a GPU: the hand-computed cases of tests/stream_flicker_cases.py
against the numpy definition (dagr_amd/streaming.py: flicker_definition), the chunking property, the outcome shares of the
random cases, the refusals of the options and of the entry points, StreamDefinition(flicker=, trail_us=) windows, and the
synthetic generator."""
import numpy as np
import pytest

from dagr_amd.streaming import (FLICKER_DEFAULTS, NEVER, StreamDefinition, _flicker_options, flicker_definition,
                                flicker_periods, flicker_state)
from dagr_amd.utils import synthetic as syn
from tests import stream_flicker_cases as fc

TW = 1000000
HAND = [c["name"] for c in fc.cases() if c["expect"] is not None]
RANDOM = [c["name"] for c in fc.cases() if c["name"].startswith("random-")]


@pytest.mark.parametrize("name", HAND)
def test_hand_computed_outcomes(name):
    case = fc.case(name)
    for k, (expect, ref) in enumerate(zip(case["expect"], fc.reference(case))):
        assert ref[0].tolist() == expect.tolist(), (name, k)


def test_the_hand_cases_leave_the_state_their_docstrings_state():
    ref = fc.reference(fc.case("hand-100hz"))[-1][1]
    assert ref["count"][0, 2, 3] == 7 and ref["blocking"][0, 2, 3] and ref["t_edge"][0, 2, 3] == fc.T0 + 90000
    assert np.all(ref["t_pass"] == NEVER) and not ref["p_pass"].any()              # the trail stage is off
    ref = fc.reference(fc.case("hand-no-predecessor"))[-1][1]
    assert np.all(ref["t_edge"] == NEVER) and ref["last_p"][0, 3, 2] == 1 and not ref["count"].any()
    ref = fc.reference(fc.case("hand-chained"))[-1][1]
    assert ref["t_pass"][0, 3, 3] == fc.T0 + 80002 and ref["p_pass"][0, 3, 3] == 1 and not ref["blocking"].any()
    ref = fc.reference(fc.case("hand-trail-gaps"))[-1][1]
    assert np.all(ref["t_edge"] == NEVER) and not ref["last_p"].any()              # the flicker stage is off
    # three lanes, one pixel: lane 0 ends blocked, lane 1 trailed, lane 2 did neither
    out, state, (flicker, trail), status = fc.reference(fc.case("three-lanes"))[-1]
    assert state["blocking"][:, 2, 3].tolist() == [True, False, False] and status == 0
    assert flicker[0] > 0 and flicker[1:].tolist() == [0, 0] and trail[1] > 0 and trail[2] == 0


def test_events_that_are_not_of_this_sensor():
    case = fc.case("not-of-this-sensor")
    first, ref = case["pushes"][0], fc.reference(case)
    out, state, removed, status = ref[0]
    outside = (first["x"] < 0) | (first["x"] >= 8) | (first["y"] < 0) | (first["y"] >= 6)
    assert outside.sum() == 4 and status == 16 and np.all(out[outside] == -1)
    assert first["batch"][-4:].tolist() == [5, -1, -1, -1] and np.all(out[-4:] == -1)
    assert (out >= 0).sum() == len(out) - 8
    assert sum(int(r.sum()) for r in removed) == int((out > 0).sum())
    assert [r[3] for r in ref[1:]] == [0, 0, 0, 0]
    assert len(ref[1][0]) == 0 and all(np.array_equal(ref[1][1][k], state[k]) for k in state)      # the empty push
    assert len(ref[4][0]) == 1


@pytest.mark.parametrize("name", RANDOM)
def test_every_outcome_has_its_share(name):
    """No random case degenerates into all-kept: each of kept / flicker / trail is at least 10 % of the events of the
    sensor."""
    shares = fc.outcome_shares(fc.case(name))
    print(name, shares)
    assert min(shares) >= 0.10, shares


def test_the_long_run_push_is_what_it_is_meant_to_be():
    for tag in ("flicker", "trail", "both"):
        case = fc.case("long-runs-" + tag)
        s = case["pushes"][0]
        runs = np.bincount(s["y"].astype(np.int64) * 16 + s["x"])
        assert sorted(runs[runs > 1].tolist()) == sorted(fc.LONG_RUNS + (300,)) and (runs == 1).sum() == 16
        assert len(s["t"]) % 64 != 0 and len(s["t"]) % 256 != 0
        out = fc.reference(case)[0][0]
        assert set(out[(s["x"] == 9) & (s["y"] == 7)].tolist()) == {"flicker": {0, 1}, "trail": {0, 2}, "both": {0, 1, 2}}[tag]


@pytest.mark.parametrize("seed", range(len(fc.RANDOM_SHAPES)))
def test_chunking_leaves_outcomes_and_state_unchanged(seed):
    whole, sliced = fc.case(f"random-seed{seed}-whole"), fc.case(f"random-seed{seed}-1ms")
    assert len(whole["pushes"]) == 1 and len(sliced["pushes"]) == 100
    assert sum(len(s["t"]) for s in sliced["pushes"]) == len(whole["pushes"][0]["t"]) <= 6000
    for a, b in zip(fc.lane_outcomes(whole), fc.lane_outcomes(sliced)):
        assert np.array_equal(a, b)
    end_a, end_b = fc.reference(whole)[-1], fc.reference(sliced)[-1]
    for k in end_a[1]:
        assert np.array_equal(end_a[1][k], end_b[1][k]), k
    assert all(np.array_equal(u, v) for u, v in zip(end_a[2], end_b[2]))


def test_refusals_by_name():
    who = "EventStream"
    assert _flicker_options(None, None, 3, 320, 215, who) == (None, None)
    assert _flicker_options(True, np.int64(7), 3, 320, 215, who) == (FLICKER_DEFAULTS, 7)
    opt, _ = _flicker_options(dict(max_hz=np.int32(130)), None, 1, 8, 6, who)
    assert opt == dict(FLICKER_DEFAULTS, max_hz=130) and flicker_periods(opt) == (7693, 20000)
    assert flicker_periods(FLICKER_DEFAULTS) == (2000, 20000)
    with pytest.raises(ValueError, match="no option 'hz'"):
        _flicker_options(dict(hz=100), None, 1, 8, 6, who)
    for bad in (False, 5, "on", [50, 500]):
        with pytest.raises(ValueError, match="flicker = "):
            _flicker_options(bad, None, 1, 8, 6, who)
    for bad in (dict(min_hz=50.0), dict(start=True), dict(max_count="7")):
        with pytest.raises(ValueError, match="must be an int"):
            _flicker_options(bad, None, 1, 8, 6, who)
    for bad in (dict(min_hz=0), dict(min_hz=600), dict(max_hz=1000001)):
        with pytest.raises(ValueError, match="min_hz"):
            _flicker_options(bad, None, 1, 8, 6, who)
    for bad in (dict(stop=4), dict(stop=-1), dict(start=8), dict(max_count=256, start=200)):
        with pytest.raises(ValueError, match="max_count"):
            _flicker_options(bad, None, 1, 8, 6, who)
    for bad in (0, -3, 2.5, True, "1000"):
        with pytest.raises(ValueError, match="trail_us"):
            _flicker_options(None, bad, 1, 8, 6, who)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        StreamDefinition(64, 8192, 4096, trail_us=10)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        StreamDefinition(32, 4096, 4096, downsample=2, flicker=True)              # the SENSOR's pixels count
    StreamDefinition(64, 8192, 4096)                                              # no filter, no state: nothing to refuse
    with pytest.raises(ValueError, match="flicker_definition"):
        flicker_definition(flicker_state(1, 8, 6), [0], [0], [0], [1], [0], dict(start=0))
    d = StreamDefinition(2, 8, 6, flicker=True, trail_us=5)
    assert (d.flicker, d.trail_us) == (FLICKER_DEFAULTS, 5) and d.flicker_state["t_edge"].shape == (2, 6, 8)
    with pytest.raises(ValueError, match="outside the sensor"):
        d.push([8], [0], [5], [1])


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Rejected on the host before any device work, so this runs without a GPU."""
    import ctypes
    from dagr_amd import _lib
    L = _lib.lib()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    for args in ((0, 8, 6, 100), (128, 8, 6, 100), (1, 0, 6, 100), (1, 8, 40000, 100), (1, 8, 6, 0), (64, 8192, 4096, 100)):
        assert L.dagr_stream_flicker_bytes(*args) == 0, args
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(512)      # non-NULL, aligned, never dereferenced
    assert L.dagr_stream_flicker_reset(None, 1 << 20, 1, 8, 6, 100, None) == bad and b"NULL" in L.dagr_last_error()
    assert L.dagr_stream_flicker_reset(one, 16, 1, 8, 6, 100, None) == bad
    assert b"dagr_stream_flicker_bytes" in L.dagr_last_error()

    def call(state=one, nbytes=1 << 20, B=1, max_push=100, lo=2000, hi=20000, start=4, stop=1, top=7, trail=1000, n=10,
             xy_out=two):
        return L.dagr_stream_flicker(state, nbytes, B, max_push, 8, 6, lo, hi, start, stop, top, trail, one, one, one, one, 1,
                                     n, xy_out, two, two, two, two, None, None, two, None)
    assert call(hi=0, trail=0) == bad and b"both off" in L.dagr_last_error()
    assert call(trail=-1) == bad and call(hi=-5) == bad
    assert call(lo=0) == bad and b"min_period_us" in L.dagr_last_error()
    assert call(lo=20001) == bad and call(hi=1000001) == bad
    assert call(stop=4) == bad and b"stop < start" in L.dagr_last_error()
    assert call(stop=-1) == bad and call(start=8) == bad and call(top=256) == bad
    assert call(n=101) == bad and b"max_push" in L.dagr_last_error()
    assert call(n=-1) == bad
    assert call(state=None) == bad and b"NULL" in L.dagr_last_error()
    assert call(xy_out=None) == bad and b"NULL" in L.dagr_last_error()
    assert call(xy_out=ctypes.c_void_p(258)) == bad and b"aligned" in L.dagr_last_error()
    assert call(B=200) == bad and b"out of range" in L.dagr_last_error()
    assert call(nbytes=64) == bad and b"dagr_stream_flicker_bytes" in L.dagr_last_error()
    assert call(nbytes=64, n=0) == bad


def test_stream_definition_windows_counts_and_reset():
    """The window holds the events of outcome 0 and nothing else, the clock stays the unfiltered push's, suppressed and the
    state follow the definition, and reset() returns both to their initial values."""
    case = fc.case("random-seed1-1ms")
    W, H = case["W"], case["H"]
    d = StreamDefinition(1, W, H, time_window=TW, window_us=20000, flicker=True, trail_us=1000)
    plain = StreamDefinition(1, W, H, time_window=TW, window_us=20000)
    kept = {k: [] for k in "xytp"}
    for s, r in list(zip(case["pushes"], fc.reference(case)))[:60]:
        d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
        plain.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
        for k in "xytp":
            kept[k].append(s[k][r[0] == 0])
        assert all(np.array_equal(u, v) for u, v in zip(d.suppressed, r[2]))
        assert all(np.array_equal(d.flicker_state[k], r[1][k]) for k in r[1])
    assert d.t_ref == plain.t_ref and d.t_last == plain.t_last
    x, y, t, p = (np.concatenate(kept[k]) for k in "xytp")
    m = d.t_ref[0] - t < 20000
    wx, wy, wt, wp, _ = d.window()
    assert np.array_equal(wx, x[m]) and np.array_equal(wy, y[m]) and np.array_equal(wp, p[m])
    assert np.array_equal(wt, (TW - (d.t_ref[0] - t[m])).astype(np.int32))
    assert 0 < d.counts()[0] < plain.counts()[0] and d.suppressed[0][0] > 0 and d.suppressed[1][0] > 0
    d.reset()
    fresh = flicker_state(1, W, H)
    assert not d.suppressed[0].any() and not d.suppressed[1].any()
    assert all(np.array_equal(d.flicker_state[k], fresh[k]) for k in fresh)


def test_flicker_runs_in_front_of_the_noise_filter():
    """A blocked pixel's events never stamp: an event beside it finds no support and the noise filter removes it.  With
    the stages the other way round the flicker events would have supported it."""
    sq = fc._square(10000, 100000)
    fx, fy, ft, fp = fc._one_pixel(3, 2, sq)
    ev = fc._merge((fx, fy, ft, fp), ([4], [2], [95010], [1]))
    s = fc.push({0: ev})
    d = StreamDefinition(1, 8, 6, time_window=TW, window_us=5000, flicker=True, denoise_us=100)
    d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    assert d.counts().tolist() == [0] and d.filtered[0] > 0 and d.suppressed[0][0] == 10
    only = StreamDefinition(1, 8, 6, time_window=TW, window_us=5000, denoise_us=100)
    only.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    assert only.window()[0].tolist() == [4]


def test_with_both_options_none_the_definition_is_unchanged():
    from tests import stream_denoise_cases as dc
    case = next(c for c in dc.cases() if c["name"] == "random-8x6-B3-both")
    kw = dict(time_window=TW, window_us=50000, denoise_us=case["D"], refractory_us=case["R"])
    a, b = StreamDefinition(3, 8, 6, **kw), StreamDefinition(3, 8, 6, flicker=None, trail_us=None, **kw)
    assert not hasattr(b, "flicker_state")
    for s in case["pushes"][:5]:
        for d in (a, b):
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
        assert all(np.array_equal(u, v) for u, v in zip(a.formatted() + (a.filtered,), b.formatted() + (b.filtered,)))
    assert not b.suppressed[0].any() and not b.suppressed[1].any()


def test_the_generator_is_deterministic_and_flickers_as_told():
    pixels = [(1, 2), (5, 0), (7, 5)]
    a = syn.flicker_events(pixels, [100, 120, 100], 100000, seed=3, t0=50)
    b = syn.flicker_events(pixels, [100, 120, 100], 100000, seed=3, t0=50)
    assert all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))
    x, y, t, p = a
    assert [v.dtype for v in a] == [np.int16, np.int16, np.int64, np.int8] and np.all(np.diff(t) >= 0)
    assert t.min() >= 50 and t.max() < 100050 and set(p.tolist()) == {-1, 1}
    assert sorted(set(zip(x.tolist(), y.tolist()))) == sorted(pixels)
    one = (x == 5) & (y == 0)
    assert abs(int(one.sum()) - 12 * 6) <= 6                       # 120 Hz over 100 ms: 12 periods of 3 ON + 3 OFF events
    out = flicker_definition(flicker_state(1, 8, 6), x, y, t, p, np.zeros(len(t), np.int64), True, None)
    assert 0.3 < (out == 1).mean() < 0.7                           # blocked from its sixth period on
    c = syn.flicker_events(pixels, 100, 100000, seed=4)
    assert not np.array_equal(c[2][:20], t[:20] - 50)
    assert len(syn.flicker_events([], 100, 1000, seed=0)[0]) == 0
