"""CPU suite: the event stream's noise filter as StreamDefinition states it (dagr_amd/streaming.py) -- three hand-computed
cases, chunking invariance, the refusals by name, and the unchanged definition when both options are None."""
import numpy as np
import pytest

from dagr_amd.streaming import NEVER, StreamDefinition, denoise_definition
from tests import stream_denoise_cases as dc

TW = 1000000


def _definition(case, **over):
    kw = dict(time_window=TW, window_us=TW, denoise_us=case["D"], refractory_us=case["R"])
    kw.update(over)
    return StreamDefinition(case["B"], case["W"], case["H"], **kw)


def _by_name(name):
    return next(c for c in dc.cases() if c["name"] == name)


@pytest.mark.parametrize("name", ["hand-boundaries", "hand-edges", "hand-carried"])
def test_hand_computed_keep_masks(name):
    """The expected masks are written out in tests/stream_denoise_cases.py, event by event with the reason."""
    case = _by_name(name)
    maps = np.full((case["B"], case["H"], case["W"]), NEVER, np.int64)
    removed = 0
    for s, want in zip(case["pushes"], case["expect"]):
        keep = denoise_definition(maps, s["x"], s["y"], s["t"], s["batch"], case["D"], case["R"])
        assert keep.tolist() == want.tolist()
        removed += int((~want).sum())
    # every event stamped, kept or not
    stamped = {(int(b), int(y), int(x)) for s in case["pushes"] for b, y, x in zip(s["batch"], s["y"], s["x"])}
    assert int((maps != NEVER).sum()) == len(stamped)
    d = _definition(case, window_us=1000)
    for s in case["pushes"]:
        d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    assert int(d.filtered.sum()) == removed and np.array_equal(d.last_t, maps)


def test_the_random_cases_hold_what_they_are_meant_to():
    """A share of every random case is removed and a share is kept, the sizes are the ones the kernel's paths need, the
    timestamps sit above 2^33 with one gap above 2^31, and the outside cases carry events off the sensor."""
    for case in dc.cases()[3:]:
        ref = dc.reference(case)
        n = sum(len(s["t"]) for s in case["pushes"])
        kept = sum(int(r[0].sum()) for r in ref)
        assert 0.1 * n < kept < 0.9 * n, (case["name"], kept, n)
        sizes = [len(s["t"]) for s in case["pushes"]]
        assert 0 in sizes and 1 in sizes and 2 in sizes and max(sizes) >= 300, case["name"]
        assert ("large" in case["name"]) == (max(sizes) >= 6000), case["name"]
        assert set(case["pushes"][2]["batch"].tolist()) == {case["B"] - 1}
        if case["B"] == 3:
            assert set(case["pushes"][4]["batch"].tolist()) == {0, 2}
        t_all = np.concatenate([s["t"][s["batch"] == 0] for s in case["pushes"]])
        assert t_all.min() >= 1 << 33 and np.diff(t_all).max() > 1 << 31 and np.all(np.diff(t_all) >= 0)
        assert ("outside" in case["name"]) == any(r[3] == 16 for r in ref), case["name"]
        assert int(ref[-1][0].sum()) > 0, case["name"]            # fresh support after the gap


def _rechunk(case, cuts):
    """The case's events as one sequence per lane, pushed to a definition in the chunks `cuts` gives (cuts(n) -> ascending
    cut points); the lanes are independent, so one after the other."""
    d = _definition(case)
    for b in range(case["B"]):
        lane = {k: np.concatenate([s[k][s["batch"] == b] for s in case["pushes"]]) for k in ("x", "y", "t", "p")}
        n = len(lane["t"])
        edges = [0] + list(cuts(n)) + [n]
        for a, e in zip(edges[:-1], edges[1:]):
            d.push(lane["x"][a:e], lane["y"][a:e], lane["t"][a:e], lane["p"][a:e], np.full(e - a, b, np.int64))
    return d


@pytest.mark.parametrize("name", ["hand-carried", "random-8x6-B3-both", "random-16x12-B1-denoise-large",
                                  "random-33x21-B3-refractory"])
def test_chunking_invariance(name):
    """One push, 1-event pushes and random cuts leave identical windows (the survivors since the case's last gap), maps
    and filtered counts."""
    case = dict(_by_name(name))
    if "large" in name:
        case["pushes"] = case["pushes"][:5]               # (1-event pushes of the large push add nothing but time)
    rng = np.random.Generator(np.random.PCG64(9))
    whole = _rechunk(case, lambda n: [])
    single = _rechunk(case, lambda n: range(1, n))
    cut = _rechunk(case, lambda n: sorted(set(rng.integers(0, n + 1, 7).tolist())))
    assert whole.filtered.sum() > 0 and whole.counts().sum() > 0
    for other in (single, cut):
        assert np.array_equal(whole.last_t, other.last_t)
        assert np.array_equal(whole.filtered, other.filtered)
        for u, v in zip(whole.window(), other.window()):
            assert np.array_equal(u, v)


def test_refusals_by_name():
    for kw in (dict(denoise_us=0), dict(denoise_us=-5), dict(denoise_us=1.5), dict(denoise_us=True), dict(denoise_us="10")):
        with pytest.raises(ValueError, match="denoise_us"):
            StreamDefinition(1, 8, 6, **kw)
    for kw in (dict(refractory_us=0), dict(refractory_us=-1), dict(refractory_us=2.0), dict(refractory_us=False)):
        with pytest.raises(ValueError, match="refractory_us"):
            StreamDefinition(1, 8, 6, **kw)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        StreamDefinition(64, 8192, 4096, denoise_us=10)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        StreamDefinition(32, 4096, 4096, downsample=2, refractory_us=10)          # the SENSOR's pixels count
    StreamDefinition(64, 8192, 4096)                                              # no filter, no stamps: nothing to refuse
    d = StreamDefinition(2, 8, 6, denoise_us=np.int64(7), refractory_us=3)
    assert (d.denoise_us, d.refractory_us) == (7, 3) and d.last_t.shape == (2, 6, 8) and np.all(d.last_t == NEVER)
    with pytest.raises(ValueError, match="outside the sensor"):
        d.push([8], [0], [5], [1])
    assert np.all(d.last_t == NEVER) and not d.filtered.any()


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Rejected on the host before any device work, so this runs without a GPU."""
    import ctypes
    from dagr_amd import _lib
    L = _lib.lib()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    for args in ((0, 8, 6, 100), (128, 8, 6, 100), (1, 0, 6, 100), (1, 8, 40000, 100), (1, 8, 6, 0), (64, 8192, 4096, 100)):
        assert L.dagr_stream_denoise_bytes(*args) == 0, args
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(512)      # non-NULL, aligned, never dereferenced
    assert L.dagr_stream_denoise_reset(None, 1 << 20, 1, 8, 6, 100, None) == bad and b"NULL" in L.dagr_last_error()
    assert L.dagr_stream_denoise_reset(one, 16, 1, 8, 6, 100, None) == bad
    assert b"dagr_stream_denoise_bytes" in L.dagr_last_error()

    def call(state=one, nbytes=1 << 20, B=1, max_push=100, D=5, R=5, n=10, xy_out=two):
        return L.dagr_stream_denoise(state, nbytes, B, max_push, 8, 6, D, R, one, one, one, one, 1, n, xy_out, two, two, two,
                                     two, None, two, None)
    assert call(D=0, R=0) == bad and b"both off" in L.dagr_last_error()
    assert call(D=-1) == bad and call(R=-3) == bad
    assert call(n=101) == bad and b"max_push" in L.dagr_last_error()
    assert call(n=-1) == bad
    assert call(state=None) == bad and b"NULL" in L.dagr_last_error()
    assert call(xy_out=None) == bad and b"NULL" in L.dagr_last_error()
    assert call(xy_out=ctypes.c_void_p(258)) == bad and b"aligned" in L.dagr_last_error()
    assert call(B=200) == bad and b"out of range" in L.dagr_last_error()
    assert call(nbytes=64) == bad and b"dagr_stream_denoise_bytes" in L.dagr_last_error()


def test_filtered_counts_and_reset():
    case = _by_name("random-8x6-B3-both")
    d = _definition(case)
    for s, r in zip(case["pushes"], dc.reference(case)):
        d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
        assert np.array_equal(d.filtered, r[2]) and np.array_equal(d.last_t, r[1])
    assert d.filtered.sum() > 0
    d.reset()
    assert not d.filtered.any() and np.all(d.last_t == NEVER)


def test_the_clock_is_the_unfiltered_push():
    """A lane whose whole push is filtered away still moves its clock: t_ref is its newest unfiltered event."""
    d = StreamDefinition(1, 8, 6, time_window=TW, window_us=100, denoise_us=50)
    d.push([1, 2], [1, 1], [1000, 1010], [1, 1])
    assert d.counts().tolist() == [1] and d.t_ref == [1010]
    d.push([6], [4], [1105], [1])                       # unsupported: filtered, but the window moves to 1105
    assert d.t_ref == [1105] and d.t_last == [1105] and d.counts().tolist() == [1] and d.filtered.tolist() == [2]
    d.push([6], [5], [1110], [1])                       # supported by the filtered event's stamp; (2,1,1010) is 100 old: out
    assert d.counts().tolist() == [1] and d.window()[0].tolist() == [6]


def test_with_both_options_none_the_definition_is_unchanged():
    """The windows of the existing stream tests' sequences (plain, downsampling, capped) are the same with the arguments
    passed as None as without them, and no stamp map exists."""
    from tests import stream_cap_cases as cc
    from tests import stream_downsample_cases as sc
    plain = dict(time_window=sc.TW, window_us=sc.WINDOW_US, downsample=sc.F, sensor_size=(sc.W_IN, sc.H_IN))
    a, b = StreamDefinition(sc.B, sc.W, sc.H, **plain), StreamDefinition(sc.B, sc.W, sc.H, denoise_us=None, refractory_us=None,
                                                                       **plain)
    assert not hasattr(b, "last_t")
    for s in sc.sequence():
        for d in (a, b):
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        for u, v in zip(a.formatted() + (a.counts(), a.change_map), b.formatted() + (b.counts(), b.change_map)):
            assert np.array_equal(u, v)
    assert not b.filtered.any()
    # the capped staging sequence
    capped = dict(time_window=cc.TW, window_us=cc.WINDOW_US, max_lane_events=cc.N_STAGE)
    a, b = StreamDefinition(cc.B, cc.W, cc.H, **capped), StreamDefinition(cc.B, cc.W, cc.H, denoise_us=None,
                                                                       refractory_us=None, **capped)
    for s in cc.stage_sequence():
        for d in (a, b):
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        for u, v in zip(a.formatted() + (a.counts(), a.dropped), b.formatted() + (b.counts(), b.dropped)):
            assert np.array_equal(u, v)
    assert a.dropped.sum() > 0
