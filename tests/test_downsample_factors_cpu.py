"""The integrate-and-fire downsampler at cell areas that are no power of two, without a GPU: oracle/downsample.py and the
stream's numpy definition (dagr_amd/streaming.py: StreamDefinition(downsample=(fx, fy))) against what the reference's own
scripts/downsample_events.py made of tests/downsample_factor_cases.py's inputs
(tests/golden/ref_py_downsample_factors.npz <- tests/make_golden_refpy_downsample.py), bit for bit.

At areas 2, 4 and 16 the increment is a power of two and every way of forming it gives the same bits; at 3, 6, 9, 12, 15
and 25 the reference's ``p * 1.0 / (fx * fy)`` -- the float64 quotient, added to the fp32 cell -- and an increment rounded to
fp32 first part ways, and the last test records that the fixture sees the difference."""
import numpy as np
import pytest

from oracle import downsample as od
from dagr_amd.streaming import StreamDefinition
from tests import downsample_factor_cases as fc
from tests.make_golden_refpy_downsample import fp32_increment_loop


@pytest.mark.parametrize("fx,fy", fc.CASES, ids=fc.IDS)
def test_the_inputs_are_the_ones_the_fixture_was_recorded_on(fx, fy):
    fc.check_inputs(fx, fy)
    ev0, ev1 = fc.chunks(fx, fy)
    assert len(ev0["t"]) == len(ev1["t"]) == fc.CHUNK_EVENTS and ev0["t"][-1] < ev1["t"][0]
    for ev in (ev0, ev1):
        assert np.all(np.diff(ev["t"]) >= 0) and set(np.unique(ev["p"]).tolist()) == {-1, 1}
        assert ev["x"].min() == 0 and ev["x"].max() == fc.CW * fx - 1 and ev["y"].min() == 0 and ev["y"].max() == fc.CH * fy - 1
        assert 0.68 < float((ev["p"] > 0).mean()) < 0.72
    for mask, sv, cm in fc.expected(fx, fy):
        assert cm.dtype == np.float32 and cm.shape == (fc.CH, fc.CW)
        assert int(mask.sum()) > 400                         # every cell fires several times in every chunk


@pytest.mark.parametrize("fx,fy", fc.CASES, ids=fc.IDS)
def test_the_oracle_equals_the_reference_script(fx, fy):
    fc.check_inputs(fx, fy)
    cm = None
    for c, (ev, (mask, sv, want_map)) in enumerate(zip(fc.chunks(fx, fy), fc.expected(fx, fy))):
        ids = np.arange(len(ev["t"]))
        got, cm = od.downsample_events(dict(ev, i=ids), fc.CH * fy, fc.CW * fx, fc.CH, fc.CW, change_map=cm)
        got_mask = np.zeros(len(ids), bool)
        got_mask[got["i"]] = True
        assert np.array_equal(got_mask, mask), c
        for k in ("x", "y", "t", "p"):
            assert np.array_equal(got[k].astype(np.int64), sv[k].astype(np.int64)), (c, k)
        assert cm.dtype == np.float32 and np.array_equal(cm, want_map), c


def _lane1(fx, fy):
    """Lane 1's side, from the oracle the test above holds to the fixture: per chunk (survivors, map)."""
    cm, out = None, []
    for ev in fc.chunks(fx, fy):
        sv, cm = od.downsample_events(fc.shifted(ev), fc.CH * fy, fc.CW * fx, fc.CH, fc.CW, change_map=cm)
        out.append((sv, cm.copy()))
    return out


@pytest.mark.parametrize("fx,fy", fc.CASES, ids=fc.IDS)
def test_the_stream_definition_equals_the_reference_script(fx, fy):
    """Lane 0 is fed the chunks and is compared with the fixture itself; lane 1 a shifted copy, compared with the oracle.
    The window outlives both chunks, so it holds every survivor, in order."""
    fc.check_inputs(fx, fy)
    TW = 1000000
    d = StreamDefinition(2, fc.CW, fc.CH, time_window=TW, window_us=TW, downsample=(fx, fy),
                         sensor_size=(fc.CW * fx, fc.CH * fy))
    assert d.change_map.shape == (2, fc.CH, fc.CW) and d.change_map.dtype == np.float32
    want = [dict(x=[], y=[], t=[], p=[]) for _ in range(2)]
    for c, (ev, (mask, sv0, map0), (sv1, map1)) in enumerate(zip(fc.chunks(fx, fy), fc.expected(fx, fy), _lane1(fx, fy))):
        other = fc.shifted(ev)
        n = len(ev["t"])
        d.push(*(np.concatenate([ev[k], other[k]]) for k in ("x", "y", "t", "p")), batch=np.repeat([0, 1], n))
        assert d.change_map.dtype == np.float32
        assert np.array_equal(d.change_map[0], map0), c
        assert np.array_equal(d.change_map[1], map1), c
        for lane, sv in enumerate((sv0, sv1)):
            for k in want[lane]:
                want[lane][k].append(np.asarray(sv[k]).astype(np.int64))
        x, y, t_rel, p, batch = d.window()
        for lane in range(2):
            m = batch == lane
            w = {k: np.concatenate(v) for k, v in want[lane].items()}
            assert int(m.sum()) == len(w["t"]), (c, lane)
            assert np.array_equal(x[m].astype(np.int64), w["x"]) and np.array_equal(y[m].astype(np.int64), w["y"]), (c, lane)
            assert np.array_equal(p[m].astype(np.int64), w["p"]), (c, lane)
            assert np.array_equal(t_rel[m].astype(np.int64) - TW + d.t_ref[lane], w["t"]), (c, lane)


def test_an_increment_rounded_to_fp32_first_does_not_match_the_fixture():
    """What the fixture is for: the fp32 increment (restated in the generator) keeps other events than the reference at
    areas 3, 6 and 15 and leaves another final map at 9, 12 and 25; at the control it is the same bit for bit."""
    for fx, fy in fc.CASES:
        fc.check_inputs(fx, fy)
        want, old = fc.expected(fx, fy), fp32_increment_loop(fc.chunks(fx, fy), fx, fy)
        kept = sum(int((w[0] != o[0]).sum()) for w, o in zip(want, old))
        cells = int((want[-1][2] != old[-1][1]).sum())
        print(f"{fx}x{fy}: kept flags that differ {kept}, final cells that differ {cells}")
        if (fx, fy) == fc.CONTROL:
            assert kept == 0 and cells == 0 and np.array_equal(want[0][2], old[0][1])
        elif fx * fy in fc.KEPT_SET_DIFFERS:
            assert kept > 0, (fx, fy)
        else:
            assert fx * fy in fc.FINAL_MAP_DIFFERS and cells > 0, (fx, fy)
