"""The camera-word decoder without a device: encode_events -> DecodeDefinition is the identity (wraps included), the
chunking property at every cut, the counters, the definition on hand-written words, and the refusals by name."""
import numpy as np
import pytest

from dagr_amd.data.evt import encode_events
from dagr_amd.streaming import (DECODE_COUNTERS, STATUS_BITS, DecodeDefinition, _decode_options, _decode_t_base, _lane_words,
                                words_as_array)
from tests import stream_decode_cases as dc


def _decode(case, **kw):
    d = DecodeDefinition(case["B"], case["format"], *case["sensor"], **kw)
    return d, d.push(case["words"], case["lane_words"])


def _same(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


ENCODED = [c for c in dc.all_cases() if c["events"] is not None]


@pytest.mark.parametrize("name", [c["name"] for c in ENCODED])
def test_decoding_the_encoders_words_gives_the_events_back(name):
    case = next(c for c in ENCODED if c["name"] == name)
    d, got = _decode(case)
    x, y, t, p, b = case["events"]
    assert _same(got, (x.astype(np.int16), y.astype(np.int16), t.astype(np.int64), p.astype(np.int8), b.astype(np.int32)))
    assert d.counts["decoded"].sum() == len(t) and not d.counts["unsynced"].any() and not d.counts["outside"].any()
    assert d.counts["skipped"].sum() > 0 and d.status == 0
    if name.startswith("a_"):
        wrap = dc.WRAP_US[case["format"]]
        assert t.min() < wrap <= t.max() and d.state["loops"][0] == 1, "the case does not cross the wrap"


def test_a_gap_of_several_wraps_is_followed():
    for fmt in ("evt3", "evt2"):
        wrap = dc.WRAP_US[fmt]
        t = np.array([5, wrap // 2 + 1, 3 * wrap + 17, 3 * wrap + 17, 7 * wrap - 1], np.int64)
        x, y, p = np.array([1, 2, 3, 4, 5]), np.array([9, 9, 8, 8, 8]), np.array([1, -1, 1, 1, -1])
        d = DecodeDefinition(1, fmt, 64, 48, t_base=1000)
        got = d.push(encode_events(x, y, t, p, fmt))
        assert got[2].tolist() == (t + 1000).tolist() and got[0].tolist() == x.tolist() and d.state["loops"][0] == 6
        # a second encoder call goes on from where the first stopped
        got = d.push(encode_events([7], [7], [7 * wrap + 3], [1], fmt, t_prev=int(t[-1])))
        assert got[2].tolist() == [7 * wrap + 3 + 1000] and d.state["loops"][0] == 7


@pytest.mark.parametrize("fmt", ["evt3", "evt2"])
def test_every_cut_of_a_stream_gives_the_same_events_counters_and_state(fmt):
    case = dc.encoded(fmt, dc.SMALL, 21, n_bursts=330 if fmt == "evt3" else 140)
    words = np.concatenate([case["words"][:40], case["words"]])      # (the head again: unsynced words, then a back jump)
    words = np.concatenate([np.array(dc.filler(fmt, np.random.default_rng(3), dc.SMALL, 20), words.dtype), words])
    assert 1500 < len(words) < 3000
    whole = DecodeDefinition(1, fmt, 60, 40)
    want = whole.push(words)
    assert whole.counts["unsynced"][0] > 0 and whole.counts["outside"][0] > 0 and whole.counts["decoded"][0] > 0
    for cut in range(len(words) + 1):
        d = DecodeDefinition(1, fmt, 60, 40)
        got = [np.concatenate(parts) for parts in zip(d.push(words[:cut]), d.push(words[cut:]))]
        assert _same(got, want), cut
        assert all(np.array_equal(d.counts[k], whole.counts[k]) for k in DECODE_COUNTERS), cut
        assert all(np.array_equal(v, whole.state[k]) for k, v in d.state.items()), cut


def test_the_definition_on_hand_written_words():
    case = dc.outside("evt3", dc.SMALL)
    d, (x, y, t, p, b) = _decode(case, t_base=[100])
    w, h = dc.SMALL
    assert x.tolist() == [w - 1] + list(range(w - 4, w)) + list(range(w - 10, w)) + [1]
    assert y.tolist() == [h - 1] * 15 + [0] and p.tolist() == [-1] + [1] * 4 + [-1] * 10 + [-1]
    assert set(t.tolist()) == {100 + (1 << 12) + 9}
    assert {k: int(v[0]) for k, v in d.counts.items()} == dict(decoded=16, unsynced=0, outside=2 + 20 + 6 + 1 + 6, skipped=0)
    assert d.status == 16 and d.state["base_x"][0] == 12 and d.state["y"][0] == 0
    d, (x, y, t, p, b) = _decode(dc.outside("evt2", dc.SMALL))
    assert list(zip(x.tolist(), y.tolist())) == [(w - 1, h - 1), (0, 0)] and d.counts["outside"][0] == 4 and p.tolist() == [1, 1]
    assert t.tolist() == [64 + 9] * 2
    for fmt, thr, shift in (("evt3", 2048, 12), ("evt2", 1 << 27, 6)):
        d, out = _decode(dc.jumps(fmt, dc.SMALL, 14))
        highs = (out[2] >> shift).tolist()
        assert d.state["loops"][0] == 1 and d.state["high"][0] == 953
        assert highs[0] == thr + 952 and 953 in highs and highs[-1] == (thr << 1) + 953 and sorted(highs) != highs
    d, out = _decode(dc.unsynced("evt3", dc.SMALL, 13))
    assert d.counts["unsynced"][0] > 12 + 4 and d.counts["decoded"][0] == len(out[0]) > 0
    d, out = _decode(dc.late_wrap("evt3", dc.SMALL, 12))
    assert d.state["loops"][0] == 1 and d.state["high"][0] == 10
    d, out = _decode(dc.carried_base(17))
    assert out[0].max() > 12 * dc.T and d.counts["outside"][0] == 0 and 8 * (2 * dc.T + 7) < d.state["base_x"][0]


def test_max_out_keeps_the_first_rows_and_the_state_goes_on():
    case = dc.full_vectors()
    full, want = _decode(case)
    assert len(want[0]) == 480 and want[0].tolist() == list(range(480)) and full.status == 0
    d, got = _decode(case, max_out=100)
    assert _same(got, [v[:100] for v in want]) and d.status == 64 and d.counts["decoded"][0] == 480
    assert all(np.array_equal(v, full.state[k]) for k, v in d.state.items())
    assert "max_out" in dict(STATUS_BITS)[64]


def test_lanes_and_word_buffers():
    case = dc.lanes("evt3", dc.LARGE, 15)
    d, got = _decode(case, t_base=[0, 5, 9])
    assert d.counts["decoded"][1] == 0 and d.counts["decoded"][2] > 0 and set(got[4].tolist()) == {0, 2}
    assert np.array_equal(got[2][got[4] == 2], case["events"][2][case["events"][4] == 2] + 9)
    raw = case["words"].astype("<u2").tobytes()
    assert np.array_equal(words_as_array(raw, "evt3", "t"), case["words"])
    assert np.array_equal(words_as_array(np.frombuffer(raw, np.uint8), "evt3", "t"), case["words"])
    d.reset()
    assert not any(v.any() for v in d.state.values()) and not any(v.any() for v in d.counts.values())


def test_refusals_by_name():
    with pytest.raises(ValueError, match="decode"):
        _decode_options("evt4", None, 64, 48, "t")
    with pytest.raises(ValueError, match="max_decoded"):
        _decode_options("evt3", 0, 64, 48, "t")
    with pytest.raises(ValueError, match="max_decoded"):
        _decode_options("evt3", 2.5, 64, 48, "t")
    with pytest.raises(ValueError, match="sensor"):
        _decode_options("evt3", None, 40000, 48, "t")
    with pytest.raises(ValueError, match="t_base"):
        _decode_t_base([1, 2], 3, "t")
    with pytest.raises(ValueError, match="t_base"):
        _decode_t_base(1.5, 1, "t")
    assert _decode_t_base(7, 3, "t").tolist() == [7, 7, 7]
    with pytest.raises(ValueError, match="lane_words is required"):
        _lane_words(None, 5, 2, "t")
    with pytest.raises(ValueError, match="lane_words"):
        _lane_words([2, 2], 5, 2, "t")
    with pytest.raises(ValueError, match="whole number"):
        words_as_array(b"abc", "evt3", "t")
    with pytest.raises(ValueError, match="uint32"):
        words_as_array(np.zeros(3, np.uint16), "evt2", "t")
    with pytest.raises(ValueError, match="non-decreasing"):
        encode_events([1, 1], [1, 1], [5, 4], [1, 1], "evt3")
    with pytest.raises(ValueError, match="11 bits"):
        encode_events([2048], [1], [5], [1], "evt2")
    with pytest.raises(ValueError, match="format"):
        encode_events([1], [1], [5], [1], "evt1")
