"""A decoding event stream on the GPU: EventStream(decode=).step_words on the camera's words against a second stream's
step on DecodeDefinition's events, on the same engine -- detections and counts bit for bit, plain, behind downsample=,
behind the noise filter and under a cap, EVT 3.0 and EVT 2.0 --, reset(), the refusals, and the status bit of a decoded
push that exceeds max_decoded.  The steps cross the time counter's wrap."""
import numpy as np
import pytest
import torch

from dagr_amd.data.evt import encode_events
from dagr_amd.streaming import DecodeDefinition, EventStream
from dagr_amd.utils import synthetic as syn
from tests import stream_decode_cases as dc
from tests.test_stream_denoise_gpu import _dense
from tests.test_streaming_gpu import _model

pytestmark = pytest.mark.gpu

W, H, B = 320, 215, 3
WINDOW_US = 20000
T_BASE = 1 << 33
E, U = syn.edges_window, syn.uniform_window
PLAN = [({0: (E, 500, 0, 6000), 1: (U, 300, 0, 5000), 2: (E, 260, 0, 5500)}, None),
        ({1: (U, 140, 6000, 9000)}, None),
        ({}, [12000] * 3),
        ({0: (E, 410, 12000, 17000), 2: (U, 220, 12500, 16000)}, [18000] * 3),
        ({1: (E, 120, 17000, 17900)}, [45000, 18000, 45000]),
        ({0: (E, 300, 45000, 49000), 1: (U, 30, 18010, 20000), 2: (E, 7, 45500, 46000)}, None)]
_STEPS = {}


def _steps(fmt, w, h):
    """Six pushes of words on a ``w x h`` sensor (the plan of tests/test_stream_denoise_gpu.py): ``(words, lane_words,
    t_now, events)`` with the lanes' times starting 9 ms before the format's wrap."""
    if (fmt, w, h) not in _STEPS:
        rel0 = dc.WRAP_US[fmt] - 9000
        rng = np.random.default_rng(31)
        last = [None] * B
        out = []
        for k, (lanes, t_now) in enumerate(PLAN):
            words, lane_words, n_events = [], [], 0
            for b in range(B):
                if b in lanes:
                    gen, n, lo, hi = lanes[b]
                    x, y, t, p = _dense(gen, n, 50 + 3 * k + b, lo, hi, w, h)
                    t = t + rel0
                    words.append(encode_events(x, y, t, p, fmt, rng=rng, t_prev=last[b]))
                    last[b] = int(t[-1])
                    n_events += len(t)
                else:
                    words.append(np.zeros(0, np.uint16 if fmt == "evt3" else np.uint32))
                lane_words.append(len(words[-1]))
            out.append((np.concatenate(words), np.array(lane_words), None if t_now is None else
                        np.asarray(t_now, np.int64) + rel0 + T_BASE, n_events))
        _STEPS[(fmt, w, h)] = out
    return _STEPS[(fmt, w, h)]


CONFIGS = {"plain": ("evt3", dict()), "downsample": ("evt3", dict(downsample=2)),
           "denoise": ("evt3", dict(denoise_us=2000, refractory_us=1)), "capped": ("evt3", dict(max_lane_events=300, max_decoded=8000)),
           "evt2": ("evt2", dict()), "evt2-downsample-denoise": ("evt2", dict(downsample=2, denoise_us=2000, refractory_us=1))}


def _same_detections(got, want, where):
    assert len(got) == len(want) == B
    for b, (g, r) in enumerate(zip(got, want)):
        assert set(g) == set(r), (where, b)
        for key in g:
            assert torch.equal(g[key], r[key]), (where, b, key)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_step_words_equals_step_on_the_definitions_events(config):
    fmt, kw = CONFIGS[config]
    w, h = (2 * W, 2 * H) if "downsample" in kw else (W, H)
    model = _model(B)
    model.engine().set_low_latency(True)
    ref_kw = {k: v for k, v in kw.items() if k != "max_decoded"}
    stream = EventStream(model, window_us=WINDOW_US, decode=fmt, t_base=T_BASE, **kw)
    ref = EventStream(model, window_us=WINDOW_US, **ref_kw)
    assert ref.state.words is None and stream.state.words is not None
    total = 0
    for rnd in range(2):
        d = DecodeDefinition(B, fmt, w, h, t_base=T_BASE)
        for k, (words, lane_words, t_now, n_events) in enumerate(_steps(fmt, w, h)):
            x, y, t, p, batch = d.push(words, lane_words)
            assert len(t) == n_events, "the decoder does not give the encoder's events back"
            want = ref.step(np.stack([x, y], -1).reshape(-1, 2), t, p, batch=batch, t_now=t_now)
            send = words.tobytes() if k == 1 else torch.from_numpy(words.view(np.int16 if fmt == "evt3" else np.int32)).cuda() \
                if k == 3 else words
            got = stream.step_words(send, lane_words, t_now=t_now)
            _same_detections(got, want, (rnd, k))
            total += sum(int(g["scores"].shape[0]) for g in got)
            assert stream.counts().tolist() == ref.counts().tolist(), (rnd, k)
            assert np.array_equal(stream.filtered(), ref.filtered()) and np.array_equal(stream.dropped(), ref.dropped()), (rnd, k)
        assert stream.counts().sum() > 0
        counts, state = stream.decode_counts(), stream.decode_state()
        assert all(np.array_equal(counts[key], d.counts[key]) for key in d.counts) and counts["decoded"].min() > 0
        assert all(np.array_equal(state[key], d.state[key]) for key in d.state) and state["loops"].tolist() == [1] * B
        if "denoise_us" in kw:
            assert ref.filtered().min() > 0
        if "max_lane_events" in kw:
            assert ref.dropped().sum() > 0
        stream.check_status()
        stream.reset()
        ref.reset()
        assert not any(v.any() for v in stream.decode_counts().values()) and not any(v.any() for v in stream.decode_state().values())
    assert total > 0, "no step kept a detection: the comparison is empty"


def test_refusals_and_the_status_bit_of_a_full_buffer():
    model = _model(B)
    model.engine().set_low_latency(True)
    plain = EventStream(model, window_us=WINDOW_US)
    words, lane_words, t_now, _ = _steps("evt3", W, H)[0]
    with pytest.raises(ValueError, match="step_words"):
        plain.step_words(words, lane_words)
    with pytest.raises(RuntimeError, match="decode="):
        plain.decode_counts()
    for kw, name in ((dict(decode="evt4"), "decode"), (dict(decode="evt3", max_decoded=0), "max_decoded"),
                     (dict(max_decoded=5), "without decode"), (dict(decode="evt2", t_base=[1, 2]), "t_base")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    stream = EventStream(model, window_us=WINDOW_US, decode="evt3", max_decoded=10, t_base=T_BASE)
    with pytest.raises(ValueError, match="step_words"):
        stream.step(np.zeros((1, 2), np.int16), np.zeros(1, np.int64), np.ones(1, np.int8))
    with pytest.raises(ValueError, match="lane_words"):
        stream.step_words_device(words)
    with pytest.raises(ValueError, match="uint16"):
        stream.step_words_device(words.astype(np.uint32), lane_words)
    stream.step_words_device(words, lane_words)
    with pytest.raises(RuntimeError, match="max_out"):
        stream.check_status()
    d = DecodeDefinition(B, "evt3", W, H, t_base=T_BASE, max_out=10)
    d.push(words, lane_words)
    assert stream.counts().sum() == 10 and d.status == 64
    assert np.array_equal(stream.decode_counts()["decoded"], d.counts["decoded"]) and d.counts["decoded"].sum() > 10


def test_a_stream_without_decode_calls_what_it_called_before(monkeypatch):
    from tests.test_stream_denoise_gpu import STEP_ENTRIES, _record_stream_calls
    model = _model(B)
    model.engine().set_low_latency(True)
    calls = _record_stream_calls(monkeypatch)
    d = DecodeDefinition(B, "evt3", W, H, t_base=T_BASE)
    stream = EventStream(model, window_us=WINDOW_US, decode=None, max_decoded=None, t_base=None)
    st = stream.state
    assert st.words is None and "words" not in st.stages and st.lane_decoded is None
    pushes = [d.push(words, lane_words) + (t_now,) for words, lane_words, t_now, _ in _steps("evt3", W, H)[:3]]
    for x, y, t, p, batch, t_now in pushes:
        stream.step_device(np.stack([x, y], -1).reshape(-1, 2), t, p, batch=batch, t_now=t_now)
    assert [c for c in calls if c in STEP_ENTRIES or "decode" in c or "clock" in c] == ["dagr_stream_stage"] * 3, calls
    stream = EventStream(model, window_us=WINDOW_US, decode="evt3", t_base=T_BASE)
    del calls[:]
    for words, lane_words, t_now, _ in _steps("evt3", W, H)[:3]:
        stream.step_words_device(words, lane_words, t_now=t_now)
    assert [c for c in calls if c in STEP_ENTRIES or c in ("dagr_stream_decode", "dagr_stream_stage_dev_clock")] == \
        ["dagr_stream_decode", "dagr_stream_stage_dev_clock"] * 3, calls
    torch.cuda.synchronize()


def test_run_stream_script_decodes_and_prints_the_counters(tmp_path, capsys):
    """scripts/run_stream.py --decode evt3 writes the detections it writes without it, composed with the filter, the front
    and a cap, and prints the decoder's counters."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import run_stream as R
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "6", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "400000", "--downsample", "2", "--denoise_us", "300", "--max_lane_events", "2000"]
    paths = []
    for name, more in (("words", ["--decode", "evt3", "--max_decoded", "60000"]), ("events", [])):
        out = tmp_path / name
        paths.append(R.main(argv + more + ["--output_directory", str(out), "--sequence", name],
                            model_factory=lambda a_, ds, dev: (a_, model)))
    words, events = (np.load(p) for p in paths)
    assert len(events) > 0 and words.tobytes() == events.tobytes()
    printed = capsys.readouterr().out
    assert "decoded from evt3 words (" in printed and " 0 unsynced, 0 outside, 0 words skipped)" in printed
    with pytest.raises(SystemExit, match="--max_decoded"):
        R.main(argv + ["--max_decoded", "5"])
