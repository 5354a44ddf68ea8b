"""EventStream on a --use_image model: the image branch runs once per frame.  B = 2, resnet18, the engine suite's small
sensor (320x215), latency mode (two captured graphs) and throughput mode (launch by launch).

Reference values of held steps come from a SECOND ``WindowEngine(model)`` that the stream never touches: it runs
``forward_detections(window, image_handle=image_handle_from(clones of stream.held_maps()))``, the launch-by-launch
window.  Given the same maps it runs the same deterministic event kernels as the stream, so the comparison is
``torch.equal``; the image branch itself (whose library kernels differ in their last bits from run to run) is not run
again on either side."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import model as om
from dagr_amd.streaming import EventStream, StreamDefinition, frame_definition
from dagr_amd.utils import synthetic as syn
from dagr_amd.utils.testing_weights import randomize_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
TW = 1000000
WINDOW_US = 20000
T0 = (1 << 33) + 777
FRAME_SIZE = (W + 7, H + 4)                  # raw frames a little larger than the crop (factors 1: no downsample)

_MODELS, _REF = {}, {}


def _model(batch_size=B, **over):
    from dagr_amd.model.networks.dagr import DAGR
    key = (batch_size, tuple(sorted(over.items())))
    if key not in _MODELS:
        torch.manual_seed(12)
        args = om.default_args(batch_size=batch_size, **over)
        model = randomize_(DAGR(args, height=H, width=W), seed=12).eval().cuda()
        model.cache_luts(width=W, height=H, radius=args.radius)
        _MODELS[key] = model
    m = _MODELS[key]
    m.conf_threshold, m.nms_threshold, m.check_device_status = 0.001, 0.65, True
    return m


def _image_model():
    return _model(B, use_image=True, img_net="resnet18")


def _ref_engine(model):
    """The second engine: built once, never handed a stream."""
    from dagr_amd.engine import WindowEngine
    if id(model) not in _REF:
        _REF[id(model)] = WindowEngine(model)
    return _REF[id(model)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _push(k, sizes=(901, 650), lanes=B):
    """Step k's new events: uniform events of 5 ms per lane, absolute int64 timestamps."""
    parts = []
    for b, n in enumerate(sizes[:lanes]):
        x, y, t, p = syn.uniform_window(n, W, H, 300 + 2 * k + b, window_us=5000, time_window=5000)
        parts.append((x, y, np.int64(T0 + 5000 * k) + t.astype(np.int64), p, np.full(n, b, np.int64)))
    cat = [np.concatenate([q[i] for q in parts]) for i in range(5)]
    return dict(x=cat[0].astype(np.int16), y=cat[1].astype(np.int16), t=cat[2], p=cat[3].astype(np.int8), batch=cat[4])


def _step(stream, d, s, **kw):
    """One step of the stream and of the definition: (out, det, n_keep) clones and the definition's window on the device."""
    d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], **kw)
    got = (stream.outputs.clone(), det.clone(), nk.clone())
    return got, tuple(_dev(v) for v in d.formatted())


def _clone_maps(maps):
    feats, cnn_out = maps
    return [f.clone() for f in feats], {k: [o.clone() for o in v] for k, v in cnn_out.items()}


def _reference(ref, window, maps):
    """(out, det, n_keep) of the second engine on ``window`` with the given maps (used as they are: pass clones)."""
    det, nk = ref.forward_detections(*window, image_handle=ref.image_handle_from(*maps))
    det, nk = det.clone(), nk.clone()
    out = ref.forward_raw(*window, image_handle=ref.image_handle_from(*maps)).clone()
    return out, det, nk


def _assert_equal(got, want, where):
    (out, det, nk), (out_w, det_w, nk_w) = got, want
    assert torch.equal(out, out_w), where
    assert torch.equal(nk, nk_w), where
    for b in range(nk.shape[0]):
        n = int(nk[b])
        assert torch.equal(det[b, :n], det_w[b, :n]), (where, b)


def _images(*seeds):
    return [torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(s)).cuda() for s in seeds]


def _warm(model, latency):
    """An engine in the asked mode whose lazy one-time work is done and, in latency mode, whose two graphs are captured
    (two eager runs and the capture for the frame body, one eager run and the capture for the held body)."""
    eng = model.engine().set_low_latency(latency)
    stream = EventStream(model, window_us=WINDOW_US)
    img = _images(5)[0]
    with torch.no_grad():
        for k in range(3):
            s = _push(40 + k)
            stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], image=img)
        for k in range(3, 5):
            s = _push(40 + k)
            stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"])
    torch.cuda.synchronize()
    assert (stream.frame_steps, stream.held_steps) == (3, 2)
    if latency:
        assert eng._wg is not None and eng._hg is not None
    return eng


def _rel_err(a, b):
    """|a - b| <= tol * (unit + |b|), unit = max(1, rms(b)) over finite entries: the engine suite's measure."""
    a, b = a.float().cpu(), b.float().cpu()
    ok = torch.isfinite(a) & torch.isfinite(b)
    a, b = a[ok], b[ok]
    unit = max(1.0, float(b.pow(2).mean().sqrt()))
    return ((a - b).abs() / (unit + b.abs())).max().item()


MODES = pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])


@MODES
def test_hold_steps_in_a_row(latency):
    """A frame step, three frame-less steps with new events, a raw frame for lane 1 only, two more frame-less steps: the
    counters follow the rule, and every held step equals the second engine on the held maps, bit for bit."""
    model = _image_model()
    eng, ref = _warm(model, latency), _ref_engine(model)
    stream = EventStream(model, window_us=WINDOW_US, frame_size=FRAME_SIZE)
    assert (stream.frame_steps, stream.held_steps) == (0, 0) and stream.held_maps() is None
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    image = _images(7)[0]
    raw = np.random.default_rng(21).integers(0, 256, (FRAME_SIZE[1], FRAME_SIZE[0], 3), dtype=np.uint8)
    # (keyword arguments of the step, frame bodies so far, held bodies so far)
    plan = [(dict(image=image), 1, 0), ({}, 1, 1), ({}, 1, 2), ({}, 1, 3),
            (dict(frame=raw, frame_lanes=[1]), 2, 3), ({}, 2, 4), ({}, 2, 5)]
    kept = 0
    with torch.no_grad():
        for k, (kw, frames, helds) in enumerate(plan):
            got, window = _step(stream, d, _push(k), **kw)
            assert (stream.frame_steps, stream.held_steps) == (frames, helds), k
            maps = stream.held_maps()
            assert maps is not None, k
            if not kw:                                    # a held step: the second engine on the same maps
                _assert_equal(got, _reference(ref, window, _clone_maps(maps)), k)
                assert stream.held_maps()[0] is maps[0]              # (the second engine's calls touch no hold)
            kept += int(got[2].sum())
            if "frame" in kw:                             # lane 1 is the raw frame's image, lane 0 kept its own
                assert torch.equal(stream.state.image[1].cpu(), frame_definition(raw, 1, 1, W, H))
                assert torch.equal(stream.state.image[0], image[0])
    assert kept > 0, "no step kept a detection: the comparison is empty"
    if latency:
        assert eng._wg is not None and eng._hg is not None, "both bodies are captured"
    stream.check_status()
    assert stream.counts().tolist() == d.counts().tolist()
    stream.reset()
    assert (stream.frame_steps, stream.held_steps) == (0, 0)
    eng.set_low_latency(True)


@MODES
def test_a_held_step_reads_the_held_maps(latency):
    """Scale the first held feature map in place after a frame step: the next held step equals the second engine on the
    MODIFIED maps and differs from it on the unmodified clones."""
    model = _image_model()
    eng, ref = _warm(model, latency), _ref_engine(model)
    stream = EventStream(model, window_us=WINDOW_US)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    with torch.no_grad():
        _step(stream, d, _push(0), image=_images(9)[0])
        before = _clone_maps(stream.held_maps())
        stream.held_maps()[0][0].mul_(1.5)
        after = _clone_maps(stream.held_maps())
        assert not torch.equal(before[0][0], after[0][0])
        got, window = _step(stream, d, _push(1))
        assert (stream.frame_steps, stream.held_steps) == (1, 1)
        _assert_equal(got, _reference(ref, window, after), "modified maps")
        assert not torch.equal(got[0], _reference(ref, window, before)[0])
    eng.set_low_latency(True)


@MODES
@pytest.mark.parametrize("case", ["plain_call_with_another_frame", "threshold_change"])
def test_what_rewrites_the_maps_makes_the_next_step_a_frame_step(case, latency):
    model = _image_model()
    eng = _warm(model, latency)
    stream = EventStream(model, window_us=WINDOW_US)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    frame, other = _images(7, 8)
    try:
        with torch.no_grad():
            _step(stream, d, _push(0), image=frame)
            _, window = _step(stream, d, _push(1))
            assert (stream.frame_steps, stream.held_steps) == (1, 1)
            if case == "plain_call_with_another_frame":
                eng.forward_detections(*window, image=other)
            else:
                model.conf_threshold = 0.002
            assert stream.held_maps() is None or case == "threshold_change"      # (the threshold is read by the step)
            got, window = _step(stream, d, _push(2))
            assert (stream.frame_steps, stream.held_steps) == (2, 1), "the step after the invalidation is a frame step"
            want = eng.forward_raw(*window, image=frame).clone()
            err, err_other = _rel_err(got[0], want), _rel_err(got[0], eng.forward_raw(*window, image=other))
            print(case, "rel err against the frame in force", err, "against the other frame", err_other)
            assert err < 1e-4 and err_other > 1e-3
            # ... and that forward_raw invalidated the hold again
            _step(stream, d, _push(3))
            assert (stream.frame_steps, stream.held_steps) == (3, 1)
            _step(stream, d, _push(4))
            assert (stream.frame_steps, stream.held_steps) == (3, 2)
    finally:
        model.conf_threshold = 0.001
        eng.set_low_latency(True)


def test_a_stream_that_outgrows_the_engine_runs_a_frame_step():
    """max_events = 1024 and the existing growth test's step totals on two lanes (804 resident, then 1304 > 1024): the step
    that grows the buffers drops both graphs and is a frame step; the steps around it are held."""
    from dagr_amd.engine import StreamState, WindowEngine
    model = _image_model()
    eng = WindowEngine(model, max_events=1024).set_low_latency(True)
    st = StreamState(B, TW, eng.device)                  # a window that never expires anything here
    d = StreamDefinition(B, W, H, time_window=TW, window_us=TW)
    frame = _images(7)[0]
    sizes = [(150, 51)] * 4 + [(301, 199)] + [(23, 16)] * 3
    want_frame_steps = [1, 1, 1, 1, 2, 2, 2, 2]
    with torch.no_grad():
        for k, lanes in enumerate(sizes):
            s = _push(k, sizes=lanes)
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
            out, _ = eng.forward_stream(st, _dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]),
                                        _dev(s["batch"]), image=frame if k == 0 else None)
            out = out.clone()
            assert st.frame_steps == want_frame_steps[k] and st.frame_steps + st.held_steps == k + 1, k
            if k == 4:
                assert eng.max_events > 1024 and st.cap == eng.max_events
                window = tuple(_dev(v) for v in d.formatted())
                err = _rel_err(out, _ref_engine(model).forward_raw(*window, image=frame))
                print("grown step: rel err against forward_raw(image=the frame in force)", err)
                assert err < 1e-4
    torch.cuda.synchronize()
    assert int(st.status) == 0 and st.lane_count.tolist() == d.counts().tolist()
    eng.check_status()


def test_refusals_by_name():
    model = _image_model()
    model.engine().set_low_latency(True)
    xy, t, p = np.zeros((0, 2), np.int16), np.zeros(0, np.int64), np.zeros(0, np.int8)
    raw = np.zeros((FRAME_SIZE[1], FRAME_SIZE[0], 3), np.uint8)
    with torch.no_grad():
        stream = EventStream(model, window_us=WINDOW_US, frame_size=FRAME_SIZE)
        with pytest.raises(RuntimeError, match="needs a frame"):                 # a first step without any frame
            stream.step_device(xy, t, p)
        with pytest.raises(ValueError, match="image= and frame="):
            stream.step_device(xy, t, p, image=_images(1)[0], frame=np.stack([raw, raw]))
        with pytest.raises(ValueError, match="frame_size"):                       # frame= on a stream built without it
            EventStream(model, window_us=WINDOW_US).step_device(xy, t, p, frame=raw, frame_lanes=[0])
        with pytest.raises(ValueError, match="name their lanes"):
            stream.step_device(xy, t, p, frame=raw)
        with pytest.raises(ValueError, match="smaller than the crop"):
            EventStream(model, window_us=WINDOW_US, frame_size=(W - 1, H))
        with pytest.raises(ValueError, match="smaller than the crop"):
            EventStream(model, window_us=WINDOW_US, downsample=2, frame_size=(2 * W, 2 * H - 1))
        with pytest.raises(ValueError, match="events-only"):
            EventStream(_model(B), window_us=WINDOW_US).step_device(xy, t, p, frame=np.stack([raw, raw]))
        assert (stream.frame_steps, stream.held_steps) == (0, 0)


def test_a_frame_for_a_lane_outside_the_batch_is_flagged_by_name():
    model = _image_model()
    model.engine().set_low_latency(True)
    model.check_device_status = False
    stream = EventStream(model, window_us=WINDOW_US, frame_size=FRAME_SIZE)
    raw = np.random.default_rng(3).integers(0, 256, (2, FRAME_SIZE[1], FRAME_SIZE[0], 3), dtype=np.uint8)
    s = _push(0)
    with torch.no_grad():
        out = stream.step(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], frame=raw, frame_lanes=[0, B])
    assert len(out) == B                                 # the call returns normally; lane 1 kept its (zero) frame
    assert float(stream.state.image[1].abs().max()) == 0.0
    assert torch.equal(stream.state.image[0].cpu(), frame_definition(raw[0], 1, 1, W, H))
    with pytest.raises(RuntimeError, match=r"lane is outside \[0, batch_size\)"):
        stream.check_status()
    stream.check_status()                                # the word is cleared
    model.check_device_status = True


def test_run_stream_raw_frames_runs_the_image_branch_once_per_frame(tmp_path, monkeypatch):
    """run_stream.py --raw_frames --downsample 2 on the synthetic source, 120 steps of 1 ms: one row block per step, and the
    frame body runs exactly as often as the source's frame index changes."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    model = _model(1, use_image=True, img_net="resnet18")
    model.engine().set_low_latency(True)
    streams = []

    class Recorded(EventStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            streams.append(self)
    monkeypatch.setattr(R, "EventStream", Recorded)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "120", "--stream", "edges", "--width", str(W),
            "--height", str(H), "--events_per_window", "200000", "--output_directory", str(tmp_path), "--sequence", "frames",
            "--downsample", "2", "--raw_frames"]
    a = C.flags("", argv, extra=R.stream_options)
    source = R.SyntheticStream(a)
    assert np.asarray(source.image(0)).shape == (2 * H, 2 * W, 3)          # sensor-size frames
    path = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    rec = np.load(path)
    t0, t1 = source.t_range()
    steps = list(range(t0 + 1000, t1 + 1, 1000))
    assert len(steps) == 120 and len(rec) > 0 and np.all(np.diff(rec["t"].astype(np.int64)) >= 0)
    assert set(rec["t"].tolist()) <= set(steps)
    changes = len(set(R._frame_index(source, t) for t in steps))
    assert changes == 3
    assert len(streams) == 1
    assert (streams[0].frame_steps, streams[0].held_steps) == (changes, 120 - changes)
    assert streams[0].state.front is not None
