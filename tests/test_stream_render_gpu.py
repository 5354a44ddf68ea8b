"""The stream's picture on the GPU: dagr_stream_render and dagr_stream_trail through the binding against the numpy
definition (dagr_amd/streaming.py: RenderDefinition) byte for byte on the scenes of tests/stream_render_cases.py; against
render_frames (the tested entry) where the two draw the same; EventStream(render=) against the definition step by step,
also capped and downsampling; and the library calls and results of streams with and without render=."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import EventStream, RenderDefinition, StreamDefinition
from dagr_amd.utils import synthetic as syn
from dagr_amd.visualization.bbox_viz import outline_colors
from dagr_amd.visualization.frames import render_frames
from tests import stream_render_cases as rc
from tests.test_stream_denoise_gpu import _dense
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import _dev, _model

pytestmark = pytest.mark.gpu

W, H, B = 320, 215, 2
TW = 1000000
WINDOW_US = 20000
TRACK = dict(max_tracks=16, max_age_us=1000)         # tracks outlive the short gaps of _pushes only: slots are freed and re-used
RENDER = dict(event_window_us=5000, trail=8, id_scale=1, linewidth=2)


# ------------------------------------------------------------------------------------------------ the kernels, scene by scene
def _track_state(ids, t_last, box, motion=False):
    """A tracker state (include/dagr_hip.h's layout) holding the given slots; labels, hits, vel and next_id are zero."""
    Bn, M = ids.shape
    parts = [ids.astype(np.int64).tobytes(), t_last.astype(np.int64).tobytes(), box.astype(np.float32).tobytes()]
    parts += [bytes(16 * Bn * M)] if motion else []
    parts += [bytes(4 * Bn * M), bytes(4 * Bn * M), bytes(8 * Bn)]
    raw = np.frombuffer(b"".join(parts), np.uint8)
    fn = _lib.lib().dagr_stream_track_cv_bytes if motion else _lib.lib().dagr_stream_track_bytes
    assert fn(Bn, M) == len(raw)
    return _dev(raw.copy())


class _Painter:
    """dagr_stream_trail / dagr_stream_render on buffers of its own, without a stream state (no events); the rings start
    out as garbage in front of their reset."""

    def __init__(self, Bn, Wn, Hn, M, T, options):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.W, self.H, self.M, self.T, self.o = Bn, Wn, Hn, M, T, options
        self.rings = None
        if T > 0:
            nbytes = self.L.dagr_stream_trail_bytes(Bn, M, T)
            assert nbytes == 12 * Bn * M + 8 * Bn * M * T
            self.rings = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
            _lib.check(self.L.dagr_stream_trail_reset(_lib.ptr(self.rings), nbytes, Bn, M, T, _lib.cur_stream(self.dev)), "reset")
        self.ws = torch.zeros((self.L.dagr_stream_render_workspace_bytes(Bn, Hn, Wn),), dtype=torch.uint8, device=self.dev)
        assert self.ws.numel() >= 8 * Bn * Hn * Wn
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.colors = _dev(options["colors"])

    def trail(self, ids, t_last, box, t_ref, motion=False):
        st = _track_state(ids, t_last, box, motion)
        _lib.check(self.L.dagr_stream_trail(_lib.ptr(self.rings), self.rings.numel(), self.B, self.M, self.T, _lib.ptr(st),
                                            st.numel(), _lib.ptr(_dev(t_ref)), _lib.cur_stream(self.dev)), "stream_trail")

    def ring_arrays(self):
        n, r = self.B * self.M, self.rings
        return (r[:8 * n].view(torch.int64).cpu().numpy().reshape(self.B, self.M),
                r[8 * n:12 * n].view(torch.int32).cpu().numpy().reshape(self.B, self.M),
                r[12 * n:].view(torch.int32).cpu().numpy().reshape(self.B, self.M, self.T, 2))

    def render(self, det, n_keep, track_id, base=None):
        P, o = _lib.ptr, self.o
        out = torch.full((self.B, self.H, self.W, 3), 0x33, dtype=torch.uint8, device=self.dev)
        det_t, nk_t = _dev(det), _dev(n_keep)
        id_t = None if track_id is None else _dev(track_id)
        base_t = None if base is None else _dev(base)
        _lib.check(self.L.dagr_stream_render(
            None, self.B, 0, -1, o["alpha"], P(det_t), P(nk_t), det.shape[1], P(id_t), P(self.rings), self.M, self.T,
            o["linewidth"], 1 if o["ids"] else 0, o["id_scale"], P(self.colors), len(o["colors"]), P(base_t),
            0 if base is None else self.H * self.W * 3, P(out), self.H, self.W, P(self.status), P(self.ws), self.ws.numel(),
            _lib.cur_stream(self.dev)), "stream_render")
        return out.cpu().numpy()


def _paint_scene(sc, options):
    """The scene through the kernels and through the definition: (frames, status, painter), (frames, definition)."""
    d = rc.run_definition(sc, options)
    p = _Painter(sc["B"], sc["W"], sc["H"], sc["M"], sc["T"], d.options)
    for ids, t_last, box, t_ref in sc["slots"] if sc["T"] > 0 else ():
        p.trail(ids, t_last, box, t_ref)
    rng = np.random.Generator(np.random.PCG64(sc["W"]))
    base = rng.integers(0, 256, (sc["B"], sc["H"], sc["W"], 3), dtype=np.uint8)
    got = p.render(sc["det"], sc["n_keep"], sc["track_id"], base)
    want = d.frames(det=sc["det"], n_keep=sc["n_keep"], track_id=sc["track_id"], base=base)
    return (got, int(p.status.item()), p), (want, d), base


@pytest.mark.parametrize("T", [0, 1, 2, 64])
@pytest.mark.parametrize("M", [1, 4, 256])
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("size", [(37, 29), (64, 48), (130, 67)], ids=["37x29", "64x48", "130x67"])
def test_the_kernels_equal_the_definition_byte_for_byte(size, Bn, M, T):
    """Below one tile, exact tiles and ragged tiles; one and three lanes, the middle one empty; every row kind of
    stream_render_cases.rows_lane0; id plates at scale 1 and 3; outlines of width 1, 2 and 3; rings that are empty, hold
    one point, wrap and do not wrap."""
    sc = rc.scene(*size, Bn, M, T)
    options = dict(trail=T, id_scale=3 if M == 4 else 1, linewidth={37: 1, 64: 2, 130: 3}[size[0]], alpha=0.5)
    (got, status, p), (want, d), base = _paint_scene(sc, options)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8].tolist()
    assert status == d.status == 0
    assert not p.ws.any(), "the call did not leave its maps zero"
    if T > 0:
        ids, counts, pts = p.ring_arrays()
        assert np.array_equal(ids, d.ring_id) and np.array_equal(counts, d.ring_count)
        live = np.minimum(counts, T)[..., None, None] > np.arange(T)[None, None, :, None]
        assert np.array_equal(np.where(live, pts, 0), np.where(live, d.ring_pt, 0))
    assert np.array_equal(p.render(sc["det"], sc["n_keep"], sc["track_id"], base), want), "a second call differs"
    if Bn == 3:
        assert np.array_equal(got[1], base[1]), "the empty lane is not its base"
    assert (got[0] != base[0]).any()


@pytest.mark.parametrize("size", [(37, 29), (130, 67)], ids=["37x29", "130x67"])
def test_a_segment_longer_than_w_plus_h_is_flagged_and_the_rest_of_the_frame_stays(size):
    sc = rc.scene(*size, 3, 4, 2, long_segment=True)
    (got, status, _), (want, d), base = _paint_scene(sc, dict(trail=2))
    assert status == d.status == 4
    assert np.array_equal(got, want)
    near = rc.scene(*size, 3, 4, 2)                         # the same scene without the jump, and without that slot's trail
    dn = rc.run_definition(near, dict(trail=2))
    dn.ring_pt[0, 3], dn.ring_count[0, 3] = 0, 0
    assert np.array_equal(got, dn.frames(det=near["det"], n_keep=near["n_keep"], track_id=near["track_id"], base=base))


def test_class_colours_and_a_class_without_one():
    """track_id = NULL: the rows take outline_colors()[class]; a class outside the table skips its row and raises bit 1."""
    sc = rc.scene(64, 48, 3, 4, 0)
    sc["det"][0, 1, 5] = 2.0                    # outline_colors() has two entries
    sc["det"][2, 3, 5] = -1.0
    d = RenderDefinition(3, 64, 48, render=True)
    assert not d.options["ids"] and d.options["trail"] == 0 and np.array_equal(d.options["colors"], outline_colors())
    p = _Painter(3, 64, 48, 4, 0, d.options)
    got = p.render(sc["det"], sc["n_keep"], None)
    assert np.array_equal(got, d.frames(det=sc["det"], n_keep=sc["n_keep"]))
    assert int(p.status.item()) == d.status == 2


@pytest.mark.parametrize("linewidth", [1, 2, 5])
def test_without_ids_and_trails_the_frame_is_render_frames(linewidth):
    """ids = False, trail = 0, track_id = NULL: the outlines of dagr_viz_render (render_frames) on the same integer rows."""
    Wn, Hn = 130, 67
    sc = rc.scene(Wn, Hn, 3, 4, 0)
    opt = RenderDefinition(3, Wn, Hn, render=dict(linewidth=linewidth)).options
    rng = np.random.Generator(np.random.PCG64(9))
    base = rng.integers(0, 256, (3, Hn, Wn, 3), dtype=np.uint8)
    got = _Painter(3, Wn, Hn, 4, 0, opt).render(sc["det"], sc["n_keep"], None, base)
    rows, ptr = [], [0]
    for b in range(3):
        for r in range(min(max(int(sc["n_keep"][b]), 0), rc.A)):
            d = sc["det"][b, r]
            if np.all(np.isfinite(d[:4])):
                rows.append([*np.floor(np.clip(d[:4], -2.0 ** 20, 2.0 ** 20)).astype(np.int64), int(d[5])])
        ptr.append(len(rows))
    none = np.zeros(0, np.int32)
    want = render_frames(base, np.arange(3), none, none, none.astype(np.int8), np.zeros(4, np.int64), boxes=np.array(rows),
                         box_ptr=np.array(ptr), linewidth=linewidth)
    assert np.array_equal(got, want.cpu().numpy())


def test_argument_errors_launch_nothing():
    L, dev = _lib.lib(), torch.device("cuda:0")
    assert L.dagr_stream_trail_bytes(1, 4, 0) == 0 and L.dagr_stream_trail_bytes(1, 4, 65) == 0
    assert L.dagr_stream_trail_bytes(1, 257, 4) == 0 and L.dagr_stream_trail_bytes(0, 4, 4) == 0
    assert L.dagr_stream_render_workspace_bytes(1, 0, 4) == 0 and L.dagr_stream_render_workspace_bytes(0, 4, 4) == 0
    p = _Painter(1, 16, 16, 4, 2, RenderDefinition(1, 16, 16, render=dict(trail=2), max_tracks=4).options)
    st = _track_state(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int64), np.zeros((1, 4, 4), np.float32))
    t_ref = _dev(np.zeros(1, np.int64))
    P, s = _lib.ptr, _lib.cur_stream(dev)
    out = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    trail = lambda **k: L.dagr_stream_trail(P(p.rings), k.get("bytes", p.rings.numel()), 1, 4, k.get("T", 2), P(st),       # noqa: E731
                                            k.get("tracks_bytes", st.numel()), P(t_ref), s)
    render = lambda **k: L.dagr_stream_render(None, 1, 0, -1, k.get("alpha", 0.5), None, None, 0, None, P(p.rings), 4, 2,  # noqa: E731
                                              k.get("linewidth", 1), 1, k.get("id_scale", 1), P(p.colors), k.get("n_colors", 32),
                                              None, 0, P(out), 16, 16, P(p.status), P(p.ws), k.get("ws_bytes", p.ws.numel()), s)
    assert trail() == 0 and render() == 0
    for bad in (dict(bytes=p.rings.numel() - 1), dict(T=3), dict(tracks_bytes=st.numel() + 8)):
        assert trail(**bad) == _lib.ENUMS["DAGR_ERR_INVALID_ARG"], bad
    for bad in (dict(alpha=1.5), dict(alpha=float("nan")), dict(linewidth=0), dict(linewidth=8), dict(id_scale=5),
                dict(n_colors=1), dict(n_colors=257), dict(ws_bytes=p.ws.numel() - 1)):
        assert render(**bad) == _lib.ENUMS["DAGR_ERR_INVALID_ARG"], bad
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_the_rings_equal_the_definition_over_a_walk_that_frees_and_reuses_slots(motion):
    """dagr_stream_trail on either tracker layout, 40 steps, trail = 8: slots are freed and taken again under new ids, a
    lane gets its instant late, rings wrap."""
    Bn, M, T = 3, 16, 8
    walk = rc.slot_walk(Bn, M)
    d = RenderDefinition(Bn, 320, 240, render=dict(trail=T), max_tracks=M)
    p = _Painter(Bn, 320, 240, M, T, d.options)
    reused = wrapped = 0
    for k, (ids, t_last, box, t_ref) in enumerate(walk):
        before = d.ring_id.copy()
        d.trail_step(ids, t_last, box, t_ref)
        p.trail(ids, t_last, box, t_ref, motion)
        got_id, got_count, got_pt = p.ring_arrays()
        assert np.array_equal(got_id, d.ring_id) and np.array_equal(got_count, d.ring_count), k
        live = np.minimum(got_count, T)[..., None, None] > np.arange(T)[None, None, :, None]
        assert np.array_equal(np.where(live, got_pt, 0), np.where(live, d.ring_pt, 0)), k
        reused += int(((before != 0) & (d.ring_id != 0) & (before != d.ring_id)).sum())
        wrapped = max(wrapped, int(d.ring_count.max()))
    assert wrapped > T and (walk[-1][0] != 0).any()
    assert len({int(i) for s in walk for i in s[0].ravel()}) > M, "no slot was ever taken again"


# ------------------------------------------------------------------------------------------------ the stream
STEPS = 30
GAPS = (1000, 1500, 500, 2000)            # the instants of steps k and k + 4 are 5000 us apart: RENDER's event window


def _pushes(w, h):
    """STEPS uneven pushes on a ``w x h`` sensor: a full window first, then 0.5 to 2 ms a step; lane 1 stays away every
    fourth step; every lane's push ends with an event AT the step's instant (age 0 now, age 5000 us four steps later)."""
    out, now = [], 0
    for k in range(STEPS):
        lo, now = now, now + (10000 if k == 0 else GAPS[k % 4])
        parts = {}
        for b in range(B):
            if b == 1 and k % 4 == 2:
                continue
            x, y, t, p = _dense(syn.edges_window, (400 - 100 * b) if k == 0 else 25 + 10 * ((k + b) % 5), 700 + 3 * k + b,
                                lo, now - 3, w, h)
            mx, my = 4 * (k % 50) + np.array([0, 1, 0, 1]), 4 * b + np.array([0, 0, 1, 1])     # four events on one 2 x 2 cell
            parts[b] = (np.append(x, mx).astype(np.int16), np.append(y, my).astype(np.int16),
                        np.append(t, [now] * 4).astype(np.int64) + rc.T0, np.append(p, [1] * 4).astype(np.int8))
        lanes = sorted(parts)
        cat = [np.concatenate([parts[b][i] for b in lanes]) for i in range(4)]
        out.append(dict(xy=np.stack(cat[:2], -1), x=cat[0], y=cat[1], t=cat[2], p=cat[3],
                        batch=np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes]),
                        t_now=np.full(B, now, np.int64) + rc.T0))
    return out


def _stream_step(stream, s):
    return stream.step_device(s["xy"], s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])


CONFIGS = {"plain": dict(), "capped": dict(max_lane_events=1200), "downsample": dict(downsample=2)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_a_drawing_stream_equals_the_definition_after_every_step(config):
    """EventStream(track=, render=) over 30 uneven pushes: render_step() after every step equals RenderDefinition fed the
    definition's window (StreamDefinition), the step's det / n_keep / track_ids and the tracker's slots -- on a black base,
    on a base per lane and on one shared base; twice in a row; with the base as output; and, before the first step and
    after reset(), the base itself."""
    kw = CONFIGS[config]
    model = _model(B)
    model.engine().set_low_latency(True)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, render=RENDER, **kw)
    sd = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **kw)
    d = RenderDefinition(B, W, H, render=RENDER, max_tracks=TRACK["max_tracks"])
    assert d.options.keys() == stream.render.keys() and all(np.array_equal(d.options[k], stream.render[k]) for k in d.options)
    rng = np.random.Generator(np.random.PCG64(17))
    bases = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    bases_t = _dev(bases)
    first = stream.render_step(bases_t)
    assert first.dtype == torch.uint8 and tuple(first.shape) == (B, H, W, 3) and torch.equal(first, bases_t)
    assert not stream.render_step().any()
    seen = dict(age0=0, at_window=0, rows=0, plates=0, trails=0, reused=0)
    ids_ever = set()
    with torch.no_grad():
        for k, s in enumerate(_pushes(*((2 * W, 2 * H) if "downsample" in kw else (W, H)))):
            sd.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
            det, n_keep = _stream_step(stream, s)
            base = (None, bases, bases[1])[k % 3]
            got = stream.render_step(None if base is None else _dev(base))
            again = stream.render_step(None if base is None else _dev(base)).clone()
            det_h, nk_h, ids_h = det.cpu().numpy(), n_keep.cpu().numpy(), stream.track_ids.cpu().numpy()
            slot_id, slot_t, slot_box = stream.state.track_slots()[:3]
            d.trail_step(slot_id, slot_t, slot_box, sd.t_ref)
            want = d.frames(lanes=sd.lanes, t_ref=sd.t_ref, det=det_h, n_keep=nk_h, track_id=ids_h, base=base)
            got_h = got.cpu().numpy()
            assert np.array_equal(got_h, want), (config, k, np.argwhere((got_h != want).any(-1))[:6].tolist())
            assert torch.equal(got, again), (config, k, "two calls after one step differ")
            for b in range(B):
                age = sd.t_ref[b] - sd.lanes[b]["t"]
                seen["age0"] += int((age == 0).sum())
                seen["at_window"] += int((age == RENDER["event_window_us"]).sum())
                n = min(max(int(nk_h[b]), 0), det_h.shape[1])
                seen["rows"] += n
                seen["plates"] += int((ids_h[b, :n] != 0).sum())
            seen["trails"] += int((d.ring_count >= 2).sum())
            ids_now = {int(i) for i in slot_id.ravel() if i}
            seen["reused"] += len(ids_now - ids_ever) if k > 5 else 0
            ids_ever |= ids_now
            if k == 7:                                      # the base as the output, per lane
                buf = bases_t.clone()
                assert stream.render_step(buf, out=buf) is buf
                assert np.array_equal(buf.cpu().numpy(), d.frames(lanes=sd.lanes, t_ref=sd.t_ref, det=det_h, n_keep=nk_h,
                                                                  track_id=ids_h, base=bases))
        trails = stream.trails()
        for b in range(B):
            want_rings = {int(d.ring_id[b, s_]): d.ring_points(b, s_).tolist() for s_ in range(TRACK["max_tracks"]) if d.ring_id[b, s_]}
            assert {i: v.tolist() for i, v in trails[b].items()} == want_rings
    assert stream.render_status() == [] and d.status == 0
    stream.check_status()
    assert all(v > 0 for v in seen.values()), seen
    stream.reset()
    assert torch.equal(stream.render_step(bases_t), bases_t) and all(not lane for lane in stream.trails())


def test_without_a_tracker_the_stream_draws_render_frames_picture():
    """EventStream(render=True) without track=: no trails, no plates, class colours -- the picture of render_frames (the
    tested entry) on the window's events and the step's rows, and the definition's."""
    model = _model(B)
    stream = EventStream(model, window_us=WINDOW_US, render=dict(linewidth=2, alpha=0.3))
    assert stream.render["trail"] == 0 and stream.render["ids"] is False and stream.state.trail_rings is None
    sd = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    d = RenderDefinition(B, W, H, render=dict(linewidth=2, alpha=0.3))
    rng = np.random.Generator(np.random.PCG64(23))
    bases = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    rows_seen = 0
    with torch.no_grad():
        for k, s in enumerate(_pushes(W, H)[:6]):
            sd.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
            det, n_keep = _stream_step(stream, s)
            got = stream.render_step(_dev(bases)).cpu().numpy()
            det_h, nk_h = det.cpu().numpy(), n_keep.cpu().numpy()
            assert np.array_equal(got, d.frames(lanes=sd.lanes, t_ref=sd.t_ref, det=det_h, n_keep=nk_h, base=bases)), k
            rows, ptr = [], [0]
            for b in range(B):
                for r in det_h[b, :int(nk_h[b])]:
                    rows.append([*np.floor(np.clip(r[:4], -2.0 ** 20, 2.0 ** 20)).astype(np.int64), int(r[5])])
                ptr.append(len(rows))
            rows_seen += len(rows)
            x, y, _, p, batch = sd.window()
            want = render_frames(bases, np.arange(B), x, y, p, np.searchsorted(batch, np.arange(B + 1)), alpha=0.3,
                                 boxes=np.array(rows).reshape(-1, 5), box_ptr=np.array(ptr), linewidth=2)
            assert np.array_equal(got, want.cpu().numpy()), k
    assert rows_seen > 0 and stream.render_status() == []
    with pytest.raises(RuntimeError, match="no rings"):
        stream.trails()
    with pytest.raises(ValueError, match="render trail = 4 needs track="):
        EventStream(model, window_us=WINDOW_US, render=dict(trail=4))
    with pytest.raises(RuntimeError, match="draws nothing"):
        EventStream(model, window_us=WINDOW_US).render_step()
    for bad in (torch.zeros((B, H, W, 3)), torch.zeros((B, H, W, 3), dtype=torch.uint8), _dev(bases)[:, :, :, :2]):
        with pytest.raises(ValueError, match="render_step base="):
            stream.render_step(bad)


# ------------------------------------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_render_adds_one_trail_call_to_a_tracking_step_and_none_without_a_tracker(latency, monkeypatch):
    """Step for step a render= tracking stream issues the library calls of the same stream without it plus exactly one
    dagr_stream_trail, the step's last call; without track= it issues none more; render_step is one dagr_stream_render; and
    detections, track_ids, track_hits and tracks() are bit-identical with and without render=."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    pushes = _pushes(W, H)[:8]
    per_stream, results = {}, {}
    for name, kw in (("warm-up", dict()), ("off", dict()), ("tracking", dict(track=TRACK)),
                     ("drawing", dict(track=TRACK, render=RENDER)), ("drawing none", dict(track=TRACK, render=None)),
                     ("drawing without a tracker", dict(render=True))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps, kept = [], []
        with torch.no_grad():
            for k, s in enumerate(pushes):
                del calls[:]
                det, n_keep = _stream_step(stream, s)
                steps.append(list(calls))
                kept.append((det.clone(), n_keep.clone()) + ((stream.track_ids.clone(), stream.track_hits.clone())
                                                             if stream.track is not None else ()))
                if stream.render is not None and k % 2:
                    del calls[:]
                    stream.render_step()
                    assert calls == ["dagr_stream_render"]
        torch.cuda.synchronize()
        per_stream[name], results[name] = steps, (kept, stream.tracks() if stream.track is not None else None)
    assert per_stream["drawing none"] == per_stream["tracking"]
    assert per_stream["drawing without a tracker"] == per_stream["off"]
    for k, (with_, without) in enumerate(zip(per_stream["drawing"], per_stream["tracking"])):
        assert with_ == without + ["dagr_stream_trail"], (k, with_, without)
    assert not any("render" in c or "trail" in c for name in ("off", "tracking") for step in per_stream[name] for c in step)
    (kept_a, tracks_a), (kept_b, tracks_b) = results["drawing"], results["tracking"]
    for k, (a, b) in enumerate(zip(kept_a, kept_b)):
        assert torch.equal(a[1], b[1]), k
        for lane in range(B):
            n = int(a[1][lane])
            assert all(torch.equal(u[lane, :n], v[lane, :n]) for u, v in zip((a[0], a[2], a[3]), (b[0], b[2], b[3]))), (k, lane)
    assert all(np.array_equal(u, v) for u, v in zip(tracks_a, tracks_b)) and sum(len(t) for t in tracks_a) > 0
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_writes_frames_and_leaves_the_detections(tmp_path, capsys):
    """scripts/run_stream.py --render DIR --render_every 3: DIR/%06d_lane0.png for every third step at the model's
    resolution, something drawn on them; detections and tracks byte for byte what they are without the flag; the render
    flags need --render, and trails need --track."""
    import os
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import run_stream as R
    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "7", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "pic", "--track", "--max_tracks", "32"]
    frames = tmp_path / "frames"
    paths = {}
    for name, extra in (("plain", []), ("drawn", ["--render", str(frames), "--render_every", "3", "--render_trail", "4",
                                                  "--render_event_window_us", "5000", "--render_id_scale", "2"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model))
    assert "3 frames drawn on the device" in capsys.readouterr().out
    for file in ("detections_pic.npy", "tracks_pic.npy"):
        with open(os.path.join(os.path.dirname(str(paths["plain"])), file), "rb") as f, \
                open(os.path.join(os.path.dirname(str(paths["drawn"])), file), "rb") as g:
            assert f.read() == g.read(), file
    assert sorted(os.listdir(frames)) == ["%06d_lane0.png" % k for k in (0, 3, 6)]
    for name in os.listdir(frames):
        img = np.asarray(Image.open(frames / name))
        assert img.shape == (H, W, 3) and img.any()

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")
    no = ["--output_directory", str(tmp_path / "no")]
    with pytest.raises(SystemExit, match="--render_trail needs --render"):
        R.main(base + no + ["--render_trail", "4"], model_factory=refuse)
    with pytest.raises(SystemExit, match="render trail = 4 needs track="):
        R.main([v for v in base if v not in ("--track", "--max_tracks", "32")] + no + ["--render", str(frames), "--render_trail", "4"],
               model_factory=refuse)
    with pytest.raises(SystemExit, match="render id_scale = 9"):
        R.main(base + no + ["--render", str(frames), "--render_id_scale", "9"], model_factory=refuse)
