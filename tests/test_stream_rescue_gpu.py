"""The stream tracker's second association round on the GPU: dagr_stream_track_rescue and dagr_stream_track_cv_rescue
through the binding against the numpy definition (dagr_amd/streaming.py: TrackDefinition(rescue=)) bit for bit after every
step of every case of tests/stream_rescue_cases.py and of the seeded walks; against dagr_stream_track / dagr_stream_track_cv
themselves where no score lies in the band; their refusals; the flicker through a stream's own tracker state;
EventStream(track=, rescue=) against a definition fed with every step's own detections, in latency and in throughput mode,
with and without motion=, and behind the frame and held steps of a --use_image model; the library calls of streams with and
without the round; and scripts/run_stream.py --track_low_score."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import EventStream, TrackDefinition, _motion_options, _rescue_options, _track_options
from dagr_amd.utils import synthetic as syn
from tests import stream_rescue_cases as rc
from tests.test_stream_motion_gpu import _Tracker as _MotionTracker
from tests.test_stream_track_gpu import STEP_ENTRIES, _record_calls
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_streaming_gpu import _chunk, _dev, _model, _push

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
WINDOW_US = 20000
SENTINEL = -7


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Tracker:
    """dagr_stream_track_rescue (motion None) or dagr_stream_track_cv_rescue on a state of its own, made and emptied by the
    base entry's _bytes and _reset; the state starts out as garbage in front of its reset, every output as the sentinel -7."""

    def __init__(self, B_, A, track, motion, rescue):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.o = B_, A, _track_options(track, "test")
        self.m = _motion_options(motion, self.o, "test")
        self.r = _rescue_options(rescue, self.o, "test")
        self.M = M = self.o["max_tracks"]
        self.family = "dagr_stream_track" if self.m is None else "dagr_stream_track_cv"
        self.nbytes = getattr(self.L, self.family + "_bytes")(B_, M)
        assert self.nbytes == (40 if self.m is None else 56) * B_ * M + 8 * B_
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(getattr(self.L, self.family + "_reset")(_lib.ptr(self.state), self.nbytes, B_, M, _lib.cur_stream(self.dev)),
                   self.family + "_reset")
        full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=self.dev)           # noqa: E731
        self.out = dict(ids=full((B_, A), torch.int64), hits=full((B_, A), torch.int32))
        if self.m is not None:
            self.out.update(box=full((B_, A, 4), torch.float32), vel=full((B_, A, 4), torch.float32),
                            coast_id=full((B_, M), torch.int64), coast_box=full((B_, M, 4), torch.float32),
                            coast_label=full((B_, M), torch.int32), coast_age=full((B_, M), torch.int64),
                            n_coast=full((B_,), torch.int32))
        self.untracked = torch.zeros((B_,), dtype=torch.int64, device=self.dev)
        self.rescued = torch.zeros((B_,), dtype=torch.int64, device=self.dev)

    def refill(self):
        for t in self.out.values():
            t.fill_(SENTINEL)

    def call(self, s, **over):
        P = _lib.ptr
        det, n_keep, t_ref = _dev(s["det"]), _dev(s["n_keep"]), _dev(s["t_ref"])
        a = dict(tracks=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, iou=self.o["iou"], age=self.o["max_age_us"],
                 min_score=self.o["min_score"], det=P(det), n_keep=P(n_keep), A=self.A, t_ref=P(t_ref),
                 untracked=P(self.untracked), low_score=self.r["low_score"], low_iou=self.r["iou"], rescued=P(self.rescued),
                 **{k: P(v) for k, v in self.out.items()})
        if self.m is not None:
            a.update(alpha=self.m["alpha"], beta=self.m["beta"])
        a.update(over)
        gains = [] if self.m is None else [a["alpha"], a["beta"]]
        outputs = [] if self.m is None else [a[k] for k in ("box", "vel", "coast_id", "coast_box", "coast_label", "coast_age",
                                                             "n_coast")]
        rc_ = getattr(self.L, self.family + "_rescue")(a["tracks"], a["bytes"], a["B"], a["M"], a["iou"], a["age"], a["min_score"],
                                                       *gains, a["det"], a["n_keep"], a["A"], a["t_ref"], a["ids"], a["hits"],
                                                       *outputs, a["untracked"], a["low_score"], a["low_iou"], a["rescued"],
                                                       _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc_

    def slots(self):
        """The state through the layouts include/dagr_hip.h documents: (id, t_last, box, [vel,] label, hits, next_id)."""
        n, raw, B_, M = self.B * self.M, self.state, self.B, self.M
        out = [raw[:8 * n].view(torch.int64).view(B_, M), raw[8 * n:16 * n].view(torch.int64).view(B_, M),
               raw[16 * n:32 * n].view(torch.float32).view(B_, M, 4)]
        at = 32 * n
        if self.m is not None:
            out.append(raw[at:at + 16 * n].view(torch.float32).view(B_, M, 4))
            at += 16 * n
        out += [raw[at:at + 4 * n].view(torch.int32).view(B_, M), raw[at + 4 * n:at + 8 * n].view(torch.int32).view(B_, M),
                raw[at + 8 * n:].view(torch.int64)]
        return tuple(t.cpu().numpy() for t in out)


def _assert_same_slots(got, want, where):
    """Slot by slot: the ids (0: free) and next_id everywhere, the other fields where a track lives."""
    assert len(got) == len(want), where
    assert rc.same(got[0], want[0]), (where, "ids of the slots")
    assert rc.same(got[-1], want[-1]), (where, "next_id")
    live = want[0] != 0
    for k in range(1, len(want) - 1):
        assert rc.same(got[k][live], want[k][live]), (where, "slot field", k)


def _assert_step(tr, want, s, where):
    """One step's outputs against the definition's: the rows below n_keep and the first n_coast coast entries are the
    definition's, everything behind them is still the sentinel; untracked, rescued, the slots."""
    out = {name: t.cpu().numpy() for name, t in tr.out.items()}
    for b in range(tr.B):
        n = min(max(int(s["n_keep"][b]), 0), tr.A)
        for name in ("ids", "hits") + (("box", "vel") if tr.m is not None else ()):
            assert rc.same(out[name][b, :n], want[name][b, :n]), (where, b, name)
            assert np.all(out[name][b, n:] == SENTINEL), (where, b, name, "behind n_keep")
        if tr.m is not None:
            c = int(want["n_coast"][b])
            assert int(out["n_coast"][b]) == c, (where, b, "n_coast")
            for name, ref in zip(("coast_id", "coast_box", "coast_label", "coast_age"), want["coast"]):
                assert rc.same(out[name][b, :c], ref[b, :c]), (where, b, name)
                assert np.all(out[name][b, c:] == SENTINEL), (where, b, name, "behind n_coast")
    assert rc.same(tr.untracked.cpu().numpy(), want["untracked"]), (where, "untracked")
    assert rc.same(tr.rescued.cpu().numpy(), want["rescued"]), (where, "rescued")
    _assert_same_slots(tr.slots(), want["slots"], where)
    return out


def _run_case(case):
    tr = _Tracker(case["B"], case["A"], case["track"], case["motion"], case["rescue"])
    steps, d = rc.run_definition(case)
    for k, (s, want) in enumerate(zip(case["steps"], steps)):
        tr.refill()
        _lib.check(tr.call(s), tr.family + "_rescue")
        out = _assert_step(tr, want, s, (case["name"], k))
        if case["expect"] is not None:
            rc.check_expectation(case, k, out["ids"], out["hits"], tr.untracked.cpu().numpy(), tr.rescued.cpu().numpy())
    return tr, d


@pytest.mark.parametrize("name", [c["name"] for c in rc.cases()])
def test_the_rescue_entries_equal_the_definition_after_every_step(name):
    """Bit for bit after every step, without and with the motion model: ids, hits, `untracked`, `rescued`, the slots and
    next_id, with motion the filtered boxes, the velocities and the coast list; the sentinel behind n_keep and behind
    n_coast; and the case's written-out expectation.  Among the cases: the flicker, 560 low rows against the cap of 256,
    a low row in front of a high row, the band's edges and a NaN score, three lanes of which one has no instant."""
    _run_case(next(c for c in rc.cases() if c["name"] == name))


@pytest.mark.parametrize("max_tracks,motion,iou", rc.WALKS)
def test_the_walks_equal_the_definition_at_every_step(max_tracks, motion, iou):
    """B = 3, A = 64, half of the rows under min_score: hundreds of rescued matches a walk (tests/test_stream_rescue_cpu.py
    holds the walks to at least 200); 8 slots overflow, 130 slots fill a thread's second and third register."""
    _, d = _run_case(rc.walk(max_tracks, motion, iou))
    assert d.events["rescued"] >= 200 and d.events["retired"] > 0 and d.events["spawned"] > 0, d.events


@pytest.mark.parametrize("name", [c["name"] for c in rc.neutral_cases()])
def test_with_an_empty_band_the_rescue_entries_leave_what_the_base_entries_leave(name):
    """Every existing case and walk through the new entry and through the existing one, side by side: after every step the
    outputs, `untracked` and every byte of the state are equal, and `rescued` stays 0."""
    case = next(c for c in rc.neutral_cases() if c["name"] == name)
    assert rc.scores_in_band(case, case["rescue"]["low_score"]) == 0
    new = _Tracker(case["B"], case["A"], case["track"], case["motion"], case["rescue"])
    if case["motion"] is None:
        old = _PlainTracker(case["B"], case["A"], case["track"])
        old_out = dict(ids=old.ids, hits=old.hits)
    else:
        old = _MotionTracker(case["B"], case["A"], case["track"], case["motion"])
        old_out = old.out
    assert sorted(old_out) == sorted(new.out)
    for k, s in enumerate(case["steps"]):
        new.refill()
        for t in old_out.values():
            t.fill_(SENTINEL)
        _lib.check(new.call(s), new.family + "_rescue")
        _lib.check(old.call(s), new.family)
        for name_, t in old_out.items():
            assert torch.equal(new.out[name_].view(torch.uint8), t.view(torch.uint8)), (name, k, name_)
        assert torch.equal(new.untracked, old.untracked) and torch.equal(new.state, old.state), (name, k)
        assert not new.rescued.any(), (name, k)


@pytest.mark.parametrize("motion", [None, True], ids=["plain", "motion"])
def test_argument_errors_launch_nothing(motion):
    case = next(c for c in rc.cases() if c["name"] == "three-lanes-count-on-their-own" + ("-with-motion" if motion else ""))
    tr, d = _run_case(case)
    assert tr.slots()[0].any() and tr.rescued.any()
    before, s = tr.state.clone(), case["steps"][-1]
    outs, untracked, rescued = {k: v.clone() for k, v in tr.out.items()}, tr.untracked.clone(), tr.rescued.clone()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    nan = float("nan")
    refusals = [(dict(tracks=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(t_ref=None), b"NULL"), (dict(ids=None), b"NULL"),
                (dict(det=None), b"NULL"), (dict(bytes=tr.nbytes - 1), b"smaller"), (dict(M=0), b"max_tracks"),
                (dict(M=257), b"max_tracks"), (dict(iou=0.0), b"iou"), (dict(iou=nan), b"iou"), (dict(age=-1), b"max_age_us"),
                (dict(B=0), b"out of range"), (dict(A=-1), b"A out of range"),
                (dict(tracks=ctypes.c_void_p(tr.state.data_ptr() + 8)), b"aligned"),
                # what the second round adds
                (dict(low_score=nan), b"low_score is NaN"), (dict(low_score=0.5), b"low_score must be below min_score"),
                (dict(low_score=0.75), b"low_score must be below min_score"), (dict(min_score=0.1), b"low_score must be below"),
                (dict(min_score=nan), b"low_score must be below"), (dict(low_iou=0.0), b"low_iou must be in (0, 1]"),
                (dict(low_iou=1.5), b"low_iou"), (dict(low_iou=-0.3), b"low_iou"), (dict(low_iou=nan), b"low_iou"),
                (dict(rescued=ctypes.c_void_p(tr.rescued.data_ptr() + 4)), b"rescued must be 8-byte aligned")]
    if motion:
        refusals += [(dict(alpha=0.0), b"alpha"), (dict(beta=1.5), b"beta"), (dict(age=1 << 24), b"max_age_us"),
                     (dict(box=None), b"track_box"), (dict(coast_id=None), b"coast_id")]
    entry = (tr.family + "_rescue").encode()
    for over, text in refusals:
        assert tr.call(s, **over) == bad, over
        said = tr.L.dagr_last_error()
        assert text in said and said.startswith(entry + b":"), (over, said)
    assert torch.equal(tr.state, before) and torch.equal(tr.untracked, untracked) and torch.equal(tr.rescued, rescued)
    assert all(torch.equal(tr.out[k].view(torch.uint8), outs[k].view(torch.uint8)) for k in outs)
    # rescued may be NULL, as untracked may: the step is the same
    _lib.check(getattr(tr.L, tr.family + "_reset")(_lib.ptr(tr.state), tr.nbytes, tr.B, tr.M, _lib.cur_stream(tr.dev)), "reset")
    for k in (0, 1):
        assert tr.call(case["steps"][k], rescued=None, untracked=None) == 0
    want = rc.run_definition(case)[0][1]
    assert rc.same(tr.out["ids"].cpu().numpy()[2, :2], want["ids"][2, :2]) and torch.equal(tr.rescued, rescued)
    _assert_same_slots(tr.slots(), want["slots"], "NULL counters")


# ------------------------------------------------------------------------------------------------ the stream's own state
def _events(k, lanes=B):
    """Step k's push: k = 0 fills the 20 ms window, every later step adds 1 ms of events."""
    lo, hi = (0, 10000) if k == 0 else (10000 + 1000 * (k - 1), 10000 + 1000 * k)
    return _push({b: _chunk(syn.edges_window, (1800 - 300 * b) if k == 0 else (170 - 20 * b), 400 + 3 * k + b, lo, hi)
                  for b in range(lanes)}, t_now=[hi] * lanes)


def _step(stream, s, **kw):
    return stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"], **kw)


@pytest.mark.parametrize("motion", [None, True], ids=["plain", "motion"])
def test_the_flicker_keeps_one_id_in_a_streams_own_tracker_state(motion):
    """EventStream(track=dict(min_score=0.5), rescue=True): the stream's tracker state, its entry and its counter, driven
    with the flicker's detections at the flicker's instants (written where the stream's state keeps t_ref): one id with
    hits 1 .. 7, bit for bit the definition, three rescued matches; reset() clears the counter."""
    case = next(c for c in rc.cases() if c["name"] == "the-flicker" + ("-with-motion" if motion else ""))
    model = _model(B)
    stream = EventStream(model, window_us=WINDOW_US, track=dict(min_score=0.5, max_age_us=1500), motion=motion, rescue=True)
    assert stream.rescue == dict(low_score=float(np.float32(0.1)), iou=float(np.float32(0.3)))
    assert not stream.rescued().any() and stream.rescued().dtype == np.int64
    st = stream.state
    with torch.no_grad():
        _step(stream, _events(0))                       # (the stream's state exists behind its first step)
    stream.reset()
    where = _lib.lib().dagr_stream_t_ref(_lib.ptr(st.state), B, st.cap)
    off = where - st.state.data_ptr()
    t_ref = st.state[off:off + 8 * B].view(torch.int64)
    d = TrackDefinition(B, stream.track, motion=motion, rescue=True)
    seen = []
    for k, s in enumerate(case["steps"]):               # lane 0 plays the flicker, lane 1 has no instant and no rows
        det = np.concatenate([s["det"], s["det"]], 0)
        nk, now = np.array([s["n_keep"][0], 0], np.int32), np.array([s["t_ref"][0], rc.NEVER], np.int64)
        t_ref.copy_(_dev(now))
        st.run_track(_dev(det), _dev(nk))
        want_ids, want_hits = d.step(det, nk, now)
        ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
        assert rc.same(ids[0, :1], want_ids[0, :1]) and rc.same(hits[0, :1], want_hits[0, :1]), k
        if motion:
            assert rc.same(stream.track_boxes.cpu().numpy()[0, :1], d.track_box[0, :1]), k
            assert rc.same(stream.track_vel.cpu().numpy()[0, :1], d.track_vel[0, :1]), k
        assert rc.same(stream.rescued(), d.rescued), k
        seen.append((int(ids[0, 0]), int(hits[0, 0])))
    assert seen == [(1, k) for k in range(1, 8)] and stream.rescued().tolist() == [3, 0]
    for got, want in zip(stream.tracks(), d.tracks()):
        assert got.tobytes() == want.tobytes()
    stream.reset()
    assert not stream.rescued().any() and all(len(t) == 0 for t in stream.tracks())


# ------------------------------------------------------------------------------------------------ the stream, end to end
_THRESHOLDS = {}


def _thresholds(model, key, **first):
    """The head's scores are not known in advance: (min_score, low_score) are the median and the lower decile of the scores
    of a plain stream's first step, so that about half of the rows are low and a tenth is under the band."""
    if key not in _THRESHOLDS:
        plain = EventStream(model, window_us=WINDOW_US)
        with torch.no_grad():
            det, nk = _step(plain, _events(0), **first)
        det, nk = det.cpu().numpy(), nk.cpu().numpy()
        scores = np.concatenate([det[b, :nk[b], 4] for b in range(B)])
        assert len(scores) >= 20, len(scores)
        cut, low = float(np.float32(np.median(scores))), float(np.float32(np.quantile(scores, 0.1)))
        assert low < cut, (low, cut)
        _THRESHOLDS[key] = (cut, low)
    return _THRESHOLDS[key]


def _compare(stream, d, det, nk, t_now, where):
    ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
    want_ids, want_hits = d.step(det, nk, t_now)
    for b in range(d.B):
        n = int(nk[b])
        assert rc.same(ids[b, :n], want_ids[b, :n]) and rc.same(hits[b, :n], want_hits[b, :n]), (where, b)
        if d.motion is not None:
            assert rc.same(stream.track_boxes.cpu().numpy()[b, :n], d.track_box[b, :n]), (where, b)
            assert rc.same(stream.track_vel.cpu().numpy()[b, :n], d.track_vel[b, :n]), (where, b)
    assert rc.same(stream.rescued(), d.rescued), where
    assert rc.same(stream.untracked(), d.untracked), where


@pytest.mark.parametrize("motion", [None, True], ids=["plain", "motion"])
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_rescue_stream_equals_the_definition_and_rescues(latency, motion):
    """B = 2, ten steps: track_ids, track_hits, with motion= track_boxes and track_vel, rescued() and untracked() equal a
    TrackDefinition(rescue=) fed with every step's own detections and t_now; some match IS rescued; nothing is captured
    again; reset() clears the counter; a stream without rescue= has none."""
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    cut, low = _thresholds(model, "events")
    track = dict(iou=0.3, max_age_us=2500, min_score=cut, max_tracks=64)
    stream = EventStream(model, window_us=WINDOW_US, track=track, motion=motion, rescue=dict(low_score=low))
    d = TrackDefinition(B, track, motion=motion, rescue=dict(low_score=low))
    assert stream.rescue == d.rescue and stream.rescue["iou"] == stream.track["iou"]
    graph, rows, low_rows = None, 0, 0
    with torch.no_grad():
        for rnd in range(2):
            for k in range(10):
                s = _events(k)
                det, nk = _step(stream, s)
                det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                _compare(stream, d, det, nk, s["t_now"], (rnd, k))
                sc = np.concatenate([det[b, :nk[b], 4] for b in range(B)])
                rows, low_rows = rows + len(sc), low_rows + int(np.sum((sc >= np.float32(low)) & ~(sc >= np.float32(cut))))
            print("round", rnd, "min_score", cut, "low_score", low, "rows", rows, "low rows", low_rows, d.events,
                  "rescued", d.rescued.tolist())
            assert d.events["rescued"] > 0 and d.events["matched"] > d.events["rescued"] and d.events["spawned"] > 0, d.events
            for got, want in zip(stream.tracks(), d.tracks()):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), rnd
            stream.check_status()
            if rnd == 0:
                graph = eng._wg
            elif latency:
                assert graph is not None and eng._wg is graph          # no re-capture
            stream.reset()
            assert not stream.rescued().any() and not stream.untracked().any() and all(len(t) == 0 for t in stream.tracks())
            d.reset()
        only = EventStream(model, window_us=WINDOW_US, track=track, motion=motion)
        assert only.rescue is None and only.state.rescue is None and only.state.lane_rescued is None
        _step(only, _events(0))
        with pytest.raises(RuntimeError, match="rescue="):
            only.rescued()
    eng.set_low_latency(True)


def test_rescue_behind_frame_steps_and_held_steps():
    """A --use_image model (resnet18, B = 2; tests/test_stream_hold_gpu.py's, warmed as that suite warms it): frame step, two
    held steps, frame step, held step, with motion=.  The image branch is not bit-reproducible, so nothing is compared with
    a second run: the tracker's outputs and rescued() equal a definition fed with every step's own det / n_keep / t_now, the
    bodies are counted, and the captured graphs are the objects they were."""
    from tests import test_stream_hold_gpu as hold
    model = hold._image_model()
    eng = hold._warm(model, True)
    graphs = (eng._wg, eng._hg)
    imgs = hold._images(7, 8)
    cut, low = _thresholds(model, "image", image=imgs[0])
    track = dict(iou=0.3, max_age_us=5000, min_score=cut, max_tracks=64)
    motion, rescue = dict(alpha=0.75, beta=0.5), dict(low_score=low, iou=0.25)
    stream = EventStream(model, window_us=WINDOW_US, track=track, motion=motion, rescue=rescue)
    d = TrackDefinition(hold.B, track, motion=motion, rescue=rescue)
    with torch.no_grad():
        for k, img in enumerate((imgs[0], None, None, imgs[1], None)):
            s = _events(k)
            det, nk = _step(stream, s, image=img)
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            _compare(stream, d, det, nk, s["t_now"], k)
            print("step", k, "frame" if img is not None else "held", "n_keep", nk.tolist(), d.events)
    assert (stream.frame_steps, stream.held_steps) == (2, 3)
    assert d.events["matched"] > 0 and d.events["spawned"] > 0, d.events
    for got, want in zip(stream.tracks(), d.tracks()):
        assert got.tobytes() == want.tobytes()
    stream.check_status()
    assert graphs[0] is not None and graphs[1] is not None and eng._wg is graphs[0] and eng._hg is graphs[1]
    model.engine().set_low_latency(True)


def test_event_stream_refuses_bad_rescue_options_by_name():
    model = _model(B)
    high = dict(min_score=0.5)
    for kw, name in ((dict(rescue=True), "rescue= needs track="), (dict(track=True, rescue=True), "raise track's min_score"),
                     (dict(track=high, rescue=dict(low_score=0.5)), "low_score"), (dict(track=high, rescue=dict(iou=0.0)), "rescue iou"),
                     (dict(track=high, rescue=dict(low_score=float("nan"))), "low_score"),
                     (dict(track=high, rescue=dict(score=0.1)), "score"), (dict(track=high, rescue="yes"), "rescue")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    stream = EventStream(model, window_us=WINDOW_US, track=high, rescue=dict(iou=0.5))
    assert stream.rescue == dict(low_score=float(np.float32(0.1)), iou=0.5)
    assert stream.state.track_state.numel() == 40 * B * 64 + 8 * B          # dagr_stream_track's state, as it is


# ------------------------------------------------------------------------------------------------ the calls
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_rescue_swaps_the_tracker_call_and_changes_no_other_stream(latency, monkeypatch):
    """Step for step a rescue stream issues the library calls of a stream without track= plus ONE _rescue entry, the step's
    last call, and neither base entry (it asks once where the state keeps t_ref, as a tracking stream does).  Streams
    without rescue= -- None or left out -- still end every step with their one dagr_stream_track / dagr_stream_track_cv,
    never call a _rescue entry and own no counter; a stream without track= issues none of the four."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    cut, low = _thresholds(model, "events")
    track = dict(iou=0.3, max_age_us=2500, min_score=cut, max_tracks=32)
    calls = _record_calls(monkeypatch)
    per_stream = {}
    # (the first stream warms the engine up -- eager steps, the capture -- so that the ones after it meet the same engine)
    for name, kw in (("warm-up", dict()), ("off", dict()), ("tracking", dict(track=track)),
                     ("tracking, rescue none", dict(track=track, rescue=None)), ("motion", dict(track=track, motion=True)),
                     ("rescue", dict(track=track, rescue=dict(low_score=low))),
                     ("motion and rescue", dict(track=track, motion=True, rescue=dict(low_score=low)))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps = []
        with torch.no_grad():
            for k in range(6):
                s = _events(k)
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
        if "rescue" not in kw or kw["rescue"] is None:
            assert stream.rescue is None and stream.state.rescue is None and stream.state.lane_rescued is None
            with pytest.raises(RuntimeError, match="rescue="):
                stream.rescued()
    off = per_stream["off"]
    four = ("dagr_stream_track", "dagr_stream_track_cv", "dagr_stream_track_rescue", "dagr_stream_track_cv_rescue")
    assert not any("track" in c or c == "dagr_stream_t_ref" for step in off for c in step)
    assert all([c for c in step if c in STEP_ENTRIES + four] == ["dagr_stream_stage"] for step in off), off
    assert per_stream["tracking, rescue none"] == per_stream["tracking"]
    for name, last in (("tracking", four[0]), ("motion", four[1]), ("rescue", four[2]), ("motion and rescue", four[3])):
        for k, (with_, without) in enumerate(zip(per_stream[name], off)):
            assert with_[-1] == last and not any(c in four for c in with_[:-1]), (name, k, with_)
            assert with_[:-1] == without + (["dagr_stream_t_ref"] if k == 0 else []), (name, k, with_, without)
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_prints_the_rescued_matches_and_leaves_the_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res"]
    track = ["--track", "--track_max_age_us", "2500", "--max_tracks", "32", "--track_min_score", "0.3"]
    paths = {}
    for name, extra in (("track", track), ("rescue", track + ["--track_low_score", "0.25", "--track_low_iou", "0.25"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    printed = capsys.readouterr().out
    with open(paths["track"], "rb") as f, open(paths["rescue"], "rb") as g:
        assert f.read() == g.read()                      # detections_<sequence>.npy is byte for byte what it was
    assert printed.count("rescued by the second round") == 1
    said = re.search(r"; (\d+) low-score detections rescued by the second round", printed)
    trk = np.load(os.path.join(os.path.dirname(str(paths["rescue"])), "tracks_res.npy"))
    low = (trk["class_confidence"] >= np.float32(0.25)) & ~(trk["class_confidence"] >= np.float32(0.3))
    assert said and int(said.group(1)) == int((trk["track_id"][low] != 0).sum()), printed
    assert np.all(trk["hits"][low & (trk["track_id"] != 0)] >= 2)           # a low row continues a track, it never starts one
    assert np.all(trk["track_id"][~(trk["class_confidence"] >= np.float32(0.25))] == 0)
