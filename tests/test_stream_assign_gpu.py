"""The stream tracker's optimal assignment on the GPU: dagr_stream_track_optimal through the binding against the numpy
definition (dagr_amd/streaming.py: TrackDefinition(assign="optimal")) bit for bit after every step, under all four flag
combinations: the hand cases of tests/stream_assign_cases.py, the crowded scene, the seeded walks at 8, 64 and 130 slots, more
rows than slots, the 256-row cut; against the four greedy entries on a twin state where nothing is contested; its refusals,
which launch nothing; EventStream(track=, assign="optimal") against a definition fed with every step's own detections, in
latency and in throughput mode; the library calls of streams with and without it; the scorer and IDF1 behind it; and
scripts/run_stream.py --track_assign."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import (EventStream, IdentityDefinition, ScoreDefinition, TrackDefinition, _motion_options,
                                _rescue_options, _track_options)
from tests import stream_assign_cases as ac
from tests import stream_rescue_cases as rc
from tests.test_stream_motion_gpu import _Tracker as _MotionTracker
from tests.test_stream_rescue_gpu import _Tracker as _RescueTracker
from tests.test_stream_rescue_gpu import _assert_same_slots, _events, _step, _thresholds
from tests.test_stream_score_gpu import _labels
from tests.test_stream_track_gpu import STEP_ENTRIES, _record_calls
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_streaming_gpu import _dev, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
WINDOW_US = 20000
SENTINEL = -7
MOTION_BIT, RESCUE_BIT = _lib.DEFINES["DAGR_TRACK_OPTIMAL_MOTION"], _lib.DEFINES["DAGR_TRACK_OPTIMAL_RESCUE"]
ENTRY = "dagr_stream_track_optimal"
MOTION_OUT = ("box", "vel", "coast_id", "coast_box", "coast_label", "coast_age", "n_coast")


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Tracker:
    """dagr_stream_track_optimal on a state of its own, made and emptied by the greedy family's _bytes and _reset; the flags
    follow the case's motion / rescue.  The state starts out as garbage in front of its reset, the workspace stays garbage,
    every output starts as the sentinel -7.  Without a flag its arguments are NULL / 0."""

    def __init__(self, B_, A, track, motion, rescue):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.o = B_, A, _track_options(track, "test")
        self.m = _motion_options(motion, self.o, "test")
        self.r = _rescue_options(rescue, self.o, "test")
        self.M = M = self.o["max_tracks"]
        self.flags = (MOTION_BIT if self.m is not None else 0) | (RESCUE_BIT if self.r is not None else 0)
        self.family = "dagr_stream_track" if self.m is None else "dagr_stream_track_cv"
        self.nbytes = getattr(self.L, self.family + "_bytes")(B_, M)
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(getattr(self.L, self.family + "_reset")(_lib.ptr(self.state), self.nbytes, B_, M, _lib.cur_stream(self.dev)),
                   self.family + "_reset")
        self.ws_bytes = self.L.dagr_stream_track_optimal_bytes(B_, M)
        assert self.ws_bytes == 2 * 4 * B_ * S.DAGR_TRACK_MAX_DETS * M             # w and its transposed copy, per lane
        self.ws = torch.full((self.ws_bytes,), 0x5a, dtype=torch.uint8, device=self.dev)
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
                 min_score=self.o["min_score"], alpha=0.0, beta=0.0, det=P(det), n_keep=P(n_keep), A=self.A, t_ref=P(t_ref),
                 untracked=P(self.untracked), low_score=0.0, low_iou=0.0, rescued=None, flags=self.flags, ws=P(self.ws),
                 ws_bytes=self.ws_bytes, **{k: None for k in MOTION_OUT})
        a.update({k: P(v) for k, v in self.out.items()})
        if self.m is not None:
            a.update(alpha=self.m["alpha"], beta=self.m["beta"])
        if self.r is not None:
            a.update(low_score=self.r["low_score"], low_iou=self.r["iou"], rescued=P(self.rescued))
        a.update(over)
        rc_ = self.L.dagr_stream_track_optimal(a["tracks"], a["bytes"], a["B"], a["M"], a["iou"], a["age"], a["min_score"],
                                               a["alpha"], a["beta"], a["det"], a["n_keep"], a["A"], a["t_ref"], a["ids"],
                                               a["hits"], *[a[k] for k in MOTION_OUT], a["untracked"], a["low_score"],
                                               a["low_iou"], a["rescued"], a["flags"], a["ws"], a["ws_bytes"],
                                               _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc_

    slots = _RescueTracker.slots


def _assert_step(tr, want, s, where):
    """One step's outputs against the definition's: the rows below n_keep and the first n_coast coast entries are the
    definition's, everything behind them is still the sentinel; untracked, rescued, the slots, next_id."""
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
    if tr.r is not None:
        assert rc.same(tr.rescued.cpu().numpy(), want["rescued"]), (where, "rescued")
    else:
        assert not tr.rescued.any(), (where, "rescued without the flag")
    _assert_same_slots(tr.slots(), want["slots"], where)
    return out


def _run_case(case):
    tr = _Tracker(case["B"], case["A"], case["track"], case["motion"], case["rescue"])
    steps, d = ac.run_definition(case)
    for k, (s, want) in enumerate(zip(case["steps"], steps)):
        tr.refill()
        _lib.check(tr.call(s), ENTRY)
        out = _assert_step(tr, want, s, (case["name"], k))
        if case["expect"] is not None:
            ac.check_expectation(case, k, out["ids"], out["hits"], tr.untracked.cpu().numpy(), tr.rescued.cpu().numpy())
    return tr, d


@pytest.mark.parametrize("name", [c["name"] for c in ac.cases()])
def test_the_entry_equals_the_definition_after_every_step(name):
    """Bit for bit after every step: ids, hits, untracked, rescued, every slot field where a track lives, next_id, with motion
    the filtered boxes, the velocities and the coast lists; the sentinel behind n_keep and behind n_coast; the case's
    written-out expectation.  Among the cases: the two-box example, the tie, more rows than slots (max_tracks = 4, 9 rows:
    the transposed matrix) and 300 rows against 256 slots (the cut, `untracked`, a 256 x 256 round with conflicts)."""
    case = next(c for c in ac.cases() if c["name"] == name)
    tr, d = _run_case(case)
    if name == "more-rows-than-slots":
        assert d.events["conflicts"] == 2 and int(tr.untracked[0]) == 10, d.events
    if name == "the-256-row-cut":
        assert d.events["conflicts"] == 1 and int(tr.untracked[0]) == 28 and d.events["matched"] == 256, d.events


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
def test_the_crowded_scene_equals_the_definition_at_every_step(motion, rescue):
    """40 steps, B = 2, 24 places in 160 x 120: dozens of rounds in which the pairing is not greedy's."""
    _, d = _run_case(ac.crowd(motion, rescue))
    assert d.events["reassigned"] >= 20 and d.events["conflicts"] > d.events["reassigned"], d.events


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
@pytest.mark.parametrize("max_tracks", [8, 64, 130])
def test_the_walks_equal_the_definition_at_every_step(max_tracks, motion, rescue):
    """B = 3, A = 64: 8 slots overflow (one slot register), 64 fill one, 130 fill two and a part of the third."""
    _, d = _run_case(ac.walk(max_tracks, motion, rescue))
    assert d.events["conflicts"] > 0 and d.events["retired"] > 0 and d.events["spawned"] > 0, d.events


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
def test_where_nothing_is_contested_the_entry_leaves_what_the_greedy_entry_leaves(motion, rescue):
    """The well-separated scene through the new entry and through dagr_stream_track / _cv / _rescue / _cv_rescue on a twin
    state, side by side: after every step the outputs, the counters and every byte of the state are equal."""
    case = ac.separated(motion, rescue)
    assert ac.run_definition(case)[1].events["conflicts"] == 0
    new = _Tracker(case["B"], case["A"], case["track"], case["motion"], case["rescue"])
    if rescue:
        old = _RescueTracker(case["B"], case["A"], case["track"], case["motion"], case["rescue"])
        old_out = old.out
    elif motion:
        old = _MotionTracker(case["B"], case["A"], case["track"], case["motion"])
        old_out = old.out
    else:
        old = _PlainTracker(case["B"], case["A"], case["track"])
        old_out = dict(ids=old.ids, hits=old.hits)
    assert sorted(old_out) == sorted(new.out)
    for k, s in enumerate(case["steps"]):
        new.refill()
        for t in old_out.values():
            t.fill_(SENTINEL)
        _lib.check(new.call(s), ENTRY)
        _lib.check(old.call(s), "the greedy entry")
        for name_, t in old_out.items():
            assert torch.equal(new.out[name_].view(torch.uint8), t.view(torch.uint8)), (case["name"], k, name_)
        assert torch.equal(new.untracked, old.untracked) and torch.equal(new.state, old.state), (case["name"], k)
        if rescue:
            assert torch.equal(new.rescued, old.rescued), (case["name"], k)
    assert new.slots()[0].any() and new.untracked.sum() >= 0


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
def test_argument_errors_launch_nothing(motion, rescue):
    case = ac.crowd(motion, rescue, steps=3)
    tr, _ = _run_case(case)
    assert tr.slots()[0].any()
    before, s = tr.state.clone(), case["steps"][-1]
    tr.ws.fill_(0x5a)
    outs, untracked, rescued = {k: v.clone() for k, v in tr.out.items()}, tr.untracked.clone(), tr.rescued.clone()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    nan = float("nan")
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)                                           # noqa: E731
    refusals = [(dict(ws=None), b"workspace is NULL"), (dict(ws_bytes=tr.ws_bytes - 1), b"workspace smaller than"),
                (dict(ws_bytes=0), b"workspace smaller than"), (dict(ws=odd(tr.ws, 8)), b"workspace must be 16-byte aligned"),
                (dict(flags=4 | tr.flags), b"unknown bits in flags"), (dict(flags=-1), b"unknown bits in flags"),
                # whatever the base entries refuse
                (dict(tracks=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(t_ref=None), b"NULL"), (dict(ids=None), b"NULL"),
                (dict(det=None), b"NULL"), (dict(bytes=tr.nbytes - 1), b"smaller"), (dict(M=0), b"max_tracks"),
                (dict(M=257), b"max_tracks"), (dict(iou=0.0), b"iou"), (dict(iou=nan), b"iou"), (dict(age=-1), b"max_age_us"),
                (dict(B=0), b"out of range"), (dict(A=-1), b"A out of range"), (dict(tracks=odd(tr.state, 8)), b"aligned")]
    if rescue:
        refusals += [(dict(low_score=nan), b"low_score is NaN"), (dict(low_score=0.5), b"low_score must be below min_score"),
                     (dict(min_score=nan), b"low_score must be below"), (dict(low_iou=0.0), b"low_iou must be in (0, 1]"),
                     (dict(low_iou=nan), b"low_iou"), (dict(rescued=odd(tr.rescued, 4)), b"rescued must be 8-byte aligned")]
    if motion:
        refusals += [(dict(alpha=0.0), b"alpha"), (dict(beta=1.5), b"beta"), (dict(age=1 << 24), b"max_age_us"),
                     (dict(box=None), b"track_box"), (dict(vel=None), b"track_vel"), (dict(coast_id=None), b"coast_id"),
                     (dict(n_coast=None), b"n_coast are NULL together"), (dict(box=odd(tr.out["box"], 8)), b"16-byte aligned")]
    if not motion:      # the motion layout is larger: the plain state is too small for the flag
        refusals += [(dict(flags=tr.flags | MOTION_BIT, alpha=1.0, beta=0.5), b"track_box")]
    for over, text in refusals:
        assert tr.call(s, **over) == bad, over
        said = tr.L.dagr_last_error()
        assert text in said and said.startswith(ENTRY.encode() + b":"), (over, said)
    assert torch.equal(tr.state, before) and torch.equal(tr.untracked, untracked) and torch.equal(tr.rescued, rescued)
    assert all(torch.equal(tr.out[k].view(torch.uint8), outs[k].view(torch.uint8)) for k in outs)
    assert (tr.ws == 0x5a).all()
    L = tr.L
    assert L.dagr_stream_track_optimal_bytes(0, 4) == 0 and L.dagr_stream_track_optimal_bytes(65536, 4) == 0
    assert L.dagr_stream_track_optimal_bytes(1, 0) == 0 and L.dagr_stream_track_optimal_bytes(1, 257) == 0
    assert L.dagr_stream_track_optimal_bytes(1, 256) == 2 * 4 * 256 * 256


def test_without_a_flag_its_arguments_are_not_looked_at():
    """flags = 0 with every motion and rescue argument given -- garbage gains, a low_score above min_score, real arrays --
    is the plain step: the arrays stay the sentinel and the counter stays 0."""
    case = ac.crowd(False, False, steps=5)
    steps, _ = ac.run_definition(case)
    tr = _Tracker(case["B"], case["A"], case["track"], None, None)
    full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=tr.dev)           # noqa: E731
    extra = dict(box=full((tr.B, tr.A, 4), torch.float32), vel=full((tr.B, tr.A, 4), torch.float32),
                 coast_id=full((tr.B, tr.M), torch.int64), n_coast=full((tr.B,), torch.int32))
    for k, (s, want) in enumerate(zip(case["steps"], steps)):
        tr.refill()
        _lib.check(tr.call(s, alpha=float("nan"), beta=7.0, low_score=2.0, low_iou=-1.0, rescued=_lib.ptr(tr.rescued),
                           **{name: _lib.ptr(t) for name, t in extra.items()}), ENTRY)
        _assert_step(tr, want, s, ("flags 0", k))
    assert all((t == SENTINEL).all() for t in extra.values())


# ------------------------------------------------------------------------------------------------ the stream, end to end
def _compare(stream, d, det, nk, t_now, where):
    ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
    want_ids, want_hits = d.step(det, nk, t_now)
    for b in range(d.B):
        n = int(nk[b])
        assert rc.same(ids[b, :n], want_ids[b, :n]) and rc.same(hits[b, :n], want_hits[b, :n]), (where, b)
        if d.motion is not None:
            assert rc.same(stream.track_boxes.cpu().numpy()[b, :n], d.track_box[b, :n]), (where, b)
            assert rc.same(stream.track_vel.cpu().numpy()[b, :n], d.track_vel[b, :n]), (where, b)
    if d.rescue is not None:
        assert rc.same(stream.rescued(), d.rescued), where
    assert rc.same(stream.untracked(), d.untracked), where


@pytest.mark.parametrize("motion,rescue", ac.COMBOS)
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_an_assign_stream_equals_the_definition(latency, motion, rescue):
    """B = 2, ten steps: track_ids, track_hits, with motion= track_boxes and track_vel, untracked() and with rescue=
    rescued() equal a TrackDefinition(assign="optimal") fed with every step's own detections and t_now; tracks() is the
    definition's; nothing is captured again; the stream owns the workspace the header sizes."""
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    cut, low = _thresholds(model, "events")
    track = dict(iou=0.3, max_age_us=2500, min_score=cut, max_tracks=64)
    kw = dict(motion=True if motion else None, rescue=dict(low_score=low) if rescue else None, assign="optimal")
    stream = EventStream(model, window_us=WINDOW_US, track=track, **kw)
    d = TrackDefinition(B, track, **kw)
    assert stream.assign == "optimal" and stream.state.assign == "optimal"
    assert stream.state.assign_ws.numel() == _lib.lib().dagr_stream_track_optimal_bytes(B, 64)
    assert stream.state.track_state.numel() == (56 if motion else 40) * B * 64 + 8 * B      # the greedy family's state, as it is
    graph = None
    with torch.no_grad():
        for rnd in range(2):
            for k in range(10):
                s = _events(k)
                det, nk = _step(stream, s)
                det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                _compare(stream, d, det, nk, s["t_now"], (rnd, k))
            print("round", rnd, d.events)
            assert d.events["matched"] > 0 and d.events["spawned"] > 0, d.events
            for got, want in zip(stream.tracks(), d.tracks()):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), rnd
            stream.check_status()
            if rnd == 0:
                graph = eng._wg
            elif latency:
                assert graph is not None and eng._wg is graph          # no re-capture
            stream.reset()
            assert not stream.untracked().any() and all(len(t) == 0 for t in stream.tracks())
            d.reset()
        for off in (None, "greedy"):
            only = EventStream(model, window_us=WINDOW_US, track=track, assign=off)
            assert only.assign is None and only.state.assign is None and only.state.assign_ws is None
    eng.set_low_latency(True)


def test_event_stream_refuses_bad_assign_options_by_name():
    model = _model(B)
    for kw, name in ((dict(assign="optimal"), "assign= needs track="), (dict(assign="greedy"), "assign= needs track="),
                     (dict(track=True, assign="hungarian"), "assign = 'hungarian' must be None or 'greedy'"),
                     (dict(track=True, assign=True), "assign = True")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)


# ------------------------------------------------------------------------------------------------ the calls
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_assign_swaps_the_tracker_call_and_changes_no_other_stream(latency, monkeypatch):
    """Step for step a stream with assign="optimal" issues the library calls of a stream without track= plus ONE
    dagr_stream_track_optimal, the step's last call, and none of the four greedy entries.  Streams without it -- None,
    "greedy" or left out -- end every step with the greedy entry they ended it with before and never call the new one."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    cut, low = _thresholds(model, "events")
    track = dict(iou=0.3, max_age_us=2500, min_score=cut, max_tracks=32)
    rescue = dict(low_score=low)
    calls = _record_calls(monkeypatch)
    per_stream = {}
    four = ("dagr_stream_track", "dagr_stream_track_cv", "dagr_stream_track_rescue", "dagr_stream_track_cv_rescue")
    greedy = (("tracking", dict(track=track)), ("motion", dict(track=track, motion=True)),
              ("rescue", dict(track=track, rescue=rescue)), ("motion and rescue", dict(track=track, motion=True, rescue=rescue)))
    # (the first stream warms the engine up -- eager steps, the capture -- so that the ones after it meet the same engine)
    for name, kw in ((("warm-up", dict()), ("off", dict()), ("tracking, assign none", dict(track=track, assign=None)),
                      ("tracking, assign greedy", dict(track=track, assign="greedy"))) + greedy +
                     tuple((n + ", optimal", dict(k, assign="optimal")) for n, k in greedy)):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps = []
        with torch.no_grad():
            for k in range(4):
                s = _events(k)
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
    off = per_stream["off"]
    assert not any("track" in c or c == "dagr_stream_t_ref" for step in off for c in step)
    assert all([c for c in step if c in STEP_ENTRIES + four + (ENTRY,)] == ["dagr_stream_stage"] for step in off), off
    assert per_stream["tracking, assign none"] == per_stream["tracking"] == per_stream["tracking, assign greedy"]
    for (name, _), last in zip(greedy, four):
        for k, (with_, without) in enumerate(zip(per_stream[name], off)):             # what they were
            assert with_[-1] == last and not any(c in four + (ENTRY,) for c in with_[:-1]), (name, k, with_)
            assert with_[:-1] == without + (["dagr_stream_t_ref"] if k == 0 else []), (name, k, with_, without)
        for k, (with_, without) in enumerate(zip(per_stream[name + ", optimal"], off)):
            assert with_[-1] == ENTRY and not any(c in four + (ENTRY,) for c in with_[:-1]), (name, k, with_)
            assert with_[:-1] == without + (["dagr_stream_t_ref"] if k == 0 else []), (name, k, with_, without)
    model.engine().set_low_latency(True)


def test_the_scorer_and_idf1_run_unchanged_behind_it(monkeypatch):
    """score=, identity= on a stream with assign="optimal": score_step is dagr_stream_score then dagr_stream_identity, and
    the counters and IDF1's integers equal the definitions fed with the stream's own detections and ids."""
    model = _model(B)
    track = dict(iou=0.3, max_age_us=2500, max_tracks=64)
    score, identity = dict(iou=0.5, max_objects=16), dict(max_tracks=24)
    stream = EventStream(model, window_us=WINDOW_US, track=track, assign="optimal", score=score, identity=identity)
    sd, d = ScoreDefinition(B, score), IdentityDefinition(B, identity, score)
    calls = _record_calls(monkeypatch)
    with torch.no_grad():
        for k in range(9):
            s = _events(k)
            det, nk = (t.clone().cpu().numpy() for t in _step(stream, s))
            assert calls[-1] == ENTRY
            if k % 3:
                continue
            ids = stream.track_ids.cpu().numpy()
            lab = _labels(det, nk, k)
            del calls[:]
            stream.score_step(*lab)
            assert list(calls) == ["dagr_stream_score", "dagr_stream_identity"]
            match, _ = sd.step(det, nk, ids, *lab)
            d.step(det, nk, ids, *lab, match, sd.id)
    got = stream.track_score()
    assert all(np.array_equal(got[name], sd.counters[name]) for name in S.SCORE_COUNTERS)
    result, want = stream.identity(), d.solve()
    for name in S.IDENTITY_RESULT:
        assert np.array_equal(result[name], want[name]), name
    assert result["idtp"].sum() > 0


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_names_the_rule_and_leaves_the_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res"]
    track = ["--track", "--track_max_age_us", "2500", "--max_tracks", "32"]
    paths = {}
    for name, extra in (("track", track), ("optimal", track + ["--track_assign", "optimal"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    printed = capsys.readouterr().out
    with open(paths["track"], "rb") as f, open(paths["optimal"], "rb") as g:
        assert f.read() == g.read()                      # detections_<sequence>.npy is byte for byte what it was
    assert printed.count("distinct track ids") == 2 and printed.count("every round matched by an optimal assignment") == 1
    trk = np.load(os.path.join(os.path.dirname(str(paths["optimal"])), "tracks_res.npy"))
    assert (trk["track_id"] != 0).any()
    for argv, said in ((base + ["--track_assign", "optimal"], "--track_assign needs --track"),
                       (base + track + ["--track_assign", "best"], "assign = 'best'")):
        with pytest.raises(SystemExit, match=said):
            R.main(argv + ["--output_directory", str(tmp_path / "refused")], model_factory=lambda a_, ds, dev: (a_, model),
                   source=R.SyntheticStream(C.flags("", base, extra=R.stream_options)))
