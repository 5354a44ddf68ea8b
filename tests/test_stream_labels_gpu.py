"""The event stream's label store on the GPU: dagr_stream_labels_push / dagr_stream_labels_at through the binding against
the numpy definition (dagr_amd/streaming.py: LabelDefinition), bit for bit after every call of every case of
tests/stream_labels_cases.py; their refusals; EventStream(labels=) scored at every step against ScoreDefinition fed with
LabelDefinition.at(t_ref), in latency and in throughput mode; the library calls of streams with and without the store; and
scripts/run_stream.py --track_score_every_step."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, LabelDefinition, ScoreDefinition
from tests import stream_labels_cases as lc
from tests.test_stream_rescue_gpu import _events, _step
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import _dev, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
WINDOW_US = 20000
SENTINEL = lc.SENTINEL


# ------------------------------------------------------------------------------------------------ the kernels, case by case
def _sections(B_, K, R):
    """Where the arrays of the state lie, by the layout include/dagr_hip.h documents: ``({name: (offset, dtype, shape)},
    bytes)``."""
    out, at = {}, 0
    for name, dtype, shape in (("lane", np.int64, (B_, 8)), ("t", np.int64, (B_, K)), ("n", np.int32, (B_, K)),
                               ("xywh", np.float64, (B_, K, R, 4)), ("label", np.int32, (B_, K, R)), ("id", np.int64, (B_, K, R))):
        out[name] = (at, dtype, shape)
        at += -(-int(np.prod(shape)) * np.dtype(dtype).itemsize // 16) * 16
    return out, at


class _Store:
    """The two entries on a state of their own; the state starts out as garbage in front of its reset, the outputs as the
    sentinel -7 (they are never refilled: what a call leaves alone stays)."""

    def __init__(self, B_, labels):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.o = B_, S._label_options(labels, "test")
        self.K, self.R = self.o["max_keyframes"], self.o["max_rows"]
        self.nbytes = self.L.dagr_stream_labels_bytes(B_, self.K, self.R)
        assert self.nbytes == _sections(B_, self.K, self.R)[1]
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_labels_reset(_lib.ptr(self.state), self.nbytes, B_, self.K, self.R,
                                                   _lib.cur_stream(self.dev)), "dagr_stream_labels_reset")
        self.out = tuple(_dev(v) for v in lc.outputs(B_, self.R))

    def _sizes(self, over):
        a = dict(state=_lib.ptr(self.state), bytes=self.nbytes, B=self.B, K=self.K, R=self.R)
        a.update({k: v for k, v in over.items() if k in a})
        return [a[k] for k in ("state", "bytes", "B", "K", "R")]

    def push(self, arg, **over):
        t = {k: _dev(np.ascontiguousarray(arg[k])) for k in ("t", "n", "xywh", "label", "id")}
        a = dict(F=int(arg["t"].shape[1]), **{k: _lib.ptr(v) for k, v in t.items()})
        a.update({k: v for k, v in over.items() if k in a})
        rc = self.L.dagr_stream_labels_push(*self._sizes(over), a["F"], a["t"], a["n"], a["xywh"], a["label"], a["id"],
                                            _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def at(self, instants, **over):
        t = _dev(np.asarray(instants, np.int64))    # the instants are handed in as a device array
        nan = float("nan")
        a = dict(t_ref=_lib.ptr(t), max_gap_us=self.o["max_gap_us"] or 0,
                 min_height=nan if self.o["min_height"] is None else self.o["min_height"],
                 min_diag=nan if self.o["min_diag"] is None else self.o["min_diag"],
                 **{k: _lib.ptr(v) for k, v in zip(("gt_box", "gt_label", "gt_id", "n_gt"), self.out)})
        a.update({k: v for k, v in over.items() if k in a})
        rc = self.L.dagr_stream_labels_at(*self._sizes(over), a["t_ref"], a["max_gap_us"], a["min_height"], a["min_diag"],
                                          a["gt_box"], a["gt_label"], a["gt_id"], a["n_gt"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()
        return rc

    def words(self):
        return self.state[:64 * self.B].view(torch.int64).cpu().numpy().reshape(self.B, 8)

    def section(self, name):
        at, dtype, shape = _sections(self.B, self.K, self.R)[0][name]
        return self.state[at:at + int(np.prod(shape)) * np.dtype(dtype).itemsize].cpu().numpy().view(dtype).reshape(shape)


def _assert_equal(store, d, out, where):
    """Every output array, whole and bit for bit (the sentinel survives wherever nothing was written), and every word."""
    for name, got, want in zip(("gt_box", "gt_label", "gt_id", "n_gt"), store.out, out):
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (where, name, got, want)
    words = store.words()
    assert np.array_equal(words, d.words()), (where, words, d.words())
    for b in range(store.B):                        # the resident instants and row counts, through the documented layout
        slots = [(int(words[b, 1]) + i) % store.K for i in range(int(words[b, 0]))]
        assert store.section("t")[b, slots].tolist() == [f[0] for f in d.frames[b]], (where, b)
        assert store.section("n")[b, slots].tolist() == [len(f[3]) for f in d.frames[b]], (where, b)


def _run_case(case):
    store = _Store(case["B"], case["labels"])

    def each(k, op, arg, d, out):
        _lib.check(store.push(arg) if op == "push" else store.at(arg), "dagr_stream_labels_" + op)
        _assert_equal(store, d, out, (case["name"], k, op))
    d = lc.run_definition(case, each)
    return store, d


@pytest.mark.parametrize("name", [c["name"] for c in lc.cases()])
def test_the_entries_equal_the_definition_after_every_call(name):
    """Bit for bit after every push and every at: the four output arrays (whole: the sentinel survives behind n_gt and in a
    lane without labels), the lanes' words with every counter, the resident instants.  Among the cases: three lanes of
    which one is empty, instants near 2**33 with odd intervals, identities above 2**32, keyframes of 0, 1, 63, 64, 65 and
    256 rows against max_rows of 64 and 256, a ring of 4 wrapped by 6 pushes, one and three keyframes a push call, the
    small-box filter exactly at a row's own fp64 diagonal, and every written-out case of the CPU suite."""
    case = next(c for c in lc.cases() if c["name"] == name)
    store, d = _run_case(case)
    if "kept" in case:
        assert store.out[3].cpu().tolist() == [case["kept"]]


def test_argument_errors_launch_nothing(monkeypatch):
    case = next(c for c in lc.cases() if c["name"].startswith("a-lane-with-nothing"))
    store, _ = _run_case(case)
    arg, t_ref = case["ops"][0][1], case["ops"][1][1]
    before, outs = store.state.clone(), [v.clone() for v in store.out]
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    calls = _record_calls(monkeypatch)
    L = store.L
    for over, text in [(dict(state=None), b"NULL"), (dict(t=None), b"NULL"), (dict(n=None), b"NULL"), (dict(xywh=None), b"NULL"),
                       (dict(label=None), b"NULL"), (dict(id=None), b"NULL"), (dict(bytes=store.nbytes - 1), b"smaller"),
                       (dict(B=0), b"out of range"), (dict(B=65536), b"out of range"), (dict(K=0), b"out of range"),
                       (dict(K=65536), b"out of range"), (dict(R=0), b"out of range"), (dict(R=257), b"out of range"),
                       (dict(F=0), b"F out of range"), (dict(F=65536), b"F out of range"), (dict(state=odd(store.state, 8)), b"aligned"),
                       (dict(xywh=odd(store.state, 8)), b"aligned"), (dict(t=odd(store.state, 4)), b"aligned"),
                       (dict(n=odd(store.state, 2)), b"aligned")]:
        assert store.push(arg, **over) == bad, over
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_labels_push:"), (over, said)
    for over, text in [(dict(state=None), b"NULL"), (dict(t_ref=None), b"NULL"), (dict(gt_box=None), b"NULL"),
                       (dict(gt_label=None), b"NULL"), (dict(gt_id=None), b"NULL"), (dict(n_gt=None), b"NULL"),
                       (dict(bytes=store.nbytes - 1), b"smaller"), (dict(B=0), b"out of range"), (dict(K=65536), b"out of range"),
                       (dict(R=257), b"out of range"), (dict(max_gap_us=-1), b"max_gap_us"), (dict(state=odd(store.state, 8)), b"aligned"),
                       (dict(gt_box=odd(store.out[0], 8)), b"aligned"), (dict(gt_id=odd(store.out[2], 4)), b"aligned"),
                       (dict(n_gt=odd(store.out[3], 2)), b"aligned")]:
        assert store.at(t_ref, **over) == bad, over
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_labels_at:"), (over, said)
    for sizes in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 65536, 4), (1, 4, 0), (1, 4, 257)):
        assert L.dagr_stream_labels_bytes(*sizes) == 0, sizes
    assert L.dagr_stream_labels_bytes(65535, 1, 1) > 0 and L.dagr_stream_labels_bytes(1, 65535, 256) == _sections(1, 65535, 256)[1]
    assert L.dagr_stream_labels_reset(_lib.ptr(store.state), store.nbytes - 1, store.B, store.K, store.R,
                                      _lib.cur_stream(store.dev)) == bad
    assert L.dagr_stream_labels_reset(None, store.nbytes, store.B, store.K, store.R, _lib.cur_stream(store.dev)) == bad
    torch.cuda.synchronize()
    assert torch.equal(store.state, before) and all(torch.equal(a, b) for a, b in zip(store.out, outs))
    # every refusal came from the entry that was asked, and none of them reached another entry of the library
    assert set(calls) <= {"dagr_stream_labels_push", "dagr_stream_labels_at", "dagr_stream_labels_bytes", "dagr_stream_labels_reset",
                          "dagr_last_error"}
    assert calls.count("dagr_stream_labels_push") == 19 and calls.count("dagr_stream_labels_at") == 15


# ------------------------------------------------------------------------------------------------ the stream, end to end
TRACK = dict(iou=0.3, max_age_us=2500, min_score=0.0, max_tracks=64)
STEPS, EVERY = 40, 10
LABELS = dict(max_keyframes=4, max_rows=16)
_KEYFRAMES = {}


_CLOCK = []


def _t_step(k):
    """_events(k)'s t_now: the stream's clock starts where the sibling suite's pushes start, and a step is 1000 us."""
    if not _CLOCK:
        _CLOCK.append(int(np.asarray(_events(0)["t_now"]).reshape(-1)[0]) - 10000)
        assert int(np.asarray(_events(3)["t_now"]).reshape(-1)[0]) == _CLOCK[0] + 13000
    return _CLOCK[0] + 10000 + 1000 * k


def _keyframes():
    """Keyframes made of a tracking stream's own detections at every 10th step: per lane the first rows as x y w h under
    identities that follow the row index, so that between two keyframes an identity moves from one detection to another
    and the scorer has matches, misses and switches to count.  Lane 1 has no keyframe at step 30."""
    if not _KEYFRAMES:
        model = _model(B)
        model.engine().set_low_latency(True)
        stream = EventStream(model, window_us=WINDOW_US, track=TRACK)
        with torch.no_grad():
            for k in range(STEPS):
                det, nk = _step(stream, _events(k))
                if k % EVERY == 0 and k:
                    det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                    frame = []
                    for b in range(B):
                        n = min(int(nk[b]), 12)
                        box = det[b, :n, :4].astype(np.float64)
                        xywh = np.concatenate([box[:, :2] + 0.25, box[:, 2:] - box[:, :2]], axis=1)
                        ids = 100 * b + 1 + np.arange(n, dtype=np.int64)
                        if n:
                            ids[-1] = 0
                        frame.append((xywh, det[b, :n, 5].astype(np.int32), ids))
                    _KEYFRAMES[k] = frame
    return _KEYFRAMES


def _push_keyframe(stream, d, k, frame, device):
    lanes = [0, 1] if k < 30 else [0]
    rows = max(len(frame[b][2]) for b in lanes)
    t = np.full((len(lanes),), _t_step(k), np.int64)
    n = np.array([len(frame[b][2]) for b in lanes], np.int32)
    xywh, label, ids = np.zeros((len(lanes), rows, 4)), np.zeros((len(lanes), rows), np.int32), np.zeros((len(lanes), rows), np.int64)
    for i, b in enumerate(lanes):
        xywh[i, :n[i]], label[i, :n[i]], ids[i, :n[i]] = frame[b]
        d.push(b, t[i], *frame[b])
    args = (t, xywh, label, ids)
    stream.push_labels(*((_dev(v) for v in args) if device else args), n=_dev(n) if device else n,
                       lanes=None if len(lanes) == B else lanes)


@pytest.mark.parametrize("metrics", [False, True], ids=["score", "identity-hota"])
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_stream_scored_at_every_step_equals_the_definitions(latency, metrics):
    """B = 2, forty steps, keyframes at every 10th, pushed one ahead of the steps that need them: after every score_step()
    the scorer's counters and tables equal a ScoreDefinition fed with LabelDefinition.at(t_ref) and the step's own
    detections and track ids, integer for integer; the steps before the first keyframe (and behind lane 1's last) leave
    the scorer's state untouched; with identity= and hota= the final identity() / hota() integers equal the definitions'."""
    frames = _keyframes()
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    score = dict(iou=0.5, max_objects=32)
    more = dict(identity=dict(max_tracks=64), hota=dict(max_instants=64)) if metrics else {}
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, score=score, labels=LABELS, **more)
    assert stream.labels == dict(LABELS, max_gap_us=None, min_height=None, min_diag=None)
    assert stream.state.labels_state.numel() == _lib.lib().dagr_stream_labels_bytes(B, 4, 16)
    with pytest.raises(RuntimeError, match="no step"):
        stream.labels_step()
    with pytest.raises(RuntimeError, match="no step"):
        stream.score_step()
    d, sd = LabelDefinition(B, LABELS), ScoreDefinition(B, score)
    idn = S.IdentityDefinition(B, more["identity"], score) if metrics else None
    hd = S.HotaDefinition(B, more["hota"], more["identity"], score) if metrics else None
    G = LABELS["max_rows"]
    gt = lc.outputs(B, G)
    gt_match, gt_flags = np.zeros((B, G), np.int64), np.zeros((B, G), np.int32)
    ahead = sorted(frames)
    with torch.no_grad():
        for k in range(STEPS):
            while ahead and (ahead[0] <= k or ahead[0] - EVERY <= k):      # one keyframe ahead of the step
                _push_keyframe(stream, d, ahead[0], frames[ahead[0]], device=ahead[0] == 20)
                ahead.pop(0)
            det, nk = _step(stream, _events(k))
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            ids = stream.track_ids.clone().cpu().numpy()
            before = stream.state.score_state.clone()
            got_gt = stream.labels_step() if k % 2 else None              # (asked for or not: one launch a step)
            got = stream.score_step()
            d.at([_t_step(k)] * B, out=gt)
            sd.step(det, nk, ids, *gt, out=(gt_match, gt_flags))
            if metrics:
                idn.step(det, nk, ids, *gt, gt_match, sd.id)
                hd.step(det, nk, ids, *gt, gt_match, sd.id, idn.track_id)
            labelled = [b for b in range(B) if gt[3][b] >= 0]
            assert labelled == ([] if k < 10 else [0, 1] if k <= 20 else [0] if k <= 30 else []), (k, gt[3])
            if not labelled:
                assert torch.equal(stream.state.score_state, before), k
            if got_gt is not None:
                assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got_gt, stream.labels_step()))
            now = [v.cpu().numpy() for v in stream.labels_step()]
            assert np.array_equal(now[3], gt[3]), (k, now[3], gt[3])
            for b in labelled:
                n = int(gt[3][b])
                assert all(now[i][b, :n].tobytes() == gt[i][b, :n].tobytes() for i in range(3)), (k, b)
                assert np.array_equal(got[0].cpu().numpy()[b, :n], gt_match[b, :n]), (k, b)
                assert np.array_equal(got[1].cpu().numpy()[b, :n], gt_flags[b, :n]), (k, b)
            counters = stream.track_score()
            assert all(np.array_equal(counters[name], sd.counters[name]) for name in S.SCORE_COUNTERS), (k, counters, sd.counters)
            for a, w in zip(stream.scored_objects(), sd.objects()):
                assert a.tobytes() == w.tobytes(), k
            with pytest.raises(RuntimeError, match="scored already"):
                stream.score_step()
        counts = stream.label_counts()
        print({k: v.tolist() for k, v in counts.items()}, {k: v.tolist() for k, v in sd.counters.items()}, sd.events)
        assert all(np.array_equal(counts[name], d.counters[name]) for name in S.LABEL_COUNTERS)
        assert counts["labelled"].tolist() == [21, 11] and counts["outside"].tolist() == [19, 29] and not counts["gap"].any()
        assert counts["keyframes"].tolist() == [3, 2] and sd.counters["match"].sum() > 0 and sd.counters["miss"].sum() > 0
        if metrics:
            got_id, want_id = stream.identity(), idn.solve()
            assert all(np.array_equal(got_id[name], want_id[name]) for name in ("idtp", "idfn", "idfp", "gt_frames", "hyp_frames"))
            got_h, want_h = stream.hota(), hd.solve()
            assert all(np.array_equal(got_h[name], want_h[name]) for name in S.HOTA_COUNTERS + S.HOTA_WORDS)
            assert got_h["instants"].tolist() == [21, 11]
        # score_step(arrays) on a labels= stream is what it always was; a host push that goes back in time raises by name
        _step(stream, _events(STEPS))
        lab = (np.zeros((B, 4, 4), np.float32), np.zeros((B, 4), np.int32), np.ones((B, 4), np.int64))
        assert stream.score_step(*lab)[0].shape == (B, 4)
        with pytest.raises(ValueError, match="not greater than"):
            stream.push_labels(np.full(B, _t_step(30), np.int64), np.zeros((B, 1, 4)), np.zeros((B, 1), np.int32), np.ones((B, 1), np.int64))
        assert np.array_equal(stream.label_counts()["refused"], [0, 0])
        stream.reset()
        assert not any(v.any() for v in stream.label_counts().values())
        with pytest.raises(RuntimeError, match="no step"):
            stream.labels_step()
    eng.set_low_latency(True)


def test_labels_need_neither_track_nor_score_and_bad_options_are_refused_by_name():
    model = _model(B)
    for kw, name in ((dict(labels=dict(max_rows=300)), "DAGR_SCORE_MAX_GT"), (dict(labels=dict(max_keyframes=0)), "max_keyframes"),
                     (dict(labels=dict(gap=3)), "gap"), (dict(labels="on"), "labels"), (dict(labels=dict(max_gap_us=-4)), "max_gap_us")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    stream = EventStream(model, window_us=WINDOW_US, labels=dict(max_rows=4, max_gap_us=5000, min_height=2.0))
    assert stream.track is None and stream.score is None
    with pytest.raises(RuntimeError, match="score="):
        stream.score_step()
    d = LabelDefinition(B, stream.labels)
    rows = np.array([[10, 10, 20, 30], [5, 5, 1, 50], [40, 40, 8, 8], [0, 0, 9, 9], [1, 1, 9, 9]], np.float64)
    # keyframes 1000 us before step 0, at step 2 and at step 10 (the second row is 1 px wide: under min_height)
    for t, shift in ((_t_step(0) - 1000, 0.0), (_t_step(2), 3.0), (_t_step(10), 9.0)):
        move = np.array([shift, shift, 0.0, 0.0])
        xywh, label, ids = np.stack([rows + move, rows - move]), np.zeros((B, 5), np.int32), np.tile(np.arange(1, 6), (B, 1))
        stream.push_labels(np.full(B, t, np.int64), xywh, label, ids)
        for b in range(B):
            d.push(b, t, xywh[b], label[b], ids[b])
    with torch.no_grad():
        for k in range(4):
            _step(stream, _events(k))
            got = [v.cpu().numpy() for v in stream.labels_step()]
            want = d.at([_t_step(k)] * B)
            # steps 0 and 1 lie between the first two keyframes; from step 2 on the bracketing pair is 8000 us apart
            assert np.array_equal(got[3], want[3]) and got[3].tolist() == ([3, 3] if k < 2 else [-1, -1]), (k, got[3])
            for b in range(B):
                n = max(int(want[3][b]), 0)
                assert all(got[i][b, :n].tobytes() == want[i][b, :n].tobytes() for i in range(3)), (k, b)
    counts = stream.label_counts()
    assert counts["cut_rows"].tolist() == [3, 3] and counts["labelled"].tolist() == [2, 2] and counts["gap"].tolist() == [2, 2]
    plain = EventStream(model, window_us=WINDOW_US, track=TRACK, score=True)
    with torch.no_grad():
        _step(plain, _events(0))
    with pytest.raises(RuntimeError, match="labels="):
        plain.score_step()
    for call in (plain.labels_step, plain.label_counts, lambda: plain.push_labels(0, 0, 0, 0)):
        with pytest.raises(RuntimeError, match="labels="):
            call()
    assert plain.state.labels is None and plain.state.labels_state is None


# ------------------------------------------------------------------------------------------------ the calls
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_the_store_changes_no_step_and_a_score_step_adds_one_call(latency, monkeypatch):
    """Step for step a labels= stream issues the library calls of the same stream without it, which issues what it issued
    before the store existed: a scoring stream's steps end with its tracker entry and its score_step(arrays) is the chain
    alone.  score_step() adds exactly one dagr_stream_labels_at in front of the chain, score_step(arrays) adds none, a push
    is one dagr_stream_labels_push, and nobody else ever calls either."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream, scored = {}, {}
    lab = (np.zeros((B, 4, 4), np.float32), np.zeros((B, 4), np.int32), np.ones((B, 4), np.int64))
    chain = ["dagr_stream_score", "dagr_stream_identity"]
    base = dict(track=TRACK, score=True, identity=True)
    for name, kw in (("warm-up", dict()), ("off", dict()), ("scoring", base), ("labels none", dict(base, labels=None)),
                     ("labels", dict(base, labels=LABELS)), ("labels alone", dict(labels=LABELS))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps, scored[name] = [], []
        if stream.labels is not None:
            del calls[:]
            stream.push_labels(np.full(B, _t_step(0), np.int64), np.ones((B, 2, 4)), np.zeros((B, 2), np.int32), np.ones((B, 2), np.int64))
            assert calls == ["dagr_stream_labels_push"]
        with torch.no_grad():
            for k in range(6):
                del calls[:]
                _step(stream, _events(k))
                steps.append(list(calls))
                del calls[:]
                if stream.score is not None:
                    if name == "labels" and k % 2 == 0:
                        stream.score_step()
                    else:
                        stream.score_step(*lab)
                elif name == "labels alone":
                    stream.labels_step()
                    stream.labels_step()
                scored[name].append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
    assert per_stream["labels"] == per_stream["labels none"] == per_stream["scoring"]
    assert per_stream["labels alone"] == per_stream["off"]
    assert not any("labels" in c for steps in per_stream.values() for step in steps for c in step)
    for k, (with_, without) in enumerate(zip(per_stream["scoring"], per_stream["off"])):
        assert with_ == without + (["dagr_stream_t_ref"] if k == 0 else []) + ["dagr_stream_track"], (k, with_, without)
    assert scored["scoring"] == scored["labels none"] == [chain] * 6
    assert scored["labels"] == [["dagr_stream_labels_at"] + chain, chain] * 3
    assert scored["labels alone"] == [["dagr_stream_t_ref", "dagr_stream_labels_at"]] + [["dagr_stream_labels_at"]] * 5
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_scores_every_step_and_leaves_the_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R

    class Labelled(R.SyntheticStream):
        """The stand-in sequence with two labelled boxes at every fourth step, the second one moving."""
        asked = ()

        def label_instants(self):
            return np.array([self.t0 + 1000 * k for k in (2, 6, 10)], np.int64)

        def labels(self, t_step):
            self.asked = self.asked + (int(t_step - self.t0) // 1000,)
            if (t_step - self.t0) // 1000 % 4 != 2:
                return None
            dx = (t_step - self.t0) / 1000.0
            return np.array([[10, 10, 60, 60], [100 + dx, 80, 180 + dx, 160]], np.float32), np.array([0, 1]), np.array([1, 2])

    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "12", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res", "--track", "--track_max_age_us", "2500",
            "--max_tracks", "32", "--track_min_score", "0.3", "--track_score", "--track_score_iou", "0.25"]
    paths, sources = {}, {}
    for name, extra in (("keyframes", []), ("every", ["--track_score_every_step", "--label_max_gap_us", "4000"]),
                        ("gap", ["--track_score_every_step", "--label_max_gap_us", "3999", "--label_min_diag", "100"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        sources[name] = Labelled(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=sources[name])
    printed = capsys.readouterr().out
    for file in ("detections_res.npy", "tracks_res.npy"):
        with open(os.path.join(os.path.dirname(str(paths["keyframes"])), file), "rb") as f:
            want = f.read()
        for name in ("every", "gap"):
            with open(os.path.join(os.path.dirname(str(paths[name])), file), "rb") as g:
                assert want == g.read(), (name, file)           # byte for byte what they are without the flag
    # one keyframe ahead of the step: instant 2 at the first step, 6 once step 2 has come, 10 at step 6; nothing else is asked
    assert sources["every"].asked == (2, 6, 10) and len(sources["keyframes"].asked) == 12
    said = re.findall(r"; scored (\d+) labelled steps: (\d+) objects.*?; every step scored against (\d+) resident keyframes, "
                      r"interpolated: (\d+) steps labelled, (\d+) outside the keyframes, (\d+) in a gap", printed)
    assert said == [("9", "2", "3", "9", "3", "0"), ("1", "1", "3", "1", "3", "8")], printed

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")

    class NoInstants(R.SyntheticStream):
        def labels(self, t_step):
            return None
    no = ["--output_directory", str(tmp_path / "no")]
    plain = NoInstants(C.flags("", base, extra=R.stream_options))
    with pytest.raises(SystemExit, match="label_instants"):
        R.main(base + ["--track_score_every_step"] + no, model_factory=refuse, source=plain)
    with pytest.raises(SystemExit, match="needs --track_score_every_step"):
        R.main(base + ["--label_min_diag", "3"] + no, model_factory=refuse, source=plain)
    with pytest.raises(SystemExit, match="needs --track_score"):
        R.main([v for v in base if v != "--track_score"][:-2] + ["--track_score_every_step"] + no, model_factory=refuse, source=plain)
