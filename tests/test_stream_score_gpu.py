"""The event stream's scorer on the GPU: dagr_stream_score through the binding against the numpy definition
(dagr_amd/streaming.py: ScoreDefinition), integer for integer after every step of every case of tests/stream_score_cases.py
and of the seeded walks; the four tracker entries chained with the scorer on the device; its refusals; EventStream(track=,
score=) against definitions fed with every step's own detections, in latency and in throughput mode; the library calls of
streams with and without the scorer; and scripts/run_stream.py --track_score."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, ScoreDefinition, TrackDefinition
from tests import stream_score_cases as sc
from tests.test_stream_motion_gpu import _Tracker as _MotionTracker
from tests.test_stream_rescue_gpu import _Tracker as _RescueTracker
from tests.test_stream_rescue_gpu import _events, _step
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import _dev, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
WINDOW_US = 20000
SENTINEL = sc.SENTINEL


def _d(v):
    return v if torch.is_tensor(v) or v is None else _dev(v)


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Scorer:
    """dagr_stream_score on a state of its own; the state starts out as garbage in front of its reset, both outputs as the
    sentinel -7 (they are never refilled: what a step leaves alone stays)."""

    def __init__(self, B_, A, G, score):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.G, self.o = B_, A, G, S._score_options(score, True, True, "test")
        self.M = M = self.o["max_objects"]
        self.nbytes = self.L.dagr_stream_score_bytes(B_, M)
        assert self.nbytes == 64 * B_ * M + 128 * B_
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_score_reset(_lib.ptr(self.state), self.nbytes, B_, M, _lib.cur_stream(self.dev)),
                   "dagr_stream_score_reset")
        self.match = torch.full((B_, G), SENTINEL, dtype=torch.int64, device=self.dev)
        self.flags = torch.full((B_, G), SENTINEL, dtype=torch.int32, device=self.dev)

    def call(self, s, **over):
        P = _lib.ptr
        t = {k: _d(s[k]) for k in ("det", "n_keep", "track_id", "gt_box", "gt_label", "gt_id", "n_gt")}
        box = _d(s["track_box"]) if self.o["boxes"] == "track" else None
        a = dict(state=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, iou=self.o["iou"], A=self.A, G=self.G,
                 track_box=None if box is None else P(box), gt_match=P(self.match), gt_flags=P(self.flags),
                 **{k: P(v) for k, v in t.items()})
        a.update(over)
        rc = self.L.dagr_stream_score(a["state"], a["bytes"], a["B"], a["M"], a["iou"], a["det"], a["n_keep"], a["A"],
                                      a["track_id"], a["track_box"], a["gt_box"], a["gt_label"], a["gt_id"], a["n_gt"], a["G"],
                                      a["gt_match"], a["gt_flags"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def words(self):
        """``(table int64 [8, B, M], lane words int64 [B, 16])`` through the layout include/dagr_hip.h documents."""
        raw, n = self.state.view(torch.int64).cpu().numpy(), self.B * self.M
        return raw[:8 * n].reshape(8, self.B, self.M), raw[8 * n:].reshape(self.B, 16)


def _assert_state(scorer, d, where):
    table, words = scorer.words()
    assert np.array_equal(words[:, 0], d.n_objects), (where, "n_objects")
    for i, name in enumerate(S.SCORE_COUNTERS):
        assert np.array_equal(words[:, 1 + i], d.counters[name]), (where, name, words[:, 1 + i], d.counters[name])
    assert not words[:, 13:].any(), where
    for i, name in enumerate(S.SCORE_OBJECT_FIELDS):          # (behind n_objects both hold what the reset left)
        assert np.array_equal(table[i], getattr(d, name)), (where, "table", name)
    return table, words


def _run_case(case):
    scorer = _Scorer(case["B"], case["A"], case["G"], case["score"])
    d = ScoreDefinition(case["B"], case["score"])
    match, flags = np.full((case["B"], case["G"]), SENTINEL, np.int64), np.full((case["B"], case["G"]), SENTINEL, np.int32)
    for k, s in enumerate(case["steps"]):
        _lib.check(scorer.call(s), "dagr_stream_score")
        d.step(s["det"], s["n_keep"], s["track_id"], s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"], track_box=s["track_box"],
               out=(match, flags))
        got_match, got_flags = scorer.match.cpu().numpy(), scorer.flags.cpu().numpy()
        # whole arrays: the rows behind n_gt and the rows of a skipped lane hold what they held (first the sentinel)
        assert np.array_equal(got_match, match), (case["name"], k, "gt_match")
        assert np.array_equal(got_flags, flags), (case["name"], k, "gt_flags")
        table, words = _assert_state(scorer, d, (case["name"], k))
        if case["expect"] is not None:
            counters = {name: words[:, 1 + i] for i, name in enumerate(S.SCORE_COUNTERS)}
            objects = [S.objects_from_arrays(int(words[b, 0]), *table[:, b]) for b in range(case["B"])]
            sc.check_expectation(case, k, got_match, got_flags, counters, objects)
    return scorer, d


@pytest.mark.parametrize("name", [c["name"] for c in sc.cases()])
def test_the_scorer_equals_the_definition_after_every_step(name):
    """Integer for integer after every step: gt_match and gt_flags (whole arrays: the sentinel survives behind n_gt and in
    a skipped lane), every counter, n_objects and the whole object table; and the case's written-out expectation.  Among
    the cases: 300 rows with ids against the cap of 256, G = 256, 1024 objects filled over four steps."""
    _run_case(next(c for c in sc.cases() if c["name"] == name))


@pytest.mark.parametrize("max_objects,boxes,iou", sc.WALKS)
def test_the_walks_equal_the_definition_at_every_step(max_objects, boxes, iou):
    """B = 3, A = 64, 36 labelled objects a lane over 40 steps, the ids TrackDefinition's on the host: a full table at 40
    objects, one table word a thread at 64, a tail at 130; the detections' and the motion model's boxes."""
    _, d = _run_case(sc.walk(max_objects, boxes, iou))
    assert all(d.events[k] > 0 for k in ("matched", "missed", "switched", "fragmented", "kept", "keep_lost", "new_objects")), d.events


@pytest.mark.parametrize("variant", [v[0] for v in sc.VARIANTS])
def test_the_tracker_entries_chained_with_the_scorer_on_the_device(variant):
    """40 steps of the labelled scene: dagr_stream_track / _cv / _rescue / _cv_rescue followed by dagr_stream_score on the
    track ids that entry left on the device.  The final counters and tables equal the definitions' chain."""
    _, motion, rescue = next(v for v in sc.VARIANTS if v[0] == variant)
    steps = 40
    want, _ = sc.scene_chain(variant, steps)
    Bs, A = sc.SCENE["B"], sc.SCENE["A"]
    if rescue:
        tr = _RescueTracker(Bs, A, sc.SCENE_TRACK, motion, rescue)
        ids, entry = tr.out["ids"], tr.family + "_rescue"
    elif motion:
        tr = _MotionTracker(Bs, A, sc.SCENE_TRACK, motion)
        ids, entry = tr.out["ids"], "dagr_stream_track_cv"
    else:
        tr = _PlainTracker(Bs, A, sc.SCENE_TRACK)
        ids, entry = tr.ids, "dagr_stream_track"
    scorer = _Scorer(Bs, A, sc.SCENE["objects"], True)
    for s in sc.scene()[:steps]:
        _lib.check(tr.call(s), entry)
        _lib.check(scorer.call(dict(s, track_id=ids, track_box=None)), "dagr_stream_score")
    _assert_state(scorer, want, variant)
    assert want.counters["match"].sum() > 0 and want.counters["switch"].sum() > 0


def test_argument_errors_launch_nothing():
    case = next(c for c in sc.cases() if c["name"].startswith("a-skipped-lane"))
    scorer, _ = _run_case(case)
    s = case["steps"][-1]
    before, match, flags = scorer.state.clone(), scorer.match.clone(), scorer.flags.clone()
    bad, nan = _lib.ENUMS["DAGR_ERR_INVALID_ARG"], float("nan")
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    refusals = [(dict(state=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(n_gt=None), b"NULL"), (dict(det=None), b"NULL"),
                (dict(track_id=None), b"NULL"), (dict(gt_box=None), b"NULL ground truth"), (dict(gt_id=None), b"NULL ground truth"),
                (dict(gt_label=None), b"NULL ground truth"), (dict(bytes=scorer.nbytes - 1), b"smaller"), (dict(B=0), b"out of range"),
                (dict(B=65536), b"out of range"), (dict(M=0), b"max_objects"), (dict(M=1025), b"max_objects"),
                (dict(G=-1), b"G out of range"), (dict(G=257), b"G out of range"), (dict(A=-1), b"A out of range"),
                (dict(iou=0.0), b"iou must be in (0, 1]"), (dict(iou=1.5), b"iou"), (dict(iou=-0.5), b"iou"), (dict(iou=nan), b"iou"),
                (dict(gt_match=None), b"NULL together"), (dict(gt_flags=None), b"NULL together"),
                (dict(state=odd(scorer.state, 8)), b"aligned"), (dict(gt_match=odd(scorer.match, 4)), b"aligned"),
                (dict(gt_flags=odd(scorer.flags, 2)), b"aligned"), (dict(track_box=odd(scorer.state, 8)), b"aligned")]
    for over, text in refusals:
        assert scorer.call(s, **over) == bad, over
        said = scorer.L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_score:"), (over, said)
    assert scorer.L.dagr_stream_score_bytes(0, 4) == 0 and scorer.L.dagr_stream_score_bytes(1, 1025) == 0
    assert scorer.L.dagr_stream_score_reset(_lib.ptr(scorer.state), scorer.nbytes - 1, scorer.B, scorer.M,
                                            _lib.cur_stream(scorer.dev)) == bad
    torch.cuda.synchronize()
    assert torch.equal(scorer.state, before) and torch.equal(scorer.match, match) and torch.equal(scorer.flags, flags)
    # both outputs may be NULL: the step counts the same
    want = ScoreDefinition(case["B"], case["score"])
    _lib.check(scorer.L.dagr_stream_score_reset(_lib.ptr(scorer.state), scorer.nbytes, scorer.B, scorer.M,
                                                _lib.cur_stream(scorer.dev)), "reset")
    for q in case["steps"]:
        assert scorer.call(q, gt_match=None, gt_flags=None) == 0
        want.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"])
    _assert_state(scorer, want, "NULL outputs")
    assert torch.equal(scorer.match, match) and torch.equal(scorer.flags, flags)


# ------------------------------------------------------------------------------------------------ the stream, end to end
TRACK = dict(iou=0.3, max_age_us=2500, min_score=0.0, max_tracks=64)
G = 8


def _labels(det, nk, k):
    """Ground truth made of the step's own detections: per lane the first rows, moved by half a pixel, under identities that
    follow the row index -- the head's rows change places from step to step, so identities change tracks.  Lane 1 has no
    labels at the steps with k % 6 == 3, and its last label has no identity."""
    gt_box = np.zeros((B, G, 4), np.float32)
    gt_label, gt_id, n_gt = np.zeros((B, G), np.int32), np.zeros((B, G), np.int64), np.zeros(B, np.int32)
    for b in range(B):
        n = min(int(nk[b]), G)
        gt_box[b, :n] = det[b, :n, :4] + np.float32(0.5)
        gt_label[b, :n] = det[b, :n, 5].astype(np.int32)
        gt_id[b, :n] = 10 * b + 1 + np.arange(n)
        n_gt[b] = n
    gt_id[1, max(int(n_gt[1]) - 1, 0)] = 0
    if k % 6 == 3:
        n_gt[1] = -1
    return gt_box, gt_label, gt_id, n_gt


@pytest.mark.parametrize("motion,boxes", [(None, "det"), (dict(alpha=0.5, beta=0.25), "track")], ids=["det", "track-boxes"])
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_scoring_stream_equals_the_definitions(latency, motion, boxes):
    """B = 2, twelve steps, a score_step on every third: gt_match, gt_flags, track_score() and scored_objects() equal a
    ScoreDefinition fed with the step's own detections and a TrackDefinition's ids; score_step raises before the first step,
    twice for one step and on a stream without score=; reset() empties the scorer."""
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    score = dict(iou=0.5, max_objects=16, boxes=boxes)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, motion=motion, score=score)
    assert stream.score == dict(iou=0.5, max_objects=16, boxes=boxes)
    assert stream.state.score_state.numel() == 64 * B * 16 + 128 * B
    empty = (np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32), np.ones((B, G), np.int64))
    with pytest.raises(RuntimeError, match="no step"):
        stream.score_step(*empty)
    trk, d = TrackDefinition(B, TRACK, motion=motion), ScoreDefinition(B, score)
    with torch.no_grad():
        for rnd in range(2):
            for k in range(12):
                s = _events(k)
                det, nk = _step(stream, s)
                det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                ids, _ = trk.step(det, nk, s["t_now"])
                assert np.array_equal(stream.track_ids.cpu().numpy()[0, :nk[0]], ids[0, :nk[0]]), k
                if k % 3:
                    continue
                lab = _labels(det, nk, k)
                device = k % 6 == 0                  # host arrays and device tensors alike
                got = stream.score_step(*(_dev(v) for v in lab)) if device else stream.score_step(*lab)
                want = d.step(det, nk, ids, *lab, track_box=trk.track_box if motion else None)
                for b in range(B):
                    n = max(int(lab[3][b]), 0)
                    assert np.array_equal(got[0].cpu().numpy()[b, :n], want[0][b, :n]), (rnd, k, b)
                    assert np.array_equal(got[1].cpu().numpy()[b, :n], want[1][b, :n]), (rnd, k, b)
                with pytest.raises(RuntimeError, match="scored already"):
                    stream.score_step(*lab)
            counters = stream.track_score()
            print("round", rnd, {name: v.tolist() for name, v in counters.items()}, d.events)
            assert all(counters[name].dtype == np.int64 and np.array_equal(counters[name], d.counters[name])
                       for name in S.SCORE_COUNTERS)
            assert counters["steps"].tolist() == [4, 2] and counters["match"].sum() > 0 and counters["unscored_gt"][1] > 0
            for got, want in zip(stream.scored_objects(), d.objects()):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), rnd
            m = S.score_summary(counters, stream.scored_objects())
            assert m["total"]["gt"] == int(d.counters["gt"].sum()) and m["total"]["mota"] <= 1.0
            stream.check_status()
            stream.reset()
            assert not any(v.any() for v in stream.track_score().values()) and all(len(t) == 0 for t in stream.scored_objects())
            with pytest.raises(RuntimeError, match="no step"):
                stream.score_step(*empty)
            trk.reset()
            d.reset()
        only = EventStream(model, window_us=WINDOW_US, track=TRACK)
        assert only.score is None and only.state.score is None and only.state.score_state is None
        _step(only, _events(0))
        for call in (lambda: only.score_step(*empty), only.track_score, only.scored_objects):
            with pytest.raises(RuntimeError, match="score="):
                call()
    eng.set_low_latency(True)


def test_event_stream_refuses_bad_score_options_by_name():
    model = _model(B)
    for kw, name in ((dict(score=True), "score= needs track="), (dict(track=True, score=dict(iou=0.0)), "score iou"),
                     (dict(track=True, score=dict(boxes="track")), "needs motion="),
                     (dict(track=True, score=dict(max_objects=2000)), "DAGR_SCORE_MAX_OBJECTS"),
                     (dict(track=True, score=dict(threshold=1)), "threshold"), (dict(track=True, score="yes"), "score")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    stream = EventStream(model, window_us=WINDOW_US, track=True, score=True)
    with torch.no_grad():
        _step(stream, _events(0))
    with pytest.raises(ValueError, match="DAGR_SCORE_MAX_GT"):
        stream.score_step(np.zeros((B, 300, 4), np.float32), np.zeros((B, 300), np.int32), np.zeros((B, 300), np.int64))
    with pytest.raises(ValueError, match="gt_label has shape"):
        stream.score_step(np.zeros((B, 4, 4), np.float32), np.zeros((B, 5), np.int32), np.zeros((B, 4), np.int64))


# ------------------------------------------------------------------------------------------------ the calls
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_scoring_changes_no_step_and_a_score_step_is_one_call(latency, monkeypatch):
    """Step for step a scoring stream issues the library calls of the tracking stream without score=, which issues what it
    issued before (a stream without track= plus its one tracker entry); a score_step issues exactly one dagr_stream_score,
    and nobody else ever calls it."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream, scored = {}, []
    lab = (np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32), np.ones((B, G), np.int64))
    for name, kw in (("warm-up", dict()), ("off", dict()), ("tracking", dict(track=TRACK)), ("scoring", dict(track=TRACK, score=True)),
                     ("score none", dict(track=TRACK, score=None))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps = []
        with torch.no_grad():
            for k in range(6):
                s = _events(k)
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
                if name == "scoring" and k % 2 == 0:
                    del calls[:]
                    stream.score_step(*lab)
                    scored.append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
    assert scored == [["dagr_stream_score"]] * 3
    assert per_stream["scoring"] == per_stream["tracking"] == per_stream["score none"]
    assert not any("score" in c for name, steps in per_stream.items() for step in steps for c in step)
    for k, (with_, without) in enumerate(zip(per_stream["tracking"], per_stream["off"])):
        assert with_ == without + (["dagr_stream_t_ref"] if k == 0 else []) + ["dagr_stream_track"], (k, with_, without)
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_prints_the_score_and_leaves_the_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R

    class Labelled(R.SyntheticStream):
        """The stand-in sequence with two labelled boxes at every other step."""
        asked = 0

        def labels(self, t_step):
            self.asked += 1
            if (t_step - self.t0) // 1000 % 2:
                return None
            return np.array([[10, 10, 60, 60], [100, 80, 180, 160]], np.float32), np.array([0, 1]), np.array([1, 2])

    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res", "--track", "--track_max_age_us", "2500",
            "--max_tracks", "32", "--track_min_score", "0.3"]
    paths, sources = {}, {}
    for name, extra in (("track", []), ("score", ["--track_score", "--track_score_iou", "0.25"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        sources[name] = Labelled(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=sources[name])
    printed = capsys.readouterr().out
    for file in ("detections_res.npy", "tracks_res.npy"):
        with open(os.path.join(os.path.dirname(str(paths["track"])), file), "rb") as f, \
                open(os.path.join(os.path.dirname(str(paths["score"])), file), "rb") as g:
            assert f.read() == g.read(), file              # byte for byte what they are without the flag
    assert (sources["track"].asked, sources["score"].asked) == (0, 10)
    said = re.findall(r"; scored (\d+) labelled steps: (\d+) objects, (\d+) id switches, (\d+) fragmentations, (\d+) misses, "
                      r"(\d+) false positives, MOTA (-?[\d.]+|nan), MOTP ([\d.]+|nan), (\d+) mostly tracked, (\d+) mostly lost", printed)
    assert len(said) == 1 and said[0][:2] == ("5", "2"), printed

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")
    plain = R.SyntheticStream(C.flags("", base, extra=R.stream_options))
    with pytest.raises(SystemExit, match="has none"):
        R.main(base + ["--track_score", "--output_directory", str(tmp_path / "no")], model_factory=refuse, source=plain)
    with pytest.raises(SystemExit, match="has none"):
        R.main(base + ["--track_score", "--output_directory", str(tmp_path / "no")], model_factory=refuse)
