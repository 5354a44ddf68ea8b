"""The event stream's identity state on the GPU: dagr_stream_identity and dagr_stream_identity_solve through the binding
against the numpy definition (dagr_amd/streaming.py: IdentityDefinition), integer for integer -- the hand-built cases, the
four tracker entries chained with the scorer and the identity step on the device, the scene that crosses the boundaries --;
the solve's pairing is checked for being right, never for being the definition's; the refusals; EventStream(identity=)
against the definitions, in latency and in throughput mode, and its library calls; scripts/run_stream.py --track_identity."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, IdentityDefinition, ScoreDefinition, check_identity
from tests import stream_identity_cases as ic
from tests import stream_score_cases as sc
from tests.test_stream_motion_gpu import _Tracker as _MotionTracker
from tests.test_stream_rescue_gpu import _Tracker as _RescueTracker
from tests.test_stream_rescue_gpu import _events, _step
from tests.test_stream_score_gpu import TRACK, WINDOW_US, _labels, _Scorer
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import _dev, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2


def _d(v):
    return v if torch.is_tensor(v) or v is None else _dev(v)


class _Identity:
    """dagr_stream_identity behind a scorer (tests/test_stream_score_gpu._Scorer) on a state of its own; the state, the
    workspace and the solve's outputs start out as garbage in front of the reset."""

    def __init__(self, scorer, identity):
        self.L, self.dev, self.scorer = _lib.lib(), scorer.dev, scorer
        self.B, self.M, self.T = scorer.B, scorer.M, S._identity_options(identity, scorer.o, "test")["max_tracks"]
        B_, M, T = self.B, self.M, self.T
        self.nbytes = self.L.dagr_stream_identity_bytes(B_, M, T)
        assert self.nbytes == -(-(16 * B_ * T + 8 * B_ * M + 64 * B_ + 4 * B_ * M * T + 4 * B_ * M) // 16) * 16
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_identity_reset(_lib.ptr(self.state), self.nbytes, B_, M, T, _lib.cur_stream(self.dev)),
                   "dagr_stream_identity_reset")
        self.ws_bytes = self.L.dagr_assign_workspace_bytes(B_, M, T)
        self.ws = torch.full((self.ws_bytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        self.obj_track = torch.full((B_, M), -7, dtype=torch.int64, device=self.dev)
        self.result = torch.full((B_, 9), -7, dtype=torch.int64, device=self.dev)

    def call(self, s, **over):
        """The identity step on the arrays the scorer has just scored (its gt_match, its state)."""
        P, sr = _lib.ptr, self.scorer
        t = {k: _d(s[k]) for k in ("det", "n_keep", "track_id", "gt_box", "gt_label", "gt_id", "n_gt")}
        box = _d(s["track_box"]) if sr.o["boxes"] == "track" else None
        a = dict(state=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, T=self.T, iou=sr.o["iou"], score=P(sr.state),
                 score_bytes=sr.nbytes, A=sr.A, G=sr.G, track_box=None if box is None else P(box), gt_match=P(sr.match),
                 **{k: P(v) for k, v in t.items()})
        a.update(over)
        rc = self.L.dagr_stream_identity(a["state"], a["bytes"], a["B"], a["M"], a["T"], a["iou"], a["score"], a["score_bytes"],
                                         a["det"], a["n_keep"], a["A"], a["track_id"], a["track_box"], a["gt_box"],
                                         a["gt_label"], a["gt_id"], a["n_gt"], a["G"], a["gt_match"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def solve(self, **over):
        P = _lib.ptr
        a = dict(state=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, T=self.T, obj_track=P(self.obj_track),
                 result=P(self.result), ws=P(self.ws), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.L.dagr_stream_identity_solve(a["state"], a["bytes"], a["B"], a["M"], a["T"], a["obj_track"], a["result"],
                                               a["ws"], a["ws_bytes"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()
        return rc

    def tables(self):
        """The state through the layout include/dagr_hip.h documents, as tests/stream_identity_cases.tables has it."""
        B_, M, T = self.B, self.M, self.T
        raw = self.state.cpu().numpy()
        n64 = 2 * B_ * T + B_ * M + 8 * B_
        q, r = raw[:8 * n64].view(np.int64), raw[8 * n64:8 * n64 + 4 * (B_ * M * T + B_ * M)].view(np.int32)
        words = q[2 * B_ * T + B_ * M:].reshape(B_, 8)
        return dict(track_id=q[:B_ * T].reshape(B_, T), track_len=q[B_ * T:2 * B_ * T].reshape(B_, T),
                    obj_len=q[2 * B_ * T:2 * B_ * T + B_ * M].reshape(B_, M), overlap=r[:B_ * M * T].reshape(B_, M, T),
                    words={name: words[:, i] for i, name in enumerate(S.IDENTITY_WORDS)})

    def solved(self):
        result, obj_track = self.result.cpu().numpy(), self.obj_track.cpu().numpy()
        return dict({name: result[:, i] for i, name in enumerate(S.IDENTITY_RESULT)}, obj_track=obj_track)


def _assert_tables(got, want, where):
    for name in ("track_id", "track_len", "obj_len", "overlap"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (where, name)
    for name in S.IDENTITY_WORDS:
        assert np.array_equal(got["words"][name], want["words"][name]), (where, name, got["words"][name], want["words"][name])


def _assert_solve(ident, want, where):
    """The solve's integers equal the definition's; its pairing is a right one for the device's own tables."""
    _lib.check(ident.solve(), "dagr_stream_identity_solve")
    got, t = ident.solved(), ident.tables()
    for name in S.IDENTITY_RESULT:
        assert np.array_equal(got[name], want[name]), (where, name, got[name], want[name])
    for b in range(ident.B):
        assert check_identity(t["overlap"][b], t["track_id"][b], got, b) is None, (where, b)
    return got


def _run(case_B, A, G_, steps, score, identity, shots, where):
    """Scorer then identity step on the device for every step; the tables equal the definition's snapshots."""
    scorer = _Scorer(case_B, A, G_, score)
    ident = _Identity(scorer, identity)
    shots = dict(shots)
    for k, s in enumerate(steps):
        _lib.check(scorer.call(s), "dagr_stream_score")
        _lib.check(ident.call(s), "dagr_stream_identity")
        if k in shots:
            _assert_tables(ident.tables(), shots[k], (where, k))
    return ident


@pytest.mark.parametrize("name", [c["name"] for c in ic.cases()])
def test_the_hand_built_cases_equal_the_definition_and_their_tables(name):
    case = next(c for c in ic.cases() if c["name"] == name)
    _, d, want = ic.run_definition(case)
    ident = _run(case["B"], case["A"], case["G"], case["steps"], case["score"], case["identity"],
                 [(len(case["steps"]) - 1, ic.tables(d))], name)
    got = _assert_solve(ident, want, name)
    ic.check_expectation(case, ident.tables(), got)


@pytest.mark.parametrize("variant", [v[0] for v in sc.VARIANTS])
def test_the_tracker_entries_chained_with_the_scorer_and_the_identity_step_on_the_device(variant):
    """150 steps of the labelled scene, B = 2, 6 objects, A = 32: dagr_stream_track / _cv / _rescue / _cv_rescue, then
    dagr_stream_score, then dagr_stream_identity on what they left on the device.  After every 25th step and at the end
    every table and word equals the definitions' chain; the solve gives its idtp / idfn / idfp and a right obj_track."""
    _, motion, rescue = next(v for v in sc.VARIANTS if v[0] == variant)
    d, shots, want = ic.scene_chain(variant)
    shots = dict(shots)
    Bs, A = ic.SCENE["B"], ic.SCENE["A"]
    if rescue:
        tr = _RescueTracker(Bs, A, sc.SCENE_TRACK, motion, rescue)
        ids, entry = tr.out["ids"], tr.family + "_rescue"
    elif motion:
        tr = _MotionTracker(Bs, A, sc.SCENE_TRACK, motion)
        ids, entry = tr.out["ids"], "dagr_stream_track_cv"
    else:
        tr = _PlainTracker(Bs, A, sc.SCENE_TRACK)
        ids, entry = tr.ids, "dagr_stream_track"
    scorer = _Scorer(Bs, A, ic.SCENE["objects"], True)
    ident = _Identity(scorer, True)
    for k, s in enumerate(ic.scene()):
        _lib.check(tr.call(s), entry)
        q = dict(s, track_id=ids, track_box=None)
        _lib.check(scorer.call(q), "dagr_stream_score")
        _lib.check(ident.call(q), "dagr_stream_identity")
        if k in shots:
            _assert_tables(ident.tables(), shots[k], (variant, k))
    assert len(shots) == 6 and d.events["pairs"] > 0 and d.events["rows_skipped"] > 0
    got = _assert_solve(ident, want, variant)
    print(variant, S.identity_summary(got)["total"])


def test_the_scene_that_crosses_the_boundaries():
    """G = 70 rows and 70 hypotheses of A = 80 (a thread's second register), max_tracks = 8 (the track table overflows),
    max_objects = 16 (the scorer leaves rows unscored, the last slot belongs to a row >= 64), 12 steps, one lane skipped
    once: the tables equal the definition's after every step."""
    c = ic.CROSSING
    steps, _, d, shots, want = ic.crossing()
    ident = _run(c["B"], c["A"], c["G"], steps, c["score"], c["identity"], shots, "crossing")
    assert len(shots) == c["steps"] and d.events["unlisted"] > 0 and d.events["duplicates"] > 0
    _assert_solve(ident, want, "crossing")


def test_argument_errors_launch_nothing():
    case = next(c for c in ic.cases() if c["name"].startswith("a-skipped-lane"))
    _, d, want = ic.run_definition(case)
    ident = _run(case["B"], case["A"], case["G"], case["steps"], case["score"], case["identity"], [], "errors")
    _lib.check(ident.solve(), "dagr_stream_identity_solve")
    s = case["steps"][-1]
    before = [t.clone() for t in (ident.state, ident.obj_track, ident.result, ident.scorer.state)]
    bad, nan = _lib.ENUMS["DAGR_ERR_INVALID_ARG"], float("nan")
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    refusals = [(dict(state=None), b"NULL"), (dict(score=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(n_gt=None), b"NULL"),
                (dict(det=None), b"NULL"), (dict(track_id=None), b"NULL"), (dict(gt_box=None), b"NULL ground truth"),
                (dict(gt_id=None), b"NULL ground truth"), (dict(gt_label=None), b"NULL ground truth"),
                (dict(gt_match=None), b"NULL ground truth"), (dict(bytes=ident.nbytes - 1), b"smaller"),
                (dict(score_bytes=ident.scorer.nbytes - 1), b"dagr_stream_score_bytes"), (dict(B=0), b"out of range"),
                (dict(B=65536), b"out of range"), (dict(M=0), b"max_objects"), (dict(M=1025), b"max_objects"),
                (dict(T=0), b"max_tracks"), (dict(T=1025), b"max_tracks"), (dict(G=-1), b"G out of range"),
                (dict(G=257), b"G out of range"), (dict(A=-1), b"A out of range"), (dict(iou=0.0), b"iou must be in (0, 1]"),
                (dict(iou=1.5), b"iou"), (dict(iou=nan), b"iou"), (dict(state=odd(ident.state, 8)), b"aligned"),
                (dict(score=odd(ident.scorer.state, 8)), b"aligned"), (dict(gt_match=odd(ident.scorer.match, 4)), b"aligned"),
                (dict(track_box=odd(ident.state, 8)), b"aligned")]
    for over, text in refusals:
        assert ident.call(s, **over) == bad, over
        said = ident.L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_identity:"), (over, said)
    for over, text in [(dict(state=None), b"NULL"), (dict(obj_track=None), b"NULL"), (dict(result=None), b"NULL"),
                       (dict(ws=None), b"NULL"), (dict(bytes=ident.nbytes - 1), b"smaller"),
                       (dict(ws_bytes=ident.ws_bytes - 1), b"dagr_assign_workspace_bytes"), (dict(B=0), b"out of range"),
                       (dict(T=1025), b"max_tracks"), (dict(ws=odd(ident.ws, 8)), b"aligned"),
                       (dict(result=odd(ident.result, 4)), b"aligned")]:
        assert ident.solve(**over) == bad, over
        said = ident.L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_identity_solve:"), (over, said)
    L = ident.L
    assert L.dagr_stream_identity_bytes(0, 4, 4) == 0 and L.dagr_stream_identity_bytes(1, 1025, 4) == 0
    assert L.dagr_stream_identity_bytes(1, 4, 1025) == 0
    assert L.dagr_stream_identity_reset(_lib.ptr(ident.state), ident.nbytes - 1, ident.B, ident.M, ident.T,
                                        _lib.cur_stream(ident.dev)) == bad
    torch.cuda.synchronize()
    for t, was in zip((ident.state, ident.obj_track, ident.result, ident.scorer.state), before):
        assert torch.equal(t, was)
    # a solve changes no count: the step after it goes on from the same tables
    _assert_tables(ident.tables(), ic.tables(d), "after the solve")


# ------------------------------------------------------------------------------------------------ the stream, end to end
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_an_identity_stream_changes_nothing_else_and_equals_the_definitions(latency, monkeypatch):
    """B = 2, twelve steps, a score_step on every third.  A stream with identity=True returns bit-identical detections,
    track ids, gt_match and track_score() to one without it; its score_step is exactly dagr_stream_score followed by
    dagr_stream_identity, and a stream without identity= records what it records today; identity() and identity_tables()
    equal an IdentityDefinition fed the read-back arrays; reset() empties the state."""
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    score, identity = dict(iou=0.5, max_objects=16), dict(max_tracks=24)
    plain = EventStream(model, window_us=WINDOW_US, track=TRACK, score=score)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, score=score, identity=identity)
    assert stream.identity_options == identity and plain.identity_options is None and plain.state.identity_state is None
    assert stream.state.identity_state.numel() == _lib.lib().dagr_stream_identity_bytes(B, 16, 24)
    sd, d = ScoreDefinition(B, score), IdentityDefinition(B, identity, score)
    calls = _record_calls(monkeypatch)
    seen = {"with": [], "without": []}
    with torch.no_grad():
        for rnd in range(2):
            for k in range(12):
                s = _events(k)
                det_p, nk_p = (t.clone() for t in _step(plain, s))
                det, nk = (t.clone() for t in _step(stream, s))
                assert torch.equal(nk, nk_p), k
                for lane in range(B):
                    n = int(nk[lane])
                    assert torch.equal(det[lane, :n], det_p[lane, :n]), (k, lane)
                    assert torch.equal(stream.track_ids[lane, :n], plain.track_ids[lane, :n]), (k, lane)
                if k % 3:
                    continue
                det, nk, ids = det.cpu().numpy(), nk.cpu().numpy(), stream.track_ids.cpu().numpy()
                lab = _labels(det, nk, k)
                del calls[:]
                want = [t.clone() for t in plain.score_step(*lab)]
                seen["without"].append(list(calls))
                del calls[:]
                got = stream.score_step(*lab)
                seen["with"].append(list(calls))
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), k
                match, _ = sd.step(det, nk, ids, *lab)
                d.step(det, nk, ids, *lab, match, sd.id)
            assert seen["with"] == [["dagr_stream_score", "dagr_stream_identity"]] * len(seen["with"])
            assert seen["without"] == [["dagr_stream_score"]] * len(seen["without"])
            a, b = stream.track_score(), plain.track_score()
            assert all(np.array_equal(a[name], b[name]) for name in S.SCORE_COUNTERS)
            del calls[:]
            got = stream.identity()
            assert list(calls) == ["dagr_stream_identity_solve"]
            t = stream.identity_tables()
            _assert_tables(t, ic.tables(d), ("stream", rnd))
            want = d.solve()
            print("round", rnd, {k: v.tolist() for k, v in got.items() if k != "obj_track"}, d.events)
            for name in S.IDENTITY_RESULT:
                assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), (rnd, name)
            full = dict(got, obj_track=np.stack([np.pad(v, (0, 16 - len(v))) for v in got["obj_track"]]))
            for lane in range(B):
                assert len(got["obj_track"][lane]) == got["n_objects"][lane]
                assert check_identity(t["overlap"][lane], t["track_id"][lane], full, lane) is None, (rnd, lane)
            assert got["idtp"].sum() > 0 and d.events["pairs"] > 0
            stream.reset()
            plain.reset()
            t = stream.identity_tables()
            assert not any(t[name].any() for name in ("track_id", "track_len", "obj_len", "overlap"))
            assert not any(v.any() for v in t["words"].values())
            assert not any(stream.identity()[name].any() for name in S.IDENTITY_RESULT)
            sd.reset()
            d.reset()
            seen = {"with": [], "without": []}
        for call in (plain.identity, plain.identity_tables):
            with pytest.raises(RuntimeError, match="identity="):
                call()
    eng.set_low_latency(True)


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_identity_changes_no_step_and_a_score_step_is_two_calls(latency, monkeypatch):
    """Step for step an identity stream issues the library calls of the scoring stream without identity=, which issues what
    it issues today; its score_step is exactly dagr_stream_score followed by dagr_stream_identity, a scoring stream's
    exactly dagr_stream_score; nobody else ever calls an identity entry."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream, scored = {}, {}
    lab = (np.zeros((B, 8, 4), np.float32), np.zeros((B, 8), np.int32), np.ones((B, 8), np.int64))
    # (the first stream warms the engine up -- eager steps, the capture -- so that those after it meet the same engine)
    for name, kw in (("warm-up", dict()), ("tracking", dict(track=TRACK)), ("scoring", dict(track=TRACK, score=True)),
                     ("identity", dict(track=TRACK, score=True, identity=True)),
                     ("identity none", dict(track=TRACK, score=True, identity=None))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps, scored[name] = [], []
        with torch.no_grad():
            for k in range(6):
                s = _events(k)
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
                if stream.score is not None and k % 2 == 0:
                    del calls[:]
                    stream.score_step(*lab)
                    scored[name].append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
    assert scored["identity"] == [["dagr_stream_score", "dagr_stream_identity"]] * 3
    assert scored["scoring"] == scored["identity none"] == [["dagr_stream_score"]] * 3
    assert per_stream["identity"] == per_stream["scoring"] == per_stream["identity none"] == per_stream["tracking"]
    assert not any("identity" in c or "assign" in c for steps in per_stream.values() for step in steps for c in step)
    model.engine().set_low_latency(True)


def test_event_stream_refuses_bad_identity_options_by_name():
    model = _model(B)
    for kw, name in ((dict(track=True, identity=True), "identity= needs score="), (dict(identity=True), "identity= needs score="),
                     (dict(track=True, score=True, identity=dict(max_tracks=0)), "identity max_tracks"),
                     (dict(track=True, score=True, identity=dict(max_tracks=2000)), "DAGR_ASSIGN_MAX"),
                     (dict(track=True, score=True, identity=dict(tracks=4)), "tracks"),
                     (dict(track=True, score=True, identity="yes"), "identity")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_prints_idf1_and_leaves_the_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R

    class Labelled(R.SyntheticStream):
        """The stand-in sequence with two labelled boxes at every other step."""

        def labels(self, t_step):
            if (t_step - self.t0) // 1000 % 2:
                return None
            return np.array([[10, 10, 60, 60], [100, 80, 180, 160]], np.float32), np.array([0, 1]), np.array([1, 2])

    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res", "--track", "--track_max_age_us", "2500",
            "--max_tracks", "32", "--track_min_score", "0.3", "--track_score", "--track_score_iou", "0.25"]
    paths = {}
    for name, extra in (("score", []), ("identity", ["--track_identity", "--track_identity_max_tracks", "64"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model),
                             source=Labelled(C.flags("", argv, extra=R.stream_options)))
    printed = capsys.readouterr().out
    for file in ("detections_res.npy", "tracks_res.npy"):
        with open(os.path.join(os.path.dirname(str(paths["score"])), file), "rb") as f, \
                open(os.path.join(os.path.dirname(str(paths["identity"])), file), "rb") as g:
            assert f.read() == g.read(), file              # byte for byte what they are without the flag
    assert len(re.findall(r"; scored 5 labelled steps", printed)) == 2
    said = re.findall(r"; IDF1 ([\d.]+|nan), IDP ([\d.]+|nan), IDR ([\d.]+|nan) \(IDTP (\d+) of (\d+) labelled and (\d+) tracked "
                      r"frames, (\d+) objects, (\d+) tracks\)", printed)
    assert len(said) == 1 and said[0][4] == "10" and said[0][6] == "2", printed

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")
    core = base[:-3]                                       # (without --track_score)
    for argv, text in ((["--track_identity"], "needs --track_score"),
                       (["--track_score", "--track_identity_max_tracks", "8"], "needs --track_identity"),
                       (["--track_score", "--track_identity", "--track_identity_max_tracks", "0"], "max_tracks")):
        with pytest.raises(SystemExit, match=text):
            R.main(core + argv + ["--output_directory", str(tmp_path / "no")], model_factory=refuse)
