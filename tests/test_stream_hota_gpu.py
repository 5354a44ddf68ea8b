"""The event stream's HOTA state on the GPU: dagr_stream_hota and dagr_stream_hota_solve through the binding against the
numpy definition (dagr_amd/streaming.py: HotaDefinition) -- every integer equal, the three fp64 sums per threshold to a
sum's rounding --: the hand-built cases, the tracker entries chained with the scorer, the identity step and HOTA on the
device, the scenes that cross the boundaries, a solve asked for twice and again after further steps; the refusals;
EventStream(hota=) end to end in latency and in throughput mode, and its library calls; scripts/run_stream.py --track_hota."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, HotaDefinition, IdentityDefinition, ScoreDefinition
from tests import stream_hota_cases as hc
from tests import stream_score_cases as sc
from tests.test_stream_identity_gpu import _d, _Identity
from tests.test_stream_rescue_gpu import _Tracker as _RescueTracker
from tests.test_stream_rescue_gpu import _events, _step
from tests.test_stream_score_gpu import TRACK, WINDOW_US, _labels, _Scorer
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 2
K, E = 19, 512


def _sections(B_, M, T, I):
    """The state's layout as include/dagr_hip.h documents it: ``{name: (byte offset, dtype, shape)}`` and the size."""
    out, at = {}, 0
    for name, dtype, shape in (("pmc", np.int64, (B_, M, T)), ("gc", np.int64, (B_, M)), ("tc", np.int64, (B_, T)),
                               ("words", np.int64, (B_, 4)), ("count", np.int64, (B_, K, 4)), ("sums", np.float64, (B_, K, 3)),
                               ("log_box", np.float32, (B_, I, E, 4)), ("log_n", np.int32, (B_, I, 2)),
                               ("log_index", np.int32, (B_, I, E)), ("log_label", np.int32, (B_, I, E)),
                               ("mc", np.int32, (B_, K, M, T))):
        out[name] = (at, dtype, shape)
        at += -(-int(np.prod(shape)) * np.dtype(dtype).itemsize // 16) * 16
    return out, at


class _Hota:
    """dagr_stream_hota behind a scorer and an identity step (tests/test_stream_identity_gpu._Identity) on a state of its
    own; the state and the workspace start out as garbage in front of the reset."""

    def __init__(self, ident, hota):
        self.L, self.dev, self.ident, self.scorer = _lib.lib(), ident.dev, ident, ident.scorer
        self.B, self.M, self.T = ident.B, ident.M, ident.T
        self.I = S._hota_options(hota, dict(max_tracks=self.T), "test")["max_instants"]
        self.sections, want = _sections(self.B, self.M, self.T, self.I)
        self.nbytes = self.L.dagr_stream_hota_bytes(self.B, self.M, self.T, self.I)
        assert self.nbytes == want
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_hota_reset(_lib.ptr(self.state), self.nbytes, self.B, self.M, self.T, self.I,
                                                 _lib.cur_stream(self.dev)), "dagr_stream_hota_reset")
        self.ws_bytes = self.L.dagr_stream_hota_workspace_bytes(self.B, self.M, self.T, self.I)
        assert self.ws_bytes == -(-(4 * min(self.B * self.I, 256) * 2 * min(self.M, 256) * min(self.T, 256)) // 16) * 16
        self.ws = torch.full((self.ws_bytes,), 0x5a, dtype=torch.uint8, device=self.dev)

    def call(self, s, **over):
        """HOTA's step on the arrays the scorer and the identity step have just been through."""
        P, sr, idn = _lib.ptr, self.scorer, self.ident
        t = {k: _d(s[k]) for k in ("det", "n_keep", "track_id", "gt_box", "gt_label", "gt_id", "n_gt")}
        box = _d(s["track_box"]) if sr.o["boxes"] == "track" else None
        a = dict(state=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, T=self.T, I=self.I, identity=P(idn.state),
                 identity_bytes=idn.nbytes, score=P(sr.state), score_bytes=sr.nbytes, A=sr.A, G=sr.G,
                 track_box=None if box is None else P(box), gt_match=P(sr.match), **{k: P(v) for k, v in t.items()})
        a.update(over)
        rc = self.L.dagr_stream_hota(a["state"], a["bytes"], a["B"], a["M"], a["T"], a["I"], a["identity"], a["identity_bytes"],
                                     a["score"], a["score_bytes"], a["det"], a["n_keep"], a["A"], a["track_id"], a["track_box"],
                                     a["gt_box"], a["gt_label"], a["gt_id"], a["n_gt"], a["G"], a["gt_match"],
                                     _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def solve(self, **over):
        P = _lib.ptr
        a = dict(state=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, T=self.T, I=self.I, ws=P(self.ws),
                 ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.L.dagr_stream_hota_solve(a["state"], a["bytes"], a["B"], a["M"], a["T"], a["I"], a["ws"], a["ws_bytes"],
                                           _lib.cur_stream(self.dev))
        torch.cuda.synchronize()
        return rc

    def read(self, *names):
        out = {}
        for name in names:
            at, dtype, shape = self.sections[name]
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            out[name] = self.state[at:at + n].cpu().numpy().view(dtype).reshape(shape)
        return out

    def tables(self):
        """The state as tests/stream_hota_cases.tables has it."""
        t = self.read("pmc", "gc", "tc", "words")
        return dict(pmc=t["pmc"], gc=t["gc"], tc=t["tc"], words={name: t["words"][:, i] for i, name in enumerate(S.HOTA_WORDS)})

    def solved(self):
        t = self.read("count", "sums", "mc", "words")
        out = {name: t["count"][:, :, i] for i, name in enumerate(S.HOTA_COUNTERS)}
        out.update({name: t["sums"][:, :, i] for i, name in enumerate(S.HOTA_SUMS)})
        out.update({name: t["words"][:, i] for i, name in enumerate(S.HOTA_WORDS)})
        return dict(out, mc=t["mc"])


def _assert_tables(got, want, where):
    for name in ("pmc", "gc", "tc"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (where, name)
    for name in S.HOTA_WORDS:
        assert np.array_equal(got["words"][name], want["words"][name]), (where, name, got["words"][name], want["words"][name])


def _assert_result(got, want, where):
    """Every integer equal; the fp64 sums within (pairs + 2) * 2**-52 relative, pairs the (object, track) pairs with mc > 0."""
    for name in S.HOTA_COUNTERS + S.HOTA_WORDS:
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), (where, name, got[name], want[name])
    if "mc" in got:
        assert got["mc"].dtype == np.int32 and np.array_equal(got["mc"], want["mc"]), (where, "mc")
    pairs = (want["mc"] > 0).sum((2, 3))
    for name in S.HOTA_SUMS:
        assert got[name].dtype == np.float64
        assert np.all(np.abs(got[name] - want[name]) <= (pairs + 2) * 2.0 ** -52 * want[name]), (where, name, got[name], want[name])


def _assert_solve(hota, want, where):
    _lib.check(hota.solve(), "dagr_stream_hota_solve")
    got = hota.solved()
    _assert_result(got, want, where)
    return got


def _run(B_, A, G_, steps, score, identity, hota, shots, where, solves=None):
    """Scorer, identity step, then HOTA's step on the device for every step; the tables equal the definition's snapshots
    and a solve asked for after a step of ``solves`` gives the definition's."""
    scorer = _Scorer(B_, A, G_, score)
    ident = _Identity(scorer, identity)
    dev = _Hota(ident, hota)
    shots = dict(shots)
    for k, s in enumerate(steps):
        _lib.check(scorer.call(s), "dagr_stream_score")
        _lib.check(ident.call(s), "dagr_stream_identity")
        _lib.check(dev.call(s), "dagr_stream_hota")
        if k in shots:
            _assert_tables(dev.tables(), shots[k], (where, k))
        if solves and k in solves:
            _assert_solve(dev, solves[k], (where, "solve after step", k))
    return dev


@pytest.mark.parametrize("name", [c["name"] for c in hc.cases()])
def test_the_hand_built_cases_equal_the_definition_and_their_numbers(name):
    case = next(c for c in hc.cases() if c["name"] == name)
    h, want = hc.run_definition(case)
    dev = _run(case["B"], case["A"], case["G"], case["steps"], case["score"], case["identity"], case["hota"],
               [(len(case["steps"]) - 1, hc.tables(h))], name)
    got = _assert_solve(dev, want, name)
    hc.check_expectation(case, dev.tables()["words"], got)


@pytest.mark.parametrize("variant", sorted(hc.SCENES))
def test_the_tracker_entries_chained_with_the_scorer_the_identity_step_and_hota_on_the_device(variant):
    """150 steps of the labelled scene, B = 2, 6 objects, A = 32: dagr_stream_track or dagr_stream_track_cv_rescue, then
    dagr_stream_score, dagr_stream_identity and dagr_stream_hota on what they left on the device.  After every 50th step
    the tables equal the definitions' chain; the solve over the 300 logged instants gives the definition's integers."""
    _, motion, rescue = next(v for v in sc.VARIANTS if v[0] == variant)
    h, shots, want, _ = hc.scene_chain(variant)
    shots = dict(shots)
    c = hc.SCENES[variant]
    if rescue:
        tr = _RescueTracker(c["B"], c["A"], sc.SCENE_TRACK, motion, rescue)
        ids, entry = tr.out["ids"], tr.family + "_rescue"
    else:
        tr = _PlainTracker(c["B"], c["A"], sc.SCENE_TRACK)
        ids, entry = tr.ids, "dagr_stream_track"
    scorer = _Scorer(c["B"], c["A"], c["objects"], True)
    ident = _Identity(scorer, True)
    dev = _Hota(ident, True)
    for k, s in enumerate(hc.scene(variant)):
        _lib.check(tr.call(s), entry)
        q = dict(s, track_id=ids, track_box=None)
        _lib.check(scorer.call(q), "dagr_stream_score")
        _lib.check(ident.call(q), "dagr_stream_identity")
        _lib.check(dev.call(q), "dagr_stream_hota")
        if k in shots:
            _assert_tables(dev.tables(), shots[k], (variant, k))
    assert len(shots) == 3 and h.events["matched"] > 0 and h.events["tall"] > 0 and h.events["wide"] > 0
    got = _assert_solve(dev, want, variant)
    print(variant, {k: round(v, 4) for k, v in S.hota_summary(got)["total"].items() if isinstance(v, float)})


def test_the_scene_that_crosses_the_boundaries():
    """B = 2, A = 80, G = 70 (a thread's second register in the step), max_objects = 16 and max_tracks = 8 (rows and
    hypotheses go without a slot or a column), max_instants = 4 over 12 steps (the log fills, 8 and 7 instants are
    dropped), lane 1 skipped once: the tables equal the definition's after every step, and a solve after the steps 2, 7
    and 11 -- a log that is not full, a full one, the same one again -- gives the definition's each time; asked for twice
    in a row it gives the same bytes."""
    c = hc.CROSSING
    steps, h, shots, solves = hc.crossing()
    dev = _run(c["B"], c["A"], c["G"], steps, c["score"], c["identity"], c["hota"], shots, "crossing", solves)
    assert dev.tables()["words"]["dropped_instants"].tolist() == [8, 7] and h.events["dropped"] == 15
    before = dev.state.clone()
    _assert_solve(dev, solves[c["solve_at"][-1]], "crossing, again")
    assert torch.equal(dev.state, before)


def test_more_than_64_rows_and_columns_in_both_orientations():
    """90 x 70, 66 x 100 and 80 x 80 participants on boxes that reach their neighbours': a thread's second register in the
    solve, assign_wave transposed and not."""
    c = hc.WIDE
    steps, h, shots, want = hc.wide()
    dev = _run(c["B"], c["A"], c["G"], steps, c["score"], c["identity"], c["hota"], shots, "wide")
    assert h.events["tall"] > 0 and h.events["wide"] > 0
    _assert_solve(dev, want, "wide")


def test_argument_errors_launch_nothing():
    case = next(c for c in hc.cases() if c["name"].startswith("a-skipped-lane"))
    h, want = hc.run_definition(case)
    dev = _run(case["B"], case["A"], case["G"], case["steps"], case["score"], case["identity"], case["hota"], [], "errors")
    _assert_solve(dev, want, "errors")
    s = case["steps"][-1]
    watched = (dev.state, dev.ws, dev.ident.state, dev.scorer.state)
    before = [t.clone() for t in watched]
    bad, L = _lib.ENUMS["DAGR_ERR_INVALID_ARG"], dev.L
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    refusals = [(dict(state=None), b"NULL"), (dict(identity=None), b"NULL"), (dict(score=None), b"NULL"),
                (dict(n_keep=None), b"NULL"), (dict(n_gt=None), b"NULL"), (dict(det=None), b"NULL"),
                (dict(track_id=None), b"NULL"), (dict(gt_box=None), b"NULL ground truth"),
                (dict(gt_id=None), b"NULL ground truth"), (dict(gt_label=None), b"NULL ground truth"),
                (dict(gt_match=None), b"NULL ground truth"), (dict(bytes=dev.nbytes - 1), b"dagr_stream_hota_bytes"),
                (dict(identity_bytes=dev.ident.nbytes - 1), b"dagr_stream_identity_bytes"),
                (dict(score_bytes=dev.scorer.nbytes - 1), b"dagr_stream_score_bytes"), (dict(B=0), b"out of range"),
                (dict(B=65536), b"out of range"), (dict(M=0), b"max_objects"), (dict(M=1025), b"max_objects"),
                (dict(T=0), b"max_tracks"), (dict(T=1025), b"max_tracks"), (dict(I=0), b"max_instants"),
                (dict(I=65536), b"max_instants"), (dict(G=-1), b"G out of range"), (dict(G=257), b"G out of range"),
                (dict(A=-1), b"A out of range"), (dict(state=odd(dev.state, 8)), b"aligned"),
                (dict(identity=odd(dev.ident.state, 8)), b"aligned"), (dict(score=odd(dev.scorer.state, 8)), b"aligned"),
                (dict(gt_match=odd(dev.scorer.match, 4)), b"aligned"), (dict(track_box=odd(dev.state, 8)), b"aligned")]
    for over, text in refusals:
        assert dev.call(s, **over) == bad, over
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_hota:"), (over, said)
    for over, text in [(dict(state=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(bytes=dev.nbytes - 1), b"dagr_stream_hota_bytes"),
                       (dict(ws_bytes=dev.ws_bytes - 1), b"dagr_stream_hota_workspace_bytes"), (dict(B=0), b"out of range"),
                       (dict(T=1025), b"max_tracks"), (dict(I=0), b"max_instants"), (dict(ws=odd(dev.ws, 8)), b"aligned"),
                       (dict(state=odd(dev.state, 8)), b"aligned")]:
        assert dev.solve(**over) == bad, over
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_hota_solve:"), (over, said)
    for sizes in ((0, 4, 4, 4), (65536, 4, 4, 4), (1, 0, 4, 4), (1, 1025, 4, 4), (1, 4, 0, 4), (1, 4, 1025, 4), (1, 4, 4, 0),
                  (1, 4, 4, 65536)):
        assert L.dagr_stream_hota_bytes(*sizes) == 0 and L.dagr_stream_hota_workspace_bytes(*sizes) == 0, sizes
    assert L.dagr_stream_hota_bytes(1, 1024, 1024, 65535) == _sections(1, 1024, 1024, 65535)[1]
    assert L.dagr_stream_hota_reset(_lib.ptr(dev.state), dev.nbytes - 1, dev.B, dev.M, dev.T, dev.I, _lib.cur_stream(dev.dev)) == bad
    assert L.dagr_stream_hota_reset(None, dev.nbytes, dev.B, dev.M, dev.T, dev.I, _lib.cur_stream(dev.dev)) == bad
    torch.cuda.synchronize()
    for t, was in zip(watched, before):
        assert torch.equal(t, was)
    _assert_tables(dev.tables(), hc.tables(h), "after the refusals")


# ------------------------------------------------------------------------------------------------ the stream, end to end
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_hota_stream_changes_nothing_else_and_equals_the_definitions(latency, monkeypatch):
    """B = 2, twelve steps, a score_step on every third, max_instants = 3 (the fourth labelled instant of lane 0 is left
    out).  A stream with hota= returns bit-identical detections, track ids, gt_match, track_score() and identity() to the
    same stream without it; its score_step is exactly dagr_stream_score, dagr_stream_identity, dagr_stream_hota, and the
    stream without hota= records what it records today; hota() -- asked for half way, at the end and once more -- and
    hota_tables() equal a HotaDefinition fed the read-back arrays; reset() empties the state."""
    model = _model(B)
    eng = model.engine()
    eng.set_low_latency(latency)
    score, identity, hota = dict(iou=0.5, max_objects=16), dict(max_tracks=24), dict(max_instants=3)
    plain = EventStream(model, window_us=WINDOW_US, track=TRACK, score=score, identity=identity)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, score=score, identity=identity, hota=hota)
    assert stream.hota_options == hota and plain.hota_options is None and plain.state.hota_state is None
    assert stream.state.hota_state.numel() == _lib.lib().dagr_stream_hota_bytes(B, 16, 24, 3)
    sd, d, h = ScoreDefinition(B, score), IdentityDefinition(B, identity, score), HotaDefinition(B, hota, identity, score)
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
                h.step(det, nk, ids, *lab, match, sd.id, d.track_id)
                if k == 6:                                         # a solve half way: the log and the tables go on
                    _assert_result(stream.hota(), h.solve(), ("stream, half way", rnd))
            assert seen["with"] == [["dagr_stream_score", "dagr_stream_identity", "dagr_stream_hota"]] * len(seen["with"])
            assert seen["without"] == [["dagr_stream_score", "dagr_stream_identity"]] * len(seen["without"])
            a, b = stream.track_score(), plain.track_score()
            assert all(np.array_equal(a[name], b[name]) for name in S.SCORE_COUNTERS)
            a, b = stream.identity(), plain.identity()
            assert all(np.array_equal(a[name], b[name]) for name in S.IDENTITY_RESULT)
            want = h.solve()
            for again in range(2):
                del calls[:]
                got = stream.hota()
                assert list(calls) == ["dagr_stream_hota_solve"]
                _assert_result(got, want, ("stream", rnd, again))
            t = stream.hota_tables()
            _assert_tables(t, hc.tables(h), ("stream", rnd))
            assert t["mc"].dtype == np.int32 and np.array_equal(t["mc"], want["mc"])
            print("round", rnd, S.hota_summary(got)["total"]["hota"], h.events)
            assert got["tp"].sum() > 0 and got["dropped_instants"].sum() > 0 and h.events["dropped"] > 0
            stream.reset()
            plain.reset()
            t = stream.hota_tables()
            assert not any(t[name].any() for name in ("pmc", "gc", "tc")) and not any(v.any() for v in t["words"].values())
            got = stream.hota()
            assert not any(got[name].any() for name in S.HOTA_COUNTERS + S.HOTA_SUMS + S.HOTA_WORDS)
            assert not stream.hota_tables()["mc"].any()
            sd.reset()
            d.reset()
            h.reset()
            seen = {"with": [], "without": []}
        for call in (plain.hota, plain.hota_tables):
            with pytest.raises(RuntimeError, match="hota="):
                call()
    eng.set_low_latency(True)


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_hota_changes_no_step_and_a_score_step_is_three_calls(latency, monkeypatch):
    """Step for step a HOTA stream issues the library calls of the identity stream without hota=, which issues what it
    issues today; its score_step is exactly three calls, the identity stream's two; nobody else ever calls a HOTA entry."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream, scored = {}, {}
    lab = (np.zeros((B, 8, 4), np.float32), np.zeros((B, 8), np.int32), np.ones((B, 8), np.int64))
    full = dict(track=TRACK, score=True, identity=True)
    # (the first stream warms the engine up -- eager steps, the capture -- so that those after it meet the same engine)
    for name, kw in (("warm-up", dict()), ("tracking", dict(track=TRACK)), ("identity", full), ("hota", dict(full, hota=True)),
                     ("hota none", dict(full, hota=None))):
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
    assert scored["hota"] == [["dagr_stream_score", "dagr_stream_identity", "dagr_stream_hota"]] * 3
    assert scored["identity"] == scored["hota none"] == [["dagr_stream_score", "dagr_stream_identity"]] * 3
    assert per_stream["hota"] == per_stream["identity"] == per_stream["hota none"] == per_stream["tracking"]
    assert not any("hota" in c for steps in per_stream.values() for step in steps for c in step)
    model.engine().set_low_latency(True)


def test_event_stream_refuses_bad_hota_options_by_name():
    model = _model(B)
    full = dict(track=True, score=True, identity=True)
    for kw, name in ((dict(track=True, score=True, hota=True), "hota= needs identity="), (dict(hota=True), "hota= needs identity="),
                     (dict(full, hota=dict(max_instants=0)), "hota max_instants"),
                     (dict(full, hota=dict(max_instants=65536)), "DAGR_HOTA_MAX_INSTANTS"),
                     (dict(full, hota=dict(instants=4)), "instants"), (dict(full, hota="yes"), "hota"),
                     (dict(full, score=dict(max_objects=1024), identity=dict(max_tracks=1024), hota=dict(max_instants=65535)),
                      "DAGR_HOTA_MAX_STATE_BYTES")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_prints_hota_and_leaves_the_detections(tmp_path, capsys):
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
            "--max_tracks", "32", "--track_min_score", "0.3", "--track_score_iou", "0.25"]
    paths = {}
    for name, extra in (("identity", ["--track_score", "--track_identity"]), ("hota", ["--track_hota", "--track_hota_max_instants", "4"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model),
                             source=Labelled(C.flags("", argv, extra=R.stream_options)))
    printed = capsys.readouterr().out
    for file in ("detections_res.npy", "tracks_res.npy"):
        with open(os.path.join(os.path.dirname(str(paths["identity"])), file), "rb") as f, \
                open(os.path.join(os.path.dirname(str(paths["hota"])), file), "rb") as g:
            assert f.read() == g.read(), file              # byte for byte what they are without the flag
    assert len(re.findall(r"; scored 5 labelled steps", printed)) == 2 and len(re.findall(r"; IDF1 ", printed)) == 2
    said = re.findall(r"; HOTA ([\d.]+|nan), DetA ([\d.]+|nan), AssA ([\d.]+|nan), LocA ([\d.]+|nan) \((\d+) logged instants, "
                      r"(\d+) left out\)", printed)
    assert len(said) == 1 and said[0][4:] == ("4", "1"), printed

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")
    for argv, text in ((["--track_score", "--track_identity", "--track_hota_max_instants", "8"], "needs --track_hota"),
                       (["--track_hota", "--track_hota_max_instants", "0"], "max_instants")):
        with pytest.raises(SystemExit, match=text):
            R.main(base + argv + ["--output_directory", str(tmp_path / "no")], model_factory=refuse)
