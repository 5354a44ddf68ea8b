"""The event stream's mAP on the GPU: dagr_stream_map_log through the binding against the numpy definition
(dagr_amd/streaming.py: MapDefinition), bit for bit after every call; dagr_stream_map_plan against build_jobs / column_layout
/ accumulate_groups on the definition's images; the metrics of the whole device chain against the host evaluate_detection;
EventStream(map=) end to end with the library calls of streams with and without it; the refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, LabelDefinition, MapDefinition
from dagr_amd.utils import coco_eval as CE
from tests import stream_map_cases as mc
from tests.test_stream_rescue_gpu import _events, _step
from tests.test_stream_track_gpu import _record_calls
from tests.test_streaming_gpu import H, W, _dev, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
WINDOW_US = 20000
WORDS = len(S.MAP_WORDS)


def _sections(B_, I, G, D):
    """Where the arrays of the state lie, by the layout include/dagr_hip.h documents: ``({name: (offset, dtype, shape)},
    bytes)``."""
    out, at = {}, 0
    for name, dtype, shape in (("lane", np.int64, (B_, WORDS)), ("t", np.int64, (B_, I)), ("n_gt", np.int32, (B_, I)),
                               ("n_dt", np.int32, (B_, I)), ("gt_box", np.float32, (B_, I, G, 4)),
                               ("gt_label", np.int32, (B_, I, G)), ("det", np.float32, (B_, I, D, 6))):
        out[name] = (at, dtype, shape)
        at += -(-int(np.prod(shape)) * np.dtype(dtype).itemsize // 16) * 16
    return out, at


class _Log:
    """The entries on a state of their own; the state starts out as garbage in front of its reset."""

    def __init__(self, scene):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.G = scene["B"], scene["A"], scene["G"]
        self.I = scene["map"]["max_images"]
        self.D = scene["map"]["max_dets"] or self.A
        self.nbytes = self.L.dagr_stream_map_bytes(self.B, self.I, self.G, self.D)
        assert self.nbytes == _sections(self.B, self.I, self.G, self.D)[1]
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_map_reset(_lib.ptr(self.state), self.nbytes, self.B, self.I, self.G, self.D,
                                                _lib.cur_stream(self.dev)), "dagr_stream_map_reset")

    def log(self, step, **over):
        t = {k: _dev(np.ascontiguousarray(step[k])) for k in ("det", "n_keep", "gt_box", "gt_label", "n_gt", "t_ref")}
        a = dict(state=_lib.ptr(self.state), bytes=self.nbytes, B=self.B, I=self.I, G=self.G, D=self.D, A=self.A,
                 **{k: _lib.ptr(v) for k, v in t.items()})
        a.update(over)
        rc = self.L.dagr_stream_map_log(a["state"], a["bytes"], a["B"], a["I"], a["G"], a["D"], a["det"], a["n_keep"], a["A"],
                                        a["gt_box"], a["gt_label"], a["n_gt"], a["t_ref"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def section(self, name):
        at, dtype, shape = _sections(self.B, self.I, self.G, self.D)[0][name]
        return self.state[at:at + int(np.prod(shape)) * np.dtype(dtype).itemsize].cpu().numpy().view(dtype).reshape(shape)

    def plan(self, n_classes):
        plan = CE.StreamMapPlan(self.B, self.I, self.G, self.D, n_classes, self.dev)
        for v in (plan.gt, plan.dt, plan.scores, plan.rng):
            v.fill_(mc.SENTINEL)
        for v in (plan.jobs, plan.info, plan.col_group, plan.entry_group, plan.group_ptr, plan.totals):
            v.fill_(int(mc.SENTINEL))
        plan.workspace.fill_(0x5a)                  # its contents do not matter
        plan.run(self.state)
        return plan


def _assert_log(log, d, where):
    """Every stored row, instant, count and lane word, bit for bit."""
    words = log.section("lane")
    assert np.array_equal(words, d.words()), (where, words, d.words())
    t, n_gt, n_dt = log.section("t"), log.section("n_gt"), log.section("n_dt")
    box, label, det = log.section("gt_box"), log.section("gt_label"), log.section("det")
    for b in range(log.B):
        for k, (tk, gb, gl, dr) in enumerate(d.log[b]):
            assert (t[b, k], n_gt[b, k], n_dt[b, k]) == (tk, len(gb), len(dr)), (where, b, k)
            assert box[b, k, :len(gb)].tobytes() == gb.tobytes() and label[b, k, :len(gb)].tobytes() == gl.tobytes(), (where, b, k)
            assert det[b, k, :len(dr)].tobytes() == dr.tobytes(), (where, b, k)


@pytest.mark.parametrize("name", [c["name"] for c in mc.log_cases()])
def test_the_log_equals_the_definition_after_every_call(name):
    """B = 1 and B = 3 with G = 4, max_images = 5 overflowed by two steps, A = 8 under max_dets = 5, lanes with n_gt = -1,
    n_gt = 0 and n_keep = 0; and A = 130 rows in a lane, more than two waves' worth."""
    scene = next(c for c in mc.log_cases() if c["name"] == name)
    log = _Log(scene)

    def each(k, step, d):
        _lib.check(log.log(step), "dagr_stream_map_log")
        _assert_log(log, d, (name, k))
    d = mc.run_definition(scene, each)
    if name.startswith("overflow"):
        assert (d.words()[:, 1] >= 2).all() and d.words()[:, 2].sum() > 0
    # a reset empties it
    _lib.check(log.L.dagr_stream_map_reset(_lib.ptr(log.state), log.nbytes, log.B, log.I, log.G, log.D, _lib.cur_stream(log.dev)),
               "dagr_stream_map_reset")
    assert not log.section("lane").any()


def _logged(scene):
    log = _Log(scene)
    d = mc.run_definition(scene, lambda k, step, d_: _lib.check(log.log(step), "dagr_stream_map_log"))
    return log, d


@pytest.mark.parametrize("name", [c["name"] for c in mc.plan_cases()])
def test_the_plan_equals_the_host_job_list(name):
    """Integers equal and float64 bit-equal: gt_xywh, dt_xywh, dt_score, jobs, area_rng, group / kept / first column / first
    entry, col_group, entry_group, group_ptr and the totals -- for two and three classes, an (image, class) with detections
    only and one with ground truth only, a class nobody has, labels outside [0, n_classes), an image with 120 detections of
    one class (the MAX_DETS cut), a log that overflowed, and an empty log; what lies behind the counts stays."""
    scene = next(c for c in mc.plan_cases() if c["name"] == name)
    log, d = _logged(scene)
    want = mc.expected_plan(d, scene["n_classes"])
    plan = log.plan(scene["n_classes"])
    torch.cuda.synchronize()
    tot = plan.totals.cpu().numpy()
    assert np.array_equal(tot, want["totals"]), (tot, want["totals"])
    J, n_gt, n_dt, n_out, n_gign = (int(v) for v in tot[:5])
    if name == "wide-A130":
        assert tot[6] == 120 and want["info"][:, 1].max() == 100
    if name == "empty-log":
        assert not tot.any()
    if name == "classes-3":
        ptr = want["group_ptr"]
        assert (np.diff(ptr)[8:] == 0).all() and tot[7] > n_dt          # class 2 has no column; some rows are in no class
    for key, n in (("gt", n_gt), ("dt", n_dt), ("scores", n_dt), ("jobs", J), ("rng", J), ("info", J), ("col_group", n_out),
                   ("entry_group", n_gign), ("group_ptr", len(want["group_ptr"]))):
        got = getattr(plan, key).cpu().numpy()
        assert got[:n].dtype == want[key].dtype and got[:n].tobytes() == want[key].tobytes(), (key, got[:n], want[key])
        assert (got[n:] == (mc.SENTINEL if got.dtype == np.float64 else int(mc.SENTINEL))).all(), key


def test_map_returns_the_floats_of_the_host_evaluator():
    """The whole device chain -- log, plan, dagr_coco_match, group_ngt, score_order, dagr_coco_accumulate -- against the host
    evaluate_detection (numpy matcher and _accumulate) on MapDefinition's images: the same floats.  The scene has equal
    scores across lanes and instants and boxes on and around the 32^2 and 96^2 area bounds, and is first shown, on the
    host, to produce all six metrics strictly between 0 and 1."""
    scene = mc.metrics_scene()
    d = mc.run_definition(scene)
    want = d.compute()
    assert all(0.0 < want[k] < 1.0 for k in CE.OUT_KEYS), want
    log, _ = _logged(scene)
    plan = log.plan(scene["n_classes"])
    tot, prec, words = plan.precision(also=log.state[:8 * WORDS * log.B])
    got = CE.summarize(prec)
    print(got, want, tot)
    assert all(got[k] == want[k] for k in CE.OUT_KEYS), (got, want)
    assert np.array_equal(words.view(np.int64).reshape(log.B, WORDS), d.words())
    # the precision array itself, against the job list's host route
    host = CE._precision_from_jobs(CE.evaluated_images(*d.images()), 2, CE.match_jobs_host)
    assert prec.tobytes() == host.tobytes()


def test_argument_errors_launch_nothing(monkeypatch):
    scene = mc.log_cases()[1]
    log, _ = _logged(scene)
    step = scene["steps"][0]
    before = log.state.clone()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    calls = _record_calls(monkeypatch)
    L = log.L
    spare = torch.zeros(4096, dtype=torch.uint8, device=log.dev)
    n_log = 0
    for over, text in [(dict(G=257), b"out of range"), (dict(A=4097), b"A out of range"), (dict(D=4097), b"out of range"),
                       (dict(bytes=log.nbytes - 1), b"smaller"), (dict(gt_box=odd(spare, 8)), b"aligned"),
                       (dict(t_ref=odd(spare, 4)), b"aligned"), (dict(det=odd(spare, 2)), b"aligned"), (dict(state=None), b"NULL"),
                       (dict(det=None), b"NULL"), (dict(n_gt=None), b"NULL"), (dict(B=0), b"out of range"),
                       (dict(I=0), b"out of range"), (dict(I=65536), b"out of range"), (dict(A=0), b"A out of range"),
                       (dict(state=odd(log.state, 8)), b"aligned")]:
        assert log.log(step, **over) == bad, over
        n_log += 1
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_map_log:"), (over, said)
    for sizes in ((0, 4, 4, 4), (65536, 4, 4, 4), (1, 0, 4, 4), (1, 65536, 4, 4), (1, 4, 0, 4), (1, 4, 257, 4), (1, 4, 4, 0),
                  (1, 4, 4, 4097), (65535, 65535, 256, 4096)):
        assert L.dagr_stream_map_bytes(*sizes) == 0, sizes
    assert L.dagr_stream_map_bytes(1, 65535, 256, 1) == _sections(1, 65535, 256, 1)[1]
    assert L.dagr_stream_map_reset(_lib.ptr(log.state), log.nbytes - 1, log.B, log.I, log.G, log.D, _lib.cur_stream(log.dev)) == bad
    assert L.dagr_stream_map_reset(None, log.nbytes, log.B, log.I, log.G, log.D, _lib.cur_stream(log.dev)) == bad
    # the plan
    plan = CE.StreamMapPlan(log.B, log.I, log.G, log.D, 2, log.dev)
    torch.cuda.synchronize()
    outs = [getattr(plan, k).clone() for k in ("gt", "jobs", "totals", "group_ptr")]
    P = _lib.ptr

    def run(**over):
        a = dict(state=P(log.state), bytes=log.nbytes, B=log.B, I=log.I, G=log.G, D=log.D, C=2, rngs=P(plan.area_rngs), n_areas=4,
                 cut=100, ws=P(plan.workspace), ws_bytes=plan.workspace.numel(), gt=P(plan.gt), totals=P(plan.totals))
        a.update(over)
        return L.dagr_stream_map_plan(a["state"], a["bytes"], a["B"], a["I"], a["G"], a["D"], a["C"], a["rngs"], a["n_areas"], a["cut"],
                                      a["ws"], a["ws_bytes"], a["gt"], P(plan.dt), P(plan.scores), P(plan.jobs), P(plan.rng),
                                      P(plan.info), P(plan.col_group), P(plan.entry_group), P(plan.group_ptr), a["totals"],
                                      _lib.cur_stream(log.dev))
    n_plan = 0
    for over, text in [(dict(G=257), b"out of range"), (dict(bytes=log.nbytes - 1), b"smaller"), (dict(C=0), b"n_classes"),
                       (dict(C=257), b"n_classes"), (dict(n_areas=0), b"n_areas"), (dict(n_areas=9), b"n_areas"), (dict(cut=0), b"max_dets_per_job"),
                       (dict(cut=101), b"max_dets_per_job"), (dict(ws_bytes=plan.workspace.numel() - 1), b"workspace smaller"),
                       (dict(gt=None), b"NULL"), (dict(totals=odd(spare, 4)), b"aligned"), (dict(ws=odd(plan.workspace, 8)), b"aligned")]:
        assert run(**over) == bad, over
        n_plan += 1
        said = L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_stream_map_plan:"), (over, said)
    assert L.dagr_stream_map_plan_workspace_bytes(1, 4, 0) == 0 and L.dagr_stream_map_plan_workspace_bytes(1, 4, 257) == 0
    assert L.dagr_stream_map_plan_workspace_bytes(65535, 65535, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(log.state, before)
    assert all(torch.equal(getattr(plan, k), v) for k, v in zip(("gt", "jobs", "totals", "group_ptr"), outs))
    # every refusal came from the entry that was asked, and none of them reached another entry of the library
    assert set(calls) <= {"dagr_stream_map_log", "dagr_stream_map_bytes", "dagr_stream_map_reset", "dagr_stream_map_plan",
                          "dagr_stream_map_plan_workspace_bytes", "dagr_last_error"}
    assert calls.count("dagr_stream_map_log") == n_log and calls.count("dagr_stream_map_plan") == n_plan


# ------------------------------------------------------------------------------------------------ the stream, end to end
LABELS = dict(max_keyframes=4, max_rows=8)
STEPS = 8
_CLOCK = []


def _t_step(k):
    """_events(k)'s t_now."""
    if not _CLOCK:
        _CLOCK.append(int(np.asarray(_events(0)["t_now"]).reshape(-1)[0]))
    return _CLOCK[0] + 1000 * k


_OWN = {}


def _keyframe(k):
    """Five labelled boxes a lane at step k's instant: the first five detections a plain stream makes at that step (so that
    the logged detections meet their ground truth and the metrics are not all zero), under identities that follow the
    row; a lane with fewer rows is filled up with boxes of its own."""
    if not _OWN:
        stream = EventStream(_model(B), window_us=WINDOW_US)
        with torch.no_grad():
            for s in range(STEPS):
                det, nk = _step(stream, _events(s))
                _OWN[s] = (det.clone().cpu().numpy(), nk.clone().cpu().numpy())
    det, nk = _OWN[k]
    rows = np.array([[10, 10, 40, 30], [60, 50, 31, 33], [120, 20, 96, 96], [30, 100, 12, 50], [200, 90, 70, 60]], np.float64)
    xywh, label = np.tile(rows, (B, 1, 1)), np.tile(np.array([0, 1, 0, 1, 1], np.int32), (B, 1))
    for b in range(B):
        n = min(int(nk[b]), 5)
        box = det[b, :n, :4].astype(np.float64)
        xywh[b, :n] = np.concatenate([box[:, :2], box[:, 2:] - box[:, :2]], 1)
        label[b, :n] = det[b, :n, 5].astype(np.int32)
    return np.full(B, _t_step(k), np.int64), xywh, label, np.tile(np.arange(1, 6), (B, 1))


def test_a_stream_logged_at_every_step_equals_the_definition():
    """B = 2 on the small model, labels= and map=True: keyframes at steps 1 and 5 (lane 1 has none at 5), map_step() after
    every step -- at odd steps behind a labels_step() of the caller's --, then map() equals MapDefinition fed with the steps'
    read-back det / n_keep and LabelDefinition.at(t_ref); map_counts() and map_log() equal its words and log; a second map()
    returns the same floats; reset() empties the log; map_step(arrays) logs the caller's tensors."""
    model = _model(B)
    model.engine().set_low_latency(True)
    stream = EventStream(model, window_us=WINDOW_US, labels=LABELS, map=True)
    assert stream.map_options == dict(max_images=1200, max_dets=None) and stream.track is None and stream.score is None
    empty = stream.map()                                            # before anything was logged: zeros, and no launch
    assert all(empty[k] == 0 for k in CE.OUT_KEYS) and not any(empty[n].any() for n in S.MAP_WORDS)
    with pytest.raises(RuntimeError, match="no step"):
        stream.map_step()
    ld, md = LabelDefinition(B, LABELS), MapDefinition(B, True)
    for k in (1, 5):
        t, xywh, label, ids = _keyframe(k)
        lanes = [0, 1] if k == 1 else [0]
        stream.push_labels(t[lanes], xywh[lanes], label[lanes], ids[lanes], lanes=None if len(lanes) == B else lanes)
        for b in lanes:
            ld.push(b, t[b], xywh[b], label[b], ids[b])
    with torch.no_grad():
        for k in range(STEPS):
            det, nk = _step(stream, _events(k))
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            if k % 2:
                stream.labels_step()
            assert stream.map_step() is None
            with pytest.raises(RuntimeError, match="logged already"):
                stream.map_step()
            gt = ld.at([_t_step(k)] * B)
            md.step(det, nk, gt[0], gt[1], gt[3], [_t_step(k)] * B)
        want = md.compute()
        assert md.words()[:, 0].tolist() == [5, 1] and md.words()[:, 3].tolist() == [3, 7], md.words()
        assert want["AP"] > 0, want                                 # the keyframes are the stream's own detections
        got = stream.map()
        print(got, want)
        assert all(got[k] == want[k] for k in CE.OUT_KEYS), (got, want)
        assert all(np.array_equal(got[n], want[n]) for n in S.MAP_WORDS)
        counts, logged = stream.map_counts(), stream.map_log()
        assert all(np.array_equal(counts[n], want[n]) for n in S.MAP_WORDS)
        for b in range(B):
            assert len(logged[b]) == len(md.log[b])
            for a, w in zip(logged[b], md.log[b]):
                assert a[0] == w[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], w[1:])), b
        again = stream.map()
        assert all(again[k] == got[k] for k in CE.OUT_KEYS)
        assert stream.state.map_sizes() == (B, 1200, LABELS["max_rows"], det.shape[1])
        stream.reset()
        assert not any(v.any() for v in stream.map_counts().values()) and stream.map_log() == [[], []]
        assert stream.map()["AP"] == 0
        with pytest.raises(RuntimeError, match="no step"):
            stream.map_step()
    # the caller's tensors, on a stream without labels=
    plain = EventStream(model, window_us=WINDOW_US, map=dict(max_images=2, max_dets=3))
    pd = MapDefinition(B, plain.map_options)
    with torch.no_grad():
        for k in range(3):
            det, nk = _step(plain, _events(k))
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            box = np.tile(np.array([[5, 5, 60, 70], [100, 40, 160, 90]], np.float32), (B, 1, 1)) + k
            label, n = np.tile(np.array([0, 1], np.int32), (B, 1)), np.array([2, 1 if k else 0], np.int32)
            plain.map_step(box, label, _dev(n) if k == 1 else n)
            pd.step(det, nk, box, label, n, [_t_step(k)] * B)
        with pytest.raises(RuntimeError, match="labels="):
            _step(plain, _events(3))
            plain.map_step()
        with pytest.raises(ValueError, match="sized for 2"):
            plain.map_step(np.zeros((B, 3, 4), np.float32), np.zeros((B, 3), np.int32))
        got, want = plain.map(), pd.compute()
        assert all(got[k] == want[k] for k in CE.OUT_KEYS), (got, want)
        assert all(np.array_equal(got[n], want[n]) for n in S.MAP_WORDS) and got["dropped_images"].tolist() == [1, 0]
        assert [[im[0] for im in lane] for lane in plain.map_log()] == [[im[0] for im in lane] for lane in pd.log]


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_the_log_changes_no_step_and_only_map_step_and_map_launch(latency, monkeypatch):
    """Step for step a map= stream issues the library calls of the same stream without it, which issues what it issued
    before the log existed; map_step() is one dagr_stream_map_log behind at most one dagr_stream_labels_at (the first also
    sizes and resets the log); map() is the plan, the matcher and the accumulation."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream, logged = {}, {}
    t, xywh, label, ids = _keyframe(0)
    for name, kw in (("warm-up", dict()), ("off", dict()), ("none", dict(map=None)), ("map", dict(map=True)),
                     ("labels", dict(labels=LABELS)), ("labels map", dict(labels=LABELS, map=dict(max_images=4)))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps, logged[name] = [], []
        if stream.labels is not None:
            stream.push_labels(t, xywh, label, ids)
        with torch.no_grad():
            for k in range(4):
                del calls[:]
                _step(stream, _events(k))
                steps.append(list(calls))
                del calls[:]
                if name == "map":
                    stream.map_step(np.zeros((B, 2, 4), np.float32), np.zeros((B, 2), np.int32))
                elif name == "labels map":
                    if k == 2:
                        stream.labels_step()
                        del calls[:]
                    stream.map_step()
                logged[name].append(list(calls))
        if stream.map_options is not None:
            del calls[:]
            stream.map()
            logged[name].append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
    assert per_stream["map"] == per_stream["none"] == per_stream["off"]
    assert per_stream["labels map"] == per_stream["labels"]
    assert not any("map" in c for steps in per_stream.values() for step in steps for c in step)
    first = ["dagr_stream_map_bytes", "dagr_stream_map_reset"]
    assert logged["map"][:4] == [first + ["dagr_stream_t_ref", "dagr_stream_map_log"]] + [["dagr_stream_map_log"]] * 3
    at = ["dagr_stream_labels_at"]
    assert logged["labels map"][:4] == [["dagr_stream_t_ref"] + at + first + ["dagr_stream_map_log"], at + ["dagr_stream_map_log"],
                                        ["dagr_stream_map_log"], at + ["dagr_stream_map_log"]]
    for name in ("map", "labels map"):
        said = logged[name][4]
        assert said[:2] == ["dagr_stream_map_plan_workspace_bytes", "dagr_stream_map_plan"], said
        assert set(said[2:]) <= {"dagr_coco_match", "dagr_coco_accumulate_workspace_bytes", "dagr_coco_accumulate"}, said
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_maps_every_step_and_leaves_the_detections(tmp_path, capsys):
    """scripts/run_stream.py --map on a source with three keyframes: the nine steps between them are offered to a log of six
    images, the last line printed carries evaluate_detection's keys and the counters, the detections written are byte for
    byte what they are without the flag, and a source without keyframes is refused in front of the model."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R

    class Labelled(R.SyntheticStream):
        """The stand-in sequence with two labelled boxes at steps 2, 6 and 10, the second one moving."""

        def label_instants(self):
            return np.array([self.t0 + 1000 * k for k in (2, 6, 10)], np.int64)

        def labels(self, t_step):
            dx = (t_step - self.t0) / 1000.0
            return np.array([[10, 10, 60, 60], [100 + dx, 80, 180 + dx, 160]], np.float32), np.array([0, 1]), np.array([1, 2])

    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "12", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "res"]
    paths = {}
    for name, extra in (("plain", []), ("map", ["--map", "--map_max_images", "6"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=Labelled(C.flags("", argv, extra=R.stream_options)))
    last = capsys.readouterr().out.strip().splitlines()[-1]
    with open(paths["plain"], "rb") as f, open(paths["map"], "rb") as g:
        assert f.read() == g.read()
    said = re.fullmatch(r"AP (-?\d\.\d{4}), AP_50 (-?\d\.\d{4}), AP_75 (-?\d\.\d{4}), AP_S (-?\d\.\d{4}), AP_M (-?\d\.\d{4}), "
                        r"AP_L (-?\d\.\d{4}) over (\d+) logged steps \((\d+) dropped, (\d+) without labels, (\d+) without a box, "
                        r"(\d+) detections cut\)", last)
    assert said and said.groups()[6:] == ("6", "3", "3", "0", "0"), last

    def refuse(a_, ds, dev):
        raise AssertionError("the model is built")
    no = ["--output_directory", str(tmp_path / "no")]
    with pytest.raises(SystemExit, match="label_instants"):
        R.main(base + ["--map"] + no, model_factory=refuse, source=R.SyntheticStream(C.flags("", base, extra=R.stream_options)))
    with pytest.raises(SystemExit, match="needs --map"):
        R.main(base + ["--map_max_images", "3"] + no, model_factory=refuse)
    with pytest.raises(SystemExit, match="max_images"):
        R.main(base + ["--map", "--map_max_images", "0"] + no, model_factory=refuse)
