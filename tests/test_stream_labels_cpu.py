"""The event stream's label store without a GPU: LabelDefinition (dagr_amd/streaming.py) against the reference's own
interpolate_tracks output (tests/golden/ref_py_data.npz), against dagr_amd.data.dsec_data.interpolate_tracks and
dsec_utils.filter_small_bboxes bit for bit, and on the written-out cases of tests/stream_labels_cases.py; the options'
refusals; the header's declarations."""
import ctypes
import os

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.data.dsec_data import interpolate_tracks
from dagr_amd.data.dsec_utils import filter_small_bboxes
from dagr_amd.streaming import LabelDefinition, labels_from_tracks
from tests import stream_labels_cases as lc

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_py_data.npz"), allow_pickle=True)


def _pair(f0, f1, **labels):
    d = LabelDefinition(1, dict(max_keyframes=2, max_rows=64, **labels))
    assert d.push(0, *labels_from_tracks(f0)) and d.push(0, *labels_from_tracks(f1))
    return d


def test_the_definition_reproduces_the_references_own_output():
    """interp_f0 / interp_f1 at t0 + 20000 (r = 0.4): x, y, w, h bit for bit what the reference's interpolate_tracks wrote;
    the golden holds track id 0, which labels_from_tracks moves to 1."""
    f0, f1, want = GOLDEN["interp_f0"], GOLDEN["interp_f1"], GOLDEN["interp_out"]
    assert 0 in f0["track_id"] and list(f0["track_id"]) != sorted(f0["track_id"])
    t = int(f0["t"][0]) + 20000
    d = _pair(f0, f1)
    what, xywh, label, ids = d.rows_at(0, t)
    assert what == "labelled" and xywh.dtype == np.float64
    assert np.array_equal(ids, want["track_id"].astype(np.int64) + 1) and ids.min() == 1
    assert np.array_equal(label, want["class_id"].astype(np.int32))
    for k, name in enumerate("xywh"):
        assert want[name].dtype == np.float64 and xywh[:, k].tobytes() == want[name].tobytes(), name
    box, gt_label, gt_id, n_gt = d.at([t])
    n = int(n_gt[0])
    assert n == len(want) and np.array_equal(gt_id[0, :n], ids) and np.array_equal(gt_label[0, :n], label)
    assert box.dtype == np.float32 and box[0, :n].tobytes() == np.stack(
        [want["x"], want["y"], want["x"] + want["w"], want["y"] + want["h"]], axis=1).astype(np.float32).tobytes()
    assert not box[0, n:].any() and d.counters["labelled"].tolist() == [1]


def _frames(rng, n, t0, t1):
    dtype = GOLDEN["interp_f0"].dtype
    f0, f1 = np.zeros(n, dtype), np.zeros(n, dtype)
    ids = rng.choice(5000, n, replace=False)
    for f, t, order in ((f0, t0, rng.permutation(n)), (f1, t1, rng.permutation(n))):
        f["t"], f["track_id"], f["class_id"] = t, ids[order], ids[order] % 2
        for k in "xy":
            f[k] = rng.uniform(-20, 600, n)
        for k in "wh":
            f[k] = rng.uniform(0.5, 120, n)
    return f0, f1


@pytest.mark.parametrize("seed", range(6))
def test_random_pairs_equal_interpolate_tracks_bit_for_bit(seed):
    """Equal id sets in shuffled row order, odd intervals near 2**33: the rows, their order and every fp64 bit are
    dagr_amd.data.dsec_data.interpolate_tracks'."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    t0 = (1 << 33) + int(rng.integers(0, 1000))
    t1 = t0 + 2 * int(rng.integers(1, 40000)) + 1
    f0, f1 = _frames(rng, n, t0, t1)
    d = _pair(f0, f1)
    for t in (t0, t0 + 1, (t0 + t1) // 2, t1 - 1, t0 + int(rng.integers(1, t1 - t0))):
        want = interpolate_tracks(f0, f1, np.uint64(t))
        _, xywh, label, ids = d.rows_at(0, t)
        assert np.array_equal(ids, want["track_id"].astype(np.int64) + 1), t
        assert np.array_equal(label, want["class_id"].astype(np.int32)), t
        for k, name in enumerate("xywh"):
            assert xywh[:, k].tobytes() == want[name].tobytes(), (t, name)


@pytest.mark.parametrize("seed", range(3))
def test_the_small_box_filter_equals_filter_small_bboxes(seed):
    rng = np.random.default_rng(100 + seed)
    n, t0, t1 = 50, 1000, 1000 + 49999
    f0, f1 = _frames(rng, n, t0, t1)
    for f in (f0, f1):
        f["w"][:10], f["h"][:10] = rng.uniform(0, 12, 10), rng.uniform(0, 12, 10)
    t, min_height, min_diag = t0 + 12345, 6.0, 11.0
    free, small = _pair(f0, f1), _pair(f0, f1, min_height=min_height, min_diag=min_diag)
    _, xywh, _, ids = free.rows_at(0, t)
    keep = filter_small_bboxes(xywh[:, 2], xywh[:, 3], min_height, min_diag)
    assert 0 < keep.sum() < n
    _, got, _, got_ids = small.rows_at(0, t)
    assert got.tobytes() == xywh[keep].tobytes() and np.array_equal(got_ids, ids[keep])
    # w = 3, h = 4, min_diag = 5: strictly greater, so the row is dropped -- there as here
    assert not filter_small_bboxes(np.array([3.0]), np.array([4.0]), 0, 5)[0]
    edge = LabelDefinition(1, dict(min_diag=5, min_height=0))
    edge.push(0, 10, [[0, 0, 3, 4], [0, 0, 3, np.nextafter(4, 5)]], [0, 0], [1, 2])
    assert edge.rows_at(0, 10)[3].tolist() == [2]


@pytest.mark.parametrize("name", [c["name"] for c in lc.cases()])
def test_the_cases_hold_in_the_definition(name):
    """Every written-out case; the walks and the filter's edge cases run through and count what they are built to count."""
    case = next(c for c in lc.cases() if c["name"] == name)
    d = lc.run_definition(case)
    if name.startswith("walk"):
        c, R = d.counters, case["labels"]["max_rows"]
        assert c["overwritten"].tolist() == [2, 0, 0] and c["refused"].sum() == 0 and d.words()[:, 0].tolist() == [4, 3, 0]
        assert c["cut_rows"].tolist() == [sum(max(n - R, 0) for n in lc.ROWS), 0, 0]
        assert c["labelled"][0] > 0 and c["labelled"][1] > 0 and c["labelled"][2] == 0 and c["outside"].min() > 0
    if "kept" in case:
        out = d.at(case["ops"][-1][1])
        assert out[3].tolist() == [case["kept"]], (name, out[3])


def test_the_counters_and_words():
    d = LabelDefinition(2, dict(max_keyframes=2, max_rows=1))
    assert d.push(1, 5, [[0, 0, 1, 1], [1, 1, 1, 1]], [0, 0], [1, 2]) and not d.push(1, 5, [[0, 0, 1, 1]], [0], [1])
    assert d.push(1, 6, np.zeros((0, 4)), [], []) and d.push(1, 7, [[0, 0, 1, 1]], [0], [1])
    assert d.words().tolist() == [[0] * 8, [2, 1, 1, 1, 1, 0, 0, 0]] and S.LABEL_WORDS[2:] == S.LABEL_COUNTERS
    box, label, ids, n = d.at([0, 6])
    assert n.tolist() == [-1, 0] and d.counters["outside"].tolist() == [1, 0] and d.counters["labelled"].tolist() == [0, 1]
    d.reset()
    assert not d.words().any()


def test_labels_from_tracks_and_bad_options():
    f0 = GOLDEN["interp_f0"]
    t, xywh, label, ids = labels_from_tracks(f0)
    assert isinstance(t, int) and t == int(f0["t"][0]) and xywh.dtype == np.float64 and xywh.shape == (len(f0), 4)
    assert label.dtype == np.int32 and ids.dtype == np.int64 and np.array_equal(ids, f0["track_id"].astype(np.int64) + 1)
    assert np.array_equal(xywh[:, 2], f0["w"]) and np.array_equal(xywh[:, 3], f0["h"]) and "+ 1" in labels_from_tracks.__doc__
    with pytest.raises(ValueError, match="empty frame"):
        labels_from_tracks(f0[:0])
    for labels, said in ((dict(max_keyframes=0), "max_keyframes"), (dict(max_keyframes=65536), "max_keyframes"),
                         (dict(max_rows=0), "max_rows"), (dict(max_rows=257), "DAGR_SCORE_MAX_GT"), (dict(max_gap_us=0), "max_gap_us"),
                         (dict(max_gap_us=1.5), "max_gap_us"), (dict(min_height="tall"), "min_height"),
                         (dict(min_diag=float("nan")), "min_diag"), (dict(rows=3), "rows"), ("yes", "labels")):
        with pytest.raises(ValueError, match=said):
            LabelDefinition(1, labels)
    with pytest.raises(ValueError, match="keeps no labels"):
        LabelDefinition(1, None)
    assert LabelDefinition(1).options == S.LABEL_DEFAULTS == dict(max_keyframes=1200, max_rows=64, max_gap_us=None,
                                                                  min_height=None, min_diag=None)


def test_the_header_declares_the_four_entries():
    sig, v, i32, i64, f64 = _lib.SIGNATURES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert sig["dagr_stream_labels_bytes"] == (ctypes.c_size_t, [i32, i32, i32])
    assert sig["dagr_stream_labels_reset"] == (ctypes.c_int, [v, ctypes.c_size_t, i32, i32, i32, v])
    assert sig["dagr_stream_labels_push"] == (ctypes.c_int, [v, ctypes.c_size_t, i32, i32, i32, i32, v, v, v, v, v, v])
    assert sig["dagr_stream_labels_at"] == (ctypes.c_int, [v, ctypes.c_size_t, i32, i32, i32, v, i64, f64, f64, v, v, v, v, v])
    assert _lib.DEFINES["DAGR_LABELS_WORDS"] == len(S.LABEL_WORDS) == 8
