"""The event stream's mAP log in numpy (dagr_amd/streaming.py: MapDefinition) and the options of EventStream(map=): the
image list and its counters under the log's rules, the metrics against evaluate_detection on the same lists, the scene of
the GPU suite's metrics test, and the refusals by name.  No GPU."""
import numpy as np
import pytest

from dagr_amd import streaming as S
from dagr_amd.streaming import EventStream, MapDefinition
from dagr_amd.utils import coco_eval as CE
from tests import stream_map_cases as mc


def test_the_image_list_is_lane_major_and_obeys_the_log_rules():
    """B = 3, max_images = 5 overflowed by two steps, max_dets = 5 under A = 8, a lane without labels, one with none, one
    without detections: every lane keeps its first five images with n_gt > 0 in step order, an image its first
    min(n_keep, 5) rows, and the counters say what went where."""
    scene = mc.log_cases()[1]
    d = mc.run_definition(scene)
    B, steps = scene["B"], scene["steps"]
    want = {name: np.zeros(B, np.int64) for name in S.MAP_WORDS}
    images = [[] for _ in range(B)]
    for s in steps:
        for b in range(B):
            if s["n_gt"][b] < 0:
                want["unlabelled"][b] += 1
            elif s["n_gt"][b] == 0:
                want["empty"][b] += 1
            elif len(images[b]) == 5:
                want["dropped_images"][b] += 1
            else:
                want["cut_dets"][b] += max(int(s["n_keep"][b]) - 5, 0)
                images[b].append((int(s["t_ref"][b]), s["gt_box"][b, :s["n_gt"][b]], s["det"][b, :min(int(s["n_keep"][b]), 5)]))
    want["images"] = np.array([len(v) for v in images], np.int64)
    assert want["dropped_images"].tolist() == [2, 2, 3] and want["images"].tolist() == [5, 5, 5]
    assert want["unlabelled"].tolist() == [1, 0, 0] and want["empty"].tolist() == [0, 1, 0] and want["cut_dets"].sum() > 0
    assert np.array_equal(d.words(), np.stack([want[name] for name in S.MAP_WORDS], 1))
    gt, dt = d.images()
    flat = [im for lane in images for im in lane]                   # all of lane 0's, then lane 1's, then lane 2's
    assert len(gt) == len(dt) == len(flat) == 15
    for g, v, (_, box, det) in zip(gt, dt, flat):
        assert g["boxes"].tobytes() == box.tobytes() and v["boxes"].tobytes() == det[:, :4].tobytes()
        assert v["scores"].tobytes() == det[:, 4].tobytes() and np.array_equal(v["labels"], det[:, 5].astype(np.int64))
    assert [im[0] for im in d.log[1]] == [im[0] for im in images[1]]
    assert any(len(v["boxes"]) == 0 for v in dt), "the image without detections is an image"
    # max_dets = None cuts nothing
    free = MapDefinition(B, dict(max_images=5))
    for s in steps:
        free.step(s["det"], s["n_keep"], s["gt_box"], s["gt_label"], s["n_gt"], s["t_ref"])
    assert not free.counters["cut_dets"].any() and max(len(im[3]) for lane in free.log for im in lane) == 8


def test_labels_that_are_no_class_number_belong_to_no_class():
    got = S.map_det_classes(np.array([0, 1, 2.0, -1, 0.5, np.nan, np.inf, 3e9, -0.0], np.float32))
    assert got.tolist() == [0, 1, 2, -1, -1, -1, -1, -1, 0]


@pytest.mark.parametrize("name", [c["name"] for c in mc.plan_cases()] + ["metrics"])
def test_compute_is_evaluate_detection_on_the_same_lists(name):
    scene = next(c for c in mc.plan_cases() + [mc.metrics_scene()] if c["name"] == name)
    d = mc.run_definition(scene)
    classes = tuple(f"c{i}" for i in range(scene["n_classes"]))
    got, want = d.compute(classes), CE.evaluate_detection(*d.images(), classes=classes)
    assert all(got[k] == want[k] for k in CE.OUT_KEYS), (got, want)
    assert all(np.array_equal(got[n], d.words()[:, i]) for i, n in enumerate(S.MAP_WORDS))
    if name == "empty-log":
        assert want == {k: 0 for k in CE.OUT_KEYS} and not got["images"].any()


def test_the_metrics_scene_is_not_degenerate():
    """What the GPU suite's metrics test relies on: all six numbers strictly between 0 and 1, equal scores across lanes and
    instants, and ground truth on both sides of the 32^2 and 96^2 area bounds and on them."""
    d = mc.run_definition(mc.metrics_scene())
    out = d.compute()
    assert all(0.0 < out[k] < 1.0 for k in CE.OUT_KEYS), out
    gt, dt = d.images()
    assert d.words()[:, 0].tolist() == [6, 5, 6]
    where = {}                                                      # score -> the (lane, instant)s that have it
    for (b, t), v in zip(((b, im[0]) for b, lane in enumerate(d.log) for im in lane), dt):
        for s in v["scores"].tolist():
            where.setdefault(s, set()).add((b, t))
    assert any(len({b for b, _ in w}) == 3 and len({t for _, t in w}) >= 5 for w in where.values()), where
    area = np.concatenate([(g["boxes"][:, 2] - g["boxes"][:, 0]) * (g["boxes"][:, 3] - g["boxes"][:, 1]) for g in gt])
    for bound in (32.0 ** 2, 96.0 ** 2):
        assert (area < bound).any() and (area > bound).any() and (np.abs(area - bound) < bound * 0.04).any()


def test_options_are_refused_by_name():
    for kw, name in ((dict(map=dict(max_images=0)), "max_images"), (dict(map=dict(max_images=65536)), "DAGR_MAP_MAX_IMAGES"),
                     (dict(map=dict(max_dets=0)), "max_dets"), (dict(map=dict(max_dets=4097)), "DAGR_COCO_MAX_DT"),
                     (dict(map=dict(images=3)), "images"), (dict(map="on"), "map"), (dict(map=dict(max_images=2.5)), "max_images"),
                     (dict(map=dict(max_dets=True)), "max_dets")):
        with pytest.raises(ValueError, match=name):
            EventStream(None, **kw)                                 # refused before the model is looked at
        with pytest.raises(ValueError, match=name):
            MapDefinition(2, kw["map"])
    assert S._map_options(None, "test") is None
    assert S._map_options(True, "test") == dict(max_images=1200, max_dets=None)
    assert S._map_options(dict(max_dets=100), "test") == dict(max_images=1200, max_dets=100)
    with pytest.raises(ValueError, match="keeps no mAP log"):
        MapDefinition(2, None)


def test_map_step_needs_labels_or_arrays_and_every_entry_needs_map():
    """The refusals that need no device: a stream object with its options alone."""
    stream = EventStream.__new__(EventStream)
    stream.map_options, stream.labels = S._map_options(True, "test"), None
    with pytest.raises(RuntimeError, match="labels="):
        stream.map_step()
    with pytest.raises(ValueError, match="together"):
        stream.map_step(gt_label=np.zeros((1, 2), np.int32))
    stream.map_options = None
    for call in (stream.map_step, stream.map, stream.map_counts, stream.map_log):
        with pytest.raises(RuntimeError, match="map="):
            call()
