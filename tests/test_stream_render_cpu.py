"""The stream's picture without a GPU: RenderDefinition (dagr_amd/streaming.py) against the reference's recorded event
frames (tests/golden/ref_py_viz.npz), against hand-computed lines, plates and colour indices, its rings, and the refusals of
``render=`` by name."""
import os

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd import streaming as S
from dagr_amd.streaming import RenderDefinition, _render_options, _track_options, render_color_index, render_line, render_plate
from tests import stream_render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_py_viz.npz"))
EV_CASES = ("repeat_p01_a05", "rows_beyond_h_a05", "pm1_a05", "pm1_a03", "p01_a03", "empty")
TRACK = _track_options(True, "test")


@pytest.mark.parametrize("name", EV_CASES)
def test_the_event_layer_equals_the_references_frames(name):
    """The six recorded inputs of draw_events_on_image as one lane's in-window events, on the recorded image as base: the
    reference's output, byte for byte."""
    g = {k: GOLD[f"ev_{name}_{k}"] for k in ("img", "x", "y", "p", "alpha", "out")}
    H, W = g["img"].shape[:2]
    d = RenderDefinition(1, W, H, render=dict(alpha=float(g["alpha"]), event_window_us=10))
    t = np.full(len(g["x"]), rc.T0, np.int64)
    out = d.frames(lanes=[dict(x=g["x"], y=g["y"], t=t, p=g["p"])], t_ref=[rc.T0 + 9], base=g["img"])
    assert out.dtype == np.uint8 and np.array_equal(out[0], g["out"])
    assert d.status == 0
    if len(t):      # one microsecond older and the window has passed; no instant yet and nothing is drawn
        assert np.array_equal(d.frames(lanes=[dict(x=g["x"], y=g["y"], t=t, p=g["p"])], t_ref=[rc.T0 + 10], base=g["img"])[0],
                              g["img"])
        assert np.array_equal(d.frames(lanes=[dict(x=g["x"], y=g["y"], t=t, p=g["p"])], t_ref=[None], base=g["img"])[0], g["img"])


def test_a_polarity_without_a_channel_is_dropped_and_flagged():
    d = RenderDefinition(1, 8, 8, render=dict(alpha=0.5))
    lane = dict(x=np.array([1, 2, 3]), y=np.array([1, 1, 1]), t=np.full(3, rc.T0), p=np.array([4, -2, 3], np.int8))
    out = d.frames(lanes=[lane], t_ref=[rc.T0])
    assert d.status == 1
    assert out[0, 1, 1].tolist() == [0, 0, 0] and out[0, 1, 2].tolist() == [127, 0, 0] and out[0, 1, 3].tolist() == [0, 0, 127]


# the eight octants on a 9 x 9 image from its centre, and the point: every pixel written out by hand
LINES = {(8, 6): [(4, 4), (5, 5), (6, 5), (7, 6), (8, 6)],            # dx 4, dy 2: offsets (4k + 4) // 8 = 0, 1, 1, 2, 2
         (6, 8): [(4, 4), (5, 5), (5, 6), (6, 7), (6, 8)],
         (2, 8): [(4, 4), (3, 5), (3, 6), (2, 7), (2, 8)],
         (0, 6): [(4, 4), (3, 5), (2, 5), (1, 6), (0, 6)],
         (0, 2): [(4, 4), (3, 3), (2, 3), (1, 2), (0, 2)],
         (2, 0): [(4, 4), (3, 3), (3, 2), (2, 1), (2, 0)],
         (6, 0): [(4, 4), (5, 3), (5, 2), (6, 1), (6, 0)],
         (8, 2): [(4, 4), (5, 3), (6, 3), (7, 2), (8, 2)],
         (8, 8): [(4, 4), (5, 5), (6, 6), (7, 7), (8, 8)],            # |dx| == |dy|: x is the major axis
         (4, 4): [(4, 4)]}                                            # n = 0: the point itself


@pytest.mark.parametrize("end", list(LINES))
def test_the_line_rule_in_every_octant(end):
    assert render_line(4, 4, *end).tolist() == [list(p) for p in LINES[end]]
    d = RenderDefinition(1, 9, 9, render=dict(trail=2, ids=False), max_tracks=1)
    for k, (x, y) in enumerate([(4, 4), end]):
        d.trail_step([[5]], [[rc.T0 + k]], [[[x - 1, y - 1, x + 1.5, y + 1.5]]], [rc.T0 + k])       # centre (x.25, y.25)
    out = d.frames()
    want = np.zeros((9, 9, 3), np.uint8)
    for x, y in LINES[end]:
        want[y, x] = S.RENDER_PALETTE[1 + (5 - 1) % 31]
    assert np.array_equal(out[0], want)


def test_a_digit_plate_above_a_box_and_inside_one():
    """id 12 on a box at (3, 9): the plate is 9 x 7 at rows 2 .. 8; at ya = 6 it sits inside, rows 7 .. 13."""
    glyph = {"1": ["010", "110", "010", "010", "111"], "2": ["111", "001", "111", "100", "111"]}
    assert [format(S.RENDER_GLYPHS[int(c)], "015b") for c in "12"] == ["".join(glyph[c]) for c in "12"]
    cells = ["0" * 9] + ["0" + glyph["1"][r] + "0" + glyph["2"][r] + "0" for r in range(5)] + ["0" * 9]
    want_mask = np.array([[c == "1" for c in row] for row in cells])
    left, top, mask = render_plate(12, 3, 9, 1)
    assert (left, top) == (3, 2) and np.array_equal(mask, want_mask) and render_plate(12, 3, 6, 1)[:2] == (3, 7)
    left, top, mask = render_plate(12, 3, 9, 2)             # 9 - 14 < 0: inside, from row 10
    assert (left, top, mask.shape) == (3, 10, (14, 18)) and np.array_equal(mask[::2, ::2], want_mask)
    assert np.array_equal(mask[1::2, 1::2], want_mask)
    colors = np.array([[1, 2, 3], [10, 20, 30], [40, 50, 60]], np.uint8)
    for ya, top in ((9, 2), (6, 7)):
        d = RenderDefinition(1, 16, 16, render=dict(trail=0, colors=colors), max_tracks=1)
        det = np.array([[[3, ya, 14, ya + 5, 0.9, 0]]], np.float32)
        out = d.frames(det=det, n_keep=[1], track_id=[[12]])[0]
        c = colors[1 + (12 - 1) % 2]
        want = np.zeros((16, 16, 3), np.uint8)
        want[ya, 3:15] = want[ya + 5, 3:15] = c
        want[ya:ya + 6, 3] = want[ya:ya + 6, 14] = c
        want[top:top + 7, 3:12] = np.where(want_mask[:, :, None], 0, c)
        assert np.array_equal(out, want), ya


def test_the_colour_index():
    n = 32
    assert [render_color_index(i, n) for i in (0, 1, n - 1, n, 10 ** 6 + 7)] == [0, 1, 31, 1, 1 + (10 ** 6 + 6) % 31]
    assert render_color_index(-1, n) == 1 + (2 ** 64 - 2) % 31       # the id as an unsigned 64-bit number
    assert [render_color_index(i, 2) for i in (0, 1, 2, 99)] == [0, 1, 1, 1]
    assert len(S.RENDER_PALETTE) == 32 and len(set(S.RENDER_PALETTE)) == 32


def test_a_ring_keeps_the_last_points_and_restarts_under_a_new_id():
    d = RenderDefinition(1, 64, 64, render=dict(trail=2), max_tracks=2)
    for k in range(5):
        d.trail_step([[9, 0]], [[rc.T0 + k, 0]], [[[10 * k, 0, 10 * k + 2, 2], [0, 0, 0, 0]]], [rc.T0 + k])
    assert d.ring_count[0].tolist() == [5, 0] and d.ring_points(0, 0).tolist() == [[31, 1], [41, 1]]
    d.trail_step([[9, 0]], [[rc.T0 + 4, 0]], [[[50, 0, 52, 2], [0, 0, 0, 0]]], [rc.T0 + 5])     # coasting: nothing appended
    assert d.ring_points(0, 0).tolist() == [[31, 1], [41, 1]]
    d.trail_step([[9, 0]], [[rc.T0 + 6, 0]], [[[np.nan, 0, 52, 2], [0, 0, 0, 0]]], [rc.T0 + 6])  # not finite: not appended
    d.trail_step([[9, 0]], [[rc.NEVER, 0]], [[[50, 0, 52, 2], [0, 0, 0, 0]]], [None])            # no instant: never
    assert d.ring_count[0, 0] == 5
    d.trail_step([[11, 0]], [[rc.T0 + 7, 0]], [[[60.5, 3, 61, 4.5], [0, 0, 0, 0]]], [rc.T0 + 7])  # re-used under a new id
    assert d.ring_id[0].tolist() == [11, 0] and d.ring_points(0, 0).tolist() == [[60, 3]]
    d.trail_step([[0, 0]], [[0, 0]], np.zeros((1, 2, 4)), [rc.T0 + 8])                           # freed
    assert d.ring_id[0].tolist() == [0, 0] and d.ring_count[0].tolist() == [0, 0]
    d.trail_step([[3, 0]], [[rc.T0 + 9, 0]], [[[-3e9, 0, 0, 5e9], [0, 0, 0, 0]]], [rc.T0 + 9])   # clamped to +-2^20
    assert d.ring_points(0, 0).tolist() == [[-(1 << 20), 1 << 20]]


def test_the_scene_holds_what_it_says():
    """The shared scene draws something on every layer the GPU test compares, and the long segment raises bit 2 while the
    rest of the frame stays."""
    sc = rc.scene(37, 29, 3, 4, 2)
    d = rc.run_definition(sc, dict(trail=2))
    out = d.frames(det=sc["det"], n_keep=sc["n_keep"], track_id=sc["track_id"])
    assert d.status == 0 and out[0].any() and not out[1].any() and out[2].any()
    assert d.ring_id[0, 2] == sc["slots"][0][0][0, 2] + 1 and d.ring_count[0, 2] == 3        # re-used at step 3
    assert (out[0] == 0).all(-1)[1:7, 25:28].any()                                         # black digit pixels at ya = 0
    far = rc.scene(37, 29, 3, 4, 2, long_segment=True)
    f = rc.run_definition(far, dict(trail=2))
    got = f.frames(det=far["det"], n_keep=far["n_keep"], track_id=far["track_id"])
    assert f.status == 4
    d.ring_pt[0, 3], d.ring_count[0, 3] = 0, 0                                             # the same frame without that trail
    assert np.array_equal(got, d.frames(det=sc["det"], n_keep=sc["n_keep"], track_id=sc["track_id"]))


def test_render_options_are_refused_by_name():
    ok = _render_options(True, TRACK, "t")
    assert ok["trail"] == 32 and ok["ids"] is True and ok["alpha"] == 0.5 and ok["linewidth"] == 1 and ok["id_scale"] == 1
    assert ok["event_window_us"] is None and np.array_equal(ok["colors"], np.array(S.RENDER_PALETTE, np.uint8))
    assert _render_options(None, TRACK, "t") is None
    off = _render_options(True, None, "t")                  # without track=: no trails, no plates, class colours
    assert off["trail"] == 0 and off["ids"] is False and off["colors"].shape == (2, 3)
    assert _render_options(dict(trail=0, ids=False, alpha=1), None, "t")["alpha"] == 1.0
    for bad, word in ((dict(trail=5), "trail"), (dict(ids=True), "ids")):
        with pytest.raises(ValueError, match=f"render {word} = .* needs track="):
            _render_options(bad, None, "EventStream")
    with pytest.raises(ValueError, match="render has no option 'colour'"):
        _render_options(dict(colour=1), TRACK, "EventStream")
    with pytest.raises(ValueError, match="render = 3 must be None"):
        _render_options(3, TRACK, "EventStream")
    for key, values in (("alpha", (-0.1, 1.5, float("nan"), "x")), ("linewidth", (0, 8, 1.5)), ("trail", (-1, 65, True)),
                        ("id_scale", (0, 5)), ("event_window_us", (-1, 2.5)), ("ids", (1, None)),
                        ("colors", (np.zeros((1, 3), np.uint8), np.zeros((257, 3), np.uint8), np.zeros((4, 3), np.int32),
                                    np.zeros((4, 4), np.uint8)))):
        for v in values:
            with pytest.raises(ValueError, match=f"render {key}"):
                _render_options({key: v}, TRACK, "EventStream")
    assert (S.RENDER_MAX_TRAIL, S.RENDER_MAX_LINEWIDTH, S.RENDER_MAX_ID_SCALE) == (64, 7, 4)


def test_the_header_declares_the_entries_and_the_glyphs():
    for name in ("dagr_stream_trail_bytes", "dagr_stream_trail_reset", "dagr_stream_trail",
                 "dagr_stream_render_workspace_bytes", "dagr_stream_render"):
        assert name in _lib.SIGNATURES
    assert [_lib.ENUMS[f"DAGR_RENDER_GLYPH_{d}"] for d in range(10)] == list(S.RENDER_GLYPHS)
    assert all(0 < g < 1 << 15 for g in S.RENDER_GLYPHS) and len(set(S.RENDER_GLYPHS)) == 10
