"""Cases of the maximum-weight assignment and of the event stream's identity state (dagr_amd/streaming.py:
assign_max_weight_definition, IdentityDefinition; dagr_assign_max_weight, dagr_stream_identity, dagr_stream_identity_solve),
shared by the CPU and the GPU tests.  Pure numpy; every definition's result is computed once and shared: nobody changes
what comes back.

An identity case is

    name, B, A, G, score (the scorer's options), identity (the options),
    steps: [the step dicts of tests/stream_score_cases.step],
    expect: dict(overlap: per lane the table's first rows and columns, track_id: per lane the listed ids,
                 words: per lane (n_tracks, n_objects, gt_frames, hyp_frames, dup_hyp, unlisted_hyp, pairs, steps),
                 idtp: per lane, idf1: of the total)

with the 8 x 8 boxes of tests/stream_score_cases: a shift of 0, 1, 2 pixels overlaps (IoU 1, 0.78, 0.6), 3 does not."""
import numpy as np

from tests import stream_score_cases as sc

hyp, gt = sc.hyp, sc.gt


# ------------------------------------------------------------------------------------------------ the assignment
def _weights(seed, n, m, high, density=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.integers(0, high + 1, (n, m)).astype(np.int32)
    if density is not None:
        w *= (rng.random((n, m)) < density).astype(np.int32)
    return w


_MATRICES = {
    "1x1": lambda: np.array([[3]], np.int32),
    "5x7": lambda: _weights(1, 5, 7, 9),
    "7x5": lambda: _weights(2, 7, 5, 9),
    "64x64": lambda: _weights(3, 64, 64, 50),
    "65x130": lambda: _weights(4, 65, 130, 50),
    "130x65": lambda: _weights(5, 130, 65, 50),
    "all-zero-10x12": lambda: np.zeros((10, 12), np.int32),
    "constant-9x6": lambda: np.full((9, 6), 4, np.int32),
    "256x300-weights-0..2": lambda: _weights(6, 256, 300, 2),
    "1024x1024-dense": lambda: _weights(7, 1024, 1024, 1000),
    "1000x1024-sparse": lambda: _weights(8, 1000, 1024, 100, density=0.004),
    "empty-0x0": lambda: np.zeros((0, 0), np.int32),
    "empty-0x3": lambda: np.zeros((0, 3), np.int32),
    "empty-4x0": lambda: np.zeros((4, 0), np.int32),
}
SCIPY_NAMES = ("1x1", "5x7", "7x5", "65x130", "130x65", "256x300-weights-0..2", "1024x1024-dense", "1000x1024-sparse")
# three lanes of different shapes in one call, one of them empty: the per-lane strides matter
BATCHES = (("1x1", "empty-0x0", "5x7"), ("7x5", "64x64", "empty-0x3"), ("65x130", "empty-4x0", "130x65"),
           ("all-zero-10x12", "constant-9x6", "empty-0x0"), ("empty-0x0", "256x300-weights-0..2", "5x7"),
           ("1024x1024-dense", "empty-0x3", "1000x1024-sparse"))
_SOLVED = {}


def matrix(name):
    return solved(name)[0]


def solved(name):
    """``(w, total, row_col, stats)`` of a named matrix under ``assign_max_weight_definition``."""
    if name not in _SOLVED:
        from dagr_amd.streaming import assign_max_weight_definition
        w, stats = _MATRICES[name](), {}
        total, row_col = assign_max_weight_definition(w, stats)
        w.setflags(write=False)
        _SOLVED[name] = (w, total, row_col, stats)
    return _SOLVED[name]


def brute_force(w):
    """The largest sum over all one-to-one pairings, by trying every injection of the smaller side."""
    from itertools import permutations
    w = np.asarray(w, np.int64)
    if w.shape[0] > w.shape[1]:
        w = w.T
    n, m = w.shape
    return max((sum(int(w[i, c]) for i, c in enumerate(cols)) for cols in permutations(range(m), n)), default=0)


# ------------------------------------------------------------------------------------------------ the identity state
def chain(B, steps, score=True, identity=True, every=None):
    """``ScoreDefinition`` then ``IdentityDefinition`` over ``steps``: ``(the scorer, the identity definition, snapshots)``,
    a snapshot being ``(k, tables)`` after step ``k`` for every ``every``-th step and the last."""
    from dagr_amd.streaming import IdentityDefinition, ScoreDefinition
    s, d, shots = ScoreDefinition(B, score), IdentityDefinition(B, identity, score), []
    for k, q in enumerate(steps):
        match, _ = s.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"],
                          track_box=q["track_box"])
        d.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"], match, s.id,
               track_box=q["track_box"])
        if (every and (k + 1) % every == 0) or k == len(steps) - 1:
            shots.append((k, tables(d)))
    return s, d, shots


def tables(d):
    """A copy of the definition's state: ``dict(track_id, track_len, obj_len, overlap, words)``."""
    return dict(track_id=d.track_id.copy(), track_len=d.track_len.copy(), obj_len=d.obj_len.copy(), overlap=d.overlap.copy(),
                words={k: v.copy() for k, v in d.words.items()})


def _case(name, steps, expect, score=True, identity=True, A=4, G=4):
    """steps: [(hyps, gts) or (hyps, gts, n_gt)] as tests/stream_score_cases._case takes them."""
    return dict(name=name, B=len(steps[0][0]), A=A, G=G, score=score, identity=identity,
                steps=[sc.step(s[0], s[1], A, G, n_gt=s[2] if len(s) > 2 else None) for s in steps], expect=expect)


CUT = dict(B=2, A=320, G=8, score=dict(max_objects=16), identity=dict(max_tracks=16))
_CUT = []


def cut_steps():
    """Two steps of A = 320 rows on a grid of disjoint 8 x 8 boxes, 300 of them with an id (every sixteenth has none), so
    that 256 take part and 44 lie behind the cut at DAGR_TRACK_MAX_DETS.  By rank among the rows with an id: below 256 an
    even rank carries one of three ids of its own block of 64 (every register of a thread has first carriers) and an odd
    rank one of the first block's three (duplicates whose first carrier is in another register): 12 ids, 244 duplicates;
    the ranks 256 .. 279 repeat those ids (carriers behind the cut) and the ranks from 280 on carry ids of their own, which
    must not be listed although four of the 16 columns stay free.  The eight ground-truth boxes sit one pixel right of the
    rows of rank 0, 64, 130, 194 (first carriers: a pair each), 65 (a duplicate), 285 (behind the cut), 2 (without an
    identity: unscored) and 1 (the other label).  Lane 1 has ids and identities of its own; n_keep is 400 (above A) and -1
    (lane 1 has no hypotheses) at the first step, and lane 1 has six labelled rows at the second."""
    if not _CUT:
        A, G = CUT["A"], CUT["G"]
        with_id = [i for i in range(A) if i % 16 != 5]

        def ident(r):
            if r >= 280:
                return 2000 + r
            if r >= 256:
                return 1000 + r % 12
            return 1000 + r % 3 + (3 * (r // 64) if r % 2 == 0 else 0)

        def lane(first_id, first_identity):
            ids = dict((i, first_id + ident(r)) for r, i in enumerate(with_id))
            rows = [hyp(20 * (i % 20), 20 * (i // 20), ids.get(i, 0), label=i % 2) for i in range(A)]
            truth = [gt(20 * (i % 20) + 1, 20 * (i // 20), 0 if g == 6 else first_identity + g, label=(i + (g == 7)) % 2)
                     for g, i in enumerate(with_id[r] for r in (0, 64, 130, 194, 65, 285, 2, 1))]
            return rows, truth
        (rows0, truth0), (rows1, truth1) = lane(0, 1), lane(5000, 101)
        _CUT.extend([sc.step([rows0, rows1], [truth0, truth1], A, G, n_gt=[8, 8], n_keep=[400, -1]),
                     sc.step([rows0, rows1], [truth0, truth1], A, G, n_gt=[8, 6], n_keep=[A, A])])
    return _CUT


def cases():
    nan = float("nan")
    two = [[hyp(0, 0, 5), hyp(40, 0, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]]
    swapped = [[hyp(0, 0, 6), hyp(40, 0, 5)]], [[gt(0, 0, 1), gt(40, 0, 2)]]
    out = [
        # row 1 carries row 0's id: it takes no part, so object 2, which only it covers, overlaps nothing
        _case("a-duplicate-id-in-a-step",
              [([[hyp(0, 0, 5), hyp(20, 0, 5), hyp(40, 0, 6)]], [[gt(0, 0, 1), gt(20, 0, 2)]])],
              dict(overlap=[[[1, 0], [0, 0]]], track_id=[[5, 6]], words=[(2, 2, 2, 2, 1, 0, 1, 1)], idtp=[1], idf1=0.5)),
        # track 7 finds the table full: its frame is an identity false positive, object 3's an identity false negative
        _case("a-full-track-table",
              [([[hyp(0, 0, 5), hyp(20, 0, 6), hyp(40, 0, 7)]], [[gt(0, 0, 1), gt(20, 0, 2), gt(40, 0, 3)]])],
              dict(overlap=[[[1, 0], [0, 1], [0, 0]]], track_id=[[5, 6]], words=[(2, 3, 3, 3, 0, 1, 2, 1)], idtp=[2],
                   idf1=4 / 6), identity=dict(max_tracks=2)),
        # an annotation without an identity, a repeated identity and a new identity at a full object table add nothing
        _case("unscored-ground-truth-rows-add-nothing",
              [([[hyp(0, 0, 5), hyp(20, 0, 6), hyp(40, 0, 7)]], [[gt(0, 0, 1), gt(20, 0, 0), gt(0, 0, 1), gt(40, 0, 9)]])],
              dict(overlap=[[[1, 0, 0]]], track_id=[[5, 6, 7]], words=[(3, 1, 1, 3, 0, 0, 1, 1)], idtp=[1], idf1=0.5),
              score=dict(max_objects=1), identity=dict(max_tracks=3)),
        _case("a-label-mismatch-overlaps-nothing",
              [([[hyp(0, 0, 5, label=1)]], [[gt(0, 0, 1, label=0)]])],
              dict(overlap=[[[0]]], track_id=[[5]], words=[(1, 1, 1, 1, 0, 0, 0, 1)], idtp=[0], idf1=0.0)),
        _case("a-nan-box-overlaps-nothing",
              [([[hyp(nan, 0, 5), hyp(40, 0, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]])],
              dict(overlap=[[[0, 0], [0, 1]]], track_id=[[5, 6]], words=[(2, 2, 2, 2, 0, 0, 1, 1)], idtp=[1], idf1=0.5)),
        # lane 1 has no labels at the second step: not one word of it changes
        _case("a-skipped-lane-changes-nothing",
              [([[hyp(0, 0, 5)], [hyp(0, 0, 8)]], [[gt(0, 0, 1)], [gt(0, 0, 3)]]),
               ([[hyp(0, 0, 5)], [hyp(0, 0, 9)]], [[gt(0, 0, 1)], [gt(0, 0, 3)]], [1, -1])],
              dict(overlap=[[[2]], [[1]]], track_id=[[5], [8]], words=[(1, 1, 2, 2, 0, 0, 2, 2), (1, 1, 1, 1, 0, 0, 1, 1)],
                   idtp=[2, 1], idf1=1.0)),
        # both objects sit on the one hypothesis: both pairs count, one of them can be paired
        _case("two-objects-on-one-hypothesis-both-count",
              [([[hyp(0, 0, 5)]], [[gt(0, 0, 1), gt(1, 0, 2)]])],
              dict(overlap=[[[1], [1]]], track_id=[[5]], words=[(1, 2, 2, 1, 0, 0, 2, 1)], idtp=[1], idf1=2 / 3)),
        _case("a-perfect-tracker-has-idf1-one", [two] * 3,
              dict(overlap=[[[3, 0], [0, 3]]], track_id=[[5, 6]], words=[(2, 2, 6, 6, 0, 0, 6, 3)], idtp=[6], idf1=1.0)),
        # three steps, then the two tracks change places for two: either pairing keeps 3 + 3 of the 10 frames
        _case("a-tracker-that-swaps-two-ids", [two] * 3 + [swapped] * 2,
              dict(overlap=[[[3, 2], [2, 3]]], track_id=[[5, 6]], words=[(2, 2, 10, 10, 0, 0, 10, 5)], idtp=[6], idf1=0.6)),
    ]
    # boxes="track": the detections' boxes are far away, the motion model's boxes sit on the objects
    moved = _case("the-motion-models-boxes", [([[hyp(100, 100, 5), hyp(140, 100, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]])],
                  dict(overlap=[[[1, 0], [0, 1]]], track_id=[[5, 6]], words=[(2, 2, 2, 2, 0, 0, 2, 1)], idtp=[2], idf1=1.0),
                  score=dict(boxes="track"))
    box = np.tile(np.asarray(sc.PAD_GT, np.float32), (1, 4, 1))
    box[0, 0], box[0, 1] = (0, 0, 8, 8), (41, 0, 49, 8)
    moved["steps"][0]["track_box"] = box
    # cut_steps: the columns in row order of the first carriers; the four first carriers under a box overlap it at both steps
    listed = [1000, 1001, 1002, 1004, 1003, 1005, 1008, 1007, 1006, 1009, 1011, 1010]
    pairs = np.zeros((7, 12), np.int32)
    pairs[[0, 1, 2, 3], [0, 3, 7, 10]] = 1
    cut = dict(name="300-rows-with-ids-256-take-part-and-duplicates-in-every-register", steps=cut_steps(), **CUT,
               expect=dict(overlap=[(2 * pairs).tolist(), pairs.tolist()], track_id=[listed, [5000 + v for v in listed]],
                           words=[(12, 7, 14, 24, 488, 0, 8, 2), (12, 7, 13, 12, 244, 0, 4, 2)], idtp=[8, 4], idf1=24 / 63))
    # G = 0: the ground-truth arrays are empty; a labelled lane lists its tracks, the lane beside it is skipped
    empty = _case("no-ground-truth-arrays-at-all", [([[hyp(0, 0, 5), hyp(20, 0, 6)], [hyp(0, 0, 8)]], [[], []], [0, -1])],
                  dict(overlap=[[[0, 0]], [[]]], track_id=[[5, 6], []], words=[(2, 0, 0, 2, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0, 0, 0)],
                       idtp=[0, 0], idf1=0.0), G=0)
    return out + [moved, cut, empty]


_RESULTS = {}


def run_definition(case):
    """``(the scorer, the identity definition, its solve)`` after the case's steps."""
    if case["name"] not in _RESULTS:
        s, d, _ = chain(case["B"], case["steps"], case["score"], case["identity"])
        _RESULTS[case["name"]] = (s, d, d.solve())
    return _RESULTS[case["name"]]


def check_expectation(case, t, result):
    """The written-out expectation against the tables ``t`` (``tables``' layout) and a solve's ``result``."""
    from dagr_amd.streaming import IDENTITY_WORDS, identity_summary
    e = case["expect"]
    for b in range(case["B"]):
        want = np.asarray(e["overlap"][b], np.int32)
        n, m = want.shape
        assert np.array_equal(t["overlap"][b, :n, :m], want), (case["name"], b, t["overlap"][b, :n, :m])
        assert t["overlap"][b].sum() == want.sum(), (case["name"], b, "overlap outside the expected block")
        assert t["track_id"][b, :m].tolist() == e["track_id"][b] and not t["track_id"][b, m:].any(), (case["name"], b)
        assert tuple(int(t["words"][k][b]) for k in IDENTITY_WORDS) == tuple(e["words"][b]), (case["name"], b, t["words"])
        assert int(result["idtp"][b]) == e["idtp"][b], (case["name"], b, result["idtp"])
    got = identity_summary(result)["total"]["idf1"]
    assert abs(got - e["idf1"]) < 1e-12, (case["name"], got)


# the scene of the chained entries: dagr_amd.utils.synthetic.track_scene
SCENE = dict(seed=4, B=2, objects=6, steps=150, A=32)
SCENE_EVERY = 25
_SCENE, _CHAINS = [], {}


def scene():
    if not _SCENE:
        from dagr_amd.utils.synthetic import track_scene
        _SCENE.append(track_scene(**SCENE))
    return _SCENE[0]


def scene_chain(variant):
    """The scene through ``TrackDefinition`` (the variants of tests/stream_score_cases.VARIANTS), ``ScoreDefinition`` and
    ``IdentityDefinition``: ``(the identity definition, snapshots every SCENE_EVERY steps and at the end, its solve)``."""
    if variant not in _CHAINS:
        from dagr_amd.streaming import TrackDefinition
        _, motion, rescue = next(v for v in sc.VARIANTS if v[0] == variant)
        trk, steps = TrackDefinition(SCENE["B"], sc.SCENE_TRACK, motion=motion, rescue=rescue), []
        for s in scene():
            ids, _ = trk.step(s["det"], s["n_keep"], s["t_ref"])
            steps.append(dict(s, track_id=ids.copy(), track_box=None))
        _, d, shots = chain(SCENE["B"], steps, every=SCENE_EVERY)
        _CHAINS[variant] = (d, shots, d.solve())
    return _CHAINS[variant]


# the scene that crosses the boundaries: more rows than a thread's first register holds, both tables overflow
CROSSING = dict(B=2, A=80, G=70, hyps=70, steps=12, score=dict(max_objects=16, iou=0.5), identity=dict(max_tracks=8))
_CROSSING = []


def crossing():
    """12 steps of 70 ground-truth boxes on a grid, 21 of them with an identity (every eighth row and the rows from 56 on,
    so that the object table of 16 fills at row 64 and rows 65 .. 69 stay unscored), and 70 rows with ids on them (of A = 80,
    the others without an id; the boxes with an identity come first in row order), moved right by 0..2 pixels; the rows'
    ids come from a pool of 12 with repeats, so most rows are duplicates and the table of 8 overflows; every fifth row has
    the wrong label.  Lane 1 is skipped at step 5.  Returns ``(steps, the scorer, the identity definition, snapshots after every step, its solve)``."""
    if not _CROSSING:
        c, rng = CROSSING, np.random.Generator(np.random.PCG64(11))
        B, A, G = c["B"], c["A"], c["G"]
        steps = []
        for k in range(c["steps"]):
            det, ids = np.zeros((B, A, 6), np.float32), np.zeros((B, A), np.int64)
            gt_box, gt_label, gt_id = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32), np.zeros((B, G), np.int64)
            for b in range(B):
                x, y = 20.0 * (np.arange(G) % 10), 20.0 * (np.arange(G) // 10)
                gt_box[b] = np.stack([x, y, x + 8, y + 8], -1)
                gt_label[b] = np.arange(G) % 2
                gt_id[b] = np.where((np.arange(G) % 8 == 0) | (np.arange(G) >= 56), 100 * b + 1 + np.arange(G), 0)
                labelled = np.flatnonzero(gt_id[b])                          # 21 identities: 16 find a slot, rows 65 .. 69 none
                on = np.concatenate([rng.permutation(labelled), rng.permutation(np.flatnonzero(gt_id[b] == 0))])[:c["hyps"]]
                rows = np.sort(rng.permutation(A)[:c["hyps"]])               # where the rows with an id sit, in row order
                shift = rng.integers(0, 3, (c["hyps"], 1)).astype(np.float32)
                det[b, rows, :4] = gt_box[b, on] + shift * np.array([1, 0, 1, 0], np.float32)
                det[b, rows, 4] = 0.9
                det[b, rows, 5] = np.where(np.arange(c["hyps"]) % 5 == 4, 1 - gt_label[b, on], gt_label[b, on])
                ids[b, rows] = 50 + rng.integers(0, 12, c["hyps"])
            n_gt = np.array([G, -1 if k == 5 else G], np.int32)
            steps.append(dict(det=det, n_keep=np.full(B, A, np.int32), track_id=ids, track_box=None, gt_box=gt_box,
                              gt_label=gt_label, gt_id=gt_id, n_gt=n_gt))
        s, d, shots = chain(B, steps, c["score"], c["identity"], every=1)
        _CROSSING.append((steps, s, d, shots, d.solve()))
    return _CROSSING[0]
