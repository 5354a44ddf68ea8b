"""Cases of the event stream's HOTA state (dagr_amd/streaming.py: HotaDefinition; dagr_stream_hota,
dagr_stream_hota_solve) and a float restatement of HOTA, shared by the CPU and the GPU tests.  Pure numpy (and scipy, for
the float restatement only); every definition's result is computed once and shared: nobody changes what comes back.

A hand-built case is

    name, B, A, G, score, identity, hota (the options),
    steps: [the step dicts of tests/stream_score_cases.step],
    expect: dict(tp, fn, fp: per lane 19 integers, words: per lane (instants, dropped_instants, rows, columns),
                 deta, assa, hota: of the total, per threshold (a number: the same at all 19))

with the 8 x 8 boxes of tests/stream_score_cases unless a size is given."""
import numpy as np

from tests import stream_identity_cases as ic
from tests import stream_score_cases as sc

hyp, gt = sc.hyp, sc.gt
K = 19


# ------------------------------------------------------------------------------------------------ the float restatement
def _iou32(gt_box, hyp_box):
    """The fp32 IoU of every pair, TrackDefinition.iou's operations, as fp64 [n, m] (NaN stays NaN)."""
    f = np.float32
    a, b = np.asarray(gt_box, f).reshape(-1, 1, 4), np.asarray(hyp_box, f).reshape(1, -1, 4)
    with np.errstate(all="ignore"):
        iw = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        ih = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, f(0))
        union = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])) - inter
        return (inter / union).astype(np.float64)


def hota_float(logs, max_objects, max_tracks):
    """HOTA as the paper has it, in fp64, on the participants of a ``HotaDefinition``'s logs (per lane a list of instants:
    ``slot``, ``col``, ``gt_box``, ``gt_label``, ``hyp_box``, ``hyp_label``).  The similarity is the fp32 IoU, 0 across labels
    and for a NaN.  Pass 1: the similarity normalised by row sum + column sum - itself is added to the potential matches
    of the (object, track) pair; the alignment score is ``pmc / (gc + tc - pmc)``.  Pass 2: scipy's
    ``linear_sum_assignment`` maximises alignment x similarity per instant; a matched pair is a TP at ``alpha = k / 20`` when
    its similarity is ``>= alpha``.  Returns ``dict(tp, fn, fp int64 [B, 19], mc int64 [B, 19, M, T], deta, assa, loca fp64
    [B, 19] (loca NaN without a TP), pairs: per lane the number of (object, track) pairs with mc > 0 at k = 1, pairing: per
    lane per instant row -> column (-1: unmatched or a product of 0), near: the smallest distance of a positive
    similarity from a threshold)``."""
    from scipy.optimize import linear_sum_assignment
    B, M, T = len(logs), max_objects, max_tracks
    alphas = np.arange(1, K + 1, dtype=np.float64) / 20.0
    out = dict(tp=np.zeros((B, K), np.int64), fn=np.zeros((B, K), np.int64), fp=np.zeros((B, K), np.int64),
               mc=np.zeros((B, K, M, T), np.int64), deta=np.zeros((B, K)), assa=np.zeros((B, K)), loca=np.full((B, K), np.nan),
               pairs=[], pairing=[], near=np.inf)
    for b, log in enumerate(logs):
        pmc, gc, tc = np.zeros((M, T)), np.zeros(M), np.zeros(T)
        sims = []
        for e in log:
            v = _iou32(e["gt_box"], e["hyp_box"])
            same = np.asarray(e["gt_label"]).reshape(-1, 1) == np.asarray(e["hyp_label"]).reshape(1, -1)
            sim = np.where(same & (v > 0), v, 0.0)
            sims.append(sim)
            if (sim > 0).any():
                out["near"] = min(out["near"], float(np.abs(sim[sim > 0][:, None] - alphas[None, :]).min()))
            den = sim.sum(1, keepdims=True) + sim.sum(0, keepdims=True) - sim
            pmc[np.ix_(e["slot"], e["col"])] += np.where(sim > 0, sim / np.where(sim > 0, den, 1.0), 0.0)
            gc[e["slot"]] += 1
            tc[e["col"]] += 1
        with np.errstate(all="ignore"):
            align = np.where(pmc > 0, pmc / (gc[:, None] + tc[None, :] - pmc), 0.0)
        loc, lane_pairing = np.zeros(K), []
        for e, sim in zip(log, sims):
            n, m = sim.shape
            score = align[np.ix_(e["slot"], e["col"])] * sim
            rows, cols = linear_sum_assignment(score, maximize=True) if n and m else ([], [])
            row_col = np.full(n, -1, np.int64)
            tps = np.zeros(K, np.int64)
            for g, i in zip(rows, cols):
                if score[g, i] <= 0:
                    continue
                row_col[g] = i
                hit = sim[g, i] >= alphas
                tps += hit
                loc += np.where(hit, sim[g, i], 0.0)
                out["mc"][b, hit, e["slot"][g], e["col"][i]] += 1
            lane_pairing.append(row_col)
            out["tp"][b] += tps
            out["fn"][b] += n - tps
            out["fp"][b] += m - tps
        out["pairing"].append(lane_pairing)
        out["pairs"].append(int((out["mc"][b, 0] > 0).sum()))
        for k in range(K):
            tp, fn, fp = (float(out[name][b, k]) for name in ("tp", "fn", "fp"))
            ass = 0.0
            for s, c in zip(*np.nonzero(out["mc"][b, k])):
                mc = float(out["mc"][b, k, s, c])
                ass += mc * (mc / (gc[s] + tc[c] - mc))
            out["deta"][b, k] = tp / max(1.0, tp + fn + fp)
            out["assa"][b, k] = ass / max(1.0, tp)
            if tp:
                out["loca"][b, k] = loc[k] / tp
    return out


# ------------------------------------------------------------------------------------------------ the definitions' chain
def chain(B, steps, score=True, identity=True, hota=True, every=None, solve_at=()):
    """``ScoreDefinition``, ``IdentityDefinition``, then ``HotaDefinition`` over ``steps``: ``(the scorer, the identity
    definition, the HOTA definition, snapshots, solves)``, a snapshot being ``(k, tables)`` after step ``k`` for every
    ``every``-th step and the last, ``solves[k]`` the definition's solve after step ``k`` for ``k`` in ``solve_at``."""
    from dagr_amd.streaming import HotaDefinition, IdentityDefinition, ScoreDefinition
    s, d, h = ScoreDefinition(B, score), IdentityDefinition(B, identity, score), HotaDefinition(B, hota, identity, score)
    shots, solves = [], {}
    for k, q in enumerate(steps):
        match, _ = s.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"],
                          track_box=q["track_box"])
        d.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"], match, s.id,
               track_box=q["track_box"])
        h.step(q["det"], q["n_keep"], q["track_id"], q["gt_box"], q["gt_label"], q["gt_id"], q["n_gt"], match, s.id,
               d.track_id, track_box=q["track_box"])
        if (every and (k + 1) % every == 0) or k == len(steps) - 1:
            shots.append((k, tables(h)))
        if k in solve_at:
            solves[k] = h.solve()
    return s, d, h, shots, solves


def tables(h):
    """A copy of the definition's state: ``dict(pmc, gc, tc, words)``."""
    return dict(pmc=h.pmc.copy(), gc=h.gc.copy(), tc=h.tc.copy(), words={k: v.copy() for k, v in h.words.items()})


def _case(name, steps, expect, score=True, identity=True, hota=True, A=4, G=4):
    """steps: [(hyps, gts) or (hyps, gts, n_gt)] as tests/stream_score_cases._case takes them."""
    return dict(name=name, B=len(steps[0][0]), A=A, G=G, score=score, identity=identity, hota=hota,
                steps=[sc.step(s[0], s[1], A, G, n_gt=s[2] if len(s) > 2 else None) for s in steps], expect=expect)


def upto(k, v, rest=0):
    """19 integers: ``v`` at the thresholds 1 .. k, ``rest`` above."""
    return [v] * k + [rest] * (K - k)


def cases():
    nan = float("nan")
    two = [[hyp(0, 0, 5), hyp(40, 0, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]]
    first, second = ([[hyp(0, 0, 5)]], [[gt(0, 0, 1)]]), ([[hyp(0, 0, 6)]], [[gt(0, 0, 1)]])
    # boxes="track": the detections' boxes are far away, the motion model's boxes sit on the objects, the second one pixel
    # to the right: IoU 56 / 72 = 0.78, a TP up to k = 15
    moved = _case("the-motion-models-boxes", [([[hyp(100, 100, 5), hyp(140, 100, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]])],
                  dict(tp=[upto(15, 2, 1)], fn=[upto(15, 0, 1)], fp=[upto(15, 0, 1)], words=[(1, 0, 2, 2)], deta=None, assa=1.0,
                       hota=None), score=dict(boxes="track"))
    box = np.tile(np.asarray(sc.PAD_GT, np.float32), (1, 4, 1))
    box[0, 0], box[0, 1] = (0, 0, 8, 8), (41, 0, 49, 8)
    moved["steps"][0]["track_box"] = box
    return [
        moved,
        # every box sits on its object at every step: every pair is a TP at every threshold, and the alignment is whole
        _case("one-tracker-that-is-perfect-has-hota-one", [two] * 3,
              dict(tp=[upto(K, 6)], fn=[upto(K, 0)], fp=[upto(K, 0)], words=[(3, 0, 6, 6)], deta=1.0, assa=1.0, hota=1.0)),
        # one object, four steps, the track id changes half way: every step is a TP, mc = 2 for either track, gc = 4,
        # tc = 2: AssA = (2 * 2 / (4 + 2 - 2) + 2 * 2 / (4 + 2 - 2)) / 4 = 1 / 2, DetA = 1, HOTA = sqrt(1 / 2)
        _case("an-id-switch-half-way", [first] * 2 + [second] * 2,
              dict(tp=[upto(K, 4)], fn=[upto(K, 0)], fp=[upto(K, 0)], words=[(4, 0, 4, 4)], deta=1.0, assa=0.5,
                   hota=0.5 ** 0.5)),
        # [0, 0, 20, 10] against [0, 0, 10, 10]: IoU = 100 / 200 = 0.5 exactly, q = 2**19: a TP for k <= 10 and no higher
        _case("an-iou-of-exactly-one-half-is-a-tp-up-to-k-10",
              [([[hyp(0, 0, 5, w=10, h=10)]], [[gt(0, 0, 1, w=20, h=10)]])],
              dict(tp=[upto(10, 1)], fn=[upto(10, 0, 1)], fp=[upto(10, 0, 1)], words=[(1, 0, 1, 1)], deta=None, assa=None,
                   hota=None)),
        # a labelled instant without a box, then one without a hypothesis: the columns are false positives, the rows misses
        _case("an-instant-without-rows-and-one-without-columns",
              [([[hyp(0, 0, 5), hyp(40, 0, 6)]], [[]]), ([[]], [[gt(0, 0, 1)]])],
              dict(tp=[upto(K, 0)], fn=[upto(K, 1)], fp=[upto(K, 2)], words=[(2, 0, 1, 2)], deta=0.0, assa=0.0, hota=0.0)),
        _case("a-label-mismatch-is-no-similarity",
              [([[hyp(0, 0, 5, label=1)]], [[gt(0, 0, 1, label=0)]])],
              dict(tp=[upto(K, 0)], fn=[upto(K, 1)], fp=[upto(K, 1)], words=[(1, 0, 1, 1)], deta=0.0, assa=0.0, hota=0.0)),
        _case("a-nan-box-is-no-similarity",
              [([[hyp(nan, 0, 5), hyp(40, 0, 6)]], [[gt(0, 0, 1), gt(40, 0, 2)]])],
              dict(tp=[upto(K, 1)], fn=[upto(K, 1)], fp=[upto(K, 1)], words=[(1, 0, 2, 2)], deta=1 / 3, assa=1.0,
                   hota=(1 / 3) ** 0.5)),
        # lane 1 has no labels at the second step: not one word of it changes, and its log keeps one instant
        _case("a-skipped-lane-changes-nothing",
              [([[hyp(0, 0, 5)], [hyp(0, 0, 8)]], [[gt(0, 0, 1)], [gt(0, 0, 3)]]),
               ([[hyp(0, 0, 5)], [hyp(0, 0, 9)]], [[gt(0, 0, 1)], [gt(0, 0, 3)]], [1, -1])],
              dict(tp=[upto(K, 2), upto(K, 1)], fn=[upto(K, 0)] * 2, fp=[upto(K, 0)] * 2, words=[(2, 0, 2, 2), (1, 0, 1, 1)],
                   deta=1.0, assa=1.0, hota=1.0)),
        # max_instants = 2 and three steps: the third changes nothing but dropped_instants; its switch is not seen
        _case("a-full-log-leaves-the-instant-out", [first] * 2 + [second],
              dict(tp=[upto(K, 2)], fn=[upto(K, 0)], fp=[upto(K, 0)], words=[(2, 1, 2, 2)], deta=1.0, assa=1.0, hota=1.0),
              hota=dict(max_instants=2)),
        # tests/stream_identity_cases.cut_steps: 7 rows and the 12 first carriers among the first 256 rows with an id are
        # an instant's participants (lane 1: no column at the first step, 6 rows at the second); the four pairs of a step
        # have an IoU of 56 / 72, a TP up to k = 15
        dict(name="300-rows-with-ids-256-take-part-and-duplicates-in-every-register", steps=ic.cut_steps(), hota=True, **ic.CUT,
             expect=dict(tp=[upto(15, 8), upto(15, 4)], fn=[upto(15, 6, 14), upto(15, 9, 13)],
                         fp=[upto(15, 16, 24), upto(15, 8, 12)], words=[(2, 0, 14, 24), (2, 0, 13, 12)], deta=None, assa=None,
                         hota=None)),
        # G = 0: the ground-truth arrays are empty; a labelled lane logs an instant of columns, the lane beside it is skipped
        _case("no-ground-truth-arrays-at-all", [([[hyp(0, 0, 5), hyp(20, 0, 6)], [hyp(0, 0, 8)]], [[], []], [0, -1])],
              dict(tp=[upto(K, 0)] * 2, fn=[upto(K, 0)] * 2, fp=[upto(K, 2), upto(K, 0)], words=[(1, 0, 0, 2), (0, 0, 0, 0)],
                   deta=0.0, assa=0.0, hota=0.0), G=0),
    ]


_RESULTS = {}


def run_definition(case):
    """``(the HOTA definition, its solve)`` after the case's steps."""
    if case["name"] not in _RESULTS:
        _, _, h, _, _ = chain(case["B"], case["steps"], case["score"], case["identity"], case["hota"])
        _RESULTS[case["name"]] = (h, h.solve())
    return _RESULTS[case["name"]]


def check_expectation(case, words, result):
    """The written-out expectation against the lane words (name -> [B]) and a solve's ``result``."""
    from dagr_amd.streaming import HOTA_WORDS, hota_summary
    e = case["expect"]
    for b in range(case["B"]):
        for name in ("tp", "fn", "fp"):
            assert np.asarray(result[name])[b].tolist() == e[name][b], (case["name"], b, name, result[name][b])
        assert tuple(int(words[k][b]) for k in HOTA_WORDS) == tuple(e["words"][b]), (case["name"], b, words)
    total = hota_summary(result)["total"]
    for name in ("deta", "assa", "hota"):
        if e[name] is not None:
            assert np.allclose(total["alphas"][name], e[name], rtol=0, atol=1e-15), (case["name"], name, total["alphas"][name])
            assert abs(total[name] - e[name]) < 1e-15, (case["name"], name, total[name])


# ------------------------------------------------------------------------------------------------ the labelled scenes
# dagr_amd.utils.synthetic.track_scene through TrackDefinition (tests/stream_score_cases.SCENE_TRACK), the scorer, the
# identity step and HOTA.  The seeds are chosen, on the CPU, so that at EVERY instant of either variant no similarity lies
# within 2**-19 of a threshold and scipy's float pairing is the definition's (tests/test_stream_hota_cpu.py asserts both).
SCENES = {"plain": dict(seed=4, B=2, objects=6, steps=150, A=32), "both": dict(seed=4, B=2, objects=6, steps=150, A=32)}
SCENE_EVERY = 50
_SCENES, _CHAINS = {}, {}


def scene(variant):
    key = tuple(sorted(SCENES[variant].items()))
    if key not in _SCENES:
        from dagr_amd.utils.synthetic import track_scene
        _SCENES[key] = track_scene(**SCENES[variant])
    return _SCENES[key]


def scene_chain(variant):
    """The variant's scene through ``TrackDefinition`` (plain, or ``motion=`` + ``rescue=``), ``ScoreDefinition``,
    ``IdentityDefinition`` and ``HotaDefinition``: ``(the HOTA definition, snapshots every SCENE_EVERY steps and at the end,
    its solve, the pairings of the solve)``."""
    if variant not in _CHAINS:
        from dagr_amd.streaming import TrackDefinition
        _, motion, rescue = next(v for v in sc.VARIANTS if v[0] == variant)
        trk, steps = TrackDefinition(SCENES[variant]["B"], sc.SCENE_TRACK, motion=motion, rescue=rescue), []
        for s in scene(variant):
            ids, _ = trk.step(s["det"], s["n_keep"], s["t_ref"])
            steps.append(dict(s, track_id=ids.copy(), track_box=None))
        _, _, h, shots, _ = chain(SCENES[variant]["B"], steps, every=SCENE_EVERY)
        pairings = []
        _CHAINS[variant] = (h, shots, h.solve(pairings), pairings)
    return _CHAINS[variant]


# more than 64 participants on either side (a thread's second register in the solve), more rows than columns at one
# instant and the reverse at another, boxes that reach their neighbours' so that the assignment has to choose
WIDE = dict(B=1, A=100, G=96, steps=((90, 70), (66, 100), (80, 80)), score=dict(max_objects=128), identity=dict(max_tracks=128),
            hota=dict(max_instants=3))
_WIDE = []


def wide():
    """Three steps of 8 x 8 boxes every 6 pixels on a grid (a neighbour's IoU is 1 / 7), ``(rows, hypotheses)`` = (90, 70),
    (66, 100), (80, 80): hypothesis ``j`` sits on a random object, 0..2 pixels to the right, under the object's own track id
    (so the alignment builds up), in a random row.  Returns ``(steps, the HOTA definition, snapshots, its solve)``."""
    if not _WIDE:
        c, rng = WIDE, np.random.Generator(np.random.PCG64(23))
        A, G, steps = c["A"], c["G"], []
        x, y = 6.0 * (np.arange(A) % 12), 6.0 * (np.arange(A) // 12)
        place = np.stack([x, y, x + 8, y + 8], -1).astype(np.float32)
        for ng, nh in c["steps"]:
            det, ids = np.zeros((1, A, 6), np.float32), np.zeros((1, A), np.int64)
            on, rows = rng.permutation(A)[:nh], np.sort(rng.permutation(A)[:nh])
            shift = rng.integers(0, 3, (nh, 1)).astype(np.float32)
            det[0, rows, :4] = place[on] + shift * np.array([1, 0, 1, 0], np.float32)
            det[0, rows, 4] = 0.9
            ids[0, rows] = 500 + on
            steps.append(dict(det=det, n_keep=np.full(1, A, np.int32), track_id=ids, track_box=None, gt_box=place[None, :G].copy(),
                              gt_label=np.zeros((1, G), np.int32), gt_id=1 + np.arange(G, dtype=np.int64)[None],
                              n_gt=np.array([ng], np.int32)))
        _, _, h, shots, _ = chain(1, steps, c["score"], c["identity"], c["hota"], every=1)
        _WIDE.append((steps, h, shots, h.solve()))
    return _WIDE[0]


# the scene that crosses the boundaries: tests/stream_identity_cases.CROSSING with a log of four instants
CROSSING = dict(ic.CROSSING, hota=dict(max_instants=4), solve_at=(2, 7, 11))
_CROSSING = []


def crossing():
    """The steps of ``tests/stream_identity_cases.crossing`` (B = 2, A = 80, G = 70, max_objects = 16, max_tracks = 8, 12
    steps, lane 1 skipped at step 5) with ``max_instants = 4``: the log fills at step 3 and 8 instants of lane 0 are
    dropped.  Returns ``(steps, the HOTA definition, snapshots after every step, the solves after the steps of solve_at)``."""
    if not _CROSSING:
        c = CROSSING
        steps = ic.crossing()[0]
        _, _, h, shots, solves = chain(c["B"], steps, c["score"], c["identity"], c["hota"], every=1, solve_at=c["solve_at"])
        _CROSSING.append((steps, h, shots, solves))
    return _CROSSING[0]
