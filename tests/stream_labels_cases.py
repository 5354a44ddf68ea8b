"""Cases of the event stream's label store (dagr_amd/streaming.py: LabelDefinition, dagr_stream_labels_push /
dagr_stream_labels_at), shared by the CPU and the GPU tests.  A case is

    name, B, labels (the options),
    ops: [("push", dict(t int64 [B, F], n int32 [B, F], xywh fp64 [B, F, R, 4], label int32 [B, F, R], id int64 [B, F, R]))
          | ("at", t_ref int64 [B])],
    expect: None, or one entry per "at" op in order: per lane None (n_gt = -1) or the rows [(id, label, x1, y1, x2, y2)],
    counters: None, or {name: per lane the final count}.

The hand cases interpolate at r = 0.25 (t0 = T0, t1 = T0 + 4, t_ref = T0 + 1) between values that are multiples of 4, so
every expected number is exact and written out.  Rows behind a keyframe's n are filled with a row that would take part
everywhere (identity 77, a large box): nothing may read them."""
import numpy as np

from dagr_amd.streaming import T_NEVER, LabelDefinition

SENTINEL = -7
T0 = 1000
PAD = (77, 9, 0.0, 0.0, 1000.0, 1000.0)


def row(ident, x, y, w, h, label=0):
    return (ident, label, float(x), float(y), float(w), float(h))


def push(R, lanes, F=None, claim=None):
    """``lanes``: per lane a list of keyframes ``(t, [row(...)])`` (an empty list: nothing for the lane); ``claim``:
    ``{(lane, f): n}``, an n other than the rows given (rows beyond ``R`` cannot be stored: they are claimed)."""
    B = len(lanes)
    F = F or max(1, max(len(lane) for lane in lanes))
    t, n = np.zeros((B, F), np.int64), np.full((B, F), -1, np.int32)
    xywh = np.tile(np.asarray(PAD[2:], np.float64), (B, F, R, 1))
    label, ident = np.full((B, F, R), PAD[1], np.int32), np.full((B, F, R), PAD[0], np.int64)
    for b, lane in enumerate(lanes):
        for f, (tf, rows) in enumerate(lane):
            t[b, f], n[b, f] = tf, len(rows)
            for g, (i, lab, *box) in enumerate(rows[:R]):
                xywh[b, f, g], label[b, f, g], ident[b, f, g] = box, lab, i
    for (b, f), v in (claim or {}).items():
        n[b, f] = v
    return "push", dict(t=t, n=n, xywh=xywh, label=label, id=ident)


def at(*t_ref):
    return "at", np.asarray(t_ref, np.int64)


def _case(name, ops, expect, counters=None, labels=None, B=1):
    return dict(name=name, B=B, labels=dict(dict(max_keyframes=8, max_rows=8), **(labels or {})), ops=ops, expect=expect,
                counters=counters)


def hand_cases():
    R = 8
    a = [row(1, 0, 4, 8, 12), row(2, 40, 40, 16, 16, label=1), row(3, 100, 100, 20, 20)]
    b = [row(3, 104, 96, 24, 16, label=1), row(2, 44, 36, 20, 12), row(4, 8, 8, 8, 8)]
    two = push(R, [[(T0, a), (T0 + 4, b)]])
    mid2 = (2, 1, 41.0, 39.0, 41.0 + 17.0, 39.0 + 15.0)              # r = 0.25: 40 -> 44, 40 -> 36, 16 -> 20, 16 -> 12
    mid3 = (3, 0, 101.0, 99.0, 101.0 + 21.0, 99.0 + 19.0)            # the label is the earlier keyframe's
    newest = [(2, 0, 44.0, 36.0, 64.0, 48.0), (3, 1, 104.0, 96.0, 128.0, 112.0), (4, 0, 8.0, 8.0, 16.0, 16.0)]
    out = [
        _case("an-identity-in-one-keyframe-only-has-no-row", [two, at(T0 + 1)], [[[mid2, mid3]]],
              dict(labelled=[1], outside=[0], gap=[0], refused=[0], cut_rows=[0], overwritten=[0])),
        _case("an-id-of-zero-or-below-takes-no-part",
              [push(R, [[(T0, [row(0, 0, 0, 8, 8), row(-3, 0, 0, 8, 8), row(5, 0, 0, 8, 8)]),
                         (T0 + 4, [row(0, 4, 4, 8, 8), row(5, 4, 8, 12, 16), row(-3, 4, 4, 8, 8)])]]), at(T0 + 1), at(T0 + 4)],
              [[[(5, 0, 1.0, 2.0, 1.0 + 9.0, 2.0 + 10.0)]], [[(5, 0, 4.0, 8.0, 16.0, 24.0)]]]),
        _case("a-duplicated-id-counts-at-its-first-row",
              [push(R, [[(T0, [row(7, 0, 0, 8, 8), row(7, 400, 400, 80, 80, label=1), row(4, 40, 40, 8, 8)]),
                         (T0 + 4, [row(4, 44, 44, 8, 8), row(7, 4, 8, 12, 16), row(7, 800, 800, 8, 8)])]]), at(T0 + 1), at(T0 + 4)],
              [[[(4, 0, 41.0, 41.0, 49.0, 49.0), (7, 0, 1.0, 2.0, 10.0, 12.0)]],
               [[(4, 0, 44.0, 44.0, 52.0, 52.0), (7, 0, 4.0, 8.0, 16.0, 24.0)]]]),
        _case("t-ref-on-a-keyframe-on-the-newest-before-after-and-never",
              [two, at(T0), at(T0 + 4), at(T0 - 1), at(T0 + 5), at(T_NEVER), at(T0 + 3)],
              [[[(2, 1, 40.0, 40.0, 56.0, 56.0), (3, 0, 100.0, 100.0, 120.0, 120.0)]], [newest], [None], [None], [None],
               [[(2, 1, 43.0, 37.0, 43.0 + 19.0, 37.0 + 13.0), (3, 0, 103.0, 97.0, 103.0 + 23.0, 97.0 + 17.0)]]],
              dict(labelled=[3], outside=[3], gap=[0])),
        _case("no-keyframe-and-one-keyframe", [at(T0), push(R, [[(T0, a)]]), at(T0), at(T0 + 1)],
              [[None], [[(1, 0, 0.0, 4.0, 8.0, 16.0), (2, 1, 40.0, 40.0, 56.0, 56.0), (3, 0, 100.0, 100.0, 120.0, 120.0)]], [None]],
              dict(labelled=[1], outside=[2])),
        _case("max-gap-exactly-at-the-interval", [two, at(T0 + 1), at(T0 + 4)], [[[mid2, mid3]], [newest]],
              dict(labelled=[2], gap=[0]), labels=dict(max_gap_us=4)),
        _case("max-gap-one-under-the-interval", [two, at(T0 + 1), at(T0), at(T0 + 4)], [[None], [None], [newest]],
              dict(labelled=[1], gap=[2], outside=[0]), labels=dict(max_gap_us=3)),
        _case("a-push-that-is-not-later-is-refused",
              [two, push(R, [[(T0 + 4, a)]]), push(R, [[(T0 + 2, a)]]), at(T0 + 4), push(R, [[(T0 + 5, a), (T0 + 5, b)]]), at(T0 + 5)],
              [[newest], [[(1, 0, 0.0, 4.0, 8.0, 16.0), (2, 1, 40.0, 40.0, 56.0, 56.0), (3, 0, 100.0, 100.0, 120.0, 120.0)]]],
              dict(refused=[3], labelled=[2], cut_rows=[0])),
        _case("rows-behind-max-rows-are-cut",
              [push(2, [[(T0, a), (T0 + 4, b)]], claim={(0, 0): 3, (0, 1): 7}), at(T0 + 1), at(T0 + 4)],
              [[[mid2]], [[(2, 0, 44.0, 36.0, 64.0, 48.0), (3, 1, 104.0, 96.0, 128.0, 112.0)]]],
              dict(cut_rows=[1 + 5], refused=[0]), labels=dict(max_rows=2)),
        _case("the-small-box-filter-is-strict",
              # w = 3, h = 4: the diagonal is 5, not greater than 5; w = 6, h = 8 passes; h = 2 fails min_height = 2
              [push(R, [[(T0, [row(1, 0, 0, 3, 4), row(2, 0, 0, 6, 8), row(3, 0, 0, 30, 2)])]]), at(T0)],
              [[[(2, 0, 0.0, 0.0, 6.0, 8.0)]]], None, labels=dict(min_diag=5, min_height=2)),
        _case("a-lane-with-nothing-is-left-alone",
              [push(R, [[(T0, a), (T0 + 4, b)], [], [(T0 + 2, b)]]), at(T0 + 1, T0 + 1, T0 + 2), push(R, [[], [(T0, a)], []]),
               at(T0 + 5, T0, T0 + 1)],
              [[[mid2, mid3], None, newest], [None, [(1, 0, 0.0, 4.0, 8.0, 16.0), (2, 1, 40.0, 40.0, 56.0, 56.0),
                                                     (3, 0, 100.0, 100.0, 120.0, 120.0)], None]],
              dict(labelled=[1, 1, 1], outside=[1, 1, 1]), B=3),
    ]
    # a ring of 4 after 6 pushes: the two oldest are gone, and a t_ref inside them is outside
    kf = [(T0 + 4 * i, [row(1, 4 * i, 0, 8, 8)]) for i in range(6)]
    out.append(_case("a-ring-of-four-after-six-pushes",
                     [push(R, [kf[:3]]), at(T0 + 1), push(R, [kf[3:]]), at(T0 + 1), at(T0 + 7), at(T0 + 8), at(T0 + 9), at(T0 + 20)],
                     [[[(1, 0, 1.0, 0.0, 9.0, 8.0)]], [None], [None], [[(1, 0, 8.0, 0.0, 16.0, 8.0)]], [[(1, 0, 9.0, 0.0, 17.0, 8.0)]],
                      [[(1, 0, 20.0, 0.0, 28.0, 8.0)]]],
                     dict(overwritten=[2], labelled=[4], outside=[2], keyframes=[4]), labels=dict(max_keyframes=4)))
    return out


def check_expectation(case, k_at, gt_box, gt_label, gt_id, n_gt):
    """The outputs after the ``k_at``-th "at" op against the case's written-out rows."""
    for b, want in enumerate(case["expect"][k_at]):
        if want is None:
            assert n_gt[b] == -1, (case["name"], k_at, b, n_gt[b])
            continue
        assert n_gt[b] == len(want), (case["name"], k_at, b, n_gt[b], want)
        for g, (ident, label, *box) in enumerate(want):
            assert gt_id[b, g] == ident and gt_label[b, g] == label, (case["name"], k_at, b, g, gt_id[b, g], gt_label[b, g])
            assert gt_box[b, g].tolist() == box, (case["name"], k_at, b, g, gt_box[b, g].tolist(), box)


def check_counters(case, counters):
    for name, want in (case["counters"] or {}).items():
        assert list(counters[name]) == want, (case["name"], name, list(counters[name]), want)


def outputs(B, R):
    """The four output arrays filled with the sentinel: what a step does not write stays."""
    return (np.full((B, R, 4), SENTINEL, np.float32), np.full((B, R), SENTINEL, np.int32), np.full((B, R), SENTINEL, np.int64),
            np.full(B, SENTINEL, np.int32))


def run_definition(case, each=None):
    """The case through ``LabelDefinition``; ``each(k, op, arg, definition, outputs)`` after every op.  Returns the
    definition."""
    d = LabelDefinition(case["B"], case["labels"])
    out = outputs(case["B"], d.options["max_rows"])
    k_at = 0
    for k, (op, arg) in enumerate(case["ops"]):
        if op == "push":
            d.push_arrays(**arg)
        else:
            d.at(arg, out=out)
            if case["expect"] is not None:
                check_expectation(case, k_at, *out)
            k_at += 1
        if each is not None:
            each(k, op, arg, d, out)
    counters = dict(d.counters, keyframes=d.words()[:, 0])
    check_counters(case, counters)
    return d


# ---- the seeded walks: what the kernels' paths need
BASE_T = 1 << 33                        # only the int64 difference of two instants is small
BASE_ID = 1 << 32                       # identities above 2**32
ROWS = (0, 1, 63, 64, 65, 256)          # rows per keyframe of lane 0: the register boundary and the cap
WALKS = [(64, 1, None), (64, 3, None), (256, 1, None), (256, 3, dict(min_height=6.0, min_diag=14.0))]


def walk(max_rows, F, small):
    """B = 3, a ring of 4: lane 0 takes six keyframes of ``ROWS`` rows (wrapping the ring), lane 1 three of a dozen rows,
    lane 2 none; ``F`` keyframes per push call.  Odd gaps between the instants, identities drawn from a pool above 2**32
    with zeros, negatives and duplicates among them, boxes of random fp64.  After every push the lanes are asked at a
    sweep of instants: on every resident keyframe, inside every interval, in front of and behind the ring."""
    rng = np.random.default_rng(1000 * max_rows + F)
    R, B = max_rows, 3
    gaps = (49999, 50001, 33333, 7, 12345)
    times = [BASE_T + int(sum(gaps[:i])) for i in range(6)]

    def keyframe(n, pool):
        ids = BASE_ID + rng.choice(pool, size=n, replace=n > pool) if n else np.zeros(0, np.int64)
        ids = ids.astype(np.int64)
        if n >= 8:                                          # annotations without an identity, and identities held twice
            ids[rng.choice(n, 3, replace=False)] = (0, -5, ids[0])
        box = np.stack([rng.uniform(0, 300, n), rng.uniform(0, 200, n), rng.uniform(1, 40, n), rng.uniform(1, 40, n)], axis=1)
        return ids, rng.integers(0, 2, n).astype(np.int32), box

    lanes = [[(times[i], keyframe(n, 300)) for i, n in enumerate(ROWS)], [(times[i] + 11, keyframe(12, 16)) for i in range(3)], []]
    ops = []
    for first in range(0, 6, F):
        t, n = np.zeros((B, F), np.int64), np.full((B, F), -1, np.int32)
        xywh = np.tile(np.asarray(PAD[2:], np.float64), (B, F, R, 1))
        label, ident = np.full((B, F, R), PAD[1], np.int32), np.full((B, F, R), PAD[0], np.int64)
        for b in range(B):
            for f, (tf, (ids, labs, box)) in enumerate(lanes[b][first:first + F]):
                m = min(len(ids), R)
                t[b, f], n[b, f] = tf, len(ids)             # (rows beyond R are claimed and cut)
                xywh[b, f, :m], label[b, f, :m], ident[b, f, :m] = box[:m], labs[:m], ids[:m]
        ops.append(("push", dict(t=t, n=n, xywh=xywh, label=label, id=ident)))
        last = min(first + F, 6) - 1
        sweep = [times[0] - 1, times[last] + 1, T_NEVER]
        for i in range(last + 1):
            sweep.append(times[i])
            if i < last:
                sweep += [times[i] + 1, (times[i] + times[i + 1]) // 2, times[i + 1] - 1]
        for s in sweep:
            ops.append(at(s, s if s == T_NEVER else s + 11, s))
    return dict(name=f"walk-{max_rows}-{F}-{'filter' if small else 'all'}", B=B,
                labels=dict(dict(max_keyframes=4, max_rows=R), **(small or {})), ops=ops, expect=None, counters=None)


def filter_edge():
    """The small-box filter at its edge: min_diag is EXACTLY the fp64 diagonal of one interpolated row (strictly greater:
    dropped) in the first case and the next fp64 below it (kept) in the second, so a sqrt or a division that is one ulp
    off shows as a row too many or too few."""
    rng = np.random.default_rng(7)
    n, R = 40, 64
    rows0 = [row(i + 1, *rng.uniform(1, 300, 4)) for i in range(n)]
    rows1 = [row(i + 1, *rng.uniform(1, 300, 4)) for i in range(n)]
    p = push(R, [[(BASE_T, rows0), (BASE_T + 33333, rows1)]])
    probe = LabelDefinition(1, dict(max_keyframes=2, max_rows=R))
    probe.push_arrays(**p[1])
    out = []
    for k, dt in enumerate((1, 11111, 33332)):
        _, xywh, _, _ = probe.rows_at(0, BASE_T + dt)
        diag = np.sqrt(xywh[:, 3] * xywh[:, 3] + xywh[:, 2] * xywh[:, 2])
        edge = float(np.sort(diag)[n // 2])
        for name, bound, kept in (("at", edge, n - n // 2 - 1), ("below", float(np.nextafter(edge, 0.0)), n - n // 2)):
            out.append(dict(name=f"filter-edge-{k}-{name}", B=1, labels=dict(max_keyframes=2, max_rows=R, min_diag=bound),
                            ops=[p, at(BASE_T + dt)], expect=None, counters=None, kept=kept))
    return out


def cases():
    return hand_cases() + [walk(*w) for w in WALKS] + filter_edge()
