"""Synthetic event streams for tests and bench.

Output contract = the reference dataset's (``src/dagr/data/utils.py:6-19``, ``dsec_data.py:141-147``):
x,y int16, t int32 (us, shifted so that the last event sits at ``time_window``), p int8 in {-1,+1}.
"""
import numpy as np


def _finish(x, y, t, rng, time_window):
    order = np.argsort(t, kind="stable")
    x, y, t = x[order], y[order], t[order]
    if len(t) > 0:
        t = time_window + t - t[-1]  # dsec_data.py:145
    p = (2 * rng.integers(0, 2, len(t)) - 1).astype(np.int8)  # dsec_data.py:146
    return x.astype(np.int16), y.astype(np.int16), t.astype(np.int32), p


def uniform_window(n, width, height, seed, window_us=50000, time_window=1000000):
    """S-uniform: x,y uniform over the sensor, t uniform over a 50 ms window."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, width, n)
    y = rng.integers(0, height, n)
    t = rng.integers(0, window_us, n)
    return _finish(x, y, t, rng, time_window)


def edges_window(n, width, height, seed, window_us=50000, time_window=1000000, n_lines=20, noise=0.1):
    """S-edges: moving line segments (<= 2 px/ms) with N(0,1.5^2) px jitter + uniform noise.
    Saturates K=16 and stresses the per-pixel FIFO depth."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_noise = int(noise * n)
    n_sig = n - n_noise
    line = rng.integers(0, n_lines, n_sig)
    x0 = rng.uniform(0, width, n_lines)
    y0 = rng.uniform(0, height, n_lines)
    ang = rng.uniform(0, np.pi, n_lines)
    length = rng.uniform(0.1, 0.4, n_lines) * width
    vx = rng.uniform(-2, 2, n_lines) / 1000.0  # px/us
    vy = rng.uniform(-2, 2, n_lines) / 1000.0
    t = rng.integers(0, window_us, n_sig)
    s = rng.uniform(-0.5, 0.5, n_sig)
    xs = x0[line] + s * length[line] * np.cos(ang[line]) + vx[line] * t + rng.normal(0, 1.5, n_sig)
    ys = y0[line] + s * length[line] * np.sin(ang[line]) + vy[line] * t + rng.normal(0, 1.5, n_sig)
    xs = np.clip(np.rint(xs), 0, width - 1).astype(np.int64)
    ys = np.clip(np.rint(ys), 0, height - 1).astype(np.int64)
    xn = rng.integers(0, width, n_noise)
    yn = rng.integers(0, height, n_noise)
    tn = rng.integers(0, window_us, n_noise)
    return _finish(np.concatenate([xs, xn]), np.concatenate([ys, yn]), np.concatenate([t, tn]), rng, time_window)


def flicker_events(pixels, hz, duration_us, seed, duty=0.5, events_per_half=3, spread_us=200, t0=0):
    """Flickering pixels, as a mains- or PWM-driven light makes them: every pixel of ``pixels`` (``[(x, y), ...]``) emits
    ``events_per_half`` ON events at the start of each period of its light (``hz``: one frequency, or one per pixel) and
    as many OFF events ``duty`` of a period later, each burst spread over ``spread_us`` microseconds, with a phase of its
    own.  Deterministic in ``seed``.  Returns ``x, y`` int16, ``t`` int64 (``t0 <= t <
    t0 + duration_us``, sorted, stable in pixel order) and ``p`` int8."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    period = 1000000 // np.broadcast_to(np.asarray(hz, np.int64), (len(pixels),))
    xs, ys, ts, ps = [], [], [], []
    for (px, py), T in zip(pixels, period):
        phase = int(rng.integers(0, T))
        starts = np.arange(phase, duration_us, T, dtype=np.int64)
        for pol, shift in ((1, 0), (-1, int(duty * T))):
            gaps = rng.integers(0, max(1, spread_us // max(1, events_per_half)), (len(starts), events_per_half))
            tt = (starts[:, None] + shift + np.cumsum(gaps, 1)).reshape(-1)
            tt = tt[tt < duration_us]
            xs.append(np.full(len(tt), px)); ys.append(np.full(len(tt), py)); ts.append(tt); ps.append(np.full(len(tt), pol))
    x, y, t, p = (np.concatenate(v) if v else np.zeros(0, np.int64) for v in (xs, ys, ts, ps))
    order = np.argsort(t, kind="stable")
    return x[order].astype(np.int16), y[order].astype(np.int16), t[order].astype(np.int64) + np.int64(t0), p[order].astype(np.int8)


def track_scene(seed, B, objects, steps, A, G=None, step_us=1000, t0=(1 << 33) + 5000, width=320, height=240, labels=2,
                speed=4.0, jitter=1.0, p_gap=0.04, gap_steps=(1, 5), p_dip=0.05, dip_steps=(1, 4), dip_score=(0.15, 0.45),
                clutter=3.0, p_death=0.01, p_unlabelled=0.01):
    """A labelled scene of moving boxes as a detector would report it, for the stream tracker and its scorer: no events, no
    model.  Per lane ``objects`` places, each holding one object at a time: a box of 14..40 px that moves at a constant
    velocity of up to ``speed`` px a step and bounces off the borders.  An object dies with ``p_death`` a step and a new
    identity is born in its place a few steps later, somewhere else.  The GROUND TRUTH of a step is every living object's
    true box with its label and identity (ids from 1, never used twice in a lane; with ``p_unlabelled`` a row carries id 0,
    an annotation without an identity).  The DETECTIONS are the living objects' boxes with N(0, ``jitter``) px on every
    corner and a score in 0.55..1, except that a detection fails for ``gap_steps`` steps with ``p_gap`` a step (the box is
    absent) and dips to a score in ``dip_score`` for ``dip_steps`` steps with ``p_dip`` a step; and on average ``clutter``
    rows a step that belong to nothing, scores 0.05..0.75.  Rows are sorted by descending score, as ``dagr_postprocess``
    leaves them, and cut at ``A``.  Seeded, pure numpy.

    Returns one dict per step: ``det`` fp32 [B, A, 6], ``n_keep`` int32 [B], ``t_ref`` int64 [B], ``gt_box`` fp32 [B, G, 4],
    ``gt_label`` int32 [B, G], ``gt_id`` int64 [B, G], ``n_gt`` int32 [B] (``G`` defaults to ``objects``)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    G = objects if G is None else G
    shape = (B, objects)

    def born(n):
        size = rng.uniform(14, 40, (n, 2))
        centre = np.stack([rng.uniform(30, width - 30, n), rng.uniform(30, height - 30, n)], -1)
        return centre, rng.uniform(-speed, speed, (n, 2)), size, rng.integers(0, labels, n)

    centre, vel, size, label = (a.reshape(shape + a.shape[1:]) for a in born(B * objects))
    ident = np.tile(np.arange(1, objects + 1, dtype=np.int64), (B, 1))     # ids 1 .. objects in every lane; 0: the place is empty
    next_id = np.full(B, objects + 1, np.int64)
    dead_until = np.zeros(shape, np.int64)                          # the place is empty before this step
    gap_until, dip_until = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    out = []
    for k in range(steps):
        centre += vel
        for axis, limit in ((0, width), (1, height)):              # bounce
            over = (centre[..., axis] < 10) | (centre[..., axis] > limit - 10)
            vel[..., axis] = np.where(over, -vel[..., axis], vel[..., axis])
        alive = dead_until <= k
        reborn = alive & (ident == 0)
        for b, o in zip(*np.nonzero(reborn)):
            c, v, s, lab = born(1)
            centre[b, o], vel[b, o], size[b, o], label[b, o] = c[0], v[0], s[0], lab[0]
            ident[b, o], next_id[b] = next_id[b], next_id[b] + 1
            gap_until[b, o] = dip_until[b, o] = 0
        dies = alive & (rng.random(shape) < p_death)
        dead_until[dies] = k + rng.integers(2, 8, int(dies.sum()))
        ident[dies] = 0
        alive &= ~dies
        starts = alive & (gap_until <= k) & (rng.random(shape) < p_gap)
        gap_until[starts] = k + rng.integers(gap_steps[0], gap_steps[1] + 1, int(starts.sum()))
        starts = alive & (dip_until <= k) & (rng.random(shape) < p_dip)
        dip_until[starts] = k + rng.integers(dip_steps[0], dip_steps[1] + 1, int(starts.sum()))
        det, n_keep = np.zeros((B, A, 6), np.float32), np.zeros(B, np.int32)
        gt_box, gt_label = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
        gt_id, n_gt = np.zeros((B, G), np.int64), np.zeros(B, np.int32)
        for b in range(B):
            there = np.flatnonzero(alive[b])[:G]
            true = np.concatenate([centre[b, there] - size[b, there] / 2, centre[b, there] + size[b, there] / 2], -1)
            n_gt[b] = len(there)
            gt_box[b, :len(there)], gt_label[b, :len(there)] = true, label[b, there]
            gt_id[b, :len(there)] = np.where(rng.random(len(there)) < p_unlabelled, 0, ident[b, there])
            seen = gap_until[b, there] <= k
            rows = true[seen] + rng.normal(0, jitter, (int(seen.sum()), 4))
            score = np.where(dip_until[b, there][seen] > k, rng.uniform(dip_score[0], dip_score[1], len(rows)),
                             rng.uniform(0.55, 1.0, len(rows)))
            n_clutter = int(rng.poisson(clutter))
            c, _, s, lab = born(n_clutter)
            rows = np.concatenate([rows, np.concatenate([c - s / 2, c + s / 2], -1)])
            score = np.concatenate([score, rng.uniform(0.05, 0.75, n_clutter)])
            lab = np.concatenate([label[b, there][seen], lab])
            order = np.argsort(-score.astype(np.float32), kind="stable")[:A]
            n_keep[b] = len(order)
            det[b, :len(order), :4], det[b, :len(order), 4], det[b, :len(order), 5] = rows[order], score[order], lab[order]
        out.append(dict(det=det, n_keep=n_keep, t_ref=np.full(B, t0 + step_us * k, np.int64), gt_box=gt_box, gt_label=gt_label,
                        gt_id=gt_id, n_gt=n_gt))
    return out


def batch_windows(gen,n_per_sample, batch_size, width, height, seed, **kw):
    """Concatenate ``batch_size`` independent windows like PyG ``Batch`` collation does:
    returns x,y,t,p and ``batch`` (int64 sample index, sorted)."""
    xs, ys, ts, ps, bs = [], [], [], [], []
    for b in range(batch_size):
        x, y, t, p = gen(n_per_sample, width, height, seed + b, **kw)
        xs.append(x); ys.append(y); ts.append(t); ps.append(p)
        bs.append(np.full(len(x), b, np.int64))
    return (np.concatenate(xs), np.concatenate(ys), np.concatenate(ts), np.concatenate(ps), np.concatenate(bs))


def format_data_np(x, y, t, width, height, time_window=1000000):
    """numpy twin of ``format_data`` (src/dagr/utils/buffers.py:33-44): fp32 true division."""
    pos = np.stack([x.astype(np.float32) / np.float32(width), y.astype(np.float32) / np.float32(height),
                    t.astype(np.float32) / np.float32(time_window)], axis=-1)
    return np.ascontiguousarray(pos.astype(np.float32))
