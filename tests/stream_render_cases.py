"""Cases of the stream's picture (dagr_amd/streaming.py: RenderDefinition, dagr_stream_trail / dagr_stream_render), shared
by the CPU and the GPU tests; nothing here needs a device.

    scene(W, H, B, M, T, ...)   one step's det / n_keep / track_id and the slot states of the steps in front of it
    slot_walk(B, M, steps)      slot states in which slots are freed and re-used, for the rings alone
    events(W, H, n, seed)       integer events of one lane, some outside the image
"""
import numpy as np

NEVER = np.iinfo(np.int64).min
T0 = (1 << 33) + 4321           # absolute microseconds: int64 matters
A = 14
PAD = (1.0, 1.0, 30.0, 25.0, 1.0, 0.0)          # rows at and behind n_keep: a box that would show if anything read it
IDS = (7, 42, 365, 1234, 56789, 999999, 10 ** 6 + 7, 10 ** 6)        # 1 to 7 digits; "7" and "0" behind the modulus


def rows_lane0(W, H):
    """The rows every scene's lane 0 holds: (x1, y1, x2, y2, score, label) and the track id of each."""
    nan, inf = float("nan"), float("inf")
    rows = [((5, 8, 20, 20), 7),                            # inside
            ((12, 12, 30.5, 25), 42),                       # overlaps row 0: the later row wins
            ((W - 10, H - 8, W + 15, H + 9), 365),          # partly outside
            ((W + 50, 10, W + 80, 30), 1234),               # wholly outside
            ((-12.5, -7.25, 6.5, 9.75), 56789),             # negative corners; the plate goes inside and is clipped
            ((30, 27, 22, 21), 999999),                     # reversed corners; a six-digit plate
            ((15.3, 3.9, 15.3, 3.9), 10 ** 6 + 7),          # zero area: one pixel; plate inside (ya - 7s < 0)
            ((3, nan, 9, 9), 99),                           # a NaN row: skipped
            ((24, 0.5, 33, 6), 10 ** 6),                    # ya = 0: the plate sits inside; text "0"
            ((2, H - 9, 9, H - 2), 0),                      # no track: entry 0, no plate
            ((4, 4, inf, 9), 98),                           # an infinite corner: skipped
            ((-1e9, -1e9, 1e9, 1e9), 5)]                    # clamped to +-2^20: nothing of it is in the image
    det = np.array([(*bx, 0.9 - 0.01 * i, i % 2) for i, (bx, _) in enumerate(rows)], np.float32)
    return det, np.array([i for _, i in rows], np.int64)


def scene(W, H, B, M, T, seed=3, steps=6, long_segment=False):
    """det fp32 [B, A, 6], n_keep int32 [B], track_id int64 [B, A], and ``slots``: per step (id int64 [B, M], t_last int64
    [B, M], box fp32 [B, M, 4], t_ref int64 [B]).  Lane 0 holds ``rows_lane0`` (n_keep 12 of A = 14), lane 1 is empty
    (n_keep 0, no track, no t_ref), lane 2 has n_keep > A and random rows.  Slots 0 and 1 of lane 0 walk the two diagonals
    and cross; one slot is not seen at step 2 (coasting), one is re-used under a new id at step 3; with ``long_segment`` the
    last slot of lane 0 jumps by more than W + H at the last step."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * M + T))
    det = np.tile(np.asarray(PAD, np.float32), (B, A, 1))
    track_id = np.full((B, A), 77, np.int64)
    n_keep = np.zeros(B, np.int32)
    d0, i0 = rows_lane0(W, H)
    det[0, :len(d0)], track_id[0, :len(d0)], n_keep[0] = d0, i0, len(d0)
    if B > 2:
        xy = rng.uniform(-5, [W, H], (A, 2))
        wh = rng.uniform(0, [W / 2, H / 2], (A, 2))
        det[2] = np.concatenate([xy, xy + wh, rng.uniform(0, 1, (A, 1)), rng.integers(0, 2, (A, 1))], 1).astype(np.float32)
        track_id[2] = rng.integers(0, 5000, A)
        n_keep[2] = A + 5
    live = np.zeros((B, M), bool)
    for b in range(B):
        if b != 1:
            live[b, rng.permutation(M)[:min(M, 40)]] = True
            live[b, :2] = True
            live[b, M - 1] = True
    ids = np.where(live, 1 + np.arange(B * M).reshape(B, M) * 3, 0).astype(np.int64)
    start = rng.uniform(0, [W, H], (B, M, 2))
    vel = rng.uniform(-6, 6, (B, M, 2))
    size = rng.uniform(2, 12, (B, M, 2))
    slots = []
    for k in range(steps):
        t_ref = np.array([T0 + 1000 * k if b != 1 else NEVER for b in range(B)], np.int64)
        c = start + vel * k
        f = k / max(steps - 1, 1)
        c[0, 0] = (2 + f * (W - 5), 2 + f * (H - 5))                    # the two diagonals of lane 0
        if M > 1:
            c[0, 1] = (W - 3 - f * (W - 5), 2 + f * (H - 5))
        if long_segment and k == steps - 1:
            c[0, M - 1] = c[0, M - 1] + (3 * (W + H), 17)
        box = np.concatenate([c - size / 2, c + size / 2], 2).astype(np.float32)
        t_last = np.where(live, t_ref[:, None], 0).astype(np.int64)
        cur = ids.copy()
        if M > 2:
            if k == 2:
                t_last[0, 2] -= 1000                                    # not seen: appends nothing
            if k >= 3:
                cur[0, 2] += 1                                          # the slot went to another track
        if k == 1:
            box[0, M - 1, 0] = np.nan                                   # a non-finite centre is not appended
        slots.append((cur, t_last, box, t_ref))
    return dict(W=W, H=H, B=B, M=M, T=T, det=det, n_keep=n_keep, track_id=track_id, slots=slots)


def slot_walk(B, M, steps=40, seed=5):
    """``steps`` slot states of a tracker-like walk: a slot is taken with probability 0.2 a step, freed with 0.08, not seen
    with 0.25; ids count up, so a slot taken again carries a new id."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids, t_last = np.zeros((B, M), np.int64), np.zeros((B, M), np.int64)
    box = np.zeros((B, M, 4), np.float32)
    next_id, out = 1, []
    for k in range(steps):
        t_ref = np.full(B, T0 + 1000 * k, np.int64)
        if k < 2:
            t_ref[B - 1] = NEVER                                        # the last lane gets its instant late
        for b in range(B):
            for s in range(M):
                if ids[b, s] and rng.random() < 0.08:
                    ids[b, s] = 0
                if not ids[b, s] and rng.random() < 0.2 and t_ref[b] != NEVER:
                    ids[b, s], next_id = next_id, next_id + 1
                    box[b, s] = rng.uniform(-20, 300, 4)
                    t_last[b, s] = t_ref[b]
                elif ids[b, s] and rng.random() > 0.25:
                    box[b, s] += rng.normal(0, 3, 4).astype(np.float32)
                    t_last[b, s] = t_ref[b]
        out.append((ids.copy(), t_last.copy(), box.copy(), t_ref))
    return out


def events(W, H, n, seed, t_lo=0, t_hi=1000):
    """``(x int16, y int16, t int64 sorted, p int8 in {-1, 1})``: ``n`` events with T0 + t_lo <= t <= T0 + t_hi, a tenth of
    them beyond the image."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    far = rng.random(n) < 0.1
    x[far] += W
    t = np.sort(rng.integers(T0 + t_lo, T0 + t_hi + 1, n)).astype(np.int64)
    return x.astype(np.int16), y.astype(np.int16), t, rng.choice(np.array([-1, 1], np.int8), n)


def run_definition(sc, render):
    """A ``RenderDefinition`` fed the scene's slot states; returns it."""
    from dagr_amd.streaming import RenderDefinition
    d = RenderDefinition(sc["B"], sc["W"], sc["H"], render=render, max_tracks=sc["M"])
    for ids, t_last, box, t_ref in sc["slots"]:
        d.trail_step(ids, t_last, box, t_ref)
    return d
