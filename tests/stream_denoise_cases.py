"""Pushes for the event stream's noise filter (tests/test_stream_denoise_cpu.py and _gpu.py).

A case is ``dict(name, B, W, H, D, R, pushes, expect)``: a ``W x H`` sensor, ``B`` lanes, ``denoise_us = D`` and
``refractory_us = R`` (None: off), a list of pushes ``dict(x, y, t, p, batch)`` in lane order with absolute int64
timestamps from ``T0 = 2^33 + 777`` on, and -- for the hand-computed cases -- the expected keep mask of every push.  The
sensors are the smallest at which the kernel can go wrong: 8x6, 16x12 and 33x21 (odd, not a multiple of anything).

``random_case`` draws uniform pixels at a rate that leaves a share of the events unsupported and a share refractory
(``D`` and ``R`` are set from the sensor's size), in pushes of 0, 1, 2, ~300 and -- on the 16x12 sensor -- ~6000 events (runs
hundreds long; the sort and the scan span several blocks), with an empty lane in the middle of a batch, a push that names
only the last lane and one gap between pushes above 2^31 us.  ``outside`` mixes events outside the sensor in."""
import numpy as np

T0 = (1 << 33) + 777
GAP = (1 << 31) + 5
SENSORS = ((8, 6), (16, 12), (33, 21))
MODES = ("denoise", "refractory", "both")


def push(parts):
    """parts: {lane: (x, y, t, p)} with t relative to T0 -> one push in lane order."""
    lanes = sorted(parts)
    cat = [np.concatenate([np.asarray(parts[b][k]) for b in lanes]) if lanes else np.zeros(0) for k in range(4)]
    batch = np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes]) if lanes else np.zeros(0, np.int64)
    return dict(x=cat[0].astype(np.int16), y=cat[1].astype(np.int16), t=cat[2].astype(np.int64) + T0, p=cat[3].astype(np.int8),
                batch=batch)


def events(rows):
    """rows: [(x, y, t)] -> (x, y, t, p) with alternating polarity."""
    a = np.asarray(rows, np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2], np.where(np.arange(len(a)) % 2 == 0, 1, -1)


def hand_boundaries():
    """D = 100 and R = 50 on their boundaries, equal timestamps on one pixel and on two neighbouring pixels, the first
    event ever on a pixel."""
    rows = [(3, 3, 0),        # the first event ever, no neighbour stamped: unsupported
            (4, 3, 100),      # (3,3) is exactly D old: supported
            (2, 3, 101),      # (3,3) is D + 1 old: unsupported
            (3, 3, 149),      # own stamp 149 old, (4,3) 49 old: kept
            (3, 3, 198),      # own stamp R - 1 old: refractory
            (4, 4, 240),      # (3,3) 42 old: kept
            (3, 3, 248),      # own stamp exactly R old: not refractory; (4,4) 8 old: kept
            (3, 3, 248),      # the same timestamp on the same pixel: the second sees the first, refractory
            (5, 5, 300),      # (4,4) 60 old: kept
            (6, 5, 300),      # (5,5) at the same timestamp, earlier in arrival: supported
            (0, 0, 400),      # a corner, its later neighbour does not count: unsupported
            (1, 0, 400)]      # sees (0,0) at t - s = 0: supported
    keep = [False, True, False, True, False, True, True, False, True, True, False, True]
    return dict(name="hand-boundaries", B=1, W=8, H=6, D=100, R=50, pushes=[push({0: events(rows)})],
                expect=[np.array(keep)])


def hand_edges():
    """Nothing wraps into the next row or the next lane: (W - 1, y) and (0, y + 1), the corners, the last pixel of lane 0
    and the first of lane 1."""
    lane0 = [(7, 2, 0),       # first: unsupported
             (0, 3, 10),      # (7,2) is the previous pixel in memory, not a neighbour: unsupported
             (7, 5, 20),      # the last pixel of lane 0: unsupported
             (6, 5, 30),      # (7,5) 10 old: supported
             (0, 0, 40),      # corner: unsupported
             (1, 1, 50),      # (0,0): supported
             (7, 0, 60),      # corner: unsupported
             (0, 5, 70)]      # corner: unsupported
    lane1 = [(0, 0, 25),      # the first pixel of lane 1, behind lane 0's (7,5) in memory (5 us old): unsupported
             (7, 5, 26),      # unsupported
             (7, 4, 27)]      # (7,5) of its own lane: supported
    keep = [False, False, False, True, False, True, False, False, False, False, True]
    return dict(name="hand-edges", B=2, W=8, H=6, D=1000, R=None, pushes=[push({0: events(lane0), 1: events(lane1)})],
                expect=[np.array(keep)])


def hand_carried():
    """Support from the carried map only, from the same push only and from both; a pixel whose neighbours were stamped in
    an earlier push and not since; a gap above 2^31 us between two pushes."""
    pushes = [[(2, 2, 0),                 # unsupported
               (3, 2, 10)],               # supported
              [(2, 3, 90),                # only the carried map: (2,2) 90 old, (3,2) 80 old
               (5, 5, 95)],               # unsupported
              [(6, 1, 500),               # unsupported
               (7, 1, 501),               # only the same push
               (5, 4, 520),               # (5,5) was stamped two pushes ago, 425 old, and not since: unsupported
               (4, 4, 530),               # the same push: (5,4) 10 old; the carried (5,5) is stale
               (5, 5, 540)],              # (5,4) and (4,4)
              [(5, 4, 540 + GAP),         # (5,5) is 2^31 + 5 old: unsupported (an int32 difference would be negative)
               (4, 5, 640 + GAP),         # (5,4) exactly D old
               (3, 5, 741 + GAP)]]        # (4,5) D + 1 old
    keep = [[False, True], [True, False], [False, True, False, True, True], [False, True, False]]
    return dict(name="hand-carried", B=1, W=8, H=6, D=100, R=None, pushes=[push({0: events(r)}) for r in pushes],
                expect=[np.array(k) for k in keep])


def _draw(rng, n, W, H, t0, border):
    """n events from t0 on, 0..3 us apart; `border`: on the sensor's outline only."""
    x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    if border:
        side = rng.integers(0, 4, n)
        x = np.where(side == 0, 0, np.where(side == 1, W - 1, x))
        y = np.where(side == 2, 0, np.where(side == 3, H - 1, y))
    t = t0 + np.cumsum(rng.integers(0, 4, n))
    return x, y, t, rng.choice(np.array([-1, 1]), n)


def random_case(W, H, B, mode, seed, large=False, outside=False):
    """Lane sizes per push; lane b's clock is its own.  D and R: 70 % of the mean time between two events of a pixel's
    neighbourhood / of a pixel, at 1.5 us per event."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pixels = W * H
    D = None if mode == "refractory" else max(2, int(0.7 * 1.5 * pixels / 8))
    R = None if mode == "denoise" else max(2, int(0.7 * 1.5 * pixels))
    last = B - 1
    plan = [{b: 300 + 7 * b for b in range(B)},            # ~300 per lane
            {},                                             # an empty push
            {last: 1},                                      # one event, and only the last lane
            {0: 2},
            {b: 281 + 13 * b for b in range(B) if not (B == 3 and b == 1)},      # an empty lane in the middle
            {b: (6000 if large else 150) // B + b for b in range(B)},
            {b: 90 for b in range(B)}]                      # after the gap: only stale stamps, then fresh ones
    clock = [0] * B
    pushes = []
    for k, sizes in enumerate(plan):
        parts = {}
        for b, n in sizes.items():
            if k == len(plan) - 1:
                clock[b] += GAP
            x, y, t, p = _draw(rng, n, W, H, clock[b], border=(k == 4))
            clock[b] = int(t[-1])
            if outside and n > 4:                           # a few events off the sensor, on every side
                bad = rng.choice(n, 4, replace=False)
                x[bad], y[bad] = [-1, W, x[bad[2]], x[bad[3]]], [y[bad[0]], y[bad[1]], -1, H]
            parts[b] = (x, y, t, p)
        pushes.append(push(parts))
    return dict(name=f"random-{W}x{H}-B{B}-{mode}" + ("-large" if large else "") + ("-outside" if outside else ""), B=B, W=W,
                H=H, D=D, R=R, pushes=pushes, expect=None)


_CASES = None


def cases():
    """Every case, built once."""
    global _CASES
    if _CASES is None:
        out = [hand_boundaries(), hand_edges(), hand_carried()]
        seed = 100
        for (W, H) in SENSORS:
            for B in (1, 3):
                for mode in MODES:
                    seed += 1
                    out.append(random_case(W, H, B, mode, seed, large=(W, H) == (16, 12)))
        out.append(random_case(8, 6, 3, "both", 201, outside=True))
        out.append(random_case(33, 21, 1, "denoise", 202, outside=True))
        _CASES = out
    return _CASES


def reference(case):
    """Per push of a case, from ``denoise_definition`` alone: ``(keep mask, stamp maps after the push, cumulative
    filtered [B], status word)``; computed once per case and left unchanged."""
    if "_ref" not in case:
        from dagr_amd.streaming import NEVER, denoise_definition
        B, W, H = case["B"], case["W"], case["H"]
        maps = np.full((B, H, W), NEVER, np.int64)
        filtered = np.zeros(B, np.int64)
        ref = []
        for s in case["pushes"]:
            keep = denoise_definition(maps, s["x"], s["y"], s["t"], s["batch"], case["D"], case["R"])
            inside = (s["x"] >= 0) & (s["x"] < W) & (s["y"] >= 0) & (s["y"] < H)
            filtered = filtered + np.bincount(s["batch"][inside & ~keep], minlength=B)
            ref.append((keep, maps.copy(), filtered.copy(), 0 if inside.all() else 16))
        case["_ref"] = ref
    return case["_ref"]
