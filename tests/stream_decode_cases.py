"""Seeded word streams for the decoder's tests (tests/test_stream_decode_*.py): each builder returns a dict of ``name``,
``format``, ``sensor`` (W, H), ``B``, ``words``, ``lane_words`` and, where ``encode_events`` made the words, ``events`` --
the source ``(x, y, t, p, batch)``.  ``T = DAGR_DECODE_TILE`` is the kernels' words per workgroup: the cases put a lane
start, a wrap and a carried ``base_x`` on and across tile boundaries."""
import numpy as np

from dagr_amd._lib import DEFINES
from dagr_amd.data.evt import encode_events

T = DEFINES["DAGR_DECODE_TILE"]
SMALL, LARGE = (64, 48), (640, 480)
WRAP_US = {"evt3": 1 << 24, "evt2": 1 << 34}
TOP = {"evt3": 12, "evt2": 28}


def case(name, fmt, sensor, words, lane_words=None, events=None):
    words = np.asarray(words, np.uint16 if fmt == "evt3" else np.uint32)
    lane_words = np.array([len(words)] if lane_words is None else lane_words, np.int64)
    return dict(name=f"{name}-{fmt}-{sensor[0]}x{sensor[1]}", format=fmt, sensor=sensor, B=len(lane_words), words=words,
                lane_words=lane_words, events=events)


def bursts(rng, sensor, n_bursts, t0, span_us):
    """Events as an edge sweeping a sensor leaves them: bursts of one row, one instant and one polarity with ascending x
    (runs and gaps), instants non-decreasing from ``t0`` over ``span_us``."""
    w, h = sensor
    ts = np.sort(rng.integers(0, span_us, n_bursts)) + t0
    x, y, t, p = [], [], [], []
    for k in range(n_bursts):
        n = int(rng.integers(1, 30))
        xs = np.unique(rng.integers(0, w, n) if rng.random() < 0.3 else
                       np.clip(rng.integers(0, w) + np.cumsum(rng.integers(1, 4, n)), 0, w - 1))
        x += xs.tolist()
        y += [int(rng.integers(0, h))] * len(xs)
        t += [int(ts[k])] * len(xs)
        p += [int(rng.integers(0, 2)) * 2 - 1] * len(xs)
    return np.array(x, np.int16), np.array(y, np.int16), np.array(t, np.int64), np.array(p, np.int8)


def encoded(fmt, sensor, seed, n_bursts=150, t0=None, span_us=6000, noisy=True):
    """(a) encoder output with redundancy and skipped words, times crossing the format's wrap."""
    rng = np.random.default_rng(seed)
    t0 = WRAP_US[fmt] - span_us // 2 if t0 is None else t0
    x, y, t, p = bursts(rng, sensor, n_bursts, t0, span_us)
    words = encode_events(x, y, t, p, fmt, rng=rng if noisy else None)
    return case("a_encoded", fmt, sensor, words, events=(x, y, t, p, np.zeros(len(t), np.int32)))


def th(fmt, v):
    return 0x8 << TOP[fmt] | v


def event_word(fmt, rng, sensor):
    """One single-event word at a random pixel inside the sensor (EVT 3.0: on the row the state holds)."""
    if fmt == "evt3":
        return 0x2 << 12 | int(rng.integers(2)) << 11 | int(rng.integers(sensor[0]))
    return int(rng.integers(2)) << 28 | int(rng.integers(64)) << 22 | int(rng.integers(sensor[0])) << 11 | int(rng.integers(sensor[1]))


def filler(fmt, rng, sensor, n):
    """n words that hold no TIME_HIGH: events, rows, TIME_LOW and skipped types."""
    out = []
    for _ in range(n):
        r = rng.random()
        if fmt == "evt3" and r < 0.15:
            out.append(0x0 << 12 | int(rng.integers(sensor[1])))
        elif fmt == "evt3" and r < 0.3:
            out.append(0x6 << 12 | int(rng.integers(4096)))
        elif r < 0.35:
            out.append((0xE if fmt == "evt3" else 0xA) << TOP[fmt] | int(rng.integers(1 << 8)))
        else:
            out.append(event_word(fmt, rng, sensor))
    return out


def carried_base(seed):
    """(b) one VECT_BASE_X, then 2T + 7 sparse vector words: base_x is carried over two tile boundaries.  The sensor is as
    wide as int16 allows, so that the carried base shows in the decoded x, not only in the outside count."""
    rng = np.random.default_rng(seed)
    words = [th("evt3", 7), 0x6 << 12 | 123, 0x0 << 12 | 5, 0x3 << 12 | 1 << 11 | 3]
    for _ in range(2 * T + 7):
        kind = 0x4 if rng.random() < 0.5 else 0x5
        mask = (1 << int(rng.integers(12))) if rng.random() < 0.3 else 0
        words.append(kind << 12 | mask | (int(rng.integers(16)) << 8 if kind == 0x5 and not mask & 0xF00 else 0))
    return case("b_carried_base", "evt3", (32767, 48), words)


def late_wrap(fmt, sensor, seed):
    """(c) more than 2T words with no TIME_HIGH, then a wrap exactly at a tile boundary (word 3T is the TIME_HIGH)."""
    rng = np.random.default_rng(seed)
    top = (1 << (12 if fmt == "evt3" else 28)) - 96
    words = [th(fmt, top)] + filler(fmt, rng, sensor, 3 * T - 1) + [th(fmt, 10)] + filler(fmt, rng, sensor, 40)
    assert len(words) == 3 * T + 41 and words[3 * T] == th(fmt, 10)
    return case("c_late_wrap", fmt, sensor, words)


def unsynced(fmt, sensor, seed):
    """(d) words before the first TIME_HIGH."""
    rng = np.random.default_rng(seed)
    head = filler(fmt, rng, sensor, 300)
    if fmt == "evt3":
        head += [0x3 << 12 | 2, 0x4 << 12 | 0xFFF, 0x5 << 12 | 0x0F]
    return case("d_unsynced", fmt, sensor, head + [th(fmt, 3)] + filler(fmt, rng, sensor, 300))


def outside(fmt, sensor):
    """(e) x / y outside the sensor, base_x + i running past sensor_w."""
    w, h = sensor
    if fmt == "evt2":
        words = [th(fmt, 1)] + [1 << 28 | 9 << 22 | x << 11 | y
                                for x, y in ((w - 1, h - 1), (w, h - 1), (w - 1, h), (2047, 2047), (0, 0), (w, h))]
        return case("e_outside", fmt, sensor, words)
    words = [th(fmt, 1), 0x6 << 12 | 9, 0x0 << 12 | (h - 1), 0x2 << 12 | (w - 1), 0x2 << 12 | w, 0x2 << 12 | 2047,
             0x3 << 12 | 1 << 11 | (w - 4), 0x4 << 12 | 0xFFF, 0x4 << 12 | 0xFFF,        # 4 inside, then all outside
             0x3 << 12 | (w - 10), 0x5 << 12 | 0xFF, 0x5 << 12 | 0xFF,                      # 8 inside, 2 inside + 6 outside
             0x0 << 12 | h, 0x2 << 12 | 0, 0x3 << 12 | 0, 0x4 << 12 | 0x5A5,              # the row is outside
             0x0 << 12 | 1 << 11 | 0, 0x2 << 12 | 1]                                        # bit 11 of ADDR_Y is ignored
    return case("e_outside", fmt, sensor, words)


def jumps(fmt, sensor, seed):
    """(f) backward TIME_HIGH jumps one below the wrap rule and at it."""
    rng = np.random.default_rng(seed)
    thr = 2048 if fmt == "evt3" else 1 << 27
    ev = lambda: filler(fmt, rng, sensor, 6) + [event_word(fmt, rng, sensor)]     # noqa: E731
    words = ([th(fmt, thr + 952)] + ev() + [th(fmt, 953)] + ev() +             # back by thr - 1: no wrap, t goes backwards
             [th(fmt, thr + 953)] + ev() + [th(fmt, 953)] + ev())              # back by thr: a wrap
    return case("f_jumps", fmt, sensor, words)


def lanes(fmt, sensor, seed):
    """(g) B = 3 with an empty middle lane and a lane boundary inside a tile."""
    a = encoded(fmt, sensor, seed, n_bursts=400)
    b = encoded(fmt, sensor, seed + 1, n_bursts=60, t0=5000)
    assert T < len(a["words"]) and len(a["words"]) % T != 0
    ev = tuple(np.concatenate([u, v]) for u, v in zip(a["events"][:4], b["events"][:4]))
    batch = np.concatenate([np.zeros(len(a["events"][0]), np.int32), np.full(len(b["events"][0]), 2, np.int32)])
    return case("g_lanes", fmt, sensor, np.concatenate([a["words"], b["words"]]), [len(a["words"]), 0, len(b["words"])],
                events=(*ev, batch))


def lengths(fmt, sensor, seed):
    """(h) n_words in {0, 1, T - 1, T, T + 1, 3T + 5}: prefixes of one encoded stream."""
    long = encoded(fmt, sensor, seed, n_bursts=700)["words"]
    assert len(long) >= 3 * T + 5
    return [case(f"h_len{n}", fmt, sensor, long[:n]) for n in (0, 1, T - 1, T, T + 1, 3 * T + 5)]


def full_vectors():
    """(i) all-ones VECT_12 words: 12 events per word, to exercise max_out."""
    words = [th("evt3", 2), 0x6 << 12 | 1, 0x0 << 12 | 7, 0x3 << 12 | 1 << 11 | 0] + [0x4 << 12 | 0xFFF] * 40
    return case("i_full_vectors", "evt3", LARGE, words)


def all_cases():
    out = []
    for fmt in ("evt3", "evt2"):
        for sensor in (SMALL, LARGE):
            out.append(encoded(fmt, sensor, 11))
        out += [late_wrap(fmt, SMALL, 12), unsynced(fmt, SMALL, 13), outside(fmt, SMALL), outside(fmt, LARGE),
                jumps(fmt, SMALL, 14), lanes(fmt, LARGE, 15)]
        out += lengths(fmt, SMALL, 16)
    out += [carried_base(17), full_vectors()]
    return out
