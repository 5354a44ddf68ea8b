"""An encoder of event-camera words (EVT 3.0 / EVT 2.0 as ``dagr_amd/streaming.py`` states them), for tests and synthetic
sources: ``encode_events`` writes the word sequence that ``DecodeDefinition`` -- and ``dagr_stream_decode`` -- turn back into
the events it was given.  It is not a model of any camera: a sensor chooses its own grouping, redundancy and word order."""
import numpy as np

EVT3_SKIPPED_TYPES = (0x1, 0x7, 0x9, 0xA, 0xB, 0xC, 0xD, 0xE, 0xF)
EVT2_SKIPPED_TYPES = (0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x9, 0xA, 0xB, 0xC, 0xD, 0xE, 0xF)


def encode_events(x, y, t, p, format, rng=None, t_prev=None):
    """The words of ONE lane for the events ``(x, y, t, p)``: ``x``, ``y`` in 0..2047, ``t`` non-negative and
    non-decreasing microseconds relative to the lane's ``t_base``, ``p`` positive for ON.  ``format`` is ``"evt3"`` (uint16
    words) or ``"evt2"`` (uint32 words).

    EVT 3.0: consecutive events of one row, one timestamp and one polarity with ascending ``x`` become a ``VECT_BASE_X`` and
    ``VECT_12`` / ``VECT_8`` words (a new base where the next event is more than a word away), a single event an ``ADDR_X``;
    ``TIME_HIGH`` / ``TIME_LOW`` / ``ADDR_Y`` are written when they change.  Both formats: the time-high counter advances by
    less than the decoder's wrap threshold per ``TIME_HIGH``, so a gap of any length -- and every wrap of the counter -- is
    followed (2^24 us for EVT 3.0, 2^34 us for EVT 2.0).

    ``t_prev``: the time the decoder's state stands at (the last event encoded for this lane before); None: the decoder
    is freshly reset, and the sequence starts with ``TIME_HIGH`` 0.  ``rng`` (a ``numpy.random.Generator``): also sprinkle
    redundant time and row words, words of skipped types and random values in ignored bits; the decoded events are the
    same."""
    if format not in ("evt2", "evt3"):
        raise ValueError(f"encode_events: format = {format!r} must be 'evt2' or 'evt3'")
    x, y = np.asarray(x).astype(np.int64).reshape(-1), np.asarray(y).astype(np.int64).reshape(-1)
    t, p = np.asarray(t).astype(np.int64).reshape(-1), np.asarray(p).reshape(-1) > 0
    n = len(t)
    if not (len(x) == len(y) == len(p) == n):
        raise ValueError("encode_events: x, y, t and p differ in length")
    if n and (x.min() < 0 or x.max() > 2047 or y.min() < 0 or y.max() > 2047):
        raise ValueError("encode_events: x and y must be in 0..2047 (11 bits)")
    if n and (t[0] < 0 or (np.diff(t) < 0).any() or (t_prev is not None and t[0] < int(t_prev))):
        raise ValueError("encode_events: t must be non-negative and non-decreasing (and not before t_prev)")
    evt3 = format == "evt3"
    shift, bits = (12, 12) if evt3 else (6, 28)         # us per time-high unit (log2), bits of the time-high counter
    step_max = (1 << (bits - 1)) - 1                    # below the decoder's wrap threshold
    skipped = EVT3_SKIPPED_TYPES if evt3 else EVT2_SKIPPED_TYPES
    top = 12 if evt3 else 28
    words = []
    high = None if t_prev is None else int(t_prev) >> shift     # the full time-high count the decoder stands at
    low = row = None

    def chance(q):
        return rng is not None and rng.random() < q

    def time_high(target):
        nonlocal high
        if high is None:
            high = 0
            words.append(0x8 << top)
        while high < target:
            high += min(target - high, step_max)
            words.append(0x8 << top | (high & ((1 << bits) - 1)))

    def noise():
        if chance(0.05):
            words.append(int(skipped[rng.integers(len(skipped))]) << top | int(rng.integers(1 << top)))
        if chance(0.05) and high is not None:
            words.append(0x8 << top | (high & ((1 << bits) - 1)))
        if evt3 and chance(0.05) and low is not None:
            words.append(0x6 << 12 | low)
        if evt3 and chance(0.05) and row is not None:
            words.append(0x0 << 12 | int(rng.integers(2)) << 11 | row)

    i = 0
    xl, yl, tl, pl = x.tolist(), y.tolist(), t.tolist(), p.tolist()
    while i < n:
        noise()
        if high is None or (tl[i] >> shift) != high:
            time_high(tl[i] >> shift)
        if not evt3:
            words.append((1 if pl[i] else 0) << 28 | (tl[i] & 0x3F) << 22 | xl[i] << 11 | yl[i])
            i += 1
            continue
        if (tl[i] & 0xFFF) != low:
            low = tl[i] & 0xFFF
            words.append(0x6 << 12 | low)
        if yl[i] != row:
            row = yl[i]
            words.append(0x0 << 12 | (int(rng.integers(2)) << 11 if rng is not None else 0) | row)
        j = i + 1
        while j < n and yl[j] == row and tl[j] == tl[i] and pl[j] == pl[i] and xl[j] > xl[j - 1]:
            j += 1
        pol = (1 if pl[i] else 0) << 11
        if j == i + 1:
            words.append(0x2 << 12 | pol | xl[i])
            i = j
            continue
        base = None
        while i < j:
            if base is None or xl[i] >= base + 12:
                base = xl[i]
                words.append(0x3 << 12 | pol | base)
            mask = 0
            while i < j and xl[i] < base + 12:
                mask |= 1 << (xl[i] - base)
                i += 1
            if mask < 0x100 and not chance(0.3):
                # VECT_8 reaches base + 7; events at base + 8 .. base + 11 wait for the next word
                words.append(0x5 << 12 | (int(rng.integers(16)) << 8 if rng is not None else 0) | mask)
                base += 8
            else:
                words.append(0x4 << 12 | mask)
                base += 12
    noise()
    return np.array(words, np.uint16 if evt3 else np.uint32)
