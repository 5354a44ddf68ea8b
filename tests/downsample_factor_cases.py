"""Inputs of the downsampler's tests at cell areas that are no power of two (tests/test_downsample_factors_cpu.py,
tests/test_downsample_gpu.py, tests/test_stream_downsample_gpu.py) and of their generator
(tests/make_golden_refpy_downsample.py).

At ``fx * fy`` = 2, 4, 16 the increment ``1 / (fx * fy)`` is a power of two and every way of forming
``state += p / (fx * fy)`` gives the same bits; at 3, 6, 9, 12, 15, 25 the reference's float64 quotient and a quotient
rounded to fp32 first part ways.  Per case ``(fx, fy)``: an 8 x 6 cell grid, so an ``8 fx`` x ``6 fy`` input; two chunks of
uniform events, +1 / -1 at 70 / 30, sorted timestamps, drawn from a fixed seed.  The fixture
``tests/golden/ref_py_downsample_factors.npz`` holds what the reference's ``scripts/downsample_events.py`` made of them (kept
mask per chunk as ``np.packbits``, change map after each chunk) and a sha256 of the inputs: the events themselves are
re-drawn here, and ``check_inputs`` tells a drifted random generator from a wrong kernel."""
import hashlib
import os

import numpy as np

CW, CH = 8, 6
CASES = ((2, 2), (3, 1), (3, 2), (3, 3), (4, 3), (5, 3), (5, 5))      # (2, 2): the control, a power of two
CONTROL = (2, 2)
KEPT_SET_DIFFERS = (3, 6, 15)            # areas at which the fp32 increment keeps other events on these inputs ...
FINAL_MAP_DIFFERS = (9, 12, 25)          # ... and at which it leaves at least another final map
CHUNK_EVENTS = 30000                     # ~1250 events per cell over both chunks
CHUNK_US = 100000
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_py_downsample_factors.npz")
IDS = [f"{fx}x{fy}" for fx, fy in CASES]

_CHUNKS = {}


def chunks(fx, fy):
    """The case's two chunks, dicts of ``x, y`` int16, ``t`` int64, ``p`` int8 (shared: do not write into them)."""
    if (fx, fy) not in _CHUNKS:
        rng = np.random.Generator(np.random.PCG64(7000 + 100 * fx + fy))
        out = []
        for c in range(2):
            n = CHUNK_EVENTS
            ev = dict(x=rng.integers(0, CW * fx, n).astype(np.int16), y=rng.integers(0, CH * fy, n).astype(np.int16),
                      t=np.sort(rng.integers(0, CHUNK_US, n)).astype(np.int64) + CHUNK_US * c,
                      p=np.where(rng.random(n) < 0.7, 1, -1).astype(np.int8))
            for v in ev.values():
                v.setflags(write=False)
            out.append(ev)
        _CHUNKS[(fx, fy)] = out
    return _CHUNKS[(fx, fy)]


def digest(fx, fy):
    h = hashlib.sha256()
    for ev in chunks(fx, fy):
        for k in ("x", "y", "t", "p"):
            h.update(np.ascontiguousarray(ev[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(FIXTURE, allow_pickle=False)
    return _G


def check_inputs(fx, fy):
    """Before anything else: the events drawn here are the ones the fixture was recorded on."""
    assert np.array_equal(digest(fx, fy), golden()[f"{fx}x{fy}_sha256"]), \
        f"{fx}x{fy}: the generator drifted -- the events drawn from the seed are not the ones the fixture was recorded on " \
        "(numpy's random stream changed?); this says nothing about the downsampler"


def expected(fx, fy):
    """The fixture's side of a case: per chunk ``(mask bool[n], survivors dict x, y, t, p at the cells, map fp32[CH, CW])``."""
    G = golden()
    out = []
    for c, ev in enumerate(chunks(fx, fy)):
        mask = np.unpackbits(G[f"{fx}x{fy}_mask{c}"])[:len(ev["t"])].astype(bool)
        sv = dict(x=ev["x"][mask] // fx, y=ev["y"][mask] // fy, t=ev["t"][mask], p=ev["p"][mask])
        out.append((mask, sv, G[f"{fx}x{fy}_map{c}"]))
    return out


def shifted(ev, by=7919):
    """Another lane's chunk: the same pixels and polarities ``by`` events later, on the same clock."""
    return dict(x=np.roll(ev["x"], by), y=np.roll(ev["y"], by), t=ev["t"], p=np.roll(ev["p"], by))
