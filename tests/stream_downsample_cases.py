"""Raw sensor pushes for the downsampling event stream (tests/test_stream_downsample_cpu.py and _gpu.py).

The synthetic generators at sensor resolution hardly survive a 2x downsampling (a cell has to collect four events of one
polarity), so raw pushes are built from model-resolution windows: a window drawn at 320x240, every event repeated 3 to 6
times, each copy at ``(2x + {0,1}, 2y + {0,1}, t + {0,1,2})`` with the same polarity, sorted stably by ``t``.

One scripted sequence of 8 pushes, B = 3 lanes, a 640x480 sensor over the 320x215 model, serves every test; the reference
is ``oracle.downsample.downsample_events`` chained per lane over all pushes, cut to the model's rows, fed to a plain
``StreamDefinition`` -- computed once and left unchanged."""
import numpy as np

from oracle import downsample as od
from dagr_amd.streaming import StreamDefinition
from dagr_amd.utils import synthetic as syn

W, H, B = 320, 215, 3
F = 2
W_IN, H_IN = 640, 480
CW, CH = W_IN // F, H_IN // F
TW = 1000000
WINDOW_US = 20000
T0 = (1 << 33) + 777


def raw_chunk(gen, n, seed, t_lo, t_hi):
    """Raw events from ``n`` base events of ``gen`` at the cell grid, T0 + t_lo <= t <= T0 + t_hi + 2."""
    x, y, t, p = gen(n, CW, CH, seed, window_us=t_hi - t_lo, time_window=t_hi - t_lo)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    rep = rng.integers(3, 7, len(t))
    x, y, t, p = (np.repeat(np.asarray(v), rep) for v in (x, y, t, p))
    m = len(t)
    x = x.astype(np.int64) * 2 + rng.integers(0, 2, m)
    y = y.astype(np.int64) * 2 + rng.integers(0, 2, m)
    t = np.int64(T0 + t_lo) + t.astype(np.int64) + rng.integers(0, 3, m)
    o = np.argsort(t, kind="stable")
    return x[o].astype(np.int16), y[o].astype(np.int16), t[o], p[o].astype(np.int8)


def one_event(x, y, t, p):
    return np.array([x], np.int16), np.array([y], np.int16), np.array([T0 + t], np.int64), np.array([p], np.int8)


def push(parts, t_now=None):
    """parts: {lane: (x, y, t, p)} -> one push in lane order."""
    lanes = sorted(parts)
    cat = [np.concatenate([parts[b][k] for b in lanes]) if lanes else np.zeros(0, dt)
           for k, dt in enumerate((np.int16, np.int16, np.int64, np.int8))]
    batch = np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes]) if lanes else np.zeros(0, np.int64)
    return dict(x=cat[0].astype(np.int16), y=cat[1].astype(np.int16), t=cat[2].astype(np.int64), p=cat[3].astype(np.int8),
                batch=batch, t_now=None if t_now is None else np.asarray(t_now, np.int64) + T0)


_SEQ = None


def sequence():
    global _SEQ
    if _SEQ is not None:
        return _SEQ
    E, U = syn.edges_window, syn.uniform_window
    seq = [
        # 0: three lanes of 1500 / 37 / 700 base events in the first 10 ms, no t_now
        push({0: raw_chunk(E, 1500, 1, 0, 10000), 1: raw_chunk(U, 37, 2, 0, 9000), 2: raw_chunk(E, 700, 3, 0, 9500)}),
        # 1: lane 1 only (lanes 0 and 2 are without events and keep their reference instants)
        push({1: raw_chunk(U, 421, 4, 10000, 15000)}),
        # 2: a single raw event, from which nothing survives (its cell was empty; it moves lane 2's clock all the same)
        push({2: one_event(639, 479, 12000, -1)}),
        # 3: an empty push with t_now
        push({}, t_now=[23000] * 3),
        # 4: lanes 0 and 2 on the maps push 0 left behind, t_now given
        push({0: raw_chunk(E, 1203, 1, 23000, 29000), 2: raw_chunk(U, 655, 6, 23500, 29000)}, t_now=[30000] * 3),
        # 5: a jump that expires lanes 0 and 2 entirely; lane 1 stays where it was and receives events
        push({1: raw_chunk(E, 333, 7, 29000, 29900)}, t_now=[55000, 30000, 55000]),
        # 6: all lanes again, no t_now; lane 2 brings one raw event
        push({0: raw_chunk(E, 801, 8, 55000, 60000), 1: raw_chunk(U, 64, 9, 30010, 34000), 2: one_event(300, 7, 56000, 1)}),
        # 7: a jump that expires everything
        push({}, t_now=[200000] * 3),
    ]
    _SEQ = seq
    return seq


def survivors(seq, carry=True):
    """Per push, what ``oracle.downsample.downsample_events`` lets through, lane by lane on the lanes' own change maps
    (chained over the pushes; ``carry=False``: every push on zeroed maps): a list of dicts ``x, y, t, p, batch`` BEFORE the
    row cut, and the final maps [B, CH, CW]."""
    maps = np.zeros((B, CH, CW), np.float32)
    out = []
    for s in seq:
        if not carry:
            maps = np.zeros((B, CH, CW), np.float32)
        parts = []
        for b in range(B):
            m = s["batch"] == b
            ev = {k: s[k][m] for k in ("x", "y", "t", "p")}
            sv, _ = od.downsample_events(ev, H_IN, W_IN, CH, CW, change_map=maps[b])
            parts.append(dict(x=sv["x"].astype(np.int16), y=sv["y"].astype(np.int16), t=sv["t"], p=sv["p"],
                              batch=np.full(len(sv["t"]), b, np.int64)))
        out.append({k: np.concatenate([q[k] for q in parts]) for k in ("x", "y", "t", "p", "batch")})
    return out, maps


_REF = None


def reference():
    """Per push: ``(pos, feat, batch, counts, t_ref list, change maps [B, CH, CW])`` of a plain ``StreamDefinition`` fed the
    oracle's survivors cut to ``x < W, y < H``, with ``t_now[b]`` = the caller's, or the lane's newest raw timestamp."""
    global _REF
    if _REF is not None:
        return _REF
    seq = sequence()
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    maps = np.zeros((B, CH, CW), np.float32)
    newest = [None] * B
    ref = []
    for s in seq:
        parts = []
        for b in range(B):
            m = s["batch"] == b
            ev = {k: s[k][m] for k in ("x", "y", "t", "p")}
            if m.any():
                newest[b] = int(ev["t"][-1])
            q, _ = od.downsample_events(ev, H_IN, W_IN, CH, CW, change_map=maps[b])
            cut = (q["x"] < W) & (q["y"] < H)
            parts.append(dict(x=q["x"][cut].astype(np.int16), y=q["y"][cut].astype(np.int16), t=q["t"][cut], p=q["p"][cut],
                              batch=np.full(int(cut.sum()), b, np.int64)))
        cat = {k: np.concatenate([q[k] for q in parts]) for k in ("x", "y", "t", "p", "batch")}
        t_now = s["t_now"] if s["t_now"] is not None else np.array(newest, np.int64)
        d.push(cat["x"], cat["y"], cat["t"], cat["p"], cat["batch"], t_now=t_now)
        ref.append(d.formatted() + (d.counts(), list(d.t_ref), maps.copy()))
    _REF = ref
    return ref
