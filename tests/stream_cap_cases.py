"""Cases of the capped event stream (``max_lane_events``), shared by tests/test_stream_cap_cpu.py and
tests/test_stream_cap_gpu.py: a brute-force restatement of the capped window that keeps every event ever pushed, the
scripted sequences, and the synthetic N-Caltech101 recording.

Shapes as in tests/test_streaming_gpu.py: B = 3 lanes on 320x215, absolute timestamps from 2^33 us on."""
import numpy as np

from dagr_amd.utils import synthetic as syn

W, H, B = 320, 215, 3
TW = 1000000
WINDOW_US = 20000
T0 = (1 << 33) + 777
N_STAGE = 257           # the cap of the staging sequence: no multiple of the 256-thread block
N_MODEL = 300           # the cap of the model-level tests


def chunk(gen, n, seed, t_lo, t_hi, width=W, height=H):
    """n events of a synthetic stream with T0 + t_lo <= t <= T0 + t_hi (sorted, int64)."""
    x, y, t, p = gen(n, width, height, seed, window_us=t_hi - t_lo, time_window=t_hi - t_lo)
    return x, y, np.int64(T0 + t_lo) + t.astype(np.int64), p


def push(parts, t_now=None):
    """parts: {lane: (x, y, t, p)} -> one push in lane order (t_now relative to T0)."""
    lanes = sorted(parts)
    cat = [np.concatenate([parts[b][k] for b in lanes]) if lanes else np.zeros(0, dt)
           for k, dt in enumerate((np.int16, np.int16, np.int64, np.int8))]
    batch = np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes]) if lanes else np.zeros(0, np.int64)
    return dict(x=cat[0].astype(np.int16), y=cat[1].astype(np.int16), t=cat[2].astype(np.int64), p=cat[3].astype(np.int8),
                batch=batch, t_now=None if t_now is None else np.asarray(t_now, np.int64) + T0)


class BruteForce:
    """The capped window restated without a running window: every event ever pushed to a lane is kept; the window is the
    time rule applied to all of them, then the last N.  ``dropped`` is counted on sets of event indices: an event counts
    once, at the first step at which it passes the time rule but is not among the last N that do.  Well-formed pushes
    only (no checks)."""

    def __init__(self, batch_size, window_us, max_lane_events, time_window=TW):
        self.B, self.window_us, self.N, self.time_window = batch_size, window_us, max_lane_events, time_window
        self.all = [dict(x=np.zeros(0, np.int16), y=np.zeros(0, np.int16), t=np.zeros(0, np.int64), p=np.zeros(0, np.int8))
                    for _ in range(batch_size)]
        self.t_ref = [None] * batch_size
        self.cut = [set() for _ in range(batch_size)]

    def push(self, x, y, t, p, batch=None, t_now=None):
        x, y, t, p = np.asarray(x, np.int16), np.asarray(y, np.int16), np.asarray(t, np.int64), np.asarray(p, np.int8)
        batch = np.zeros(len(t), np.int64) if batch is None else np.asarray(batch, np.int64)
        if t_now is not None:
            t_now = np.broadcast_to(np.asarray(t_now, np.int64).reshape(-1), (self.B,))
        for b in range(self.B):
            m = batch == b
            lane = self.all[b]
            for k, v in (("x", x), ("y", y), ("t", t), ("p", p)):
                lane[k] = np.concatenate([lane[k], v[m]])
            if t_now is not None:
                self.t_ref[b] = int(t_now[b])
            elif len(lane["t"]):
                self.t_ref[b] = int(lane["t"].max())
            self.cut[b] |= set(self._valid(b)[:-self.N].tolist()) if self.N is not None else set()

    def _valid(self, b):
        """Indices (arrival order) of the lane's events that pass the time rule now."""
        if self.t_ref[b] is None:
            return np.zeros(0, np.int64)
        age = self.t_ref[b] - self.all[b]["t"]
        return np.flatnonzero((age >= 0) & (age < self.window_us))

    def lane_window(self, b):
        idx = self._valid(b)
        idx = idx if self.N is None else idx[-self.N:]
        lane = self.all[b]
        t_rel = (self.time_window - (self.t_ref[b] - lane["t"][idx])).astype(np.int32) if len(idx) else np.zeros(0, np.int32)
        return lane["x"][idx], lane["y"][idx], t_rel, lane["p"][idx]

    def window(self):
        lanes = [self.lane_window(b) for b in range(self.B)]
        counts = [len(l[0]) for l in lanes]
        return tuple(np.concatenate([l[k] for l in lanes]) for k in range(4)) + \
            (np.repeat(np.arange(self.B, dtype=np.int64), counts),)

    def dropped(self):
        return np.array([len(c) for c in self.cut], np.int64)


def same_window(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


_STAGE_SEQ = None


def stage_sequence():
    """The scripted sequence of the staging test, N = 257, capacity B * N = 771, WINDOW_US = 20 ms:

    0  lanes of 200 / 37 / 150 events in the first 5 ms: all under N
    1  lane 0 +150 (350 > N: cut inside its survivors), lane 2 +50; lane 1 stays under N for the whole sequence
    2  lane 2 alone receives 400 > N: none of its survivors stays and the front of the push goes too
    3  lane 0 +120 with t_now = 24.5 ms: in lane 0 the time rule AND the count rule remove events; the push is empty in
       lanes 1 and 2, where t_now expires lane 1 entirely
    4  an empty push, t_now = 28 ms: the time rule removes events of lanes 0 and 2 (the count rule cannot remove any from
       a lane that receives nothing: what it held was within N already -- test_stream_cap_gpu.py has that case across an
       uncapped step)
    5  500 + 20 + 400 = 920 events: larger than the whole capacity
    6  300 events for lane 0 on five timestamps: the count cut falls between events of equal t
    7  a jump that expires everything"""
    global _STAGE_SEQ
    if _STAGE_SEQ is not None:
        return _STAGE_SEQ
    E, U = syn.edges_window, syn.uniform_window
    seq = [push({0: chunk(E, 200, 1, 0, 5000), 1: chunk(U, 37, 2, 0, 4000), 2: chunk(E, 150, 3, 0, 4500)})]
    seq.append(push({0: chunk(E, 150, 4, 5000, 8000), 2: chunk(U, 50, 5, 4500, 7000)}))
    seq.append(push({2: chunk(E, 400, 6, 7000, 9000)}))
    seq.append(push({0: chunk(U, 120, 7, 22000, 24000)}, t_now=[24500] * 3))
    seq.append(push({}, t_now=[28000] * 3))
    seq.append(push({0: chunk(E, 500, 8, 28000, 30000), 1: chunk(U, 20, 9, 28000, 29000), 2: chunk(U, 400, 10, 28000, 29500)}))
    x, y, _, p = chunk(U, 300, 11, 0, 1000)
    seq.append(push({0: (x, y, T0 + 31000 + np.arange(300, dtype=np.int64) // 60, p)}))
    seq.append(push({}, t_now=[200000] * 3))
    _STAGE_SEQ = seq
    return seq


def burst_sequence(burst):
    """The model-level sequence, N = 300, WINDOW_US = 20 ms: six pushes of about 100 to 450 events per lane and step, so
    that lanes 0 and 2 run into the cap; with ``burst`` push 3 also brings 5 000 events to lane 1 (inside the 2 ms of the
    push, so that every later timestamp of lane 1 is the same in both sequences)."""
    E, U = syn.edges_window, syn.uniform_window
    seq = []
    for k, sizes in enumerate(((450, 90, 210), (130, 40, 0), (0, 31, 120), (97, 60, 301), (220, 0, 45), (160, 75, 90))):
        t = 2000 * k
        parts = {b: chunk(E if b != 1 else U, n, 40 + 3 * k + b, t, t + 1500) for b, n in enumerate(sizes) if n}
        if burst and k == 3:
            a, extra = parts[1], chunk(U, 5000, 99, t + 1500, t + 1900)
            parts[1] = tuple(np.concatenate([u, v]) for u, v in zip(a, extra))
        seq.append(push(parts, t_now=[t + 2000] * 3))
    return seq


def recording(n=3000, seed=5, width=240, height=180):
    """A synthetic N-Caltech101 recording: n events over 300 ms on the 240 x 180 sensor, p in {-1, +1}, with runs of
    equal timestamps."""
    x, y, t, p = syn.edges_window(n, width, height, seed, window_us=300000, time_window=300000)
    t = (t.astype(np.int64) // 7) * 7 + T0
    return dict(x=x, y=y, t=t, p=p)


def write_recording(root, rec):
    """The recording as the one sample of a stand-in N-Caltech101 tree (``.npz`` files, ``reader=np.load``)."""
    (root / "training" / "airplanes").mkdir(parents=True)
    (root / "annotations" / "airplanes").mkdir(parents=True)
    np.savez(root / "training" / "airplanes" / "image_0001.npz", **rec)
    np.array([0, 0, 10, 20, 110, 20, 110, 90, 10, 90, 0, 0], dtype=np.int16).tofile(
        root / "annotations" / "airplanes" / "annotation_0001.bin")


def ncaltech_sample(root, num_events):
    from dagr_amd.data.ncaltech101_data import NCaltech101
    ds = NCaltech101(root, "training", transform=None, num_events=num_events, reader=lambda p: np.load(p), suffix=".npz")
    return ds, ds[0]
