"""dagr_sample_features (csrc/sample.hip) called directly, on each of its six instantiations -- batch index int32 / int64
x {4 channels a thread with float4 accesses, 4 channels a thread with scalar accesses, 1 channel a thread} -- at batch
sizes where the depth index is and is not an integer, on 1x1 and odd maps, at and past the map's edge.

Which kernel a layout (C, ldo, coff) selects (dagr_sample_features: four = C % 4 == 0, aligned = four and ldo % 4 == 0
and coff % 4 == 0, both with 16-byte aligned bases, which torch's allocations are):
    (16, 32, 16)            k_sample_features<BatchT, 4, true>      the pooled levels' skip columns
    (16, 19, 3)             k_sample_features<BatchT, 4, false>     level 0's own input matrix
    (3, 5, 1), (6, 9, 2)    k_sample_features<BatchT, 1, false>

Reference (tests/kernel_refs.py, pinned on the CPU to oracle.model.sample_features): coordinates and the eight corner
weights in np.float32 in the kernel's documented order -- every step one rounded operation, none a multiply feeding an add,
so nothing there can be contracted -- and sum(w_i * f_i) in float64.  Bars:
    |got - ref| <= 2^-20 * sum |w_i * f_i| + 1e-30        (eight products and eight adds, or eight FMAs, each rounded at 2^-24
                                                           of at most sum |w_i * f_i|: under 2^-20 with a margin below 2)
    |got - oracle.model.sample_features| <= 1e-5 * max(1, max |feat|)      (the bar the engine tests hold)
Features are finite: the kernel's skip of zero-weight taps is documented and not under test."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from oracle import model as om
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
LAYOUTS = [(16, 32, 16), (16, 19, 3), (3, 5, 1), (6, 9, 2)]
MAPS = [(1, 1), (2, 3), (54, 80)]
SENSORS = [(320, 215), (640, 480)]
GUARD = 128          # rows kept after n_max in every per-node array


def _positions(W, H, n, seed):
    """[n, 3] float32: the sensor's corners, edge midpoints and centre as x / W; pos = 1.0 and a slightly negative
    position on either axis (both past the map: zero padding); integer pixels; subpixel values as pooled levels have."""
    r = np.random.default_rng(seed)
    xs, ys = [0.0, (W // 2) / W, (W - 1) / W], [0.0, (H // 2) / H, (H - 1) / H]
    fixed = [(x, y) for x in xs for y in ys]
    fixed += [(1.0, 1.0), (1.0, 0.5), (0.5, 1.0), (-1e-4, 0.5), (0.5, -1e-4), (-1e-4, -1e-4), (1.0, -1e-4)]
    p = np.empty((n, 3), np.float32)
    p[:, 0] = r.uniform(0, (W - 1) / W, n)
    p[:, 1] = r.uniform(0, (H - 1) / H, n)
    p[::2, 0] = r.integers(0, W, len(p[::2])) / W
    p[::2, 1] = r.integers(0, H, len(p[::2])) / H
    p[:, 2] = r.uniform(0, 1, n)
    k = min(n, len(fixed))
    p[:k, :2] = np.asarray(fixed[:k], np.float32)
    return p


def _case(B, h, w, C, W, H, n, seed):
    r = np.random.default_rng(seed)
    pos = _positions(W, H, n + GUARD, seed)
    batch = r.integers(0, B, n + GUARD)
    batch[:2 * B] = np.repeat(np.arange(B), 2)[:n + GUARD]
    feat = (r.standard_normal((B, h, w, C)) * 3).astype(np.float32)
    return pos, batch, feat


def _run(pos, batch, batch_dtype, feat, W, H, n_max, ldo, coff, count=None):
    """out[n_max + GUARD, ldo] after the call (pre-filled with the sentinel); the inputs are checked to be unchanged."""
    B, h, w, C = feat.shape
    dpos = torch.from_numpy(pos).cuda()
    dbatch = torch.from_numpy(batch.astype(batch_dtype)).cuda()
    dfeat = torch.from_numpy(feat).cuda()
    dcount = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    out = torch.full((n_max + GUARD, ldo), SENTINEL, dtype=torch.float32, device="cuda")
    rc = _lib.lib().dagr_sample_features(_lib.ptr(dcount), n_max, _lib.ptr(dpos), _lib.ptr(dbatch),
                                         1 if batch_dtype == np.int64 else 0, _lib.ptr(dfeat), B, h, w, C, W, H,
                                         _lib.ptr(out), ldo, coff, _lib.cur_stream(torch.device("cuda:0")))
    assert rc == 0, _lib.lib().dagr_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(dpos.cpu().numpy(), pos) and np.array_equal(dfeat.cpu().numpy(), feat)
    assert np.array_equal(dbatch.cpu().numpy(), batch.astype(batch_dtype))
    if dcount is not None:
        assert int(dcount.cpu()) == count
    return got


def _check(got, n_rows, pos, batch, feat, W, H, coff, what):
    """Rows [0, n_rows) hold the samples in [coff, coff + C); every other element of ``got`` holds the sentinel."""
    C = feat.shape[3]
    ref, mag = kr.sample_features(pos[:n_rows], batch[:n_rows], feat, W, H, coord_dtype=np.float32)
    block = got[:n_rows, coff:coff + C]
    rest = got.copy()
    rest[:n_rows, coff:coff + C] = SENTINEL
    assert np.all(rest == SENTINEL), f"{what}: written outside rows [0, {n_rows}) x columns [{coff}, {coff + C})"
    if n_rows == 0:
        return
    err = np.abs(block - ref)
    assert np.all(err <= 2.0 ** -20 * mag + 1e-30), f"{what}: {float((err / (2.0 ** -20 * mag + 1e-30)).max())} x the bound"
    want = om.sample_features(torch.from_numpy(pos[:n_rows]), torch.from_numpy(batch[:n_rows].astype(np.int64)),
                              torch.from_numpy(feat).permute(0, 3, 1, 2), W, H).numpy()
    assert float(np.abs(block - want).max()) <= 1e-5 * max(1.0, float(np.abs(feat).max())), what


@pytest.mark.parametrize("batch_dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda t: "C%d_ldo%d_coff%d" % t)
@pytest.mark.parametrize("B", [1, 2, 3, 4, 7, 8])
def test_every_instantiation_at_every_batch_size_map_and_sensor(batch_dtype, layout, B):
    C, ldo, coff = layout
    n = 300
    for h, w in MAPS:
        for W, H in SENSORS:
            pos, batch, feat = _case(B, h, w, C, W, H, n, seed=B * 1000 + h * 10 + W)
            got = _run(pos, batch, batch_dtype, feat, W, H, n, ldo, coff)
            _check(got, n, pos, batch, feat, W, H, coff, f"B={B} map={h}x{w} sensor={W}x{H} layout={layout}")


def test_depth_index_misses_the_integer_at_seven_and_eight_samples():
    """What the larger batch sizes are in the list for: 2b / (B - 1) - 1 is rounded from B = 4 on.  At B = 4 the later steps
    round it back onto the integer; at B = 7 sample 1 lands 2^-23 above it and at B = 8 2^-24 BELOW it (floor gives plane 0,
    with weight 2^-24, and plane 1 the rest): both depth planes are read -- in the reference as in the kernel."""
    for B, off in ((1, []), (2, []), (3, []), (4, []), (7, [2.0 ** -23]), (8, [-2.0 ** -24])):
        b = np.arange(B, dtype=np.float32)
        g = (np.float32(2) * b) / np.float32(max(B, 2) - 1) - np.float32(1)
        iz = ((g + np.float32(1)) / np.float32(2)) * np.float32(B - 1)
        assert (iz - b)[iz != b].tolist() == off, (B, iz)


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("layout", [(16, 32, 16), (16, 19, 3), (6, 9, 2)], ids=lambda t: "C%d_ldo%d_coff%d" % t)
def test_node_counts_and_the_device_side_count(n, layout):
    """n_max around the 256-thread block; n_ptr NULL, below n_max (rows beyond it stay) and above it (clamped)."""
    C, ldo, coff = layout
    B, h, w, W, H = 3, 7, 9, 320, 215
    pos, batch, feat = _case(B, h, w, C, W, H, n, seed=n)
    for count, rows in ((None, n), (n // 2, n // 2), (n + 100, n)):
        got = _run(pos, batch, np.int32, feat, W, H, n, ldo, coff, count=count)
        _check(got, rows, pos, batch, feat, W, H, coff, f"n_max={n} count={count} layout={layout}")
