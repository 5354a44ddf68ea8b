"""Kernel-level parity of the generic level-0 SplineConv, through the C ABI: dagr_spline_tap_window,
dagr_spline_l0_table and all twelve instantiations of dagr_spline_conv_l0 (k_conv_l0<CIN, CSKIP, NT>,
csrc/spline_conv.hip) against the float64 references of tests/spline_refs.py (tests/test_spline_refs_cpu.py vouches
for them).  The engine takes this kernel whenever max_neighbors != 16, the tap window is 5x5 or the level-0 width does
not suit the tiled kernel.

Domains: spline_refs.L0_DOMAINS; their windows come from dagr_spline_tap_window and must give 3x3, 3x5, 5x3 and 5x5.

Bars
  * table: every entry within 4e-6 ABSOLUTE of float64.  A factor lies in [0, 1] and is reached through at most four
    fp32 roundings of quantities of at most 4 (the division, + 0.5, * 4, the subtraction of the floor): < 4 * 2^-22 =
    9.5e-7 per factor, and an entry is a product of two factors, each <= 1.  Padding columns and the taps the float64
    table leaves at zero are exactly 0.0; every row sums to 1 within the same bound.
  * conv: max abs error <= 1e-4 of max(1, max|want|), the bar of tests/test_conv_l0_tiles_gpu.py.

Conv cases (cin, cskip) x domain -> ntaps, K, N, relu; every instantiation once, the K / N / degree edges spread:
    (3, 0)    dom 3 ->  9   K  8  N    17  relu 1        (16, 3)   dom 3 ->  9   K 32  N  3001  relu 0
    (3, 0)    dom 0 -> 15   K 16  N  3001  relu 0        (16, 3)   dom 2 -> 15   K 24  N    17  relu 1
    (3, 0)    dom 5 -> 25   K 24  N     1  relu 1        (16, 3)   dom 4 -> 25   K 16  N  3001  relu 1
    (19, 0)   dom 3 ->  9   K 16  N  3001  relu 1        (16, 19)  dom 3 ->  9   K 16  N     1  relu 0
    (19, 0)   dom 1 -> 15   K 32  N    17  relu 0        (16, 19)  dom 0 -> 15   K 32  N  3001  relu 1
    (19, 0)   dom 4 -> 25   K 32  N  3001  relu 1        (16, 19)  dom 5 -> 25   K  8  N    17  relu 0
    (16, 3)   dom 2 -> 15   K 16  N 40000  relu 1   persistent grid: more node groups than the grid holds
K = 24 and 32 send the 16-slot loop through a second step.  Degrees are drawn from 0..K; the first rows are planted with
degree K, 0, 1, 17, 16, 15 (those <= K, as many as N holds: all of them from N = 17 on).  Slots past the degree hold valid
random sources and codes, which the reference ignores; a kernel that reads them computes wrong values.  Input rows are
padded (ldx = cin rounded up to 4, plus 4; ldskip likewise) with random padding; the output has ldo = 20 and is preset to
a sentinel that columns 16..19 must keep bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spline_refs as sr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)
TABLE_BAR = 4e-6


def _c_window(L, r, den):
    lo, cnt = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.dagr_spline_tap_window(r, den, ctypes.byref(lo), ctypes.byref(cnt)) == 0
    return lo.value, cnt.value


def _kernel_window(L, r, den):
    """The engine's choice (engine.py): a 3-tap window clamped into the 5-tap kernel, else all five."""
    lo, cnt = _c_window(L, r, den)
    return (min(lo, 2), 3) if cnt <= 3 else (0, 5)


def _win(L, dom):
    rx, ry, den_x, den_y = dom
    return _kernel_window(L, rx, den_x) + _kernel_window(L, ry, den_y)


def _table(L, dom, win, dev):
    """(tab[ncodes, ntp] on the device, bad flag) of dagr_spline_l0_table; the buffer is preset to NaN."""
    from dagr_amd import _lib
    rx, ry, den_x, den_y = dom
    ncodes, ntp = (2 * rx + 1) * (2 * ry + 1), (win[1] * win[3] + 3) // 4 * 4
    tab = torch.full((ncodes, ntp), float("nan"), dtype=torch.float32, device=dev)
    bad = torch.full((1,), 77, dtype=torch.int32, device=dev)
    _lib.check(L.dagr_spline_l0_table(rx, ry, den_x, den_y, win[0], win[1], win[2], win[3], _lib.ptr(tab), _lib.ptr(bad),
                                      _lib.cur_stream(dev)), "l0_table")
    torch.cuda.synchronize()
    return tab, int(bad.item())


def test_domains_cover_the_four_window_forms():
    from dagr_amd import _lib
    L = _lib.lib()
    forms = set()
    for dom in sr.L0_DOMAINS:
        w = _win(L, dom)
        forms.add((w[1], w[3]))
    assert forms == {(3, 3), (3, 5), (5, 3), (5, 5)}
    assert {tx * ty for tx, ty in forms} == {9, 15, 25}
    assert (7, 7, 32.0, 24.0) in sr.L0_DOMAINS and (4, 4, 20.0, 13.4375) in sr.L0_DOMAINS      # the two real geometries
    assert any(d[0] != d[1] for d in sr.L0_DOMAINS)


@pytest.mark.parametrize("dom", sr.L0_DOMAINS)
def test_tap_window_matches_float64(dom):
    from dagr_amd import _lib
    L = _lib.lib()
    rx, ry, den_x, den_y = dom
    assert _c_window(L, rx, den_x) == sr.tap_window(rx, den_x)
    assert _c_window(L, ry, den_y) == sr.tap_window(ry, den_y)


@pytest.mark.parametrize("dom", sr.L0_DOMAINS)
def test_l0_table_matches_float64(dom):
    from dagr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    win = _win(L, dom)
    tab, bad = _table(L, dom, win, dev)
    assert bad == 0
    got = tab.cpu().numpy()
    want = sr.l0_table(*dom, win)
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"l0_table {dom}: window {win}, max abs error {err:.3e}")
    assert err <= TABLE_BAR, err
    assert (got[want == 0.0] == 0.0).all()                   # padding columns and zero-weight taps: exactly zero
    assert (got[:, win[1] * win[3]:] == 0.0).all()
    assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= TABLE_BAR


def test_l0_table_flags_a_window_that_is_too_narrow():
    """den = 2 r spans all five taps: a 4-tap window on either side of either axis loses a weighted tap."""
    from dagr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    dom = (3, 3, 6.0, 6.0)
    assert _win(L, dom) == (0, 5, 0, 5)
    assert _table(L, dom, (0, 5, 0, 5), dev)[1] == 0
    for win in [(0, 4, 0, 5), (1, 4, 0, 5), (0, 5, 0, 4), (0, 5, 1, 4)]:
        assert _table(L, dom, win, dev)[1] != 0, win
    # a 3-tap domain with the window shifted off its first tap
    dom = (4, 4, 20.0, 20.0)
    assert _win(L, dom) == (1, 3, 1, 3)
    assert _table(L, dom, (2, 3, 1, 3), dev)[1] != 0
    assert _table(L, dom, (1, 3, 0, 3), dev)[1] != 0
    assert _table(L, dom, (1, 3, 1, 3), dev)[1] == 0


def test_l0_table_rejects_bad_arguments():
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    tab = torch.zeros((49, 40), dtype=torch.float32, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    S = _lib.cur_stream(dev)
    assert L.dagr_spline_l0_table(3, 3, 6.0, 6.0, 0, 6, 0, 5, P(tab), P(bad), S) != 0           # tx > 5
    assert b"bad tap window" in L.dagr_last_error()
    assert L.dagr_spline_l0_table(3, 3, 6.0, 6.0, 3, 3, 0, 5, P(tab), P(bad), S) != 0           # win_x + tx > 5
    assert b"bad tap window" in L.dagr_last_error()
    assert L.dagr_spline_l0_table(3, 3, 6.0, 6.0, 0, 5, 2, 4, P(tab), P(bad), S) != 0           # win_y + ty > 5
    assert b"bad tap window" in L.dagr_last_error()
    assert L.dagr_spline_l0_table(3, 3, 6.0, 6.0, 0, 5, 0, 5, None, P(bad), S) != 0
    assert b"bad arguments" in L.dagr_last_error()
    assert L.dagr_spline_l0_table(3, 3, 6.0, 6.0, 0, 5, 0, 5, P(tab), None, S) != 0
    assert b"bad arguments" in L.dagr_last_error()
    torch.cuda.synchronize()
    assert bool((tab == 0).all())


def _pad4(c):
    return (c + 3) // 4 * 4 + 4 if c else 0


def _run_case(cin, cskip, dom, K, N, relu):
    """One dagr_spline_conv_l0 call on random lists; returns (got[N, 20], want[N, 16], ntaps, deg)."""
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    rx, ry, den_x, den_y = dom
    win = _win(L, dom)
    (wx0, tx, wy0, ty) = win
    ntaps = tx * ty
    ncodes = (2 * rx + 1) * (2 * ry + 1)
    rng = np.random.default_rng(N * 7 + cin * 131 + cskip * 17 + K)
    deg = rng.integers(0, K + 1, size=N).astype(np.int32)
    planted = [d for d in (K, 0, 1, 17, 16, 15) if d <= K][:N]
    deg[:len(planted)] = planted
    src = rng.integers(0, N, size=(N, K)).astype(np.int32)              # valid in every slot, used or not
    code = rng.integers(0, ncodes, size=(N, K)).astype(np.int16)
    ldx, ldskip = _pad4(cin), _pad4(cskip)
    x = rng.standard_normal((N, ldx)).astype(np.float32)
    xs = rng.standard_normal((N, ldskip)).astype(np.float32) if cskip else None
    W = (rng.standard_normal((25, cin, 16)) * 0.3).astype(np.float32)
    root = (rng.standard_normal((cin, 16)) * 0.3).astype(np.float32)
    wskip = (rng.standard_normal((cskip, 16)) * 0.3).astype(np.float32) if cskip else None
    shift = rng.standard_normal(16).astype(np.float32)
    rows = [W[(wx0 + a) + 5 * (wy0 + b)] for b in range(ty) for a in range(tx)] + [root] + ([wskip] if cskip else [])
    wpack = np.concatenate(rows, 0).astype(np.float32)
    assert wpack.shape == ((ntaps + 1) * cin + cskip, 16)
    want = sr.conv_l0(src, code, deg, x[:, :cin], xs[:, :cskip] if cskip else None, W, root, wskip, shift, relu, rx, ry,
                      (den_x, den_y))
    tab, bad = _table(L, dom, win, dev)
    assert bad == 0
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_src, d_code, d_deg, d_x, d_w, d_s = T(src), T(code), T(deg), T(x), T(wpack), T(shift)
    d_xs = T(xs) if cskip else None
    out = torch.full((N, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    _lib.check(L.dagr_spline_conv_l0(cin, cskip, ntaps, N, K, ncodes, P(d_src), P(d_code), P(d_deg), P(d_x), ldx, P(d_xs),
                                     ldskip, P(tab), P(d_w), P(d_s), 1 if relu else 0, P(out), 20, _lib.cur_stream(dev)),
               "conv_l0")
    torch.cuda.synchronize()
    return out.cpu().numpy(), want, ntaps, deg


def _assert_case(got, want, label):
    assert np.array_equal(got[:, 16:].view(np.int32), np.full((len(got), 4), SENTINEL).view(np.int32)), label
    assert np.isfinite(got[:, :16]).all(), label
    err = np.abs(got[:, :16].astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
    print(f"conv_l0 {label}: max abs error / scale = {err:.3e}")
    assert err <= 1e-4, (label, err)


CASES = [  # cin, cskip, domain index, ntaps expected, K, N, relu
    (3, 0, 3, 9, 8, 17, 1),
    (3, 0, 0, 15, 16, 3001, 0),
    (3, 0, 5, 25, 24, 1, 1),
    (16, 3, 3, 9, 32, 3001, 0),
    (16, 3, 2, 15, 24, 17, 1),
    (16, 3, 4, 25, 16, 3001, 1),
    (19, 0, 3, 9, 16, 3001, 1),
    (19, 0, 1, 15, 32, 17, 0),
    (19, 0, 4, 25, 32, 3001, 1),
    (16, 19, 3, 9, 16, 1, 0),
    (16, 19, 0, 15, 32, 3001, 1),
    (16, 19, 5, 25, 8, 17, 0),
]


def test_cases_cover_every_instantiation_and_edge():
    assert {(c[0], c[1], c[3]) for c in CASES} == {(ci, cs, nt) for ci, cs in ((3, 0), (16, 3), (19, 0), (16, 19))
                                                    for nt in (9, 15, 25)}
    assert {c[4] for c in CASES} == {8, 16, 24, 32} and {c[5] for c in CASES} == {1, 17, 3001}
    assert {c[6] for c in CASES} == {0, 1}
    for ci, cs in ((3, 0), (16, 3), (19, 0), (16, 19)):      # every width runs the slot loop once and twice
        ks = {c[4] for c in CASES if (c[0], c[1]) == (ci, cs)}
        assert min(ks) <= 16 < max(ks)


@pytest.mark.parametrize("cin,cskip,dom,ntaps,K,N,relu", CASES)
def test_conv_l0_matches_float64(cin, cskip, dom, ntaps, K, N, relu):
    got, want, nt, deg = _run_case(cin, cskip, sr.L0_DOMAINS[dom], K, N, relu)
    assert nt == ntaps
    if N >= 17:
        assert {0, 1, K}.issubset(set(deg.tolist())) and (K < 17 or {15, 16, 17}.issubset(set(deg.tolist())))
    _assert_case(got, want, (cin, cskip, ntaps, K, N, relu))


def test_conv_l0_persistent_grid():
    """N = 40 000: persistent_grid launches at most 256 CUs x 4 workgroups x 16 node groups = 16 384 groups, so every
    group walks its grid-stride loop more than once (and the eight XCD chunks of xcd_split are all in use)."""
    got, want, nt, _ = _run_case(16, 3, sr.L0_DOMAINS[2], 16, 40000, 1)
    assert nt == 15
    _assert_case(got, want, (16, 3, 15, 16, 40000, 1))


def test_conv_l0_rejects_unsupported_widths():
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    S = _lib.cur_stream(dev)
    for cin, cskip, ntaps in [(5, 0, 9), (16, 4, 15), (3, 0, 12)]:
        rc = L.dagr_spline_conv_l0(cin, cskip, ntaps, 1, 8, 9, P(z), P(z), P(z), P(f), 8, P(f), 8, P(f), P(f), P(f), 1, P(f),
                                   16, S)
        assert rc != 0 and b"unsupported" in L.dagr_last_error(), (cin, cskip, ntaps)
    torch.cuda.synchronize()
    assert bool((f == 0).all())
