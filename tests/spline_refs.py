"""Plain numpy restatements, in float64, of SplineConv as the kernels of csrc/spline_conv.hip, csrc/conv_l0_tiles.hip and
csrc/gemm.hip compute it: the degree-1 open B-spline over 5 taps per axis (the comment above spline_axis in
csrc/common.hpp, from torch_spline_conv), the level-0 offset table, and the conv itself over fixed-stride neighbour
lists (level 0) and over a CSR-by-destination graph (pooled levels).  The GPU tests compare against these;
tests/test_spline_refs_cpu.py pins them to the textbook per-edge form on oracle.ops.spline_basis, so a wrong reference
fails without a GPU.

One step is NOT float64: the offset is divided by ``den`` in fp32, as the kernels and the model do (the pseudo-coordinate
is an fp32 tensor in the reference); everything after that division is float64."""
import numpy as np

TAPS = 5

# (rx, ry, den_x, den_y) of the level-0 tests: the two real geometries (640x480: r = 7, 320x215: r = 4; den = 2 x the
# Cartesian maximum, ev_tgn.py:29), their transposes in tap count, a square one, and den = 2 r, which spans all five taps.
L0_DOMAINS = [
    (7, 7, 32.0, 24.0),        # 3 x 5 taps
    (4, 4, 20.0, 13.4375),     # 3 x 5
    (7, 5, 17.5, 32.0),        # 5 x 3, rx != ry
    (4, 4, 20.0, 20.0),        # 3 x 3
    (7, 7, 14.0, 17.5),        # 5 x 5 (den_x = 2 r: pseudo reaches 0 and 1)
    (3, 3, 6.0, 6.0),          # 5 x 5 on 49 codes
]


def axis(idx, r, den):
    """(k0, k1, b0, b1) of integer offset index ``idx`` in 0..2r: pseudo = (idx - r) / den + 0.5, v = 4 pseudo,
    taps floor(v) % 5 and (floor(v) + 1) % 5 with weights 1 - frac(v) and frac(v)."""
    q = ((np.asarray(idx, np.int64) - int(r)).astype(np.float32) / np.float32(den)).astype(np.float64)
    v = (q + 0.5) * (TAPS - 1)
    fl = np.floor(v)
    frac = v - fl
    f = fl.astype(np.int64)
    return f % TAPS, (f + 1) % TAPS, 1.0 - frac, frac


def tap_window(r, den):
    """(first, count) of the taps that carry a non-zero weight for some offset in 0..2r."""
    k0, k1, b0, b1 = axis(np.arange(2 * r + 1), r, den)
    used = np.concatenate([k0[b0 != 0.0], k1[b1 != 0.0]])
    return int(used.min()), int(used.max() - used.min() + 1)


def _axis_row(idx, r, den):
    """[len(idx), 5] weights per tap."""
    k0, k1, b0, b1 = axis(idx, r, den)
    w = np.zeros((len(k0), TAPS))
    rows = np.arange(len(k0))
    w[rows, k0] += b0
    w[rows, k1] += b1
    return w


def l0_table(rx, ry, den_x, den_y, win):
    """[ncodes, ntp] table of the level-0 kernels: code = ix * (2 ry + 1) + iy, win = (win_x, tx, win_y, ty), the product
    bx[win_x + a] * by[win_y + b] at column a + tx * b, ntp = tx * ty rounded up to 4, padding columns zero."""
    win_x, tx, win_y, ty = win
    sx, sy = 2 * rx + 1, 2 * ry + 1
    bx = _axis_row(np.arange(sx), rx, den_x)[:, win_x:win_x + tx]          # [sx, tx]
    by = _axis_row(np.arange(sy), ry, den_y)[:, win_y:win_y + ty]          # [sy, ty]
    tab = np.zeros((sx * sy, (tx * ty + 3) // 4 * 4))
    tab[:, :tx * ty] = (by[None, :, :, None] * bx[:, None, None, :]).reshape(sx * sy, ty * tx)
    return tab


def _aggregate(T, dst, src, ix, iy, x, rx, ry, den):
    """A[T, 25, cin]: sum over the edges (src -> dst) of basis * x[src] per tap kx + 5 ky."""
    cin = x.shape[1]
    kx0, kx1, bx0, bx1 = axis(ix, rx, den[0])
    ky0, ky1, by0, by1 = axis(iy, ry, den[1])
    at = np.stack([kx0 + TAPS * ky0, kx1 + TAPS * ky0, kx0 + TAPS * ky1, kx1 + TAPS * ky1], 1)
    at = (at + np.asarray(dst, np.int64)[:, None] * TAPS * TAPS).ravel()
    wgt = np.stack([bx0 * by0, bx1 * by0, bx0 * by1, bx1 * by1], 1)
    xj = np.asarray(x, np.float64)[src]
    A = np.empty((T * TAPS * TAPS, cin))
    for c in range(cin):
        A[:, c] = np.bincount(at, weights=(wgt * xj[:, c:c + 1]).ravel(), minlength=T * TAPS * TAPS)
    return A.reshape(T, TAPS * TAPS, cin)


def conv_l0(src, code, deg, x, xskip, W, root, wskip, shift, relu, rx, ry, den):
    """Level-0 conv over fixed-stride neighbour lists src[N, K], code[N, K], of which row n holds deg[n] valid slots
    (slot < deg; the rest is never read).  x[N, cin], xskip[N, cskip] or None, W[25, cin, cout] the full weight tensor,
    root[cin, cout], wskip[cskip, cout] or None, shift[cout]."""
    N, cin = x.shape
    deg = np.asarray(deg, np.int64)
    dst = np.repeat(np.arange(N), deg)
    slot = np.concatenate([np.arange(d) for d in deg]) if len(dst) else np.zeros(0, np.int64)
    e_src, e_code = np.asarray(src)[dst, slot], np.asarray(code)[dst, slot].astype(np.int64)
    sy = 2 * ry + 1
    A = _aggregate(N, dst, e_src, e_code // sy, e_code % sy, x, rx, ry, den)
    x = np.asarray(x, np.float64)
    out = A.reshape(N, -1) @ np.asarray(W, np.float64).reshape(TAPS * TAPS * cin, -1) + x @ np.asarray(root, np.float64)
    if xskip is not None:
        out = out + np.asarray(xskip, np.float64) @ np.asarray(wskip, np.float64)
    out = out + np.asarray(shift, np.float64)
    return np.maximum(out, 0.0) if relu else out


def conv_csr(rowptr, col, code, x, xs, Wm, bias, relu, r, den):
    """Pooled-level conv over a CSR-by-destination graph: code[e] = ix | iy << 16, Wm[26 cin + cskip, N] with rows
    [25 taps x cin | cin root | cskip skip input], ``r`` one radius or (rx, ry), den = (den_x, den_y)."""
    rx, ry = (r, r) if np.isscalar(r) else r
    T = len(rowptr) - 1
    code = np.asarray(code, np.int64)
    dst = np.repeat(np.arange(T), np.diff(rowptr))
    A = _aggregate(T, dst, np.asarray(col, np.int64), code & 0xFFFF, code >> 16, x, rx, ry, den)
    full = [A.reshape(T, -1), np.asarray(x, np.float64)]
    if xs is not None:
        full.append(np.asarray(xs, np.float64))
    out = np.concatenate(full, 1) @ np.asarray(Wm, np.float64)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return np.maximum(out, 0.0) if relu else out
