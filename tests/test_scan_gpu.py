"""The int32 exclusive prefix sum (csrc/scan.hip) called on its own through dagr_exclusive_scan_i32, at sizes on both sides
of every threshold of its dispatch.  Bar: BIT-EQUAL to np.cumsum in int64, shifted by one (tests/kernel_refs.py).

Which code a size selects (exclusive_scan_i32 / exclusive_scan_i32_chained; a tile is 2048 entries):

    chained = 0     n <= 65 536                     scan_single_block               1 .. 65 536
                    beyond                          reduce / scan of sums / apply   65 537 .. 10 498 105
    chained = 1     n <= 320 tiles = 655 360        scan_chained                    1 .. 655 360
                    n <= 320 * 1024 *  8            scan_chained_wide<1024,  8>     655 361, 2 621 440
                    n <= 320 * 1024 * 16            scan_chained_wide<1024, 16>     2 621 441, 5 242 880
                    n <= 320 * 1024 * 32            scan_chained_wide<1024, 32>     5 242 881, 10 485 760
                    beyond                          scan_chained_wide<1024, 48>     10 485 761, 10 498 105

(the per-pixel offsets of a 1280x720 sensor at B = 8 are 7 372 801 entries: EPT 32; VGA at B = 16 is 4 915 201: EPT 16).
Left out: the chained entry's own fallback to the three-launch form beyond 2048 tiles of 1024 x 48 (n > 100 M, 400 MB a
buffer), and the wrap of the 24-bit launch tag (16 M launches).

The chained kernels spin on their predecessors' words: a wrong look-back shows as a hang, not as a failure, so this file is
to be run under a time limit of its own."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537, 655360, 655361, 2621440, 2621441,
         5242880, 5242881, 10485760, 10485761, 10498105]
N_MAX = max(SIZES)
GUARD = 16            # entries kept after n in every buffer
SENTINEL = -7


def _sparse(n):
    """Up to 61 large values, anywhere in the array, whose total is exactly 2^31 - 1."""
    r = np.random.default_rng(n)
    k = min(n, 61)
    v = np.zeros(n, np.int32)
    where = r.choice(n, k, replace=False)
    v[where] = (2 ** 31 - 1) // k
    v[where[0]] += (2 ** 31 - 1) % k
    assert int(v.sum(dtype=np.int64)) == 2 ** 31 - 1
    return v


@pytest.fixture(scope="module")
def shared():
    """Inputs of N_MAX entries and their scans, on the device, made once: the scan of a prefix is the prefix of the scan.
    Never written (the calls that write their input get a copy)."""
    r = np.random.default_rng(0)
    out = {}
    for kind, v in (("zeros", np.zeros(N_MAX, np.int32)), ("ones", np.ones(N_MAX, np.int32)),
                    ("random", r.integers(0, 16, N_MAX).astype(np.int32))):
        ref = kr.exclusive_scan(v)
        assert int(ref[-1]) + int(v[-1]) < 2 ** 31
        out[kind] = (torch.from_numpy(v).cuda(), torch.from_numpy(ref.astype(np.int32)).cuda())
    return out


def _buffers(n, chained):
    L = _lib.lib()
    nbytes = int(L.dagr_scan_chained_state_bytes(n)) if chained else 4 * int(L.dagr_scan_scratch_elems(n))
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def _scan(src, dst, n, scratch, chained, zero_input):
    rc = _lib.lib().dagr_exclusive_scan_i32(_lib.ptr(src), _lib.ptr(dst), n, _lib.ptr(scratch), scratch.numel(),
                                            1 if chained else 0, 1 if zero_input else 0,
                                            _lib.cur_stream(torch.device("cuda:0")))
    assert rc == 0, _lib.lib().dagr_last_error()


def _guarded(v):
    """A writable copy of v followed by GUARD sentinels."""
    buf = torch.full((v.numel() + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    buf[:v.numel()] = v
    return buf


def _three_forms(v, ref, n, scratch, chained, what):
    """The forms the product uses, one after the other on the same scratch / chained state."""
    # out of place, the input kept
    src, dst = _guarded(v), torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    _scan(src, dst, n, scratch, chained, False)
    assert torch.equal(dst[:n], ref), f"{what}: out of place"
    assert bool((dst[n:] == SENTINEL).all()), f"{what}: written past n"
    assert torch.equal(src[:n], v) and bool((src[n:] == SENTINEL).all()), f"{what}: the input was written"
    # out of place, the input cleared
    dst.fill_(SENTINEL)
    _scan(src, dst, n, scratch, chained, True)
    assert torch.equal(dst[:n], ref), f"{what}: zero_input"
    assert bool((dst[n:] == SENTINEL).all()), f"{what}: written past n"
    assert not bool(src[:n].any()), f"{what}: the input is not all zero afterwards"
    assert bool((src[n:] == SENTINEL).all()), f"{what}: cleared past n"
    # in place
    buf = _guarded(v)
    _scan(buf, buf, n, scratch, chained, False)
    assert torch.equal(buf[:n], ref), f"{what}: in place"
    assert bool((buf[n:] == SENTINEL).all()), f"{what}: written past n"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("chained", [0, 1], ids=["launches", "chained"])
def test_scan_is_bit_equal_to_cumsum(shared, chained, n):
    """Four kinds of values x three forms = twelve consecutive calls on one scratch; with chained = 1 that is one state,
    zeroed once, re-armed by the last ticket of every launch."""
    scratch = _buffers(n, chained)
    for kind, (v, ref) in shared.items():
        _three_forms(v[:n], ref[:n], n, scratch, chained, f"n={n} {kind}")
    v = _sparse(n)
    ref = kr.exclusive_scan(v)
    assert int(ref.max()) < 2 ** 31
    _three_forms(torch.from_numpy(v).cuda(), torch.from_numpy(ref.astype(np.int32)).cuda(), n, scratch, chained,
                 f"n={n} sparse")


def test_one_chained_state_serves_every_size_in_turn(shared):
    """The state is zeroed once, sized for the largest n; then three calls of one size and calls that alternate across every
    path boundary.  Each launch must find the ticket counter re-armed and must not take a word of an earlier launch
    (other tile width, other tag) for one of its own."""
    v, ref = shared["random"]
    state = _buffers(N_MAX, 1)
    dst = torch.full((N_MAX + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    order = [2621441] * 3 + [2049, 655361, 655360, 2621441, 1, 5242881, 2621440, 10485761, 65, 5242880, 10498105, 10485760,
                             2048, 655361, 10485761, 655360]
    for i, n in enumerate(order):
        dst.fill_(SENTINEL)
        _scan(v, dst, n, state, 1, False)
        assert torch.equal(dst[:n], ref[:n]), f"call {i}, n={n}"
        assert bool((dst[n:] == SENTINEL).all()), f"call {i}, n={n}: written past n"
