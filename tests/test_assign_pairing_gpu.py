"""WHICH optimal pairing dagr_assign_max_weight returns: row_col equals assign_max_weight_definition's entry for entry
(dagr_amd/streaming.py), on matrices on which almost every optimal pairing is one of many -- weights 0..2, identical rows,
identical columns -- at 5 x 7, 7 x 5 (transposed), 64 x 65 and 130 x 70.  tests/test_assign_gpu.py compares the total and
checks that the pairing is right; the stream tracker's optimal assignment (dagr_stream_track_optimal) needs more: its track
ids hang on the pairing being the definition's, the same walk comparison for comparison."""
import functools

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd.streaming import assign_max_weight_definition
from tests.test_assign_gpu import _Assign

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (7, 5), (64, 65), (130, 70)]
KINDS = ("weights-0-to-2", "identical-rows", "identical-columns", "constant")


@functools.lru_cache(maxsize=None)
def _matrix(kind, shape):
    """Seeded; the same for everyone (nobody changes what comes back)."""
    n, m = shape
    rng = np.random.Generator(np.random.PCG64(100 * n + m))
    if kind == "weights-0-to-2":
        return rng.integers(0, 3, (n, m)).astype(np.int32)
    if kind == "identical-rows":                    # three kinds of row, each many times
        return rng.integers(0, 3, (3, m)).astype(np.int32)[rng.integers(0, 3, n)]
    if kind == "identical-columns":
        return np.ascontiguousarray(rng.integers(0, 3, (n, 3)).astype(np.int32)[:, rng.integers(0, 3, m)])
    return np.full((n, m), 2, np.int32)


@functools.lru_cache(maxsize=None)
def _defined(kind, shape):
    return assign_max_weight_definition(_matrix(kind, shape))


@pytest.mark.parametrize("kind", KINDS)
def test_the_pairing_is_the_definitions_entry_for_entry(kind):
    """The four shapes as four lanes of one call: total and every entry of row_col."""
    mats = [_matrix(kind, shape) for shape in SHAPES]
    a = _Assign(mats)
    _lib.check(a.call(), "dagr_assign_max_weight")
    total, row_col = a.total.cpu().numpy(), a.row_col.cpu().numpy()
    for b, shape in enumerate(SHAPES):
        want_total, want = _defined(kind, shape)
        got = row_col[b, :shape[0]]
        print(kind, shape, "total", int(total[b]), "pairs", int((got >= 0).sum()), "entries that differ", int((got != want).sum()))
        assert int(total[b]) == want_total, (kind, shape)
        assert np.array_equal(got, want), (kind, shape, got.tolist(), want.tolist())
