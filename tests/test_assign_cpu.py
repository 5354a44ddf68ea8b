"""The maximum-weight assignment's definition (dagr_amd/streaming.py: assign_max_weight_definition) without a GPU: against
brute force over every injection for every shape up to 5 x 6 in both orientations, against scipy on the larger matrices,
and the check that decides whether a pairing is right (check_assignment) against right and wrong pairings."""
import numpy as np
import pytest

from dagr_amd.streaming import DAGR_ASSIGN_MAX, assign_max_weight_definition, check_assignment
from tests import stream_identity_cases as ic


def test_the_definition_equals_brute_force_on_every_small_shape():
    """0 x 0 .. 5 x 6 and 6 x 5, weights 0..3 (many ties): the total is the largest over all injections, and the pairing is
    one-to-one, lists no pair of weight 0 and sums to it."""
    rng = np.random.Generator(np.random.PCG64(0))
    seen_transposed = seen_unpaired = 0
    for n in range(6):
        for m in range(7):
            for shape in {(n, m), (m, n)}:
                for _ in range(3):
                    w = rng.integers(0, 4, shape).astype(np.int32)
                    stats = {}
                    total, row_col = assign_max_weight_definition(w, stats)
                    assert total == ic.brute_force(w), (shape, w.tolist())
                    assert check_assignment(w, total, row_col) is None, (shape, w.tolist(), row_col)
                    assert row_col.dtype == np.int64 and stats["transposed"] == (shape[0] > shape[1])
                    seen_transposed += stats["transposed"]
                    seen_unpaired += int((row_col == -1).any())
    assert seen_transposed > 0 and seen_unpaired > 0


def test_the_definition_equals_scipy():
    optimize = pytest.importorskip("scipy.optimize")
    for name in ic.SCIPY_NAMES:
        w, total, row_col, stats = ic.solved(name)
        r, c = optimize.linear_sum_assignment(w, maximize=True)
        assert total == int(w[r, c].astype(np.int64).sum()), name
        assert check_assignment(w, total, row_col) is None, name
        print(name, "total", total, "path steps", stats["steps"])


def test_the_named_matrices_and_the_edges():
    for name in ("all-zero-10x12", "constant-9x6", "empty-0x0", "empty-0x3", "empty-4x0", "64x64"):
        w, total, row_col, stats = ic.solved(name)
        assert check_assignment(w, total, row_col) is None, name
    assert ic.solved("all-zero-10x12")[1] == 0 and (ic.solved("all-zero-10x12")[2] == -1).all()
    assert ic.solved("constant-9x6")[1] == 24 and (ic.solved("constant-9x6")[2] >= 0).sum() == 6
    assert ic.solved("empty-4x0")[2].tolist() == [-1] * 4 and ic.solved("empty-0x3")[2].shape == (0,)
    assert ic.solved("256x300-weights-0..2")[3]["steps"] > 256          # paths longer than one step
    for bad in (np.zeros((2, 2), np.float32), np.zeros(3, np.int32), np.zeros((1, DAGR_ASSIGN_MAX + 1), np.int32),
                np.array([[1, -1]], np.int32)):
        with pytest.raises(ValueError, match="assign_max_weight_definition"):
            assign_max_weight_definition(bad)


def test_the_pairing_check_itself():
    w = np.array([[4, 1, 0], [4, 3, 0]], np.int32)
    assert check_assignment(w, 7, [0, 1]) is None
    assert check_assignment(w, 5, [1, 0]) is None                       # (it checks a pairing against A total, not optimality)
    assert "sum" in check_assignment(w, 7, [1, 0])
    assert "twice" in check_assignment(w, 8, [0, 0])
    assert "weight 0" in check_assignment(w, 4, [0, 2])
    assert "range" in check_assignment(w, 4, [0, 3])
    assert "range" in check_assignment(w, 4, [0, -2])
    assert "shape" in check_assignment(w, 4, [0])
    assert check_assignment(w, 4, [0, -1]) is None and check_assignment(w, 0, [-1, -1]) is None
    assert check_assignment(np.zeros((0, 3), np.int32), 0, np.zeros(0, np.int64)) is None
