"""The maximum-weight assignment on the GPU: dagr_assign_max_weight through the binding against the numpy definition
(dagr_amd/streaming.py: assign_max_weight_definition) on the matrices of tests/stream_identity_cases.py -- the total is
compared, the pairing is checked for being right, never for being the definition's -- three lanes of different shapes in
one call; a leading dimension larger than the matrix; and the refusals, which launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import DAGR_ASSIGN_MAX, check_assignment
from tests import stream_identity_cases as ic
from tests.test_streaming_gpu import _dev

pytestmark = pytest.mark.gpu
SENTINEL = -7


class _Assign:
    """dagr_assign_max_weight on buffers of its own: lane b's matrix sits in the top-left corner of w[b] (the rest is a
    weight that would win everything: nothing may read it), the workspace starts out as garbage, the outputs as -7."""

    def __init__(self, mats, max_rows=None, max_cols=None, ld_rows=None, ld=None):
        self.L, self.dev, self.mats, self.B = _lib.lib(), torch.device("cuda:0"), mats, len(mats)
        self.max_rows = max_rows or max(1, max(m.shape[0] for m in mats))
        self.max_cols = max_cols or max(1, max(m.shape[1] for m in mats))
        self.ld_rows, self.ld = ld_rows or self.max_rows, ld or self.max_cols
        w = np.full((self.B, self.ld_rows, self.ld), 1 << 20, np.int32)
        for b, m in enumerate(mats):
            w[b, :m.shape[0], :m.shape[1]] = m
        self.w = _dev(w)
        self.n_rows = _dev(np.array([m.shape[0] for m in mats], np.int32))
        self.n_cols = _dev(np.array([m.shape[1] for m in mats], np.int32))
        self.nbytes = self.L.dagr_assign_workspace_bytes(self.B, self.max_rows, self.max_cols)
        assert self.nbytes >= 4 * self.B * self.max_rows * self.max_cols and self.nbytes % 16 == 0
        self.ws = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        self.row_col = torch.full((self.B, self.max_rows), SENTINEL, dtype=torch.int32, device=self.dev)
        self.total = torch.full((self.B,), SENTINEL, dtype=torch.int64, device=self.dev)

    def call(self, **over):
        P = _lib.ptr
        a = dict(w=P(self.w), B=self.B, ld_rows=self.ld_rows, ld=self.ld, n_rows=P(self.n_rows), n_cols=P(self.n_cols),
                 max_rows=self.max_rows, max_cols=self.max_cols, row_col=P(self.row_col), total=P(self.total), ws=P(self.ws),
                 bytes=self.nbytes)
        a.update(over)
        rc = self.L.dagr_assign_max_weight(a["w"], a["B"], a["ld_rows"], a["ld"], a["n_rows"], a["n_cols"], a["max_rows"],
                                           a["max_cols"], a["row_col"], a["total"], a["ws"], a["bytes"],
                                           _lib.cur_stream(self.dev))
        torch.cuda.synchronize()
        return rc

    def check(self, totals, where):
        total, row_col = self.total.cpu().numpy(), self.row_col.cpu().numpy()
        for b, m in enumerate(self.mats):
            assert int(total[b]) == totals[b], (where, b, m.shape, int(total[b]), totals[b])
            assert check_assignment(m, totals[b], row_col[b, :m.shape[0]]) is None, (where, b, m.shape)
            assert (row_col[b, m.shape[0]:] == -1).all(), (where, b, "rows behind n_rows")


@pytest.mark.parametrize("names", ic.BATCHES, ids=["+".join(n) for n in ic.BATCHES])
def test_the_total_equals_the_definitions_and_the_pairing_is_right(names):
    """Three lanes a call, one of them empty: 1 x 1; 5 x 7 and 7 x 5 (the transposition); 64 x 64, 65 x 130, 130 x 65 (the
    thread and register stripes); all-zero; constant; 256 x 300 with weights 0..2 (long paths); 1024 x 1024 dense and
    1000 x 1024 at 0.4 % (the cap)."""
    a = _Assign([ic.matrix(n) for n in names])
    _lib.check(a.call(), "dagr_assign_max_weight")
    a.check([ic.solved(n)[1] for n in names], names)


def test_leading_dimensions_larger_than_the_matrices():
    names = ("5x7", "130x65", "7x5")
    a = _Assign([ic.matrix(n) for n in names], max_rows=140, max_cols=70, ld_rows=150, ld=77)
    _lib.check(a.call(), "dagr_assign_max_weight")
    a.check([ic.solved(n)[1] for n in names], names)
    # counts outside their range are clamped: 7 x 5 asked for as 9 x -3 is 9 x 0, an empty matrix
    a.n_rows[2], a.n_cols[2] = 9, -3
    _lib.check(a.call(), "dagr_assign_max_weight")
    assert int(a.total[2]) == 0 and (a.row_col[2] == -1).all()


def test_argument_errors_launch_nothing():
    a = _Assign([ic.matrix("5x7"), ic.matrix("7x5")])
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)             # noqa: E731
    refusals = [(dict(w=None), b"NULL"), (dict(n_rows=None), b"NULL"), (dict(n_cols=None), b"NULL"), (dict(row_col=None), b"NULL"),
                (dict(total=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(B=0), b"out of range"), (dict(B=65536), b"out of range"),
                (dict(max_rows=0), b"out of range"), (dict(max_cols=DAGR_ASSIGN_MAX + 1, ld=2000), b"out of range"),
                (dict(ld_rows=6), b"ld_rows < max_rows"), (dict(ld=6), b"ld < max_cols"), (dict(bytes=a.nbytes - 1), b"smaller"),
                (dict(ws=odd(a.ws, 8)), b"aligned"), (dict(total=odd(a.total, 4)), b"aligned"), (dict(w=odd(a.w, 2)), b"aligned"),
                (dict(row_col=odd(a.row_col, 1)), b"aligned")]
    for over, text in refusals:
        assert a.call(**over) == bad, over
        said = a.L.dagr_last_error()
        assert text in said and said.startswith(b"dagr_assign_max_weight:"), (over, said)
    assert a.L.dagr_assign_workspace_bytes(0, 4, 4) == 0 and a.L.dagr_assign_workspace_bytes(1, 1025, 4) == 0
    assert a.L.dagr_assign_workspace_bytes(1, 4, 0) == 0
    assert (a.row_col == SENTINEL).all() and (a.total == SENTINEL).all() and (a.ws == 0x5a).all()
