"""Inputs the backward aggregation's suites share (tests/test_aggbwd_cpu.py, tests/test_gpu_aggbwd.py, tests/test_gpu_agg_autograd.py):
graphs whose COLUMNS have given in-degrees, and the cases that tell a wrong order of L_c, a division on the wrong side of the weight,
a fused multiply-add and a wrong winner apart.  tests/test_aggbwd_cpu.py asserts, on the model, that each case does tell them apart."""
import numpy as np

from tests import agg_cases as fwd_cases
from tests.agg_cases import features, graph_rows, weights  # noqa: F401

# transposed row lengths at MGX_AGG_SEG=64: the cut, two segments, 5 segments and one entry
IN_DEGREES = [0, 1, 2, 7, 8, 9, 17, 63, 64, 65, 128, 129, 321]
FEATS = [1, 3, 4, 8, 60, 64, 256, 260, 516]
X_ROWS = [1, 3, 63, 64, 65, 257]


def graph_cols(in_degrees, seed=0, rows=None, long_rows=()):
    """a graph of n vertices in which column 3 k + 1 has in_degrees[k] entries, between a column without entries (3 k) and a column
    of one (3 k + 2); the entries are dealt to `rows` forward rows at random (duplicates and self-loops included) and stored in a
    random order.  long_rows: these forward rows get 70 .. 200 entries more to random columns of one entry or more, so that at seg
    64 the winners' items and fold run too -> (ro, ci), n = max(3 len(in_degrees), rows, 64)"""
    rng = np.random.default_rng(100 + seed)
    cols = []
    for k, d in enumerate(in_degrees):
        cols += [3 * k + 1] * int(d) + [3 * k + 2]
    n = max(3 * len(in_degrees), rows or 0, 64)
    rows = rows or n
    cols = np.array(cols, dtype=np.int64)
    src = rng.integers(0, rows, len(cols))
    for r in long_rows:
        more = rng.integers(70, 200)
        cols = np.concatenate([cols, 3 * rng.integers(0, len(in_degrees), more) + 2])
        src = np.concatenate([src, np.full(more, r)])
    order = rng.permutation(len(cols))
    cols, src = cols[order], src[order]
    order = np.argsort(src, kind="stable")
    ro = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    return ro.astype(np.int32), cols[order].astype(np.int32)


def star_in(entries=100000, n=1000, seed=3):
    """a star pointing inward: column 0 has `entries` in-entries, from rows of about entries / n entries each (row 1: 300 more, a long
    forward row at every seg up to 256); column 5 three"""
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, entries), np.full(300, 1), [7, 8, 9]])
    cols = np.concatenate([np.zeros(entries, dtype=np.int64), rng.integers(1, n, 300), [5, 5, 5]])
    order = rng.permutation(len(cols))
    cols, src = cols[order], src[order]
    order = np.argsort(src, kind="stable")
    ro = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    return ro.astype(np.int32), cols[order].astype(np.int32)


def stability_case(feats=4):
    """(a) column 0 gets one entry from each of 48 rows whose gradients span 2^-20 .. 2^20 with mixed signs: the sum in ascending e
    and the sum in descending e differ in their bits -> (ro, ci, gy)"""
    ro, ci = graph_cols([48, 5, 0, 2], seed=7, rows=48)
    return ro, ci, features(len(ro) - 1, feats, seed=77)


def mean_case(feats=8):
    """(b) rows of d = 3 and d = 7 entries, weighted: w * (gy / d) and (w * gy) / d differ in some element for each d
    -> (ro, ci, w, gy)"""
    ro = np.array([0, 3, 10, 10], dtype=np.int32)
    ci = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 2], dtype=np.int32)
    return ro, ci, weights(10, seed=8), features(3, feats, seed=88)


def fma_case(feats):
    """(c) the forward's fused-multiply-add case, transposed: column 0 gets 1 * -(1 + 2^-11) from row 0 and (1 + 2^-12) * (1 + 2^-12)
    from row 1, 0.0 with a separate multiply and add and 2^-24 fused -> (ro, ci, w, gy)"""
    _, _, w, x = fwd_cases.fma_case(feats)
    return np.array([0, 1, 2], dtype=np.int32), np.array([0, 0], dtype=np.int32), w, x


def tie_case(feats=4, op="max"):
    """(d) at seg 64: row 0 has 130 entries to the columns 0 .. 129 in order; the extreme value stands at the entries 10 and 20 (a tie
    inside segment 0), 70 (across the boundary) and 129: the winner is entry 10.  Row 1 ties +0.0 against -0.0 (entry 130 wins),
    row 2 starts with a NaN (which keeps the win), row 3 has a NaN later (which never wins), row 4 names column 5 three times and
    itself -> (ro, ci, x)"""
    sign = np.float32(1.0 if op == "max" else -1.0)
    x = -np.abs(features(140, feats, seed=9)) * sign
    x[[10, 20, 70, 129]] = np.float32(5.0) * sign
    x[130], x[131] = 0.0, -0.0
    x[132] = np.nan
    ro = np.array([0, 130, 132, 135, 138, 142], dtype=np.int32)
    ci = np.concatenate([np.arange(130), [130, 131], [132, 1, 2], [3, 132, 133], [5, 5, 4, 5]]).astype(np.int32)
    ro = np.concatenate([ro, np.full(140 - 5, 142)]).astype(np.int32)
    return ro, ci, x.astype(np.float32)
