"""Inputs the neighbour feature aggregation's suites share (tests/test_agg_cpu.py, tests/test_gpu_agg.py): graphs whose rows have
given lengths, features and weights with mixed signs and magnitudes (so that the order of the additions shows in the bits), and the
rows that tell a fused multiply-add, a missing segment tree and the order of +-0 apart."""
import numpy as np

from tests.lpa_cases import directed, empty, random_digraph, random_symmetric  # noqa: F401

# feature widths: the vector path's team widths G = 1, 2, 4, .., 64 and column tiles 1 -> 2 -> 3; the scalar path's
VECTOR_FEATS = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516]
SCALAR_FEATS = [1, 2, 3, 5, 7, 9, 17, 33, 63, 65, 127, 129]
TEAM_ROWS = [0, 1, 2, 7, 70]
SEG_EDGE_ROWS = [63, 64, 65, 127, 128, 129, 64 * 5 + 1]          # at MGX_AGG_SEG=64


def graph_rows(lengths, seed=0, n=None):
    """a graph of n >= len(lengths) vertices whose row i has lengths[i] entries (the rows behind them none) to random vertices,
    duplicates and self-loops included, in a random stored order -> (ro, ci)"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = max(len(lengths), n or 0, 1)
    d = np.concatenate([lengths, np.zeros(n - len(lengths), dtype=np.int64)])
    ro = np.concatenate([[0], np.cumsum(d)])
    return ro.astype(np.int32), rng.integers(0, n, int(ro[-1])).astype(np.int32)


def features(rows, feats, seed=0):
    """float32[rows, feats]: mixed signs, magnitudes 2^-20 .. 2^20, full mantissas"""
    rng = np.random.default_rng(1000 + seed)
    mag = np.exp2(rng.uniform(-20.0, 20.0, (rows, feats)))
    return (np.where(rng.random((rows, feats)) < 0.5, -1.0, 1.0) * mag).astype(np.float32)


def weights(m, seed=0):
    """float32[m]: mixed signs, magnitudes 2^-4 .. 2^4"""
    rng = np.random.default_rng(2000 + seed)
    return (np.where(rng.random(m) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(-4.0, 4.0, m))).astype(np.float32)


def interleaved(lengths, seed=0):
    """every length between a row without entries and a row of one: neighbouring lanes (teams) get rows of all three kinds"""
    out = []
    for d in lengths:
        out += [0, d, 1]
    return graph_rows(out, seed, n=max(64, len(out)))


def zeros_case(feats):
    """rows over x[0] = +0.0 and x[1] = -0.0: row 0 reads (+0, -0), row 1 (-0, +0), row 2 (-0, -0, +0) -> (ro, ci, x).  max and
    min keep the FIRST of equal values (t > acc and t < acc are both false), the sum of -0 and -0 is -0"""
    ro = np.array([0, 2, 4, 7, 7], dtype=np.int32)
    ci = np.array([0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    x = np.zeros((4, feats), dtype=np.float32)
    x[1] = -0.0
    x[2:] = features(2, feats, 5)
    return ro, ci, x


def fma_case(feats):
    """one row of two entries whose weighted sum is 0.0 with a separate multiply and add and 2^-24 when they are fused:
    t_0 = 1 * -(1 + 2^-11), t_1 = (1 + 2^-12) * (1 + 2^-12) = 1 + 2^-11 + 2^-24 exactly, which rounds (a tie, to even) to
    1 + 2^-11 -> (ro, ci, w, x)"""
    a = np.float32(1.0 + 2.0 ** -12)
    acc = np.float32(-(1.0 + 2.0 ** -11))
    exact = float(a) * float(a)                                               # (48 bits: exact in float64)
    assert exact == 1.0 + 2.0 ** -11 + 2.0 ** -24
    separate = np.float32(np.float32(a * a) + acc)
    fused = np.float32(exact + float(acc))                                    # (the sum is exact in float64 too)
    assert separate == np.float32(0.0) and fused == np.float32(2.0 ** -24) and separate != fused
    ro = np.array([0, 2, 2], dtype=np.int32)
    ci = np.array([0, 1], dtype=np.int32)
    x = np.empty((2, feats), dtype=np.float32)
    x[0], x[1] = acc, a
    return ro, ci, np.array([1.0, a], dtype=np.float32), x


def huge_row(entries=100000, n=1000, seed=3):
    """row 0 has `entries` entries, row 1 three, the others none"""
    return graph_rows([entries, 3], seed, n=n)
