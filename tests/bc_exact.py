"""An exact reference for the betweenness centrality of DESIGN 3.11: textbook Brandes, a label test per entry, sigma in Python
integers, delta and bc in fractions.Fraction, rounded to double ONCE at the end.  No parity arrays, no scipy: a mistake of
formulation that tests/bc_model.py and include/mgx/bc_fused.hpp could share (both sum over ALL entries of a row and rely on zeros
in the parity they read) does not reach this file.

The definition is the one of 3.11: a CSR entry (u, v) is an edge u -> v; every entry counts once, so duplicates are parallel edges
and distinct shortest paths; self-loops lie on no shortest path (a label test never lets one through); `symmetric` is the caller's
word that row v holds the in-entries of v too -- otherwise the in-rows are the transpose.
    label[v]  BFS depth over the out-entries, -1 unreached
    sigma[v]  = sum over the in-entries (u, v) with label[u] = label[v] - 1 of sigma[u],  sigma[s] = 1
    delta[v]  = sum over the out-entries (v, w) with label[w] = label[v] + 1 of sigma[v] / sigma[w] * (1 + delta[w])
    bc[v]     = sum over the sources s != v of delta_s[v]
delta[s] of the source itself is reported as 0, as every path of the library stores it (level 0 is never visited backward).

The comparison rule for ONE implementation against these values (close): zeros are exact; elsewhere
    |got - exact| <= (bc_model.rtol(L, R, S) / 2 + 2^-53) * exact
-- 3.11's derivation ((L * (R + 2) + S) roundings of non-negative terms) for one implementation, not two, plus the one rounding of
the exact value to double.  Derived, not tuned."""
from fractions import Fraction

import numpy as np

from tests import bc_model as model


def bound(levels, longest_row, sources):
    """the relative bound of one implementation against the exact values rounded once"""
    return model.rtol(levels, longest_row, sources) / 2.0 + 2.0 ** -53


def _rows(ro, ci):
    ro = [int(x) for x in ro]
    ci = [int(x) for x in ci]
    return [ci[ro[v]:ro[v + 1]] for v in range(len(ro) - 1)]


def _transpose(rows):
    inn = [[] for _ in rows]
    for u, row in enumerate(rows):
        for v in row:
            inn[v].append(u)
    return inn


def _to_double(x):
    """an integer or a Fraction, rounded to nearest even; +inf past the largest double"""
    try:
        return float(x)
    except OverflowError:
        return float("inf")


def one_source(out, inn, s):
    """(labels, sigma as integers, delta as Fractions, the vertices level by level) of source s"""
    n = len(out)
    label = [-1] * n
    label[s] = 0
    levels = [[s]]
    while True:
        d = len(levels)
        nxt = []
        for u in levels[-1]:
            for w in out[u]:
                if label[w] < 0:
                    label[w] = d
                    nxt.append(w)
        if not nxt:
            break
        levels.append(nxt)
    sigma = [0] * n
    sigma[s] = 1
    for d in range(1, len(levels)):
        for v in levels[d]:
            sigma[v] = sum(sigma[u] for u in inn[v] if label[u] == d - 1)
    delta = [Fraction(0)] * n
    carry = [None] * n                                  # (1 + delta[w]) / sigma[w], made once per w
    for d in range(len(levels) - 2, 0, -1):
        for v in levels[d]:
            t = Fraction(0)
            for w in out[v]:
                if label[w] == d + 1:
                    if carry[w] is None:
                        assert sigma[w] > 0, "a reached vertex without a shortest path: the in-rows are not the out-rows' transpose"
                        carry[w] = (1 + delta[w]) / sigma[w]
                    t += carry[w]
            delta[v] = sigma[v] * t
    return label, sigma, delta, levels


def run(ro, ci, sources=None, symmetric=False):
    """-> dict(labels int32, sigma (Python integers) and sigma_f (doubles) and delta (doubles) of the LAST source; bc (doubles);
    depth = the deepest traversal in levels; reached summed over the sources; longest_in, longest_out; stats in the order of
    bc_model.run: [sources, depth, reached, inexact, overflow] as 3.11 defines the two flags for doubles)"""
    n = len(ro) - 1
    out = _rows(ro, ci)
    inn = out if symmetric else _transpose(out)
    if sources is None:
        sources = range(n)
    sources = [int(s) for s in sources]
    bc = [Fraction(0)] * n
    label, sigma, delta = [-1] * n, [0] * n, [Fraction(0)] * n
    depth = reached = inexact = overflow = 0
    for s in sources:
        label, sigma, delta, levels = one_source(out, inn, s)
        for v in range(n):
            if delta[v]:
                bc[v] += delta[v]
        depth = max(depth, len(levels))
        reached += sum(len(lv) for lv in levels)
        big = max(sigma)
        inexact |= int(_to_double(big) >= model.TWO53)
        overflow |= int(_to_double(big) == float("inf"))
    return {"labels": np.array(label, dtype=np.int32), "sigma": sigma,
            "sigma_f": np.array([_to_double(x) for x in sigma], dtype=np.float64),
            "delta": np.array([_to_double(x) for x in delta], dtype=np.float64),
            "bc": np.array([_to_double(x) for x in bc], dtype=np.float64),
            "depth": depth, "reached": reached, "stats": [len(sources), depth, reached, inexact, overflow],
            "longest_in": max((len(r) for r in inn), default=0), "longest_out": max((len(r) for r in out), default=0)}


def close(tag, got, exact, rel):
    """one implementation against the truth: zeros exact, elsewhere within rel * exact; prints the worst ratio as _close does"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    assert got.shape == exact.shape, tag + ": shapes differ"
    assert np.isfinite(exact).all(), tag + ": the exact values are not finite"
    assert np.isfinite(got).all(), "%s: %d values are not finite" % (tag, int((~np.isfinite(got)).sum()))
    zero = (got == 0) | (exact == 0)
    assert np.array_equal(got[zero], exact[zero]), "%s: the exact zeros differ at %d vertices" % (tag, int((got[zero] != exact[zero]).sum()))
    err = np.abs(got - exact)
    worst = float((err[~zero] / exact[~zero]).max()) if (~zero).any() else 0.0
    print("%s: max rel %.3g (bound %.3g)" % (tag, worst, rel))
    assert (err <= rel * exact).all(), "%s: %d outside the bound %.3g (max %.3g)" % (tag, int((err > rel * exact).sum()), rel, worst)
