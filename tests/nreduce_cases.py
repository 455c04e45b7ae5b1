"""Inputs and the reference of the neighbour-reduce's path tests, shared by the CPU suite (tests/test_nreduce_cases_cpu.py: the
builder yields what it promises, the reference agrees with the oracle) and the GPU suite (tests/test_gpu_nreduce_paths.py,
tests/nreduce_child.py).  numpy only; everything is generated.

The operator (include/gunrock/neighborhood.hxx): reduced[i] = op over the neighbours u of frontier[i] of value(u); a row without
entries receives the caller's identity; the identity is never folded into a row that has entries.

Values are per VERTEX, so "the entry at position p of row r" means the vertex ci[ro[r] + p]: what planted() hands an extreme to."""
import numpy as np

N = 1 << 17                        # four slices of 40 000 ids: MGX_NR_SLICES=1 leaves a tail; ids stay below 2^23 (24-bit unit blocks)
UNIT = 64                          # entries of a unit block
WHERE = ("first", "last", "unit_end", "tail_first")
OPS = ("f32_plus", "i32_min", "i32_max")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def edge_degrees(long_min=64):
    """row lengths at every class edge of include/mgx/nreduce.hpp: the short rows' classes (1 .. 4 / 5 .. 16 / 17 .. long_min - 1
    entries), the long-row threshold, whole and partial 64-entry units, 64 / 65 units (NR_BIG_UNITS: a workgroup per row in
    k_nr_fold, 65 units with and without an entry left over) and the tiers of k_nrs_fold (256 / 4096 / 65536 entries)"""
    degs = [0, 1, 4, 5, 16, 17, long_min - 1, long_min, long_min + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097,
            4160, 4161, 65535, 65536, 65537]
    return tuple(sorted(set(degs)))


def edge_graph(long_min=64, seed=0, n=N):
    """(ro, ci, special): a directed CSR over n vertices, rows sorted by neighbour.  special: {degree: vertex} -- one vertex per
    degree of edge_degrees(long_min), its neighbours distinct and drawn over the whole id range; every other vertex has 0 .. 8
    random entries (parallel entries and self loops included)."""
    rng = np.random.default_rng(seed)
    degs = edge_degrees(long_min)
    ids = rng.choice(n, len(degs), replace=False)
    deg = rng.integers(0, 9, n).astype(np.int64)
    deg[ids] = degs
    ro = np.concatenate([[0], np.cumsum(deg)])
    assert ro[-1] < 2 ** 31
    ci = rng.integers(0, n, int(ro[-1])).astype(np.int32)
    for v, d in zip(ids, degs):
        if d:
            ci[ro[v]:ro[v + 1]] = rng.choice(n, d, replace=False)
    # rows sorted by neighbour: one sort of (row, neighbour) keys
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    ci = ci[np.lexsort((ci, row))]
    return ro.astype(np.int32), ci, {int(d): int(v) for v, d in zip(ids, degs)}


def transpose(ro, ci):
    """(co, ri): the CSC of (ro, ci) -- sources of every vertex's in-edges, ascending, parallel entries kept"""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    order = np.lexsort((rows, ci))
    co = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return co, rows[order].astype(np.int32)


# ---- values ------------------------------------------------------------------------------------------------------------------------
def small_int_values(n, rng):
    """float32 1 .. 8: sums of up to 2^21 of them are exact in float32 whatever the order, and without zeros a dropped or doubled
    entry always changes its row's sum"""
    return rng.integers(1, 9, n).astype(np.float32)


def real_values(n, rng):
    """signed float32 in [-3, 3)"""
    return (rng.random(n) * 6.0 - 3.0).astype(np.float32)


def int_values(n, rng, sign=0):
    """int32; sign > 0: all in [1000, 2000), sign < 0: all in (-2000, -1000], 0: in [-1000, 1000)"""
    if sign > 0:
        return rng.integers(1000, 2000, n).astype(np.int32)
    if sign < 0:
        return (-rng.integers(1000, 2000, n)).astype(np.int32)
    return rng.integers(-1000, 1000, n).astype(np.int32)


def position(d, where):
    """the position `where` names in a row of d entries (None: the row has no such position)"""
    if d <= 0:
        return None
    if where == "first":
        return 0
    if where == "last":
        return d - 1
    if where == "unit_end":                      # the last entry of the row's last FULL unit
        return (d // UNIT) * UNIT - 1 if d >= UNIT else None
    if where == "tail_first":                    # the first entry of the last, partial unit of a row of more than one unit
        return (d // UNIT) * UNIT if d > UNIT and d % UNIT else None
    raise KeyError(where)


def planted(ro, ci, rows, where, is_max=False, seed=0):
    """int32 values (all positive for a minimum, all negative for a maximum: 0 is a non-neutral identity for both) so that the UNIQUE
    minimum / maximum of a checked row sits at position `where` of it (position()).  Returns batches [(values, {row: extreme})]: every
    row of `rows` that has the position is in exactly one batch.

    Values belong to vertices: the holder of row r's extreme is h_r = ci[ro[r] + p].  Within a batch row k (in descending degree)
    gets the k-th most extreme value, every other vertex a value beyond all of them; h_j inside row r masks r's extreme iff j is
    more extreme than r -- so a row joins the first batch in which no holder of an earlier row lies in it (rows must have distinct
    neighbours: the holder then appears once in its own row)."""
    rng = np.random.default_rng(seed)
    n = len(ro) - 1
    deg = np.diff(ro).astype(np.int64)
    todo = [int(r) for r in sorted(rows, key=lambda r: -deg[r]) if position(int(deg[r]), where) is not None]
    batches = []
    while todo:
        holders, members, rest = [], [], []
        for r in todo:
            row = ci[ro[r]:ro[r + 1]]
            h = int(row[position(int(deg[r]), where)])
            if any(np.any(row == x) for x in holders):
                rest.append(r)
                continue
            holders.append(h); members.append(r)
        vals = int_values(n, rng, -1 if is_max else 1)
        want = {}
        for k, (r, h) in enumerate(zip(members, holders)):
            vals[h] = -(k + 1) if is_max else k + 1
            want[r] = int(vals[h])
        batches.append((vals, want))
        todo = rest
    return batches


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def reduce_f64(ro, ci, ids, vals, identity, op):
    """(reduced, edges) by frontier position.  f32_plus: float64 sums of the float32 values (np.add.reduceat over each row's gathered
    entries); i32_min / i32_max: int64 np.minimum / np.maximum.reduceat.  Empty rows give the identity; the identity is never folded in."""
    ro = np.asarray(ro).astype(np.int64)
    ids = np.asarray(ids).astype(np.int64)
    lo, cnt = ro[ids], ro[ids + 1] - ro[ids]
    total = int(cnt.sum())
    start = np.cumsum(cnt) - cnt
    plus = op == "f32_plus"
    out = np.full(len(ids), np.float64(np.float32(identity)) if plus else int(identity), dtype=np.float64 if plus else np.int64)
    if total == 0:
        return out, 0
    idx = np.repeat(lo - start, cnt) + np.arange(total, dtype=np.int64)
    x = np.asarray(vals)[np.asarray(ci)[idx]].astype(np.float64 if plus else np.int64)
    some = cnt > 0
    fn = {"f32_plus": np.add, "i32_min": np.minimum, "i32_max": np.maximum}[op]
    out[some] = fn.reduceat(x, start[some])
    return out, total


def sum_bound(ro, ci, ids, vals):
    """float32 sums of d entries in ANY order, per row: |got - want| <= gamma(d - 1) sum |x_e| with gamma(k) = k u / (1 - k u), u = 2^-24
    (every one of the d - 1 additions rounds once, an entry passes through at most d - 1 of them); k u <= 2^-8 for d <= 65537, so
    gamma(k) <= 1.004 k u: the bound is 1.01 (d - 1) 2^-24 sum |x_e|, atol 0 -- and 0 for d <= 1.  Derived, not measured."""
    mag, _ = reduce_f64(ro, ci, ids, np.abs(np.asarray(vals, dtype=np.float64)).astype(np.float32), 0.0, "f32_plus")
    ids = np.asarray(ids).astype(np.int64)
    d = (np.asarray(ro).astype(np.int64)[ids + 1] - np.asarray(ro).astype(np.int64)[ids]).astype(np.float64)
    return 1.01 * np.maximum(d - 1.0, 0.0) * 2.0 ** -24 * mag


# ---- frontiers ---------------------------------------------------------------------------------------------------------------------
def subset_frontiers(n, special, seed=0):
    """ascending subsets of 0 .. n - 1 by name: every special row inside (n / 2 ids), every special row outside (n / 2 ids), exactly
    ceil(n / 8) ids (the smallest subset the layout's kernels take) and one fewer (the general kernel), both with the special rows"""
    rng = np.random.default_rng(1000 + seed)
    sp = np.array(sorted(special.values()), dtype=np.int64)
    others = np.setdiff1d(np.arange(n), sp)
    eighth = -(-n // 8)

    def with_special(k):
        return np.sort(np.concatenate([sp, rng.choice(others, k - len(sp), replace=False)])).astype(np.int32)
    return {
        "inside": with_special(n // 2),
        "outside": np.sort(rng.choice(others, n // 2, replace=False)).astype(np.int32),
        "eighth": with_special(eighth),
        "below_eighth": with_special(eighth - 1),
    }
