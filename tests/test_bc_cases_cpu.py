"""CPU suite: every case of tests/bc_cases.py holds what it claims -- row lengths and classes, level widths, the depth the traversal
reports, the sigma table, the launch plan -- and tests/bc_model.py keeps the one-implementation bound against tests/bc_exact.py on
every case small enough for both.  No GPU, no library."""
import numpy as np
import pytest

from tests import bc_cases as cases
from tests import bc_exact as exact
from tests import bc_model as model

# the exact reference and the model can afford these; past 2^1024 there is no finite truth (test_sigma_table pins those two)
SMALL = [k for k in cases.NAMES if not k.startswith("bounds_growth") and k not in ("sigma_limits-1025", "sigma_limits-1026")]


def _labels(c):
    out, _ = model.matrices(c["ro"], c["ci"], c["symmetric"])
    return model.bfs(out, int(c["sources"][0]))


def test_names_and_groups():
    assert len(set(cases.NAMES)) == len(cases.NAMES)
    assert {cases.get(k)["group"] for k in cases.NAMES} =={"key_bits", "bounds_growth", "sigma_limits", "class_edges", "plan", "behind_the_trace", "parity_back_edges"}
    assert len(cases.names("key_bits")) == 2 * 14 + 2 and len(cases.names("plan")) == 6 and len(cases.names("sigma_limits")) == 5


# ---- key_bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.names("key_bits"))
def test_key_bits_depth_and_largest_key(name):
    c = cases.get(name)
    o = cases.opts(c["env"])
    labels = _labels(c)
    assert cases.traversal_levels(c["ro"], labels) == c["levels"]
    depth = int(labels.max()) + 1
    assert c["levels"] == depth - (0 if c["symmetric"] else 1)              # both meanings of `levels`
    # the largest key of the forward sort fits the width, and fits no width one bit smaller where the case says so
    cls = np.array([cases.row_class(x, o) for x in np.diff(cases.in_offsets(c["ro"], c["ci"]) if not c["symmetric"] else c["ro"]).tolist()])
    keys = (labels.astype(np.int64) + 1) * cases.KEY_STRIDE + cls
    K, bits = cases.key_count(c["levels"]), cases.end_bit(c["levels"])
    assert keys.max() < K <= (1 << bits) and (bits == 1 or (1 << (bits - 1)) < K)
    if "leaves" in c:
        p = c["path_n"]
        assert np.diff(c["ro"])[p - 1] == 71 and cls[p - 1] == cases.HUGE and labels[p - 1] == depth - 2
        assert (labels[p:] == depth - 1).all() and (cls[p:] == cases.LANE).all() and len(labels) - p == 70
        assert keys[p:].min() == 1 << (bits - 1)                            # the leaves' key is the first that needs the top bit
        assert cases.class_counts(c["ro"], o) == (p - 1 + 70, 0, 1, 2)


def test_key_bits_stand_on_256_and_4096():
    """K just below, on and just above both powers of two, for both meanings of `levels`; the directed path at K = 260 and 4100
    holds a key that needs the top bit (its sink's: 4 n)"""
    for sym, shift in ((True, 2), (False, 1)):
        ks = [cases.key_count(cases.get("key_bits-%s-%d" % ("sym" if sym else "dir", n))["levels"]) for n in cases.KEY_BITS_N]
        assert ks == [(n + shift) * 4 for n in cases.KEY_BITS_N]
        for power in (256, 4096):
            assert power - 4 in ks and power in ks and power + 4 in ks
    for n, bits in ((63, 8), (64, 9), (1023, 12), (1024, 13)):
        c = cases.get("key_bits-dir-%d" % n)
        assert cases.end_bit(c["levels"]) == bits
    assert 4 * 64 == 1 << 8 and 4 * 1024 == 1 << 12                          # the sinks' keys at n = 64 and 1024: lost with one bit less
    for n, bits in ((62, 8), (63, 9), (64, 9), (1022, 12), (1023, 13), (1024, 13)):
        assert cases.end_bit(cases.get("key_bits-sym-%d" % n)["levels"]) == bits
    # symmetric n = 64 and 1024: the last vertex's key 4 n = 256 and 4096 needs the top bit too
    assert cases.key_count(64) == 264 and cases.key_count(1024) == 4104


# ---- bounds_growth --------------------------------------------------------------------------------------------------------------------
def test_bounds_growth_stands_on_the_formula():
    small, big = (cases.get(k) for k in cases.names("bounds_growth"))
    assert (small["path_n"], big["path_n"]) == (65537, 65538)
    for c in (small, big):
        n = c["path_n"]
        assert len(c["ro"]) - 1 == n and c["levels"] == n                   # the symmetric path: the last vertex expands its back entry
        assert cases.grows(c["levels"], cases.bound_cap(n)) == c["grows"]
    assert not small["grows"] and big["grows"]
    assert cases.bound_cap(65537) == cases.bound_cap(1 << 20) == 65540 * 4 + 1
    # the largest that does not grow, the smallest that does -- and the same n on a handle that has grown does not grow again
    assert not cases.grows(65537, cases.bound_cap(65537)) and cases.grows(65538, cases.bound_cap(65538))
    grown = (65538 + 1 + 2) * cases.KEY_STRIDE + 1
    assert not cases.grows(65538, grown)
    # a short graph's handle: min(n, 65536) = n, a traversal has at most n levels, D' <= n + 1 < n + 3
    assert not cases.grows(300, cases.bound_cap(300))
    w = cases.expected(small["name"])
    assert w["stats"] == [1, 65537, 65537, 0, 0] and w["delta"][1] == 65535 and w["delta"][0] == 0 and w["delta"][-1] == 0


# ---- sigma_limits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SIGMA_N)
def test_sigma_table(n):
    c = cases.get("sigma_limits-%d" % n)
    m = model.run(c["ro"], c["ci"], c["sources"], True)
    e = exact.run(c["ro"], c["ci"], c["sources"], True)
    assert e["sigma"] == [2 ** v for v in range(n)]                         # exactly, as integers
    assert m["stats"] == [1, n, n] + list(c["flags"]) == e["stats"]
    v = np.arange(n)
    line = (n - 1.0 - v) * (v > 0)
    if n <= 1024:
        w = cases.expected(c["name"])
        for k in ("labels", "sigma", "delta", "bc"):
            assert np.array_equal(m[k], w[k]), k                            # the model computes the closed form bit for bit
        assert np.array_equal(w["delta"], line) and np.array_equal(e["delta"], line) and np.array_equal(e["sigma_f"], w["sigma"])
        if n == 1024:
            q = 1.0 / w["sigma"][1023]
            assert q == 2.0 ** -1023 and 0.0 < q < np.finfo(np.float64).tiny     # a subnormal; flushed, delta[1022] is 0 in place of 1
            assert w["sigma"][1022] * (2.0 * q) == 1.0 == w["delta"][1022]
    elif n == 1025:
        assert np.isinf(m["sigma"][1024]) and np.isfinite(m["sigma"][:1024]).all()
        assert not np.isnan(m["delta"]).any() and m["delta"][1023] == 0 and m["delta"][1024] == 0
        assert np.array_equal(m["delta"][:1023], (1023.0 - v[:1023]) * (v[:1023] > 0))
    else:
        assert np.isinf(m["sigma"][1024:]).all()
        assert np.isnan(m["delta"][1:1025]).all() and m["delta"][0] == 0 and m["delta"][1025] == 0


# ---- class_edges ----------------------------------------------------------------------------------------------------------------------
def test_class_edges_rows():
    o = cases.opts({})
    c = cases.get("class_edges-sym")
    d = np.diff(c["ro"])
    assert tuple(d[1:8]) == cases.HUB_ROWS and d[0] == 7 and d[8:].max() == 7 and d[8:].min() == 1 and len(c["ci"]) == c["entries"] == 114756
    assert d.max() == c["longest_in"] == 16385
    huge = [r for r in cases.HUB_ROWS if r >= 8192]
    segs = [(r + 8191) // 8192 for r in huge]
    assert segs == [1, 2, 2, 3] and [r % 8192 for r in huge] == [0, 1, 0, 1]    # exact multiples and a last segment of one entry
    assert cases.class_counts(c["ro"], o) == (len(d) - 6, 2, 4, sum(segs))      # lane: all but 17, 8191 (wave) and the four huge
    assert [cases.row_class(r, o) for r in cases.HUB_ROWS] == [0, 1, 1, 2, 2, 2, 2]
    first = 8
    assert [int(x) for x in c["sources"]] == [0, first, first + 8190, 3] and d[3] == 8191
    # the pool's sigma from the root run from 1 to 7: hub k reaches the first HUB_ROWS[k] - 1 pool vertices
    e = exact.run(c["ro"], c["ci"], [0], True)
    assert sorted(set(e["sigma"][8:])) == [1, 2, 3, 4, 5, 6, 7] and e["depth"] == 3
    # directed: the downward entries only; the in-rows and the out-rows have classes of their own
    c = cases.get("class_edges-dir")
    out, inn = np.diff(c["ro"]), np.diff(cases.in_offsets(c["ro"], c["ci"]))
    assert tuple(out[1:8]) == tuple(r - 1 for r in cases.HUB_ROWS) and out[0] == 7 and not out[8:].any() and len(c["ci"]) == c["entries"]
    assert inn.max() == 7 and inn[0] == 0 and (inn[1:8] == 1).all()
    assert cases.class_counts(cases.in_offsets(c["ro"], c["ci"]), o) == (len(out), 0, 0, 0)
    assert cases.class_counts(c["ro"], o) == (len(out) - 5, 2, 3, 1 + 2 + 2)    # 15, 16 lane; 8190, 8191 wave; 8192, 16383, 16384 huge


# ---- plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.names("plan") + ["behind_the_trace"])
def test_level_widths(name):
    c = cases.get(name)
    labels = _labels(c)
    assert np.bincount(labels).tolist() == c["widths"] and (labels >= 0).all()
    assert cases.traversal_levels(c["ro"], labels) == c["levels"] == len(c["widths"])
    o = cases.opts(c["env"])
    lane, wave, huge, segs = cases.class_counts(c["ro"], o)
    assert huge == 0                                                        # a grid level is one launch in both directions
    if name == "behind_the_trace":
        d = np.diff(c["ro"])
        assert c["levels"] > cases.TRACE and c["widths"][4100] == 3000 > o["chain"]
        assert (d[labels == 4100] == 21).all() and (d[labels == 4101] == 1000).all() and d[4099] == 3001
        assert cases.row_class(21, o) == cases.WAVE and wave == 3000 + 60 + 1
        # the big level and the one behind it are behind the trace: small, in one chain with the path's tail, forward and backward
        fwd, bwd, launches = cases.predicted(c["widths"], o["chain"], c["levels"])
        assert (fwd, bwd) == (1, 1) and launches == 5 + 3 + 3 + 1 + 2
    else:
        assert c["levels"] < cases.TRACE and max(c["widths"]) == o["chain"] + 1 and o["chain"] in c["widths"]


def test_predicted_against_hand_counts():
    """widths a, levels 9, D' = 10.  small: 1, 3, 6, 7, 8 and 9 (behind the deepest: an empty list, not traced).
         forward 1 .. 9:   1 grid, 2 grid, 3 grid (a run of one stays on the grid), 4 grid, 5 grid, [6 7 8 9] one chain       -> 5 + 1
         backward 8 .. 1:  [8 7 6] one chain, 5 grid, 4 grid, 3 grid, 2 grid, 1 grid (the walk stops at 1: a run of one)      -> 1 + 5
       widths c, levels 4, D' = 5.  small: 2, 3, 4.
         forward 1 .. 4:   1 grid, [2 3 4] one chain;   backward 3 .. 1:  [3 2] one chain, 1 grid                             -> 2 + 2
       fixed: 5 (begin_run) + 3 (clear, seed, keys) + 3 (one sort) + 1 (finish) = 12"""
    for chain in (1024, 4):
        a, b, c = (cases.get("plan-%s-chain%d" % (w, chain))["widths"] for w in "abc")
        assert cases.predicted(a, chain, 9) == (1, 1, 12 + 6 + 6)
        assert cases.predicted(c, chain, 4) == (1, 1, 12 + 2 + 2)
        assert cases.predicted(b, chain, 9) == (2, 2, 12 + 6 + 6)             # [1 2] 3 4 5 6 [7 8 9];  [8 7] 6 5 4 3 [2 1]
        # were the deepest level a sink level (levels = 3): forward [2 3], backward starts at 2 -- a run of one, no chain
        assert cases.predicted(c, chain, 3) == (1, 0, 12 + 2 + 2)
        # chain off: every level on the grid, 2 D' - 3 launches
        assert cases.predicted(a, 0, 9) == (0, 0, 12 + 9 + 8)
    # a level of exactly `chain` vertices is small, one of chain + 1 is not
    assert cases.predicted([1, 1024, 1024, 1], 1024, 4)[0] == 1 and cases.predicted([1, 1025, 1025, 1], 1024, 4)[:2] == (1, 0)
    # huge rows cost a grid level two launches more; a directed graph sorts twice
    assert cases.predicted(cases.WIDTHS["c"], 1024, 4, huge_in=True, huge_out=True, two_sorts=True)[2] == 12 + 3 + (3 + 1) + (1 + 3)


# ---- parity_back_edges ----------------------------------------------------------------------------------------------------------------
def test_back_edges_land_on_the_read_parity():
    c = cases.get("parity_back_edges")
    ro, ci = c["ro"].astype(np.int64), c["ci"].astype(np.int64)
    labels = _labels(c)
    assert np.array_equal(labels, np.arange(41))
    rows = np.repeat(np.arange(41), np.diff(ro))
    back = ci < rows
    assert back.sum() == 40 + 38 + 36 and ((labels[rows[back]] - labels[ci[back]]) % 2 == 1).all()      # the parity of level d + 1
    assert set((rows[back] - ci[back]).tolist()) == {1, 3, 5} and (ci[~back] == rows[~back] + 1).all()
    w = cases.expected(c["name"])
    assert np.array_equal(w["delta"], (40.0 - np.arange(41)) * (np.arange(41) > 0)) and (w["sigma"] == 1).all()


# ---- the model keeps the bound it is given ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_model_within_the_one_implementation_bound(name):
    c = cases.get(name)
    e = exact.run(c["ro"], c["ci"], c["sources"], c["symmetric"]) if c["want"] != "exact" else None
    if e is None:
        w = cases.expected(name)
        e = {"labels": w["labels"], "sigma_f": w["sigma"], "delta": w["delta"], "bc": w["bc"], "stats": w["stats"],
             "longest_in": w["longest_in"], "longest_out": w["longest_out"]}
    m = model.run(c["ro"], c["ci"], c["sources"], c["symmetric"])
    assert np.array_equal(m["labels"], e["labels"]) and m["stats"] == e["stats"]
    assert (m["longest_in"], m["longest_out"]) == (e["longest_in"], e["longest_out"])
    if m["max_sigma"] < model.TWO53:
        assert np.array_equal(m["sigma"], e["sigma_f"])
    rel = exact.bound(m["stats"][1], max(m["longest_in"], m["longest_out"]), len(c["sources"]))
    exact.close(name + ": model delta", m["delta"], e["delta"], rel)
    exact.close(name + ": model bc", m["bc"], e["bc"], rel)
    w = cases.expected(name)
    assert w["stats"] == e["stats"] and (w["longest_in"], w["longest_out"]) == (e["longest_in"], e["longest_out"])
