"""CPU suite for the betweenness centrality (mgx_bc_*, include/mgx/bc_fused.hpp, include/gunrock/bc/): the library exports it, refuses
bad arguments, its kernels keep their registers, and the model the GPU tests compare against (tests/bc_model.py: the parity
formulation, no label test per entry) agrees with networkx, with a textbook Brandes that tests labels, with a brute-force
enumeration of entry-paths and with closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bc_model as model
from tests import coloring_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
NAMES = ["mgx_bc_create", "mgx_bc_free", "mgx_bc_run", "mgx_bc_enact", "mgx_bc_centrality", "mgx_bc_centrality_device", "mgx_bc_sigma",
         "mgx_bc_delta", "mgx_bc_labels", "mgx_bc_info"]
KERNELS = ["k_bc_keys", "k_bc_bounds", "k_bc_seed", "k_bc_finish", "k_bc_level", "k_bc_huge_seg", "k_bc_huge_fold", "k_bc_chain"]


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_library_exports_bc(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "BcProblem")
    for member in ("run", "enact", "centrality", "sigma", "delta", "labels", "info", "close"):
        assert hasattr(mini_amd.BcProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    assert lib.mgx_bc_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_bc_run(None, None, 0, 1, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_bc_enact(None, None, 0, 1, st) == mini_amd.MGX_E_INVALID
    for fn in (lib.mgx_bc_centrality, lib.mgx_bc_sigma, lib.mgx_bc_delta, lib.mgx_bc_labels):
        assert fn(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_bc_centrality_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_bc_info(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_bc_free(None) == 0


def test_bc_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert {"MGX_BC_LANE_MAX", "MGX_BC_HUGE_MIN", "MGX_BC_SEG", "MGX_BC_CHAIN"} <= names


def test_bc_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: every k_bc_* kernel uses no scratch and spills nothing"""
    path = os.path.join(ROOT, "mini_amd", "kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resource remarks"
    cur, res = None, {}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key, pat in (("scratch", r"ScratchSize[^:]*: (\d+)"), ("vspill", r"VGPRs Spill[^:]*: (\d+)"),
                         ("sspill", r"SGPRs Spill[^:]*: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                res.setdefault(cur, {})[key] = int(m.group(1))
    for name in KERNELS:
        found = [k for k in res if name in k]
        assert found, (name, sorted(k for k in res if "k_bc" in k))
    for k in res:
        if "k_bc_" in k:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


# ---- the model against networkx and against a textbook Brandes --------------------------------------------------------------------
def _textbook(ro, ci, sources=None):
    """Brandes as it is written down: BFS, then sigma over the entries whose head is one level deeper, then delta backwards over
    the same entries -- a label test per entry.  Entries count with multiplicity."""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    cols = np.asarray(ci, dtype=np.int64)
    bc = np.zeros(n)
    last = None
    for s in (range(n) if sources is None else sources):
        label = np.full(n, -1, dtype=np.int64)
        label[s] = 0
        d = 0
        while True:
            e = (label[rows] == d) & (label[cols] < 0)
            if not e.any():
                break
            d += 1
            label[cols[e]] = d
        sigma = np.zeros(n)
        sigma[s] = 1.0
        for lv in range(1, d + 1):
            e = (label[rows] == lv - 1) & (label[cols] == lv)
            np.add.at(sigma, cols[e], sigma[rows[e]])
        delta = np.zeros(n)
        for lv in range(d - 1, 0, -1):
            e = (label[rows] == lv) & (label[cols] == lv + 1)
            np.add.at(delta, rows[e], sigma[rows[e]] / sigma[cols[e]] * (1.0 + delta[cols[e]]))
        delta[s] = 0.0
        bc += delta
        last = (label.astype(np.int32), sigma, delta)
    return bc, last


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    zero = (a == 0) | (b == 0)
    assert np.array_equal(a[zero], b[zero]), "the exact zeros differ"
    big = np.maximum(np.abs(a), np.abs(b))
    assert (np.abs(a - b) <= rtol * big).all(), float((np.abs(a - b) / np.where(big > 0, big, 1)).max())


def _check_against_networkx(ro, ci, symmetric):
    import networkx as nx
    n = len(ro) - 1
    ro, ci = model.dedup(ro, ci)
    r = model.run(ro, ci, None, symmetric)
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(np.repeat(np.arange(n), np.diff(ro)).tolist(), ci.tolist()))
    want = nx.betweenness_centrality(g, normalized=False)
    want = np.array([want[v] for v in range(n)])
    # (both are sums of non-negative doubles in different orders: a few roundings per level and source)
    tol = model.rtol(r["stats"][1], max(r["longest_in"], r["longest_out"]), n)
    _close(r["bc"], want, tol)
    tb, last = _textbook(ro, ci)
    _close(r["bc"], tb, tol)
    assert np.array_equal(last[0], r["labels"]) and np.array_equal(last[1], r["sigma"])
    _close(last[2], r["delta"], tol)
    return r


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_model_equals_networkx_on_fixtures(oracle, name, undir):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check_against_networkx(ro, ci, False)
    if undir:
        _check_against_networkx(ro, ci, True)


@pytest.mark.parametrize("undir", [True, False])
def test_model_equals_networkx_on_rmat10(oracle, undir):
    n, ro, ci, _ = oracle.rmat_csr(10, 8, 10, undir=undir)
    r = _check_against_networkx(ro, ci, undir)
    assert r["max_sigma"] < model.TWO53 and r["stats"][3] == 0 and r["stats"][4] == 0


def _grid(w):
    v = np.arange(w * w).reshape(w, w)
    s, d = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return cm.csr(w * w, s, d)


def test_model_equals_networkx_on_a_grid():
    ro, ci = _grid(24)
    r = _check_against_networkx(ro, ci, True)
    assert r["stats"][1] == 47


def test_duplicates_count_and_self_loops_do_not():
    """the model on a multigraph against the textbook form with multiplicity; a self-loop changes nothing"""
    rng = np.random.default_rng(5)
    n = 60
    s, d = rng.integers(0, n, 200), rng.integers(0, n, 200)
    s2, d2 = np.concatenate([s, s[:50], s[:50]]), np.concatenate([d, d[:50], d[:50]])
    ro, ci = cm.csr(n, s2, d2, symmetric=False)
    r = model.run(ro, ci, None, False)
    tb, _ = _textbook(ro, ci)
    _close(r["bc"], tb, 1e-13)
    loops = np.arange(0, n, 3)
    ro2, ci2 = cm.csr(n, np.concatenate([s2, loops]), np.concatenate([d2, loops]), symmetric=False)
    r2 = model.run(ro2, ci2, None, False)
    assert np.array_equal(r2["bc"], r["bc"])


# ---- the model against brute force -------------------------------------------------------------------------------------------------
def _brute_force(n, src, dst):
    """enumerate the entry-walks of length dist(s, t) from s to t (each is a shortest entry-path): bc[v] = sum over s != v != t of the
    share of them that pass through v"""
    INF = 10 ** 9
    dist = np.full((n, n), INF, dtype=np.int64)
    np.fill_diagonal(dist, 0)
    for a, b in zip(src, dst):
        if a != b:
            dist[a, b] = 1
    for k in range(n):
        dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
    out = [[] for _ in range(n)]
    for a, b in zip(src, dst):
        out[a].append(b)
    bc = np.zeros(n)
    for s in range(n):
        for t in range(n):
            if s == t or dist[s, t] >= INF:
                continue
            total = 0
            through = np.zeros(n)
            stack = [(s, [s])]
            while stack:
                u, path = stack.pop()
                if len(path) - 1 == dist[s, t]:
                    if u == t:
                        total += 1
                        for v in path[1:-1]:
                            through[v] += 1
                    continue
                for w in out[u]:
                    if dist[s, w] == len(path) and dist[w, t] == dist[s, t] - len(path):      # (prunes only; every kept walk is shortest)
                        stack.append((w, path + [w]))
            bc += through / total
    return bc


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("symmetric", [False, True])
def test_model_equals_brute_force_on_small_multigraphs(seed, symmetric):
    rng = np.random.default_rng(100 + seed)
    n, m = 9, 16
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    s, d = np.concatenate([s, s[:5], [1, 4]]), np.concatenate([d, d[:5], [1, 4]])       # duplicates and two self-loops
    ro, ci = cm.csr(n, s, d, symmetric=symmetric)
    rows = np.repeat(np.arange(n), np.diff(ro))
    want = _brute_force(n, rows.tolist(), ci.tolist())
    got = model.run(ro, ci, None, symmetric)["bc"]
    _close(got, want, 1e-14)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_closed_forms():
    for n in (2, 3, 10, 41):                                             # a path: 2 i (n - 1 - i) over both directions
        a = np.arange(n - 1)
        bc = model.run(*cm.csr(n, a, a + 1), None, True)["bc"]
        assert np.array_equal(bc, 2.0 * np.arange(n) * (n - 1 - np.arange(n)))
    for k in (1, 2, 7, 30):                                              # a star: every ordered pair of leaves passes the centre
        bc = model.run(*cm.csr(k + 1, np.zeros(k, dtype=np.int64), 1 + np.arange(k)), None, True)["bc"]
        assert bc[0] == k * (k - 1) and not bc[1:].any()
    for n in (3, 4, 17):                                                 # a complete graph: nothing lies between
        assert not model.run(*cm.clique(n), None, True)["bc"].any()
    for k in (3, 5, 12):                                                 # two K_k joined by the bridge {0, k}
        s, d = [], []
        for ids in (np.arange(k), k + np.arange(k)):
            x, y = np.meshgrid(ids, ids, indexing="ij")
            s.append(x[x < y])
            d.append(y[x < y])
        s.append(np.array([0]))
        d.append(np.array([k]))
        bc = model.run(*cm.csr(2 * k, np.concatenate(s), np.concatenate(d)), None, True)["bc"]
        want = np.zeros(2 * k)
        want[0] = want[k] = 2.0 * k * (k - 1)
        assert np.array_equal(bc, want)


def test_identity_sum_of_delta(oracle):
    """for every source: sum over v of delta[v] = sum over the reached t != s of (label[t] - 1)"""
    for ro, ci, sym in ([*oracle.rmat_csr(10, 8, 10)[1:3], True], [*oracle.rmat_csr(10, 8, 10, undir=False)[1:3], False], [*_grid(12), True]):
        out, inn = model.matrices(ro, ci, sym)
        for s in range(0, len(ro) - 1, 7):
            label, sigma, delta = model.one_source(out, inn, s)
            want = float((label[label > 0] - 1).sum())
            assert abs(delta.sum() - want) <= 1e-12 * max(want, 1.0), (s, delta.sum(), want)
            assert delta[s] == 0.0


def test_grid_sides_and_two53():
    """C(56, 28) is below 2^53 and C(58, 29) is not: a 29 x 29 grid from a corner is exact, a 31 x 31 one sets `inexact`"""
    from math import comb
    assert comb(56, 28) < 2 ** 53 <= comb(58, 29)
    r = model.run(*_grid(29), [0], True)
    assert r["max_sigma"] == float(comb(56, 28)) and r["stats"][3:] == [0, 0]
    r = model.run(*_grid(31), [0], True)
    assert r["stats"][3:] == [1, 0]
