"""CPU suite: the numpy model of PageRank (tests/pagerank_model.py) against networkx.pagerank -- a MultiDiGraph, so that
duplicate entries count once each -- and against cases worked by hand."""
import os

import numpy as np
import pytest

from tests import coloring_model as cm
from tests import pagerank_model as model

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
TOL = 1e-13


def _networkx(ro, ci, alpha, tol):
    import networkx as nx
    n = len(ro) - 1
    g = nx.MultiDiGraph()
    g.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(ro))
    g.add_edges_from(zip(rows.tolist(), np.asarray(ci).tolist()))
    pr = nx.pagerank(g, alpha=alpha, tol=tol / n, max_iter=10000)        # (networkx stops at e < n * tol)
    return np.array([pr[v] for v in range(n)])


def _check(ro, ci, symmetric, alpha=0.85):
    r, res = model.ranks(ro, ci, alpha, TOL, 10000, symmetric)
    assert res[-1] <= TOL
    assert abs(r.sum() - 1.0) <= 1e-12
    want = _networkx(ro, ci, alpha, TOL)
    assert np.abs(r - want).max() <= 1e-9
    return r


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_fixtures_against_networkx(oracle, name, undir):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check(ro, ci, symmetric=undir)
    if undir:                                  # a symmetric graph read through its transpose is the same graph
        a, _ = model.ranks(ro, ci, 0.85, TOL, 10000, True)
        b, _ = model.ranks(ro, ci, 0.85, TOL, 10000, False)
        assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("scale,ef", [(10, 8), (12, 4)])
@pytest.mark.parametrize("undir", [True, False])
def test_rmat_against_networkx(oracle, scale, ef, undir):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale, undir=undir)
    _check(ro, ci, symmetric=undir)


@pytest.mark.parametrize("alpha", [0.5, 0.99])
def test_other_dampings_against_networkx(oracle, alpha):
    n, ro, ci, _ = oracle.rmat_csr(10, 4, 3, undir=False)
    _check(ro, ci, symmetric=False, alpha=alpha)


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_all_dangling_is_uniform(n):
    ro, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    for symmetric in (True, False):
        r, res = model.ranks(ro, ci, 0.85, 0.0, 50, symmetric)
        # (1 - alpha) / n + alpha * (n * (1 / n)) / n is 1 / n up to a rounding of float64: the residual is 0 or a few 1e-16
        assert len(res) <= 2 and res[-1] == 0.0 and res[0] <= 1e-15
        assert np.allclose(r, 1.0 / n, rtol=1e-14, atol=0)


def test_three_vertices_by_hand():
    """0 -> 1, 0 -> 2, 1 -> 2; vertex 2 dangles.  alpha = 1/2, r_0 = (1/3, 1/3, 1/3):
         D_0 = 1/3, S_0 = (0, 1/6, 1/6 + 1/3) -> r_1 = 1/6 + 1/2 (S_0 + 1/9) = (4/18, 11/36, 17/36), e_1 = 1/9 + 1/36 + 5/36 = 5/18
         D_1 = 17/36, S_1 = (0, 1/9, 1/9 + 11/36) -> r_2 = 1/6 + 1/2 (S_1 + 17/108) = (53/216, 65/216, 98/216)"""
    ro, ci = np.array([0, 2, 3, 3]), np.array([1, 2, 2])
    r1, res = model.ranks(ro, ci, 0.5, 0.0, 1, False)
    assert np.allclose(r1, [4 / 18, 11 / 36, 17 / 36], rtol=1e-15, atol=0) and abs(res[0] - 5 / 18) < 1e-15
    r2, res = model.ranks(ro, ci, 0.5, 0.0, 2, False)
    assert np.allclose(r2, [53 / 216, 65 / 216, 98 / 216], rtol=1e-15, atol=0) and len(res) == 2
    assert abs(r2.sum() - 1.0) < 1e-15
    # duplicates count once each, self-loops count: 0 -> 1 twice and 0 -> 0; d(0) = 3, nothing dangles but 1
    ro, ci = np.array([0, 3, 3]), np.array([0, 1, 1])
    r1, _ = model.ranks(ro, ci, 0.5, 0.0, 1, False)
    # r_0 = (1/2, 1/2), D = 1/2, S = (1/6, 2/6) -> r_1 = 1/4 + 1/2 (S + 1/4) = (11/24, 13/24)
    assert np.allclose(r1, [11 / 24, 13 / 24], rtol=1e-15, atol=0)


def test_stops_at_the_first_residual_within_tol_or_at_max_iter(oracle):
    n, ro, ci, _ = oracle.rmat_csr(10, 8, 10)
    _, res = model.ranks(ro, ci, 0.85, 0.0, 30, True)
    assert len(res) == 30 and (np.diff(res) < 0).all()
    tol = float(np.sqrt(res[6] * res[7]))
    _, short = model.ranks(ro, ci, 0.85, tol, 30, True)
    assert len(short) == 8 and np.array_equal(short, res[:8])


def test_symmetric_flag_reads_the_rows_as_they_stand():
    ro, ci = cm.csr(50, np.arange(49), np.arange(1, 50), symmetric=False)        # a directed path
    a, _ = model.ranks(ro, ci, 0.85, 1e-12, 500, False)
    b, _ = model.ranks(ro, ci, 0.85, 1e-12, 500, True)
    assert a[49] > a[0] and not np.allclose(a, b)


# ---- the library side that needs no GPU --------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_pagerank_create", "mgx_pagerank_free", "mgx_pagerank_run", "mgx_pagerank_enact", "mgx_pagerank_ranks",
         "mgx_pagerank_ranks_device", "mgx_pagerank_residuals", "mgx_pagerank_bins"]
KERNELS = ["k_pagerank_init", "k_pagerank_begin", "k_pagerank_reduce", "k_pagerank_huge_list", "k_pagerank_reduce_huge",
           "k_pagerank_update", "k_pagerank_verdict", "k_pagerank_unpermute", "k_pagerank_iota"]


def test_library_exports_pagerank(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "PageRankProblem")


def test_null_arguments_are_invalid(built):
    import ctypes as C
    import mini_amd
    lib = mini_amd.lib
    h, p, it = C.c_void_p(), C.c_void_p(), C.c_int()
    st, res = (C.c_int64 * 6)(), C.c_double()
    assert lib.mgx_pagerank_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_run(None, 0.85, 1e-6, 10, 1, st, C.byref(res)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_enact(None, 0.85, 1e-6, 10, 1, st, C.byref(res)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_ranks(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_ranks_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_residuals(None, None, 0, C.byref(it)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_bins(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_pagerank_free(None) == 0


def test_pagerank_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the PageRank kernels use no scratch and spill nothing"""
    import re
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
        assert found, (name, sorted(k for k in res if "pagerank" in k))
        for k in found:
            assert res[k] == {"scratch": 0, "vspill": 0, "sspill": 0}, (k, res[k])
