"""CPU suite for the triangle count (mgx_tc_*, include/mgx/tc_fused.hpp, include/gunrock/tc/): the library exports it, refuses
NULL handles, its kernels keep their registers, and the model the GPU tests compare against (tests/tc_model.py) agrees with
networkx, with closed forms and with a brute-force count."""
import ctypes as C
import os
import re
from math import comb

import numpy as np
import pytest

from tests import coloring_model as cm
from tests import tc_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
NAMES = ["mgx_tc_bins", "mgx_tc_create", "mgx_tc_free", "mgx_tc_run", "mgx_tc_enact", "mgx_tc_triangles", "mgx_tc_triangles_device",
         "mgx_tc_simple_degrees", "mgx_tc_simple_degrees_device", "mgx_tc_dag"]
KERNELS = ["k_tc_init", "k_tc_rowinfo", "k_tc_select", "k_tc_orient", "k_tc_check", "k_tc_sort_classify", "k_tc_dagstats",
           "k_tc_worklist", "k_tc_short", "k_tc_wave", "k_tc_block", "k_tc_sum"]


def test_library_exports_tc(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "TcProblem")
    for member in ("run", "enact", "triangles", "simple_degrees", "dag", "bins", "clustering", "transitivity", "close"):
        assert hasattr(mini_amd.TcProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    assert lib.mgx_tc_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_run(None, 1, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_enact(None, 0, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_triangles(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_triangles_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_simple_degrees(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_simple_degrees_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_dag(None, None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_bins(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_tc_free(None) == 0


def test_tc_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert {"MGX_TC_SHORT_MAX", "MGX_TC_WAVE_MAX", "MGX_TC_STAGE"} <= names


def test_tc_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the triangle-count kernels use no scratch and spill nothing"""
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
        assert found, (name, sorted(k for k in res if "k_tc" in k))
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


def _check_against_networkx(ro, ci, symmetric):
    import networkx as nx
    n = len(ro) - 1
    r = model.count(ro, ci, symmetric)
    g = model.simple_graph(ro, ci)
    want = nx.triangles(g)
    assert np.array_equal(r["tri"], np.array([want[v] for v in range(n)], dtype=np.int64))
    assert r["stats"]["triangles"] * 3 == int(r["tri"].sum())
    assert np.array_equal(r["sdeg"], np.array([g.degree(v) for v in range(n)], dtype=np.int32))
    # the DAG: ascending duplicate-free rows without self-loops, each simple edge exactly once
    dro, dci = r["dag_ro"].astype(np.int64), r["dag_ci"].astype(np.int64)
    assert dro[0] == 0 and dro[-1] == len(dci) == r["stats"]["edges"] == g.number_of_edges()
    rows = np.repeat(np.arange(n), np.diff(dro))
    assert (rows != dci).all()
    same_row = rows[1:] == rows[:-1]
    assert (dci[1:][same_row] > dci[:-1][same_row]).all()
    pairs = set(zip(np.minimum(rows, dci).tolist(), np.maximum(rows, dci).tolist()))
    assert len(pairs) == len(dci)
    assert pairs == {(min(a, b), max(a, b)) for a, b in g.edges()}
    # the per-entry supports ((L L^T) o L): the same triangles counted where the GPU paths count them
    sup = model.supports(r["dag_ro"], r["dag_ci"])
    third = np.zeros(n, dtype=np.int64)
    for a in range(n):
        row_a = dci[dro[a]:dro[a + 1]]
        for b in row_a:
            np.add.at(third, np.intersect1d(row_a, dci[dro[b]:dro[b + 1]], assume_unique=True), 1)
    assert int(sup.sum()) == r["stats"]["triangles"]
    assert np.array_equal(np.asarray(sup.sum(axis=1)).ravel() + np.asarray(sup.sum(axis=0)).ravel() + third, r["tri"])
    d = np.diff(dro)
    assert r["stats"]["max_row"] == (int(d.max()) if n else 0) and r["stats"]["wedges"] == int((d * (d - 1) // 2).sum())
    return r


@pytest.mark.parametrize("n,m,symmetric,seed", [(1, 0, True, 1), (40, 120, True, 2), (40, 120, False, 3), (300, 2000, True, 4),
                                                (300, 2000, False, 5), (2000, 9000, True, 6), (2000, 9000, False, 7)])
def test_model_equals_networkx_on_random_graphs(n, m, symmetric, seed):
    """self-loops and every pair three times, symmetric and directed"""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    loops = np.arange(0, n, 5)
    s, d = np.concatenate([s, s, s, loops]), np.concatenate([d, d, d, loops])
    ro, ci = cm.csr(n, s, d, symmetric=symmetric)
    r = _check_against_networkx(ro, ci, symmetric)
    if symmetric:                                        # a symmetric graph counts the same without the caller's word
        r0 = model.count(ro, ci, False)
        assert np.array_equal(r0["tri"], r["tri"]) and np.array_equal(r0["sdeg"], r["sdeg"])
        assert r["stats"]["rows_sorted"] == 1 and r0["stats"]["rows_sorted"] == 0


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_model_equals_networkx_on_fixtures(oracle, name, undir):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check_against_networkx(ro, ci, False)
    if undir:
        _check_against_networkx(ro, ci, True)


def _totals(ro, ci, symmetric=True):
    r = model.count(ro, ci, symmetric)
    return r["stats"]["triangles"], r["tri"]


def test_closed_forms():
    for n in (3, 4, 17, 60):
        total, tri = _totals(*cm.clique(n))
        assert total == comb(n, 3) and (tri == comb(n - 1, 2)).all()
    p, q = 7, 9                                                          # K_{p,q}
    s, d = np.meshgrid(np.arange(p), p + np.arange(q), indexing="ij")
    total, tri = _totals(*cm.csr(p + q, s.ravel(), d.ravel()))
    assert total == 0 and not tri.any()
    w = 20                                                               # a w x w grid
    v = np.arange(w * w).reshape(w, w)
    s, d = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    total, tri = _totals(*cm.csr(w * w, s, d))
    assert total == 0 and not tri.any()
    for k in (3, 4, 9, 40):                                              # a wheel: hub 0, rim 1 .. k
        rim = 1 + np.arange(k)
        s, d = np.concatenate([np.zeros(k, np.int64), rim]), np.concatenate([rim, 1 + (rim % k)])
        total, tri = _totals(*cm.csr(k + 1, s, d))
        if k == 3:                                                       # W_3 is K_4
            assert total == 4
        else:
            assert total == k and tri[0] == k and (tri[1:] == 2).all()
    k = 12                                                               # two K_k that share the edge {0, 1}
    a, b = np.arange(k), np.concatenate([[0, 1], k + np.arange(k - 2)])
    s, d = [], []
    for ids in (a, b):
        x, y = np.meshgrid(ids, ids, indexing="ij")
        s.append(x[x < y])
        d.append(y[x < y])
    total, tri = _totals(*cm.csr(2 * k - 2, np.concatenate(s), np.concatenate(d)))
    assert total == 2 * comb(k, 3)
    assert tri[0] == tri[1] == 2 * comb(k - 1, 2) and (tri[2:] == comb(k - 1, 2)).all()


def test_model_rmat14_equals_brute_force(oracle):
    """every oriented entry (a, b): the common elements of rows a and b, by plain numpy"""
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 14)
    r = model.count(ro, ci, True)
    dro, dci = r["dag_ro"], r["dag_ci"]
    total = 0
    tri = np.zeros(n, dtype=np.int64)
    for a in range(n):
        row_a = dci[dro[a]:dro[a + 1]]
        for b in row_a:
            common = np.intersect1d(row_a, dci[dro[b]:dro[b + 1]], assume_unique=True)
            if len(common):
                total += len(common)
                tri[a] += len(common)
                tri[b] += len(common)
                tri[common] += 1
    assert total == r["stats"]["triangles"] and total > 0
    assert np.array_equal(tri, r["tri"])
