"""CPU suite for the minimum spanning forest (mgx_mst_*, include/mgx/mst_fused.hpp, include/gunrock/mst/): the library exports it,
refuses NULL handles, its kernels keep their registers, its switches are in the table, and the models the GPU tests compare against
(tests/mst_model.py) agree with networkx, with scipy, with a brute force over all spanning trees and with each other on every input
of the GPU suite up to RMAT-14."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import cc_model
from tests import mst_cases as cases
from tests import mst_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["mgx_mst_create", "mgx_mst_free", "mgx_mst_run", "mgx_mst_enact", "mgx_mst_edges", "mgx_mst_edges_device", "mgx_mst_weight",
         "mgx_mst_labels", "mgx_mst_labels_device", "mgx_mst_info"]
KERNELS = ["k_mst_incident", "k_mst_sort_classify", "k_mst_init", "k_mst_worklist", "k_mst_scan", "k_mst_weight", "k_mst_pair",
           "k_mst_hook", "k_mst_compress", "k_mst_sum_tiles", "k_mst_finish"]


def test_library_exports_mst(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "MstProblem")
    for member in ("run", "enact", "edges", "weight", "labels", "info", "edges_device_ptrs", "close"):
        assert hasattr(mini_amd.MstProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    t = C.c_double()
    assert lib.mgx_mst_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_run(None, 1, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_enact(None, 1, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_edges(None, None, None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_edges_device(None, C.byref(p), C.byref(p), C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_weight(None, C.byref(t)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_labels(None, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_labels_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_info(None, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_mst_free(None) == 0


def test_mst_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert {"MGX_MST_LONG_MIN", "MGX_MST_SEG"} <= names


def test_mst_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the forest's kernels use no scratch and spill nothing"""
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
        assert found, (name, sorted(k for k in res if "mst" in k))
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


# ---- the model against others ------------------------------------------------------------------------------------------------
def test_key_is_monotone_and_folds_the_zeros():
    fmax = np.finfo(np.float32).max
    w = np.array([-np.inf, -fmax, -2.0, -1.5, -1e-40, -0.0, 0.0, 1e-40, 1.0, 1.5, fmax, np.inf], dtype=np.float32)
    k = model.key(w).astype(np.int64)
    assert k[5] == k[6] == 0x80000000
    assert (np.diff(np.delete(k, 5)) > 0).all()
    back = model.weight_of_key(model.key(w))
    assert np.array_equal(np.delete(back, 5).view(np.uint32), np.delete(w, 5).view(np.uint32))
    assert back[5].view(np.uint32) == 0                                         # -0.0 comes back as +0.0


def _random_pairs(rng, n, m):
    """m distinct pairs a < b"""
    s, d = rng.integers(0, n, 3 * m), rng.integers(0, n, 3 * m)
    a, b = np.minimum(s, d), np.maximum(s, d)
    keep = a != b
    pairs = np.unique(np.stack([a[keep], b[keep]], axis=1), axis=0)
    return pairs[rng.permutation(len(pairs))[:m]]


@pytest.mark.parametrize("n,m,seed", [(30, 60, 1), (200, 300, 2), (1000, 5000, 3), (3000, 4000, 4)])
def test_model_equals_networkx_on_distinct_weights(n, m, seed):
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(seed)
    pairs = _random_pairs(rng, n, m)
    w = rng.permutation(len(pairs)).astype(np.float32) - 7.0               # distinct, some negative
    ro, ci, ww = cases.wcsr(n, pairs[:, 0], pairs[:, 1], w)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from((int(a), int(b), float(x)) for (a, b), x in zip(pairs, w))
    want = sorted((min(a, b), max(a, b), d["weight"]) for a, b, d in nx.minimum_spanning_edges(g, data=True))
    (a, b, x), total, lab = model.kruskal(ro, ci, ww)
    assert sorted(zip(a.tolist(), b.tolist(), x.tolist())) == want
    assert total == sum(t[2] for t in want)
    bo = model.boruvka(ro, ci, ww)
    assert model.same_triples(bo["edges"], (a, b, x)) and np.array_equal(bo["labels"], lab)


@pytest.mark.parametrize("n,m,seed", [(100, 300, 5), (2000, 10000, 6), (5000, 6000, 7)])
def test_model_total_equals_networkx_and_scipy_on_tied_weights(n, m, seed):
    """weights 0 .. 7 (the R-MAT inputs' are % 64: heavy ties, zeros among them).  scipy's csgraph reads a weight of 0 as "no edge":
    it gets every weight + 1, and its total is corrected by the number of edges"""
    nx = pytest.importorskip("networkx")
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(seed)
    pairs = _random_pairs(rng, n, m)
    w = rng.integers(0, 8, len(pairs)).astype(np.float32)
    ro, ci, ww = cases.wcsr(n, pairs[:, 0], pairs[:, 1], w)
    (a, b, x), total, lab = model.kruskal(ro, ci, ww)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from((int(p), int(q), float(y)) for (p, q), y in zip(pairs, w))
    nx_edges = list(nx.minimum_spanning_edges(g, data=True))
    assert len(nx_edges) == len(a) == n - len(np.unique(lab))
    assert total == sum(d["weight"] for _, _, d in nx_edges)
    m1 = sp.csr_matrix((w.astype(np.float64) + 1.0, (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    t = csgraph.minimum_spanning_tree(m1)
    assert t.nnz == len(a)
    assert total == float(t.sum()) - t.nnz
    assert model.boruvka(ro, ci, ww)["total"] == total


def _root(p, x):
    while p[x] != x:
        x = p[x]
    return x


def _is_forest(n, edges):
    p = list(range(n))
    for _, a, b in edges:
        ra, rb = _root(p, a), _root(p, b)
        if ra == rb:
            return False
        p[max(ra, rb)] = min(ra, rb)
    return True


@pytest.mark.parametrize("n,m,seed", [(4, 5, 1), (5, 8, 2), (6, 9, 3), (7, 10, 4), (7, 11, 5), (6, 6, 6)])
def test_model_equals_brute_force(n, m, seed):
    """over every acyclic subset of n - components distinct triples (key, a, b): the model's forest has the smallest total, and
    among all of them the smallest sorted sequence of triples (what "minimum under the strict order" means: the greedy forest of a
    matroid is the lexicographically smallest)"""
    rng = np.random.default_rng(seed)
    pairs = _random_pairs(rng, n, m)
    w = rng.integers(-1, 3, len(pairs)).astype(np.float32)                 # ties everywhere
    ro, ci, ww = cases.wcsr(n, pairs[:, 0], pairs[:, 1], w)
    triples = sorted({(int(k), int(a), int(b)) for (a, b), k in zip(pairs, model.key(w))})
    (a, b, x), total, lab = model.kruskal(ro, ci, ww)
    size = n - len(np.unique(lab))
    forests = [s for s in itertools.combinations(triples, size) if _is_forest(n, s)]
    assert forests
    mine = tuple(sorted(zip(model.key(x).tolist(), a.tolist(), b.tolist())))
    assert mine == min(forests)
    value = {int(k): float(y) for k, y in zip(model.key(w), w)}
    assert total == min(sum(value[k] for k, _, _ in s) for s in forests)
    assert model.same_triples(model.boruvka(ro, ci, ww)["edges"], (a, b, x))


# ---- the two models against each other, on the GPU suite's inputs -------------------------------------------------------------
def _agree(ro, ci, w, symmetric):
    (a, b, x), total, lab = model.kruskal(ro, ci, w)
    bo = model.boruvka(ro, ci, w, symmetric=symmetric)
    n = len(ro) - 1
    assert model.same_triples(bo["edges"], (a, b, x))
    assert np.array_equal(bo["labels"], lab) and np.array_equal(lab, cc_model.labels(ro, ci))
    assert len(a) == n - len(np.unique(lab))
    assert abs(bo["total"] - total) <= model.total_bound(x)
    keep = np.repeat(np.arange(n), np.diff(ro)) != ci
    assert bo["entries"] == int(keep.sum()) * (1 if symmetric else 2)
    return bo


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_models_agree_on_the_gpu_cases(name):
    ro, ci, w, symmetric = cases.CASES[name]()
    bo = _agree(ro, ci, w, symmetric)
    if name.startswith("no_entries") or name == "self_loops_only":
        assert bo["rounds"] == 0 and len(bo["edges"][0]) == 0
    if name == "increasing_path_4096":
        assert len(bo["edges"][0]) == 4095


def test_model_refuses_nan():
    ro, ci, w, _ = cases.one_nan()
    assert model.has_nan(ro, ci, w)
    with pytest.raises(ValueError):
        model.kruskal(ro, ci, w)
    ro, ci, w, _ = cases.self_loops_only(10)
    w[:] = np.nan                                                          # a NaN on a self-loop is ignored with it
    assert not model.has_nan(ro, ci, w)
    assert len(model.kruskal(ro, ci, w)[0][0]) == 0


@pytest.mark.parametrize("scale,ef", cases.RMAT_SYMMETRIC[:5])
def test_models_agree_on_rmat_symmetric(oracle, scale, ef):
    n, ro, ci, w = oracle.rmat_csr(scale, ef, scale)
    _agree(ro, ci, w, True)


@pytest.mark.parametrize("scale,ef", cases.RMAT_DIRECTED)
def test_models_agree_on_rmat_directed(oracle, scale, ef):
    n, ro, ci, w = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    _agree(ro, ci, w, False)


@pytest.mark.parametrize("name", cases.FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_models_agree_on_the_fixtures(oracle, name, undir):
    n, ro, ci, w, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _agree(ro, ci, w, undir)
