"""CPU suite for the k-truss decomposition (mgx_ktruss_*, include/mgx/ktruss_fused.hpp, include/gunrock/ktruss/): the library
exports it, refuses NULL handles, its kernels keep their registers, and the model the GPU tests compare against
(tests/ktruss_model.py) agrees with networkx.k_truss for every k and with closed forms."""
import ctypes as C
import os
import re
from math import comb

import numpy as np
import pytest

from tests import coloring_model as cm
from tests import ktruss_cases as cases
from tests import ktruss_model as model
from tests import tc_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
NAMES = ["mgx_ktruss_create", "mgx_ktruss_free", "mgx_ktruss_run", "mgx_ktruss_enact", "mgx_ktruss_edges", "mgx_ktruss_support",
         "mgx_ktruss_vertex_truss", "mgx_ktruss_histogram", "mgx_ktruss_order", "mgx_ktruss_adjacency", "mgx_ktruss_truss_device",
         "mgx_ktruss_vertex_truss_device", "mgx_ktruss_step_kinds", "mgx_ktruss_set_timing", "mgx_ktruss_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts; ILb1E is <true>)
KERNELS = [("k_ktruss_adj_fill",), ("k_ktruss_adj_check",), ("k_ktruss_sum",), ("k_ktruss_step",), ("k_tc_shortILb1E",),
           ("k_tc_waveILb1E",), ("k_tc_blockILb1E",), ("6ktruss", "support_functor_t"), ("6ktruss", "collect_functor_t"),
           ("6ktruss", "expand_functor_t"), ("6ktruss", "seal_functor_t")]


def test_library_exports_ktruss(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "KtrussProblem")
    assert mini_amd.KtrussProblem.KEYS == ("max_truss", "edges", "triangles", "levels", "passes", "built", "host_waits", "launches")
    for member in ("run", "enact", "edges", "support", "vertex_truss", "histogram", "order", "adjacency", "step_kinds", "truss_edges",
                   "close"):
        assert hasattr(mini_amd.KtrussProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    n = C.c_int64()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_ktruss_create(None, C.byref(h)) == bad
    assert lib.mgx_ktruss_run(None, 1, st) == bad
    assert lib.mgx_ktruss_enact(None, 0, st) == bad
    assert lib.mgx_ktruss_edges(None, None, None, None) == bad
    assert lib.mgx_ktruss_support(None, None) == bad
    assert lib.mgx_ktruss_vertex_truss(None, None) == bad
    assert lib.mgx_ktruss_histogram(None, None, 0) == bad
    assert lib.mgx_ktruss_order(None, None) == bad
    assert lib.mgx_ktruss_adjacency(None, None, None, None) == bad
    assert lib.mgx_ktruss_truss_device(None, C.byref(p)) == bad
    assert lib.mgx_ktruss_vertex_truss_device(None, C.byref(p)) == bad
    assert lib.mgx_ktruss_step_kinds(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_ktruss_set_timing(None, 1) == bad
    assert lib.mgx_ktruss_phase_ms(None, None) == bad
    assert lib.mgx_ktruss_free(None) == 0


def test_ktruss_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert {"MGX_KTRUSS_SHORT_MAX", "MGX_KTRUSS_SEG"} <= names


def test_ktruss_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the new kernels, the count kernels with the adds sent to the entries and the
    operator path's instantiations use no scratch and spill nothing"""
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
    for parts in KERNELS:
        found = [k for k in res if all(x in k for x in parts)]
        assert found, parts
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


def _check_against_networkx(ro, ci, symmetric):
    import networkx as nx
    n = len(ro) - 1
    r = model.decompose(ro, ci, symmetric)
    g = tc_model.simple_graph(ro, ci)
    st = r["stats"]
    assert st["edges"] == g.number_of_edges() and 3 * st["triangles"] == int(r["sup0"].sum()) == sum(nx.triangles(g).values())
    # supports: the triangles of each edge
    for a, b, s in list(zip(r["u"].tolist(), r["v"].tolist(), r["sup0"][r["perm"]].tolist()))[:2000]:
        assert s == len(set(g[a]) & set(g[b])), (a, b)
    # the adjacency: every row the sorted neighbours, every entry's edge id names the pair
    ro_a, ci_a, eid = r["adj_ro"].astype(np.int64), r["adj_ci"], r["adj_eid"]
    rows = np.repeat(np.arange(n), np.diff(ro_a))
    assert len(ci_a) == 2 * st["edges"]
    assert all(ci_a[ro_a[v]:ro_a[v + 1]].tolist() == sorted(g[v]) for v in range(n))
    assert np.array_equal(np.minimum(rows, ci_a), np.minimum(r["src"], r["dag_ci"])[eid])
    assert np.array_equal(np.maximum(rows, ci_a), np.maximum(r["src"], r["dag_ci"])[eid])
    # every k-truss
    assert (r["truss"] >= 2).all() and int(r["hist"].sum()) == st["edges"]
    for k in range(2, st["max_truss"] + 2):
        want = {(min(a, b), max(a, b)) for a, b in nx.k_truss(g, k).edges()}
        assert model.truss_edge_set(r, k) == want, k
    # every edge enters a front exactly once
    order = np.concatenate(r["fronts"]) if r["fronts"] else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(order), np.arange(st["edges"])) and len(r["fronts"]) == st["passes"]
    vt = np.zeros(n, np.int32)
    for a, b, t in zip(r["src"].tolist(), r["dag_ci"].tolist(), r["truss"].tolist()):
        vt[a], vt[b] = max(vt[a], t), max(vt[b], t)
    assert np.array_equal(vt, r["vtruss"])
    return r


@pytest.mark.parametrize("n,m,seed", [(200, 2000, 1), (200, 2000, 2), (200, 2000, 3), (1000, 20000, 4), (1000, 20000, 5)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_model_equals_networkx_on_random_graphs(n, m, seed, symmetric):
    """self-loops and every pair three times, symmetric and directed"""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    loops = np.arange(0, n, 5)
    ro, ci = cm.csr(n, np.concatenate([s, s, s, loops]), np.concatenate([d, d, d, loops]), symmetric=symmetric)
    r = _check_against_networkx(ro, ci, symmetric)
    assert r["stats"]["max_truss"] >= 3
    if symmetric:                                        # the canonical form does not depend on the orientation
        r0 = model.decompose(ro, ci, False)
        assert np.array_equal(r0["u"], r["u"]) and np.array_equal(r0["v"], r["v"])
        assert np.array_equal(r0["truss"][r0["perm"]], r["truss"][r["perm"]]) and r0["stats"] == r["stats"]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_model_equals_networkx_on_fixtures(oracle, name, undir):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check_against_networkx(ro, ci, False)
    if undir:
        _check_against_networkx(ro, ci, True)


def _stats(ro, ci):
    r = model.decompose(ro, ci, True)
    return r, r["stats"]


def test_closed_forms():
    for n in (3, 4, 17, 60):                                             # K_n: every edge n, one level, one pass
        r, st = _stats(*cm.clique(n))
        assert (r["truss"] == n).all() and st["levels"] == 1 and st["passes"] == 1 and st["triangles"] == comb(n, 3)
        assert (r["sup0"] == n - 2).all() and (r["vtruss"] == n).all() and r["hist"][n] == comb(n, 2)
    for p, q in ((5, 9), (12, 12), (30, 4)):                             # two cliques sharing one edge
        ro, ci, ids = cases.two_cliques_sharing_an_edge(p, q)
        r, st = _stats(ro, ci)
        t = dict(zip(zip(r["u"].tolist(), r["v"].tolist()), r["truss"][r["perm"]].tolist()))
        assert t[(0, 1)] == max(p, q) and st["max_truss"] == max(p, q)
        assert sorted(set(t.values())) == sorted({p, q}) and st["levels"] == len({p, q})
        assert r["hist"][min(p, q)] == (comb(p, 2) + comb(q, 2) - 1 if p == q else comb(min(p, q), 2) - 1)
    for ro, ci in (cases.star(50, 7), cm.csr(40, np.arange(1, 40), (np.arange(1, 40) - 1) // 2), cases.grid(20, 13, False)):
        r, st = _stats(ro, ci)                                           # star, tree, plain grid: all 2
        assert (r["truss"] == 2).all() and st == {"max_truss": 2, "edges": len(r["truss"]), "triangles": 0, "levels": 1, "passes": 1}
    s, d = np.meshgrid(np.arange(7), 7 + np.arange(9), indexing="ij")    # K_{7,9}
    r, st = _stats(*cm.csr(16, s.ravel(), d.ravel()))
    assert (r["truss"] == 2).all() and st["edges"] == 63 and st["passes"] == 1
    r, st = _stats(*cases.disjoint_triangles(25))
    assert (r["truss"] == 3).all() and st["triangles"] == 25 and st["levels"] == 1 and st["passes"] == 1
    r, st = _stats(*cases.clique_chain(2, 40))
    assert st["max_truss"] == 40 and st["levels"] == 39 and st["passes"] == 39
    assert all(r["hist"][k] == comb(k, 2) for k in range(2, 41))


@pytest.mark.parametrize("w,h", [(8, 8), (64, 64), (100, 40)])
def test_triangulated_grid_peels_in_min_w_h_passes(w, h):
    r, st = _stats(*cases.grid(w, h, True))
    assert (r["truss"] == 3).all() and st["levels"] == 1 and st["passes"] == min(w, h)
    assert st["triangles"] == 2 * (w - 1) * (h - 1) and st["edges"] == (w - 1) * h + w * (h - 1) + (w - 1) * (h - 1)
