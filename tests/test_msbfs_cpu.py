"""CPU suite for the bit-parallel multi-source BFS (mgx_msbfs_*, include/mgx/msbfs_fused.hpp, include/gunrock/msbfs/): the header
declares and the library exports them, NULL handles and arguments are statuses, the switches are in the table, the step kernel
keeps its registers, and the model the GPU tests compare against (tests/msbfs_model.py) has the properties and closed forms of
the definition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import msbfs_cases as cases
from tests import msbfs_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
NAMES = ["mgx_msbfs_create", "mgx_msbfs_free", "mgx_msbfs_run", "mgx_msbfs_enact", "mgx_msbfs_reach", "mgx_msbfs_far", "mgx_msbfs_ecc",
         "mgx_msbfs_harmonic", "mgx_msbfs_vertex_sums", "mgx_msbfs_vertex_sums_device", "mgx_msbfs_depths", "mgx_msbfs_level_kinds",
         "mgx_msbfs_bins", "mgx_msbfs_set_timing", "mgx_msbfs_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts; k_msbfs_step holds both EXPAND bodies)
KERNELS = [("k_msbfs_step",), ("5msbfs", "expand_functor_t"), ("5msbfs", "finalize_functor_t"), ("5msbfs", "clear_functor_t")]
SWITCHES = {"MGX_MSBFS_SHORT_MAX", "MGX_MSBFS_WAVE_MAX", "MGX_MSBFS_SEG", "MGX_MSBFS_PULL_DIV"}


def test_header_declares_and_library_exports_msbfs(built):
    import mini_amd
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    for name in NAMES:
        assert re.search(r"MGX_API int %s\(" % name, header), name
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "MsBfsProblem")
    assert mini_amd.MsBfsProblem.KEYS == ("sources", "batches", "deepest", "reach", "push_levels", "pull_levels", "host_waits", "launches",
                                          "csc", "depths")
    assert (mini_amd.MsBfsProblem.PUSH, mini_amd.MsBfsProblem.PULL) == (model.PUSH, model.PULL)
    for member in ("run", "enact", "reach", "farness", "eccentricity", "harmonic", "closeness", "vertex_sums", "depths", "level_kinds",
                   "bins", "set_timing", "phase_ms", "close"):
        assert hasattr(mini_amd.MsBfsProblem, member), member
    assert "OUT-closeness" in mini_amd.MsBfsProblem.__doc__


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    n = C.c_int64()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_msbfs_create(None, C.byref(h)) == bad
    assert lib.mgx_msbfs_run(None, None, 0, 1, 0, st) == bad
    assert lib.mgx_msbfs_enact(None, None, 0, 1, 0, st) == bad
    for fn in (lib.mgx_msbfs_reach, lib.mgx_msbfs_far, lib.mgx_msbfs_ecc, lib.mgx_msbfs_harmonic, lib.mgx_msbfs_depths):
        assert fn(None, None) == bad
    assert lib.mgx_msbfs_vertex_sums(None, None, None) == bad
    assert lib.mgx_msbfs_vertex_sums_device(None, C.byref(p), C.byref(q)) == bad
    assert lib.mgx_msbfs_level_kinds(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_msbfs_bins(None, None) == bad
    assert lib.mgx_msbfs_set_timing(None, 1) == bad
    assert lib.mgx_msbfs_phase_ms(None, None) == bad
    assert lib.mgx_msbfs_free(None) == 0


def test_msbfs_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names


def test_msbfs_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the step kernel (both EXPAND bodies, LONG and FINALIZE) and the operator path's
    instantiations use no scratch and spill nothing"""
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


def _rows_equal_oracle(oracle, ro, ci, sources, r):
    for i, s in enumerate(sources):
        assert np.array_equal(r["depths"][i], oracle.bfs_cpu(ro, ci, int(s))), (i, s)


def _consistent(r, n):
    """the per-source and per-vertex results are what the depth matrix says"""
    d = r["depths"].astype(np.int64)
    pos = d >= 1
    assert np.array_equal(r["reach"], pos.sum(axis=1)) and np.array_equal(r["far"], np.where(pos, d, 0).sum(axis=1))
    assert np.array_equal(r["ecc"], np.where(pos, d, 0).max(axis=1, initial=0))
    assert np.array_equal(r["reach_in"], pos.sum(axis=0)) and np.array_equal(r["far_in"], np.where(pos, d, 0).sum(axis=0))
    for i in range(len(d)):
        cnt = np.bincount(d[i][pos[i]], minlength=2)
        h = np.float64(0.0)
        for depth in range(1, len(cnt)):
            if cnt[depth]:
                h += np.float64(cnt[depth]) / np.float64(depth)
        assert r["harm"][i] == h
    assert r["stats"]["reach"] == int(pos.sum()) and r["stats"]["deepest"] == (int(d.max(initial=0)) + 1 if len(d) and n else 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_depth_rows_equal_the_oracle_on_the_fixtures(oracle, name):
    for undir in (True, False):
        n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
        r = model.traverse(ro, ci, None, symmetric=undir, csc=True)
        _rows_equal_oracle(oracle, ro, ci, range(n), r)
        _consistent(r, n)
        assert r["stats"]["batches"] == (n + 63) // 64 and len(r["kinds"]) == r["stats"]["push_levels"] + r["stats"]["pull_levels"]


@pytest.mark.parametrize("symmetric", [True, False])
def test_depth_rows_equal_the_oracle_on_random_graphs(oracle, symmetric):
    n = 700
    ro, ci = cases.random_symmetric(n, 1500, 3) if symmetric else cases.random_digraph(n, 2500, 4)
    rng = np.random.default_rng(5)
    sources = np.concatenate([rng.integers(0, n, 129), [7, 7]])          # three batches, duplicates
    r = model.traverse(ro, ci, sources, symmetric=symmetric, csc=True)
    _rows_equal_oracle(oracle, ro, ci, sources, r)
    _consistent(r, n)
    assert np.array_equal(r["depths"][-1], r["depths"][-2])
    for div in (0, 1 << 30):                                             # the kind changes no result
        f = model.traverse(ro, ci, sources, symmetric=symmetric, csc=True, pull_div=div)
        assert np.array_equal(f["depths"], r["depths"]) and np.array_equal(f["harm"], r["harm"])
        assert set(f["kinds"].tolist()) == ({model.PUSH} if div == 0 else {model.PULL}) and f["e"] == r["e"]
    push_only = model.traverse(ro, ci, sources, symmetric=False, csc=False)
    assert push_only["stats"]["pull_levels"] == 0 and push_only["stats"]["csc"] == 0 and push_only["bins_in"]["none"] == 0


def test_symmetric_graph_with_all_sources():
    n = 300
    ro, ci = cases.random_symmetric(n, 500, 9)
    r = model.traverse(ro, ci, None, symmetric=True)
    assert np.array_equal(r["far"], r["far_in"]) and np.array_equal(r["reach"], r["reach_in"])
    assert np.array_equal(r["depths"], r["depths"].T)
    assert r["stats"]["sources"] == n and r["stats"]["batches"] == 5


def test_closeness_and_harmonic_equal_networkx():
    import networkx as nx
    g = nx.gnm_random_graph(90, 200, seed=4)
    e = np.array(g.edges())
    ro, ci = cases.sym(90, e[:, 0], e[:, 1])
    r = model.traverse(ro, ci, None, symmetric=True)
    want_c = nx.closeness_centrality(g, wf_improved=True)
    want_h = nx.harmonic_centrality(g)
    close = model.closeness(r["reach"], r["far"], 90)
    assert max(abs(close[v] - want_c[v]) for v in range(90)) <= 1e-12
    assert max(abs(r["harm"][v] - want_h[v]) for v in range(90)) <= 1e-12


def test_both_kinds_occur_on_rmat(oracle):
    """symmetric R-MAT at the default divisor: the first level pushes, the dense middle pulls, the tail pushes again"""
    for scale in (10, 12):
        n, ro, ci, _ = oracle.rmat_csr(scale, 16, scale + 300, undir=True)
        deg = np.diff(ro)
        sources = np.random.default_rng(scale).choice(np.flatnonzero(deg > 0), 64, replace=False)
        r = model.traverse(ro, ci, sources, symmetric=True, depths=False)
        k = r["kinds"].tolist()
        assert k[0] == model.PUSH and k[-1] == model.PUSH and model.PULL in k, k
        m = len(ci)
        assert all((kind == model.PULL) == (e * 8 >= m) for kind, e in zip(k, r["e"]))


def test_closed_forms():
    n = 200
    r = model.traverse(*cases.path(n), [0, n - 1, 100], symmetric=True)
    assert np.array_equal(r["depths"][0], np.arange(n)) and np.array_equal(r["depths"][1], np.arange(n)[::-1])
    assert r["reach"].tolist() == [n - 1] * 3 and r["far"][0] == n * (n - 1) // 2 and r["ecc"].tolist() == [n - 1, n - 1, 100]
    h = np.float64(0.0)
    for d in range(1, n):
        h += np.float64(1.0) / np.float64(d)
    assert r["harm"][0] == h and r["stats"]["deepest"] == n
    k = 50
    r = model.traverse(*cases.star(k), [0, 1], symmetric=True)
    assert r["reach"].tolist() == [k, k] and r["far"].tolist() == [k, 1 + 2 * (k - 1)] and r["ecc"].tolist() == [1, 2]
    assert r["harm"].tolist() == [float(k), 1.0 + (k - 1) / 2.0]
    r = model.traverse(*cases.complete(17), None, symmetric=True)
    assert (r["reach"] == 16).all() and (r["far"] == 16).all() and (r["ecc"] == 1).all() and (r["harm"] == 16.0).all()
    assert (model.closeness(r["reach"], r["far"], 17) == 1.0).all()
    for nn in (1, 100):
        r = model.traverse(*cases.empty(nn), None, symmetric=True)
        assert not r["reach"].any() and not r["far"].any() and not r["harm"].any() and not r["reach_in"].any()
        assert (r["depths"] == np.where(np.eye(nn, dtype=bool), 0, -1)).all()
        assert r["stats"]["deepest"] == 1 and len(r["kinds"]) == (nn + 63) // 64
        assert (model.closeness(r["reach"], r["far"], nn) == 0.0).all()
    r = model.traverse(*cases.path(10), [], symmetric=True)
    assert r["stats"] == {"sources": 0, "batches": 0, "deepest": 0, "reach": 0, "push_levels": 0, "pull_levels": 0, "csc": 0, "depths": 1}
    assert r["depths"].shape == (0, 10) and not r["reach_in"].any()


def test_rows_per_body():
    ro, ci, root, hubs, sinks = cases.fans(cases.cuts(4, 10, 16))
    r = model.traverse(ro, ci, [root], symmetric=False, csc=True, short_max=4, wave_max=10, seg=16)
    out, inn = np.diff(ro), np.bincount(ci, minlength=len(ro) - 1)
    for side, ln in ((r["bins_out"], out), (r["bins_in"], inn)):
        assert side["none"] == int((ln == 0).sum()) and side["short"] == int(((ln >= 1) & (ln <= 4)).sum())
        assert side["wave"] == int(((ln > 4) & (ln <= 10)).sum()) and side["long"] == int((ln > 10).sum())
        assert side["segments"] == int(sum(-(-x // 16) for x in ln[ln > 10]))
    assert r["bins_out"]["long"] == 7 + 1 and r["bins_in"]["long"] == 7      # 11, 15 - 17, 31 - 33; and the root's row of 12
    assert (r["depths"][0][hubs] == 1).all() and (r["depths"][0][sinks] == 3).all()
