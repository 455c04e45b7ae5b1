"""CPU suite for the local sparsification (mgx_lspar_*, include/mgx/lspar_fused.hpp, include/gunrock/lspar/) and the segmented
sort (mgx_segmented_sort_i32, include/mgx/segsort.hpp): the library exports them, refuses NULL handles and bad parameters, their
kernels keep their registers, and the numpy model the GPU tests compare against (tests/lspar_model.py) holds the properties
DESIGN 3.7 states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import lspar_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_lspar_create", "mgx_lspar_free", "mgx_lspar_run", "mgx_lspar_enact", "mgx_lspar_result", "mgx_lspar_result_device",
         "mgx_lspar_minhashes", "mgx_lspar_graph", "mgx_segmented_sort_i32"]


def test_library_exports_lspar_and_segmented_sort(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "LsparProblem") and hasattr(mini_amd, "segmented_sort")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib, bad = mini_amd.lib, mini_amd.MGX_E_INVALID
    h = C.c_void_p()
    assert lib.mgx_lspar_create(None, C.byref(h)) == bad
    st = (C.c_int64 * 3)()
    assert lib.mgx_lspar_run(None, 1, 1, 0.5, st) == bad
    assert lib.mgx_lspar_enact(None, 1, 1, 0.5, st) == bad
    assert lib.mgx_lspar_result(None, None, None, None, None) == bad
    p = C.c_void_p()
    assert lib.mgx_lspar_result_device(None, C.byref(p), None, None, None) == bad
    assert lib.mgx_lspar_minhashes(None, None) == bad
    assert lib.mgx_lspar_graph(None, C.byref(p)) == bad
    assert lib.mgx_segmented_sort_i32(None, None, None, 0, None, 0, 0) == bad
    assert lib.mgx_lspar_free(None) == 0


def _resources():
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
    return res


def test_lspar_and_segsort_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the new kernels use no scratch and spill nothing"""
    res = _resources()
    lspar = [k for k in res if "k_lspar_" in k]
    segsort = [k for k in res if "k_segsort_" in k]
    assert len(lspar) >= 9, sorted(lspar)
    assert len(segsort) >= 10, sorted(segsort)
    for k in lspar + segsort:
        assert res[k].get("scratch", 0) == 0, (k, res[k])
        assert res[k].get("vspill", 0) == 0, (k, res[k])
        assert res[k].get("sspill", 0) == 0, (k, res[k])


def test_keep_count_is_exact_on_perfect_powers():
    r = np.arange(1, 3000, dtype=np.int64)
    assert np.array_equal(model.keep_count(r * r, 0.5), r)
    assert np.array_equal(model.keep_count(r[:170] ** 4, 0.25), r[:170])
    assert int(model.keep_count([10 ** 6], 0.5)[0]) == 1000
    assert int(model.keep_count([4], 0.5)[0]) == 2
    # between the squares: floor(sqrt(d))
    d = np.arange(1, 200000, dtype=np.int64)
    assert np.array_equal(model.keep_count(d, 0.5), np.floor(np.sqrt(d)).astype(np.int64))
    assert list(model.keep_count([0, 1, 2, 7], 0.0)) == [0, 1, 1, 1]
    assert list(model.keep_count([0, 1, 2, 7], 1.0)) == [0, 1, 2, 7]
    assert list(model.keep_count([5, 9], 2.0)) == [5, 9]


def _random_graph(rng, n, m, symmetric=True):
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)            # self-loops and duplicates kept
    return model.csr(n, s, d, symmetric=symmetric)


def _subsequence(ro, ci, oro, oci, oeid):
    for v in range(len(ro) - 1):
        e = oeid[oro[v]:oro[v + 1]]
        if len(e) and not ((np.diff(e) > 0).all() and e[0] >= ro[v] and e[-1] < ro[v + 1]):
            return False
    return np.array_equal(oci, ci[oeid])


@pytest.mark.parametrize("k,e", [(1, 0.5), (4, 0.25), (8, 0.5), (32, 0.75), (2, 1.0), (3, 0.0)])
def test_model_properties(k, e):
    rng = np.random.default_rng(k * 100 + int(e * 10))
    ro, ci = _random_graph(rng, 400, 3000)
    oro, oci, oeid, osim, mh = model.sparsify(ro, ci, seed=7, k=k, e=e)
    d = np.diff(ro.astype(np.int64))
    t = model.keep_count(d, e)
    assert np.array_equal(np.diff(oro.astype(np.int64)), t)
    assert len(oci) == len(oeid) == len(osim) == int(t.sum()) == int(oro[-1])
    assert _subsequence(ro, ci, oro, oci, oeid)
    if e == 1.0:
        assert np.array_equal(oeid, np.arange(len(ci)))
    if e == 0.0:
        assert np.array_equal(np.diff(oro), (d > 0).astype(np.int64))
    # no dropped entry of a row has a sim above a kept one
    rows = np.repeat(np.arange(len(d)), d)
    sim_all = (mh[rows] == mh[ci]).sum(axis=1)
    kept = np.zeros(len(ci), bool)
    kept[oeid] = True
    for v in range(len(d)):
        a, b = ro[v], ro[v + 1]
        if kept[a:b].all() or not kept[a:b].any():
            continue
        assert sim_all[a:b][~kept[a:b]].max() <= sim_all[a:b][kept[a:b]].min()
    assert (osim >= 0).all() and (osim <= k).all()
    # self-loops have sim k
    loops = ci == rows
    assert (sim_all[loops] == k).all()


@pytest.mark.parametrize("k,e,symmetric", [(1, 0.5, True), (4, 0.5, True), (3, 0.3, False), (8, 0.0, False), (2, 1.0, True)])
def test_model_matches_brute_force(k, e, symmetric):
    rng = np.random.default_rng(k + 17)
    for n, m in ((1, 0), (5, 3), (40, 150), (90, 700)):
        ro, ci = _random_graph(rng, n, m, symmetric)
        want = model.brute_force(ro, ci, seed=31, k=k, e=e)
        got = model.sparsify(ro, ci, seed=31, k=k, e=e)
        for a, b in zip(got[:4], want[:4]):
            assert list(a) == list(b)
        assert np.array_equal(got[4], np.array(want[4], dtype=np.uint32).reshape(n, k))


def test_model_empty_rows_and_parallel_entries():
    ro = np.array([0, 0, 3, 3, 5], np.int32)
    ci = np.array([3, 3, 1, 1, 0], np.int32)                         # row 1: two parallel entries and a self-loop
    oro, oci, oeid, osim, mh = model.sparsify(ro, ci, k=4, e=1.0)
    assert (mh[0] == 0xFFFFFFFF).all() and (mh[2] == 0xFFFFFFFF).all()
    assert osim[0] == osim[1] and osim[2] == 4
