"""CPU suite for the connected components (mgx_cc_*, include/mgx/cc_fused.hpp, include/gunrock/cc/): the library exports them,
refuses NULL handles, its kernels keep their registers, and the numpy model the GPU tests compare against (tests/cc_model.py)
agrees with scipy and with a plain union-find."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cc_model as model
from tests import coloring_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_cc_create", "mgx_cc_free", "mgx_cc_run", "mgx_cc_enact", "mgx_cc_labels", "mgx_cc_labels_device"]
KERNELS = ["k_cc_init", "k_cc_neighbor", "k_cc_compress", "k_cc_sample", "k_cc_worklist", "k_cc_link", "k_cc_sizes", "k_cc_largest"]


def test_library_exports_cc(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "CcProblem")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h = C.c_void_p()
    assert lib.mgx_cc_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    st = (C.c_int64 * 5)()
    assert lib.mgx_cc_run(None, 1, 7, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_cc_enact(None, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_cc_labels(None, None) == mini_amd.MGX_E_INVALID
    p = C.c_void_p()
    assert lib.mgx_cc_labels_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_cc_free(None) == 0


def test_cc_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the CC kernels use no scratch and spill nothing"""
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
        assert found, (name, sorted(k for k in res if "cc" in k))
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


def _union_find(n, ro, ci):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for v in range(n):
        for e in range(ro[v], ro[v + 1]):
            a, b = find(v), find(int(ci[e]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(n)], dtype=np.int32)


def _random_graph(rng, n, m, symmetric):
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    return cm.csr(n, s, d, symmetric=symmetric)


@pytest.mark.parametrize("n,m,symmetric,seed", [(1, 0, True, 1), (50, 30, False, 2), (200, 150, True, 3), (500, 400, False, 4),
                                                (1000, 3000, False, 5), (2000, 1500, True, 6)])
def test_model_equals_union_find(n, m, symmetric, seed):
    ro, ci = _random_graph(np.random.default_rng(seed), n, m, symmetric)
    assert np.array_equal(model.labels(ro, ci), _union_find(n, ro, ci))


@pytest.mark.parametrize("n,m,symmetric,seed", [(300, 200, False, 11), (3000, 2500, False, 12), (3000, 2500, True, 13),
                                                (20000, 30000, False, 14), (20000, 12000, True, 15)])
def test_model_equals_scipy_weak_components(n, m, symmetric, seed):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    ro, ci = _random_graph(np.random.default_rng(seed), n, m, symmetric)
    a = sp.csr_matrix((np.ones(len(ci)), ci, ro), shape=(n, n))
    k, lab = csgraph.connected_components(a, directed=True, connection="weak")
    smallest = np.full(k, n, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    want = smallest[lab].astype(np.int32)
    got = model.labels(ro, ci)
    assert np.array_equal(got, want)
    st = model.stats(got)
    assert st["components"] == k
    sizes = np.bincount(lab)
    assert st["largest"] == sizes.max()
    assert st["largest_label"] == min(int(smallest[c]) for c in np.nonzero(sizes == sizes.max())[0])


def test_model_self_loops_duplicates_and_isolated():
    ro, ci = cm.csr(6, [0, 0, 0, 2, 5], [0, 1, 1, 2, 3], symmetric=False)
    assert model.labels(ro, ci).tolist() == [0, 0, 2, 3, 4, 3]
    assert model.stats(model.labels(ro, ci)) == {"components": 4, "largest": 2, "largest_label": 0}


def test_model_skip_stats_partition_refines_components():
    rng = np.random.default_rng(21)
    ro, ci = _random_graph(rng, 5000, 6000, True)
    lab = model.labels(ro, ci)
    for seed in (1, 2, model.SEED):
        sk = model.skip_stats(ro, ci, seed, symmetric=True)
        part = sk["partition"]
        assert (part <= np.arange(len(part))).all()
        assert np.array_equal(lab[part], lab)                   # every neighbour-round set lies inside one component
        assert part[sk["c"]] == sk["c"]
        assert 0 <= sk["skipped"] <= int((part == sk["c"]).sum())
    assert model.skip_stats(ro, ci, symmetric=False, has_csc=False)["skipped"] == 0


def test_model_samples_follow_the_colouring_salt():
    ids = model.sample_ids(1000, 77)
    assert len(ids) == model.SAMPLES
    for j in (0, 1, 500, 1023):
        assert ids[j] == int(cm.salt(77, j)) % 1000


def test_model_transpose():
    rng = np.random.default_rng(3)
    ro, ci = _random_graph(rng, 100, 300, False)
    co, ri = model.transpose(ro, ci)
    fwd = sorted((v, int(u)) for v in range(100) for u in ci[ro[v]:ro[v + 1]])
    bwd = sorted((int(ri[e]), u) for u in range(100) for e in range(co[u], co[u + 1]))
    assert fwd == bwd
