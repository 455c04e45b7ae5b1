"""CPU suite for the fused k-core (mgx_kcore_run, include/mgx/kcore_fused.hpp): the library exports it, refuses NULL arguments, its
kernels keep their registers, and the numpy worklist model the GPU tests compare against (tests/kcore_model.py) computes what
the oracle's restatement of kcore_enactor_t::enact computes -- stranded vertices and the k <= n cap included."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import kcore_model as model
from tests.golden_inputs import case_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [c for c in json.load(open(os.path.join(GOLD, "reference_goldens.json")))["cases"] if "kcore_largest" in c]


def test_library_exports_kcore_run(built):
    import mini_amd
    assert hasattr(mini_amd.lib, "mgx_kcore_run")
    assert hasattr(mini_amd.KcoreProblem, "run")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    largest = C.c_int()
    st = (C.c_int64 * 6)()
    assert lib.mgx_kcore_run(None, C.byref(largest), st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_kcore_run(None, None, None) == mini_amd.MGX_E_INVALID
    # (a NULL largest_k_core on a live handle is refused by the same test before any device work: checked on the GPU suite)


def test_kcore_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the k-core kernels use no scratch and spill nothing"""
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
    found = [k for k in res if "k_kcore_" in k]
    assert found, sorted(k for k in res if "kcore" in k)
    for k in found:
        assert res[k].get("scratch", 0) == 0, (k, res[k])
        assert res[k].get("vspill", 0) == 0, (k, res[k])
        assert res[k].get("sspill", 0) == 0, (k, res[k])


def _check(oracle, ro, ci, symmetric=False):
    """the model against the enactor's restatement; on symmetric graphs also against the CPU validator"""
    cores, largest, deg, st = model.decompose(ro, ci)
    ecores, elargest, est = oracle.kcore_enact(ro, ci)
    assert np.array_equal(cores, ecores)
    assert largest == elargest
    assert model.check_against_enactor(st, est), (st, est.tolist())
    assert st["levels"] <= int(est[0])
    assert not ((deg > 0) & (cores > 0)).any()               # whoever left is at 0 or below
    if symmetric:
        want, wlargest = oracle.kcore_cpu(ro, ci)
        assert np.array_equal(cores, want)
        assert wlargest == largest or (len(ci) == 0 and wlargest == 0 and largest == -1)
    return cores, largest, deg, st


def test_model_path3_strands_the_middle(oracle):
    cores, largest, deg, st = _check(oracle, *model.path3(), symmetric=True)
    assert cores.tolist() == [1, 0, 1] and st["stranded"] == 1 and st["removed"] == 2
    assert deg.tolist() == [0, 0, 0] and largest == 1


def test_model_graph_without_entries(oracle):
    cores, largest, deg, st = _check(oracle, *model.no_entries(), symmetric=True)
    assert largest == -1 and not cores.any() and st == dict.fromkeys(model.STAT_NAMES, 0)


def test_model_cap_at_n(oracle):
    ro, ci = model.capped_multigraph()
    assert np.diff(ro).max() >= 6
    cores, largest, deg, st = _check(oracle, ro, ci)
    assert largest == -1 and not cores.any() and np.array_equal(deg, np.diff(ro))
    cores, largest, deg, st = _check(oracle, *model.tripled_clique())
    assert largest == -1 and not cores.any()


def test_model_star_forest(oracle):
    ro, ci = model.star_forest()
    cores, largest, deg, st = _check(oracle, ro, ci, symmetric=True)
    # a hub with two or more leaves falls from its degree to 0 in the one pass its leaves leave in; a hub with one leaf leaves
    # with it (8 of the 50 stars)
    assert st["stranded"] == 42 and st["levels"] == 1 and st["passes"] == 1 and largest == 1


@pytest.mark.parametrize("loop", [False, True])
def test_model_single_vertex(oracle, loop):
    _check(oracle, *model.single(loop), symmetric=True)


def test_model_grid(oracle):
    cores, largest, deg, st = _check(oracle, *model.grid(64, 64), symmetric=True)
    assert st["passes"] >= 63


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_golden_fixtures(oracle, case, tmp_path):
    n, ro, ci, w, _ = oracle.load_mtx(case_path(case, oracle, tmp_path, GOLD), undir=True)
    _check(oracle, ro, ci, symmetric=True)


@pytest.mark.parametrize("seed", range(12))
def test_model_directed_ragged_multigraphs(oracle, seed):
    n = [5, 8, 13, 30, 60, 100, 200, 300, 400, 500, 600, 37][seed]
    _check(oracle, *model.ragged_directed(seed, n))


@pytest.mark.parametrize("seed", range(6))
def test_model_sparse_symmetric_graphs(oracle, seed):
    cores, largest, deg, st = _check(oracle, *model.sparse_symmetric(100 + seed), symmetric=True)
    assert st["stranded"] > 0


@pytest.mark.parametrize("scale,ef,seed", [(10, 16, 10), (12, 8, 12), (14, 4, 14), (16, 16, 16)])
def test_model_rmat(oracle, scale, ef, seed):
    n, ro, ci, w = oracle.rmat_csr(scale, ef, seed)
    _check(oracle, ro, ci, symmetric=True)
