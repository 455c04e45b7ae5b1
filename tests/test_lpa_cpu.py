"""CPU suite for the label propagation and modularity (mgx_lpa_*, mgx_modularity, include/mgx/lpa_fused.hpp,
include/gunrock/lpa/): the library exports them, refuses NULL handles, its kernels keep their registers, its switches are in the
table, and the model the GPU tests compare against (tests/lpa_model.py) has the properties and closed forms of the definition."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import lpa_cases as cases
from tests import lpa_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_lpa_create", "mgx_lpa_free", "mgx_lpa_run", "mgx_lpa_enact", "mgx_lpa_labels", "mgx_lpa_labels_device", "mgx_lpa_trace",
         "mgx_lpa_step_kinds", "mgx_lpa_bins", "mgx_lpa_set_timing", "mgx_lpa_phase_ms", "mgx_modularity"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_lpa_step",), ("k_mod_votes",), ("k_mod_squares",), ("3lpa", "gather_out_functor_t"), ("3lpa", "gather_in_functor_t"),
           ("3lpa", "want_functor_t"), ("3lpa", "apply_functor_t")]
SWITCHES = {"MGX_LPA_SHORT_MAX", "MGX_LPA_WAVE_MAX", "MGX_LPA_TABLE", "MGX_LPA_LIST_DIV"}


def test_library_exports_lpa(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "LpaProblem") and hasattr(mini_amd, "modularity")
    assert mini_amd.LpaProblem.KEYS == ("communities", "largest", "largest_label", "iterations", "converged", "unstable", "evaluated",
                                        "overflowed", "host_waits", "launches")
    assert mini_amd.LpaProblem.KEYS[:6] == model.STAT_KEYS
    assert (mini_amd.LpaProblem.SYNC, mini_amd.LpaProblem.LAZY) == (model.SYNC, model.LAZY) == (mini_amd.MGX_LPA_SYNC, mini_amd.MGX_LPA_LAZY)
    assert mini_amd.LpaProblem.SEED == model.SEED
    for member in ("run", "enact", "labels", "labels_device_ptr", "trace", "step_kinds", "bins", "set_timing", "phase_ms", "modularity",
                   "close"):
        assert hasattr(mini_amd.LpaProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    n = C.c_int64()
    out = (C.c_uint64 * 3)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_lpa_create(None, C.byref(h)) == bad
    assert lib.mgx_lpa_run(None, 1, 1, 1, 10, st) == bad
    assert lib.mgx_lpa_enact(None, 1, 1, 1, 10, st) == bad
    assert lib.mgx_lpa_labels(None, None) == bad
    assert lib.mgx_lpa_labels_device(None, C.byref(p)) == bad
    assert lib.mgx_lpa_trace(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_lpa_step_kinds(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_lpa_bins(None, None) == bad
    assert lib.mgx_lpa_set_timing(None, 1) == bad
    assert lib.mgx_lpa_phase_ms(None, None) == bad
    assert lib.mgx_modularity(None, None, 1, out) == bad
    assert lib.mgx_lpa_free(None) == 0


def test_lpa_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names


def test_lpa_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the step kernel, the modularity kernels and the operator path's
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


def _graphs(n, symmetric, seed):
    if n == 1:
        return cases.empty(1)
    return cases.random_symmetric(n, 2 * n, seed) if symmetric else cases.random_digraph(n, 3 * n, seed)


@pytest.mark.parametrize("mode", [model.SYNC, model.LAZY])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [1, 50, 1000, 20000])
def test_properties_on_random_graphs(n, symmetric, mode):
    ro, ci = _graphs(n, symmetric, 7 * n + mode)
    r = model.propagate(ro, ci, symmetric, mode, check_active=True)             # (asserts want == lab outside A_t on the way)
    lab, st = r["labels"], r["stats"]
    assert lab.dtype == np.int32 and len(lab) == n and (lab >= 0).all() and (lab < n).all()
    rcv, _ = model.votes(ro, ci, symmetric)
    voteless = np.ones(n, dtype=bool)
    voteless[rcv] = False
    assert (lab[voteless] == np.flatnonzero(voteless)).all()
    assert (st["communities"], st["largest"], st["largest_label"]) == model.label_stats(lab)
    assert len(r["trace"]) == st["iterations"] + 1 and r["trace"][-1] == (st["unstable"], 0)
    if st["converged"]:
        assert st["unstable"] == 0 and model.is_equilibrium(ro, ci, symmetric, lab)
    else:
        assert st["iterations"] == 100 and st["unstable"] > 0
    only = model.propagate(ro, ci, symmetric, mode, active_only=True)           # evaluating A_t alone: the same run
    assert np.array_equal(only["labels"], lab) and only["stats"] == st and only["trace"] == r["trace"]
    assert all(0 <= a <= n for a in r["active"]) and r["active"][0] == int((~voteless).sum())


def test_lazy_converges_on_random_graphs():
    for symmetric in (True, False):
        r = model.propagate(*_graphs(20000, symmetric, 3), symmetric, model.LAZY)
        assert r["stats"]["converged"] == 1


@pytest.mark.parametrize("k", [3, 4, 17, 100])
def test_clique_converges_synchronously(k):
    ro, ci = cases.sym(k, *cases.clique(k))
    r = model.propagate(ro, ci, True, model.SYNC)
    assert not r["labels"].any()
    assert r["stats"] == {"communities": 1, "largest": k, "largest_label": 0, "iterations": 2, "converged": 1, "unstable": 0}


@pytest.mark.parametrize("ro_ci,n", [(cases.sym(2, [0], [1]), 2), (cases.star(50), 51)])
def test_bipartite_oscillates_synchronously_and_converges_lazily(ro_ci, n):
    ro, ci = ro_ci
    r = model.propagate(ro, ci, True, model.SYNC, max_iter=7)
    assert r["stats"]["converged"] == 0 and r["stats"]["iterations"] == 7 and r["stats"]["unstable"] == n
    assert all(u == n for u, _ in r["trace"])
    r = model.propagate(ro, ci, True, model.LAZY)
    assert r["stats"]["converged"] == 1 and r["stats"]["communities"] == 1 and r["stats"]["largest"] == n


def test_lazy_converges_on_path_and_grid():
    for ro, ci in (cases.path(5000), cases.grid(64, 64)):
        r = model.propagate(ro, ci, True, model.LAZY, check_active=True)
        assert r["stats"]["converged"] == 1 and model.is_equilibrium(ro, ci, True, r["labels"])
        assert sum(r["evaluated"]) < len(ro) * len(r["evaluated"]) // 2        # the active set pays
        s = model.propagate(ro, ci, True, model.SYNC, max_iter=30)
        assert s["stats"]["converged"] == 0


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(n):
    for ro, ci in (cases.empty(n), cases.directed(n, np.arange(n), np.arange(n))):        # (and self-loops only)
        for symmetric in (True, False):
            r = model.propagate(ro, ci, symmetric, model.SYNC)
            assert np.array_equal(r["labels"], np.arange(n))
            assert r["stats"] == {"communities": n, "largest": 1, "largest_label": 0, "iterations": 0, "converged": 1, "unstable": 0}
            assert r["active"] == [0]


def test_multiplicity_decides():
    r = model.propagate(*cases.multiplicity(), True, model.SYNC, max_iter=1)
    assert r["labels"][0] == 2                                           # three votes for b = 2 against one for a = 1
    r = model.propagate(*cases.multiplicity(dedup=True), True, model.SYNC, max_iter=1)
    assert r["labels"][0] == 1                                           # one each: the smaller
    ro, ci = cases.random_symmetric(500, 1500, 4)
    plain = model.propagate(ro, ci, True, model.LAZY)
    thrice = model.propagate(*cases.tripled_with_loops(ro, ci), True, model.LAZY)
    assert np.array_equal(plain["labels"], thrice["labels"]) and plain["trace"] == thrice["trace"]


# the seeds on which the model alone returns exactly the planted blocks: found by running it, asserted here so that the GPU test
# cannot hide behind a seed on which label propagation itself merges or splits blocks
PLANTED_SEEDS = {model.SYNC: (0, 1, 2), model.LAZY: (0, 3, 4)}          # (LAZY splits a block on seeds 1, 2 and 5)


@pytest.mark.parametrize("mode", [model.SYNC, model.LAZY])
def test_planted_blocks(mode):
    for seed in PLANTED_SEEDS[mode]:
        ro, ci, block = cases.planted_blocks(seed)
        r = model.propagate(ro, ci, True, mode)
        assert r["stats"]["converged"] == 1 and r["stats"]["communities"] == 40 and r["stats"]["largest"] == 50, (seed, r["stats"])
        assert cases.same_partition(r["labels"], block), seed


def test_two_seeds_two_equilibria():
    ro, ci = cases.random_symmetric(3000, 9000, 5)
    a = model.propagate(ro, ci, True, model.LAZY, seed=1)
    b = model.propagate(ro, ci, True, model.LAZY, seed=2)
    assert a["stats"]["converged"] and b["stats"]["converged"] and not np.array_equal(a["labels"], b["labels"])
    assert model.is_equilibrium(ro, ci, True, a["labels"]) and model.is_equilibrium(ro, ci, True, b["labels"])


def test_overflow_and_kinds_are_predicted():
    r = model.propagate(*cases.star(5000), True, model.LAZY)
    assert r["overflowed"] >= 1 and r["kinds"][:3] == [model.SETUP, model.EVAL_DENSE, model.LONG] and r["kinds"][-1] == model.IDLE
    r = model.propagate(*cases.star(5000), True, model.LAZY, table=8192)
    assert r["overflowed"] == 0
    r = model.propagate(*cases.path(5000), True, model.LAZY)
    assert model.LONG not in r["kinds"] and model.EVAL_LIST in r["kinds"] and model.EVAL_DENSE in r["kinds"]
    assert model.propagate(*cases.path(5000), True, model.LAZY, list_div=0)["kinds"].count(model.EVAL_LIST) == 0
    assert model.propagate(*cases.path(5000), True, model.LAZY, list_div=1)["kinds"].count(model.EVAL_DENSE) == 0


def test_modularity_equals_networkx():
    import networkx as nx
    from networkx.algorithms.community import modularity as nx_modularity
    rng = np.random.default_rng(11)
    for n, m in ((60, 150), (500, 2000)):
        g = nx.gnm_random_graph(n, m, seed=n)
        e = np.array(g.edges())
        ro, ci = cases.sym(n, e[:, 0], e[:, 1])
        for labels in (rng.integers(0, 7, n), model.propagate(ro, ci, True, model.LAZY)["labels"]):
            q, s_in, s_sq, w = model.modularity(ro, ci, labels, True)
            groups = [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]
            assert w == 2 * m and abs(float(q) - nx_modularity(g, groups)) <= 1e-12
            q2, s_in2, s_sq2, w2 = model.modularity(ro, ci, labels, False)     # both ends of every entry: every count doubled
            assert (s_in2, s_sq2, w2) == (2 * s_in, 4 * s_sq, 2 * w) and q2 == q


def test_modularity_closed_forms():
    ro, ci = cases.random_symmetric(400, 1200, 2)
    n = 400
    q, s_in, s_sq, w = model.modularity(ro, ci, np.zeros(n, dtype=np.int64), True)
    assert q == 0 and s_in == w and s_sq == w * w                        # one community
    q, s_in, s_sq, w = model.modularity(ro, ci, np.arange(n), True)
    assert s_in == 0 and q < 0                                           # singletons
    labels = np.random.default_rng(3).integers(0, 9, n)
    renamed = (n - 1 - labels * 3) % n                                   # an injective renaming of 0 .. 8
    assert model.modularity(ro, ci, labels, True) == model.modularity(ro, ci, renamed, True)
    assert model.modularity(*cases.empty(5), np.arange(5), True) == (Fraction(0), 0, 0, 0)
