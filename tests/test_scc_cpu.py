"""CPU suite for the strongly connected components (mgx_scc_*, include/mgx/scc_fused.hpp, include/gunrock/scc/): the library
exports them, refuses NULL handles, its kernels keep their registers, its switches are in the table, and the model the GPU tests
compare against (tests/scc_model.py) agrees with scipy, networkx and closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import scc_cases as cases
from tests import scc_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_scc_create", "mgx_scc_free", "mgx_scc_run", "mgx_scc_enact", "mgx_scc_labels", "mgx_scc_labels_device",
         "mgx_scc_step_kinds", "mgx_scc_set_timing", "mgx_scc_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_scc_step",), ("3scc", "trim_collect_functor_t"), ("3scc", "trim_seal_functor_t"), ("3scc", "pivot_max_functor_t"),
           ("3scc", "pivot_pick_functor_t"), ("3scc", "init_functor_t"), ("3scc", "forward_functor_t"), ("3scc", "root_functor_t"),
           ("3scc", "backward_functor_t"), ("3scc", "pivot_min_functor_t"), ("3scc", "seal_functor_t")]


def test_library_exports_scc(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "SccProblem")
    assert mini_amd.SccProblem.KEYS == ("components", "largest", "largest_label", "trimmed", "pivot_size", "rounds", "host_waits",
                                        "launches")
    assert mini_amd.SccProblem.KEYS[:6] == model.STAT_KEYS
    for member in ("run", "enact", "labels", "labels_device_ptr", "step_kinds", "set_timing", "phase_ms", "close"):
        assert hasattr(mini_amd.SccProblem, member), member


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    n = C.c_int64()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_scc_create(None, C.byref(h)) == bad
    assert lib.mgx_scc_run(None, st) == bad
    assert lib.mgx_scc_enact(None, st) == bad
    assert lib.mgx_scc_labels(None, None) == bad
    assert lib.mgx_scc_labels_device(None, C.byref(p)) == bad
    assert lib.mgx_scc_step_kinds(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_scc_set_timing(None, 1) == bad
    assert lib.mgx_scc_phase_ms(None, None) == bad
    assert lib.mgx_scc_free(None) == 0


def test_scc_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert {"MGX_SCC_LONG_MIN", "MGX_SCC_SEG"} <= names


def test_scc_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the step kernel and the operator path's instantiations use no scratch and
    spill nothing"""
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


def _consistent(ro, ci, r):
    """what every result of the model satisfies, whatever the graph"""
    n = len(ro) - 1
    lab, st = r["labels"], r["stats"]
    assert lab.dtype == np.int32 and len(lab) == n
    assert (lab[lab] == lab).all() and (lab <= np.arange(n)).all()                 # a label names its own component's smallest id
    assert (st["components"], st["largest"], st["largest_label"]) == model.label_stats(lab)
    alive = [a for _, a in r["phases"]]
    assert len(alive) == 1 + (1 if st["pivot_size"] else 0) + st["rounds"] and not alive[-1].any()
    assert all((later <= earlier).all() for earlier, later in zip(alive, alive[1:]))
    assert st["trimmed"] <= n and (st["pivot_size"] > 0) == bool(alive[0].any())


@pytest.mark.parametrize("n,m", [(1, 0), (50, 60), (300, 400), (1000, 1500), (1000, 3000), (5000, 6000), (20000, 30000)])
def test_model_equals_scipy_on_random_digraphs(n, m):
    ro, ci = cases.random_digraph(n, m, n + m)
    r = model.decompose(ro, ci)
    assert np.array_equal(r["labels"], model.scipy_labels(ro, ci))
    _consistent(ro, ci, r)
    # every entry three times and a self-loop on every fifth vertex: the same labels, the same run
    src = np.repeat(np.arange(n), np.diff(ro))
    loops = np.arange(0, n, 5)
    ro3, ci3 = cases.directed(n, np.concatenate([src, src, src, loops]), np.concatenate([ci, ci, ci, loops]))
    r3 = model.decompose(ro3, ci3)
    assert np.array_equal(r3["labels"], r["labels"]) and r3["stats"] == r["stats"]


def test_model_equals_networkx():
    import networkx as nx
    n = 5000
    ro, ci = cases.random_digraph(n, 6000, 11000)
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(np.repeat(np.arange(n), np.diff(ro)).tolist(), ci.tolist()))
    want = np.empty(n, dtype=np.int32)
    for comp in nx.strongly_connected_components(g):
        want[list(comp)] = min(comp)
    r = model.decompose(ro, ci)
    assert np.array_equal(r["labels"], want)
    assert r["stats"]["rounds"] >= 1 and r["stats"]["pivot_size"] > 1


def _stats(ro, ci):
    r = model.decompose(ro, ci)
    _consistent(ro, ci, r)
    return r, r["stats"]


def test_closed_forms():
    for n in (1, 2, 3, 100):                                             # a path: n components, all trimmed
        r, st = _stats(*cases.path(n))
        assert np.array_equal(r["labels"], np.arange(n))
        assert st == {"components": n, "largest": 1, "largest_label": 0, "trimmed": n, "pivot_size": 0, "rounds": 0}
    for n in (2, 3, 100):                                                # a ring: one component, the pivot's
        r, st = _stats(*cases.ring(n))
        assert not r["labels"].any()
        assert st == {"components": 1, "largest": n, "largest_label": 0, "trimmed": 0, "pivot_size": n, "rounds": 0}
    v = np.arange(50)                                                    # self-loops only
    r, st = _stats(*cases.directed(50, v, v))
    assert np.array_equal(r["labels"], v) and st["components"] == 50 and st["trimmed"] == 50 and st["pivot_size"] == 0
    r, st = _stats(*cases.star(100, out=True, back=True))                # the bidirected star: one component
    assert st["components"] == 1 and st["pivot_size"] == 101 and st["trimmed"] == 0
    r, st = _stats(*cases.star(100, out=True, back=False))               # the out-star: all trimmed
    assert st["components"] == 101 and st["trimmed"] == 101


@pytest.mark.parametrize("k", [2, 5, 40])
def test_chains_of_two_cycles(k):
    """the known weakness: ascending, colour 0 floods everything and a round finds one cycle; descending, one round finds all"""
    want = 2 * (np.arange(2 * k) // 2)
    r, st = _stats(*cases.cycle_chain(k, ascending=True))
    assert np.array_equal(r["labels"], want) and st["pivot_size"] == 2 and st["rounds"] == k - 1 and st["trimmed"] == 0
    r, st = _stats(*cases.cycle_chain(k, ascending=False))
    assert np.array_equal(r["labels"], want) and st["pivot_size"] == 2 and st["rounds"] == 1 and st["trimmed"] == 0


@pytest.mark.parametrize("nc,maxsz,cross,chords", [(300, 64, 3000, 0), (300, 64, 3000, 4), (2000, 8, 20000, 0), (2000, 8, 20000, 2)])
def test_planted_returns_its_partition(nc, maxsz, cross, chords):
    ro, ci, labels = cases.planted(nc, maxsz, cross, nc + chords, chords)
    r, st = _stats(ro, ci)
    assert np.array_equal(r["labels"], labels) and np.array_equal(labels, model.scipy_labels(ro, ci))
    assert st["components"] == nc and st["rounds"] > 1


@pytest.mark.parametrize("k", [1, 127, 129])
def test_fan_and_layered_trim(k):
    r, st = _stats(*cases.fan(k))
    assert st["pivot_size"] == 2 and st["rounds"] == 1 and st["components"] == k + 1 and st["trimmed"] == 0
    assert r["labels"][1] == 0 and np.array_equal(r["labels"][2:], 2 + 2 * (np.arange(2 * k) // 2))
    r, st = _stats(*cases.layered_trim(k))
    assert st["trimmed"] == k + 1 and st["pivot_size"] == 2 and st["rounds"] == 0 and st["components"] == k + 2
