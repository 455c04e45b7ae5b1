"""CPU suite for the Louvain community detection (mgx_louvain_*, include/mgx/louvain_fused.hpp, include/mgx/louvain_aggregate.hpp):
the library exports it, refuses NULL handles, its kernels keep their registers, its switches are in the table, and the model the
GPU tests compare against (tests/louvain_model.py) has the properties and closed forms of the definition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import louvain_cases as cases
from tests import louvain_model as model
from tests import lpa_cases
from tests import lpa_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_louvain_create", "mgx_louvain_free", "mgx_louvain_run", "mgx_louvain_enact", "mgx_louvain_labels",
         "mgx_louvain_labels_device", "mgx_louvain_levels", "mgx_louvain_trace", "mgx_louvain_step_kinds", "mgx_louvain_bins",
         "mgx_louvain_set_timing", "mgx_louvain_phase_ms", "mgx_device_allocations"]
KERNELS = [("7louvain", "gather_out_functor_t"), ("7louvain", "gather_in_functor_t"), ("7louvain", "best_functor_t"),
           ("7louvain", "apply_functor_t"), "k_louvain_step", "k_lv_flag", "k_lv_map", "k_lv_compose", "k_lv_fill", "k_lv_starts", "k_lv_compact", "k_lv_rows"]
SWITCHES = {"MGX_LOUVAIN_SHORT_MAX", "MGX_LOUVAIN_WAVE_MAX", "MGX_LOUVAIN_SEG"}


def test_library_exports_louvain(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    lp = mini_amd.LouvainProblem
    assert lp.KEYS[:7] == model.STAT_KEYS and lp.SEED == model.SEED == 0x9E3779B9
    assert {v: k for k, v in lp.STEP_KINDS.items()} == {"setup": model.SETUP, "evaluate": model.EVAL, "long_fill": model.LONG_FILL,
                                                        "long_scan": model.LONG_SCAN, "apply": model.APPLY, "qnum": model.QNUM,
                                                        "done": model.DONE}
    for member in ("run", "enact", "labels", "labels_device_ptr", "levels", "dendrogram", "modularity", "trace", "step_kinds", "bins",
                   "set_timing", "phase_ms", "close"):
        assert hasattr(lp, member), member
    assert mini_amd.lib.mgx_device_allocations() >= 0


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, p = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    n = C.c_int64()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_louvain_create(None, C.byref(h)) == bad
    assert lib.mgx_louvain_run(None, 1, 1, 10, 10, 0.0, st) == bad
    assert lib.mgx_louvain_enact(None, 1, 1, 10, 10, 0.0, st) == bad
    assert lib.mgx_louvain_labels(None, -1, None) == bad
    assert lib.mgx_louvain_labels_device(None, -1, C.byref(p)) == bad
    assert lib.mgx_louvain_levels(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_louvain_trace(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_louvain_step_kinds(None, None, 0, C.byref(n)) == bad
    assert lib.mgx_louvain_bins(None, None) == bad
    assert lib.mgx_louvain_set_timing(None, 1) == bad
    assert lib.mgx_louvain_phase_ms(None, None) == bad
    assert lib.mgx_louvain_free(None) == 0


def test_louvain_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names


def test_louvain_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the step kernel and the contraction's kernels use no scratch and spill
    nothing"""
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
        parts = (name,) if isinstance(name, str) else name       # (parts of a mangled name: a kernel matches when it holds them all)
        found = [k for k in res if all(x in k for x in parts)]
        assert found, name
        for k in found:
            assert res[k] == {"scratch": 0, "vspill": 0, "sspill": 0}, (k, res[k])


def _edges(ro, ci, symmetric):
    n, rcv, snd, wt, lens = model.level0(ro, ci, symmetric)
    return n, rcv, snd, wt


def _replay(ro, ci, symmetric, r):
    """walk the levels of a result again: the per-level labels, their graphs and W"""
    n, rcv, snd, wt = _edges(ro, ci, symmetric)
    out = []
    for dense in r["maps"]:
        out.append((n, rcv, snd, wt, dense.astype(np.int64)))
        rcv, snd, wt = model.aggregate(rcv, snd, wt, dense.astype(np.int64))
        n = int(dense.max()) + 1
    return out, (n, rcv, snd, wt)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [1, 50, 1000, 5000])
def test_properties_on_random_graphs(n, symmetric):
    ro, ci = lpa_cases.empty(1) if n == 1 else (lpa_cases.random_symmetric(n, 2 * n, 7 * n) if symmetric else
                                               lpa_cases.random_digraph(n, 3 * n, 7 * n))
    r = model.louvain(ro, ci, symmetric)
    lab, st = r["labels"], r["stats"]
    assert lab.dtype == np.int32 and len(lab) == n
    assert np.array_equal(np.unique(lab), np.arange(st["communities"]))                       # dense
    assert st["levels"] == len(r["maps"]) and len(r["levels"]) in (st["levels"], st["levels"] + 1)
    # Qnum is strictly increasing over the accepted iterations, run-wide (the levels follow each other at the same Qnum)
    qs = [q for moved, ok, q in r["trace"] if ok]
    assert all(a < b for a, b in zip(qs, qs[1:]))
    assert sum(lv[2] for lv in r["levels"]) == len(r["trace"]) and sum(lv[3] for lv in r["levels"]) == len(qs)
    # the labels of every level are dense, W is equal on all levels, the composition of the maps is the result
    steps, last = _replay(ro, ci, symmetric, r)
    comp = np.arange(n, dtype=np.int64)
    for (n_l, rcv, snd, wt, dense), lv in zip(steps, r["levels"]):
        assert len(dense) == n_l == lv[0] and np.array_equal(np.unique(dense), np.arange(lv[4]))
        assert int(wt.sum()) == st["w"]
        comp = dense[comp]
    assert np.array_equal(comp, lab) and int(last[3].sum()) == st["w"]
    # Qnum / W^2 of the final labels is the label propagation model's modularity of them
    q, s_in, s_sq, w = lpa_model.modularity(ro, ci, lab, symmetric)
    assert (s_in, s_sq, w) == (st["s_in"], st["s_sq"], st["w"])
    assert abs(model.modularity(r) - float(q)) <= 1e-12
    if r["levels"]:
        assert r["levels"][-1][5] == st["s_in"] * st["w"] - st["s_sq"]


@pytest.mark.parametrize("symmetric", [True, False])
def test_level_end_is_a_fixed_point_for_both_parities(symmetric):
    ro, ci = lpa_cases.random_symmetric(800, 2400, 3) if symmetric else lpa_cases.random_digraph(800, 2400, 3)
    r = model.louvain(ro, ci, symmetric)
    steps, last = _replay(ro, ci, symmetric, r)
    steps.append(last + (np.arange(last[0], dtype=np.int64),))                                # the level that accepted nothing
    assert all(r["ended"]) and len(steps) == len(r["levels"])
    for n_l, rcv, snd, wt, dense in steps:
        k = model.degrees(n_l, rcv, wt)
        w = int(k.sum())
        # the level's own labels, not yet renumbered, cut the vertices the same way: the rule only compares keys of labels, so it
        # is replayed on the run itself
        lab, trace, accepted, q, ended = model.run_level(n_l, rcv, snd, wt, model.SEED, 100, 0)
        assert lpa_cases.same_partition(lab, dense)
        for t in (0, 1):
            new, moved = model.iterate(n_l, rcv, snd, wt, k, w, lab, t, model.SEED)
            assert moved == 0 or model.qnum(n_l, rcv, snd, wt, k, new)[0] <= q


def test_k2_is_one_community():
    r = model.louvain(*lpa_cases.sym(2, [0], [1]))
    assert r["labels"].tolist() == [0, 0] and r["stats"]["communities"] == 1 and r["stats"]["levels"] == 1
    assert (r["stats"]["s_in"], r["stats"]["s_sq"], r["stats"]["w"]) == (2, 4, 2) and model.modularity(r) == 0.0


def test_star_is_one_community_and_its_first_iteration_is_rejected():
    r = model.louvain(*lpa_cases.star(50))
    assert r["stats"]["communities"] == 1 and r["stats"]["largest"] == 51
    moved, ok, q = r["trace"][0]
    assert moved > 0 and ok == 0                                 # the centre and some leaves move past each other
    assert r["trace"][1][1] == 1                                 # ... and the next one is accepted
    r = model.louvain(*lpa_cases.star(5000))
    assert r["stats"]["communities"] == 1 and r["items"] > 0 and model.LONG_FILL in r["kinds"]


def test_two_triangles():
    r = model.louvain(*cases.two_triangles())
    assert r["stats"]["communities"] == 2 and lpa_cases.same_partition(r["labels"], [0, 0, 0, 1, 1, 1])
    assert abs(model.modularity(r) - 5.0 / 14.0) <= 1e-15


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(n):
    for ro, ci in (lpa_cases.empty(n), lpa_cases.directed(n, np.arange(n), np.arange(n))):    # (and self-loops only)
        for symmetric in (True, False):
            r = model.louvain(ro, ci, symmetric)
            assert np.array_equal(r["labels"], np.arange(n)) and r["levels"] == [] and r["trace"] == [] and r["kinds"] == []
            assert r["stats"] == dict(communities=n, largest=1, largest_id=0, levels=0, s_in=0, s_sq=0, w=0)
            assert model.modularity(r) == 0.0


def test_multiplicity_and_dropped_self_loops():
    ro, ci = lpa_cases.random_symmetric(500, 1500, 4)
    plain = model.louvain(ro, ci)
    looped = model.louvain(*lpa_cases.tripled_with_loops(ro, ci))           # every entry three times, self-loops on a third
    assert looped["stats"]["w"] == 3 * plain["stats"]["w"]
    # (weights times three: every score and every Qnum difference times nine, the same moves, the same labels)
    assert np.array_equal(plain["labels"], looped["labels"])
    assert [(m, ok, 9 * q) for m, ok, q in plain["trace"]] == looped["trace"]
    r = model.louvain(*cases.loops_and_duplicates())
    assert r["stats"]["w"] == 2 * 6 and r["stats"]["communities"] in (1, 2)
    r = model.louvain(*lpa_cases.multiplicity(), max_iter=1, max_levels=1)
    assert r["labels"][0] == r["labels"][2]                     # three entries to 2 against one to 1


def test_caps():
    ro, ci = lpa_cases.random_symmetric(300, 900, 1)
    r = model.louvain(ro, ci, max_iter=0)
    assert np.array_equal(r["labels"], np.arange(300)) and r["stats"]["levels"] == 0 and r["levels"][0][2:4] == (0, 0)
    assert r["kinds"] == [model.SETUP, model.DONE]
    r = model.louvain(ro, ci, max_levels=0)
    assert np.array_equal(r["labels"], np.arange(300)) and r["levels"] == [] and r["stats"]["w"] > 0
    q = lpa_model.modularity(ro, ci, r["labels"], True)
    assert (q[1], q[2], q[3]) == (r["stats"]["s_in"], r["stats"]["s_sq"], r["stats"]["w"])
    one = model.louvain(ro, ci, max_levels=1)
    full = model.louvain(ro, ci)
    assert one["stats"]["levels"] == 1 and len(one["levels"]) == 1 and full["stats"]["levels"] > 1
    assert np.array_equal(one["maps"][0], full["maps"][0]) and one["stats"]["communities"] == full["levels"][0][4]
    r = model.louvain(ro, ci, max_iter=3)
    assert all(lv[2] <= 3 for lv in r["levels"]) and r["levels"][0][2] == 3 and not r["ended"][0]
    r = model.louvain(ro, ci, tol=1.0)                           # nothing gains W^2
    assert r["stats"]["levels"] == 0 and [ok for _, ok, _ in r["trace"]] == [0, 0] and r["ended"] == [True]
    assert model.threshold(1.0, 1 << 31) == 1 << 62 and model.threshold(0.0, 5) == 0 and model.threshold(1e-3, 1000) == 1000


def test_ties():
    """a 4-cycle under identity labels: both neighbours of every vertex score the same, so the smaller key is best; and a vertex
    whose best is there but lies the wrong way round for the iteration's parity stays (the direction test alone blocks it)"""
    ro, ci = cases.tie_square()
    n, rcv, snd, wt = _edges(ro, ci, True)
    k = model.degrees(n, rcv, wt)
    lab = np.arange(4, dtype=np.int64)
    best = model.best_labels(n, rcv, snd, wt, k, 8, lab, model.SEED)
    key = model.keys(np.arange(4), model.SEED)
    for v in range(4):
        a, b = (v - 1) % 4, (v + 1) % 4
        assert best[v] == (a if key[a] < key[b] else b)
    even, moved_even = model.iterate(n, rcv, snd, wt, k, 8, lab, 0, model.SEED)
    odd, moved_odd = model.iterate(n, rcv, snd, wt, k, 8, lab, 1, model.SEED)
    assert moved_even + moved_odd == 4 and 0 < moved_even < 4    # every vertex is blocked in exactly one of the parities
    # a tie the current label wins: a vertex between its own community and an equally good one stays
    ro, ci = lpa_cases.sym(5, [0, 1, 2, 3], [1, 2, 3, 4])
    n, rcv, snd, wt = _edges(ro, ci, True)
    k = model.degrees(n, rcv, wt)
    lab = np.array([0, 0, 2, 4, 4], dtype=np.int64)              # 2 alone between {0, 1} and {3, 4}: equal scores left and right
    best = model.best_labels(n, rcv, snd, wt, k, 8, lab, model.SEED)
    assert best[2] in (0, 4) and best[2] == (0 if model.keys([0], model.SEED)[0] < model.keys([4], model.SEED)[0] else 4)
    lab = np.array([0, 0, 0, 4, 4], dtype=np.int64)              # 2 inside {0, 1, 2}: k_{2,0} W - (5 - 2) 2 = 2 = k_{2,4} W - 3 * 2
    assert model.best_labels(n, rcv, snd, wt, k, 8, lab, model.SEED)[2] == 0


@pytest.mark.parametrize("seed", range(6))
def test_planted_blocks(seed):
    ro, ci, block = lpa_cases.planted_blocks(seed)
    r = model.louvain(ro, ci)
    assert r["stats"]["communities"] == 40 and r["stats"]["largest"] == 50 and lpa_cases.same_partition(r["labels"], block), seed


def test_coarse_levels_have_weights_and_self_entries():
    """a star of cliques: level 0 merges every clique (and the hub into one of them), so the coarse graph has self entries of
    weight clique x (clique - 1) and a hub row of one entry per clique: a wave's row with 100 cliques, a long one with 300"""
    for cliques, body in ((100, 2), (300, 3)):
        ro, ci = cases.star_of_cliques(cliques, 5)
        r = model.louvain(ro, ci)
        steps, (n1, rcv, snd, wt) = _replay(ro, ci, True, r)
        assert r["stats"]["levels"] == 1 and len(r["levels"]) == 2 and n1 == cliques
        assert (rcv == snd).sum() == cliques and int(wt[rcv == snd].min()) >= 20 and int(wt.sum()) == r["stats"]["w"]
        longest = int(np.bincount(rcv).max())
        assert longest == cliques and model.body_bins(np.array([longest]), model.SHORT_MAX, model.WAVE_MAX)[body] == 1


QUALITY = [("random_symmetric(2000, 8000, 3)", lambda: lpa_cases.random_symmetric(2000, 8000, 3)),
           ("grid(40, 40)", lambda: lpa_cases.grid(40, 40)),
           ("path(5000)", lambda: lpa_cases.path(5000)),
           ("planted_blocks(0)", lambda: lpa_cases.planted_blocks(0)[:2]),
           ("planted_blocks(3)", lambda: lpa_cases.planted_blocks(3)[:2])]


@pytest.mark.parametrize("name,make", QUALITY, ids=[q[0] for q in QUALITY])
def test_quality_against_networkx(name, make):
    nx = pytest.importorskip("networkx")
    ro, ci = make()
    n = len(ro) - 1
    g = nx.MultiGraph()
    g.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(ro))
    keep = rows < np.asarray(ci)                                 # (every pair once; duplicates stay duplicates)
    g.add_edges_from(zip(rows[keep].tolist(), np.asarray(ci)[keep].tolist()))
    theirs = nx.community.modularity(g, nx.community.louvain_communities(g, seed=1))
    ours = model.modularity(model.louvain(ro, ci))
    print(name, "model", round(ours, 4), "networkx", round(theirs, 4), "ratio", round(ours / theirs, 4))
    assert ours >= 0.95 * theirs


def test_two_seeds_two_results():
    ro, ci = lpa_cases.random_symmetric(3000, 9000, 5)
    a = model.louvain(ro, ci, seed=1)
    b = model.louvain(ro, ci, seed=2)
    for r in (a, b):
        q = lpa_model.modularity(ro, ci, r["labels"], True)
        assert (q[1], q[2], q[3]) == (r["stats"]["s_in"], r["stats"]["s_sq"], r["stats"]["w"]) and model.modularity(r) > 0.3
    assert not lpa_cases.same_partition(a["labels"], b["labels"])
