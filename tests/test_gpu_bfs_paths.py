"""Fused BFS: every level body at its threshold and capacity edges.

The graphs are tests/bfs_cases.py's (labels known by construction; tests/test_bfs_cases_cpu.py proves that they sit on their edges),
the expected counters tests/bfs_model.py's walk of the launches.  A case runs on a fresh Graph and BfsProblem with its switches set
before either is made (the layout and the handle read them once), from its source three times, from another source, and from its
source again: the handle learns its launch sequence from the runs before (slots_hint, cls_max, tail_from), and the cases are
built so that the counters do not depend on it -- the labels never may.  (One case cannot be: mini_short_rows is marked adaptive,
its runs report one of the counter sets the model's walks give, in the order a fresh handle's learning implies.)

`slots` is the number of slots the host ENQUEUED (bfs_fused_state_t::slots_used), which is what the handle learns: it is only
bounded from below here, by the slots the model says find work.  The fused traversal writes no predecessors (mgx_bfs_preds stays
-1 as in the reference, tests/test_gpu_parity.py); that the labels are a BFS tree's -- every reached vertex has an in-neighbour one
level up -- is part of what the constructed labels are checked for on the CPU."""
import numpy as np
import pytest

from tests import bfs_cases as bc
from tests import bfs_model as bm
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

SWITCHES = sorted({k for c in bc.CASES.values() for k in c["env"]})
EXACT = ("levels", "reached", "m_t", "frontier_vertices", "push_levels", "small_levels", "dense_slots", "vshort_slots", "lazy_slots",
         "cold_slots", "mini_slots", "pull_edges")


def _cold_pairs(G, g, long_min):
    """entries of the layout's long rows that point behind the unit-block body's LDS prefix, counted in the layout's CSR"""
    if g.n <= bc.HOT_N:
        return 0
    lro, lci, _, _ = G.layout_arrays()
    deg = np.diff(lro.astype(np.int64))
    rows_long = int((deg >= long_min).sum())                   # a degree-sorted layout: the long rows come first
    return int((lci[:lro[rows_long]] >= bc.HOT_N).sum())


def _setup(ctx, monkeypatch, name, member, ids, layout):
    import mini_amd
    case = bc.CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    g = case["graph"](member, ids)
    G = mini_amd.Graph.from_host(ctx, g.ro, g.ci, None)
    cold_pairs = 0
    if case["mode"] == 1:
        G.build_csc()               # (a directed graph: the bottom-up levels need its in-edges)
    if layout:
        G.build_layout()
        long_min = bm.Config(case["env"], g.n, False).long_min
        info = G.layout_info()
        ub, vs = bm.layout_numbers(g.deg, long_min)
        assert info["has_layout"] == 1 and info["units"] == ub, (name, info, ub)
        lro = G.layout_arrays()[0].astype(np.int64)
        assert np.all(np.diff(np.diff(lro)) <= 0), "the layout is sorted by degree: its classes follow from the degrees alone"
        if long_min > 0:
            cold_pairs = _cold_pairs(G, g, long_min)
            want = cold_pairs if (0 < cold_pairs * 4 <= ub * 64) else 0
            assert info["cold_pairs"] == want, (name, info, cold_pairs)
        if 0 < long_min <= 64:
            # the lane classes the vertex-by-vertex body cuts the layout into are those of the case's degrees
            assert bm.vs_classes(np.diff(lro), long_min) == bm.vs_classes(np.sort(g.deg)[::-1], long_min)
    cfg = bm.config_for(case["env"], g, layout, case["mode"], case["alpha"], cold_pairs=cold_pairs)
    shapes = g.shapes(cfg.long_min)
    want = [c for c, _ in bm.outcomes(cfg, shapes, g.tree)] if case["adaptive"] else bm.predict(cfg, shapes, g.tree)[0]
    return case, g, G, mini_amd.BfsProblem(G, g.src), shapes, want


def _check_run(bfs, g, shapes, want, st, tag):
    assert np.array_equal(bfs.labels(), g.labels), tag
    got = {k: st[k] for k in EXACT}
    print(tag, "slots", st["slots"], got)
    if isinstance(want, list):        # (an adaptive case: one of what the handle's launch sequences can give)
        assert got in [{k: w[k] for k in EXACT} for w in want], (tag, got, want)
        want = want[0]                # (the slots that find work are the same in all of them)
    else:
        assert got == {k: want[k] for k in EXACT}, (tag, got, want)
    assert st["slots"] >= want["slots_found"], (tag, st["slots"], want["slots_found"])
    assert bfs.level_trace() == bm.trace(shapes), tag
    return got


def _run_members(ctx, monkeypatch, name, ids, layout):
    case = bc.CASES[name]
    seen = {}
    for member in case["members"]:
        case, g, G, bfs, shapes, want = _setup(ctx, monkeypatch, name, member, ids, layout)
        # another source: the last vertex of the last level.  Its entries (if it has any) are filler -- they name the source -- so what
        # it reaches is known by construction too: itself, the source one level down, and everything else one level deeper than before
        other = int(np.flatnonzero(g.labels == len(g.level_rows) - 1)[-1])
        assert other != g.src
        if g.deg[other] == 0:
            moved = np.full(g.n, -1, dtype=np.int32)
        else:
            moved = np.where(g.labels >= 0, g.labels + 1, -1).astype(np.int32)
        moved[other] = 0
        runs = []
        for i, src in enumerate((g.src, g.src, g.src, other, g.src)):
            st = bfs.run(src, case["mode"], case["alpha"])
            if src == other:
                assert np.array_equal(bfs.labels(), moved), (name, member, "the other source")
                assert st["reached"] == int((moved >= 0).sum()) and st["m_t"] == int(g.deg[moved >= 0].sum())
                continue
            runs.append(_check_run(bfs, g, shapes, want, st, (name, member, ids, layout, "run %d" % i)))
        assert np.all(bfs.preds() == -1)          # (the fused traversal writes no predecessors: include/mgx.h)
        if case["adaptive"]:
            # what always holds: every level is a chain's, an M launch's or a slot's -- and a fresh handle's five slots take level 2
            # themselves, a handle that has seen the traversal leaves it to the M launch behind its one slot when it is mid-size
            assert all(r["small_levels"] == r["mini_slots"] and r["levels"] == 3 for r in runs)
            assert [r["mini_slots"] for r in runs] == ([1, 2, 2, 2] if len(want) == 2 else [1, 1, 1, 1]), (name, member, runs)
            runs = runs[1:]
        assert all(r == runs[0] for r in runs)
        seen[member] = runs[0]
        bfs.close()
        G.close()
    if case["pair"]:
        counter, delta = case["pair"][1], (case["pair"][2] if len(case["pair"]) > 2 else 1)
        assert seen["at"][counter] == seen["beyond"][counter] + delta, (name, counter, seen)
        assert seen["at"]["levels"] == seen["beyond"]["levels"]


def _params():
    out = []
    for name in sorted(bc.CASES):
        for layout in bc.CASES[name]["layouts"]:
            for ids in bc.CASES[name]["ids"]:
                out.append(pytest.param(name, ids, layout, id="%s-%s-%s" % (name, ids, "layout" if layout else "plain")))
    return out


@pytest.mark.parametrize("name,ids,layout", _params())
def test_case(gpu_ctx, monkeypatch, name, ids, layout):
    _run_members(gpu_ctx, monkeypatch, name, ids, layout)


ONE_CU = sorted(bc.CASES)


@pytest.mark.parametrize("name", ONE_CU)
def test_case_on_one_compute_unit(built, torch_mod, monkeypatch, name):
    """the same with grids of one compute unit's workgroups: every grid-stride loop takes several trips"""
    layout = bc.CASES[name]["layouts"][-1]
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _run_members(ctx, monkeypatch, name, bc.CASES[name]["ids"][-1], layout)


@pytest.mark.parametrize("name", ["contested_chain", "contested_mini", "contested_slot"])
@pytest.mark.parametrize("layout", [False, True])
def test_contested_claims_cover_the_discoveries(gpu_ctx, monkeypatch, name, layout):
    """with the claims counted (the kernel-timing mode of the tools: the parts of a push as launches of their own) every discovery
    but the source has at least one claim"""
    case, g, G, bfs, shapes, want = _setup(gpu_ctx, monkeypatch, name, "at", 7, layout)
    bfs.set_kernel_timing(True)
    for i in range(2):
        st = bfs.run(g.src)
        assert np.array_equal(bfs.labels(), g.labels), (name, layout, i)
        assert st["reached"] == g.reachable
        print(name, layout, "claims", st["claims"], "reached", st["reached"])
        assert st["claims"] >= st["reached"] - 1, (name, layout, st["claims"], st["reached"])


def test_run_many_over_a_deep_path_and_a_hub(gpu_ctx, monkeypatch):
    """a batch of [the path's head, a hub, the path's head]: a traversal of 5000 levels next to one of one level; the last
    source's labels are the handle's"""
    import mini_amd
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    d, fan = 5000, 300
    p = bc.Layered([[bc.rows(1, 1, 1)]] * d + [[bc.rows(1, 0)]], ids="spec")
    # the hub and its leaves behind the path's vertices (two components; ids as specified)
    n = p.n + 1 + fan
    ro = np.concatenate([p.ro, p.ro[-1] + np.concatenate([[fan], np.full(fan, fan)])]).astype(np.int32)
    ci = np.concatenate([p.ci, np.arange(p.n + 1, n)]).astype(np.int32)
    hub = p.n
    lab_path = np.concatenate([p.labels, np.full(1 + fan, -1)]).astype(np.int32)
    lab_hub = np.full(n, -1, dtype=np.int32)
    lab_hub[hub] = 0
    lab_hub[hub + 1:] = 1
    assert np.array_equal(bc.numpy_bfs(ro, ci, hub), lab_hub) and np.array_equal(bc.numpy_bfs(ro, ci, p.src), lab_path)
    for layout in (False, True):
        G = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
        if layout:
            G.build_layout()
        bfs = mini_amd.BfsProblem(G, p.src)
        for srcs, last in (([p.src, hub, p.src], lab_path), ([hub, p.src, hub], lab_hub)):
            stats, reruns = bfs.run_many(srcs)
            assert np.array_equal(bfs.labels(), last), (layout, srcs)
            for s, st in zip(srcs, stats):
                lv, re_, mt = (d, d + 1, d) if s == p.src else (1, fan + 1, fan)
                assert (st["levels"], st["reached"], st["m_t"]) == (lv, re_, mt), (layout, srcs, s, st)
        bfs.close()
        G.close()
