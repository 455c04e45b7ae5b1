"""GPU suite (-m gpu): strongly connected components (mgx_scc_*).  The fused path (mgx_scc_run), the operator path
(mgx_scc_enact) and the numpy model (tests/scc_model.py) agree bit for bit -- labels and stats [0] - [5] -- on the golden
fixtures, hand-made shapes for every step (trim chains, both counters emptied in one pass, long rows at the cuts, fronts at the
sizes of the LDS stage, many rounds), planted partitions, directed R-MAT 10 - 16 and, at RMAT-18, against scipy."""
import os

import numpy as np
import pytest

from tests import cc_model, chain_model
from tests import scc_cases as cases
from tests import scc_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
STATS_WAITS = 1               # the wait for stats [0] - [2], behind the batches'; nothing is built that waits
LONG_MIN, SEG = 32, 256       # the defaults of MGX_SCC_LONG_MIN and MGX_SCC_SEG
DEGREES, LIST, EXPAND, PMAX, PPICK, RINIT, FWD, ROOTS, BWD, SEAL, IDLE = range(1, 12)


def _graph(ctx, ro, ci, upload=False, layout=False):
    import mini_amd
    if upload:
        co, ri = cc_model.transpose(ro, ci)
        g = mini_amd.Graph.from_host(ctx, ro, ci, None, co, ri)
    else:
        g = mini_amd.Graph.from_host(ctx, ro, ci, None)
        g.build_csc()
    if layout:
        g.build_layout()
    return g


def launches_by_the_log(kinds):
    """K of a run whose log holds its end: the number of the first idle launch, plus one.  Where no model predicts the launches (a
    forward sweep's length depends on what a load sees), this is what ties the host's loop to the device's end: the launches
    enqueued and the host's waits follow from it (tests/chain_model.py), not from what the host enqueued"""
    idle = np.flatnonzero(kinds == IDLE)
    assert len(idle) and (kinds[idle[0]:] == IDLE).all(), "nothing runs behind the first idle launch"
    return int(idle[0]) + 1


def _check(ctx, ro, ci, want=None, upload=False, layout=False, operator=True, want_kinds=None):
    """fused == operator path == model on labels and stats [0] - [5]; the repeat run; the launches' kinds; the launches and the host
    waits from the run's end.  want_kinds: the kinds of every launch up to the first idle one, where the graph determines them
    (scc_model.path_kinds, ring_kinds); else the end is read from the log"""
    import mini_amd
    w = model.decompose(ro, ci) if want is None else want
    g = _graph(ctx, ro, ci, upload, layout)
    sp = mini_amd.SccProblem(g)
    s1 = sp.run()
    print("fused", s1)
    l1 = sp.labels()
    assert l1.dtype == np.int32
    assert np.array_equal(l1, w["labels"]), "fused: %d of %d labels differ" % (int((l1 != w["labels"]).sum()), len(l1))
    assert {k: s1[k] for k in KEYS} == w["stats"], (s1, w["stats"])
    kinds = sp.step_kinds()
    st = w["stats"]
    if want_kinds is not None:
        assert kinds.tolist() == chain_model.logged(want_kinds, IDLE), "the log: the predicted kinds, then IDLE, its first 2^16"
        n_kinds = len(want_kinds)
    else:
        n_kinds = launches_by_the_log(kinds)
    waits, launches = chain_model.waits_and_launches(n_kinds)
    assert s1["launches"] == launches and s1["host_waits"] == waits + STATS_WAITS, (s1, n_kinds, launches, waits)
    assert len(kinds) == min(launches, chain_model.LOG_CAP) and kinds[0] == DEGREES and kinds[1] == LIST
    count = {k: int((kinds == k).sum()) for k in range(1, 12)}
    phases = st["rounds"] + (1 if st["pivot_size"] else 0)
    assert sum(count.values()) == len(kinds)                     # (every launch is one of the eleven kinds)
    assert count[DEGREES] == 1 and count[LIST] == 1 and count[PMAX] == count[PPICK] == (1 if st["pivot_size"] else 0)
    if launches <= chain_model.LOG_CAP:
        assert kinds[-1] == IDLE and count[IDLE] == launches - n_kinds + 1
        assert count[RINIT] == count[ROOTS] == count[SEAL] == phases
        assert count[FWD] >= phases and count[BWD] >= phases and count[EXPAND] >= phases
    else:
        # the log ends before the run does: what it holds is the run's first 2^16 launches, and the run ended all the same
        # (bit 1 of `done`, a fixpoint that did not end, would have thrown; the labels and stats above are the model's)
        assert count[RINIT] <= phases and count[ROOTS] <= phases and count[SEAL] <= phases and count[RINIT] >= min(phases, 1)
        assert count[IDLE] == max(chain_model.LOG_CAP - (n_kinds - 1), 0)
    s2 = sp.run()
    assert s2 == s1, (s1, s2)                                    # a repeat run: the same launches, the same waits
    assert np.array_equal(sp.labels(), l1)
    if operator:
        so = sp.enact()
        print("operator", so)
        lo = sp.labels()
        assert np.array_equal(lo, w["labels"]), "operator path: %d of %d labels differ" % (int((lo != w["labels"]).sum()), len(lo))
        assert {k: so[k] for k in KEYS} == w["stats"], (so, w["stats"])
        assert so["host_waits"] >= 1
    sp.close()
    g.close()
    return w, s1


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("upload", [False, True])
def test_fixtures(gpu_ctx, oracle, name, upload):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=False)
    w, _ = _check(gpu_ctx, ro, ci, upload=upload, layout=upload)           # (an attached layout is ignored)
    assert np.array_equal(w["labels"], model.scipy_labels(ro, ci))


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    w, s = _check(gpu_ctx, np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    assert s["components"] == n and s["trimmed"] == n and s["pivot_size"] == 0 and s["rounds"] == 0


def test_self_loops_only(gpu_ctx):
    v = np.arange(3000)
    w, s = _check(gpu_ctx, *cases.directed(3000, v, v))
    assert s["components"] == 3000 and s["trimmed"] == 3000 and s["pivot_size"] == 0


def test_every_arc_three_times_plus_self_loops(gpu_ctx):
    n = 3000
    ro, ci = cases.random_digraph(n, 4500, 5)
    plain = model.decompose(ro, ci)
    src = np.repeat(np.arange(n), np.diff(ro))
    loops = np.arange(0, n, 3)
    w, s = _check(gpu_ctx, *cases.directed(n, np.concatenate([src, src, src, loops]), np.concatenate([ci, ci, ci, loops])))
    assert np.array_equal(w["labels"], plain["labels"]) and w["stats"] == plain["stats"] and s["pivot_size"] > 1


def test_unsorted_rows(gpu_ctx):
    ro, ci = cases.random_digraph(2000, 6000, 6)
    rng = np.random.default_rng(6)
    ci = ci.copy()
    for v in range(2000):
        rng.shuffle(ci[ro[v]:ro[v + 1]])
    _check(gpu_ctx, ro, ci)
    _check(gpu_ctx, ro, ci, upload=True)


@pytest.mark.parametrize("n", [2, 3, 5000])
def test_ring(gpu_ctx, n):
    """one component, the pivot's; 5000: as many forward and backward sweeps, across the first batches of launches"""
    w, s = _check(gpu_ctx, *cases.ring(n), want_kinds=model.ring_kinds(n))           # (one hop a launch: the kinds are the graph's)
    assert s["components"] == 1 and s["pivot_size"] == n and s["trimmed"] == 0 and s["launches"] >= 2 * n


@pytest.mark.parametrize("n", [3, 5000])
def test_path(gpu_ctx, n):
    """3: the middle vertex loses both counters in one pass and is removed once; 5000: 2500 trim passes"""
    w, s = _check(gpu_ctx, *cases.path(n), want_kinds=model.path_kinds(n))           # (trim only: the kinds are the graph's)
    assert s["components"] == n and s["trimmed"] == n and s["pivot_size"] == 0
    assert s["launches"] >= n // 2


def test_stars_and_clique(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.star(100000))                  # a long out-row and a long in-row: one component
    assert s["components"] == 1 and s["pivot_size"] == 100001
    w, s = _check(gpu_ctx, *cases.star(100000, back=False))      # the out-star: all trimmed
    assert s["components"] == 100001 and s["trimmed"] == 100001
    v = np.arange(300)
    a, b = np.meshgrid(v, v, indexing="ij")
    w, s = _check(gpu_ctx, *cases.directed(300, a[a != b], b[a != b]))
    assert s["components"] == 1 and s["pivot_size"] == 300


@pytest.mark.parametrize("leaves", [LONG_MIN - 1, LONG_MIN, SEG - 1, SEG, SEG + 1, 2 * SEG + 1])
def test_centre_rows_at_the_cuts(gpu_ctx, leaves):
    """bidirected stars whose centre rows have exactly `leaves` entries, and the same with a tail that is trimmed first"""
    w, s = _check(gpu_ctx, *cases.star(leaves))
    assert s["components"] == 1 and s["pivot_size"] == leaves + 1
    l = 1 + np.arange(leaves)
    z = np.zeros(leaves, dtype=np.int64)
    tail = leaves + 1 + np.arange(40)                            # leaf 1 -> a path of 40: trimmed from its far end
    ro, ci = cases.directed(leaves + 41, np.concatenate([z, l, [1], tail[:-1]]), np.concatenate([l, z, [tail[0]], tail[1:]]))
    w, s = _check(gpu_ctx, ro, ci)
    assert s["trimmed"] == 40 and s["pivot_size"] == leaves + 1


@pytest.mark.parametrize("env", [{"MGX_SCC_SEG": "1"}, {"MGX_SCC_LONG_MIN": "1"}, {"MGX_SCC_SEG": "1", "MGX_SCC_LONG_MIN": "1"},
                                 {"MGX_SCC_SEG": "3", "MGX_SCC_LONG_MIN": "2"}])
def test_forced_work_shapes(gpu_ctx, monkeypatch, env):
    """every row long, every segment one entry: the items' paths on small graphs (the switches are read once per handle)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ro, ci, labels = cases.planted(60, 9, 300, 3, 2)
    w, _ = _check(gpu_ctx, ro, ci)
    assert np.array_equal(w["labels"], labels)
    _check(gpu_ctx, *cases.random_digraph(500, 900, 8))
    _check(gpu_ctx, *cases.star(70))
    _check(gpu_ctx, *cases.cycle_chain(6))


@pytest.mark.parametrize("k", [127, 128, 129, 257, 5120])
def test_trim_fronts_appended_by_the_expand(gpu_ctx, k):
    """s -> a_1 .. a_k -> one 2-cycle: the expand of {s} appends a front of exactly k"""
    w, s = _check(gpu_ctx, *cases.layered_trim(k))
    assert s["trimmed"] == k + 1 and s["pivot_size"] == 2 and s["rounds"] == 0


@pytest.mark.parametrize("k", [127, 128, 129, 257, 5120])
def test_sweep_fronts(gpu_ctx, k):
    """the fan: the pivot's forward sweep appends a front of exactly k, then one round takes all k cycles"""
    w, s = _check(gpu_ctx, *cases.fan(k))
    assert s["pivot_size"] == 2 and s["rounds"] == 1 and s["components"] == k + 1


def test_chains_of_two_cycles(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.cycle_chain(40, ascending=True))
    assert s["rounds"] == 39 and s["pivot_size"] == 2
    w, s = _check(gpu_ctx, *cases.cycle_chain(40, ascending=False))
    assert s["rounds"] == 1 and s["pivot_size"] == 2


@pytest.mark.parametrize("nc,maxsz,cross,chords", [(300, 64, 3000, 4), (2000, 8, 20000, 2)])
def test_planted(gpu_ctx, nc, maxsz, cross, chords):
    ro, ci, labels = cases.planted(nc, maxsz, cross, nc + chords, chords)
    w, s = _check(gpu_ctx, ro, ci)
    assert np.array_equal(w["labels"], labels) and s["components"] == nc and s["rounds"] > 1


@pytest.mark.parametrize("scale,ef", [(10, 2), (12, 4), (14, 8), (16, 4)])
def test_rmat_directed(gpu_ctx, oracle, scale, ef):
    """fused == model; up to RMAT-14 the operator path as well"""
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    w, s = _check(gpu_ctx, ro, ci, operator=scale <= 14)
    assert s["pivot_size"] == s["largest"] > n // 8 and s["trimmed"] > 0


def test_rmat18_against_scipy(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(18, 8, 118, undir=False)
    g = _graph(gpu_ctx, ro, ci)
    sp = mini_amd.SccProblem(g)
    s = sp.run()
    want = model.scipy_labels(ro, ci)
    assert np.array_equal(sp.labels(), want)
    assert (s["components"], s["largest"], s["largest_label"]) == model.label_stats(want)
    waits, launches = chain_model.waits_and_launches(launches_by_the_log(sp.step_kinds()))
    assert s["launches"] == launches and s["host_waits"] == waits + STATS_WAITS, (s, launches, waits)
    sp.close()
    g.close()


def test_rmat12_on_one_compute_unit(monkeypatch, torch_mod, oracle, built):
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 112, undir=False)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, ro, ci)


def test_needs_the_genuine_csc(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_digraph(400, 700, 9)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.SccProblem(g)
    for go in (sp.run, sp.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go()
        assert err.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(err.value)
    g.build_csc()                                                # the handle is still usable
    want = model.decompose(ro, ci)
    assert {k: v for k, v in sp.run().items() if k in KEYS} == want["stats"] and np.array_equal(sp.labels(), want["labels"])
    assert {k: v for k, v in sp.enact().items() if k in KEYS} == want["stats"] and np.array_equal(sp.labels(), want["labels"])
    sp.close()
    g.close()


def test_labels_before_any_run(gpu_ctx):
    import mini_amd
    g = _graph(gpu_ctx, *cases.ring(5))
    sp = mini_amd.SccProblem(g)
    for call in (sp.labels, sp.labels_device_ptr, sp.step_kinds, sp.phase_ms):
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert "no run yet" in str(err.value)
    sp.set_timing(True)
    sp.run()
    ms = sp.phase_ms()
    assert set(ms) == {"init", "trim", "pivot", "rounds"} and all(v >= 0.0 for v in ms.values()) and ms["pivot"] > 0.0
    assert sp.labels_device_ptr()
    sp.close()
    g.close()
