"""GPU suite (-m gpu): the launch chain's protocol (include/mgx/launch_chain.hpp) on its edges, for the six fused paths
that run as one: k-core, k-truss, SCC, label propagation, multi-source BFS and Louvain.

K is the number of a run's first idle launch plus one, predicted by the algorithm's model and pinned per case in
tests/chain_cases.py.  The host enqueues 64, 128, 256, 256 ... launches and waits once per batch, so K = 64 | 65, 192 | 193 and
448 | 449 are where one launch decides whether it needs another batch, and K = 65 535, 65 536, 65 537 where the log of kinds ends.
  seams       every algorithm at every seam value (Louvain: where 3 t + 2 or 5 t + 2 allows, see chain_cases), through the
              algorithm's own check -- labels, stats, traces and kinds against the model -- and then: the launches enqueued and the
              host's waits are chain_model.waits_and_launches(K)'s, the log the model's kinds and IDLE behind them
  timed       a case on each side of 64 | 65 per algorithm that has set_timing: the timed run gives what the untimed one gave
  short after long   K = 449, then K <= 64, then 449 again: the log is not cleared between runs, and nothing of the run before shows
  the cap     label propagation at K = 65 535, 65 536, 65 537; multi-source BFS with as many levels; SCC on the first ring past the cap
Not covered: k-core, k-truss and Louvain have no small input of 65 536 launches (stairs and grids grow quadratically, Louvain's
guarded moves converge).  k-core and k-truss read their log with the reader label propagation and SCC use, which the cap cases
run; Louvain copies each level's log into a host vector with a reader of its own (louvain_fused.hpp), and that one's slice at
the cap no test executes."""
import numpy as np
import pytest

from tests import chain_cases as cases
from tests import chain_model, lpa_model, msbfs_model, scc_model
from tests import test_gpu_kcore_paths as t_kcore
from tests import test_gpu_ktruss as t_ktruss
from tests import test_gpu_louvain as t_louvain
from tests import test_gpu_lpa as t_lpa
from tests import test_gpu_msbfs as t_msbfs
from tests import test_gpu_scc as t_scc

pytestmark = pytest.mark.gpu

# the host waits of a run beside its chain's (each suite names its own)
EXTRA_WAITS = {"lpa": t_lpa.STATS_WAITS, "scc": t_scc.STATS_WAITS, "msbfs": t_msbfs.READ_BACK_WAITS, "kcore": 0}


def _setenv(monkeypatch, case):
    """the switches a case's handle reads (once, when it is made)"""
    opts = case.args.get("opts") or {}
    if case.algo == "lpa":
        t_lpa._setenv(monkeypatch, opts)
    if case.algo == "louvain":
        t_louvain._setenv(monkeypatch, opts)


def _check_case(ctx, case, operator=True):
    """the case through its algorithm's check (results, stats, traces, kinds against the model; the repeat run; the operator path),
    then the launches and the host waits against the pinned K"""
    ro, ci = cases.graph(case)
    a = case.args
    want = cases.wanted(case)
    assert cases.predicted_k(case) == case.K
    waits, launches = chain_model.waits_and_launches(case.K)
    if case.algo == "lpa":
        _, s = t_lpa._check(ctx, ro, ci, True, a["mode"], max_iter=a["max_iter"], operator=operator, opts=a["opts"], want=want)
    elif case.algo == "scc":
        _, s = t_scc._check(ctx, ro, ci, want=want, operator=operator, want_kinds=a["kinds"]())
    elif case.algo == "msbfs":
        _, s = t_msbfs._check(ctx, ro, ci, a["sources"], a["symmetric"], operator=operator, want=want)
    elif case.algo == "ktruss":
        # (launches counts the build's and the supports' too: the peel's own count is the log's length, which the check holds
        # against the model's kinds, IDLE up to `launches` included)
        assert len(chain_model.logged(t_ktruss.model.peel_kinds(want), t_ktruss.IDLE)) == launches
        _, s = t_ktruss._check(ctx, ro, ci, True, want=want, operator=operator)
        assert s["host_waits"] == waits + t_ktruss.BUILD_WAITS, (s, waits)
        return
    elif case.algo == "kcore":
        import mini_amd
        g = t_kcore._graph(ctx, ro, ci)
        kc = mini_amd.KcoreProblem(g)
        largest, s = kc.run()
        t_kcore.check_run(kc, largest, s, want)
        s = dict(s, launches=len(kc.step_kinds()))
        largest2, s2 = kc.run()                                  # a repeat run: the same launches, the same waits
        t_kcore.check_run(kc, largest2, s2, want)
        kc.close()
        g.close()
    else:
        _, s = t_louvain._check(ctx, ro, ci, True, max_iter=a["max_iter"], opts=a["opts"], operator=operator, want=want)
        chains = t_louvain.model.chains(want["kinds"])           # (the first level's is the pinned K: asserted above)
        assert s["launches"] == sum(chain_model.waits_and_launches(k)[1] for k in chains), (s, chains)
        return                                                   # (the waits beside the chains' are the aggregation's: the check counts them)
    assert s["launches"] == launches and s["host_waits"] == waits + EXTRA_WAITS[case.algo], (s, case.K, launches, waits)


@pytest.mark.parametrize("case", cases.SEAM_CASES, ids=cases.case_id)
def test_seam(gpu_ctx, monkeypatch, case):
    _setenv(monkeypatch, case)
    # (the k-truss operator path rescans every edge in every pass: beside the fused path on the smallest grids only)
    _check_case(gpu_ctx, case, operator=case.algo != "ktruss" or case.K < 100)


# ---- a timed run is the untimed run ----
def _open(ctx, case):
    """-> (graph, handle, run: () -> stats as a dict, results: () -> arrays and lists, the kinds among them)"""
    import mini_amd
    ro, ci = cases.graph(case)
    a = case.args
    if case.algo == "lpa":
        g = t_lpa._graph(ctx, ro, ci)
        p = mini_amd.LpaProblem(g)
        return g, p, lambda: p.run(symmetric=True, mode=a["mode"], max_iter=a["max_iter"]), lambda: [p.labels(), p.trace(), p.step_kinds()]
    if case.algo == "scc":
        g = t_scc._graph(ctx, ro, ci)
        p = mini_amd.SccProblem(g)
        return g, p, p.run, lambda: [p.labels(), p.step_kinds()]
    if case.algo == "msbfs":
        g = t_msbfs._graph(ctx, ro, ci)
        p = mini_amd.MsBfsProblem(g)
        return (g, p, lambda: p.run(a["sources"], a["symmetric"], depths=True),
                lambda: [p.depths(), p.reach(), p.farness(), p.eccentricity(), p.harmonic(), p.level_kinds()] + list(p.vertex_sums()))
    if case.algo == "ktruss":
        g = t_ktruss._graph(ctx, ro, ci)
        p = mini_amd.KtrussProblem(g)
        # (not the peel order: inside a pass's front it is the order of the appends, no run's is another's)
        return g, p, lambda: p.run(True), lambda: list(p.edges()) + [p.support(), p.vertex_truss(), p.histogram(), p.step_kinds()]
    g = t_louvain._graph(ctx, ro, ci)
    p = mini_amd.LouvainProblem(g)
    return (g, p, lambda: p.run(symmetric=True, max_iter=a["max_iter"]),
            lambda: [p.labels(), p.trace(), p.step_kinds()] + list(p.dendrogram()))


TIMED = [c for algo in ("lpa", "scc", "msbfs", "ktruss", "louvain") for c in cases.SEAM_CASES
         if c.algo == algo and c.K in ((62, 65) if algo == "louvain" else (64, 65)) and not c.name.startswith("ring")]


@pytest.mark.parametrize("case", TIMED, ids=cases.case_id)
def test_timing_changes_nothing(gpu_ctx, monkeypatch, case):
    """the clock's tick is the first thread's, beside the kind's decision: a timed run takes the same launches, the host the same
    waits, and every result is the same"""
    _setenv(monkeypatch, case)
    g, p, run, results = _open(gpu_ctx, case)
    run()                                                        # (k-truss: the run that builds)
    plain, plain_results = run(), results()
    p.set_timing(True)
    timed, timed_results = run(), results()
    ms = p.phase_ms()
    p.set_timing(False)
    again = run()
    print(case.name, plain, ms)
    assert timed == plain == again, (plain, timed, again)        # (stats, launches and host waits)
    waits, launches = chain_model.waits_and_launches(case.K)
    if case.algo != "louvain":                                   # (Louvain: one chain per level; the seam test holds their sum)
        assert (len(p.step_kinds()) if case.algo == "ktruss" else timed["launches"]) == launches
    assert len(timed_results) == len(plain_results)
    for a, b in zip(plain_results, timed_results):
        assert np.array_equal(a, b)
    assert set(ms) == set(p.PHASES) and all(v >= 0.0 for v in ms.values()) and any(v > 0.0 for v in ms.values()), ms
    p.close()
    g.close()


# ---- the log is not cleared between runs ----
def test_lpa_short_after_long_on_one_handle(gpu_ctx):
    """the pair of vertices: max_iter 223 is K = 449 (704 launches), max_iter 30 is K = 63 (64 launches).  The short run's log is its
    own 64 entries although entries 64 .. 703 of the long run's still lie behind them on the device; the long run after it
    overwrites all 704"""
    import mini_amd
    long_case, short_case = cases.by_k("lpa", 449), cases.by_k("lpa", 63)
    assert cases.graph(long_case)[0].tolist() == cases.graph(short_case)[0].tolist()          # one graph, two max_iter
    g = t_lpa._graph(gpu_ctx, *cases.graph(long_case))
    lp = mini_amd.LpaProblem(g)
    seen = []
    for case, entries in ((long_case, 704), (short_case, 64), (long_case, 704)):
        w = cases.wanted(case)
        s = lp.run(symmetric=True, mode=lpa_model.SYNC, max_iter=case.args["max_iter"])
        kinds = lp.step_kinds()
        assert len(kinds) == entries == s["launches"] and kinds.tolist() == chain_model.logged(w["kinds"], lpa_model.IDLE)
        assert s["host_waits"] == chain_model.waits_and_launches(case.K)[0] + t_lpa.STATS_WAITS
        assert np.array_equal(lp.labels(), w["labels"]) and {k: s[k] for k in t_lpa.KEYS} == w["stats"]
        assert [tuple(x) for x in lp.trace()[:, :2].tolist()] == w["trace"]
        seen.append((s, kinds.tolist()))
    assert seen[0] == seen[2]
    lp.close()
    g.close()


def test_kcore_short_between_long_runs(gpu_ctx):
    """a k-core handle is its graph's, so a handle's log is only ever overwritten by an equal run: the K = 449 stairs and a K <= 64
    case take turns, each on its handle, as tests/test_gpu_kcore_paths.py interleaves its two -- 704, 64, 704 entries, each the
    run's own, and the long handle's log still its own after the short run"""
    import mini_amd
    long_case, short_case = cases.by_k("kcore", 449), cases.by_k("kcore", 64)
    graphs = {c.name: t_kcore._graph(gpu_ctx, *cases.graph(c)) for c in (long_case, short_case)}
    kcs = {name: mini_amd.KcoreProblem(g) for name, g in graphs.items()}
    seen = []
    for case, entries in ((long_case, 704), (short_case, 64), (long_case, 704)):
        kc = kcs[case.name]
        largest, st = kc.run()
        t_kcore.check_run(kc, largest, st, cases.wanted(case))
        assert len(kc.step_kinds()) == entries
        seen.append((largest, st, kc.step_kinds().tolist()))
        assert len(kcs[long_case.name].step_kinds()) == 704      # (the other handle's log still describes ITS last run)
    assert seen[0] == seen[2]
    for name in graphs:
        kcs[name].close()
        graphs[name].close()


# ---- at and past the log's cap ----
@pytest.mark.parametrize("case", cases.LPA_CAP, ids=cases.case_id)
def test_lpa_at_the_cap(gpu_ctx, monkeypatch, case):
    """K = 65 535, 65 536, 65 537: the log holds 65 536 kinds in all three; the IDLE is its last entry but one, its last, and not in
    it.  Labels, trace and stats are the model's all the same.  (Without the operator path, which waits once per iteration.)"""
    _setenv(monkeypatch, case)
    w = cases.wanted(case)
    log = chain_model.logged(w["kinds"], lpa_model.IDLE)
    assert len(w["kinds"]) == case.K and len(log) == chain_model.LOG_CAP
    if case.K <= chain_model.LOG_CAP:
        assert log.index(lpa_model.IDLE) == case.K - 1 and log[case.K - 2] != lpa_model.IDLE
    else:
        assert lpa_model.IDLE not in log and log[-1] == w["kinds"][chain_model.LOG_CAP - 1] and w["kinds"][chain_model.LOG_CAP] == lpa_model.IDLE
    _check_case(gpu_ctx, case, operator=False)


@pytest.mark.parametrize("levels", cases.MSBFS_CAP_LEVELS)
def test_msbfs_at_the_cap(gpu_ctx, levels):
    """the path of `levels` vertices from vertex 0: as many levels, all PUSH; level_kinds keeps the first 65 536.  Vertex v is at
    depth v: deepest, reach, farness and depths in closed form (the model would loop once per level; tests/test_chain_cases_cpu.py
    holds the closed form against it on a short path).  (Without the operator path, which waits once per level.)"""
    want = msbfs_model.path_from_its_end(levels)
    assert len(want["kinds"]) == levels and want["launches"] == 2 * levels + 3 > chain_model.LOG_CAP
    w, s = t_msbfs._check(gpu_ctx, *t_msbfs.cases.path(levels), [0], True, operator=False, want=want)
    waits, launches = chain_model.waits_and_launches(2 * levels + 3)
    assert s["launches"] == launches and s["host_waits"] == waits + t_msbfs.READ_BACK_WAITS
    assert s["deepest"] == levels and s["push_levels"] == levels and s["reach"] == levels - 1


def test_scc_ring_past_the_cap(gpu_ctx):
    """the first directed ring whose launches exceed the log: 2 n + 9 = 65 537.  One component; the log is the run's first 65 536
    kinds, its end not among them; no fixpoint is reported as endless (n launches of one kind are within n + 2).  (The model's
    sweeps would loop once per vertex: the result is stated.  Without the operator path, which waits once per sweep.)"""
    n = cases.SCC_CAP_RING
    kinds = scc_model.ring_kinds(n)
    assert len(kinds) == chain_model.LOG_CAP + 1
    want = {"labels": np.zeros(n, dtype=np.int32),
            "stats": dict(zip(scc_model.STAT_KEYS, (1, n, 0, 0, n, 0)))}
    w, s = t_scc._check(gpu_ctx, *t_scc.cases.ring(n), want=want, operator=False, want_kinds=kinds)
    waits, launches = chain_model.waits_and_launches(len(kinds))
    assert s["launches"] == launches > chain_model.LOG_CAP and s["host_waits"] == waits + t_scc.STATS_WAITS
