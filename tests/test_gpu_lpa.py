"""GPU suite (-m gpu): label propagation and modularity (mgx_lpa_*, mgx_modularity).  The fused path (mgx_lpa_run),
the operator path (mgx_lpa_enact) and the numpy model (tests/lpa_model.py) agree bit for bit -- labels, stats [0] - [5], the
unstable and changed columns of the trace -- on the golden fixtures, rows at every cut between the bodies, tables that overflow,
runs that do not converge, long tails of list iterations, planted blocks and R-MAT 10 - 16; the launches' kinds, the rows
evaluated and the overflowed rows are the ones the model predicts, the host waits exact.  The operator path is compared up to
R-MAT-14: beyond, its segmented sort of every vote per iteration takes more than seconds."""
import os

import numpy as np
import pytest

from tests import cc_model, chain_model
from tests import lpa_cases as cases
from tests import lpa_model as model
from tests.grid_cus import one_cu_context
from tests.test_lpa_cpu import PLANTED_SEEDS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
STATS_WAITS = 1               # the wait for stats [0] - [2], behind the batches'
SHORT_MAX, WAVE_MAX, TABLE, LIST_DIV = model.SHORT_MAX, model.WAVE_MAX, model.TABLE, model.LIST_DIV
SYNC, LAZY = model.SYNC, model.LAZY


def _graph(ctx, ro, ci, csc=None, layout=False):
    """csc: None none, "build" by the library, "upload" with the graph"""
    import mini_amd
    if csc == "upload":
        co, ri = cc_model.transpose(ro, ci)
        g = mini_amd.Graph.from_host(ctx, ro, ci, None, co, ri)
    else:
        g = mini_amd.Graph.from_host(ctx, ro, ci, None)
        if csc == "build":
            g.build_csc()
    if layout:
        g.build_layout()
    return g


def _check(ctx, ro, ci, symmetric=True, mode=LAZY, seed=model.SEED, max_iter=100, csc=None, layout=False, operator=True, opts=None,
           want=None):
    """fused == operator path == model on labels, stats [0] - [5] and the trace; the repeat run; the host waits; the kinds, the
    rows evaluated and the overflowed rows as the model predicts them.  opts: the switches the handle reads, for the model; want: the
    model's result where the caller has it."""
    import mini_amd
    opts = opts or {}
    w = model.propagate(ro, ci, symmetric, mode, seed, max_iter, **opts) if want is None else want
    n = len(ro) - 1
    g = _graph(ctx, ro, ci, csc if csc else (None if symmetric else "build"), layout)
    lp = mini_amd.LpaProblem(g)
    args = dict(symmetric=symmetric, mode=mode, seed=seed, max_iter=max_iter)
    s1 = lp.run(**args)
    print("fused", s1)
    l1 = lp.labels()
    assert l1.dtype == np.int32
    assert np.array_equal(l1, w["labels"]), "fused: %d of %d labels differ" % (int((l1 != w["labels"]).sum()), len(l1))
    assert {k: s1[k] for k in KEYS} == w["stats"], (s1, w["stats"])
    # the launches the model predicts end the run: the host enqueues whole batches up to the one that holds the IDLE, and no more
    waits, launches = chain_model.waits_and_launches(len(w["kinds"]))
    assert s1["launches"] == launches and s1["host_waits"] == waits + STATS_WAITS, (s1, len(w["kinds"]), launches, waits)
    tr = lp.trace()
    assert tr.shape == (w["stats"]["iterations"] + 1, 3)
    assert [tuple(x) for x in tr[:, :2].tolist()] == w["trace"]
    assert tr[:, 2].tolist() == w["evaluated"], (tr[:, 2].tolist(), w["evaluated"], w["active"])
    assert s1["evaluated"] == sum(w["evaluated"]) and s1["overflowed"] == w["overflowed"], (s1, w["overflowed"])
    kinds = lp.step_kinds()
    assert len(kinds) == min(launches, chain_model.LOG_CAP)
    assert kinds.tolist() == chain_model.logged(w["kinds"], model.IDLE), "the log: the model's kinds, then IDLE, its first 2^16"
    b = lp.bins()
    ln = model.row_entries(ro, ci, symmetric)
    sm, wm = b["short_max"], b["wave_max"]
    assert (b["rows_none"], b["rows_short"], b["rows_wave"], b["rows_long"]) == (
        int((ln == 0).sum()), int(((ln > 0) & (ln <= sm)).sum()), int(((ln > sm) & (ln <= wm)).sum()), int((ln > wm).sum()))
    assert b["overflowed"] == s1["overflowed"]
    assert (sm, wm, b["table"], b["list_div"]) == (opts.get("short_max", SHORT_MAX), max(opts.get("wave_max", WAVE_MAX), sm),
                                                   opts.get("table", TABLE), opts.get("list_div", LIST_DIV))
    s2 = lp.run(**args)
    assert s2 == s1, (s1, s2)                                    # a repeat run: the same launches, the same waits
    assert np.array_equal(lp.labels(), l1) and np.array_equal(lp.trace(), tr)
    q, s_in, s_sq, ww = lp.modularity()
    mq, m_in, m_sq, m_w = model.modularity(ro, ci, l1, symmetric)
    assert (s_in, s_sq, ww) == (m_in, m_sq, m_w) and abs(q - float(mq)) <= 1e-12
    if operator:
        so = lp.enact(**args)
        print("operator", so)
        lo = lp.labels()
        assert np.array_equal(lo, w["labels"]), "operator path: %d of %d labels differ" % (int((lo != w["labels"]).sum()), len(lo))
        assert {k: so[k] for k in KEYS} == w["stats"], (so, w["stats"])
        assert so["evaluated"] == n * (w["stats"]["iterations"] + 1) and so["overflowed"] == 0 and so["host_waits"] >= 1
        to = lp.trace()
        assert [tuple(x) for x in to[:, :2].tolist()] == w["trace"] and (to[:, 2] == n).all()
    lp.close()
    g.close()
    return w, s1


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", [SYNC, LAZY])
@pytest.mark.parametrize("upload", [False, True])
@pytest.mark.parametrize("layout", [False, True])
def test_fixtures(gpu_ctx, oracle, name, mode, upload, layout):
    """symmetric = 1 on the symmetrised fixture (the caller's word must be true), symmetric = 0 on the directed one, the CSC built
    or uploaded, each with and without an attached layout, which is ignored"""
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=True)
    _check(gpu_ctx, ro, ci, True, mode, csc="upload" if upload else None, layout=layout)
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=False)
    _check(gpu_ctx, ro, ci, False, mode, csc="upload" if upload else "build", layout=layout)


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    for ro, ci in (cases.empty(n), cases.directed(n, np.arange(n), np.arange(n))):          # (and self-loops only)
        for symmetric in (True, False):
            w, s = _check(gpu_ctx, ro, ci, symmetric)
            assert s["communities"] == n and s["iterations"] == 0 and s["converged"] == 1 and s["launches"] == 64


def test_every_entry_three_times_plus_self_loops(gpu_ctx):
    ro, ci = cases.random_symmetric(3000, 6000, 5)
    plain = model.propagate(ro, ci, True, LAZY)
    w, s = _check(gpu_ctx, *cases.tripled_with_loops(ro, ci), True)
    assert np.array_equal(w["labels"], plain["labels"]) and w["trace"] == plain["trace"]
    ro, ci = cases.random_digraph(3000, 6000, 6)
    _check(gpu_ctx, *cases.tripled_with_loops(ro, ci), False)


def test_multiplicity_decides(gpu_ctx):
    w, _ = _check(gpu_ctx, *cases.multiplicity(), True, SYNC, max_iter=1)
    assert w["labels"][0] == 2
    w, _ = _check(gpu_ctx, *cases.multiplicity(dedup=True), True, SYNC, max_iter=1)
    assert w["labels"][0] == 1


CUTS = [1, SHORT_MAX, SHORT_MAX + 1, WAVE_MAX, WAVE_MAX + 1, TABLE, TABLE + 1]
FORCED = [{}, {"short_max": 0, "wave_max": 0}, {"short_max": 0, "wave_max": 512}, {"short_max": 16, "wave_max": 16},
          {"short_max": 3, "wave_max": 40, "table": 32}]
ENV = {"short_max": "MGX_LPA_SHORT_MAX", "wave_max": "MGX_LPA_WAVE_MAX", "table": "MGX_LPA_TABLE", "list_div": "MGX_LPA_LIST_DIV"}


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(ENV[k], str(v))


@pytest.mark.parametrize("opts", FORCED)
@pytest.mark.parametrize("mode", [SYNC, LAZY])
def test_rows_at_every_cut(gpu_ctx, monkeypatch, opts, mode):
    """disjoint cliques and stars whose vertices have exactly 1, SHORT_MAX, SHORT_MAX + 1 ... TABLE + 1 votes: at the defaults, with
    every row a workgroup's, every row (up to 512 entries) a wave's, no wave rows, and small cuts with a small table (the switches
    are read once per handle)"""
    _setenv(monkeypatch, opts)
    ro, ci = cases.cliques_and_stars(CUTS)
    w, s = _check(gpu_ctx, ro, ci, True, mode, max_iter=12, opts=opts)
    assert s["overflowed"] > 0                                    # (the star of TABLE + 1 leaves, in iteration 0)
    _check(gpu_ctx, ro, ci, False, mode, max_iter=12, opts=opts)  # (both rows of every vertex: every count doubled)
    _check(gpu_ctx, *cases.random_symmetric(500, 3000, 8), True, mode, opts=opts)


@pytest.mark.parametrize("table", [TABLE, 64])
def test_star_overflows_its_table(gpu_ctx, monkeypatch, table):
    monkeypatch.setenv("MGX_LPA_TABLE", str(table))
    w, s = _check(gpu_ctx, *cases.star(5000), True, LAZY, opts={"table": table})
    assert s["overflowed"] >= 1 and s["communities"] == 1 and s["converged"] == 1
    w, s = _check(gpu_ctx, *cases.star(TABLE), True, LAZY, opts={"table": table})           # exactly what the default table holds
    assert (s["overflowed"] == 0) == (table == TABLE)


@pytest.mark.parametrize("table", [TABLE, 64, 256])
def test_winner_among_the_spilled(gpu_ctx, monkeypatch, table):
    """300 distinct labels of one vote each but one with two: it must be found whichever hash class it falls into"""
    monkeypatch.setenv("MGX_LPA_TABLE", str(table))
    monkeypatch.setenv("MGX_LPA_WAVE_MAX", "128")
    for repeated in (1, 217, 300):
        ro, ci = cases.one_repeated_among_many(300, repeated)
        w, s = _check(gpu_ctx, ro, ci, True, SYNC, max_iter=1, opts={"table": table, "wave_max": 128})
        assert w["labels"][0] == repeated and (s["overflowed"] > 0) == (table < 300)


@pytest.mark.parametrize("rows", [32, 33, 256, 257, 513, 100000])
def test_movers_with_long_rows(gpu_ctx, rows):
    """two stars joined at their centres, whose rows have exactly `rows` entries.  Synchronously both centres move in iteration 0:
    a row of up to 32 entries is marked by its lane, a longer one goes out as (vertex, segment) items of 256 -- one item, two,
    many -- for a MARK launch, which the kinds show"""
    ro, ci = cases.joined_stars(rows)
    w, s = _check(gpu_ctx, ro, ci, True, SYNC, max_iter=9)
    assert (model.MARK in w["kinds"]) == (rows > 32)
    _check(gpu_ctx, ro, ci, True, LAZY, max_iter=30)
    w, s = _check(gpu_ctx, ro, ci, False, SYNC, max_iter=5)      # both rows of a centre: twice the entries
    assert model.MARK in w["kinds"]


@pytest.mark.parametrize("ro_ci", [cases.sym(2, [0], [1]), cases.star(5000)])
def test_synchronous_runs_that_do_not_converge(gpu_ctx, ro_ci):
    n = len(ro_ci[0]) - 1
    w, s = _check(gpu_ctx, *ro_ci, True, SYNC, max_iter=7)
    assert s["converged"] == 0 and s["iterations"] == 7 and s["unstable"] == n
    w, s = _check(gpu_ctx, *ro_ci, True, LAZY)
    assert s["converged"] == 1 and s["communities"] == 1


def test_max_iter_zero(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.random_symmetric(300, 600, 1), True, LAZY, max_iter=0)
    assert np.array_equal(w["labels"], np.arange(300)) and s["converged"] == 0 and s["iterations"] == 0 and s["unstable"] > 0
    w, s = _check(gpu_ctx, *cases.empty(300), True, LAZY, max_iter=0)
    assert s["converged"] == 1


def test_path_has_a_long_list_tail(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.path(5000), True, LAZY)
    assert s["converged"] == 1 and s["iterations"] >= 10 and s["communities"] > 1000
    assert w["kinds"].count(model.EVAL_LIST) >= 8 and s["evaluated"] < 5000 * (s["iterations"] + 1) // 2
    _check(gpu_ctx, *cases.grid(64, 64), True, LAZY)


@pytest.mark.parametrize("div", [0, 1, 3])
def test_forced_iteration_kinds(gpu_ctx, monkeypatch, div):
    """all DENSE, all LIST, a cut of its own: the same labels and trace (the model's are the same by construction)"""
    monkeypatch.setenv("MGX_LPA_LIST_DIV", str(div))
    ro, ci = cases.random_symmetric(4000, 10000, 12)
    w, s = _check(gpu_ctx, ro, ci, True, LAZY, opts={"list_div": div})
    base = model.propagate(ro, ci, True, LAZY)
    assert np.array_equal(w["labels"], base["labels"]) and w["trace"] == base["trace"]
    if div == 0:
        assert model.EVAL_LIST not in w["kinds"] and s["evaluated"] == 4000 * (s["iterations"] + 1)
    if div == 1:
        assert model.EVAL_DENSE not in w["kinds"] and s["evaluated"] == sum(w["active"])
    _check(gpu_ctx, *cases.random_digraph(4000, 10000, 13), False, LAZY, opts={"list_div": div})


@pytest.mark.parametrize("mode", [SYNC, LAZY])
def test_planted_blocks(gpu_ctx, mode):
    for seed in PLANTED_SEEDS[mode]:
        ro, ci, block = cases.planted_blocks(seed)
        w, s = _check(gpu_ctx, ro, ci, True, mode)
        assert s["communities"] == 40 and s["largest"] == 50 and cases.same_partition(w["labels"], block)


def test_two_seeds_two_equilibria(gpu_ctx):
    ro, ci = cases.random_symmetric(3000, 9000, 5)
    a, _ = _check(gpu_ctx, ro, ci, True, LAZY, seed=1)
    b, _ = _check(gpu_ctx, ro, ci, True, LAZY, seed=2)
    assert not np.array_equal(a["labels"], b["labels"])
    assert model.is_equilibrium(ro, ci, True, a["labels"]) and model.is_equilibrium(ro, ci, True, b["labels"])


@pytest.mark.parametrize("scale,ef", [(10, 8), (12, 8), (14, 8), (16, 16)])
def test_rmat_symmetric(gpu_ctx, oracle, scale, ef):
    """fused == model; up to RMAT-14 the operator path as well"""
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 200, undir=True)
    w, s = _check(gpu_ctx, ro, ci, True, LAZY, operator=scale <= 14)
    assert s["converged"] == 1 and s["evaluated"] < n * (s["iterations"] + 1)


def test_rmat14_directed(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 214, undir=False)
    w, s = _check(gpu_ctx, ro, ci, False, LAZY)
    assert s["converged"] == 1
    _check(gpu_ctx, ro, ci, False, SYNC, max_iter=6, csc="upload")


def test_modularity_of_other_labellings(gpu_ctx, oracle):
    import mini_amd
    ro, ci, block = cases.planted_blocks(0)
    n = len(ro) - 1
    rng = np.random.default_rng(4)
    g = _graph(gpu_ctx, ro, ci, "build")
    cp = mini_amd.CcProblem(g)
    cp.run()
    labellings = [cp.labels(), block.astype(np.int32), rng.integers(0, n, n).astype(np.int32), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)]
    for labels in labellings:
        for symmetric in (True, False):
            q, s_in, s_sq, w = mini_amd.modularity(g, labels, symmetric)
            mq, m_in, m_sq, m_w = model.modularity(ro, ci, labels, symmetric)
            assert (s_in, s_sq, w) == (m_in, m_sq, m_w) and abs(q - float(mq)) <= 1e-12
    assert mini_amd.modularity(g, labellings[1], True)[0] > 0.5 and mini_amd.modularity(g, labellings[3], True)[0] == 0.0
    bad = labellings[2].copy()
    bad[n // 2] = n
    for wrong in (bad, np.full(n, -1, np.int32)):
        with pytest.raises(mini_amd.MgxError) as err:
            mini_amd.modularity(g, wrong, True)
        assert err.value.status == mini_amd.MGX_E_INVALID
    cp.close()
    g.close()
    g = _graph(gpu_ctx, ro, ci)                                  # without a CSC: symmetric = 0 is refused
    with pytest.raises(mini_amd.MgxError) as err:
        mini_amd.modularity(g, labellings[1], False)
    assert err.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(err.value)
    g.close()
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 212, undir=False)      # long rows on both sides
    g = _graph(gpu_ctx, ro, ci, "build")
    labels = rng.integers(0, 50, n).astype(np.int32)
    for symmetric in (True, False):
        assert mini_amd.modularity(g, labels, symmetric)[1:] == model.modularity(ro, ci, labels, symmetric)[1:]
    g.close()


def test_lifecycle(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_digraph(400, 900, 9)
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LpaProblem(g)
    getters = (lp.labels, lp.labels_device_ptr, lp.trace, lp.step_kinds, lp.bins, lp.phase_ms)
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
    for go in (lp.run, lp.enact):                                # symmetric = 0 without a CSC; bad arguments
        with pytest.raises(mini_amd.MgxError) as err:
            go(symmetric=False)
        assert err.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(err.value)
        for bad in (dict(mode=2), dict(mode=-1), dict(max_iter=-1), dict(max_iter=(1 << 20) + 1)):
            with pytest.raises(mini_amd.MgxError) as err:
                go(symmetric=True, **bad)
            assert err.value.status == mini_amd.MGX_E_INVALID
    lp.run(symmetric=True)
    assert lp.labels_device_ptr()
    with pytest.raises(mini_amd.MgxError):
        lp.run(symmetric=False)                                  # a failed run leaves nothing to the getters
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert "no run yet" in str(err.value)
    lp.run(symmetric=True)
    with pytest.raises(mini_amd.MgxError):
        lp.enact(symmetric=False)                                # a refused operator run leaves nothing either, of the fused run before it too
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert "no run yet" in str(err.value)
    g.build_csc()                                                # the handle is still usable
    want = model.propagate(ro, ci, False, LAZY)
    assert {k: v for k, v in lp.run().items() if k in KEYS} == want["stats"] and np.array_equal(lp.labels(), want["labels"])
    assert {k: v for k, v in lp.enact().items() if k in KEYS} == want["stats"] and np.array_equal(lp.labels(), want["labels"])
    lp.set_timing(True)
    lp.run()
    ms = lp.phase_ms()
    assert set(ms) == {"setup", "evaluate", "long_rows", "apply"} and all(v >= 0.0 for v in ms.values()) and ms["evaluate"] > 0.0
    lp.close()
    g.close()


def test_rmat12_on_one_compute_unit(monkeypatch, torch_mod, oracle, built):
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 112, undir=True)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, ro, ci, True, LAZY)
        _check(ctx, *cases.star(5000), True, LAZY)
