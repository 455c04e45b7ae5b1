"""GPU suite (-m gpu): bit-parallel multi-source BFS (mgx_msbfs_*).  The fused path (mgx_msbfs_run), the operator path
(mgx_msbfs_enact) and the numpy model (tests/msbfs_model.py) agree bit for bit -- depths, reach, far, ecc, harm, the per-vertex
sums -- on the golden fixtures, every source count round a batch's edge, rows at every cut between the bodies on the out- and on
the in-side, a star's hub pushed and pulled in segments, R-MAT 10 - 16, a path of 5 000 levels and a grid.  The fused path's
stats [0] - [5], [8], [9], its level kinds and its bins are the ones the model predicts, its host waits exact.  The operator
path always pushes: of its stats [0] - [3] and [9] are the model's, [4] is all the levels, [5] and [8] are 0.  It is compared up
to R-MAT-14."""
import os

import numpy as np
import pytest

from tests import cc_model, chain_model
from tests import msbfs_cases as cases
from tests import msbfs_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
READ_BACK_WAITS = 1           # the wait for the per-source results, behind the batches'
ALWAYS = 1 << 30
ENV = {"short_max": "MGX_MSBFS_SHORT_MAX", "wave_max": "MGX_MSBFS_WAVE_MAX", "seg": "MGX_MSBFS_SEG", "pull_div": "MGX_MSBFS_PULL_DIV"}


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(ENV[k], str(v))


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


def _same_results(mp, w, who, depths=True):
    n = mp.graph.num_nodes
    if depths:
        d = mp.depths()
        assert d.dtype == np.int32 and d.shape == w["depths"].shape
        assert np.array_equal(d, w["depths"]), "%s: %d depths differ" % (who, int((d != w["depths"]).sum()))
    assert np.array_equal(mp.reach(), w["reach"]), who
    assert np.array_equal(mp.farness(), w["far"]), who
    assert np.array_equal(mp.eccentricity(), w["ecc"]), who
    h = mp.harmonic()
    assert h.dtype == np.float64 and np.array_equal(h, w["harm"]), who                # bit for bit: the additions' order is fixed
    assert np.array_equal(mp.closeness(), model.closeness(w["reach"], w["far"], n)), who
    r, f = mp.vertex_sums()
    assert np.array_equal(r, w["reach_in"]) and np.array_equal(f, w["far_in"]), who


def _check(ctx, ro, ci, sources=None, symmetric=True, csc=None, layout=False, operator=True, opts=None, depths=True, operator_first=False,
           want=None):
    """fused == operator path == model; the repeat run; the host waits; the kinds and the bins as the model predicts them.
    opts: the switches the handle reads, for the model; want: the model's result where the caller has it."""
    import mini_amd
    opts = opts or {}
    w = model.traverse(ro, ci, sources, symmetric, csc is not None, depths=depths, **opts) if want is None else want
    g = _graph(ctx, ro, ci, csc, layout)
    mp = mini_amd.MsBfsProblem(g)
    args = dict(sources=sources, symmetric=symmetric, depths=depths)
    if operator_first:
        so = mp.enact(**args)
        _same_results(mp, w, "operator path first", depths)
    s1 = mp.run(**args)
    print("fused", s1)
    _same_results(mp, w, "fused", depths)
    assert {k: s1[k] for k in KEYS} == w["stats"], (s1, w["stats"])
    ran = s1["batches"] > 0
    # the launches the model predicts end the run: the host enqueues whole batches up to the one that holds the DONE, and no more
    waits, launches = chain_model.waits_and_launches(w["launches"]) if ran else (0, 0)
    assert w["launches"] == (2 * s1["batches"] + 2 * len(w["kinds"]) + sum(w["long"]) + 1 if ran else 0)
    assert s1["launches"] == launches and s1["host_waits"] == (waits + READ_BACK_WAITS if ran else 0), (s1, w["launches"], launches, waits)
    kinds = mp.level_kinds()
    want_kinds = w["kinds"][:chain_model.LOG_CAP].tolist()       # (the log keeps a run's first 2^16 levels)
    assert kinds.tolist() == want_kinds, (kinds.tolist()[:40], want_kinds[:40], w["e"][:40])
    b = mp.bins()
    for side, want in (("out", w["bins_out"]), ("in", w["bins_in"])):
        assert {k: b[side + "_" + k] for k in model.BIN_KEYS} == want, (side, b, want)
    sm = opts.get("short_max", model.SHORT_MAX)
    assert (b["short_max"], b["wave_max"], b["seg"], b["pull_div"]) == (sm, max(opts.get("wave_max", model.WAVE_MAX), sm),
                                                                      opts.get("seg", model.SEG), opts.get("pull_div", model.PULL_DIV))
    s2 = mp.run(**args)
    assert s2 == s1, (s1, s2)                                    # a repeat run: the same launches, the same waits
    _same_results(mp, w, "fused, repeated", depths)
    assert mp.level_kinds().tolist() == kinds.tolist() and mp.bins() == b
    if operator:
        so = mp.enact(**args)
        print("operator", so)
        _same_results(mp, w, "operator path", depths)
        for k in ("sources", "batches", "deepest", "reach", "depths"):
            assert so[k] == w["stats"][k], (k, so, w["stats"])
        assert so["push_levels"] == len(w["kinds"]) and so["pull_levels"] == 0 and so["csc"] == 0
        assert so["host_waits"] >= so["push_levels"]
    mp.close()
    g.close()
    return w, s1


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(gpu_ctx, oracle, name):
    """all vertices as sources; symmetric = 1 on the symmetrised fixture, symmetric = 0 on the directed one with the CSC built,
    uploaded and without one (every level pushes), with an attached layout, which is ignored"""
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=True)
    w, s = _check(gpu_ctx, ro, ci, None, True)
    assert s["csc"] == 0
    for src in range(0, n, max(n // 7, 1)):
        assert np.array_equal(w["depths"][src], oracle.bfs_cpu(ro, ci, src))
    _check(gpu_ctx, ro, ci, None, False)                          # the caller does not say so: push only
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=False)
    w, s = _check(gpu_ctx, ro, ci, None, False, csc="build")
    assert s["csc"] == 1
    _check(gpu_ctx, ro, ci, None, False, csc="upload", layout=True)
    w, s = _check(gpu_ctx, ro, ci, None, False, csc=None)
    assert s["csc"] == 0 and s["pull_levels"] == 0 and s["push_levels"] > 0
    for src in range(0, n, max(n // 7, 1)):
        assert np.array_equal(w["depths"][src], oracle.bfs_cpu(ro, ci, src))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129])
def test_source_counts_round_a_batch(gpu_ctx, count):
    """a source in bit 63, a partial last batch, the hand-over from batch to batch on the device"""
    ro, ci = cases.random_digraph(200, 700, 21)
    sources = np.random.default_rng(count).integers(0, 200, count)
    w, s = _check(gpu_ctx, ro, ci, sources, False, csc="build")
    assert s["batches"] == (count + 63) // 64
    _check(gpu_ctx, *cases.random_symmetric(200, 400, 22), sources, True)


def test_duplicate_isolated_and_all_sources(gpu_ctx):
    ro, ci = cases.with_isolated(*cases.random_symmetric(150, 300, 23), 10)
    w, s = _check(gpu_ctx, ro, ci, [5, 5, 155, 9, 5, 155], True)
    assert np.array_equal(w["depths"][0], w["depths"][1]) and np.array_equal(w["depths"][0], w["depths"][4])
    assert w["reach"][2] == 0 and w["ecc"][2] == 0 and w["harm"][2] == 0.0
    w, s = _check(gpu_ctx, ro, ci, [155], True)
    assert s["reach"] == 0 and s["deepest"] == 1
    w, s = _check(gpu_ctx, ro, ci, None, True)
    assert s["sources"] == 160 and s["batches"] == 3
    assert np.array_equal(w["far"], w["far_in"]) and np.array_equal(w["reach"], w["reach_in"])


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    for ro, ci in (cases.empty(n), cases.directed(n, np.arange(n), np.arange(n))):          # (and self-loops only)
        for symmetric in (True, False):
            w, s = _check(gpu_ctx, ro, ci, None, symmetric)
            assert s["reach"] == 0 and s["deepest"] == 1 and s["batches"] == (n + 63) // 64


def test_no_sources_and_statuses(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_symmetric(100, 200, 24)
    w, s = _check(gpu_ctx, ro, ci, [], True)
    assert s["sources"] == 0 and s["batches"] == 0 and s["launches"] == 0 and s["host_waits"] == 0
    g = _graph(gpu_ctx, ro, ci)
    mp = mini_amd.MsBfsProblem(g)
    mp.run([1, 2], True)
    for go in (mp.run, mp.enact):
        for bad in ([100], [-1], [3, 4, 1000]):
            with pytest.raises(mini_amd.MgxError) as err:
                go(bad, True)
            assert err.value.status == mini_amd.MGX_E_INVALID
    one = np.zeros(1, dtype=np.int32)
    assert mini_amd.lib.mgx_msbfs_run(mp._h, one.ctypes.data, -1, 1, 0, None) == mini_amd.MGX_E_INVALID
    assert mini_amd.lib.mgx_msbfs_enact(mp._h, one.ctypes.data, -1, 1, 0, None) == mini_amd.MGX_E_INVALID
    with pytest.raises(mini_amd.MgxError):                       # a refused run leaves nothing to the getters
        mp.reach()
    mp.close()
    g.close()


CUTS = [{}, {"short_max": 4, "wave_max": 10, "seg": 16}, {"short_max": 0, "wave_max": 0, "seg": 5}, {"short_max": 0, "wave_max": 70, "seg": 64}]


@pytest.mark.parametrize("opts", CUTS)
@pytest.mark.parametrize("div", [0, ALWAYS])
def test_rows_at_every_cut(gpu_ctx, monkeypatch, opts, div):
    """hubs whose out-rows and sinks whose in-rows have one entry fewer than, exactly and one entry more than short_max, wave_max,
    one segment and two segments: forced PUSH meets the out-rows, forced PULL the in-rows; at the defaults and at small forced cuts"""
    opts = dict(opts, pull_div=div)
    _setenv(monkeypatch, opts)
    sm, wm, seg = opts.get("short_max", model.SHORT_MAX), opts.get("wave_max", model.WAVE_MAX), opts.get("seg", model.SEG)
    ro, ci, root, hubs, sinks = cases.fans(cases.cuts(max(sm, 1), max(wm, sm, 1), seg))
    w, s = _check(gpu_ctx, ro, ci, [root, hubs[0], sinks[-1], root], False, csc="upload", opts=opts)
    if div == 0:
        assert s["pull_levels"] == 0
    else:                                                        # (a front without out-entries has e_t = 0: 0 x DIV >= m never holds)
        assert s["pull_levels"] > 0 and all(k == model.PULL or e == 0 for k, e in zip(w["kinds"].tolist(), w["e"]))
    assert w["bins_out"]["long"] >= 3 and w["bins_in"]["long"] >= 3 and (w["depths"][0][sinks] == 3).all()
    _check(gpu_ctx, *cases.random_symmetric(500, 3000, 8), np.arange(70), True, opts=opts)


@pytest.mark.parametrize("div", [0, ALWAYS, model.PULL_DIV])
def test_star_of_100000_leaves(gpu_ctx, monkeypatch, div):
    """the centre as a source and a leaf as a source: the hub's row pushed as items, and pulled in segments that meet in next"""
    monkeypatch.setenv("MGX_MSBFS_PULL_DIV", str(div))
    ro, ci = cases.star(100000)
    w, s = _check(gpu_ctx, ro, ci, [0, 77, 100000], True, opts={"pull_div": div}, operator=div == 0)
    assert w["ecc"].tolist() == [1, 2, 2] and w["bins_out"]["long"] == 1 and w["bins_out"]["segments"] == -(-100000 // model.SEG)
    w, s = _check(gpu_ctx, ro, ci, [5], True, opts={"pull_div": div}, operator=False)
    assert w["far"][0] == 1 + 2 * 99999


@pytest.mark.parametrize("scale", [10, 12, 14, 16])
@pytest.mark.parametrize("div", [0, ALWAYS, model.PULL_DIV])
def test_rmat_symmetric(gpu_ctx, oracle, monkeypatch, scale, div):
    """all PUSH, all PULL and the default rule: the kinds are the model's; up to RMAT-14 the operator path as well"""
    monkeypatch.setenv("MGX_MSBFS_PULL_DIV", str(div))
    n, ro, ci, _ = oracle.rmat_csr(scale, 16, scale + 300, undir=True)
    sources = np.random.default_rng(scale).choice(np.flatnonzero(np.diff(ro) > 0), 64, replace=False)
    w, s = _check(gpu_ctx, ro, ci, sources, True, opts={"pull_div": div}, operator=scale <= 14 and div == model.PULL_DIV)
    if div == model.PULL_DIV:
        assert s["push_levels"] > 0 and s["pull_levels"] > 0
    else:
        assert (s["pull_levels"] == 0) if div == 0 else (s["push_levels"] == 0)


@pytest.mark.parametrize("div", [0, ALWAYS, model.PULL_DIV])
def test_rmat14_directed(gpu_ctx, oracle, monkeypatch, div):
    monkeypatch.setenv("MGX_MSBFS_PULL_DIV", str(div))
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 314, undir=False)
    sources = np.random.default_rng(14).choice(np.flatnonzero(np.diff(ro) > 0), 100, replace=False)
    w, s = _check(gpu_ctx, ro, ci, sources, False, csc="build", opts={"pull_div": div}, operator=div == 0)
    assert s["csc"] == 1 and ((s["pull_levels"] > 0) == (div != 0))
    if div == model.PULL_DIV:
        w, s = _check(gpu_ctx, ro, ci, sources, False, csc=None, opts={"pull_div": div}, operator=False)
        assert s["pull_levels"] == 0


def test_path_of_5000_levels(gpu_ctx):
    """two sources at the path's ends: 5 000 levels, the chain's batches of launches grow to 256"""
    w, s = _check(gpu_ctx, *cases.path(5000), [0, 4999], True)
    assert s["deepest"] == 5000 and s["launches"] >= 10000 and s["host_waits"] > 30
    assert w["far"].tolist() == [5000 * 4999 // 2] * 2


def test_grid(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.grid(64, 64), [0, 64 * 64 - 1, 32 * 64 + 32] + list(range(100, 170)), True)
    assert w["ecc"][:3].tolist() == [126, 126, 64]


def test_results_without_depths(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_symmetric(300, 900, 25)
    w, s = _check(gpu_ctx, ro, ci, np.arange(80), True, depths=False)
    assert s["depths"] == 0
    g = _graph(gpu_ctx, ro, ci)
    mp = mini_amd.MsBfsProblem(g)
    for go in (mp.run, mp.enact):
        go(np.arange(80), True, depths=True)
        assert mp.depths().shape == (80, 300)
        go(np.arange(80), True, depths=False)
        mp.reach()
        with pytest.raises(mini_amd.MgxError) as err:
            mp.depths()
        assert err.value.status == mini_amd.MGX_E_INVALID and "kept no depths" in str(err.value)
    mp.close()
    g.close()


def test_operator_path_first_on_a_fresh_handle(gpu_ctx):
    _check(gpu_ctx, *cases.random_symmetric(400, 1200, 26), np.arange(0, 400, 3), True, operator_first=True)
    _check(gpu_ctx, *cases.random_digraph(400, 1200, 27), None, False, csc="build", operator_first=True)


def test_another_stream(gpu_ctx, torch_mod):
    import mini_amd
    ro, ci = cases.random_symmetric(2000, 8000, 28)
    a, _ = _check(gpu_ctx, ro, ci, np.arange(100), True)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        b, _ = _check(ctx, ro, ci, np.arange(100), True)
        assert np.array_equal(a["depths"], b["depths"])
    finally:
        ctx.close()


def test_lifecycle(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_digraph(400, 1500, 29)
    g = _graph(gpu_ctx, ro, ci)
    mp = mini_amd.MsBfsProblem(g)
    getters = (mp.reach, mp.farness, mp.eccentricity, mp.harmonic, mp.closeness, mp.vertex_sums, mp.vertex_sums_device_ptrs, mp.depths,
               mp.level_kinds, mp.bins, mp.phase_ms)
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
    want = model.traverse(ro, ci, [3, 4], False, False)
    s = mp.run([3, 4], False, depths=True)                       # no CSC: valid, every level pushes
    assert s["csc"] == 0 and s["pull_levels"] == 0 and np.array_equal(mp.depths(), want["depths"])
    r, f = mp.vertex_sums_device_ptrs()
    assert r and f
    mp.enact([3, 4], False, depths=True)                         # after an operator run the fused run's kinds are gone
    for call in (mp.level_kinds, mp.bins, mp.phase_ms):
        with pytest.raises(mini_amd.MgxError):
            call()
    assert np.array_equal(mp.depths(), want["depths"])
    g.build_csc()                                                # the handle is still usable, and now it pulls
    want = model.traverse(ro, ci, None, False, True)
    s = mp.run(None, False, depths=True)
    assert s["csc"] == 1 and {k: s[k] for k in KEYS} == want["stats"] and np.array_equal(mp.depths(), want["depths"])
    mp.set_timing(True)
    mp.run(None, False)
    ms = mp.phase_ms()
    assert set(ms) == {"push", "pull", "long_rows", "finalize"} and all(v >= 0.0 for v in ms.values()) and ms["finalize"] > 0.0
    mp.close()
    mp.close()
    g.close()


def test_rmat12_on_one_compute_unit(monkeypatch, torch_mod, oracle, built):
    n, ro, ci, _ = oracle.rmat_csr(12, 16, 312, undir=True)
    sources = np.random.default_rng(12).choice(np.flatnonzero(np.diff(ro) > 0), 130, replace=False)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, ro, ci, sources, True)
        _check(ctx, *cases.star(5000), [0, 1], True)
