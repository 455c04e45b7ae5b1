"""GPU suite (-m gpu): random walks and node2vec sampling (mgx_rw_*).  The fused path (mgx_rw_run), the operator path
(mgx_rw_enact) and the numpy model (tests/rw_model.py) agree bit for bit -- paths, ends, lengths, visits, the eight model stats and
the bins -- on the golden fixtures in all four instantiations with and without restarts, walker counts round the wave and the
workgroup, the grid-stride loop, every path length round the tile for three tile sizes with dead ends at a tile's edges, rows of
degree 0, 1, 2 and 100 000, rows at every cut of the setup's maximum, the membership search at its edges on ascending and on
descending rows, forced fallbacks, and R-MAT 10 - 16.  The fused path's launches and host waits are exact; a repeat run gives the
same with the setup's launches and waits gone."""
import os

import numpy as np
import pytest

from tests import rw_cases as cases
from tests import rw_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
ENV = {"tries": "MGX_RW_TRIES", "tile": "MGX_RW_TILE", "short_max": "MGX_RW_SHORT_MAX", "wave_max": "MGX_RW_WAVE_MAX", "seg": "MGX_RW_SEG"}
FOUR = [dict(), dict(weighted=True), dict(p=0.25, q=4.0), dict(weighted=True, p=2.0, q=0.5)]


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(ENV[k], str(v))


def _same_results(rp, w, who, paths, visits):
    import mini_amd
    if paths:
        p = rp.paths()
        assert p.dtype == np.int32 and p.shape == w["paths"].shape
        assert np.array_equal(p, w["paths"]), "%s: %d path slots differ" % (who, int((p != w["paths"]).sum()))
    else:
        with pytest.raises(mini_amd.MgxError) as err:
            rp.paths()
        assert err.value.status == mini_amd.MGX_E_INVALID and "kept no paths" in str(err.value)
    assert np.array_equal(rp.ends(), w["ends"]), who
    assert np.array_equal(rp.lengths(), w["lengths"]), who
    if visits:
        v = rp.visits()
        assert v.dtype == np.int64 and np.array_equal(v, w["visits"]), who
        total = w["visits"].sum()
        assert np.array_equal(rp.ppr(), w["visits"] / total if total else w["visits"].astype(np.float64)), who
    else:
        with pytest.raises(mini_amd.MgxError) as err:
            rp.visits()
        assert err.value.status == mini_amd.MGX_E_INVALID and "kept no visits" in str(err.value)


def _check(ctx, ro, ci, w=None, starts=None, operator=True, opts=None, paths=True, visits=True, operator_first=False, **mode):
    """fused == operator path == model; the repeat run; launches and host waits; the bins.  opts: the switches the handle reads."""
    import mini_amd
    opts = opts or {}
    mopts = {k: v for k, v in opts.items() if k != "tile"}
    want = model.walk(ro, ci, w, starts, **mode, **mopts)
    n, W = len(ro) - 1, want["stats"]["walkers"]
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    rp = mini_amd.RandomWalkProblem(g)
    args = dict(mode, starts=starts, paths=paths, visits=visits)
    ran = n > 0 and W > 0
    setup = want["setup"] and ran
    if operator_first:
        so = rp.enact(**args)
        _same_results(rp, want, "operator path first", paths, visits)
        assert {k: so[k] for k in KEYS} == want["stats"], (so, want["stats"])
        setup = False
    s1 = rp.run(**args)
    print("fused", s1)
    _same_results(rp, want, "fused", paths, visits)
    assert {k: s1[k] for k in KEYS} == want["stats"], (s1, want["stats"])
    sort = setup and want["stats"]["sorted_copy"]
    assert (s1["launches"], s1["host_waits"]) == model.fused_counts(W, n, starts is not None, setup, sort), s1
    b = rp.bins()
    rows = want["bins"] if (want["setup"] and ran) else dict.fromkeys(model.BIN_KEYS, 0)
    assert {k: b[k] for k in model.BIN_KEYS} == rows, (b, rows)
    sm = opts.get("short_max", model.SHORT_MAX)
    assert (b["short_max"], b["wave_max"], b["seg"], b["tries"], b["tile"]) == (
        sm, max(opts.get("wave_max", model.WAVE_MAX), sm), opts.get("seg", model.SEG), opts.get("tries", model.TRIES), opts.get("tile", model.TILE))
    s2 = rp.run(**args)                                          # a repeat run: the setup is there
    assert {k: s2[k] for k in KEYS} == want["stats"], (s2, want["stats"])
    assert (s2["launches"], s2["host_waits"]) == model.fused_counts(W, n, starts is not None, False, False), s2
    _same_results(rp, want, "fused, repeated", paths, visits)
    assert rp.bins() == b
    if operator:
        so = rp.enact(**args)
        print("operator", so)
        _same_results(rp, want, "operator path", paths, visits)
        assert {k: so[k] for k in KEYS} == want["stats"], (so, want["stats"])
        assert so["host_waits"] >= min(int(want["lengths"].max(initial=0)), want["stats"]["length"])
    rp.close()
    g.close()
    return want, s1


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("restart", [0.0, 0.15])
def test_fixtures(gpu_ctx, oracle, name, restart):
    """every vertex a start, two walks each, the fixtures' own weights: the four instantiations on the symmetrised and on the
    directed fixture"""
    for undir in (True, False):
        n, ro, ci, w, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
        for mode in FOUR:
            want, s = _check(gpu_ctx, ro, ci, w, None, length=12, walks_per_start=2, seed=5, restart=restart, **mode)
            assert (s["restarts"] > 0) == (restart > 0 and s["steps"] > 0)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_walker_counts_round_the_wave_and_the_workgroup(gpu_ctx, count):
    ro, ci = cases.random_digraph(300, 1500, 31)
    starts = np.random.default_rng(count).integers(0, 300, count)
    _check(gpu_ctx, ro, ci, cases.weights(ci, 32), starts, length=20, seed=count, weighted=True, p=0.5, q=2.0)
    _check(gpu_ctx, ro, ci, None, starts, length=20, seed=count, operator=False)


def test_grid_stride_loop_on_one_compute_unit(monkeypatch, torch_mod, built):
    """8 workgroups: 5 000 walkers are 20 blocks of 256, every workgroup runs its loop two or three times, the last block partly"""
    ro, ci = cases.random_symmetric(1000, 5000, 33)
    w = cases.weights(ci, 34)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, ro, ci, w, None, length=17, walks_per_start=5, seed=1, weighted=True, p=0.5, q=2.0, restart=0.05)
        _check(ctx, ro, ci, None, np.arange(0, 1000, 3), length=40, walks_per_start=9, seed=2, paths=False)


@pytest.mark.parametrize("tile", [1, 4, 16])
def test_path_lengths_round_the_tile(gpu_ctx, monkeypatch, tile):
    """length + 1 in {1, 2, TILE - 1, TILE, TILE + 1, 2 TILE, 2 TILE + 1}; on the path into a sink the walks from vertex k end after
    n - 1 - k steps, so dead ends fall on every slot of a tile, its first and its last included, and the -1 padding crosses flushes"""
    _setenv(monkeypatch, {"tile": tile})
    n = 2 * tile + 6
    ro, ci = cases.directed(n, np.arange(n - 1), np.arange(1, n))              # 0 -> 1 -> ... -> n - 1
    rnd = cases.random_symmetric(300, 900, 35)
    for slots in sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1} - {0}):
        want, s = _check(gpu_ctx, ro, ci, None, None, opts={"tile": tile}, length=slots - 1, walks_per_start=2, seed=slots)
        assert want["lengths"].tolist() == np.repeat(np.minimum(n - 1 - np.arange(n), slots - 1), 2).tolist()
        _check(gpu_ctx, *rnd, None, None, opts={"tile": tile}, operator=False, length=slots - 1, seed=slots, p=0.5, q=2.0)


@pytest.mark.parametrize("paths, visits", [(False, True), (True, False), (False, False)])
def test_results_on_request(gpu_ctx, paths, visits):
    ro, ci = cases.with_isolated(*cases.random_symmetric(400, 1600, 36), 7)
    _check(gpu_ctx, ro, ci, cases.weights(ci, 37), None, paths=paths, visits=visits, length=33, walks_per_start=3, seed=9, weighted=True, restart=0.15)
    _check(gpu_ctx, ro, ci, None, None, paths=paths, visits=visits, length=33, seed=9)


def test_rows_of_degree_0_1_2(gpu_ctx):
    """an isolated start, a sink reached mid-walk, rows of one and of two entries"""
    #   0 -> 1 -> 2 (sink);  3 -> {4, 5};  4 -> 3;  5 -> 2;  6 isolated
    ro, ci = cases.directed(7, np.array([0, 1, 3, 3, 4, 5]), np.array([1, 2, 4, 5, 3, 2]))
    for mode in FOUR:
        want, s = _check(gpu_ctx, ro, ci, np.array([1.0, 1.0, 2.0, 1.0, 1.0, 3.0], dtype=np.float32), None, length=9, walks_per_start=40, seed=3, **mode)
        assert (want["lengths"][6 * 40:] == 0).all() and (want["lengths"][:40] == 2).all() and s["dead_ends"] > 6 * 40 // 2
        _check(gpu_ctx, ro, ci, None, [6, 0, 3], length=9, walks_per_start=3, seed=4, restart=0.3, **mode)


def test_star_of_100000_leaves(gpu_ctx):
    """umulhi over a long row from the centre; the setup's maximum over its 98 segments"""
    ro, ci = cases.star(100000)
    w = cases.weights(ci, 38)
    starts = np.concatenate([np.zeros(3000, dtype=np.int64), [5, 99999, 100000]])
    want, s = _check(gpu_ctx, ro, ci, w, starts, length=4, seed=6, weighted=True)
    assert want["bins"]["long"] == 1 and want["bins"]["segments"] == -(-100000 // model.SEG)
    assert len(np.unique(want["paths"][:3000, 1])) > 2900 and want["paths"][:3000, 1].max() > 99000
    _check(gpu_ctx, ro, ci, None, starts, length=4, seed=6, p=0.5, q=2.0, operator=False)


CUTS = [{}, {"short_max": 4, "wave_max": 10, "seg": 16}, {"short_max": 0, "wave_max": 0, "seg": 5}, {"short_max": 0, "wave_max": 70, "seg": 64}]


@pytest.mark.parametrize("opts", CUTS)
@pytest.mark.parametrize("place", ["first", "last", "twice", "random"])
def test_row_maximum_at_every_cut(gpu_ctx, monkeypatch, opts, place):
    """hubs whose rows have one entry fewer than, exactly and one more than short_max, wave_max, one segment and two segments; the
    maximum first, last, or twice (amax is the first); TRIES = 1 and a maximum of 1000 among weights below 1 make nearly every step
    from a hub a fallback to amax"""
    opts = dict(opts, tries=1)
    _setenv(monkeypatch, opts)
    sm, wm, seg = opts.get("short_max", model.SHORT_MAX), opts.get("wave_max", model.WAVE_MAX), opts.get("seg", model.SEG)
    ro, ci, root, hubs, sinks = cases.fans(cases.cuts(max(sm, 1), max(wm, sm, 1), seg))
    rng = np.random.default_rng(39)
    w = (rng.integers(1, 8, len(ci)) / 8.0).astype(np.float32)
    for h in hubs:
        lo, hi = ro[h], ro[h + 1]
        at = {"first": [lo], "last": [hi - 1], "twice": [lo + (hi - lo) // 3, hi - 1], "random": [rng.integers(lo, hi)]}[place]
        w[at] = 1000.0
    want, s = _check(gpu_ctx, ro, ci, w, np.array(hubs), opts=opts, length=2, walks_per_start=8, seed=40, weighted=True)
    assert s["fallbacks"] > 4 * len(hubs) and want["bins"]["long"] >= 3
    wmax, amax = model.row_maxima(ro, w)
    fell = want["paths"][:, 1] == ci[ro[np.repeat(hubs, 8)] + amax[np.repeat(hubs, 8)]]
    assert fell.sum() >= s["fallbacks"]                          # (a leaf's row of one entry accepts at once: every fallback is a hub's)


def test_negative_and_nan_weights(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_symmetric(200, 3000, 41)
    for bad in (-1.0, float("nan")):
        w = cases.weights(ci, 42)
        w[len(w) // 2] = bad
        g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
        rp = mini_amd.RandomWalkProblem(g)
        for go in (rp.run, rp.enact):
            with pytest.raises(mini_amd.MgxError) as err:
                go(None, length=5, weighted=True)
            assert err.value.status == mini_amd.MGX_E_NEGATIVE_WEIGHT
            with pytest.raises(mini_amd.MgxError):                   # a refused run leaves nothing to the getters
                rp.ends()
        rp.run(None, length=5, p=2.0)                                # an unweighted run does not read them
        assert np.array_equal(rp.paths(), model.walk(ro, ci, None, None, length=5, p=2.0)["paths"])
        rp.close()
        g.close()


@pytest.mark.parametrize("desc", [False, True])
def test_membership_search(gpu_ctx, desc):
    """prev rows of 1, 2, 3, 2^k - 1, 2^k, 2^k + 1 entries with duplicates; candidates below all, above all, first, last, absent
    between two entries and prev itself; the same graph with descending rows walks on a sorted copy"""
    ro, ci, hubs = cases.prev_rows([1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129])
    w = cases.weights(ci, 43)
    if desc:
        ro, ci, w = cases.descending(ro, ci, w)
    for mode in (dict(p=0.25, q=4.0), dict(weighted=True, p=4.0, q=0.25)):
        want, s = _check(gpu_ctx, ro, ci, w, np.array(hubs), length=6, walks_per_start=60, seed=44, **mode)
        assert s["sorted_copy"] == int(desc) and s["tries"] > s["steps"]
    want, s = _check(gpu_ctx, ro, ci, w, np.array(hubs), length=6, walks_per_start=60, seed=44, operator_first=True, p=0.25, q=4.0)
    assert s["sorted_copy"] == int(desc)
    want, s = _check(gpu_ctx, ro, ci, w, np.array(hubs), length=6, seed=44, operator=False)         # first order: no check, no copy
    assert s["sorted_copy"] == 0


@pytest.mark.parametrize("tries", [1, 2])
def test_fallbacks_are_counted(gpu_ctx, monkeypatch, tries):
    _setenv(monkeypatch, {"tries": tries})
    ro, ci, w = cases.one_row([1.0, 1000.0, 1.0, 1.0, 1000.0, 1.0])
    for mode in (dict(weighted=True), dict(weighted=True, p=0.5, q=2.0), dict(p=0.01, q=100.0)):
        want, s = _check(gpu_ctx, ro, ci, w, [0], opts={"tries": tries}, length=8, walks_per_start=500, seed=45, **mode)
        assert s["fallbacks"] > 100 and s["tries"] <= tries * s["steps"]


@pytest.mark.parametrize("scale", [10, 12, 14, 16])
@pytest.mark.parametrize("undir", [True, False])
def test_rmat(gpu_ctx, oracle, scale, undir):
    """weighted, one walk per vertex, L = 20: the four instantiations; the operator path up to R-MAT-14"""
    n, ro, ci, w = oracle.rmat_csr(scale, 16, scale + 400, undir=undir)
    for mode in (FOUR if scale <= 12 else [dict(), dict(weighted=True, p=2.0, q=0.5)]):
        _check(gpu_ctx, ro, ci, w, None, operator=scale <= 14, length=20, seed=scale, **mode)
    if scale == 10:
        _check(gpu_ctx, ro, ci, w, None, length=20, walks_per_start=3, seed=scale, weighted=True, p=0.5, q=2.0, restart=0.15)


def test_empty_runs_and_statuses(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_symmetric(100, 300, 46)
    want, s = _check(gpu_ctx, ro, ci, None, [], length=5)
    assert s["walkers"] == 0 and s["launches"] == 0 and s["host_waits"] == 0
    _check(gpu_ctx, *cases.empty(50), None, None, length=5, restart=0.5, p=2.0)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    rp = mini_amd.RandomWalkProblem(g)
    for call in (rp.paths, rp.ends, rp.lengths, rp.visits, rp.ppr, rp.paths_device_ptr, rp.visits_device_ptr, rp.bins, rp.phase_ms):
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
    rp.run([1, 2], length=3, visits=True)
    assert rp.paths_device_ptr() and rp.visits_device_ptr()
    for go in (rp.run, rp.enact):
        for bad in ([100], [-1], [3, 4, 1000]):
            with pytest.raises(mini_amd.MgxError) as err:
                go(bad, length=3)
            assert err.value.status == mini_amd.MGX_E_INVALID
        for bad in (dict(length=-1), dict(walks_per_start=0), dict(p=0.0), dict(q=-2.0), dict(p=float("inf")), dict(restart=1.0), dict(restart=-0.1)):
            with pytest.raises(mini_amd.MgxError) as err:
                go([1], **bad)
            assert err.value.status == mini_amd.MGX_E_INVALID
        with pytest.raises(mini_amd.MgxError) as err:
            go(None, length=1, walks_per_start=1 << 25, paths=False)         # 100 x 2^25 walkers
        assert err.value.status == mini_amd.MGX_E_FRONTIER_OVERFLOW
    with pytest.raises(mini_amd.MgxError):                                    # a refused run leaves nothing to the getters
        rp.ends()
    rp.set_timing(True)
    rp.run(None, length=10, weighted=True)
    ms = rp.phase_ms()
    assert set(ms) == {"setup", "walk"} and ms["walk"] > 0.0 and ms["setup"] > 0.0
    rp.close()
    rp.close()
    g.close()


def test_another_stream(gpu_ctx, torch_mod):
    import mini_amd
    ro, ci = cases.random_symmetric(2000, 8000, 47)
    a, _ = _check(gpu_ctx, ro, ci, None, None, length=15, seed=3, p=0.5, q=2.0)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        b, _ = _check(ctx, ro, ci, None, None, length=15, seed=3, p=0.5, q=2.0)
        assert np.array_equal(a["paths"], b["paths"])
    finally:
        ctx.close()
