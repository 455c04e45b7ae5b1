"""GPU suite (-m gpu): fan-out neighbour sampling (mgx_nsample_*).  The fused path (mgx_nsample_run), the operator path
(mgx_nsample_enact) and the numpy model (tests/nsample_model.py) agree bit for bit -- vertices, hop_offsets, row_offsets, cols,
entry_pos, seed_local, the twelve model stats and the bins -- on the golden fixtures, every group width with rows round the
fan-out and of 100 000 entries, frontier sizes round the wave and the workgroup and past one grid, the last partial group of a wave,
every copy cut, the bitmap's word edges, the bounds' clamps, handle reuse, H = 0 .. 16 and R-MAT 10 - 16.  The fused path's launches
and host waits are exact; a repeat run gives the same and allocates nothing."""
import os

import numpy as np
import pytest

from tests import nsample_cases as cases
from tests import nsample_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
ENV = {"short_max": "MGX_NSAMPLE_SHORT_MAX", "wave_max": "MGX_NSAMPLE_WAVE_MAX", "seg": "MGX_NSAMPLE_SEG"}
SMALL_CUTS = {"short_max": 4, "wave_max": 16, "seg": 16}


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(ENV[k], str(v))


def _same_results(sp, want, who):
    for name in model.ARRAYS:
        got = getattr(sp, name)()
        assert got.dtype == np.int32 and got.shape == want[name].shape, (who, name, got.shape, want[name].shape)
        assert np.array_equal(got, want[name]), "%s: %d of %s differ" % (who, int((got != want[name]).sum()), name)
    off = want["hop_offsets"]
    for h in range(len(off) - 2):
        ro, co = sp.block(h)
        lo, hi = want["row_offsets"][off[h]], want["row_offsets"][off[h + 1]]
        assert np.array_equal(ro, want["row_offsets"][off[h]:off[h + 1] + 1] - lo) and np.array_equal(co, want["cols"][lo:hi]), (who, h)


def _check(ctx, ro, ci, seeds=None, fanouts=(3, 2), replace=False, seed=1, opts=None, operator=True, operator_first=False):
    """fused == operator path == model; the repeat run and its allocations; launches and host waits; the bins.  opts: the switches
    the handle reads."""
    import mini_amd
    opts = opts or {}
    fanouts = list(fanouts)
    want = model.sample(ro, ci, seeds, fanouts, replace, seed, **opts)
    n = len(ro) - 1
    count = n if seeds is None else len(seeds)
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    sp = mini_amd.NeighborSampleProblem(g)
    args = dict(seeds=seeds, fanouts=fanouts, replace=replace, seed=seed)
    if operator_first:
        so = sp.enact(**args)
        _same_results(sp, want, "operator path first")
        assert {k: so[k] for k in KEYS} == want["stats"], (so, want["stats"])
    s1 = sp.run(**args)
    print("fused", s1)
    _same_results(sp, want, "fused")
    assert {k: s1[k] for k in KEYS} == want["stats"], (s1, want["stats"])
    assert (s1["launches"], s1["host_waits"]) == model.fused_counts(n, count, len(fanouts), seeds is not None), s1
    b = sp.bins()
    assert {k: b[k] for k in model.BIN_KEYS} == want["bins"], (b, want["bins"])
    sm = opts.get("short_max", model.SHORT_MAX)
    assert (b["short_max"], b["wave_max"], b["seg"]) == (sm, max(opts.get("wave_max", model.WAVE_MAX), sm), opts.get("seg", model.SEG))
    before = mini_amd.lib.mgx_device_allocations()
    s2 = sp.run(**args)                                          # a repeat run: the same, and nothing allocated
    assert mini_amd.lib.mgx_device_allocations() == before
    assert s2 == s1
    _same_results(sp, want, "fused, repeated")
    assert sp.bins() == b
    if operator:
        so = sp.enact(**args)
        print("operator", so)
        _same_results(sp, want, "operator path")
        assert {k: so[k] for k in KEYS} == want["stats"], (so, want["stats"])
        s3 = sp.run(**args)                                      # fused behind the operator path on one handle
        assert s3 == s1
        _same_results(sp, want, "fused behind the operator path")
    sp.close()
    g.close()
    return want, s1


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("replace", [False, True])
def test_fixtures(gpu_ctx, oracle, name, replace):
    for undir in (True, False):
        n, ro, ci, w, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
        for fanouts in ([2], [3, 2], [-1, 1]):
            _check(gpu_ctx, ro, ci, None, fanouts, replace, seed=5)
            _check(gpu_ctx, ro, ci, np.arange(0, n, 3), fanouts, replace, seed=6, operator_first=True)


@pytest.mark.parametrize("k", cases.WIDTHS)
def test_group_widths(gpu_ctx, k):
    """seed rows of k - 1, k, k + 1, 2 k + 1, 1 000 and 100 000 entries: whole rows, the first Floyd row (every draw but one
    collides with high probability: the masked ballot), and rows whose cost must not be their length"""
    ro, ci, degrees = cases.width_rows(k)
    seeds = np.arange(len(degrees))
    want, s = _check(gpu_ctx, ro, ci, seeds, [k], seed=k)
    assert s["whole_rows"] == (2 if k > 1 else 1) and s["sampled_rows"] == 4 and s["draws"] == 4 * k
    if k >= 8:
        only = model.sample(ro, ci, [2], [k], seed=k)             # the row of k + 1 entries alone
        assert only["stats"]["collisions"] > 0
    want, s = _check(gpu_ctx, ro, ci, seeds, [k], True, seed=k, operator=False)
    assert s["sampled_rows"] == (6 if k > 1 else 5) and s["collisions"] == 0


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_frontier_sizes_round_the_wave_and_the_workgroup(gpu_ctx, count):
    ro, ci = cases.random_digraph(3000, 30000, 31)
    seeds = np.random.default_rng(count).choice(3000, count, replace=False)
    _check(gpu_ctx, ro, ci, seeds, [5, 2], seed=count)
    _check(gpu_ctx, ro, ci, seeds, [1], True, seed=count, operator=False)


def test_grid_stride_loops_on_one_compute_unit(monkeypatch, torch_mod, built):
    """8 workgroups: 20 000 frontier rows are 10 tiles of 2 048, 1 200 000 vertices 10 tiles of bitmap words, and a wave samples
    a run of many passes"""
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, *cases.random_digraph(20000, 60000, 32), None, [2, 2], seed=3)
        ro, ci = cases.random_digraph(1200000, 2400000, 33)
        _check(ctx, ro, ci, np.random.default_rng(1).integers(0, 1200000, 300), [3, -1], seed=4)


@pytest.mark.parametrize("k, rows", [(16, 5), (16, 7), (3, 17), (3, 33), (64, 3)])
def test_last_partial_group_of_a_wave(gpu_ctx, k, rows):
    ro, ci = cases.fan_rows([2 * k + 3] * rows, seed=rows, back=2)
    _check(gpu_ctx, ro, ci, np.arange(rows), [k, 1], seed=k)


@pytest.mark.parametrize("k", [3, 16])
def test_floyd_whole_and_empty_rows_alternate(gpu_ctx, k):
    ro, ci = cases.fan_rows([k + 3, 2, 0] * 50, seed=k)
    want, s = _check(gpu_ctx, ro, ci, np.arange(150), [k], seed=2)
    assert (s["sampled_rows"], s["whole_rows"], s["empty_rows"]) == (50, 50, 50)


def test_copy_cuts(gpu_ctx, monkeypatch):
    """fan-out -1 with small cuts: rows at every edge of a lane's, a wave's and the segmented copy; at the defaults a row of 100 000"""
    ro, ci = cases.fan_rows([100000], seed=1)
    want, s = _check(gpu_ctx, ro, ci, [0], [-1])
    assert want["bins"]["long"] == 1 and want["bins"]["segments"] == -(-100000 // model.SEG) and s["edges"] == 100000
    _setenv(monkeypatch, SMALL_CUTS)
    degrees = [0, 1, 4, 5, 16, 17, 32, 33]
    ro, ci = cases.fan_rows(degrees * 9, seed=2, back=3)
    want, s = _check(gpu_ctx, ro, ci, np.arange(len(degrees) * 9), [-1, -1], opts=SMALL_CUTS)
    assert want["bins"]["long"] >= 27 and want["bins"]["wave"] >= 18 and want["bins"]["short"] >= 18 and want["bins"]["none"] >= 9


def test_bitmap_and_map_edges(gpu_ctx):
    ro, ci, edge = cases.bitmap_edges(200)
    _check(gpu_ctx, ro, ci, edge, [2, 2])                                       # as seeds
    want, s = _check(gpu_ctx, ro, ci, [10], [-1, 1, 1])                         # as destinations
    assert want["vertices"].tolist()[1:8] == edge.tolist()
    want, s = _check(gpu_ctx, np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), None, [3, 3])   # n = 1, a self-loop
    assert s["vertices"] == 1 and s["revisits"] == 1 and s["edges"] == 1
    want, s = _check(gpu_ctx, *cases.empty(0), None, [2])                       # n = 0
    assert (s["launches"], s["host_waits"], s["vertices"]) == (0, 0, 0)
    want, s = _check(gpu_ctx, *cases.empty(50), None, [2, -1])                  # m = 0
    assert s["vertices"] == 50 and s["edges"] == 0 and s["empty_rows"] == 50
    ro, ci = cases.random_digraph(300, 2000, 5)
    want, s = _check(gpu_ctx, ro, ci, [], [2])                                  # no seeds
    assert (s["launches"], s["host_waits"]) == (0, 0)
    seeds = np.array([7, 299, 7, 0, 7, 299, 150])
    want, s = _check(gpu_ctx, ro, ci, seeds, [3, 2])                            # duplicate seeds
    assert s["unique_seeds"] == 4 and want["vertices"][want["seed_local"]].tolist() == seeds.tolist()
    want, s = _check(gpu_ctx, ro, ci, None, [2, 2])                             # every vertex: nothing is left for the later hops
    assert s["unique_seeds"] == 300 and s["vertices"] == 300 and s["revisits"] == s["edges"]
    want, s = _check(gpu_ctx, *cases.reached_twice(), [0], [-1, -1, -1])
    assert s["revisits"] == 1 and want["vertices"].tolist() == [0, 1, 2, 3]
    want, s = _check(gpu_ctx, *cases.loops_and_duplicates(), [0, 5, 9], [4, 4, 4])
    assert s["sampled_rows"] > 0 and s["revisits"] > 0


def test_bounds(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_digraph(50, 120, 6)
    assert model.bounds(50, len(ci), 50, [5, 5], False) == ([50, 50, 50], [len(ci), len(ci)])       # F clamps at n, E at m
    _check(gpu_ctx, ro, ci, None, [5, 5])
    ro, ci = cases.directed_path(20)
    want, s = _check(gpu_ctx, ro, ci, None, [10], True)                         # rows of one entry drawn ten times: E > m
    assert s["edges"] == 190 > len(ci)
    ro, ci = cases.empty(2200000)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.NeighborSampleProblem(g)
    for go in (sp.run, sp.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go(None, [64] * 16, replace=True)                                   # 16 x 64 x 2.2 M entries
        assert err.value.status == mini_amd.MGX_E_FRONTIER_OVERFLOW
        with pytest.raises(mini_amd.MgxError) as err:
            sp.vertices()
        assert err.value.status == mini_amd.MGX_E_INVALID
    sp.close()
    g.close()


def test_handle_reuse(gpu_ctx):
    """on ONE handle a large batch, a small disjoint one and the large one again: each what a fresh handle gives -- the run's end
    must have cleared every `seen` bit, and no stale map entry may be read"""
    import mini_amd
    ro, ci = cases.random_digraph(5000, 40000, 7)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    large, small = np.arange(0, 4000, 2), np.arange(4001, 4100, 7)
    one = mini_amd.NeighborSampleProblem(g)
    for seeds, fanouts in ((large, [6, 3]), (small, [2, 2, 2]), (large, [6, 3]), (small, [-1]), (None, [1])):
        want = model.sample(ro, ci, seeds, fanouts, seed=9)
        s = one.run(seeds, fanouts, seed=9)
        _same_results(one, want, "one handle")
        assert {k: s[k] for k in KEYS} == want["stats"]
        fresh = mini_amd.NeighborSampleProblem(g)
        assert fresh.run(seeds, fanouts, seed=9) == s
        _same_results(fresh, want, "fresh handle")
        so = fresh.enact(seeds, fanouts, seed=9)                                # operator behind fused on one handle
        _same_results(fresh, want, "operator behind fused")
        assert {k: so[k] for k in KEYS} == want["stats"]
        fresh.close()
    for call in (lambda: one.run([5000], [2]), lambda: one.run([1], [65]), lambda: one.enact([-1], [2])):
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID
        for getter in (one.vertices, one.hop_offsets, one.row_offsets, one.cols, one.entry_pos, one.seed_local, one.vertices_device_ptr, one.bins):
            with pytest.raises(mini_amd.MgxError) as err:                       # a refused run leaves nothing to the getters
                getter()
            assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
    one.run(small, [2])
    assert one.vertices_device_ptr() and one.row_offsets_device_ptr() and one.cols_device_ptr() and one.entry_pos_device_ptr()
    one.close()
    one.close()
    g.close()


@pytest.mark.parametrize("hops", [0, 1, 4, 16])
def test_hops(gpu_ctx, hops):
    want, s = _check(gpu_ctx, *cases.directed_path(40), [0], [1] * hops)        # one new vertex per hop
    assert want["vertices"].tolist() == list(range(hops + 1)) and s["launches"] == 5 * hops + 4
    for fanouts in ([4] * hops, [-1] * hops, [2] * hops):
        want, s = _check(gpu_ctx, *cases.grid(20, 20), [0], fanouts)            # a diagonal per hop
        if fanouts != [2] * hops:
            assert np.diff(want["hop_offsets"]).tolist() == [1] + list(range(2, hops + 2))


@pytest.mark.parametrize("scale", [10, 12, 14, 16])
@pytest.mark.parametrize("replace", [False, True])
def test_rmat(gpu_ctx, oracle, scale, replace):
    n, ro, ci, w = oracle.rmat_csr(scale, 16, scale + 500, undir=False)
    seeds = np.random.default_rng(scale).integers(0, n, 200)
    for fanouts in ([5, 3, 2], [15, 10]):
        _check(gpu_ctx, ro, ci, seeds, fanouts, replace, seed=scale, operator=scale <= 14 or fanouts[0] == 5)
    ro, ci = cases.random_digraph(1 << scale, 8 << scale, scale)
    _check(gpu_ctx, ro, ci, seeds, [15, 10], replace, seed=scale, operator=False)


def test_timing_changes_nothing(gpu_ctx):
    import mini_amd
    ro, ci = cases.random_digraph(4000, 40000, 8)
    seeds = np.arange(0, 4000, 40)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.NeighborSampleProblem(g)
    with pytest.raises(mini_amd.MgxError):
        sp.phase_ms()
    plain = sp.run(seeds, [5, 5, -1], seed=3)
    want = model.sample(ro, ci, seeds, [5, 5, -1], seed=3)
    sp.set_timing(True)
    timed = sp.run(seeds, [5, 5, -1], seed=3)
    assert timed == plain
    _same_results(sp, want, "timed")
    ms = sp.phase_ms()
    assert set(ms) == {"sample", "dedup"} and ms["sample"] > 0.0 and ms["dedup"] > 0.0
    sp.close()
    g.close()


def test_another_stream(gpu_ctx, torch_mod):
    import mini_amd
    ro, ci = cases.random_symmetric(2000, 8000, 47)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _check(ctx, ro, ci, np.arange(100), [4, 4], seed=3)
    finally:
        ctx.close()
