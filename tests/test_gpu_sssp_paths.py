"""GPU suite (-m gpu): the fused SSSP (include/mgx/sssp_fused.hpp) path by path.  Every path is forced by the switches of
include/mgx/env.hpp on a fresh Graph (the layout-time switches are read when the layout is built, MGX_SSSP_DENSE once per graph),
asserted through SsspProblem.path_info(), and run on inputs built so that every entry matters (tests/sssp_cases.py).

Every comparison is np.array_equal against oracle.sssp_dijkstra_f32 -- unreached vertices as FLT_MAX; there is no tolerance: the
min-plus fixed point is unique in float32 whatever the order of the relaxations.  tests/test_sssp_cases_cpu.py shows the oracle
right on the same inputs.

path_info's contract: swept + walked_with_bounds + walked_without_bounds + threshold_moves == iterations; threshold_moves is 0
without near / far buckets."""
import numpy as np
import pytest

from tests import sssp_cases as sc
from tests.sssp_checks import check_shortest_path_tree

pytestmark = pytest.mark.gpu

FLT_MAX = sc.FLT_MAX
SWITCHES = ("MGX_SSSP_DENSE", "MGX_SSSP_HOT_MIN_EDGES", "MGX_SSSP_BUILD_LIST", "MGX_BFS_PACK24", "MGX_BFS_LONG_MIN")
TRACE_CAP = 4096                    # iterations the device's trace holds: path_info counts no longer run (include/mgx.h)
SWEEP_ALL = str(1 << 20)            # MGX_SSSP_DENSE: an iteration is heavy from m / 2^20 frontier edges -- one vertex's row

# name -> (switches, library-built weighted layout, delta)
PATHS = {
    "walk": ({"MGX_SSSP_DENSE": "0", "MGX_SSSP_HOT_MIN_EDGES": str(1 << 30)}, True, None),
    "walk_bounds": ({"MGX_SSSP_DENSE": "0", "MGX_SSSP_HOT_MIN_EDGES": "0"}, True, None),
    "sweep_default": ({}, True, None),
    "sweep_all": ({"MGX_SSSP_DENSE": SWEEP_ALL, "MGX_SSSP_HOT_MIN_EDGES": "0"}, True, None),
    "sweep_all_ids32": ({"MGX_SSSP_DENSE": SWEEP_ALL, "MGX_BFS_PACK24": "0"}, True, None),
    "list": ({"MGX_SSSP_BUILD_LIST": "1"}, True, None),
    "delta0.5": ({}, True, 0.5),
    "delta4": ({}, True, 4.0),
    "delta1e9": ({}, True, 1e9),
    "delta20000": ({}, True, 20000.0),
    "no_layout": ({"MGX_SSSP_HOT_MIN_EDGES": "0"}, False, None),
}


def _setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph(ctx, ro, ci, w, layout):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    if layout:
        g.build_layout(weights=True)
    return g


def _run(sssp, src, want, delta=None, tag=None):
    """one run: the oracle's distances, and counts that add up"""
    st = sssp.run(src) if delta is None else sssp.run(src, delta)
    got = sssp.distances()
    assert got.dtype == np.float32
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s src=%d: %d distances differ, first at %d: got %r, want %r" % (tag, src, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    if st["iterations"] > TRACE_CAP:
        # (narrow buckets under wide-ranged weights: a threshold move per vertex)  the documented status, not a wrong count
        import mini_amd
        assert delta, (tag, st)
        with pytest.raises(mini_amd.MgxError):
            sssp.path_info()
        return st, None
    pi = sssp.path_info()
    assert pi["swept"] + pi["walked_with_bounds"] + pi["walked_without_bounds"] + pi["threshold_moves"] == st["iterations"], (tag, src, st, pi)
    assert min(pi["swept"], pi["walked_with_bounds"], pi["walked_without_bounds"], pi["threshold_moves"]) >= 0
    if delta is None or delta == 0:
        assert pi["threshold_moves"] == 0, (tag, pi)
    return st, pi


def _expect_off(pi, tag):
    assert not pi["sweep_available"] and pi["sweep_variant"] == 0 and pi["swept"] == 0, (tag, pi)


def _check_path(name, pi, st, units24_variant, tag, m):
    """what path_info must say on path `name`; units24_variant: the variant of the weight class on a 24-bit layout"""
    env, layout, delta = PATHS[name]
    if pi is None:
        assert delta
        return
    assert pi["layout_space"] == layout, (tag, pi)
    assert pi["queue_build"] == ("list" if name == "list" else "direct"), (tag, pi)
    if name in ("walk", "walk_bounds", "list", "no_layout") or delta is not None:
        _expect_off(pi, tag)
    if name == "walk":
        assert pi["walked_with_bounds"] == 0 and pi["walked_without_bounds"] == st["iterations"], (tag, pi)
    if name in ("walk_bounds", "no_layout"):
        assert pi["walked_without_bounds"] == 0 and pi["walked_with_bounds"] == st["iterations"], (tag, pi)
    if name == "sweep_default":
        assert pi["sweep_available"] and pi["sweep_variant"] == units24_variant, (tag, pi)
    if name == "sweep_all":
        assert pi["sweep_available"] and pi["sweep_variant"] == units24_variant, (tag, pi)
        assert pi["walked_without_bounds"] == 0, (tag, pi)
    if name == "sweep_all_ids32":
        assert pi["sweep_available"] and pi["sweep_variant"] == 1, (tag, pi)
    if name in ("sweep_all", "sweep_all_ids32") and st["iterations"] > 0:
        assert pi["swept"] >= 1, (tag, pi)
        if m <= (1 << 20):
            assert pi["swept"] == st["iterations"], (tag, pi)          # one frontier edge x 2^20 >= m: nothing is left to the queue walk


_RMAT = {}


def _matrix_graph(oracle, name):
    if name == "ladder":
        return sc.ladder()
    if name not in _RMAT:
        scale = int(name[4:])
        _, ro, ci, _ = oracle.rmat_csr(scale, 16, scale)
        _RMAT[name] = (ro, ci)
    return _RMAT[name]


def _matrix_sources(name, ro):
    deg = np.diff(ro)
    if name == "ladder":
        h = len(sc.LADDER_DEGS)
        return [0, h, len(deg) - 1, 1 + sc.LADDER_DEGS.index(5)]      # the source of the ladder, its largest hub, a leaf, a short hub
    leaf = np.nonzero(deg == 1)[0]
    short = np.nonzero((deg >= 2) & (deg <= 16))[0]
    return [int(np.argmax(deg)), int(leaf[len(leaf) // 2]), int(short[len(short) // 3])]


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name", ["ladder", "rmat13", "rmat16"])
def test_path_matrix(gpu_ctx, oracle, monkeypatch, name, kind):
    """graph x weight class, on every path, from a hub, a leaf and a short row: the oracle's distances and the path that was asked for"""
    import mini_amd
    ro, ci = _matrix_graph(oracle, name)
    w = sc.weights(kind, ro, ci, np.random.default_rng(sc.KINDS.index(kind)))
    srcs = _matrix_sources(name, ro)
    want = {s: oracle.sssp_dijkstra_f32(ro, ci, w, s) for s in srcs}
    swept_default = 0
    for pname, (env, layout, delta) in PATHS.items():
        _setenv(monkeypatch, env)
        g = _graph(gpu_ctx, ro, ci, w, layout)
        if layout:
            info = g.layout_info()
            assert info["units"] >= 16 and info["units_24bit"] == (0 if pname == "sweep_all_ids32" else 1), (pname, info)
        sssp = mini_amd.SsspProblem(g, 0)
        with pytest.raises(mini_amd.MgxError):
            sssp.path_info()                                            # a status before the first run, as mgx_sssp_iteration_trace
        for s in srcs:
            tag = "%s/%s/%s" % (name, kind, pname)
            st, pi = _run(sssp, s, want[s], delta, tag)
            _check_path(pname, pi, st, sc.VARIANT[kind], tag, len(ci))
            if pname == "sweep_default":
                swept_default += pi["swept"]
                if name == "ladder" and s == 0:
                    # iteration 1 holds every hub: sum(degs) of the graph's 2 sum(degs) entries -- heavy at the default m / 4
                    assert pi["swept"] >= 1, (tag, pi)
        sssp.close()
    if name != "ladder":
        assert swept_default >= 1, "no R-MAT source reached a heavy iteration: the default threshold is not exercised"


def _threshold_graph(extra):
    """vertex 0 holds D = 1024 entries (16 units) to vertices of out-degree 0; the other 3 D entries sit in rows nobody reaches:
    m = 4 D exactly -- iteration 0 has D frontier edges, D * 4 >= m.  extra: one more entry in an unreachable row, m = 4 D + 1."""
    D = 1024
    s = [np.zeros(D, dtype=np.int64), np.repeat(np.arange(D + 1, 2 * D + 1), 3)]
    d = [np.arange(1, D + 1), np.tile(np.arange(D + 1, D + 4), D)]
    if extra:
        s.append(np.array([2 * D + 1])); d.append(np.array([D + 1]))
    return sc.csr_from_edges(2 * D + 2, np.concatenate(s), np.concatenate(d))


@pytest.mark.parametrize("extra", [0, 1])
def test_an_iteration_exactly_at_the_sweep_threshold(gpu_ctx, oracle, monkeypatch, extra):
    import mini_amd
    _setenv(monkeypatch, {"MGX_SSSP_HOT_MIN_EDGES": "0"})
    ro, ci = _threshold_graph(extra)
    assert len(ci) == 4 * 1024 + extra and ro[1] - ro[0] == 1024
    w = sc.weights("distinct", ro, ci, np.random.default_rng(0))
    g = _graph(gpu_ctx, ro, ci, w, True)
    sssp = mini_amd.SsspProblem(g, 0)
    st, pi = _run(sssp, 0, oracle.sssp_dijkstra_f32(ro, ci, w, 0), None, "threshold+%d" % extra)
    assert st["iterations"] == 1 and st["relaxations"] == 1024
    assert pi["sweep_available"] and pi["sweep_variant"] == 3
    if extra:
        assert (pi["swept"], pi["walked_with_bounds"]) == (0, 1), pi     # 1024 * 4 < 4097: the queue walk
    else:
        assert (pi["swept"], pi["walked_with_bounds"]) == (1, 0), pi     # 1024 * 4 >= 4096: the sweep


@pytest.mark.parametrize("long_min", [17, 32, 64, 16, 65])
def test_long_row_threshold_of_the_layout(gpu_ctx, oracle, monkeypatch, long_min):
    """the sweep takes layouts cut at 17 .. 64 (the short rows' degree classes end below the threshold, a unit is 64 entries); at 16
    and 65 mgx_sssp_run falls back to the queue walk.  The ladder's hubs stand on both sides of every one of these cuts."""
    import mini_amd
    _setenv(monkeypatch, {"MGX_SSSP_DENSE": SWEEP_ALL, "MGX_SSSP_HOT_MIN_EDGES": "0", "MGX_BFS_LONG_MIN": str(long_min)})
    ro, ci = sc.ladder()
    for kind in ("distinct", "one_inexact_short", "mixed_range"):
        w = sc.weights(kind, ro, ci, np.random.default_rng(1))
        g = _graph(gpu_ctx, ro, ci, w, True)
        sssp = mini_amd.SsspProblem(g, 0)
        for s in _matrix_sources("ladder", ro):
            st, pi = _run(sssp, s, oracle.sssp_dijkstra_f32(ro, ci, w, s), None, "long_min=%d/%s" % (long_min, kind))
            if 17 <= long_min <= 64:
                assert pi["sweep_available"] and pi["sweep_variant"] == sc.VARIANT[kind] and pi["swept"] == st["iterations"] >= 2, pi
            else:
                _expect_off(pi, long_min)
                assert pi["walked_with_bounds"] == st["iterations"]
        sssp.close()


# ---- structural graphs ------------------------------------------------------------------------------------------------------------
def _structural_cases():
    out = []
    for shuffled in (False, True):
        ro, ci = sc.path(3000, shuffled)
        order = sc.path_order(3000, shuffled)
        w = sc.weights("int2048", ro, ci, np.random.default_rng(1))
        out.append(("path%d" % shuffled, ro, ci, w, [int(order[0]), int(order[1500]), int(order[2999])], None))
    ro, ci = sc.grid(96, 96)
    out.append(("grid", ro, ci, sc.weights("half_edges", ro, ci, np.random.default_rng(2)), [0, 96 * 48 + 48], None))
    out.append(("grid_mixed", ro, ci, sc.weights("mixed_range", ro, ci, np.random.default_rng(2)), [96 * 96 - 1], None))
    for centre in (0, 100000):
        ro, ci = sc.star(100000, centre)
        out.append(("star%d" % centre, ro, ci, sc.weights("distinct", ro, ci, np.random.default_rng(3)), [centre, 5], 3))
        out.append(("star%d_real" % centre, ro, ci, sc.weights("mixed_range", ro, ci, np.random.default_rng(3)), [centre, 99999], 2))
    ro, ci, w = sc.bf_worst()
    out.append(("bf_worst", ro, ci, w, [0, 700], None))
    ro, ci, w = sc.dups_and_loops()
    out.append(("dups_and_loops", ro, ci, w, [0, 999], None))
    ro, ci = sc.directed_with_sinks()
    out.append(("directed_with_sinks", ro, ci, sc.weights("int2048", ro, ci, np.random.default_rng(4)),
                [sc.DWS_ROOT, sc.DWS_DEG0_SOURCE, sc.DWS_PAIR[0]], None))
    ro, ci, w = sc.overflow_chain()
    out.append(("overflow_chain", ro, ci, w, [0, 5, 11], None))
    return out


def _check_stats(ro, ci, want, src, st, tag):
    deg = np.diff(ro).astype(np.int64)
    reached = want < FLT_MAX
    depth = sc.bfs_depth(ro, ci, src)
    assert st["relaxations"] >= int(deg[reached].sum()), (tag, st)
    assert st["frontier_total"] >= int((reached & (deg > 0)).sum()), (tag, st)
    assert st["iterations"] >= int(depth[reached].max()), (tag, st)


STRUCT_PATHS = ("walk", "walk_bounds", "sweep_all", "sweep_all_ids32", "list", "delta20000", "no_layout")


@pytest.mark.parametrize("pname", STRUCT_PATHS)
def test_structural_graphs_on_every_path(gpu_ctx, oracle, monkeypatch, pname):
    """long diameters (thousands of iterations in batches of two), one row of 100 000 entries, vertices that improve many times,
    parallel entries and self loops, sinks and unreachable parts, sums that overflow -- and the predecessors built from each result"""
    import mini_amd
    env, layout, delta = PATHS[pname]
    _setenv(monkeypatch, env)
    for name, ro, ci, w, srcs, variant in _structural_cases():
        g = _graph(gpu_ctx, ro, ci, w, layout)
        sssp = mini_amd.SsspProblem(g, 0)
        for s in srcs:
            tag = "%s/%s" % (name, pname)
            want = oracle.sssp_dijkstra_f32(ro, ci, w, s)
            st, pi = _run(sssp, s, want, delta, tag)
            _check_stats(ro, ci, want, s, st, tag)
            if pname in ("walk", "walk_bounds", "list", "no_layout", "delta20000"):
                _check_path(pname, pi, st, 0, tag, len(ci))
            elif variant is not None:                                   # the stars: a row of 1563 units
                _check_path(pname, pi, st, variant, tag, len(ci))
            elif name.startswith(("path", "grid", "bf_worst", "overflow")):
                _expect_off(pi, tag)                                    # no row reaches the long-row threshold: no units, no sweep
            if name == "overflow_chain" and s == 0:
                assert np.all(want[4:] == FLT_MAX) and want[3] < FLT_MAX
            if name.startswith("path") and s == srcs[0] and delta is None:
                assert st["iterations"] == 3000, st                    # one vertex per iteration, end to end
            sssp.build_preds()
            check_shortest_path_tree(ro, ci, w, sssp.distances(), sssp.preds(), s)
        sssp.close()


@pytest.mark.parametrize("n", sc.SIZED_NS)
def test_n_around_the_lds_tables(gpu_ctx, oracle, monkeypatch, n):
    """n at and around the sizes of the two tables of 16-bit bounds (32768 entries for the queue walk, 73728 for the sweep; an odd n
    below them keeps n & ~1 bounds), bounds forced on, with and without a layout, queue walk and sweep; half the entries point at the
    vertices on both sides of the tables' ends"""
    import mini_amd
    ro, ci = sc.sized(n)
    for kind in ("distinct", "mixed_range"):
        w = sc.weights(kind, ro, ci, np.random.default_rng(n))
        srcs = sorted({0, n - 1, n // 2})
        want = {s: oracle.sssp_dijkstra_f32(ro, ci, w, s) for s in srcs}
        for pname in ("walk_bounds", "sweep_all", "sweep_all_ids32", "no_layout"):
            env, layout, delta = PATHS[pname]
            _setenv(monkeypatch, env)
            g = _graph(gpu_ctx, ro, ci, w, layout)
            sssp = mini_amd.SsspProblem(g, 0)
            for s in srcs:
                tag = "sized(%d)/%s/%s" % (n, kind, pname)
                st, pi = _run(sssp, s, want[s], delta, tag)
                _check_path(pname, pi, st, sc.VARIANT[kind], tag, len(ci))
                _check_stats(ro, ci, want[s], s, st, tag)
            sssp.close()


# ---- state carried between the runs of one problem ----------------------------------------------------------------------------------
def _long_and_short():
    """a path of 3000 vertices (a run from its end: 3000 iterations) and, apart from it, a star of 50 leaves (a run from a leaf: 3)"""
    a = np.concatenate([np.arange(2999), np.full(50, 3000)])
    b = np.concatenate([np.arange(1, 3000), np.arange(3001, 3051)])
    ro, ci = sc.csr_from_edges(3051, np.concatenate([a, b]), np.concatenate([b, a]))
    return ro, ci


@pytest.mark.parametrize("layout", [False, True])
def test_state_carried_from_run_to_run(gpu_ctx, oracle, monkeypatch, layout):
    """iters_hint (the first batch of a run is as long as the last run was), the bucket width, the predecessors' staleness and the
    path record are per problem: whatever ran before, equal calls give equal distances and equal path_info"""
    import mini_amd
    _setenv(monkeypatch, {})
    ro, ci = _long_and_short()
    w = sc.weights("int2048", ro, ci, np.random.default_rng(8))
    g = _graph(gpu_ctx, ro, ci, w, layout)
    LONG, SHORT = 0, 3001
    want = {s: oracle.sssp_dijkstra_f32(ro, ci, w, s) for s in (LONG, SHORT)}
    a, b = mini_amd.SsspProblem(g, 0), mini_amd.SsspProblem(g, 0)
    first = {}
    for s in (LONG, SHORT, SHORT, LONG, LONG, SHORT):
        st, pi = _run(a, s, want[s], None, "long/short")
        assert st["iterations"] == (3000 if s == LONG else 3), st
        assert first.setdefault(s, (st, pi)) == (st, pi), "the same call, another answer"
    # the other order on a second problem of the same graph, interleaved with the first
    for s in (SHORT, LONG, SHORT):
        st, pi = _run(b, s, want[s], None, "second problem")
        assert (st, pi) == first[s]
        st, pi = _run(a, LONG if s == SHORT else SHORT, want[LONG if s == SHORT else SHORT], None, "first problem")
        assert (st, pi) == first[LONG if s == SHORT else SHORT]
    # plain -> delta -> plain
    st_d, pi_d = _run(a, LONG, want[LONG], 20000.0, "delta")
    assert pi_d["swept"] == 0 and pi_d["sweep_variant"] == 0 and pi_d["threshold_moves"] >= 1
    assert _run(a, LONG, want[LONG], None, "plain after delta") == first[LONG]
    assert _run(a, LONG, want[LONG], 20000.0, "delta again") == (st_d, pi_d)
    assert _run(a, SHORT, want[SHORT], None, "plain after delta") == first[SHORT]
    # run -> enact -> run: the operator path shares the problem's distances, not the fused loop's state
    a.reset(SHORT)
    a.enact(8.0)
    assert np.array_equal(a.distances(), want[SHORT])
    assert a.path_info() == first[SHORT][1], "path_info describes the last fused run"
    assert _run(a, LONG, want[LONG], None, "run after enact") == first[LONG]
    a.close(); b.close()


def test_sweep_state_from_run_to_run(gpu_ctx, oracle, monkeypatch):
    """the same on a graph whose runs sweep: the frontier bitmap and the unit blocks' weights outlive a run"""
    import mini_amd
    _setenv(monkeypatch, {"MGX_SSSP_DENSE": SWEEP_ALL})
    ro, ci = sc.ladder()
    w = sc.weights("distinct", ro, ci, np.random.default_rng(0))
    g = _graph(gpu_ctx, ro, ci, w, True)
    a, b = mini_amd.SsspProblem(g, 0), mini_amd.SsspProblem(g, 0)
    srcs = _matrix_sources("ladder", ro)
    want = {s: oracle.sssp_dijkstra_f32(ro, ci, w, s) for s in srcs}
    first = {s: _run(a, s, want[s], None, "first") for s in srcs}
    for s in srcs[::-1] + srcs:
        assert _run(b, s, want[s], None, "second problem") == first[s]
        assert _run(a, s, want[s], 4.0, "delta")[1]["swept"] == 0
        assert _run(a, s, want[s], None, "again") == first[s]
        assert first[s][1]["swept"] == first[s][0]["iterations"] and first[s][1]["sweep_variant"] == 3


# ---- attached layouts ---------------------------------------------------------------------------------------------------------------
def test_no_sweep_on_an_attached_layout(gpu_ctx, oracle, monkeypatch, torch_mod):
    """mgx_graph_attach_layout / _attach_layout_weights borrow the caller's arrays at exactly num_edges entries; the sweep's short-row
    walk loads 16 bytes from a row's start whatever its length and counts on the 8 entries of slack a library-built layout carries.  So
    the sweep stays off on borrowed arrays (ensure_unit_weights: no degree classes there) -- path_info must say so even when the
    sweep is asked for on every iteration -- and the queue walk gives the oracle's distances in layout space."""
    import mini_amd
    torch = torch_mod
    _setenv(monkeypatch, {"MGX_SSSP_DENSE": SWEEP_ALL, "MGX_SSSP_HOT_MIN_EDGES": "0"})
    ro, ci = sc.ladder()
    w = sc.weights("distinct", ro, ci, np.random.default_rng(0))
    built = _graph(gpu_ctx, ro, ci, w, True)
    lro, lci, n2o, o2n, lw = built.layout_arrays(weights=True)
    assert len(lci) == len(ci) == len(lw)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (lro, lci, n2o, o2n, lw)]
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    g.attach_layout(*dev)
    assert g.layout_info()["units"] >= 16                              # (the unit blocks are there, for the fused BFS)
    sssp = mini_amd.SsspProblem(g, 0)
    ref = mini_amd.SsspProblem(built, 0)
    for s in _matrix_sources("ladder", ro):
        want = oracle.sssp_dijkstra_f32(ro, ci, w, s)
        st, pi = _run(sssp, s, want, None, "attached")
        _expect_off(pi, "attached")
        assert pi["layout_space"] and pi["walked_with_bounds"] == st["iterations"]
        st2, pi2 = _run(ref, s, want, None, "built")
        assert pi2["sweep_available"] and pi2["swept"] == st2["iterations"]
    sssp.close(); ref.close()
