"""GPU suite (-m gpu): betweenness centrality (mgx_bc_*).  The fused path (mgx_bc_run: atomic-free pull sweeps over
level lists), the operator path (mgx_bc_enact: the textbook form with atomic adds) and the numpy model (tests/bc_model.py).

The comparison rule (one helper, _same):
  * labels and sigma are bit-equal between the three -- the helper first asserts that the model's largest sigma is below 2^53, so
    the integer sums are exact in any order;
  * delta and bc match exactly where either side is 0; elsewhere |a - b| <= rtol * max(a, b) with
        rtol = 2 * (L * (R + 2) + S) * 2^-53
    L the deepest traversal, R the longest in- or out-row, S the number of sources (tests/bc_model.py: rtol): every term is
    non-negative, a level adds at most R + 2 roundings to the relative error, the sum over the sources at most S, and two
    implementations double it.  Derived, not tuned; computed from each case's own L, R and S (about 1e-10 on RMAT-18);
  * two fused runs with the same arguments are bit-equal in bc, sigma and delta; a fused run waits for the host once."""
import os

import numpy as np
import pytest

from tests import bc_model as model
from tests import coloring_model as cm

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
ARRAYS = ("labels", "sigma", "delta", "bc")


def _graph(ctx, ro, ci, csc=False, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, np.ascontiguousarray(ro, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), None)
    if csc:
        g.build_csc()
    if layout:
        g.build_layout()
    return g


def _arrays(bp):
    return {"labels": bp.labels(), "sigma": bp.sigma(), "delta": bp.delta(), "bc": bp.centrality()}


def _close(tag, a, b, rtol):
    # (a directed graph declared symmetric can leave sigma = 0 on a reached vertex: 1 / 0 and 0 * inf follow on every side alike.
    #  NaN and inf must sit at the same vertices; the rule below is for the finite values)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), tag + ": the non-finite values differ"
    fin = np.isfinite(a)
    a, b = a[fin], b[fin]
    zero = (a == 0) | (b == 0)
    assert np.array_equal(a[zero], b[zero]), "%s: the exact zeros differ at %d vertices" % (tag, int((a[zero] != b[zero]).sum()))
    big = np.maximum(a, b)
    err = np.abs(a - b)
    worst = float((err[~zero] / big[~zero]).max()) if (~zero).any() else 0.0
    print("%s: max rel %.3g (rtol %.3g)" % (tag, worst, rtol))
    assert (err <= rtol * big).all(), "%s: %d outside rtol %.3g (max %.3g)" % (tag, int((err > rtol * big).sum()), rtol, worst)


def _same(tag, got, want, rtol):
    assert got["labels"].dtype == np.int32 and got["sigma"].dtype == np.float64
    assert np.array_equal(got["labels"], want["labels"]), tag + ": labels"
    assert np.array_equal(got["sigma"], want["sigma"], equal_nan=True), tag + ": sigma"
    _close(tag + ": delta", got["delta"], want["delta"], rtol)
    _close(tag + ": bc", got["bc"], want["bc"], rtol)


def _bit_equal(tag, a, b):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (tag, k)


def _check(ctx, ro, ci, sources, symmetric, csc=False, layout=False, operator=True, want=None):
    """fused (twice), operator path and model; returns (fused arrays, fused stats, model, info)"""
    import mini_amd
    if want is None:
        want = model.run(ro, ci, sources, symmetric)
    assert want["max_sigma"] < model.TWO53                                  # the sigma sums are exact in any order
    S = want["stats"][0]
    rtol = model.rtol(want["stats"][1], max(want["longest_in"], want["longest_out"]), S)
    g = _graph(ctx, ro, ci, csc, layout)
    bp = mini_amd.BcProblem(g)
    sf = bp.run(sources, symmetric)
    af = _arrays(bp)
    info = bp.info()
    sf2 = bp.run(sources, symmetric)
    _bit_equal("two fused runs", _arrays(bp), af)
    _same("fused against model", af, want, rtol)
    got = [sf[k] for k in ("sources", "levels", "reached", "inexact", "overflow")]
    assert got == want["stats"], (sf, want["stats"])
    assert sf["host_waits"] == 1 and sf2["host_waits"] == 1, (sf, sf2)
    assert sf["used_csc"] == int(not symmetric)
    assert info["longest_in"] == want["longest_in"] and info["longest_out"] == want["longest_out"], info
    if operator:
        so = bp.enact(sources, symmetric)
        ao = _arrays(bp)
        _same("operator against model", ao, want, rtol)
        _same("operator against fused", ao, af, rtol)
        assert [so[k] for k in ("sources", "levels", "reached", "inexact", "overflow")] == want["stats"], (so, want["stats"])
    bp.close()
    g.close()
    return af, sf, want, info


def _sources(ro, seed):
    """the largest-degree vertex, the first and the last non-isolated vertex, 5 seeded random ones"""
    deg = np.diff(ro)
    nz = np.nonzero(deg)[0]
    rng = np.random.default_rng(seed)
    return np.array([int(np.argmax(deg)), int(nz[0]), int(nz[-1])] + [int(x) for x in rng.choice(nz, 5, replace=False)], dtype=np.int32)


def _grid(w):
    v = np.arange(w * w).reshape(w, w)
    s, d = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return cm.csr(w * w, s, d)


def _path(n):
    a = np.arange(n - 1)
    return cm.csr(n, a, a + 1)


# ---- fixtures, all sources ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
def test_fixtures(gpu_ctx, oracle, name, undir, symmetric):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    # a directed load declared symmetric is the caller's business: the model takes the same word, the operator path (which reads
    # the out-entries alone) is compared where the word is true
    _check(gpu_ctx, ro, ci, None, symmetric, csc=not symmetric, operator=undir or not symmetric)


@pytest.mark.parametrize("undir", [True, False])
def test_rmat10_all_sources_and_networkx(gpu_ctx, oracle, undir):
    import mini_amd
    import networkx as nx
    n, ro, ci, _ = oracle.rmat_csr(10, 8, 10, undir=undir)
    _check(gpu_ctx, ro, ci, None, undir, csc=not undir)
    ro, ci = model.dedup(ro, ci)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.repeat(np.arange(n), np.diff(ro)).tolist(), ci.tolist()))
    ref = nx.betweenness_centrality(G, normalized=False)
    ref = np.array([ref[v] for v in range(n)])
    g = _graph(gpu_ctx, ro, ci, csc=not undir)
    bp = mini_amd.BcProblem(g)
    st = bp.run(None, undir)
    R = int(max(np.diff(ro).max(), np.bincount(ci, minlength=n).max()))
    _close("fused against networkx", bp.centrality(), ref, model.rtol(st["levels"], R, n))
    if undir:                                                              # networkx's two scalings, on the host
        und = nx.betweenness_centrality(nx.Graph(G), normalized=True)
        np.testing.assert_allclose(bp.centrality(normalized=True, undirected=True), np.array([und[v] for v in range(n)]), rtol=1e-12, atol=1e-18)
    bp.close()
    g.close()


# ---- sampled sources --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,ef,undir", [(12, 4, True), (14, 16, True), (14, 8, False), (16, 16, True)])
@pytest.mark.parametrize("layout", [False, True])
def test_rmat_sampled_sources(gpu_ctx, oracle, scale, ef, undir, layout):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale, undir=undir)
    _check(gpu_ctx, ro, ci, _sources(ro, scale), undir, csc=not undir, layout=layout)


def test_rmat18_fused_against_model(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(18, 16, 18)
    af, sf, want, info = _check(gpu_ctx, ro, ci, _sources(ro, 18)[:3], True, operator=False)
    assert info["in_huge"] > 0 and info["in_wave"] > 0 and info["in_lane"] > 0, info      # the default thresholds use every class here


def _device_graph(ctx, d):
    import mini_amd
    return mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])


def _device_sources(d, count):
    ro = d["row_offsets"].cpu().numpy()
    return _sources(ro, 7)[:count], ro


def test_rmat20_fused_against_operator_path(gpu_ctx):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(gpu_ctx, 20, 16)
    src, ro = _device_sources(d, 2)
    g = _device_graph(gpu_ctx, d)
    bp = mini_amd.BcProblem(g)
    sf = bp.run(src, True)
    af = _arrays(bp)
    so = bp.enact(src, True)
    ao = _arrays(bp)
    print("fused", sf, "operator", so)
    assert float(af["sigma"].max()) < model.TWO53
    _same("operator against fused", ao, af, model.rtol(sf["levels"], int(np.diff(ro).max()), 2))
    assert [sf[k] for k in ("sources", "levels", "reached", "inexact", "overflow")] == [so[k] for k in ("sources", "levels", "reached", "inexact", "overflow")]
    assert sf["host_waits"] == 1
    bp.close()
    g.close()


def test_rmat22_identities_and_sampled_cpu_check(gpu_ctx):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(gpu_ctx, 22, 16)
    src, ro = _device_sources(d, 2)
    n = d["n"]
    g = _device_graph(gpu_ctx, d)
    bp = mini_amd.BcProblem(g)
    sf = bp.run(src, True)
    a = _arrays(bp)
    print("fused", sf, bp.info())
    assert sf["host_waits"] == 1 and sf["inexact"] == 0
    rtol = model.rtol(sf["levels"], int(np.diff(ro).max()), 2)
    label, sigma, delta = a["labels"], a["sigma"], a["delta"]
    s = int(src[-1])
    bfs = mini_amd.BfsProblem(g, s)
    bfs.run(s)
    assert np.array_equal(label, bfs.labels())
    # the identity: sum of delta = sum over the reached t != s of (label[t] - 1)
    want = float((label[label > 0].astype(np.int64) - 1).sum())
    assert abs(float(delta.sum()) - want) <= rtol * n * max(want, 1.0) and delta[s] == 0.0, (delta.sum(), want)
    # 1000 seeded vertices: sigma from the in-row exactly, delta from the out-row within rtol (the graph is symmetric: the same row)
    ro64, ci = ro.astype(np.int64), d["col_indices"].cpu().numpy()
    rng = np.random.default_rng(22)
    for v in rng.choice(np.nonzero(label > 0)[0], 1000, replace=False):
        row = ci[ro64[v]:ro64[v + 1]]
        up = row[label[row] == label[v] - 1]
        assert float(sigma[up].sum()) == sigma[v], (v, sigma[v])
        down = row[label[row] == label[v] + 1]
        dv = float((sigma[v] / sigma[down] * (1.0 + delta[down])).sum())
        assert abs(dv - delta[v]) <= rtol * max(dv, delta[v]), (v, dv, delta[v])
    bfs.close()
    bp.close()
    g.close()


# ---- every class forced ---------------------------------------------------------------------------------------------------------------
def _class_counts(ro, lane_max, huge_min, seg):
    d = np.diff(ro).astype(np.int64)
    lane = d <= lane_max
    huge = ~lane & (d >= huge_min)
    return int(lane.sum()), int((~lane & ~huge).sum()), int(huge.sum()), int(((d[huge] + seg - 1) // seg).sum())


@pytest.mark.parametrize("env", [{"MGX_BC_LANE_MAX": "1"}, {"MGX_BC_HUGE_MIN": "64", "MGX_BC_SEG": "64"}, {"MGX_BC_HUGE_MIN": "64", "MGX_BC_SEG": "1000"}],
                         ids=["lane1", "huge64-seg64", "huge64-seg1000"])
def test_every_class_forced(gpu_ctx, oracle, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lane_max, huge_min, seg = int(env.get("MGX_BC_LANE_MAX", 16)), int(env.get("MGX_BC_HUGE_MIN", 8192)), int(env.get("MGX_BC_SEG", 8192))
    n, ro, ci, _ = oracle.rmat_csr(12, 16, 12)
    d = np.diff(ro)
    assert ((d >= huge_min) & (d % seg != 0)).any() or huge_min > d.max()         # a huge row that is no multiple of the segment
    af, sf, want, info = _check(gpu_ctx, ro, ci, _sources(ro, 12), True)
    lane, wave, huge, segs = _class_counts(ro, lane_max, huge_min, seg)
    assert (info["in_lane"], info["in_wave"], info["in_huge"], info["in_segments"]) == (lane, wave, huge, segs), info
    assert (info["lane_max"], info["huge_min"], info["seg"], info["chain"]) == (lane_max, huge_min, seg, 1024), info
    if "MGX_BC_HUGE_MIN" in env:
        assert huge > 0 and segs > huge
    # directed with a CSC: the in-rows and the out-rows have classes of their own
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 112, undir=False)
    af, sf, want, info = _check(gpu_ctx, ro, ci, _sources(ro, 13), False, csc=True)
    iro = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))])
    assert (info["in_lane"], info["in_wave"], info["in_huge"], info["in_segments"]) == _class_counts(iro, lane_max, huge_min, seg), info
    assert (info["out_lane"], info["out_wave"], info["out_huge"], info["out_segments"]) == _class_counts(ro, lane_max, huge_min, seg), info
    # 1024 vertices: every level is small, the chain folds the wave rows and the huge rows too -- exactly as the grid kernels do
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(10, 16, 10)
    src = _sources(ro, 10)
    af, sf, want, info = _check(gpu_ctx, ro, ci, src, True)
    assert sf["chain_launches"] > 0
    monkeypatch.setenv("MGX_BC_CHAIN", "0")
    g = _graph(gpu_ctx, ro, ci)
    bp = mini_amd.BcProblem(g)
    assert bp.run(src, True)["chain_launches"] == 0
    _bit_equal("chain off against chain on", _arrays(bp), af)
    bp.close()
    g.close()


def test_star_default_thresholds(gpu_ctx):
    """a star of 100 001 vertices under the defaults: the centre's row is cut into 13 segments"""
    k = 100000
    ro, ci = cm.csr(k + 1, np.zeros(k, dtype=np.int64), 1 + np.arange(k))
    want = model.run(ro, ci, [0, 5], True)
    af, sf, _, info = _check(gpu_ctx, ro, ci, np.array([0, 5], dtype=np.int32), True, want=want)
    assert info["in_huge"] == 1 and info["in_segments"] == 13 and info["in_lane"] == k and info["in_wave"] == 0, info
    # from the centre nothing lies between; from a leaf the centre carries the other k - 1 leaves
    assert af["bc"][0] == k - 1 and not af["bc"][1:].any()
    assert af["sigma"][0] == 1 and af["delta"][0] == k - 1 and (af["sigma"][1:] == 1).all()


# ---- depth ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["path300", "path5000", "grid29"])
def test_depth_with_and_without_the_chain(gpu_ctx, monkeypatch, case):
    import mini_amd
    from math import comb
    ro, ci = {"path300": lambda: _path(300), "path5000": lambda: _path(5000), "grid29": lambda: _grid(29)}[case]()
    src = np.array([0], dtype=np.int32)
    want = model.run(ro, ci, src, True)
    af, sf, _, info = _check(gpu_ctx, ro, ci, src, True, want=want)
    assert sf["chain_launches"] > 0 and info["chain_launches"] > 0, (sf, info)
    if case == "grid29":
        assert af["sigma"].max() == float(comb(56, 28)) and sf["levels"] == 57 and sf["inexact"] == 0
    else:
        assert sf["levels"] == len(ro) - 1 and (af["sigma"] == 1).all()
    monkeypatch.setenv("MGX_BC_CHAIN", "0")
    g = _graph(gpu_ctx, ro, ci)
    bp = mini_amd.BcProblem(g)
    s0 = bp.run(src, True)
    _bit_equal("chain off against chain on", _arrays(bp), af)
    assert s0["chain_launches"] == 0 and bp.info()["chain"] == 0 and s0["host_waits"] == 1, s0
    assert s0["launches"] > sf["launches"]
    bp.close()
    g.close()


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 6])
def test_graph_without_entries(gpu_ctx, n):
    ro, ci = np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    af, sf, _, _ = _check(gpu_ctx, ro, ci, None, True)
    assert not af["bc"].any() and sf["levels"] == 1 and sf["reached"] == n


def test_sources_without_a_way_out(gpu_ctx):
    """a source with no out-entries; a source whose only entry is a self-loop; two components"""
    #   0 -> 1 -> 2 -> 3,  4 (nothing),  5 -> 5,  6 <-> 7 <-> 8
    s = [0, 1, 2, 5, 6, 7, 7, 8]
    d = [1, 2, 3, 5, 7, 6, 8, 7]
    ro, ci = cm.csr(9, s, d, symmetric=False)
    for src in ([4], [5], [3], [0], [6], None):
        af, sf, want, _ = _check(gpu_ctx, ro, ci, None if src is None else np.array(src, dtype=np.int32), False, csc=True)
        if src in ([4], [5], [3]):
            assert sf["levels"] == 1 and sf["reached"] == 1 and not af["bc"].any() and af["sigma"].sum() == 1
    assert np.array_equal(af["bc"], np.array([0, 2, 2, 0, 0, 0, 0, 2, 0], dtype=np.float64))


def test_tripled_entries(gpu_ctx):
    """every entry three times: sigma grows by powers of 3 along a path while the path's bc stays the same"""
    n = 20
    a = np.arange(n - 1)
    ro, ci = cm.csr(n, np.tile(a, 3), np.tile(a + 1, 3))
    af, sf, want, _ = _check(gpu_ctx, ro, ci, None, True)
    # (sigma[v] / sigma[w] = 1 / 3 is rounded: the simple path's values within the case's own bound, the zeros exactly)
    _close("tripled path against the simple path's closed form", af["bc"], 2.0 * np.arange(n) * (n - 1 - np.arange(n)),
           model.rtol(want["stats"][1], want["longest_out"], n))
    assert np.array_equal(af["sigma"], 3.0 ** (n - 1 - np.arange(n)))             # the last source is n - 1


def test_grid31_sets_inexact(gpu_ctx):
    import mini_amd
    ro, ci = _grid(31)
    g = _graph(gpu_ctx, ro, ci)
    bp = mini_amd.BcProblem(g)
    for go in (bp.run, bp.enact):
        st = go(np.array([0], dtype=np.int32), True)
        assert st["inexact"] == 1 and st["overflow"] == 0 and st["levels"] == 61, st
    bp.close()
    g.close()


def test_count_zero_statuses_and_operator_first(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(12, 4, 12)
    g = _graph(gpu_ctx, ro, ci)
    bp = mini_amd.BcProblem(g)
    for getter in (bp.centrality, bp.sigma, bp.delta, bp.labels, bp.info, bp.centrality_device_ptr):
        with pytest.raises(mini_amd.MgxError):
            getter()                                                       # before any run
    with pytest.raises(mini_amd.MgxError) as e:
        bp.run(None, False)                                                # no CSC
    assert e.value.status == mini_amd.MGX_E_INVALID
    for bad in ([n], [-1], [0, n + 5]):
        for go in (bp.run, bp.enact):
            with pytest.raises(mini_amd.MgxError) as e:
                go(np.array(bad, dtype=np.int32), True)
            assert e.value.status == mini_amd.MGX_E_INVALID
    import ctypes as C
    assert mini_amd.lib.mgx_bc_run(bp._h, np.zeros(1, dtype=np.int32).ctypes.data_as(C.c_void_p), -1, 1, None) == mini_amd.MGX_E_INVALID
    with pytest.raises(mini_amd.MgxError):
        bp.centrality()                                                    # still no run
    st = bp.run(np.zeros(0, dtype=np.int32), True)                         # count == 0: a valid run, bc all zero
    assert st["sources"] == 0 and not bp.centrality().any() and bp.centrality_device_ptr()
    # the operator path first on a fresh handle, then the fused path
    src = _sources(ro, 3)
    want = model.run(ro, ci, src, True)
    rtol = model.rtol(want["stats"][1], want["longest_out"], len(src))
    fresh = mini_amd.BcProblem(g)
    fresh.enact(src, True)
    ao = _arrays(fresh)
    sf = fresh.run(src, True)
    af = _arrays(fresh)
    _same("operator first against model", ao, want, rtol)
    _same("fused second against operator", af, ao, rtol)
    assert sf["host_waits"] == 1
    fresh.close()
    bp.close()
    g.close()


def test_another_stream(gpu_ctx, oracle, torch_mod):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(13, 8, 41)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _check(ctx, ro, ci, _sources(ro, 41), True, layout=True)
    finally:
        ctx.close()
