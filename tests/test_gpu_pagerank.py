"""GPU suite (-m gpu): PageRank to convergence (mgx_pagerank_*).  The fused path (mgx_pagerank_run, on the layout's
sliced kernels and on the general reduce) and the operator path (mgx_pagerank_enact) against the float64 model
(tests/pagerank_model.py).

Parity at a fixed iteration count is np.allclose(got, want, rtol=R, atol=0) with

    R = max(2e-5, 0.5 * 6e-8 * dmax_in) / (1 - alpha)

the project's tolerance for one float neighbour-reduce (tests/test_gpu_parity.py) times how far an error per iteration can grow in
a contraction of factor alpha; dmax_in is the longest in-row.  atol is 0: every rank is at least (1 - alpha) / n > 0.  The exact
cases (regular graphs, power-of-two degrees) are compared bit for bit."""
import math
import os

import numpy as np
import pytest

from tests import coloring_model as cm
from tests import pagerank_model as model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
FIRST_BATCH, MIN_BATCH = 32, 8                 # include/mgx/pagerank_fused.hpp: PGR_FIRST_BATCH, PGR_MIN_BATCH


def _graph(ctx, ro, ci, csc=False, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if csc:
        g.build_csc()
    if layout:
        g.build_layout()
    return g


def _dmax_in(ro, ci, symmetric):
    n = len(ro) - 1
    if len(ci) == 0:
        return 0
    return int(np.diff(ro).max()) if symmetric else int(np.bincount(ci, minlength=n).max())


def _rtol(dmax_in, alpha):
    return max(2e-5, 0.5 * 6e-8 * dmax_in) / (1.0 - alpha)


def _compare(tag, got, st, res, want, want_res, R, T):
    """every vertex against the model; the sum; the iteration count; the residuals that float32 rounding does not reach"""
    assert got.dtype == np.float32 and got.shape == want.shape
    rel = np.abs(got.astype(np.float64) - want) / want
    print("%s: max rel %.3g (R %.3g) sum-1 %.3g iterations %d residual %.3g" % (
        tag, rel.max(), R, float(got.astype(np.float64).sum()) - 1.0, st["iterations"], st["residual"]))
    assert np.allclose(got, want, rtol=R, atol=0), "%s: %d of %d ranks outside rtol %.3g (max %.3g)" % (
        tag, int((rel > R).sum()), len(want), R, rel.max())
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 2e-5, tag
    # tol = 0: the run makes T iterations unless float32 reached an exact fixed point (then later iterations change nothing)
    assert st["iterations"] == T or (st["converged"] == 1 and st["residual"] == 0.0 and st["iterations"] < T), (tag, st)
    assert len(res) == st["iterations"] and res[-1] == st["residual"], (tag, st, len(res))
    for t in range(min(len(res), len(want_res))):
        if want_res[t] >= 1e-4:
            assert abs(res[t] - want_res[t]) <= 1e-2 * want_res[t], (tag, t, res[t], want_res[t])


def _check(ctx, ro, ci, symmetric, csc=False, layout=False, alpha=0.85, T=20, want_layout_path=None):
    """fused and operator path against the model after T iterations (tol = 0); returns the fused ranks"""
    import mini_amd
    want, want_res = model.ranks(ro, ci, alpha, 0.0, T, symmetric)
    R = _rtol(_dmax_in(ro, ci, symmetric), alpha)
    g = _graph(ctx, ro, ci, csc, layout)
    pp = mini_amd.PageRankProblem(g)
    sf = pp.run(alpha, 0.0, T, symmetric)
    rf, ef = pp.ranks(), pp.residuals()
    so = pp.enact(alpha, 0.0, T, symmetric)
    r_o, eo = pp.ranks(), pp.residuals()
    _compare("fused", rf, sf, ef, want, want_res, R, T)
    _compare("operator", r_o, so, eo, want, want_res, R, T)
    dangling = int((np.diff(ro) == 0).sum())
    assert sf["dangling"] == dangling and so["dangling"] == dangling
    assert sf["host_waits"] == 1 if T <= FIRST_BATCH else sf["host_waits"] <= 1 + math.ceil((T - FIRST_BATCH) / MIN_BATCH)
    assert so["host_waits"] >= so["iterations"] and so["layout_path"] == 0
    built = g.nr_slices_info()["mini_units"] > 0
    assert sf["layout_path"] == int(bool(layout and symmetric and built)), (sf, g.nr_slices_info())
    if want_layout_path is not None:
        assert sf["layout_path"] == want_layout_path, (sf, g.nr_slices_info())
    pp.close()
    g.close()
    return rf


# ---- parity at a fixed iteration count ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
def test_fixtures(gpu_ctx, oracle, name, undir):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check(gpu_ctx, ro, ci, symmetric=undir, csc=not undir)


@pytest.mark.parametrize("scale,ef", [(10, 1), (11, 2), (12, 4), (13, 8), (14, 16), (15, 1), (16, 16)])
@pytest.mark.parametrize("layout", [False, True])
def test_rmat_symmetric(gpu_ctx, oracle, scale, ef, layout):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale)
    # (the edge factor 16 graphs have rows of hundreds of entries: the layout carries unit blocks, the slices are built)
    _check(gpu_ctx, ro, ci, symmetric=True, layout=layout, want_layout_path=1 if layout and ef == 16 else None)


@pytest.mark.parametrize("scale,ef", [(10, 2), (12, 4), (14, 8), (16, 1)])
def test_rmat_directed_with_csc(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    _check(gpu_ctx, ro, ci, symmetric=False, csc=True)


@pytest.mark.parametrize("alpha", [0.5, 0.85, 0.99])
@pytest.mark.parametrize("layout", [False, True])
def test_dampings(gpu_ctx, oracle, alpha, layout):
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 7)
    _check(gpu_ctx, ro, ci, symmetric=True, layout=layout, alpha=alpha)


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    import mini_amd
    ro, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    g = _graph(gpu_ctx, ro, ci)
    pp = mini_amd.PageRankProblem(g)
    for go in (pp.run, pp.enact):
        for tol in (0.0, 1e-6):
            st = go(0.85, tol, 20, True)
            assert st["iterations"] == 1 and st["converged"] == 1 and st["residual"] == 0.0 and st["dangling"] == n, st
            assert np.array_equal(pp.ranks(), np.full(n, np.float32(1.0 / n)))
            assert np.array_equal(pp.residuals(), [0.0])
    pp.close()
    g.close()


def test_self_loops_and_duplicates(gpu_ctx):
    n = 3000
    v = np.arange(n)
    ro, ci = cm.csr(n, v, v, symmetric=False)                             # self-loops only: a self-loop is its own reverse
    r = _check(gpu_ctx, ro, ci, True)
    assert np.array_equal(r, np.full(n, np.float32(1.0 / n)))
    rng = np.random.default_rng(4)
    s, d = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    s, d = np.concatenate([s, s, s, v[::7]]), np.concatenate([d, d, d, v[::7]])   # every pair three times, some self-loops
    ro, ci = cm.csr(n, s, d)
    _check(gpu_ctx, ro, ci, True)
    ro, ci = cm.csr(n, s, d, symmetric=False)
    _check(gpu_ctx, ro, ci, False, csc=True)


@pytest.mark.parametrize("centre", [0, 77777])
def test_star_long_row(gpu_ctx, centre):
    n = 100001
    leaves = np.setdiff1d(np.arange(n), [centre])
    ro, ci = cm.csr(n, np.full(len(leaves), centre), leaves)
    assert ro[centre + 1] - ro[centre] == 100000
    for layout in (False, True):
        _check(gpu_ctx, ro, ci, True, layout=layout)
    ro, ci = cm.csr(n, np.full(len(leaves), centre), leaves, symmetric=False)   # only the centre's row: 100 000 dangling leaves
    assert int((np.diff(ro) == 0).sum()) == 100000
    _check(gpu_ctx, ro, ci, False, csc=True)
    ro, ci = cm.csr(n, leaves, np.full(len(leaves), centre), symmetric=False)   # the reverse: one in-row of 100 000 entries
    _check(gpu_ctx, ro, ci, False, csc=True)


def test_shuffled_path(gpu_ctx):
    n = 200000
    p = np.random.default_rng(8).permutation(n)
    ro, ci = cm.csr(n, p[:-1], p[1:])
    _check(gpu_ctx, ro, ci, True)
    ro, ci = cm.csr(n, p[:-1], p[1:], symmetric=False)                     # directed: one out-entry a row, the last vertex dangles
    _check(gpu_ctx, ro, ci, False, csc=True)


def test_two_cliques_joined_by_one_entry(gpu_ctx):
    k = 300
    rng = np.random.default_rng(2)
    ids = rng.permutation(2 * k + 50)
    a, b = ids[:k], ids[k:2 * k]
    s = np.concatenate([np.repeat(a, k), np.repeat(b, k)])
    d = np.concatenate([np.tile(a, k), np.tile(b, k)])
    n = len(ids)
    ro, ci = cm.csr(n, np.concatenate([s, [a[5]]]), np.concatenate([d, [b[7]]]), symmetric=False)
    _check(gpu_ctx, ro, ci, False, csc=True)
    ro, ci = cm.csr(n, np.concatenate([s, [a[5]]]), np.concatenate([d, [b[7]]]))
    for layout in (False, True):
        _check(gpu_ctx, ro, ci, True, layout=layout)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def _circulant(n, d):
    v = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(1, d // 2 + 1, dtype=np.int64)[None, :]
    ci = np.sort(np.concatenate([(v + k) % n, (v - k) % n], axis=1), axis=1).astype(np.int32).ravel()
    return (np.arange(n + 1, dtype=np.int64) * d).astype(np.int32), ci


@pytest.mark.parametrize("n,d", [(1 << 16, 16), (1 << 16, 128), (1 << 13, 4096)])
@pytest.mark.parametrize("layout", [False, True])
def test_regular_graph_is_exact(gpu_ctx, n, d, layout):
    """every term is the same power of two: whatever the order of the sums every rank is exactly 1 / n, every residual exactly 0"""
    import mini_amd
    ro, ci = _circulant(n, d)
    g = _graph(gpu_ctx, ro, ci, layout=layout)
    pp = mini_amd.PageRankProblem(g)
    want = np.full(n, np.float32(1.0 / n))
    for go in (pp.run, pp.enact):
        for tol in (0.0, 1e-6):
            st = go(0.5, tol, 20, True)
            assert st["iterations"] == 1 and st["converged"] == 1 and st["residual"] == 0.0 and st["dangling"] == 0, st
            got = pp.ranks()
            assert np.array_equal(got, want), int((got != want).sum())
            assert np.array_equal(pp.residuals(), [0.0])
    pp.close()
    g.close()


def _padded_to_powers_of_two(ro, ci):
    """every row padded with self-loops to the next power of two, empty rows to one entry"""
    n = len(ro) - 1
    deg = np.diff(ro).astype(np.int64)
    target = np.where(deg > 0, 1 << np.ceil(np.log2(np.maximum(deg, 1))).astype(np.int64), 1)
    assert ((target & (target - 1)) == 0).all() and (target >= deg).all() and (target >= 1).all()
    rows = np.repeat(np.arange(n), deg)
    pad = np.repeat(np.arange(n), target - deg)
    return cm.csr(n, np.concatenate([rows, pad]), np.concatenate([ci, pad]), symmetric=False)


@pytest.mark.parametrize("directed,layout", [(False, False), (False, True), (True, False)])      # (a layout over the CSC is out of scope)
def test_one_iteration_on_power_of_two_rows_is_exact(gpu_ctx, oracle, directed, layout):
    """alpha = 1/2, one iteration: every contribution is 2^-12 over a power of two, so every partial sum in any order and the update
    are exact in float32 as long as 2 * (longest in-row) * (longest out-row) <= 2^24"""
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(12, 4, 12, undir=not directed)
    ro, ci = _padded_to_powers_of_two(ro, ci)
    out_max = int(np.diff(ro).max())
    in_max = int(np.bincount(ci, minlength=n).max())
    assert (np.diff(ro) > 0).all() and 2 * in_max * out_max <= 1 << 24, (in_max, out_max)
    want, want_res = model.ranks(ro, ci, 0.5, 0.0, 1, not directed)
    want32 = want.astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want)                 # the model's r_1 is a float32 already
    g = _graph(gpu_ctx, ro, ci, csc=directed, layout=layout)
    pp = mini_amd.PageRankProblem(g)
    for go in (pp.run, pp.enact):
        st = go(0.5, 0.0, 1, not directed)
        assert st["iterations"] == 1 and st["dangling"] == 0
        got = pp.ranks()
        assert np.array_equal(got, want32), int((got != want32).sum())
    pp.close()
    g.close()


# ---- residuals and stopping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["general", "layout", "directed"])
def test_residuals_and_stopping(gpu_ctx, oracle, kind):
    import mini_amd
    directed = kind == "directed"
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 5, undir=not directed)
    sym = not directed
    _, res = model.ranks(ro, ci, 0.85, 0.0, 60, sym)
    T = int(np.nonzero(res >= 3e-4)[0][-1]) + 1                           # the last T with e_T >= 3e-4 (e_T = res[T - 1])
    assert T + 1 <= len(res)
    tol = float(np.sqrt(res[T - 1] * res[T]))
    g = _graph(gpu_ctx, ro, ci, csc=directed, layout=kind == "layout")
    pp = mini_amd.PageRankProblem(g)
    for go in (pp.run, pp.enact):
        st = go(0.85, tol, 100, sym)
        got = pp.residuals()
        print(kind, go.__name__, "T", T, "tol", tol, st, "ratio", res[T] / res[T - 1])
        assert st["iterations"] == T + 1 and st["converged"] == 1 and st["residual"] <= tol and len(got) == T + 1, (st, T, tol)
        for t in range(T + 1):
            if res[t] >= 1e-4:
                assert abs(got[t] - res[t]) <= 1e-2 * res[t], (t, got[t], res[t])
        st = go(0.85, 0.0, 3, sym)
        assert st["iterations"] == 3 and st["converged"] == 0 and len(pp.residuals()) == 3, st
    if kind == "layout":
        assert pp.run(0.85, tol, 100, sym)["layout_path"] == 1
    pp.close()
    g.close()


# ---- fused-path properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [False, True])
def test_runs_are_bit_equal_and_paths_alternate(gpu_ctx, oracle, layout):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(15, 16, 3)
    want, _ = model.ranks(ro, ci, 0.85, 0.0, 20, True)
    R = _rtol(_dmax_in(ro, ci, True), 0.85)
    g = _graph(gpu_ctx, ro, ci, layout=layout)
    pp = mini_amd.PageRankProblem(g)
    s1 = pp.run(0.85, 0.0, 20, True)
    r1, e1 = pp.ranks(), pp.residuals()
    s2 = pp.run(0.85, 0.0, 20, True)
    assert s1 == s2 and s1["layout_path"] == int(layout) and s1["host_waits"] == 1
    assert np.array_equal(r1, pp.ranks()) and np.array_equal(e1, pp.residuals())
    so = pp.enact(0.85, 0.0, 20, True)
    ro1 = pp.ranks()
    assert np.allclose(ro1, want, rtol=R, atol=0) and so["host_waits"] >= 20
    s3 = pp.run(0.85, 0.0, 20, True)                                      # a run after an enact ...
    assert s3 == s1 and np.array_equal(r1, pp.ranks()) and np.array_equal(e1, pp.residuals())
    pp.enact(0.85, 0.0, 20, True)                                         # ... and the reverse
    assert np.allclose(pp.ranks(), want, rtol=R, atol=0)
    # more iterations than the first batch holds: a look per batch
    s4 = pp.run(0.85, 0.0, 48, True)
    assert s4["iterations"] == 48 and 2 <= s4["host_waits"] <= 1 + math.ceil((48 - FIRST_BATCH) / MIN_BATCH), s4
    s5 = pp.run(0.85, 1e-6, 100, True)
    assert s5["converged"] == 1 and s5["host_waits"] <= 1 + math.ceil((100 - FIRST_BATCH) / MIN_BATCH), s5
    assert pp.ranks_device_ptr()
    pp.close()
    g.close()


def test_errors(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(10, 4, 1, undir=False)
    g = _graph(gpu_ctx, ro, ci)
    pp = mini_amd.PageRankProblem(g)
    for call in (pp.ranks, pp.ranks_device_ptr, pp.residuals):
        with pytest.raises(mini_amd.MgxError):
            call()
    bad = [dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=float("nan")), dict(tol=float("nan")), dict(tol=-1.0),
           dict(tol=float("inf")), dict(max_iter=0)]
    for go in (pp.run, pp.enact):
        for kw in bad:
            args = dict(alpha=0.85, tol=1e-6, max_iter=10, symmetric=True)
            args.update(kw)
            with pytest.raises(mini_amd.MgxError) as ei:
                go(**args)
            assert ei.value.status == mini_amd.MGX_E_INVALID, kw
        with pytest.raises(mini_amd.MgxError) as ei:                       # no genuine CSC: no silent wrong answer
            go(0.85, 1e-6, 10, False)
        assert ei.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(ei.value)
    with pytest.raises(mini_amd.MgxError):                                 # the refused calls were no runs
        pp.ranks()
    g.build_csc()
    st = pp.run(0.85, 0.0, 20, False)
    assert st["iterations"] == 20 and st["converged"] == 0
    want, _ = model.ranks(ro, ci, 0.85, 0.0, 20, False)
    assert np.allclose(pp.ranks(), want, rtol=_rtol(_dmax_in(ro, ci, False), 0.85), atol=0)
    pp.close()
    g.close()


def test_non_default_stream(gpu_ctx, oracle, torch_mod):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 41)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        for layout in (False, True):
            _check(ctx, ro, ci, True, layout=layout)
        n, ro, ci, _ = oracle.rmat_csr(12, 8, 42, undir=False)
        _check(ctx, ro, ci, False, csc=True)
    finally:
        ctx.close()


# ---- full size -------------------------------------------------------------------------------------------------------------------
def test_rmat20_against_model(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(20, 16, 20)
    _check(gpu_ctx, ro, ci, True, layout=True, T=10, want_layout_path=1)


def test_rmat22_fused_operator_and_an_independent_step(gpu_ctx, torch_mod):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    torch = torch_mod
    alpha, T = 0.85, 20
    d = rmat_csr(gpu_ctx, 22, 16)
    g = mini_amd.Graph.from_device(gpu_ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    g.build_layout()
    pp = mini_amd.PageRankProblem(g)
    sf = pp.run(alpha, 0.0, T, True)
    rf = pp.ranks()
    so = pp.enact(alpha, 0.0, T, True)
    r_o = pp.ranks()
    n = d["n"]
    ro = d["row_offsets"].long()
    deg = ro[1:] - ro[:-1]
    dmax = int(deg.max().item())
    eps = max(2e-5, 0.5 * 6e-8 * dmax)
    R = eps / (1.0 - alpha)
    rel = np.abs(rf.astype(np.float64) - r_o.astype(np.float64)) / r_o.astype(np.float64)
    print("rmat22: dmax %d R %.3g fused vs operator max rel %.3g; %s" % (dmax, R, rel.max(), sf))
    assert sf["layout_path"] == 1 and sf["iterations"] == T and so["iterations"] == T and sf["host_waits"] == 1
    assert np.allclose(rf, r_o, rtol=R, atol=0)
    assert abs(float(rf.astype(np.float64).sum()) - 1.0) <= 2e-5
    # one step of the definition, computed by torch in float64 from the returned ranks: an alpha-contraction in L1, and r_T is the
    # rounded step of r_{T-1}, so |step(r_T) - r_T|_1 <= alpha * e_T + eps
    dev = d["row_offsets"].device
    r = torch.from_numpy(rf).to(dev).double()
    rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64), deg)
    cols = d["col_indices"].long()
    contrib = torch.where(deg > 0, r / deg.clamp(min=1).double(), torch.zeros_like(r))
    S = torch.zeros(n, device=dev, dtype=torch.float64)
    S.scatter_add_(0, cols, contrib[rows])                                 # entry (u, v): u = rows, v = cols
    D = r[deg == 0].sum()
    nxt = (1.0 - alpha) / n + alpha * (S + D / n)
    gap = float((nxt - r).abs().sum().item())
    print("rmat22: |step(r_T) - r_T|_1 = %.3g, alpha e_T + eps = %.3g" % (gap, alpha * sf["residual"] + eps))
    assert gap <= alpha * sf["residual"] + eps
    pp.close()
    g.close()
