"""GPU suite (-m gpu): graph colouring (mgx_color_*).  The fused path (mgx_color_run), the operator path
(mgx_color_enact) and the numpy model (tests/coloring_model.py) agree bit for bit -- colours, per-round active counts and
stats -- on the reference's colouring fixture, R-MAT 10-16 with duplicates and self-loops, hand-made shapes and, at full size,
RMAT-20 / RMAT-22."""
import math
import os

import numpy as np
import pytest

from tests import coloring_model as model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _graph(ctx, ro, ci, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if layout:
        g.build_layout()
    return g


def _check(ctx, ro, ci, seed=model.SEED, max_iter=model.MAX_ITER, layout=False, want=None):
    """fused == operator path == model; returns the colours"""
    import mini_amd
    g = _graph(ctx, ro, ci, layout)
    cp = mini_amd.ColorProblem(g)
    sf = cp.run(seed, max_iter)
    cf, tf = cp.colors(), cp.round_trace()
    so = cp.enact(seed, max_iter)
    co, to = cp.colors(), cp.round_trace()
    wc, wt, left = want if want is not None else model.color(ro, ci, seed, max_iter)
    assert np.array_equal(cf, wc), "fused: %d of %d colours differ" % (int((cf != wc).sum()), len(wc))
    assert np.array_equal(co, wc), "operator path: %d of %d colours differ" % (int((co != wc).sum()), len(wc))
    assert np.array_equal(tf, wt) and np.array_equal(to, wt)
    for st in (sf, so):
        assert st["rounds"] == len(wt) and st["uncolored"] == left
        assert st["max_color"] == (int(wc.max()) if len(wc) else 0)
    cp.close()
    g.close()
    return wc


@pytest.mark.parametrize("seed,max_iter", [(31, 10), (31, 0), (model.SEED, 10), (model.SEED, 0)])
def test_reference_fixture(gpu_ctx, oracle, seed, max_iter):
    """the reference's colouring fixture (tests/coloring/test.mtx == tests/golden/pr_test.mtx), symmetrised as its driver loads it"""
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, "pr_test.mtx"), undir=True)
    c = _check(gpu_ctx, ro, ci, seed, max_iter)
    assert model.conflicts(ro, ci, c) == 0


@pytest.mark.parametrize("scale,ef,seed", [(10, 16, 10), (11, 4, 11), (12, 8, 12), (13, 16, 13), (14, 2, 14), (16, 16, 16)])
def test_rmat(gpu_ctx, oracle, scale, ef, seed):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, seed)
    c = _check(gpu_ctx, ro, ci, seed=seed, max_iter=0)
    assert (c > 0).all() and model.conflicts(ro, ci, c) == 0
    # max_iter = 3 leaves exactly the model's uncoloured set
    c3 = _check(gpu_ctx, ro, ci, seed=seed, max_iter=3)
    assert np.array_equal(c3 == 0, c > 6)


def test_graph_without_entries(gpu_ctx):
    ro, ci = np.zeros(101, np.int32), np.zeros(0, np.int32)
    c = _check(gpu_ctx, ro, ci, max_iter=0)
    assert (c == 1).all()


def test_isolated_vertices_and_a_self_loop(gpu_ctx):
    rng = np.random.default_rng(5)
    n = 2000
    s, d = rng.integers(0, n // 2, 3000), rng.integers(0, n // 2, 3000)   # the upper half has no entries
    s = np.concatenate([s, [n - 1]])
    d = np.concatenate([d, [n - 1]])                                      # vertex n - 1: a self-loop only
    ro, ci = model.csr(n, s, d)
    c = _check(gpu_ctx, ro, ci, max_iter=0)
    assert (c[n // 2:] == 1).all() and model.conflicts(ro, ci, c) == 0


def test_star_long_row(gpu_ctx):
    leaves = 200000
    ro, ci = model.csr(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))
    for max_iter in (0, 1):
        c = _check(gpu_ctx, ro, ci, max_iter=max_iter)
    assert model.conflicts(ro, ci, c) == 0


def test_clique_512(gpu_ctx):
    ro, ci = model.clique(512)
    for layout in (False, True):
        c = _check(gpu_ctx, ro, ci, seed=3, max_iter=0, layout=layout)
        assert len(np.unique(c)) == 512
    import mini_amd
    g = _graph(gpu_ctx, ro, ci)
    cp = mini_amd.ColorProblem(g)
    assert cp.run(3, 0)["rounds"] == 256
    cp.close()


def test_path(gpu_ctx):
    n = 100000
    ro, ci = model.csr(n, np.arange(n - 1), np.arange(1, n))
    c = _check(gpu_ctx, ro, ci, max_iter=0)
    assert model.conflicts(ro, ci, c) == 0


def test_directed_ragged(gpu_ctx):
    """not symmetric, rows from 0 to 300 entries, duplicates: the rule on out-rows, model equality only"""
    rng = np.random.default_rng(11)
    n = 5000
    deg = rng.integers(0, 12, size=n)
    deg[rng.integers(0, n, 40)] = rng.integers(40, 300, 40)
    deg[rng.integers(0, n, 300)] = 0
    ro = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, n, size=int(ro[-1])).astype(np.int32)
    for max_iter in (0, 4):
        _check(gpu_ctx, ro, ci, seed=77, max_iter=max_iter)


def test_layout_stream_and_repeat(gpu_ctx, oracle, torch_mod):
    """with and without the layout, on a non-default stream, twice with one seed: the same colours"""
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 99)
    want = model.color(ro, ci, 5, 0)
    a = _check(gpu_ctx, ro, ci, seed=5, max_iter=0, want=want)
    b = _check(gpu_ctx, ro, ci, seed=5, max_iter=0, layout=True, want=want)
    assert np.array_equal(a, b)
    torch = torch_mod
    s = torch.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        c = _check(ctx, ro, ci, seed=5, max_iter=0, want=want)
        assert np.array_equal(a, c)
        g = _graph(ctx, ro, ci)
        cp = mini_amd.ColorProblem(g)
        st1 = cp.run(5, 0)
        c1, t1 = cp.colors(), cp.round_trace()
        st2 = cp.run(5, 0)
        assert st1 == st2 and np.array_equal(c1, cp.colors()) and np.array_equal(t1, cp.round_trace())
        cp.close()
        g.close()
    finally:
        ctx.close()


def test_colors_before_any_run_is_invalid(gpu_ctx):
    import mini_amd
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    cp = mini_amd.ColorProblem(g)
    with pytest.raises(mini_amd.MgxError):
        cp.colors()
    assert len(cp.round_trace()) == 0
    cp.close()


def test_rmat20_against_model(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(20, 16, 20)
    for max_iter in (model.MAX_ITER, 0):
        c = _check(gpu_ctx, ro, ci, max_iter=max_iter, layout=True)
    assert (c > 0).all() and model.conflicts(ro, ci, c) == 0


def _device_proper(torch, ro, ci, colours):
    """one vectorised pass on the device: no entry (v, u), u != v, with one non-zero colour at both ends"""
    n = ro.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, device=ro.device, dtype=torch.int32), (ro[1:] - ro[:-1]).long())
    c = colours
    cu = c[ci.long()]
    cv = c[rows.long()]
    return int(((rows != ci) & (cv == cu) & (cv != 0)).sum().item()) == 0 and bool((c > 0).all().item())


def _device_graph(ctx, d, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    if layout:
        g.build_layout()
    return g


def test_rmat22_fused_equals_operator_path(gpu_ctx, torch_mod):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    torch = torch_mod
    d = rmat_csr(gpu_ctx, 22, 16)
    g = _device_graph(gpu_ctx, d, layout=True)
    cp = mini_amd.ColorProblem(g)
    sf = cp.run(model.SEED, 0)
    cf, tf = cp.colors(), cp.round_trace()
    so = cp.enact(model.SEED, 0)
    co, to = cp.colors(), cp.round_trace()
    assert np.array_equal(cf, co) and np.array_equal(tf, to)
    assert {k: sf[k] for k in ("rounds", "uncolored", "max_color")} == {k: so[k] for k in ("rounds", "uncolored", "max_color")}
    assert sf["uncolored"] == 0 and sf["rounds"] <= math.ceil(d["n"] / 2)
    assert sf["host_waits"] < sf["rounds"]                  # the fused path does not wait once per round
    assert _device_proper(torch, d["row_offsets"], d["col_indices"], torch.from_numpy(cf).to(d["row_offsets"].device))
    cp.close()
    g.close()


@pytest.mark.parametrize("kind", ["uniform", "grid2d"])
def test_scale18_uniform_grid_proper_and_complete(gpu_ctx, torch_mod, kind):
    import mini_amd
    from mini_amd.rmat import grid2d_csr, uniform_csr
    torch = torch_mod
    d = (uniform_csr if kind == "uniform" else grid2d_csr)(gpu_ctx, 18)
    g = _device_graph(gpu_ctx, d)
    cp = mini_amd.ColorProblem(g)
    st = cp.run(model.SEED, 0)
    c = cp.colors()
    assert st["uncolored"] == 0
    assert _device_proper(torch, d["row_offsets"], d["col_indices"], torch.from_numpy(c).to(d["row_offsets"].device))
    so = cp.enact(model.SEED, 0)
    assert np.array_equal(cp.colors(), c) and so["rounds"] == st["rounds"]
    cp.close()
    g.close()
