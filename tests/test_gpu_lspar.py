"""GPU suite (-m gpu): local sparsification (mgx_lspar_*).  The fused path (mgx_lspar_run), the operator path
(mgx_lspar_enact) and the numpy model (tests/lspar_model.py) agree bit for bit -- the four result arrays and the minhash table --
on the reference's lspar fixture, R-MAT 10-16 with duplicates and self-loops, hand-made shapes and, at full size, RMAT-20 / 22."""
import os

import numpy as np
import pytest

from tests import lspar_model as model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KS = [1, 4, 8, 32]
ES = [0.0, 0.25, 0.5, 1.0]
FULL = [(k, e) for k in KS for e in ES]
DIAGONAL = list(zip(KS, ES))


def _graph(ctx, ro, ci, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if layout:
        g.build_layout()
    return g


def _same(got, want, what):
    for name, a, b in zip(("out_ro", "out_ci", "out_eid", "out_sim"), got, want):
        assert np.array_equal(a, b), "%s: %s differs in %d of %d" % (what, name, int((np.asarray(a) != np.asarray(b)).sum())
                                                                    if len(a) == len(b) else -1, len(b))


def _check(ctx, ro, ci, params, layout=False, seed=model.SEED):
    """fused == operator path == model for every (k, e) in params"""
    import mini_amd
    g = _graph(ctx, ro, ci, layout)
    lp = mini_amd.LsparProblem(g)
    d = np.diff(ro.astype(np.int64))
    for k, e in params:
        want = model.sparsify(ro, ci, seed, k, e)
        t = model.keep_count(d, e)
        for path in (lp.run, lp.enact):
            st = path(seed, k, e)
            what = "%s k=%d e=%g layout=%s" % (path.__name__, k, e, layout)
            _same(lp.result(), want[:4], what)
            assert np.array_equal(lp.minhashes(), want[4]), what + ": minhashes"
            assert st["kept"] == int(t.sum()) and st["rows_cut"] == int((t < d).sum()), what
        assert lp.run(seed, k, e)["host_waits"] == 1
    lp.close()
    g.close()


def test_reference_fixture(gpu_ctx, oracle):
    """the reference's lspar fixture (byte-identical to tests/golden/pr_test.mtx), symmetrised as its driver loads it"""
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, "pr_test.mtx"), undir=True)
    for layout in (False, True):
        _check(gpu_ctx, ro, ci, FULL, layout)


@pytest.mark.parametrize("scale,ef", [(10, 16), (11, 4), (12, 8)])
def test_rmat_full_sweep(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale)
    for layout in (False, True):
        _check(gpu_ctx, ro, ci, FULL, layout, seed=scale)


@pytest.mark.parametrize("scale,ef", [(13, 16), (14, 2), (16, 16)])
def test_rmat_diagonal(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale)
    for layout in (False, True):
        _check(gpu_ctx, ro, ci, DIAGONAL, layout, seed=scale)


def test_directed_rmat(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(12, 16, 5, undir=False)
    _check(gpu_ctx, ro, ci, FULL)


def test_star_clique_empty_rows(gpu_ctx):
    leaves = 100000                                              # one row of 100 000 entries: several wave segments
    ro, ci = model.csr(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))
    _check(gpu_ctx, ro, ci, DIAGONAL)
    v = np.arange(300)
    s, d = np.meshgrid(v, v, indexing="ij")
    ro, ci = model.csr(300, s.ravel(), d.ravel(), symmetric=False)   # a clique with self-loops: rows of 300
    _check(gpu_ctx, ro, ci, FULL)
    rng = np.random.default_rng(3)
    n = 3000
    deg = rng.integers(0, 12, n)
    deg[rng.integers(0, n, 500)] = 0
    deg[rng.integers(0, n, 20)] = rng.integers(60, 9000, 20)
    ro = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, n, int(ro[-1])).astype(np.int32)
    _check(gpu_ctx, ro, ci, FULL)
    _check(gpu_ctx, np.zeros(11, np.int32), np.zeros(0, np.int32), DIAGONAL)


def test_minhash_columns_against_the_oracle_reduce(gpu_ctx, oracle):
    """column j of the table is the i32 minimum of the flipped hashes over each row (oracle.neighbor_reduce_i32), flipped back"""
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(12, 16, 12)
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    lp.run(99, 8, 0.5)
    mh = lp.minhashes()
    for j in range(8):
        vals = (model.keys(n, model.salt(99, j)) ^ np.uint32(0x80000000)).view(np.int32)
        red, _ = oracle.neighbor_reduce_i32(ro, ci, np.arange(n, dtype=np.int32), vals, 2 ** 31 - 1, 0)
        assert np.array_equal(mh[:, j], red.view(np.uint32) ^ np.uint32(0x80000000)), j
    lp.close()
    g.close()


def test_bad_parameters_and_no_run(gpu_ctx):
    import mini_amd
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    with pytest.raises(mini_amd.MgxError):
        lp.result()
    with pytest.raises(mini_amd.MgxError):
        lp.graph()
    for k, e in ((0, 0.5), (33, 0.5), (1, -0.1), (1, float("nan")), (1, float("inf"))):
        for path in (lp.run, lp.enact):
            with pytest.raises(mini_amd.MgxError) as ex:
                path(1, k, e)
            assert ex.value.status == mini_amd.MGX_E_INVALID
    lp.close()
    g.close()


def test_result_graph_runs_bfs(gpu_ctx, oracle):
    """LsparProblem.graph(): a new graph other entry points run on -- push BFS labels equal the oracle's on the model's CSR"""
    import mini_amd
    n, ro, ci, w = oracle.rmat_csr(14, 16, 14)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    lp = mini_amd.LsparProblem(g)
    lp.run(model.SEED, 4, 0.5)
    oro, oci, oeid, _, _ = model.sparsify(ro, ci, model.SEED, 4, 0.5)
    g2 = lp.graph()
    assert (g2.num_nodes, g2.num_edges) == (n, len(oci))
    lp.close()                                                   # the new graph owns its copy
    g.close()
    src = int(np.argmax(np.diff(ro)))
    bfs = mini_amd.BfsProblem(g2, src)
    bfs.run(src, mode=mini_amd.MGX_BFS_PUSH)
    assert np.array_equal(bfs.labels(), oracle.bfs_cpu(oro, oci, src))
    ro2, ci2, _ = g2.csc_arrays()                                # (the CSR mirror) and the gathered weights
    assert np.array_equal(ro2, oro) and np.array_equal(ci2, oci)
    g2.close()


def test_rmat20_fused_equals_model(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(20, 16, 20)
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    lp.run(model.SEED, 1, 0.5)
    want = model.sparsify(ro, ci, model.SEED, 1, 0.5)
    _same(lp.result(), want[:4], "rmat20 fused")
    assert np.array_equal(lp.minhashes(), want[4])
    lp.close()
    g.close()


@pytest.mark.parametrize("k", [1, 8])
def test_rmat22_fused_equals_operator_path(gpu_ctx, k):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(gpu_ctx, 22, 16)
    g = mini_amd.Graph.from_device(gpu_ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    g.build_layout()
    lp = mini_amd.LsparProblem(g)
    sf = lp.run(model.SEED, k, 0.5)
    rf, mf = lp.result(), lp.minhashes()
    so = lp.enact(model.SEED, k, 0.5)
    _same(lp.result(), rf, "rmat22 k=%d" % k)
    assert np.array_equal(lp.minhashes(), mf)
    assert sf["kept"] == so["kept"] and sf["rows_cut"] == so["rows_cut"] and sf["host_waits"] == 1
    lp.close()
    g.close()
