"""GPU suite (-m gpu): the fused sparsification at the edges of its row classes and for every shape of its minhash table
(tests/lspar_cases.py, built from the thresholds LsparProblem.info() reports; tests/test_lspar_cases_cpu.py proves each case's
property from the model alone).  Every case runs on the session context and on a context of one compute unit (tests/grid_cus.py):
fused path == operator path == model bit for bit -- the four result arrays and the minhash table --, the table's stride and the
long rows' item count are the predicted ones."""
import ctypes as C

import numpy as np
import pytest

from tests import lspar_cases as cases
from tests import lspar_model as model
from tests.grid_cus import one_cu_context
from tests.test_gpu_lspar import DIAGONAL, _graph, _same
from tests.test_gpu_lspar import _check as check_lspar

pytestmark = pytest.mark.gpu


@pytest.fixture
def one_cu(gpu_ctx, torch_mod, monkeypatch):
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def consts(gpu_ctx):
    """the thresholds the library runs with: (short_max, seg, k_max)"""
    import mini_amd
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    lp.run(model.SEED, 1, 0.5)
    info = lp.info()
    lp.close()
    g.close()
    return info["short_max"], info["seg"], info["k_max"]


def _check(ctxs, ro, ci, params, consts, seed=model.SEED):
    """fused == operator path == model for every (k, e) of params on every context, as tests/test_gpu_lspar.py's _check has it, and
    the fused run's stride and item count == the prediction.  The model runs once per (k, e)."""
    import mini_amd
    short_max, seg = consts[0], consts[1]
    d = np.diff(ro.astype(np.int64))
    items = cases.long_items(ro, short_max, seg)
    wants = [(model.sparsify(ro, ci, seed, k, e), model.keep_count(d, e)) for k, e in params]
    for ctx in ctxs:
        g = _graph(ctx, ro, ci)
        lp = mini_amd.LsparProblem(g)
        for (k, e), (want, t) in zip(params, wants):
            for path in (lp.run, lp.enact):
                st = path(seed, k, e)
                what = "%s k=%d e=%g num_cus=%d" % (path.__name__, k, e, ctx.num_cus)
                _same(lp.result(), want[:4], what)
                assert np.array_equal(lp.minhashes(), want[4]), what + ": minhashes"
                assert st["kept"] == int(t.sum()) and st["rows_cut"] == int((t < d).sum()), what
                info = lp.info()                             # (after an enact: still the last fused run's)
                assert (info["short_max"], info["seg"], info["k_max"]) == tuple(consts)
                assert info["stride"] == cases.stride(k) and info["items"] == items, (what, info)
        lp.close()
        g.close()


def test_info_reports_the_constants_and_needs_a_fused_run(gpu_ctx, consts):
    import mini_amd
    assert consts == (cases.SHORT_MAX, cases.SEG, cases.K_MAX) == (64, 4096, 32)
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    with pytest.raises(mini_amd.MgxError) as ex:
        lp.info()
    assert ex.value.status == mini_amd.MGX_E_INVALID
    lp.enact(model.SEED, 3, 0.5)                             # (an enact is no fused run)
    with pytest.raises(mini_amd.MgxError):
        lp.info()
    lp.run(model.SEED, 3, 0.5)
    assert lp.info() == {"short_max": 64, "seg": 4096, "k_max": 32, "stride": 4, "items": 0}
    assert mini_amd.lib.mgx_lspar_info(lp._h, None) == mini_amd.MGX_E_INVALID
    lp.close()
    g.close()


@pytest.fixture(scope="module")
def length_edges(consts):
    return cases.length_edges(consts[0], consts[1])[:2]


@pytest.mark.parametrize("k", cases.KS)
def test_length_edges(gpu_ctx, one_cu, consts, length_edges, k):
    ro, ci = length_edges
    _check((gpu_ctx, one_cu), ro, ci, [(k, 0.5)], consts)


@pytest.mark.parametrize("k", cases.KS)
def test_graded_long(gpu_ctx, one_cu, consts, k):
    """a hub of three segments and five entries whose cut falls inside a level that lies in all three: an e each for the cut in
    the level's first, a middle and its last segment"""
    ro, ci = cases.graded_long(k, consts[1])
    params = cases.graded_params(ro, ci, model.SEED, k, consts[1])
    assert all(e is not None for _, e in params), params
    _check((gpu_ctx, one_cu), ro, ci, [(k, e) for _, e in params], consts)


@pytest.mark.parametrize("k", cases.KS)
def test_graded_short(gpu_ctx, one_cu, consts, k):
    """the same on a row of exactly short_max entries: the cut inside a level that recurs in each of the select's register rounds"""
    ro, ci = cases.graded_short(k, consts[0])
    params = cases.graded_params(ro, ci, model.SEED, k, consts[0] // cases.SEL_ROUNDS)
    assert all(e is not None for _, e in params), params
    _check((gpu_ctx, one_cu), ro, ci, [(k, e) for _, e in params], consts)


def test_a_smaller_k_after_a_larger_on_one_handle(gpu_ctx, one_cu, consts, length_edges):
    """k = 32 and then k = 5 (and 2, and 1) on the same handle: columns of the bigger table left behind would show in the sims"""
    ro, ci = length_edges
    _check((gpu_ctx, one_cu), ro, ci, [(32, 0.5), (5, 0.5), (31, 0.25), (2, 0.5), (9, 0.75), (1, 0.5)], consts)


def test_keep_count_edges(gpu_ctx, one_cu):
    """rows of j^p - 1, j^p, j^p + 1 entries: the keep counts of both paths (device pow, host pow) are the exact integer roots"""
    import mini_amd
    ro, ci = cases.keep_count_edges()
    d = np.diff(ro.astype(np.int64))
    for ctx in (gpu_ctx, one_cu):
        g = _graph(ctx, ro, ci)
        lp = mini_amd.LsparProblem(g)
        for e in cases.KEEP_ES:
            t = cases.exact_keep(d, e)
            out_ro = np.concatenate([[0], np.cumsum(t)]).astype(np.int32)
            for path in (lp.run, lp.enact):
                st = path(model.SEED, 1, float(e))
                what = "%s e=%s num_cus=%d" % (path.__name__, e, ctx.num_cus)
                got = np.empty(len(ro), dtype=np.int32)
                assert mini_amd.lib.mgx_lspar_result(lp._h, got.ctypes.data_as(C.c_void_p), None, None, None) == 0
                bad = np.nonzero(np.diff(got) != t)[0]
                assert len(bad) == 0, "%s: t differs on rows of %s entries" % (what, d[bad][:8].tolist())
                assert np.array_equal(got, out_ro), what
                assert st["kept"] == int(t.sum()) and st["rows_cut"] == int((t < d).sum()), what
        lp.close()
        g.close()


def test_one_unit_sweep_sparsification(one_cu, oracle):
    n, ro, ci, _ = oracle.rmat_csr(14, 2, 14)
    check_lspar(one_cu, ro, ci, DIAGONAL, seed=14)
