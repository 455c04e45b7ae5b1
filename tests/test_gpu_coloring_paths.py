"""GPU suite (-m gpu): the fused colouring at the edges of its row classes (tests/coloring_cases.py, built from the thresholds
ColorProblem.info() reports; tests/test_coloring_cases_cpu.py proves each case's property from the model alone).  Every case runs on
the session context and on a context of one compute unit (tests/grid_cus.py): fused path == operator path == model bit for bit, and
the short rows, long items and long rows the fused run counted per round are the predicted ones.  Behind them, one small case each
of the colouring, the connected components and the segmented sort on the one-unit context: every grid-stride loop's later
iterations."""
import ctypes as C

import numpy as np
import pytest

from tests import coloring_cases as cases
from tests import coloring_model as model
from tests.grid_cus import one_cu_context
from tests.test_gpu_cc import _check as check_cc
from tests.test_gpu_coloring import _check as check_colouring
from tests.test_gpu_coloring import _graph
from tests.test_gpu_segsort import test_band_edges as segsort_band_edges

pytestmark = pytest.mark.gpu

MAX_ITERS = (0, 1, cases.FIRST_BATCH, cases.FIRST_BATCH + 1)


@pytest.fixture
def one_cu(gpu_ctx, torch_mod, monkeypatch):
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def consts(gpu_ctx):
    """the thresholds the library runs with: (long_min, seg, stage, batch_max)"""
    import mini_amd
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    cp = mini_amd.ColorProblem(g)
    cp.run(model.SEED, 0)
    info = cp.info()
    cp.close()
    g.close()
    return info["long_min"], info["seg"], info["stage"], info["batch_max"]


def _check(ctx, ro, ci, seed, want, consts, max_iters=(0,)):
    """fused == operator path == model (colours, per-round active counts, stats) as tests/test_gpu_coloring.py's _check has it, and the
    fused run's per-round row classes == the prediction; one graph and one problem for all of max_iters"""
    import mini_amd
    long_min, seg = consts[0], consts[1]
    g = _graph(ctx, ro, ci)
    cp = mini_amd.ColorProblem(g)
    for max_iter in max_iters:
        wc, wt, left = cases.truncated(want, max_iter)
        what = "max_iter=%d num_cus=%d" % (max_iter, ctx.num_cus)
        sf = cp.run(seed, max_iter)
        cf, tf, info = cp.colors(), cp.round_trace(), cp.info()
        so = cp.enact(seed, max_iter)
        co, to = cp.colors(), cp.round_trace()
        assert np.array_equal(cf, wc), "fused, %s: %d of %d colours differ" % (what, int((cf != wc).sum()), len(wc))
        assert np.array_equal(co, wc), "operator path, %s: %d of %d colours differ" % (what, int((co != wc).sum()), len(wc))
        assert np.array_equal(tf, wt) and np.array_equal(to, wt), what
        for st in (sf, so):
            assert st["rounds"] == len(wt) and st["uncolored"] == left, what
            assert st["max_color"] == (int(wc.max()) if len(wc) else 0), what
        assert (info["long_min"], info["seg"], info["stage"], info["batch_max"]) == tuple(consts)
        rows = cases.round_rows(ro, want[0], len(wt), long_min, seg)
        assert np.array_equal(info["rounds"], rows), "%s: row classes per round\n%s\npredicted\n%s" % (what, info["rounds"], rows)
    cp.close()
    g.close()


def test_info_reports_the_constants_and_needs_a_fused_run(gpu_ctx, consts):
    import mini_amd
    assert consts == (cases.LONG_MIN, cases.SEG, cases.STAGE, cases.BATCH_MAX) == (32, 2048, 128, 128)
    ro, ci = model.csr(4, [0, 1], [1, 2])
    g = _graph(gpu_ctx, ro, ci)
    cp = mini_amd.ColorProblem(g)
    with pytest.raises(mini_amd.MgxError) as ex:
        cp.info()
    assert ex.value.status == mini_amd.MGX_E_INVALID
    cp.enact(model.SEED, 0)                                  # (an enact is no fused run)
    with pytest.raises(mini_amd.MgxError):
        cp.info()
    st = cp.run(model.SEED, 0)
    info = cp.info()
    assert info["rounds"][0].tolist() == [4, 0, 0] and len(info["rounds"]) == st["rounds"]      # 0 - 1 - 2 and an isolated vertex
    four, rounds = (C.c_int64 * 4)(), C.c_int()
    assert mini_amd.lib.mgx_color_info(cp._h, four, None, 0, C.byref(rounds)) == 0 and rounds.value == st["rounds"]   # the count only
    assert list(four) == list(consts)
    assert mini_amd.lib.mgx_color_info(cp._h, four, None, 1, C.byref(rounds)) == mini_amd.MGX_E_INVALID
    assert mini_amd.lib.mgx_color_info(cp._h, None, None, 0, C.byref(rounds)) == mini_amd.MGX_E_INVALID
    assert mini_amd.lib.mgx_color_info(cp._h, four, None, 0, None) == mini_amd.MGX_E_INVALID
    cp.enact(model.SEED, 0)
    assert np.array_equal(cp.info()["rounds"], info["rounds"])      # still the last FUSED run
    cp.run(model.SEED, 1)
    assert cp.info()["rounds"].tolist() == [[4, 0, 0]]
    cp.close()
    g.close()


def test_grid_cus_only_lowers_the_count(gpu_ctx, torch_mod, monkeypatch):
    import mini_amd
    stream = torch_mod.cuda.current_stream().cuda_stream
    real = gpu_ctx.num_cus
    assert real == torch_mod.cuda.get_device_properties(0).multi_processor_count

    def count(value):
        if value is None:
            monkeypatch.delenv("MGX_GRID_CUS", raising=False)
        else:
            monkeypatch.setenv("MGX_GRID_CUS", value)
        ctx = mini_amd.Context(0, stream)
        try:
            return ctx.num_cus
        finally:
            ctx.close()

    assert count("1") == 1 and count("7") == min(7, real)
    assert count("0") == 1 and count("-3") == 1              # clamped from below
    assert count(str(real + 1)) == real and count("100000") == real
    assert count("") == real and count(None) == real         # empty counts as unset
    assert gpu_ctx.num_cus == real                           # read when a context is created, never later


@pytest.mark.parametrize("tail", cases.EDGE_TAILS)
def test_degree_edges(gpu_ctx, one_cu, consts, tail):
    long_min, seg = consts[0], consts[1]
    n = 128 * 3 + tail
    ro, ci, _ = cases.degree_edges(n, long_min, seg)
    want = model.color(ro, ci, model.SEED, 0)
    assert want[2] == 0 and want[0][n - 1] > 2
    for ctx in (gpu_ctx, one_cu):
        _check(ctx, ro, ci, model.SEED, want, consts, MAX_ITERS)


def test_hub_clique(gpu_ctx, one_cu, consts):
    seg = consts[1]
    ro, ci, hubs = cases.hub_clique(cases.HUB_CLIQUE_H, cases.hub_clique_leaves(cases.HUB_CLIQUE_H, seg))
    found = cases.hub_clique_seed(ro, ci, hubs, seg)
    assert found is not None
    seed, want = found
    for ctx in (gpu_ctx, one_cu):
        _check(ctx, ro, ci, seed, want, consts, MAX_ITERS)


def _shared_leaf_hubs(ctxs, consts, lengths):
    ro, ci = cases.shared_leaf_hubs(lengths)
    want = model.color(ro, ci, model.SEED, 0)
    assert (want[0][:len(lengths)] == 3).all()               # every hub survives round 0
    for ctx in ctxs:
        _check(ctx, ro, ci, model.SEED, want, consts, (0, 1))


def test_hubs_beyond_the_stage(gpu_ctx, one_cu, consts):
    """rows of `stage` segments (the last that waits in a wave's stage), stage + 1 (the first that goes out on its own) and more"""
    _shared_leaf_hubs((gpu_ctx, one_cu), consts, cases.beyond_stage_lengths(consts[1], consts[2]))


def test_stage_pressure(gpu_ctx, one_cu, consts):
    """96 surviving rows of stage / 3 + 1 segments: on the one-unit context a wave decides several, and its third flushes the stage
    (which wave arrives last at a row's tally is a race: the results are asserted, not that the flush ran)"""
    _shared_leaf_hubs((one_cu, gpu_ctx), consts, cases.stage_pressure_lengths(consts[1], consts[2]))


def test_late_evidence(gpu_ctx, one_cu, consts):
    """hubs of more segments than a one-unit grid has waves, whose uncoloured neighbours all lie in the last segment: the wave that
    scans it has added an earlier segment of the same row to the tally before -- the early exit must not fire on arrivals alone.  Only the one-unit grid orders the two
    segments; on the session context every segment has a wave of its own and the case is one more model comparison"""
    lengths = cases.stage_pressure_lengths(consts[1], consts[2], cases.LATE_EVIDENCE_ROWS)
    ro, ci = cases.shared_leaf_hubs(lengths, clique=True)
    want = model.color(ro, ci, model.SEED, 0)
    assert len(want[1]) == 1 + len(lengths) // 2
    for ctx in (one_cu, gpu_ctx):
        _check(ctx, ro, ci, model.SEED, want, consts, (0, 2))


def test_one_unit_sweep_colouring(one_cu, oracle):
    n, ro, ci, _ = oracle.rmat_csr(13, 16, 13)
    c = check_colouring(one_cu, ro, ci, seed=13, max_iter=0)
    assert (c > 0).all() and model.conflicts(ro, ci, c) == 0


def test_one_unit_sweep_connected_components(one_cu, oracle):
    n, ro, ci, _ = oracle.rmat_csr(13, 8, 13)
    check_cc(one_cu, ro, ci, symmetric=True)
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 114, undir=False)
    check_cc(one_cu, ro, ci, symmetric=False, csc=True)


@pytest.mark.parametrize("pairs", [False, True])
def test_one_unit_sweep_segmented_sort(one_cu, torch_mod, pairs):
    """tests/test_gpu_segsort.py's test_band_edges, called as a function: four of its eight combinations on purpose (each
    direction and each key range once per `pairs`), enough for every band's kernels to loop"""
    segsort_band_edges(gpu_ctx=one_cu, torch_mod=torch_mod, pairs=pairs, descending=pairs, distinct=3)
    segsort_band_edges(gpu_ctx=one_cu, torch_mod=torch_mod, pairs=pairs, descending=not pairs, distinct=1 << 30)
