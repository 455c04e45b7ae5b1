"""GPU suite (-m gpu): PageRank's reduce (include/mgx/pagerank_fused.hpp) class by class, bit for bit.

tests/test_gpu_pagerank.py compares at a tolerance that grows with the longest in-row: a dropped, doubled or misindexed entry of a
long row is far inside it.  Here ONE iteration at alpha = 1/2 on graphs whose every term is a power of two (tests/pagerank_cases.py,
shown right by tests/test_pagerank_cases_cpu.py): every sum is exact in float32 in any order, so the ranks of pp.run AND pp.enact
must equal the rounded float64 model bit for bit (np.array_equal on the case's exact mask; the leaves of a symmetric graph, whose
terms are rounded quotients, within the derived pagerank_cases.LEAF_RTOL), and the residual must be the exact e_1 of those ranks.

The graphs hold one in-row of every length at which the general reduce changes class or its unrolled loops change their remainder
(pagerank_cases.edge_lengths, built around the constants PageRankProblem.bins() reports), 130 rows for the huge rows' 64-workgroup
stride, the huge list filled to its capacity, and for the layout path the tiers of k_nrs_fold.  The general cases run on the
session's context and on a one-CU context (tests/grid_cus.py), where the grid-stride loops of k_pagerank_reduce and
k_pagerank_update take 64 trips and the verdict adds 8 partials."""
import numpy as np
import pytest

from tests import pagerank_cases as pc
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

SWITCHES = ("MGX_NR_SLICES", "MGX_NR_FOLD_DEGS", "MGX_BFS_LONG_MIN", "MGX_NR_SLICED", "MGX_NR_SUBSET", "MGX_NR_PARTS")
# the two configurations of tests/test_gpu_nreduce_paths.py: the library's own cut; ONE hot slice + tail, every tier of the fold one class down
LAYOUT_CONFIGS = {"default": {}, "slices1": {"MGX_NR_SLICES": "1", "MGX_NR_FOLD_DEGS": "4096/256/64"}}
LONG_MIN = 32                      # rows the layout's slices hold (the library's default cut)


def _setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph(ctx, case, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, case.ro, case.ci, None)
    if case.directed:
        g.build_csc()
    if layout:
        g.build_layout()
        assert g.layout_info()["units"] > 0 and g.layout_info()["units_24bit"] == 1
    return g


def _exact_run(tag, pp, case, go, layout_path=None):
    """one iteration of `go` (pp.run / pp.enact) against the case's reference; returns (ranks, residual, stats)"""
    st = go(pc.ALPHA, 0.0, 1, case.symmetric)
    got, res = pp.ranks(), pp.residuals()
    assert got.dtype == np.float32 and got.shape == case.want.shape
    bad, hub_lengths = case.differing(got)
    off = int((got.view(np.uint32) != case.want.view(np.uint32)).sum())
    print("%s: %d ranks differ from the rounded model in any bit, %d outside the comparison; residual %r (want %r); %s" % (
        tag, off, bad.size, st["residual"], case.e1, st))
    assert not bad.size, "%s: %d ranks outside the comparison (first ids %s); differing hubs have in-lengths %s" % (
        tag, bad.size, bad[:8].tolist(), hub_lengths)
    assert np.array_equal(got[case.exact].view(np.uint32), case.want[case.exact].view(np.uint32)), tag
    assert st["iterations"] == 1 and st["dangling"] == case.dangling, (tag, st)
    assert len(res) == 1 and res[0] == st["residual"], (tag, res, st)
    # e_1 is exact in double in any order: of the returned ranks always, and of the reference wherever those are bit-equal to it
    # (all of a directed graph); the leaves of a symmetric graph may move it by their tolerance
    assert st["residual"] == pc.want_e1(got, case.n), (tag, st["residual"], pc.want_e1(got, case.n))
    if off == 0:
        assert st["residual"] == case.e1, (tag, st["residual"], case.e1)
    else:
        assert case.symmetric and abs(st["residual"] - case.e1) <= float(case.leaf_bound().sum()), (tag, st["residual"], case.e1)
    if layout_path is not None:                      # the fused run
        assert st["host_waits"] == 1 and st["layout_path"] == layout_path, (tag, st)
    else:
        assert st["layout_path"] == 0, (tag, st)
    return got, res, st


def _bins(pp, case, layout_path):
    b = pp.bins()
    assert (b["lane_max"], b["huge_min"], b["huge_blocks"]) == (pc.LANE_MAX, pc.HUGE_MIN, pc.HUGE_BLOCKS), \
        "the reduce's thresholds moved: rebuild the edge lengths around them (%s)" % b
    assert b["huge_rows"] == (0 if layout_path else int((case.in_len >= b["huge_min"]).sum())), b
    return b


def _both_paths(tag, ctx, case, layout=False, layout_path=0):
    import mini_amd
    g = _graph(ctx, case, layout)
    pp = mini_amd.PageRankProblem(g)
    _exact_run(tag + " fused", pp, case, pp.run, layout_path)
    b = _bins(pp, case, layout_path)
    _exact_run(tag + " operator", pp, case, pp.enact)
    assert pp.bins() == b                            # (the report is of the last FUSED run)
    return g, pp, b


def test_no_bins_before_the_first_fused_run(gpu_ctx):
    import mini_amd
    g = mini_amd.Graph.from_host(gpu_ctx, np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32))
    pp = mini_amd.PageRankProblem(g)
    for _ in range(2):
        with pytest.raises(mini_amd.MgxError) as e:
            pp.bins()
        assert e.value.status == mini_amd.MGX_E_INVALID
        pp.enact(0.5, 0.0, 1, True)                  # the operator path has no row classes to report
    pp.run(0.5, 0.0, 1, True)
    assert pp.bins() == {"huge_rows": 0, "lane_max": pc.LANE_MAX, "huge_min": pc.HUGE_MIN, "huge_blocks": pc.HUGE_BLOCKS}
    pp.close(); g.close()


# ---- 1, 2: the general reduce ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_cu", [False, True])
@pytest.mark.parametrize("directed", [True, False])
def test_general_reduce_at_every_class_edge(gpu_ctx, monkeypatch, torch_mod, directed, one_cu):
    """directed: the in-rows of the genuine CSC (mgx_graph_build_csc), every vertex exact; symmetric without a layout: the CSR's own
    rows.  Lanes (0 .. 16 entries), waves (17 .. 8191, every remainder of the 128-entry trips), workgroups (8192 .., every remainder
    of the 512-entry trips)."""
    _setenv(monkeypatch, {})
    case = pc.edge_case(directed)
    tag = "%s%s" % ("directed" if directed else "symmetric", " one CU" if one_cu else "")
    if one_cu:
        with one_cu_context(monkeypatch, torch_mod) as ctx:
            g, pp, b = _both_paths(tag, ctx, case)
            pp.close(); g.close()
    else:
        g, pp, b = _both_paths(tag, gpu_ctx, case)
        pp.close(); g.close()
    assert b["huge_rows"] == 9
    print(tag, "bins", b)


# ---- 3: more huge rows than two trips of their launch's stride -------------------------------------------------------------------------
def test_many_huge_rows(gpu_ctx, monkeypatch):
    _setenv(monkeypatch, {})
    case = pc.many_huge()
    g, pp, b = _both_paths("many huge", gpu_ctx, case)
    assert b["huge_rows"] == 130 > 2 * b["huge_blocks"]
    r1, e1, s1 = _exact_run("many huge, again", pp, case, pp.run, 0)
    r2, e2, s2 = _exact_run("many huge, a third time", pp, case, pp.run, 0)
    assert s1 == s2 and np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(e1, e2)
    print("many huge: bins", b)
    pp.close(); g.close()


# ---- 4: the huge list filled to its capacity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64])
def test_huge_list_at_its_capacity(gpu_ctx, monkeypatch, k):
    """k rows of exactly huge_min entries and no other entry: the list's capacity in_entries / huge_min + 1 is k + 1"""
    _setenv(monkeypatch, {})
    case = pc.capacity_case(k)
    assert len(case.ci) // pc.HUGE_MIN + 1 == k + 1
    g, pp, b = _both_paths("capacity %d" % k, gpu_ctx, case)
    assert b["huge_rows"] == k
    print("capacity", k, "bins", b)
    pp.close(); g.close()


# ---- 5: the layout path -----------------------------------------------------------------------------------------------------------------
def _layout_problem(ctx, monkeypatch, case, env, tag):
    """the graph with its layout; the first run builds the slices under `env`"""
    import mini_amd
    _setenv(monkeypatch, env)
    g = _graph(ctx, case, layout=True)
    pp = mini_amd.PageRankProblem(g)
    _exact_run(tag + " fused", pp, case, pp.run, 1)
    _setenv(monkeypatch, {})
    sl = g.nr_slices_info()
    assert sl["mini_units"] > 0 and sl["long_rows"] == int(np.count_nonzero(case.out_deg >= LONG_MIN)), sl
    return g, pp, sl


@pytest.mark.parametrize("one_cu", [False, True])
@pytest.mark.parametrize("config", list(LAYOUT_CONFIGS))
def test_layout_path_at_every_class_edge_and_fold_tier(gpu_ctx, monkeypatch, torch_mod, config, one_cu):
    """symmetric with the library's layout: k_nrs_edges + k_nrs_fold driven by pagerank_state_t::run's own plumbing (identity
    old_of_new, its fold grid, its partials' address), the general edge lengths and the fold's tiers 4096 / 65536 (slices1: 256 /
    4096 as well, and a tail behind one hot slice)"""
    case = pc.edge_case(False, True)
    tag = "layout %s%s" % (config, " one CU" if one_cu else "")

    def body(ctx):
        g, pp, sl = _layout_problem(ctx, monkeypatch, case, LAYOUT_CONFIGS[config], tag)
        if config == "slices1":
            assert sl["hot_slices"] == 1 and sl["tail_mini_units"] > 0, sl
        else:
            assert sl["hot_slices"] == 4 and sl["tail_mini_units"] == 0, sl      # ceil(2^17 / 40 000) slices hold every id
        b = _bins(pp, case, 1)
        _exact_run(tag + " operator", pp, case, pp.enact)
        _exact_run(tag + " fused again", pp, case, pp.run, 1)
        print(tag, "bins", b, "slices", sl)
        pp.close(); g.close()

    if one_cu:
        with one_cu_context(monkeypatch, torch_mod) as ctx:
            body(ctx)
    else:
        body(gpu_ctx)


# ---- 6: the chunked fold ----------------------------------------------------------------------------------------------------------------
def test_chunked_fold_from_pagerank(gpu_ctx, monkeypatch):
    """n = 2^20 with 24 hot slices: nrs_slices + 1 = 25 ranges a row, above NRS_FOLD_CHUNK = 17 -- run() launches k_nrs_fold<.., true>"""
    case = pc.chunked_fold_case()
    g, pp, sl = _layout_problem(gpu_ctx, monkeypatch, case, {"MGX_NR_SLICES": "24"}, "chunked fold")
    assert sl["hot_slices"] == 24 > 16, sl
    _bins(pp, case, 1)
    _exact_run("chunked fold operator", pp, case, pp.enact)
    print("chunked fold: slices", sl)
    pp.close(); g.close()


# ---- 7: what an earlier run leaves behind ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["general", "layout"])
def test_stale_state_across_runs_on_one_handle(gpu_ctx, monkeypatch, kind):
    """a run of three iterations first, so that S, the contributions, the ranks and the trace hold later values; then fused ->
    operator -> fused of ONE iteration each on the same handle: every one bit-equal to the reference"""
    import mini_amd
    _setenv(monkeypatch, {})
    layout = kind == "layout"
    case = pc.edge_case(False, True) if layout else pc.edge_case(True)
    g = _graph(gpu_ctx, case, layout)
    pp = mini_amd.PageRankProblem(g)
    st = pp.run(pc.ALPHA, 0.0, 3, case.symmetric)
    assert st["iterations"] == 3 and st["layout_path"] == int(layout) and len(pp.residuals()) == 3, st
    assert not np.array_equal(pp.ranks(), case.want)
    st = pp.enact(pc.ALPHA, 0.0, 3, case.symmetric)
    assert st["iterations"] == 3, st
    a, ea, _ = _exact_run(kind + " fused after three iterations", pp, case, pp.run, int(layout))
    _exact_run(kind + " operator after the fused run", pp, case, pp.enact)
    b, eb, _ = _exact_run(kind + " fused after the operator", pp, case, pp.run, int(layout))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ea, eb)
    _bins(pp, case, int(layout))
    pp.close(); g.close()
