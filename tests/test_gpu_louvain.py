"""GPU suite (-m gpu): Louvain community detection (mgx_louvain_*).  The fused path (mgx_louvain_run) and the numpy
model (tests/louvain_model.py) agree bit for bit -- the final labels, the map of every level, the levels' records, the trace, the
stats -- on rows at every cut between the bodies under several settings of the switches, hubs with more distinct labels than any
LDS table holds, coarse levels with weights and self entries and long coarse rows, ties, rejected iterations, the caps, W = 0,
both values of `symmetric`, planted blocks and R-MAT 10 - 14; the operator path (mgx_louvain_enact) gives the same on everything
but R-MAT-14 and the 10^5-entry rows (its thread per vertex takes more than seconds there).  The launches' kinds, the rows per
body and the long rows' items are the ones the model predicts, the host waits are exact, the repeat run is equal and allocates
nothing; mgx_modularity of the final labels gives back the stats' sums."""
import numpy as np
import pytest

from tests import cc_model, chain_model
from tests import louvain_cases as cases
from tests import louvain_model as model
from tests import lpa_cases
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

KEYS = model.STAT_KEYS
ENV = {"short_max": "MGX_LOUVAIN_SHORT_MAX", "wave_max": "MGX_LOUVAIN_WAVE_MAX", "seg": "MGX_LOUVAIN_SEG"}


def _graph(ctx, ro, ci, csc=None, layout=False):
    """csc: None none, "build" by the library, "upload" with the graph"""
    import mini_amd
    if csc == "upload":
        co, ri = cc_model.transpose(ro, ci)
        g = mini_amd.Graph.from_host(ctx, ro, ci, None, co, ri)
    else:
        g = mini_amd.Graph.from_host(ctx, ro, ci, None)
        if csc == "build":
            g.build_csc()
    if layout:
        g.build_layout()
    return g


def _setenv(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv(ENV[k], str(v))


def _check(ctx, ro, ci, symmetric=True, seed=model.SEED, max_iter=100, max_levels=32, tol=0.0, csc=None, layout=False, opts=None,
           operator=True, want=None):
    """fused == operator path == model on the labels of every level, levels, trace and stats; the kinds, the rows per body and the long rows' items
    as the model predicts them; the host waits and launches; the repeat run; mgx_modularity of the final labels.
    opts: the switches the handle reads, for the model; want: the model's result where the caller has it."""
    import mini_amd
    opts = opts or {}
    w = model.louvain(ro, ci, symmetric, seed, max_iter, max_levels, tol, **opts) if want is None else want
    n = len(ro) - 1
    g = _graph(ctx, ro, ci, csc if csc else (None if symmetric else "build"), layout)
    lp = mini_amd.LouvainProblem(g)
    args = dict(symmetric=symmetric, seed=seed, max_iter=max_iter, max_levels=max_levels, tol=tol)
    s1 = lp.run(**args)
    print("fused", s1, lp.levels())
    l1 = lp.labels()
    assert l1.dtype == np.int32 and len(l1) == n
    tr = lp.trace()
    assert [tuple(x) for x in tr.tolist()] == w["trace"], (tr.tolist()[:6], w["trace"][:6])
    assert [tuple(lv[k] for k in lp.LEVEL_KEYS) for lv in lp.levels()] == w["levels"], (lp.levels(), w["levels"])
    assert {k: s1[k] for k in KEYS} == w["stats"], (s1, w["stats"])
    maps = lp.dendrogram()
    assert len(maps) == len(w["maps"])
    for a, b in zip(maps, w["maps"]):
        assert np.array_equal(a, b), "a level's map: %d of %d labels differ" % (int((a != b).sum()), len(a))
    assert np.array_equal(l1, w["labels"]), "%d of %d labels differ" % (int((l1 != w["labels"]).sum()), len(l1))
    assert s1["iterations"] == len(w["trace"])
    assert abs(lp.modularity() - model.modularity(w)) <= 1e-15
    kinds = lp.step_kinds()
    assert kinds.tolist() == w["kinds"], (kinds.tolist()[:12], w["kinds"][:12])
    b = lp.bins()
    assert [b["rows_none"], b["rows_short"], b["rows_wave"], b["rows_long"]] == w["bins"], (b, w["bins"])
    assert b["long_items"] == w["items"], (b, w["items"])
    sm = opts.get("short_max", model.SHORT_MAX)
    assert (b["short_max"], b["wave_max"], b["seg"]) == (sm, max(opts.get("wave_max", model.WAVE_MAX), sm), opts.get("seg", model.SEG))
    # the chains: whole batches are enqueued per level (the run of max_levels == 0 and of W == 0 is one SETUP chain), one wait each;
    # the aggregation waits once per renumbering (the communities) and twice per contraction: the segmented sort's list sizes (its
    # lists are the handle's: no second wait before a release) and the coarse entries; one wait for the stats
    chains = model.chains(w["kinds"])             # (K of every level's chain, from the model)
    assert s1["launches"] == sum(chain_model.waits_and_launches(c)[1] for c in chains)
    # (a run that ended at max_levels does not contract its last level)
    contractions = s1["levels"] if len(w["levels"]) > s1["levels"] else max(s1["levels"] - 1, 0)
    assert s1["host_waits"] == sum(chain_model.waits_and_launches(c)[0] for c in chains) + s1["levels"] + 2 * contractions + 1, (s1, chains)
    before = mini_amd.lib.mgx_device_allocations()
    s2 = lp.run(**args)
    assert mini_amd.lib.mgx_device_allocations() == before       # a repeat run allocates nothing
    assert s2 == s1, (s1, s2)                                    # ... and is equal: the same launches, the same waits
    assert np.array_equal(lp.labels(), l1) and np.array_equal(lp.trace(), tr)
    for a, b2 in zip(lp.dendrogram(), maps):
        assert np.array_equal(a, b2)
    q, s_in, s_sq, ww = mini_amd.modularity(g, lp.labels_device_ptr() or 0, symmetric)
    assert (s_in, s_sq, ww) == (s1["s_in"], s1["s_sq"], s1["w"]), ((s_in, s_sq, ww), s1)
    if operator:
        so = lp.enact(**args)
        print("operator", so)
        assert {k: so[k] for k in KEYS} == w["stats"], (so, w["stats"])
        assert [tuple(x) for x in lp.trace().tolist()] == w["trace"]
        assert [tuple(lv[k] for k in lp.LEVEL_KEYS) for lv in lp.levels()] == w["levels"], (lp.levels(), w["levels"])
        mo = lp.dendrogram()
        assert len(mo) == len(maps) and all(np.array_equal(a, b2) for a, b2 in zip(mo, maps))
        assert np.array_equal(lp.labels(), l1) and so["iterations"] == s1["iterations"] and so["host_waits"] >= 1
    lp.close()
    g.close()
    return w, s1


CUTS = [1, model.SHORT_MAX, model.SHORT_MAX + 1, model.WAVE_MAX, model.WAVE_MAX + 1, 2 * model.SEG, 2 * model.SEG + 1]
FORCED = [{}, {"short_max": 0, "wave_max": 0, "seg": 64}, {"short_max": 0, "wave_max": 512}, {"short_max": 16, "wave_max": 16, "seg": 1024},
          {"short_max": 3, "wave_max": 40, "seg": 128}]


@pytest.mark.parametrize("opts", FORCED)
def test_rows_at_every_cut(gpu_ctx, monkeypatch, opts):
    """disjoint cliques and stars whose vertices have exactly 1, SHORT_MAX, SHORT_MAX + 1 ... entries: at the defaults, with every
    row long, every row (up to 512 entries) a wave's, no wave rows, and small cuts (the switches are read once per handle)"""
    _setenv(monkeypatch, opts)
    ro, ci = lpa_cases.cliques_and_stars(CUTS)
    w, s = _check(gpu_ctx, ro, ci, True, opts=opts)
    assert w["items"] > 0 and w["bins"][3] > 0
    _check(gpu_ctx, ro, ci, False, opts=opts)                   # (both rows of every vertex: every weight doubled)
    _check(gpu_ctx, *lpa_cases.random_symmetric(500, 3000, 8), True, opts=opts)


@pytest.mark.parametrize("leaves", [65, 257, 2049, 5000])
def test_hubs_with_many_distinct_labels(gpu_ctx, leaves):
    """a star's centre sees one label per leaf in iteration 0: more than tables of 64, 256 and 2 048 would hold"""
    w, s = _check(gpu_ctx, *lpa_cases.star(leaves), True)
    assert s["communities"] == 1 and w["trace"][0][1] == 0 and w["trace"][1][1] == 1      # rejected, then accepted


@pytest.mark.parametrize("wave_max", [64, 256])
def test_winner_among_many(gpu_ctx, monkeypatch, wave_max):
    """300 distinct labels of weight one but one of weight two: it must be found wherever it lies in the row's table"""
    monkeypatch.setenv("MGX_LOUVAIN_WAVE_MAX", str(wave_max))
    for repeated in (1, 217, 300):
        ro, ci = lpa_cases.one_repeated_among_many(300, repeated)
        w, s = _check(gpu_ctx, ro, ci, True, max_iter=1, max_levels=1, opts={"wave_max": wave_max})
        assert w["items"] > 0


def test_mover_with_a_long_row(gpu_ctx):
    """two stars of 10^5 leaves joined at their centres: the centres' rows are items of many segments, and a centre moves"""
    ro, ci = lpa_cases.joined_stars(100000)
    w, s = _check(gpu_ctx, ro, ci, True, operator=False)
    assert w["items"] >= 2 * 391 and s["communities"] <= 2
    _check(gpu_ctx, ro, ci, False, max_iter=4, max_levels=1, operator=False)     # both rows of a centre: twice the entries


@pytest.mark.parametrize("cliques", [100, 300])
def test_coarse_levels_with_weights_and_long_rows(gpu_ctx, cliques):
    """a star of cliques: the coarse graph has self entries, weights >= 2 and a hub row of a wave's (100) or the long body's (300)
    length; few, large blocks: coarse rows that gather many members' entries"""
    w, s = _check(gpu_ctx, *cases.star_of_cliques(cliques, 5), True)
    assert s["levels"] == 1 and len(w["levels"]) == 2 and w["levels"][1][0] == cliques
    ro, ci, block = cases.few_large_blocks(cliques)
    w, s = _check(gpu_ctx, ro, ci, True)
    assert lpa_cases.same_partition(w["labels"], block)
    _check(gpu_ctx, ro, ci, False)


def test_several_levels(gpu_ctx):
    for ro, ci in (lpa_cases.path(5000), lpa_cases.grid(40, 40), lpa_cases.random_symmetric(2000, 8000, 3)):
        w, s = _check(gpu_ctx, ro, ci, True)
        assert s["levels"] >= 4


def test_ties_and_the_direction_test(gpu_ctx):
    """a 4-cycle: equal scores, the key decides, and every vertex is blocked by the direction test in one of the parities; a path
    of five: a tie the current label wins; two triangles: the closed form"""
    w, s = _check(gpu_ctx, *cases.tie_square(), True)
    assert 0 < w["trace"][0][0] < 4
    _check(gpu_ctx, *cases.tie_square(), True, max_iter=1)
    _check(gpu_ctx, *lpa_cases.sym(5, [0, 1, 2, 3], [1, 2, 3, 4]), True)
    w, s = _check(gpu_ctx, *cases.two_triangles(), True)
    assert s["communities"] == 2 and (s["s_in"], s["s_sq"], s["w"]) == (12, 98, 14)
    w, s = _check(gpu_ctx, *lpa_cases.sym(2, [0], [1]), True)
    assert s["communities"] == 1


def test_caps_and_tolerance(gpu_ctx):
    ro, ci = lpa_cases.random_symmetric(300, 900, 1)
    w, s = _check(gpu_ctx, ro, ci, True, max_iter=0)
    assert s["levels"] == 0 and s["communities"] == 300 and s["w"] > 0
    w, s = _check(gpu_ctx, ro, ci, True, max_levels=0)
    assert s["levels"] == 0 and s["communities"] == 300 and s["w"] > 0 and s["launches"] == 64
    w, s = _check(gpu_ctx, ro, ci, True, max_levels=1)
    assert s["levels"] == 1
    w, s = _check(gpu_ctx, ro, ci, True, max_levels=2)
    assert s["levels"] == 2
    w, s = _check(gpu_ctx, ro, ci, True, max_iter=3)
    assert w["levels"][0][2] == 3
    w, s = _check(gpu_ctx, ro, ci, True, tol=1.0)                # nothing gains W^2: two rejected iterations
    assert s["levels"] == 0 and s["iterations"] == 2
    w, s = _check(gpu_ctx, ro, ci, True, tol=1e-4)
    assert s["levels"] >= 1


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    for ro, ci in (lpa_cases.empty(n), lpa_cases.directed(n, np.arange(n), np.arange(n))):    # (and self-loops only)
        for symmetric in (True, False):
            w, s = _check(gpu_ctx, ro, ci, symmetric)
            assert s["communities"] == n and s["levels"] == 0 and s["w"] == 0 and s["launches"] == 64


def test_multiplicity_and_self_loops(gpu_ctx):
    ro, ci = lpa_cases.random_symmetric(3000, 6000, 5)
    plain = model.louvain(ro, ci)
    w, s = _check(gpu_ctx, *lpa_cases.tripled_with_loops(ro, ci), True)
    assert np.array_equal(w["labels"], plain["labels"])
    _check(gpu_ctx, *lpa_cases.tripled_with_loops(*lpa_cases.random_digraph(3000, 6000, 6)), False)
    _check(gpu_ctx, *cases.loops_and_duplicates(), True)


@pytest.mark.parametrize("layout", [False, True])
@pytest.mark.parametrize("upload", [False, True])
def test_both_symmetric_values(gpu_ctx, layout, upload):
    """symmetric = 1 on a symmetric graph, symmetric = 0 on a directed one with the CSC built or uploaded, each with and without
    an attached layout, which is ignored"""
    _check(gpu_ctx, *lpa_cases.random_symmetric(1500, 5000, 21), True, csc="upload" if upload else None, layout=layout)
    _check(gpu_ctx, *lpa_cases.random_digraph(1500, 5000, 22), False, csc="upload" if upload else "build", layout=layout)


@pytest.mark.parametrize("seed", [0, 5])
def test_planted_blocks(gpu_ctx, seed):
    ro, ci, block = lpa_cases.planted_blocks(seed)
    w, s = _check(gpu_ctx, ro, ci, True)
    assert s["communities"] == 40 and s["largest"] == 50 and lpa_cases.same_partition(w["labels"], block)
    _check(gpu_ctx, ro, ci, True, seed=12345)


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_rmat_symmetric(gpu_ctx, oracle, scale):
    n, ro, ci, _ = oracle.rmat_csr(scale, 8, scale + 300, undir=True)
    w, s = _check(gpu_ctx, ro, ci, True, operator=scale <= 12)
    assert s["levels"] >= 1 and w["items"] > 0


def test_rmat12_directed(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 312, undir=False)
    _check(gpu_ctx, ro, ci, False)
    _check(gpu_ctx, ro, ci, False, csc="upload", max_iter=6, max_levels=2)


def test_rmat12_on_one_compute_unit(monkeypatch, torch_mod, oracle, built):
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 112, undir=True)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _check(ctx, ro, ci, True)
        _check(ctx, *lpa_cases.star(5000), True)


def test_lifecycle_and_invalid_arguments(gpu_ctx):
    import mini_amd
    ro, ci = lpa_cases.random_digraph(400, 900, 9)
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LouvainProblem(g)
    getters = (lp.labels, lp.labels_device_ptr, lp.levels, lp.trace, lp.step_kinds, lp.bins, lp.phase_ms)
    for go in (lp.run, lp.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go(symmetric=False)
        assert err.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(err.value)
        with pytest.raises(mini_amd.MgxError):
            go(symmetric=True, max_levels=65)
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
    with pytest.raises(mini_amd.MgxError) as err:
        lp.run(symmetric=False)                                  # symmetric = 0 without a CSC
    assert err.value.status == mini_amd.MGX_E_INVALID and "mgx_graph_build_csc" in str(err.value)
    for bad in (dict(max_iter=-1), dict(max_iter=(1 << 20) + 1), dict(max_levels=-1), dict(max_levels=65), dict(tol=-1e-9),
                dict(tol=1.5), dict(tol=float("nan"))):
        with pytest.raises(mini_amd.MgxError) as err:
            lp.run(symmetric=True, **bad)
        assert err.value.status == mini_amd.MGX_E_INVALID
    st = lp.run(symmetric=True)
    assert lp.labels_device_ptr() and len(lp.labels(0)) == 400
    for level in (-2, st["levels"]):
        out = np.empty(400, dtype=np.int32)
        assert mini_amd.lib.mgx_louvain_labels(lp._h, level, out.ctypes.data) == mini_amd.MGX_E_INVALID
    with pytest.raises(mini_amd.MgxError):
        lp.run(symmetric=False)                                  # a failed run leaves nothing to the getters
    for call in getters:
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert "no run yet" in str(err.value)
    g.build_csc()                                                # the handle is still usable
    want = model.louvain(ro, ci, False)
    assert {k: v for k, v in lp.run(symmetric=False).items() if k in KEYS} == want["stats"] and np.array_equal(lp.labels(), want["labels"])
    assert {k: v for k, v in lp.enact(symmetric=False).items() if k in KEYS} == want["stats"] and np.array_equal(lp.labels(), want["labels"])
    for call in (lp.step_kinds, lp.bins, lp.phase_ms):           # these describe fused runs only
        with pytest.raises(mini_amd.MgxError):
            call()
    lp.set_timing(True)
    lp.run(symmetric=False)
    ms = lp.phase_ms()
    assert set(ms) == set(lp.PHASES) and all(v >= 0.0 for v in ms.values()) and ms["evaluate"] > 0.0 and ms["aggregate"] > 0.0
    assert np.array_equal(lp.labels(), want["labels"])
    lp.close()
    g.close()
