"""GPU suite (-m gpu): k-truss decomposition (mgx_ktruss_*).  The fused path (mgx_ktruss_run), the operator path
(mgx_ktruss_enact) and the numpy model (tests/ktruss_model.py) agree exactly -- edges, supports, vertex trussness, histogram, the
adjacency with edge ids, stats [0] - [4], and the fused path's peel order pass by pass -- on the golden fixtures, R-MAT 10 - 14,
hand-made shapes for the in-front rules, many passes, many levels, every work shape forced on small graphs, fronts at the sizes of
the LDS stage, and, at RMAT-18, fused == operator path with a scipy check of two trusses."""
import functools
import os

import numpy as np
import pytest

from tests import chain_model
from tests import coloring_model as cm
from tests import ktruss_cases as cases
from tests import ktruss_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
KEYS = model.STAT_KEYS
# The waits beside the peel's (include/mgx/ktruss_fused.hpp: ensure_graph).  A first run's: the oriented graph's stats, the
# adjacency's size check, the sort's two; without an edge only the first of them, the rest is not enqueued.  A repeat run builds
# nothing and the supports wait for nothing.  Neither depends on the data beyond "is there an edge".
BUILD_WAITS, BUILD_WAITS_NO_EDGES, REPEAT_WAITS = 4, 1, 0
MIN, LIST, EXPAND, SEAL, IDLE = model.MIN, model.LIST, model.EXPAND, model.SEAL, model.IDLE


def _graph(ctx, ro, ci, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if layout:
        g.build_layout()
    return g


def _arrays(kp):
    u, v, t = kp.edges()
    ro, ci, eid = kp.adjacency()
    return {"u": u, "v": v, "truss": t, "sup0": kp.support(), "vtruss": kp.vertex_truss(), "hist": kp.histogram(), "adj_ro": ro,
            "adj_ci": ci, "adj_eid": eid}


def _wanted(w):
    return {"u": w["u"], "v": w["v"], "truss": w["truss"][w["perm"]], "sup0": w["sup0"][w["perm"]], "vtruss": w["vtruss"],
            "hist": w["hist"], "adj_ro": w["adj_ro"], "adj_ci": w["adj_ci"], "adj_eid": w["adj_eid"]}


def _same(got, want, who):
    for k in want:
        assert got[k].dtype == want[k].dtype, (who, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), "%s: %s differs in %d of %d places" % (
            who, k, int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1, len(want[k]))


def _check(ctx, ro, ci, symmetric, layout=False, want=None, operator=True):
    """fused == operator path == model; the peel order pass by pass; the repeat run; the host waits"""
    import mini_amd
    w = model.decompose(ro, ci, symmetric) if want is None else want
    wa = _wanted(w)
    g = _graph(ctx, ro, ci, layout)
    kp = mini_amd.KtrussProblem(g)
    s1 = kp.run(symmetric)
    print("fused", s1)
    a1 = _arrays(kp)
    _same(a1, wa, "fused")
    assert {k: s1[k] for k in KEYS} == w["stats"], (s1, w["stats"])
    # the peel's launches are the model's (3 levels + 2 passes + 2): the host enqueues whole batches up to the one that holds the
    # DONE, and waits once behind each
    waits, peel = chain_model.waits_and_launches(model.peel_launches(w["stats"]))
    build_waits = BUILD_WAITS if s1["edges"] else BUILD_WAITS_NO_EDGES
    assert s1["built"] == 1 and s1["host_waits"] == waits + build_waits, (s1, waits, peel)
    assert int(a1["hist"].sum()) == s1["edges"] and int(a1["sup0"].astype(np.int64).sum()) == 3 * s1["triangles"]
    order = kp.order()
    assert np.array_equal(np.sort(order), np.arange(s1["edges"]))
    at = 0
    for front in w["fronts"]:                                    # every front is a range of the order
        assert np.array_equal(np.sort(order[at:at + len(front)]), front), "pass whose front begins at %d" % at
        at += len(front)
    kinds = kp.step_kinds()
    assert s1["edges"] == 0 or {MIN, LIST, EXPAND, SEAL, IDLE} <= set(kinds.tolist()), set(kinds.tolist())
    assert int((kinds == EXPAND).sum()) == s1["passes"] and int((kinds == LIST).sum()) == s1["levels"]
    assert len(kinds) == peel and kinds.tolist() == chain_model.logged(model.peel_kinds(w), IDLE), "the log: the model's kinds, then IDLE"
    s2 = kp.run(symmetric)
    assert s2["built"] == 0 and s2["launches"] < s1["launches"] and s2["host_waits"] == waits + REPEAT_WAITS, (s1, s2)
    assert np.array_equal(kp.step_kinds(), kinds)
    assert {k: s2[k] for k in KEYS} == w["stats"]
    _same(_arrays(kp), a1, "fused repeat")
    if operator:
        so = kp.enact(symmetric)
        print("operator", so)
        _same(_arrays(kp), wa, "operator path")
        assert {k: so[k] for k in KEYS} == w["stats"], (so, w["stats"])
        assert so["built"] == 0 and so["host_waits"] >= 1
        with pytest.raises(mini_amd.MgxError):                   # the operator path leaves no peel order
            kp.order()
        kp2 = mini_amd.KtrussProblem(g)                          # the operator path first: it builds the same
        so = kp2.enact(symmetric)
        assert so["built"] == 1 and {k: so[k] for k in KEYS} == w["stats"]
        _same(_arrays(kp2), wa, "operator path, own build")
        kp2.close()
    kp.close()
    g.close()
    return w, s1


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
def test_fixtures(gpu_ctx, oracle, name, undir, symmetric):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check(gpu_ctx, ro, ci, symmetric)


@functools.lru_cache(maxsize=None)
def _rmat14():
    from tests.oracle_binding import Oracle
    n, ro, ci, _ = Oracle().rmat_csr(14, 16, 14)
    return ro, ci, model.decompose(ro, ci, True)


@pytest.mark.parametrize("scale,ef", [(10, 1), (11, 2), (12, 4), (13, 8), (14, 16)])
def test_rmat_symmetric(gpu_ctx, oracle, scale, ef):
    if scale == 14:
        ro, ci, want = _rmat14()
    else:
        (n, ro, ci, _), want = oracle.rmat_csr(scale, ef, scale), None
    w, _ = _check(gpu_ctx, ro, ci, True, want=want)
    assert w["stats"]["levels"] > 1 and w["stats"]["passes"] > w["stats"]["levels"]


@pytest.mark.parametrize("scale,ef", [(10, 2), (11, 4), (12, 4)])
def test_rmat_directed(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    _check(gpu_ctx, ro, ci, False)


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    ro, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    for symmetric in (True, False):
        w, s = _check(gpu_ctx, ro, ci, symmetric)
        assert s["max_truss"] == 0 and s["edges"] == 0 and s["levels"] == 0 and not w["vtruss"].any()


def test_self_loops_only(gpu_ctx):
    v = np.arange(3000)
    ro, ci = cm.csr(3000, v, v, symmetric=False)
    for symmetric in (True, False):
        w, s = _check(gpu_ctx, ro, ci, symmetric)
        assert s["edges"] == 0 and s["max_truss"] == 0


def test_tripled_pairs_and_self_loops_equal_the_simple_graph(gpu_ctx):
    n = 3000
    rng = np.random.default_rng(4)
    s, d = rng.integers(0, n, 40000), rng.integers(0, n, 40000)
    v = np.arange(n)
    for symmetric in (True, False):
        simple = model.decompose(*cm.csr(n, s, d, symmetric=symmetric), symmetric)
        ro, ci = cm.csr(n, np.concatenate([s, s, s, v[::7]]), np.concatenate([d, d, d, v[::7]]), symmetric=symmetric)
        w, _ = _check(gpu_ctx, ro, ci, symmetric)
        assert w["stats"] == simple["stats"] and w["stats"]["triangles"] > 0
        assert np.array_equal(w["u"], simple["u"]) and np.array_equal(w["v"], simple["v"])
        assert np.array_equal(w["truss"][w["perm"]], simple["truss"][simple["perm"]])


def test_unsorted_rows(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 77)
    rng = np.random.default_rng(5)
    shuffled = ci.copy()
    for v in range(n):
        shuffled[ro[v]:ro[v + 1]] = rng.permutation(ci[ro[v]:ro[v + 1]])
    assert not np.array_equal(shuffled, ci)
    want = model.decompose(ro, ci, True)
    _check(gpu_ctx, ro, ci, True, want=want)
    _check(gpu_ctx, ro, shuffled, True, want=want)               # (the same DAG, so the same edge ids)
    _check(gpu_ctx, ro, shuffled, False)


def test_directed_only_triangle(gpu_ctx):
    ro, ci = cm.csr(5, [1, 3, 4], [3, 4, 1], symmetric=False)             # 1 -> 3 -> 4 -> 1, no reverses
    w, s = _check(gpu_ctx, ro, ci, False)
    assert s["triangles"] == 1 and s["max_truss"] == 3 and w["vtruss"].tolist() == [0, 3, 0, 3, 3]


# ---- the in-front rules ----
def test_clique_300_decrements_nothing(gpu_ctx):
    """every triangle has all three edges in the one front"""
    w, s = _check(gpu_ctx, *cm.clique(300), True)
    assert s["max_truss"] == 300 and s["levels"] == 1 and s["passes"] == 1 and (w["truss"] == 300).all()


def test_two_cliques_sharing_an_edge(gpu_ctx):
    """the shared edge stays alive while K_200 leaves around it: a double charge shows as a wrong trussness"""
    ro, ci, ids = cases.two_cliques_sharing_an_edge(300, 200, seed=3, extra=40)
    for symmetric in (True, False):
        w, s = _check(gpu_ctx, ro, ci, symmetric, operator=symmetric)
        t = dict(zip(zip(w["u"].tolist(), w["v"].tolist()), w["truss"][w["perm"]].tolist()))
        assert t[(min(ids[0], ids[1]), max(ids[0], ids[1]))] == 300 and s["levels"] == 2 and s["passes"] == 2
        assert w["hist"][200] == 200 * 199 // 2 - 1 and w["hist"][300] == 300 * 299 // 2


def test_ten_thousand_disjoint_triangles(gpu_ctx):
    ro, ci = cases.disjoint_triangles(10000, seed=10, extra=500)
    for symmetric in (True, False):
        w, s = _check(gpu_ctx, ro, ci, symmetric)
        assert (w["truss"] == 3).all() and s["triangles"] == 10000 and s["passes"] == 1


# ---- many passes, many levels ----
def test_triangulated_grid_has_forty_passes_across_a_batch_boundary(gpu_ctx, torch_mod, monkeypatch):
    """40 passes of one level are 83 launches, more than the first batch of 64; on one unit every grid-stride loop takes several trips"""
    ro, ci = cases.grid(100, 40, True)
    want = model.decompose(ro, ci, True)
    assert want["stats"]["passes"] == 40 and want["stats"]["levels"] == 1
    w, s = _check(gpu_ctx, ro, ci, True, want=want)
    assert s["passes"] == 40 and s["levels"] == 1 and s["host_waits"] <= 2 + BUILD_WAITS
    with one_cu_context(monkeypatch, torch_mod) as one_cu:
        _, s = _check(one_cu, ro, ci, True, want=want)
        assert s["passes"] == 40 and s["host_waits"] <= 2 + BUILD_WAITS


def test_clique_chain_has_78_levels(gpu_ctx):
    w, s = _check(gpu_ctx, *cases.clique_chain(3, 80, seed=5), True)
    assert s["levels"] == 78 and s["max_truss"] == 80 and s["passes"] == 78


# ---- bins and segments ----
@pytest.mark.parametrize("short_max", ["0", "1000000000"])
def test_every_work_shape_on_rmat14(gpu_ctx, monkeypatch, short_max):
    monkeypatch.setenv("MGX_KTRUSS_SHORT_MAX", short_max)
    monkeypatch.setenv("MGX_KTRUSS_SEG", "64")
    ro, ci, want = _rmat14()
    _check(gpu_ctx, ro, ci, True, want=want, operator=False)


@pytest.mark.parametrize("d", [5, 6, 64, 65, 128])
@pytest.mark.parametrize("short_max", ["0", "5", "1000000000"])
def test_cliques_at_the_bin_and_segment_edges(gpu_ctx, monkeypatch, d, short_max):
    """K_{d + 1} has rows of d neighbours: exactly SHORT_MAX and SHORT_MAX + 1 entries, exactly SEG, SEG + 1 and 2 SEG entries"""
    monkeypatch.setenv("MGX_KTRUSS_SHORT_MAX", short_max)
    monkeypatch.setenv("MGX_KTRUSS_SEG", "64")
    w, s = _check(gpu_ctx, *cm.clique(d + 1), True, operator=False)
    assert s["max_truss"] == d + 1 and s["passes"] == 1
    # the same rows with decrements to make: K_{d + 1} with a pendant triangle on one of its edges
    ids = np.arange(d + 2)
    ro, ci = cases.cliques([ids[:d + 1], np.array([0, 1, d + 1])], d + 2)
    w, s = _check(gpu_ctx, ro, ci, True, operator=False)
    assert s["max_truss"] == d + 1 and s["levels"] == 2 and w["hist"][3] == 2


def test_item_list_overflow_goes_to_whole_rows(gpu_ctx, monkeypatch):
    """K_300 with segments of one entry: 299 items an edge are more than the item list's m + 64, so most edges are walked whole"""
    monkeypatch.setenv("MGX_KTRUSS_SHORT_MAX", "0")
    monkeypatch.setenv("MGX_KTRUSS_SEG", "1")
    ro, ci, ids = cases.two_cliques_sharing_an_edge(300, 200, seed=3, extra=40)
    _check(gpu_ctx, ro, ci, True, operator=False)


# ---- front sizes at the LDS stage ----
def _stage():
    """entries of a wave's LDS stage of list appends, from the header"""
    import re
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "mgx", "ktruss_fused.hpp")).read()
    m = re.search(r"constexpr int KTRUSS_STAGE = (\d+) \* WAVE;", text)
    return int(m.group(1)) * 64


@pytest.mark.parametrize("which", ["stage-1", "stage", "stage+1", "2stage+1", "40stage"])
def test_front_sizes_at_the_stage(gpu_ctx, torch_mod, monkeypatch, which):
    """Fronts of exactly `front` edges, one listed (LIST) and one crossed (EXPAND).  Listed: a path of `front` edges, all of
    trussness 2.  Crossed: `front` disjoint pairs of triangles {x, y, z}, {y, z, t}: level 3 lists the 4 * front outer edges, both
    triangles of every {y, z} have their other two edges in that front and charge it once each, so it goes from 2 to 0 and the next
    front is exactly the `front` edges {y, z}.  40 stages on one unit: a wave's appends outgrow its stage inside its loop."""
    stage = _stage()
    assert stage == 128
    front = {"stage-1": stage - 1, "stage": stage, "stage+1": stage + 1, "2stage+1": 2 * stage + 1, "40stage": 40 * stage}[which]
    v = np.arange(front + 1)
    path = cm.csr(front + 1, v[:-1], v[1:])
    path_want = model.decompose(*path, True)
    assert [len(f) for f in path_want["fronts"]] == [front]
    t = np.arange(front)
    x, y, z, tail = 4 * t, 4 * t + 1, 4 * t + 2, 4 * t + 3
    ro, ci = cm.csr(4 * front, np.concatenate([x, x, y, y, z]), np.concatenate([y, z, z, tail, tail]))
    want = model.decompose(ro, ci, True)
    assert [len(f) for f in want["fronts"]] == [4 * front, front] and want["stats"]["levels"] == 1
    with one_cu_context(monkeypatch, torch_mod) as one_cu:
        for ctx in (gpu_ctx, one_cu):
            _check(ctx, *path, True, want=path_want, operator=False)
            _check(ctx, ro, ci, True, want=want, operator=False)


def test_star_of_100000_leaves(gpu_ctx):
    """the centre's adjacency row of 100 000 entries is the long-row path of the build's sort"""
    ro, ci = cases.star(100000, 77777)
    for symmetric in (True, False):
        w, s = _check(gpu_ctx, ro, ci, symmetric)
        assert s["max_truss"] == 2 and s["passes"] == 1 and s["edges"] == 100000 and (w["truss"] == 2).all()


# ---- handle and context behaviour ----
def test_layout_stream_and_no_run(gpu_ctx, oracle, torch_mod):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(12, 8, 41)
    want = model.decompose(ro, ci, True)
    _check(gpu_ctx, ro, ci, True, layout=True, want=want)        # (the layout is ignored)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _check(ctx, ro, ci, True, want=want)
        g = _graph(ctx, ro, ci)
        kp = mini_amd.KtrussProblem(g)
        for getter in (kp.edges, kp.support, kp.vertex_truss, kp.histogram, kp.order, kp.adjacency, kp.step_kinds, kp.truss_device_ptr,
                       kp.vertex_truss_device_ptr, lambda: kp.truss_edges(3)):
            with pytest.raises(mini_amd.MgxError):
                getter()
        st = kp.run(True)
        assert kp.truss_device_ptr() and kp.vertex_truss_device_ptr()
        # both `symmetric` values live on the handle: the other one builds its own, the first is still there
        s0 = kp.run(False)
        assert s0["built"] == 1 and {k: s0[k] for k in KEYS} == {k: st[k] for k in KEYS}
        u, v, t = kp.edges()
        assert np.array_equal(u, want["u"]) and np.array_equal(v, want["v"]) and np.array_equal(t, want["truss"][want["perm"]])
        assert kp.run(True)["built"] == 0 and kp.run(False)["built"] == 0 and kp.enact(True)["built"] == 0
        kp.close()
        g.close()
    finally:
        ctx.close()


def test_truss_edges_against_networkx_on_rmat12(gpu_ctx, oracle):
    """every k up to the largest.  networkx.k_truss(G, k) from scratch for every k takes most of a minute; the (k + 1)-truss of G
    lies inside its k-truss H and is the (k + 1)-truss of H (a subgraph whose every edge has k - 1 triangles inside it has k - 2),
    so each k starts from the truss before it."""
    import mini_amd
    import networkx as nx
    from tests import tc_model
    n, ro, ci, _ = oracle.rmat_csr(12, 4, 12)
    g = _graph(gpu_ctx, ro, ci)
    kp = mini_amd.KtrussProblem(g)
    st = kp.run(True)
    H = tc_model.simple_graph(ro, ci)
    assert st["max_truss"] > 10
    for k in range(2, st["max_truss"] + 2):
        H = nx.k_truss(H, k)
        u, v = kp.truss_edges(k)
        want = {(min(a, b), max(a, b)) for a, b in H.edges()}
        assert set(zip(u.tolist(), v.tolist())) == want, k
    assert H.number_of_edges() == 0
    kp.close()
    g.close()


def _device_problem(ctx, scale):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(ctx, scale, 16)
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    return d, g, mini_amd.KtrussProblem(g)


def test_rmat18_identities_and_trusses(gpu_ctx):
    """the fused path at RMAT-18: the identities, and for the largest k and a middle one every edge of truss_edges(k) has at least
    k - 2 triangles inside it (scipy)"""
    import scipy.sparse as sp
    d, g, kp = _device_problem(gpu_ctx, 18)
    sf = kp.run(True)
    af = _arrays(kp)
    order = kp.order()
    print("fused", sf)
    waits, peel = chain_model.waits_and_launches(model.peel_launches(sf))   # (no model at this size: the device's own counts)
    assert sf["host_waits"] == waits + BUILD_WAITS and len(kp.step_kinds()) == min(peel, chain_model.LOG_CAP) and sf["passes"] > 1000
    assert np.array_equal(np.sort(order), np.arange(sf["edges"]))
    assert int(af["hist"].sum()) == sf["edges"] and int(af["sup0"].astype(np.int64).sum()) == 3 * sf["triangles"]
    for k in (sf["max_truss"], (sf["max_truss"] + 2) // 2):
        u, v = kp.truss_edges(k)
        assert len(u) > 0
        A = sp.csr_matrix((np.ones(2 * len(u), np.int64), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(d["n"], d["n"]))
        inside = np.asarray(A[u].multiply(A[v]).sum(axis=1)).ravel()
        assert (inside >= k - 2).all(), (k, int(inside.min()))
    kp.close()
    g.close()


def test_rmat16_fused_equals_operator_path(gpu_ctx):
    """fused == operator path on everything, on a graph the model does not see.  At RMAT-16, not 18: the operator path rescans all
    3.8 M edges of RMAT-18 in each of its 1291 passes and waits for the host three times a pass, which took it past ten seconds."""
    d, g, kp = _device_problem(gpu_ctx, 16)
    sf = kp.run(True)
    af = _arrays(kp)
    so = kp.enact(True)
    print("fused", sf, "operator", so)
    _same(_arrays(kp), af, "operator path against fused")
    assert {k: sf[k] for k in KEYS} == {k: so[k] for k in KEYS}, (sf, so)
    kp.close()
    g.close()
