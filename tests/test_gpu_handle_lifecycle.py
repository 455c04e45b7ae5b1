"""GPU suite (-m gpu): the life of a problem handle -- create, run, read, free, again -- for every problem class, and the host-side
resources a handle makes on the way: the pinned blocks a state owns from its constructor, the ones made at first use (the SSSP
predecessors' counters, the source-shape request of a single-source BFS) or regrown (the heads of a BFS batch), and the HIP events
of the timed runs.  Nothing here is provoked: every case is an ordinary create / run / free, and every repeat must return what the
first one did, bit for bit.

Two paths are not reproducible bit for bit by construction, and are compared accordingly:
  * the operator path of the betweenness centrality adds its dependencies with double atomic adds in whatever order the device
    schedules them (gunrock/bc/bc_functor.hxx).  Its depths and path counts (integers in doubles) are compared bit for bit; its
    centrality and its last source's dependencies against the first cycle's within 4 m eps relative: every term is positive, a
    value is built from at most m additions per source (one per entry, over all levels), and each rounds once.
  * the operator path of the spanning forest appends its edges through an atomic cursor: the triples are compared sorted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CYCLES = 8
MANY_CHUNK = 512                    # gunrock::bfs::bfs_fused_enactor_t::MANY_CHUNK


@pytest.fixture(scope="module")
def rmat(oracle):
    n, ro, ci, w = oracle.rmat_csr(10, 16, 10)
    assert n == 1024
    for a in (ro, ci, w):
        a.setflags(write=False)
    return n, ro, ci, w


@pytest.fixture(scope="module")
def graph(gpu_ctx, rmat):
    """the weighted graph with its genuine CSC: what every class runs on"""
    import mini_amd
    _, ro, ci, w = rmat
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    g.build_csc()
    yield g
    g.close()


@pytest.fixture(scope="module")
def laid_graph(gpu_ctx, rmat):
    """the same graph with the hub-first layout: the source shapes and the batches' shape tables exist only with it"""
    import mini_amd
    _, ro, ci, w = rmat
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    g.build_layout(weights=True)
    yield g
    g.close()


@pytest.fixture(scope="module")
def sources(rmat):
    from mini_amd import rmat as gen
    return gen.pick_sources(rmat[1], 4, 10)


def _bytes(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _sorted_triples(a, b, w):
    order = np.lexsort((w.view(np.uint32), b, a))
    return a[order], b[order], w[order]


# One cycle of a class: create, run() and enact() (what the class has of the two), read after each, close.  Returns
# {name: tuple of bytes} of what must repeat bit for bit, and {name: float64 array} of what repeats within the bound above.
def _bfs(m, g, src):
    p = m.BfsProblem(g, src[0])
    p.run(src[0])
    run = p.labels()
    p.reset(src[0])
    p.enact_pushpull()
    out = {"run": _bytes(run), "enact_pushpull": _bytes(p.labels())}
    p.close()
    return out, {}


def _sssp(m, g, src):
    p = m.SsspProblem(g, src[0])
    p.enact(1.5)
    enact = p.distances()
    p.run(src[0])
    out = {"enact": _bytes(enact), "run": _bytes(p.distances())}
    p.close()
    return out, {}


def _pr(m, g, src):
    p = m.PrProblem(g, 10)
    lens = p.enact()
    out = {"enact": _bytes(p.ranks(), np.asarray(lens, dtype=np.int64))}
    p.close()
    return out, {}


def _kcore(m, g, src):
    p = m.KcoreProblem(g)
    k_run, _ = p.run()
    run = (p.num_cores(), p.degrees(), np.int64(k_run))
    p.reset()
    k_enact, _ = p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(p.num_cores(), p.degrees(), np.int64(k_enact))}
    p.close()
    return out, {}


def _color(m, g, src):
    p = m.ColorProblem(g)
    p.run()
    run = (p.colors(), p.round_trace())
    p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(p.colors(), p.round_trace())}
    p.close()
    return out, {}


def _lspar(m, g, src):
    p = m.LsparProblem(g)
    p.run()
    run = p.result() + (p.minhashes(),)
    p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(*(p.result() + (p.minhashes(),)))}
    p.close()
    return out, {}


def _cc(m, g, src):
    p = m.CcProblem(g)
    st = p.run()
    run = (p.labels(), np.int64(st["components"]))
    st = p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(p.labels(), np.int64(st["components"]))}
    p.close()
    return out, {}


def _tc(m, g, src):
    p = m.TcProblem(g)
    st = p.run()
    run = (p.triangles(), p.simple_degrees(), np.int64(st["triangles"]))
    st = p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(p.triangles(), p.simple_degrees(), np.int64(st["triangles"]))}
    p.close()
    return out, {}


def _bc(m, g, src):
    p = m.BcProblem(g)
    p.run(src)
    run = (p.centrality(), p.sigma(), p.delta(), p.labels())
    p.enact(src)
    out = {"run": _bytes(*run), "enact": _bytes(p.sigma(), p.labels())}
    close = {"enact centrality": p.centrality(), "enact delta": p.delta()}
    p.close()
    return out, close


def _mst(m, g, src):
    p = m.MstProblem(g)
    p.run()
    run = p.edges() + (np.float64(p.weight()), p.labels())
    p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(*(_sorted_triples(*p.edges()) + (p.labels(),)))}
    p.close()
    return out, {}


def _pagerank(m, g, src):
    p = m.PageRankProblem(g)
    st = p.run()
    run = (p.ranks(), p.residuals(), np.int64(st["iterations"]))
    st = p.enact()
    out = {"run": _bytes(*run), "enact": _bytes(p.ranks(), p.residuals(), np.int64(st["iterations"]))}
    p.close()
    return out, {}


CLASSES = {"BfsProblem": _bfs, "SsspProblem": _sssp, "PrProblem": _pr, "KcoreProblem": _kcore, "ColorProblem": _color,
           "LsparProblem": _lspar, "CcProblem": _cc, "TcProblem": _tc, "BcProblem": _bc, "MstProblem": _mst,
           "PageRankProblem": _pagerank}


@pytest.mark.parametrize("name", list(CLASSES))
def test_create_run_free_repeats(graph, rmat, sources, name):
    import mini_amd
    assert hasattr(mini_amd, name)
    m_edges = len(rmat[2])
    first, first_close = CLASSES[name](mini_amd, graph, sources)
    for cycle in range(1, CYCLES):
        got, got_close = CLASSES[name](mini_amd, graph, sources)
        for key in first:
            assert got[key] == first[key], "%s cycle %d: %s() returned something else than cycle 0" % (name, cycle, key)
        for key in first_close:
            err = np.abs(got_close[key] - first_close[key])
            bound = 4.0 * m_edges * np.finfo(np.float64).eps * np.abs(first_close[key])
            print("%s cycle %d %s(): largest difference %.3g, bound there %.3g" % (name, cycle, key, err.max(), bound[err.argmax()]))
            assert (err <= bound).all(), "%s cycle %d: %s() is off by more than its summation bound" % (name, cycle, key)


def test_sssp_preds_twice_on_one_handle(graph, sources):
    """the predecessors' pinned counters are made by the first build_preds() and serve the second"""
    import mini_amd
    p = mini_amd.SsspProblem(graph, sources[0])
    p.run(sources[0])
    dist = p.distances()
    first = p.build_preds()
    preds = p.preds()
    second = p.build_preds()
    assert second == first
    assert np.array_equal(p.preds(), preds)
    assert np.array_equal(p.distances(), dist)
    p.close()


def test_bfs_fresh_source_then_free(gpu_ctx, rmat, graph, sources, monkeypatch):
    """a single-source run from a source the graph's shape cache has not seen asks for its shape on the stream, into pinned words made
    at that moment; the handle is freed right behind the run.  (Small graphs get source shapes only with the M launches forced.)
    The graph is made here, so that its cache is empty whatever ran before.  The cache's request counter is not part of the C ABI:
    that the request is made under this switch and in this mode is what gunrock/bfs/bfs_enactor.hxx says, and is not asserted here."""
    import mini_amd
    monkeypatch.setenv("MGX_BFS_MINI", "2")
    laid_graph = mini_amd.Graph.from_host(gpu_ctx, rmat[1], rmat[2], rmat[3])
    laid_graph.build_layout(weights=True)
    ref = mini_amd.BfsProblem(graph, sources[1])
    ref.run(sources[1])
    want = ref.labels()
    ref.close()
    p = mini_amd.BfsProblem(laid_graph, sources[1])
    p.run(sources[1])
    p.close()
    again = mini_amd.BfsProblem(laid_graph, sources[1])         # (the shape is in the cache now)
    again.run(sources[1])
    assert np.array_equal(again.labels(), want)
    again.close()
    laid_graph.close()


def test_bfs_batches_regrow_heads(laid_graph, rmat, monkeypatch):
    """1, then 3, then 600 sources on one handle: the pinned heads grow twice, and 600 is more than one chunk"""
    import mini_amd
    from mini_amd import rmat as gen
    monkeypatch.setenv("MGX_BFS_MINI", "2")
    many = gen.pick_sources(rmat[1], 600, 77)
    assert len(many) == 600 > MANY_CHUNK
    p = mini_amd.BfsProblem(laid_graph, many[0])
    for count in (1, 3, 600):
        stats, _ = p.run_many(many[:count])
        assert len(stats) == count
        assert all(s["levels"] > 0 and s["reached"] > 1 for s in stats)
    got = p.labels()
    single = mini_amd.BfsProblem(laid_graph, many[-1])
    st = single.run(many[-1])
    assert np.array_equal(got, single.labels())
    assert stats[-1]["reached"] == st["reached"] and stats[-1]["levels"] == st["levels"]
    single.close()
    p.close()


def test_timed_runs_own_their_events(graph, sources):
    """the events of the timed runs: BFS makes its pool with the state, SSSP and BC grow theirs at the first timed run.  The same
    handles with timing off again return what the timed runs did."""
    import mini_amd
    src = sources[0]
    bfs, sssp, bc = mini_amd.BfsProblem(graph, src), mini_amd.SsspProblem(graph, src), mini_amd.BcProblem(graph)
    bfs.set_kernel_timing(True)
    sssp.set_kernel_timing(True)
    bc.set_timing(True)
    bfs.run(src)
    sssp.run(src)
    bc.run(sources)
    kt = bfs.kernel_times()
    assert kt["stream"]["launches"] + kt["wave"]["launches"] > 0
    assert kt["stream"]["ns"] + kt["wave"]["ns"] > 0
    st = sssp.kernel_times()
    assert st["launches"] > 0 and st["ns"] > 0
    ph = bc.phase_ms()
    assert ph["sources_timed"] == len(sources)
    assert all(ph[k] > 0.0 for k in ("traversal", "lists", "forward", "backward"))
    timed = _bytes(bfs.labels(), sssp.distances(), bc.centrality())
    bfs.set_kernel_timing(False)
    sssp.set_kernel_timing(False)
    bc.set_timing(False)
    bfs.run(src)
    sssp.run(src)
    bc.run(sources)
    assert _bytes(bfs.labels(), sssp.distances(), bc.centrality()) == timed
    for p in (bfs, sssp, bc):
        p.close()
