"""Batches of sources with two traversal states (MGX_BFS_BATCH_OVERLAP, default on): the tail launches of traversal i of
a batch share their launches with the head of traversal i + 1 (bfs_fused_run.hpp: k_bfs_seam_*).  Everything here is
checked against the CPU oracle AND against the same batch with the switch off (one state, launches strictly one after
the other), on a fresh handle per setting: the switches are read when a handle's state is made."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _graph(ctx, ro, ci):
    import mini_amd
    return mini_amd.Graph.from_host(ctx, ro, ci, None)


def _triples(sts):
    return [(st["m_t"], st["reached"], st["levels"]) for st in sts]


def _want_triple(ro, want, src):
    deg = np.diff(ro)
    levels = int(want.max()) + 1 if deg[src] > 0 else None       # (an isolated source: whatever both settings agree on)
    return int(deg[want >= 0].sum()), int((want >= 0).sum()), levels


def _check_batch(bfs, oracle, ro, ci, batch, tag):
    """one batch: the labels are the LAST source's, every traversal's counters are the oracle's; returns the counters"""
    import mini_amd
    sts, reruns = bfs.run_many(batch, mini_amd.MGX_BFS_PUSH, 0.0)
    assert len(sts) == len(batch), tag
    assert np.array_equal(bfs.labels(), oracle.bfs_cpu(ro, ci, batch[-1])), (tag, "labels of the last source")
    for s, t in zip(batch, _triples(sts)):
        m_t, reached, levels = _want_triple(ro, oracle.bfs_cpu(ro, ci, s), s)
        assert (t[0], t[1]) == (m_t, reached), (tag, s, t)
        if levels is not None:
            assert t[2] == levels, (tag, s, t)
    return _triples(sts), reruns


def _both_settings(monkeypatch, make_handle, body):
    """body(bfs, tag) on a fresh handle with the switch on and off; the two must return the same"""
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("MGX_BFS_BATCH_OVERLAP", sw)
        out[sw] = body(make_handle(), "overlap=" + sw)
    assert out["1"] == out["0"]
    return out["1"]


@pytest.mark.parametrize("mini", [None, "2"])
@pytest.mark.parametrize("layout", [False, True])
@pytest.mark.parametrize("scale,ef", [(14, 16), (16, 8)])
def test_batches_of_every_parity_and_rotation(gpu_ctx, oracle, monkeypatch, scale, ef, layout, mini):
    """batches of 1, 2, 3, 4 and 7 sources -- both parities of the label buffer -- every rotation of the source list, with M
    launches forced (MGX_BFS_MINI=2) and without (the default at this size): counters per traversal, labels of the last"""
    import mini_amd
    if mini is not None:
        monkeypatch.setenv("MGX_BFS_MINI", mini)
    n, ro, ci, w = oracle.rmat_csr(scale, ef, 900 + scale)
    deg = np.diff(ro)
    rng = np.random.default_rng(5 + scale)
    pool = [int(np.argmax(deg))] + [int(v) for v in rng.choice(np.where(deg > 0)[0], size=5, replace=False)] + [int(np.where(deg == 0)[0][0])]

    def make():
        g = _graph(gpu_ctx, ro, ci)
        if layout:
            g.build_layout()
        return mini_amd.BfsProblem(g, pool[0])

    def body(bfs, tag):
        res = []
        for count in (1, 2, 3, 4, 7):
            srcs = pool[:count]
            for rot in range(count):
                batch = srcs[rot:] + srcs[:rot]
                t, _ = _check_batch(bfs, oracle, ro, ci, batch, (tag, scale, layout, mini, count, rot))
                res.append(t)
        return res

    _both_settings(monkeypatch, make, body)


def _rmat_with_path(oracle, scale, ef, seed, length):
    """an R-MAT with a path of `length` vertices hanging off its biggest hub: a traversal from the hub ends with `length`
    levels of one vertex each -- the chain behind its slots runs them all"""
    n, ro, ci, w = oracle.rmat_csr(scale, ef, seed)
    deg = np.diff(ro)
    hub = int(np.argmax(deg))
    t0 = np.repeat(np.arange(n, dtype=np.int32), deg)
    t1 = ci.astype(np.int32)
    p0 = [hub] + [n + k for k in range(length - 1)]
    p1 = [n + k for k in range(length)]
    t0 = np.concatenate([t0, np.array(p0 + p1, dtype=np.int32)])
    t1 = np.concatenate([t1, np.array(p1 + p0, dtype=np.int32)])
    ro2, ci2, _ = oracle.csr_from_tuples(n + length, t0, t1, None, undir=False)
    return n + length, ro2, ci2, hub


@pytest.mark.parametrize("mini", [None, "2"])
@pytest.mark.parametrize("layout", [False, True])
def test_neighbours_that_stress_the_seam(gpu_ctx, oracle, monkeypatch, layout, mini):
    """an isolated source (its head ends at once) behind a hub and in front of one; the same source twice in a row; a source
    whose tail runs many chained levels (a path hanging off the R-MAT's hub) next to short ones"""
    import mini_amd
    if mini is not None:
        monkeypatch.setenv("MGX_BFS_MINI", mini)
    n, ro, ci, hub = _rmat_with_path(oracle, 14, 16, 321, 25)
    deg = np.diff(ro)
    iso = int(np.where(deg == 0)[0][0])
    rng = np.random.default_rng(9)
    mid = [int(v) for v in rng.choice(np.where((deg > 2) & (deg < 40))[0], size=2, replace=False)]
    end = n - 1                                          # the far end of the path: its traversal STARTS with 25 chained levels
    batches = [[hub, iso, hub], [iso, hub, iso, hub], [hub, hub], [mid[0], mid[0], mid[0]], [iso, iso], [end, hub, end, mid[1]],
               [hub, end], [mid[0], hub, iso, end, end, mid[1], hub]]

    def make():
        g = _graph(gpu_ctx, ro, ci)
        if layout:
            g.build_layout()
        return mini_amd.BfsProblem(g, hub)

    def body(bfs, tag):
        # (a warm batch first: it allocates the second state, so that every batch of the list -- the first one too -- alternates)
        res = [_check_batch(bfs, oracle, ro, ci, [mid[1], mid[1]], (tag, layout, mini, "warm"))[0]]
        return res + [_check_batch(bfs, oracle, ro, ci, b, (tag, layout, mini, bi))[0] for bi, b in enumerate(batches)]

    _both_settings(monkeypatch, make, body)


def test_label_array_keeps_its_address_and_single_runs_mix_with_batches(gpu_ctx, oracle, monkeypatch):
    """the handle's label array holds the LAST source's labels after a batch of either parity (the last traversal of a batch
    runs in the state that owns the array; an odd one writes into the second state's), and a plain run() after a batch and a
    batch after a plain run() leave the oracle's labels there: that comparison is the test.  (The address
    mgx_bfs_labels_device returns is read before and after as well; it is the problem's own array and is not expected to
    move.)"""
    import mini_amd
    monkeypatch.setenv("MGX_BFS_MINI", "2")
    n, ro, ci, w = oracle.rmat_csr(14, 16, 77)
    deg = np.diff(ro)
    rng = np.random.default_rng(4)
    srcs = [int(np.argmax(deg))] + [int(v) for v in rng.choice(np.where(deg > 0)[0], size=4, replace=False)]

    def make():
        g = _graph(gpu_ctx, ro, ci)
        g.build_layout()
        return mini_amd.BfsProblem(g, srcs[0])

    def body(bfs, tag):
        res = []
        addr = bfs.labels_device_ptr
        bfs.run(srcs[1])
        assert np.array_equal(bfs.labels(), oracle.bfs_cpu(ro, ci, srcs[1])), tag
        for count in (2, 3, 5):
            res.append(_check_batch(bfs, oracle, ro, ci, srcs[:count], (tag, count))[0])
            assert bfs.labels_device_ptr == addr, (tag, count)
            st = bfs.run(srcs[count - 2])                # a plain run behind the batch: state 0, the handle's labels
            assert np.array_equal(bfs.labels(), oracle.bfs_cpu(ro, ci, srcs[count - 2])), (tag, count)
            res.append((st["m_t"], st["reached"], st["levels"]))
            assert bfs.labels_device_ptr == addr, (tag, count)
        return res

    _both_settings(monkeypatch, make, body)


def _star_and_layers(oracle, layers, width, fan, seed, with_root):
    """a star (hub 0, 2000 leaves: two levels from anywhere) and, as a component of its own, `layers` layers of `width`
    vertices, every vertex with `fan` random neighbours in the next layer: a traversal from the first layer has one level of
    about 2 * fan * width edges per layer -- too many for a chain launch, and (width * fan large enough) for an M launch.
    with_root: one more vertex joined to the whole first layer, so that those levels start at level 1."""
    rng = np.random.default_rng(seed)
    t0, t1 = [np.zeros(2000, dtype=np.int32)], [np.arange(1, 2001, dtype=np.int32)]
    base = 2001
    for k in range(layers - 1):
        lo = base + k * width
        t0.append(np.repeat(np.arange(lo, lo + width, dtype=np.int32), fan))
        t1.append(rng.integers(lo + width, lo + 2 * width, size=width * fan).astype(np.int32))
    n = base + layers * width
    root = None
    if with_root:
        root = n
        t0.append(np.full(width, root, dtype=np.int32)); t1.append(np.arange(base, base + width, dtype=np.int32))
        n += 1
    ro, ci, _ = oracle.csr_from_tuples(n, np.concatenate(t0), np.concatenate(t1), None, undir=True)
    return n, ro, ci, root if with_root else base


@pytest.mark.parametrize("mini", [None, "2"])
@pytest.mark.parametrize("layout", [False, True])
def test_first_batch_of_a_handle_allocates_and_alternates(gpu_ctx, oracle, monkeypatch, layout, mini):
    """a handle's FIRST batch of two or more sources allocates the second state behind its first two traversals, which run in
    state 0, and alternates from there inside the same batch: fresh handles whose first batch has 4, 5, 6 and 9 sources (seams
    behind the allocation, both parities), then a second batch on the same handle (two states from its first traversal on)"""
    import mini_amd
    if mini is not None:
        monkeypatch.setenv("MGX_BFS_MINI", mini)
    n, ro, ci, w = oracle.rmat_csr(15, 12, 4242)
    deg = np.diff(ro)
    rng = np.random.default_rng(15)
    pool = [int(np.argmax(deg))] + [int(v) for v in rng.choice(np.where(deg > 0)[0], size=7, replace=False)] + [int(np.where(deg == 0)[0][0])]

    def make():
        g = _graph(gpu_ctx, ro, ci)
        if layout:
            g.build_layout()
        return mini_amd.BfsProblem(g, pool[0])

    def body(_, tag):
        res = []
        for count in (4, 5, 6, 9):
            bfs = make()                                  # (a fresh handle: no second state yet)
            res.append(_check_batch(bfs, oracle, ro, ci, pool[:count], (tag, layout, mini, count, "first"))[0])
            res.append(_check_batch(bfs, oracle, ro, ci, pool[:count][::-1], (tag, layout, mini, count, "second"))[0])
        return res

    _both_settings(monkeypatch, make, body)


@pytest.mark.parametrize("old_switches", [False, True])
def test_rerun_of_a_traversal_that_needs_more_slots(gpu_ctx, oracle, monkeypatch, old_switches):
    """the re-run case with the switch on, in batches that DO run in two states: a handle that has only seen the star's hub --
    four plain runs and a warm batch [hub, hub], which allocates the second state and teaches nothing new -- sizes a batch for
    the hub's two levels; the layered component needs a device-wide slot per layer, does not finish inside the batch and is run
    again on its own, in state 0, behind the batch (and the last source once more).  The unfinished traversal's tail chain sits
    in a seam launch (no M launches at this size: k_bfs_seam_chain_init), and its head reaches the host
      * [hub, far, hub, hub]: from state 0, copied by the seam init of the last traversal;
      * [hub, hub, far, hub]: from state 1, by the publish kernel at the end of the batch;
      * [hub, far, hub] (the batch of the test named below): from state 1 again, between two traversals in state 0.
    Each on a fresh handle: a re-run teaches the handle more slots, and the next batch would finish.
    old_switches: the exact setting of test_bfs_run_many_reruns_a_traversal_that_needs_more_slots (no chain launches at all: such a
    batch has no seam launches and takes the one-state path whatever the switch says)"""
    import mini_amd
    if old_switches:
        monkeypatch.setenv("MGX_BFS_CHAIN_MAX_EDGES", "0")
        monkeypatch.setenv("MGX_BFS_SEED_CHAIN", "0")
    n, ro, ci, far = _star_and_layers(oracle, 12, 3000, 5, 11, False)
    hub = 0

    def make():
        bfs = mini_amd.BfsProblem(_graph(gpu_ctx, ro, ci), hub)
        for _ in range(4):
            bfs.run(hub)
        _check_batch(bfs, oracle, ro, ci, [hub, hub], "warm batch")
        return bfs

    def body(_, tag):
        res = []
        for batch in ([hub, far, hub, hub], [hub, hub, far, hub], [hub, far, hub]):
            bfs = make()
            t, reruns = _check_batch(bfs, oracle, ro, ci, batch, (tag, batch))
            assert reruns >= 1, (tag, batch)
            res.append(t)
            res.append(_check_batch(bfs, oracle, ro, ci, [far, far], (tag, batch, "behind"))[0])
            res.append(_check_batch(bfs, oracle, ro, ci, [far, hub, far], (tag, batch, "behind"))[0])
        return res

    _both_settings(monkeypatch, make, body)


@pytest.mark.parametrize("layout", [False, True])
def test_tail_m_launch_forwards_a_level_inside_a_batch(gpu_ctx, oracle, monkeypatch, layout):
    """the M launch behind a traversal's slots finds a level that is too big for it (layers of 20 000 vertices, ~200 000 edges
    a level, limit 131 072) and FORWARDS it -- inside a seam launch, where "the last workgroup through" must count the M
    role's 64 workgroups, not the grid's.  The handle has only seen the star's hub, so the layered traversal runs out of slots
    with every level behind its first still big: whatever its tail M launch gets is forwarded, the chain behind it finds it
    too big as well, the traversal is reported unfinished with its ring entry intact and run again.  A ticket that never
    came up would leave the forwarded level's entry empty: the host would take the traversal for finished, short of
    most of its levels."""
    import mini_amd
    monkeypatch.setenv("MGX_BFS_MINI", "2")
    n, ro, ci, root = _star_and_layers(oracle, 9, 20000, 5, 23, True)
    hub = 0

    def make():
        g = _graph(gpu_ctx, ro, ci)
        if layout:
            g.build_layout()
        bfs = mini_amd.BfsProblem(g, hub)
        for _ in range(4):
            bfs.run(hub)
        return bfs

    def body(bfs, tag):
        t, reruns = _check_batch(bfs, oracle, ro, ci, [hub, root, hub, root, hub], (tag, layout))
        assert reruns >= 1, (tag, layout)
        t2, _ = _check_batch(bfs, oracle, ro, ci, [root, hub, root], (tag, layout))
        return t, t2

    _both_settings(monkeypatch, make, body)
