"""GPU suite (-m gpu): connected components (mgx_cc_*).  The fused path (mgx_cc_run), the operator path
(mgx_cc_enact) and the numpy model (tests/cc_model.py) agree bit for bit -- labels and stats [0] - [2], and the fused path's
skip count (stats[3]) -- on the golden fixtures, R-MAT 10 - 16 symmetric and directed, hand-made shapes and, at full size,
RMAT-20 / RMAT-22, uniform-18 and grid2d-18."""
import os

import numpy as np
import pytest

from tests import cc_model as model
from tests import coloring_model as cm
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
STAT_KEYS = ("components", "largest", "largest_label")


def _graph(ctx, ro, ci, csc=False, layout=False):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    if csc:
        g.build_csc()
    if layout:
        g.build_layout()
    return g


def _check(ctx, ro, ci, symmetric, csc=False, seed=model.SEED, layout=False, want=None):
    """fused == operator path == model (labels, stats [0] - [2]); fused stats[3] == model; returns the labels"""
    import mini_amd
    g = _graph(ctx, ro, ci, csc, layout)
    cp = mini_amd.CcProblem(g)
    sf = cp.run(symmetric, seed)
    lf = cp.labels()
    so = cp.enact()
    lo = cp.labels()
    want = model.labels(ro, ci) if want is None else want
    assert np.array_equal(lf, want), "fused: %d of %d labels differ" % (int((lf != want).sum()), len(want))
    assert np.array_equal(lo, want), "operator path: %d of %d labels differ" % (int((lo != want).sum()), len(want))
    ws = model.stats(want)
    for st in (sf, so):
        assert {k: st[k] for k in STAT_KEYS} == ws, (st, ws)
    if len(want):
        sk = model.skip_stats(ro, ci, seed, symmetric=symmetric, has_csc=csc)
        assert sf["skipped"] == sk["skipped"], (sf, sk["skipped"])
        assert sf["host_waits"] == 1
    assert so["skipped"] == 0 and so["host_waits"] >= 1
    cp.close()
    g.close()
    return want


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("undir", [True, False])
@pytest.mark.parametrize("csc", [False, True])
def test_fixtures(gpu_ctx, oracle, name, undir, csc):
    n, ro, ci, _, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=undir)
    _check(gpu_ctx, ro, ci, symmetric=undir, csc=csc)


@pytest.mark.parametrize("scale,ef", [(10, 1), (11, 2), (12, 4), (13, 8), (14, 16), (15, 1), (16, 16)])
def test_rmat_symmetric(gpu_ctx, oracle, scale, ef):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale)
    _check(gpu_ctx, ro, ci, symmetric=True)


@pytest.mark.parametrize("scale,ef", [(10, 2), (12, 4), (14, 8), (16, 1)])
@pytest.mark.parametrize("csc", [False, True])
def test_rmat_directed(gpu_ctx, oracle, scale, ef, csc):
    n, ro, ci, _ = oracle.rmat_csr(scale, ef, scale + 100, undir=False)
    _check(gpu_ctx, ro, ci, symmetric=False, csc=csc)


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_entries(gpu_ctx, n):
    ro, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    for symmetric in (True, False):
        lab = _check(gpu_ctx, ro, ci, symmetric)
        assert np.array_equal(lab, np.arange(n))


def test_self_loops_and_duplicates(gpu_ctx):
    n = 3000
    v = np.arange(n)
    ro, ci = cm.csr(n, v, v, symmetric=False)                             # self-loops only
    for symmetric in (True, False):
        assert np.array_equal(_check(gpu_ctx, ro, ci, symmetric), v)
    rng = np.random.default_rng(4)
    s, d = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    s, d = np.concatenate([s, s, s, v[::7]]), np.concatenate([d, d, d, v[::7]])   # every pair three times, some self-loops
    ro, ci = cm.csr(n, s, d)
    _check(gpu_ctx, ro, ci, True)
    ro, ci = cm.csr(n, s, d, symmetric=False)
    for csc in (False, True):
        _check(gpu_ctx, ro, ci, False, csc=csc)


@pytest.mark.parametrize("centre", [0, 77777])
def test_star_long_row(gpu_ctx, centre):
    n = 100001
    leaves = np.setdiff1d(np.arange(n), [centre])
    ro, ci = cm.csr(n, np.full(len(leaves), centre), leaves)
    assert ro[centre + 1] - ro[centre] == 100000
    lab = _check(gpu_ctx, ro, ci, True)
    assert (lab == 0).all()
    ro, ci = cm.csr(n, np.full(len(leaves), centre), leaves, symmetric=False)   # only the centre's row
    for csc in (False, True):
        _check(gpu_ctx, ro, ci, False, csc=csc)


def test_work_list_stage_and_segment_edges(gpu_ctx, torch_mod, monkeypatch):
    """k_cc_worklist at its edges, on a one-unit context (8 workgroups: a pass covers 2048 vertices): 3 * 2048 + 1 short rows, all
    listed (directed, no CSC: nothing is skipped), so every wave's stage of 128 goes out inside the loop in its third pass and
    again behind it; a row of exactly CC_SEG entries left to link whose last one is the only entry into the second group, and a
    row of CC_SEG + 1 whose last one -- a segment of its own -- is the only entry into the third."""
    seg, rounds = 2048, 2                                                 # CC_SEG, CC_NEIGHBOR_ROUNDS (include/mgx/cc_fused.hpp)
    groups = [np.arange(0, 2100), np.arange(2100, 4200), np.arange(4200, 3 * 2048 + 1)]
    s = np.concatenate([np.repeat(g, 3) for g in groups])
    d = np.concatenate([g[(np.arange(len(g))[:, None] + [1, 2, 3]) % len(g)].ravel() for g in groups])
    hub_a, hub_b = 3 * 2048 + 1, 3 * 2048 + 2
    row_a = np.concatenate([np.arange(rounds + seg - 1), [groups[1][-1]]])      # rows are sorted: the far group's vertex comes last
    row_b = np.concatenate([np.arange(rounds + seg), [groups[2][-1]]])
    s = np.concatenate([s, np.full(len(row_a), hub_a), np.full(len(row_b), hub_b)])
    d = np.concatenate([d, row_a, row_b])
    n = hub_b + 1
    ro, ci = cm.csr(n, s, d, symmetric=False)
    left = np.diff(ro) - rounds
    assert left[hub_a] == seg and left[hub_b] == seg + 1 and ci[ro[hub_a + 1] - 1] == 4199 and ci[ro[hub_b + 1] - 1] == 3 * 2048
    assert ((left[:hub_a] >= 1) & (left[:hub_a] < 32)).all()              # CC_LONG_MIN
    with one_cu_context(monkeypatch, torch_mod) as one_cu:
        for ctx in (one_cu, gpu_ctx):
            assert (_check(ctx, ro, ci, False) == 0).all()


def test_shuffled_path(gpu_ctx):
    n = 200000
    p = np.random.default_rng(8).permutation(n)
    ro, ci = cm.csr(n, p[:-1], p[1:])
    lab = _check(gpu_ctx, ro, ci, True, want=np.zeros(n, np.int32))
    assert (lab == 0).all()
    ro, ci = cm.csr(n, p[:-1], p[1:], symmetric=False)                     # directed: one out-entry a row
    _check(gpu_ctx, ro, ci, False, want=np.zeros(n, np.int32))


def test_two_cliques_joined_by_one_entry(gpu_ctx):
    k = 300
    rng = np.random.default_rng(2)
    ids = rng.permutation(2 * k + 50)
    a, b = ids[:k], ids[k:2 * k]
    s = np.concatenate([np.repeat(a, k), np.repeat(b, k)])
    d = np.concatenate([np.tile(a, k), np.tile(b, k)])
    n = len(ids)
    ro, ci = cm.csr(n, np.concatenate([s, [a[5]]]), np.concatenate([d, [b[7]]]), symmetric=False)
    lab = _check(gpu_ctx, ro, ci, False)
    assert model.stats(lab)["largest"] == 2 * k
    for csc in (False, True):
        _check(gpu_ctx, ro, ci, False, csc=csc)
    ro, ci = cm.csr(n, np.concatenate([s, [a[5]]]), np.concatenate([d, [b[7]]]))
    _check(gpu_ctx, ro, ci, True)


def test_ten_thousand_small_components(gpu_ctx):
    rng = np.random.default_rng(10)
    sizes = rng.integers(1, 9, 10000)
    n = int(sizes.sum())
    ids = rng.permutation(n)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    s, d = [], []
    for st, sz in zip(starts, sizes):                                     # a random tree per component
        for j in range(1, sz):
            s.append(ids[st + j])
            d.append(ids[st + rng.integers(0, j)])
    ro, ci = cm.csr(n, s, d)
    lab = _check(gpu_ctx, ro, ci, True)
    assert model.stats(lab)["components"] == 10000
    ro, ci = cm.csr(n, s, d, symmetric=False)
    for csc in (False, True):
        _check(gpu_ctx, ro, ci, False, csc=csc)


def _in_entries_only_graph():
    """set A: a directed cycle with one chord (rows [A(i + 1), A(i + 2)] first), so the neighbour rounds make A one set, the
    sampled one; set B: no rows of its own, each b the third or later entry of one A row -- reachable only as in-entries"""
    rng = np.random.default_rng(31)
    na, nb = 2000, 3000
    ids = rng.permutation(na + nb)
    A, B = ids[:na], ids[na:]
    rows = [[A[(i + 1) % na], A[(i + 2) % na]] for i in range(na)]
    for k, b in enumerate(B):
        rows[k % na].append(b)
    n = na + nb
    ro = np.zeros(n + 1, np.int64)
    deg = np.zeros(n, np.int64)
    for i in range(na):
        deg[A[i]] = len(rows[i])
    ro[1:] = np.cumsum(deg)
    ci = np.zeros(int(ro[-1]), np.int32)
    for i in range(na):
        ci[ro[A[i]]:ro[A[i] + 1]] = rows[i]
    return ro.astype(np.int32), ci


def test_directed_connected_only_through_in_entries(gpu_ctx):
    import mini_amd
    ro, ci = _in_entries_only_graph()
    want = np.zeros(len(ro) - 1, np.int32)
    sk = model.skip_stats(ro, ci, symmetric=False, has_csc=True)
    assert sk["skipped"] == 2000                                         # every A row has a B entry left to link
    for csc in (True, False):
        _check(gpu_ctx, ro, ci, False, csc=csc, want=want)
    # the same graph declared symmetric: the skipped rows hid B, which the CSC pass (or no skip) finds
    g = _graph(gpu_ctx, ro, ci, csc=True)
    cp = mini_amd.CcProblem(g)
    st = cp.run(True)
    assert st["components"] == 1 + 3000 and not np.array_equal(cp.labels(), want)
    assert cp.run(False)["components"] == 1 and np.array_equal(cp.labels(), want)
    cp.close()
    g.close()


def _chord_cycle(ids):
    """a cycle over ids with chords to the second and third vertex on: 6 entries a row once symmetrised"""
    return np.concatenate([ids, ids, ids]), np.concatenate([np.roll(ids, 1), np.roll(ids, 2), np.roll(ids, 3)])


def test_seed_changes_the_sample_not_the_labels(gpu_ctx):
    """two components of 5000 and 5001 vertices, each two chord cycles of different sizes joined by one bridge between their
    largest ids: the bridge is no row's first or second entry, so only the final pass joins the halves.  Seeds that sample a half
    of either component as c skip different vertices and give the same labels"""
    rng = np.random.default_rng(5)
    ids = rng.permutation(10001)
    halves = [np.sort(ids[:2400]), np.sort(ids[2400:5000]), np.sort(ids[5000:7450]), np.sort(ids[7450:])]
    s, d = [], []
    for h in halves:
        hs, hd = _chord_cycle(rng.permutation(h))
        s.append(hs)
        d.append(hd)
    bridges = [(halves[0][-1], halves[1][-1]), (halves[2][-1], halves[3][-1])]
    s.append(np.array([x for x, _ in bridges]))
    d.append(np.array([y for _, y in bridges]))
    ro, ci = cm.csr(10001, np.concatenate(s), np.concatenate(d))
    want = model.labels(ro, ci)
    assert model.stats(want)["components"] == 2
    picked = {}                                                   # component label -> (seed, skipped)
    for seed in range(256):
        sk = model.skip_stats(ro, ci, seed)
        part = sk["partition"]
        assert all(part[x] != part[y] for x, y in bridges)      # the neighbour rounds leave every bridge to the final pass
        picked.setdefault(int(want[sk["c"]]), (seed, sk["skipped"]))
        if len(picked) == 2:
            break
    assert len(picked) == 2, picked
    (s0, k0), (s1, k1) = picked.values()
    assert k0 > 0 and k1 > 0 and k0 != k1, picked
    for seed in (s0, s1):
        _check(gpu_ctx, ro, ci, True, seed=seed, want=want)


def test_operator_path_entry_count_not_a_float(gpu_ctx):
    """m = 2^24 + 1 entries, which a float rounds to 2^24: the hook advance still has a slot for every entry"""
    import mini_amd
    n = 1 << 20
    v = np.arange(n, dtype=np.int64)
    ci = ((v[:, None] + np.arange(1, 17)) % n).astype(np.int32).ravel()      # 16 entries a row, v + 1 .. v + 16
    ci = np.concatenate([[0], ci]).astype(np.int32)                           # and a self-loop in row 0
    ro = np.concatenate([[0], 16 * v + 17]).astype(np.int32)
    assert len(ci) == (1 << 24) + 1 and np.float32(len(ci)) == np.float32(1 << 24)
    g = _graph(gpu_ctx, ro, ci)
    cp = mini_amd.CcProblem(g)
    so = cp.enact()
    assert (cp.labels() == 0).all()
    assert {k: so[k] for k in STAT_KEYS} == {"components": 1, "largest": n, "largest_label": 0}
    cp.close()
    g.close()


def test_layout_stream_repeat_and_no_run(gpu_ctx, oracle, torch_mod):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(14, 8, 41)
    want = model.labels(ro, ci)
    _check(gpu_ctx, ro, ci, True, layout=True, want=want)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _check(ctx, ro, ci, True, want=want)
        g = _graph(ctx, ro, ci)
        cp = mini_amd.CcProblem(g)
        with pytest.raises(mini_amd.MgxError):
            cp.labels()
        with pytest.raises(mini_amd.MgxError):
            cp.labels_device_ptr()
        st1 = cp.run(True)
        l1 = cp.labels()
        st2 = cp.run(True)
        assert st1 == st2 and np.array_equal(l1, cp.labels())
        so1 = cp.enact()
        l2 = cp.labels()
        so2 = cp.enact()
        # the operator path's iterations and jump passes (so its host waits) depend on the order its hooks race in; its
        # labels and stats do not
        same = STAT_KEYS + ("skipped",)
        assert {k: so1[k] for k in same} == {k: so2[k] for k in same}
        assert np.array_equal(l2, cp.labels()) and np.array_equal(l1, l2)
        assert {k: so1[k] for k in STAT_KEYS} == {k: st1[k] for k in STAT_KEYS}
        for so in (so1, so2):
            assert so["host_waits"] >= 3                          # a hook advance and its count, then the stats
        assert cp.labels_device_ptr()
        cp.close()
        g.close()
    finally:
        ctx.close()


def test_lspar_result_components(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, _ = oracle.rmat_csr(14, 16, 14)
    g = _graph(gpu_ctx, ro, ci)
    lp = mini_amd.LsparProblem(g)
    lp.run()
    sro, sci, _, _ = lp.result()
    sg = lp.graph()
    cp = mini_amd.CcProblem(sg)
    want = model.labels(sro, sci)
    st = cp.run(False)
    assert np.array_equal(cp.labels(), want)
    assert {k: st[k] for k in STAT_KEYS} == model.stats(want)
    cp.enact()
    assert np.array_equal(cp.labels(), want)
    cp.close()
    sg.close()
    lp.close()
    g.close()


def _device_graph(ctx, d, csc=False):
    import mini_amd
    g = mini_amd.Graph.from_device(ctx, d["n"], d["m"], d["row_offsets"], d["col_indices"])
    if csc:
        g.build_csc()
    return g


@pytest.mark.parametrize("scale", [16, 20])
def test_bfs_from_largest_label_reaches_its_component(gpu_ctx, scale):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    d = rmat_csr(gpu_ctx, scale, 16)
    g = _device_graph(gpu_ctx, d)
    cp = mini_amd.CcProblem(g)
    st = cp.run(True)
    lab = cp.labels()
    bfs = mini_amd.BfsProblem(g, st["largest_label"])
    bfs.run(st["largest_label"])
    reached = bfs.labels() >= 0
    assert np.array_equal(reached, lab == st["largest_label"])
    assert int(reached.sum()) == st["largest"]
    bfs.close()
    cp.close()
    g.close()


def test_rmat20_against_model(gpu_ctx, oracle):
    n, ro, ci, _ = oracle.rmat_csr(20, 16, 20)
    _check(gpu_ctx, ro, ci, True)


def _device_check(torch, ro, ci, lab):
    """on the device: entries' endpoints share a label; label[v] <= v and labels are fixed points; a min-label propagation
    (with pointer jumping) from the identity reaches the same labels"""
    n = ro.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, device=ro.device, dtype=torch.int64), (ro[1:] - ro[:-1]).long())
    cols = ci.long()
    assert bool((lab[rows] == lab[cols]).all().item())
    v = torch.arange(n, device=ro.device, dtype=torch.int64)
    assert bool((lab <= v).all().item()) and bool((lab[lab] == lab).all().item())
    cur = v.clone()
    for _ in range(200):
        nxt = cur.clone()
        nxt.scatter_reduce_(0, rows, cur[cols], reduce="amin")
        nxt.scatter_reduce_(0, cols, cur[rows], reduce="amin")
        nxt = nxt[nxt]
        if torch.equal(nxt, cur):
            break
        cur = nxt
    assert torch.equal(cur, lab)


def test_rmat22_fused_equals_operator_path(gpu_ctx, torch_mod):
    import mini_amd
    from mini_amd.rmat import rmat_csr
    torch = torch_mod
    d = rmat_csr(gpu_ctx, 22, 16)
    g = _device_graph(gpu_ctx, d)
    cp = mini_amd.CcProblem(g)
    sf = cp.run(True)
    lf = cp.labels()
    so = cp.enact()
    assert np.array_equal(lf, cp.labels())
    assert {k: sf[k] for k in STAT_KEYS} == {k: so[k] for k in STAT_KEYS}
    assert sf["host_waits"] == 1 and sf["skipped"] > 0
    _device_check(torch, d["row_offsets"], d["col_indices"], torch.from_numpy(lf).long().to(d["row_offsets"].device))
    cp.close()
    g.close()


@pytest.mark.parametrize("kind", ["uniform", "grid2d"])
def test_scale18_uniform_grid_single_component(gpu_ctx, kind):
    import mini_amd
    from mini_amd.rmat import grid2d_csr, uniform_csr
    d = (uniform_csr if kind == "uniform" else grid2d_csr)(gpu_ctx, 18)
    g = _device_graph(gpu_ctx, d)
    cp = mini_amd.CcProblem(g)
    sf = cp.run(True)
    lf = cp.labels()
    so = cp.enact()
    assert np.array_equal(lf, cp.labels())
    assert (lf == 0).all()
    for st in (sf, so):
        assert {k: st[k] for k in STAT_KEYS} == {"components": 1, "largest": d["n"], "largest_label": 0}
    cp.close()
    g.close()
