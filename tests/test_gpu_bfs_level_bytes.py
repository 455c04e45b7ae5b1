"""Fused BFS: the queue build's level bytes and their translation (mgx/bfs_fused.hpp: lvl8, bfs_translate_body; MGX_BFS_LEVEL_BYTES).

Under a hub-first layout k_bfs_build2 stores the level of a discovery as a byte in layout order (levels up to 254) instead of
scattering labels[old_of_new[v]], and a translation role beside the batch of launches' tail writes the labels.  Every case here runs on
a fresh Graph and BfsProblem with the switch on and with MGX_BFS_LEVEL_BYTES=0 and asserts that labels, levels / reached / m_t, the level
trace and the path counters are the same in both and the labels those of the construction (tests/bfs_cases.py) or of the CPU oracle --
on the device's own grids and on one compute unit's (tests/grid_cus.py).  `level_byte_slot` (stats entry 22) is 1 + the last slot whose
build stored a byte, 0 when none did: what the translation role looks at before it sweeps."""
import numpy as np
import pytest

from tests import bfs_cases as bc
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

rows = bc.rows
SWITCHES = sorted({k for c in bc.CASES.values() for k in c["env"]} |
                  {"MGX_BFS_LEVEL_BYTES", "MGX_BFS_BATCH_OVERLAP", "MGX_BFS_MINI", "MGX_BFS_BUILD_LIST"})
SAME = ("levels", "reached", "m_t", "frontier_vertices", "push_levels", "small_levels", "slots", "dense_slots", "vshort_slots",
        "lazy_slots", "cold_slots", "mini_slots", "pull_edges")


@pytest.fixture(params=["device", "one_cu"])
def ctx(request, built, torch_mod, monkeypatch):
    if request.param == "device":
        yield request.getfixturevalue("gpu_ctx")
    else:
        with one_cu_context(monkeypatch, torch_mod) as c:
            yield c


def _on_and_off(ctx, monkeypatch, env, ro, ci, body, layout=True, src=0):
    """body(bfs, on) -> anything comparable, on a fresh graph and handle with the switch on, then off: both results must be equal"""
    import mini_amd
    out = []
    for on in (True, False):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if not on:
            monkeypatch.setenv("MGX_BFS_LEVEL_BYTES", "0")
        G = mini_amd.Graph.from_host(ctx, np.ascontiguousarray(ro, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), None)
        if layout:
            G.build_layout()
        bfs = mini_amd.BfsProblem(G, int(src))
        try:
            out.append(body(bfs, on))
        finally:
            bfs.close()
            G.close()
    assert out[0] == out[1], "the switch changed a counter or the trace"
    return out[0]


def _one(bfs, src, want, tag, mode=0, alpha=0.0):
    """a traversal: labels against `want`; what must not depend on the switch, and the level-byte flag"""
    st = bfs.run(int(src), mode, alpha)
    lab = bfs.labels()
    assert np.array_equal(lab, want), (tag, int((lab != want).sum()), np.flatnonzero(lab != want)[:8])
    return {k: st[k] for k in SAME}, bfs.level_trace(), st["level_byte_slot"]


def _runs(g, times=2, expect_bytes=None, mode=0):
    """body: `times` traversals from the graph's source on one handle"""
    def body(bfs, on):
        res = []
        for i in range(times):
            same, trace, flag = _one(bfs, g.src, g.labels, ("run", i, "on" if on else "off"), mode)
            assert same["reached"] == g.reachable and same["levels"] == len([1 for d, _, _ in g.level_rows if (d > 0).any()])
            if not on:
                assert flag == 0
            elif expect_bytes is not None:
                assert (flag > 0) == expect_bytes, (i, flag)
            res.append((same, trace))
        return res
    return body


# ---- the byte / int cut: labels up to 254 are bytes, from 255 on the build's int stores ------------------------------------------------
def _deep(last_label, ids=7):
    # a few vertices per level, every level a device-wide slot (WIDE): level k's three rows each discover one vertex of level k + 1
    return bc.Layered([[rows(1, 3, 3)]] + [[rows(3, 1, 1)]] * (last_label - 1) + [[rows(3, 0)]], pad=5, ids=ids)


@pytest.mark.parametrize("last_label", [259, 254, 255])
def test_cut_between_byte_and_int_levels(ctx, monkeypatch, last_label):
    """259: labels 253, 254 (the last byte level), 255 (the first int one) and 256 inside the traversal; 254 / 255: the cut on the
    traversal's last level -- nothing / one level on the int path.  A fresh handle (slot hint 5) needs several batches of slots: the
    later ones translate again, and those that begin behind level 254 have nothing to translate.  Chains are off: the translation is a
    launch of its own behind every batch."""
    g = _deep(last_label)
    assert g.labels.max() == last_label and all(int((g.labels == k).sum()) == 3 for k in (253, 254, last_label))
    res = _on_and_off(ctx, monkeypatch, bc.WIDE, g.ro, g.ci, _runs(g, times=2, expect_bytes=True), src=g.src)
    assert res[0][0]["slots"] >= last_label and res[0][0]["small_levels"] == 0


def test_cut_with_the_tail_chain_launch(ctx, monkeypatch):
    """the same depth with the chains on and levels too big for them (4200 entries each, all but three filler): every level a slot, the
    translation beside the in-place chain launch behind every batch of slots"""
    g = bc.Layered([[rows(1, 3, 3)]] + [[rows(1, 4198, 1), rows(2, 1, 1)]] * 257 + [[rows(3, 0)]], pad=5, ids=7)
    assert g.labels.max() == 258
    res = _on_and_off(ctx, monkeypatch, {}, g.ro, g.ci, _runs(g, times=2, expect_bytes=True), src=g.src)
    assert res[0][0]["slots"] >= 257


# ---- mixed writers: chain -> M launch -> slot (lazy build) -> slot -> M launch -> chain ------------------------------------------------
def _mixed(ids):
    return bc.Layered([
        [rows(1, 4, 4)],                       # 0: the in-place chain's
        [rows(4, 512, 512)],                   # 1: 2048 entries, early: the M launch's in front of the slots
        [rows(2048, 20, 20)],                  # 2: a slot; 40960 marks of n = 99013: its build is lazy
        [rows(2000, 40, 1), rows(38960, 0)],   # 3: a slot on the queue-less bodies; 2000 marks: its build writes queues
        [rows(2000, 10, 1)],                   # 4: 20000 entries, late: the M launch's behind the slots (a handle that enqueues two) or a slot's
        [rows(2000, 1, 1)],                    # 5: the chain's
        [rows(2000, 0)],
    ], pad=50000, ids=ids)


@pytest.mark.parametrize("ids", ["spec", 7])
def test_mixed_writers(ctx, monkeypatch, ids):
    """every vertex's label comes from exactly one writer -- the chain, an M launch, or a build's byte through the translation --, the
    isolated vertices stay -1; ids as specified: the source is vertex 0"""
    g = _mixed(ids)
    assert ids != "spec" or g.src == 0
    res = _on_and_off(ctx, monkeypatch, dict(bc.MINI, **bc.RULES), g.ro, g.ci, _runs(g, times=3, expect_bytes=True), src=g.src)
    print([r[0] for r in res])
    assert all(r[0]["lazy_slots"] == 1 and r[0]["mini_slots"] >= 1 and r[0]["small_levels"] >= 3 for r in res)
    # (a fresh handle enqueues five slots and ends on the chain; once it has learnt the traversal an M launch runs behind the slots too)
    assert res[0][0]["mini_slots"] == 1 and any(r[0]["mini_slots"] == 2 for r in res[1:])
    assert int((g.labels == -1).sum()) == 50000


# ---- edges of the sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [15, 16, 17, 16385 - 16, 16385, 16385 + 16])
def test_sweep_edges(ctx, monkeypatch, n):
    """a star over n vertices: a build discovers every vertex but the source -- the one whose layout id is n - 1 among them; n % 16 in
    {15, 0, 1}: the build's last 16-byte piece and the translation's last trip are partial, whole, one vertex"""
    g = bc.Layered([[rows(1, n - 1, n - 1)], [rows(n - 1, 0)]], ids=3)
    assert g.n == n
    _on_and_off(ctx, monkeypatch, bc.WIDE, g.ro, g.ci, _runs(g, times=2, expect_bytes=True), src=g.src)


# ---- no bytes, no sweep --------------------------------------------------------------------------------------------------------------------
def test_chains_alone_store_no_byte(ctx, monkeypatch):
    g = bc.Layered([[rows(1, 4, 4)], [rows(4, 4, 4)], [rows(16, 4, 1)], [rows(16, 0)]], pad=9, ids=7)
    res = _on_and_off(ctx, monkeypatch, {}, g.ro, g.ci, _runs(g, times=2, expect_bytes=False), src=g.src)
    assert all(r[0]["small_levels"] == 3 for r in res)


# ---- the path is off: no layout, the list-based build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,layout", [({}, False), ({"MGX_BFS_BUILD_LIST": "1"}, True)])
def test_path_off(ctx, monkeypatch, env, layout):
    g = _mixed(7)
    _on_and_off(ctx, monkeypatch, dict(bc.MINI, **bc.RULES, **env), g.ro, g.ci, _runs(g, times=2, expect_bytes=False), layout=layout, src=g.src)


# ---- batches of sources ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat12(gpu_ctx, oracle):
    from mini_amd import rmat
    g = rmat.rmat_csr(gpu_ctx, scale=12, edgefactor=16, seed=12)
    ro, ci = g["row_offsets"].cpu().numpy(), g["col_indices"].cpu().numpy()
    srcs = [int(s) for s in rmat.pick_sources(ro, 5, 12)]
    return ro, ci, srcs, {s: oracle.bfs_cpu(ro, ci, s) for s in srcs}


@pytest.mark.parametrize("env,mode", [({}, 0), ({"MGX_BFS_BATCH_OVERLAP": "0"}, 0), ({"MGX_BFS_MINI": "0"}, 0), ({"MGX_BFS_MINI": "2"}, 0),
                                      ({}, 1)],
                         ids=["default", "one_state", "no_mini", "mini", "direction_opt"])
def test_batches(ctx, monkeypatch, rmat12, env, mode):
    """run_many over 2, 3 and 5 sources on one handle: the batch that allocates the second state and the ones behind it, both states,
    seams with and without M launches; labels() are the last source's, the earlier ones are checked by batches that end on them"""
    ro, ci, srcs, want = rmat12

    def body(bfs, on):
        res = []
        for batch in (srcs[:2], srcs[:3], srcs[:5], srcs[1:4][::-1], srcs[3:0:-1], [srcs[4], srcs[0]]):
            stats, reruns = bfs.run_many(batch, mode, 4.0 if mode else 0.0)
            assert np.array_equal(bfs.labels(), want[batch[-1]]), (batch, "on" if on else "off")
            for s, st in zip(batch, stats):
                assert st["reached"] == int((want[s] >= 0).sum()), (batch, s, st)
            res.append(([{k: st[k] for k in SAME if k != "slots"} for st in stats], reruns))
        same, trace, _ = _one(bfs, srcs[2], want[srcs[2]], "a single call behind the batches", mode, 4.0 if mode else 0.0)
        res.append((same, trace))
        return res
    _on_and_off(ctx, monkeypatch, env, ro, ci, body, src=srcs[0])
