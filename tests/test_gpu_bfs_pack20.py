"""Fused BFS: the unit blocks without the cold-edge lists' entries at 20 bits per entry (mgx/pack20.hpp, MGX_BFS_PACK20).

Those blocks exist only where cold-edge lists do: n a little above the LDS prefix (bfs_cases.HOT_N = 652 288 vertices), a few long
rows, few cold entries.  The graphs here are layered like tests/bfs_cases.py's -- source -> level-1 rows -> level-2 leaves, labels
known by construction -- but written out entry by entry, because WHICH id sits in WHICH slot of a lane's five words is the point
(Layered deals ids, it does not take them).  Vertices are numbered by non-increasing degree and every row is sorted, so the
layout's renumbering (stable, by degree) is the identity and the blocks hold exactly the ids written here; the test checks that.

  * every slot 0..7 of a lane carries, in some row, each of 0, 1, 0x55555, 0x80000 (bit 19: a sign-extending unpack loses it),
    0x8AAAA and 652 287 (the last id of the prefix), the entry in front and the one behind of the opposite bit pattern, the rest of
    the row ids that no other row names -- a field that bleeds into its neighbour loses a level-2 vertex and marks a stranger
  * rows of 63, 64, 65, 127, 128, 129 hot entries (unit padding reads as "no entry"), six of them with cold entries as well
  * unit counts that are no multiple of 8 or 16 (chunk and group tails, the slack behind the array); the "bulk" graph has enough
    units for every wave of a one-compute-unit grid to take several batches
"""
import functools

import numpy as np
import pytest

from tests import bfs_cases as bc
from tests.grid_cus import one_cu_context

N = 700001
HOT_N = bc.HOT_N
TARGETS = (0, 1, 0x55555, 0x80000, 0x8AAAA, HOT_N - 1)
LENS = (63, 64, 65, 127, 128, 129)
# target -> (the entry in front, the entry behind, where the unique ids in front of that end (descending; None: copies of the entry
# in front), where the unique ids behind start (ascending; None: copies -- nothing hot lies above))
BESIDE = {
    0: (0, 0x7FFFF, None, 0x80100),
    1: (0, 0x7FFFE, None, 0x81100),
    0x55555: (0x2AAAA, 0x8AAAA, 0x2AAAA - 0x100, 0x8CBAA),
    0x80000: (0x7FFFF, HOT_N - 1, 0x7FFFF - 0x100, None),
    0x8AAAA: (0x75555, 0x95555, 0x75555 - 0x100, 0x99655),
    HOT_N - 1: (0x60C00, HOT_N - 1, 0x60C00 - 0x100, None),
}
ENV = dict(bc.WIDE, MGX_BFS_DENSE="1000000", MGX_BFS_LAZY="0")      # every level a device-wide slot that reads the unit blocks
SWITCHES = sorted(set(ENV) | {"MGX_BFS_PACK20", "MGX_BFS_PACK24", "MGX_BFS_HOT_UNITS", "MGX_BFS_COLD", "MGX_BFS_COLD_LISTS", "MGX_BFS_LONG_MIN"})
EXACT = ("levels", "reached", "m_t", "frontier_vertices", "push_levels", "small_levels", "dense_slots", "vshort_slots", "lazy_slots",
         "cold_slots", "mini_slots", "pull_edges")
GRAPHS = {"small": (0, 0), "bulk": (10, 3000)}          # name -> (extra one-unit rows, bulk rows of 192 entries)


class Graph20:
    pass


@functools.lru_cache(maxsize=None)
def graph(name):
    extra, bulk = GRAPHS[name]
    rows, slots, used = [], set(), set()                # rows: (hot entries, cold entries)
    cold_next = HOT_N
    for xi, X in enumerate(TARGETS):
        lo, hi, below, above = BESIDE[X]
        for p in range(8):
            L = LENS[(xi + p) % 6]
            i = p + 8 * ((3 * xi + p) % (L // 8))        # X's index in its row: slot p of lane i >> 3 of the row's unit i >> 6
            nb, na = i, L - i - 1
            front, behind = [], []
            if nb:
                uniq = [] if below is None else [below - k for k in range(nb - 1)]
                if below is not None:
                    below -= nb - 1
                front = (sorted(uniq) + [lo]) if uniq or below is not None else [lo] * nb
            if na:
                uniq = [] if above is None else [above + k for k in range(na - 1)]
                if above is not None:
                    above += na - 1
                behind = ([hi] + uniq) if above is not None else [hi] * na
            for u in (front[:-1] if BESIDE[X][2] is not None else []) + (behind[1:] if BESIDE[X][3] is not None else []):
                assert u not in used and u not in TARGETS and 0 < u < HOT_N
                used.add(u)
            hot = front + [X] + behind
            assert len(hot) == L and hot == sorted(hot) and hot[i] == X and max(hot) < HOT_N
            cold = []
            if p == 0:                                  # six rows with cold entries: the first and the last cold id among them
                k = 40 if xi == 0 else 3
                cold = list(range(cold_next, cold_next + k - 1)) + [N - 1 - xi]
                cold_next += k - 1
            slots.add((X, i % 8))
            rows.append((hot, cold))
    for r in range(extra):                               # one unit each: they only move the unit count
        rows.append(([0x10000 + 64 * r + k for k in range(64)], []))
    for r in range(bulk):
        rows.append((sorted(100000 + (r * 191 + 3 * k) % 400000 for k in range(192)), []))
    assert slots == {(X, p) for X in TARGETS for p in range(8)}
    rows.sort(key=lambda hc: -(len(hc[0]) + len(hc[1])))        # (stable) ids by non-increasing degree: the layout keeps them
    R = len(rows)
    d0 = max(R, len(rows[0][0]) + len(rows[0][1]))
    src_row = [0] * (d0 - R) + list(range(1, R + 1))             # the source names every row (and itself: filler)
    assert R + 1 < 0x10000
    all_rows = [(src_row, [])] + rows
    deg = np.zeros(N, dtype=np.int64)
    deg[:R + 1] = [len(h) + len(c) for h, c in all_rows]
    assert np.all(np.diff(deg) <= 0)
    g = Graph20()
    g.n, g.src, g.R = N, 0, R
    g.ro = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    g.ci = np.concatenate([np.array(h + c, dtype=np.int32) for h, c in all_rows])
    g.deg = deg
    g.labels = np.full(N, -1, dtype=np.int32)
    g.labels[g.ci[g.ro[1]:]] = 2                                 # whatever a level-1 row names ...
    g.labels[1:R + 1] = 1                                        # ... unless it is a level-1 row itself
    g.labels[0] = 0
    g.levels = 2                                                 # the leaves have no entries: no third level is opened
    g.reached = int((g.labels >= 0).sum())
    g.m_t = int(deg[g.labels >= 0].sum())
    long_rows = [(h, c) for h, c in all_rows if len(h) + len(c) >= 32]
    g.units = sum((len(h) + len(c) + 63) // 64 for h, c in long_rows)
    g.hot_units = sum((len(h) + 63) // 64 for h, c in long_rows)
    g.cold_pairs = sum(len(c) for h, c in long_rows)
    return g


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graphs_are_what_they_promise(name):
    g = graph(name)
    assert np.array_equal(bc.numpy_bfs(g.ro, g.ci, g.src), g.labels)
    assert g.hot_units % 8 != 0 and g.hot_units % 16 != 0, g.hot_units
    assert 0 < g.cold_pairs * 4 <= g.units * 64                  # the layout builds the lists, hence the blocks without their entries
    assert int(g.labels.max()) == g.levels and g.n > HOT_N
    # rows of every length in LENS hold hot entries only up to the prefix, the cold ones behind them
    hot_len = {int((g.ci[g.ro[v]:g.ro[v + 1]] < HOT_N).sum()) for v in range(1, g.R + 1)}
    assert set(LENS) <= hot_len


def _run(ctx, monkeypatch, oracle, g, pack20, tag):
    import mini_amd
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    if pack20 is not None:
        monkeypatch.setenv("MGX_BFS_PACK20", pack20)
    G = mini_amd.Graph.from_host(ctx, g.ro, g.ci, None)
    G.build_layout()
    info = G.layout_info()
    lro, lci, _, _ = G.layout_arrays()
    assert np.array_equal(lro, g.ro) and np.array_equal(lci[:len(g.ci)], g.ci), "the layout keeps the ids: the blocks hold what was written"
    assert (info["units"], info["hot_units"], info["cold_pairs"]) == (g.units, g.hot_units, g.cold_pairs), (tag, info)
    bfs = mini_amd.BfsProblem(G, g.src)
    want = oracle.bfs_cpu(g.ro, g.ci, g.src)
    assert np.array_equal(want, g.labels)
    runs = []
    for i in range(3):
        st = bfs.run(g.src)
        lab = bfs.labels()
        bad = np.flatnonzero(lab != g.labels)
        assert len(bad) == 0, (tag, i, "first differences (vertex, got, want)", [(int(v), int(lab[v]), int(g.labels[v])) for v in bad[:8]])
        got = {k: st[k] for k in EXACT}
        print(tag, "run", i, "slots", st["slots"], got, "device_bytes", info["device_bytes"])
        assert (st["levels"], st["reached"], st["m_t"]) == (g.levels, g.reached, g.m_t), (tag, i, got)
        assert st["dense_slots"] >= 1 and st["cold_slots"] >= 1, (tag, i, got)      # the body under test really ran
        runs.append(got)
    assert all(r == runs[0] for r in runs), (tag, runs)
    bfs.close()
    G.close()
    return runs[0], info


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_pack20_on_and_off(gpu_ctx, oracle, monkeypatch, name):
    g = graph(name)
    on, info_on = _run(gpu_ctx, monkeypatch, oracle, g, None, (name, "unset"))
    off, info_off = _run(gpu_ctx, monkeypatch, oracle, g, "0", (name, "0"))
    assert on == off, (name, on, off)
    assert info_on["device_bytes"] < info_off["device_bytes"], (info_on, info_off)
    # what the switch is about: hot_units_pad * 64 entries at 20 instead of 24 bits (and the few words of slack behind either array)
    pad = (g.hot_units + 15) // 16 * 16
    assert info_off["device_bytes"] - info_on["device_bytes"] == ((pad * 16 + 1) * 3 + 4) * 4 - (pad * 64 * 20 // 8 + 32), (info_on, info_off)


@pytest.mark.gpu
@pytest.mark.parametrize("pack20", [None, "0"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_pack20_on_one_compute_unit(built, torch_mod, oracle, monkeypatch, name, pack20):
    """grids of one compute unit's workgroups: on the bulk graph every wave takes several batches of groups"""
    g = graph(name)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _run(ctx, monkeypatch, oracle, g, pack20, (name, pack20, "one CU"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lengths_dense32", "lengths_dense"])
def test_split_launch_reads_the_full_blocks_as_before(gpu_ctx, monkeypatch, name):
    """the timing runs' long-rows launch (the parts of a push as launches of their own) carries the 20-bit body too and keeps the
    steps of its 32-bit body as a loop: rows of 63 .. 129 entries from the full blocks at 32 and at 24 bits, labels as constructed"""
    import mini_amd
    case = bc.CASES[name]
    for k in SWITCHES + sorted(case["env"]):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    g = case["graph"]("at", 7)
    G = mini_amd.Graph.from_host(gpu_ctx, g.ro, g.ci, None)
    G.build_layout()
    assert G.layout_info()["units_24bit"] == (0 if name == "lengths_dense32" else 1)
    bfs = mini_amd.BfsProblem(G, g.src)
    bfs.set_kernel_timing(True)
    for i in range(2):
        st = bfs.run(g.src)
        assert np.array_equal(bfs.labels(), g.labels), (name, i)
        assert st["dense_slots"] >= 1 and st["reached"] == g.reachable, (name, i, st["dense_slots"], st["reached"])
    bfs.close()
    G.close()
