"""Inputs of the fused colouring's path tests, shared by the CPU suite (tests/test_coloring_cases_cpu.py: by
tests/coloring_model.py alone, each case has the property it was built for) and the GPU suite
(tests/test_gpu_coloring_paths.py: fused path == operator path == model on them, and the row classes the library reports are the
predicted ones).  numpy only; everything is generated from the thresholds handed in (include/mgx/color_fused.hpp: rows of at
least long_min entries are long, a wave scans seg entries, a wave's stage holds `stage` segments).

Builders return (row_offsets, col_indices) as int32.  The helpers below them read a finished colouring: a vertex is uncoloured at
the start of round i when its final colour is 0 or above 2i."""
import numpy as np

from tests import coloring_model as model

LONG_MIN, SEG, STAGE, BATCH_MAX = 32, 2048, 128, 128      # today's constants (the GPU suite passes ColorProblem.info()'s)
FIRST_BATCH = 8                                           # rounds the host enqueues before its first wait
EDGE_TAILS = (1, 31, 33)                                  # n = 128 j + each: the bitmap's last word, last uint4


def edge_degrees(long_min=LONG_MIN, seg=SEG):
    return (0, 1, long_min - 1, long_min, long_min + 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1)


def _csr_of_rows(n, rows):
    """rows: {vertex: neighbour array}; the other vertices have no entries"""
    deg = np.zeros(n, dtype=np.int64)
    for v, r in rows.items():
        deg[v] = len(r)
    ro = np.concatenate([[0], np.cumsum(deg)])
    ci = np.zeros(int(ro[-1]), dtype=np.int32)
    for v, r in rows.items():
        ci[ro[v]:ro[v + 1]] = r
    return ro.astype(np.int32), ci


def degree_edges(n, long_min=LONG_MIN, seg=SEG, seed=model.SEED, graph_seed=1):
    """Directed, ragged: of every degree of edge_degrees() three rows of random neighbours (from 2 entries on they almost surely
    survive round 0) and, from 1 entry on, one row drawn at random from the vertices of a larger round-0 key and one from those of a
    smaller (decided in round 0 as 2i + 1 and 2i + 2 after every segment was read to its end).  Vertex n - 1 has a random row of
    long_min + 1 entries that holds the smallest and the largest round-0 key; every other vertex has 0 .. 5.  -> (ro, ci, {degree: its vertices})"""
    rng = np.random.default_rng(graph_seed)
    key = model.keys(n, model.salt(seed, 0))
    order = np.argsort(key)                                # vertices by round-0 key
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    free = rng.permutation(n - 1)                          # (n - 1 is taken)
    mid = [int(v) for v in free if n // 4 <= rank[v] < 3 * n // 4]      # rows that must find a key on either side
    rows, by_degree, at = {}, {}, 0
    for d in edge_degrees(long_min, seg):
        mine = []
        for kind in ("random", "random", "random", "above", "below"):
            if kind != "random" and d == 0:
                continue
            v = mid[at]
            at += 1
            if kind == "random":
                r = rng.integers(0, n, d)
            elif kind == "above":                          # every neighbour's key is larger: v is a minimum
                r = order[rng.integers(rank[v] + 1, n, d)]
            else:
                r = order[rng.integers(0, rank[v], d)]
            rows[v] = r.astype(np.int32)
            mine.append(v)
        by_degree[d] = mine
    last = rng.integers(0, n, long_min + 1)                # vertex n - 1 sees the smallest and the largest key: it survives round 0
    last[:2] = [order[0] if order[0] != n - 1 else order[1], order[-1] if order[-1] != n - 1 else order[-2]]
    rows[n - 1] = last.astype(np.int32)
    for v in range(n - 1):
        if v not in rows:
            rows[v] = rng.integers(0, n, int(rng.integers(0, 6))).astype(np.int32)
    ro, ci = _csr_of_rows(n, rows)
    return ro, ci, by_degree


def hub_clique(h, leaves):
    """h hubs, pairwise adjacent, `leaves` private leaves each, symmetric.  Hub j is vertex j * (leaves + 1) and its leaves follow it,
    so a hub's row is: the hubs below it, its leaves, the hubs above it -- the first and the last segment hold the other hubs.
    -> (ro, ci, hub ids)"""
    step = leaves + 1
    hubs = np.arange(h, dtype=np.int64) * step
    a, b = np.meshgrid(hubs, hubs, indexing="ij")
    m = a != b
    leaf_of = np.repeat(hubs, leaves)
    leaf = leaf_of + np.tile(np.arange(1, leaves + 1, dtype=np.int64), h)
    ro, ci = model.csr(h * step, np.concatenate([a[m], leaf_of, leaf]), np.concatenate([b[m], leaf, leaf_of]), symmetric=False)
    return ro, ci, hubs.astype(np.int64)


def hub_clique_leaves(h, seg=SEG):
    """rows of three segments, the last one short of full"""
    return 3 * seg - 6 * h


def shared_leaf_hubs(lengths, clique=False):
    """Directed: hub r (vertex r) has the first lengths[r] leaves as its row, the leaves (vertices len(lengths) ..) have none.  Every
    leaf is coloured 1 in round 0; a hub with a leaf key on either side survives it and is coloured 3 in round 1.
    clique: every hub's row ENDS with the other hubs (rows are read as they stand), so from round 1 on the hubs colour each other two a
    round and all a row's evidence lies in its last segment."""
    hubs = len(lengths)
    n = hubs + int(max(lengths))
    others = np.arange(hubs, dtype=np.int32)
    rows = {r: np.concatenate([np.arange(hubs, hubs + int(d), dtype=np.int32), others[others != r] if clique else others[:0]])
            for r, d in enumerate(lengths)}
    return _csr_of_rows(n, rows)


def beyond_stage_lengths(seg=SEG, stage=STAGE):
    """the last row whose segments fit the stage, the first that goes out on its own, and one well beyond"""
    return (stage * seg, stage * seg + 1, (6 * stage * seg) // 5 + 13)


def stage_pressure_lengths(seg=SEG, stage=STAGE, rows=96):
    """rows of stage / 3 + 1 segments each: two of them fit a wave's stage, the third makes it flush"""
    segs = stage // 3 + 1
    return tuple((segs - 1) * seg + 1 + 7 * r for r in range(rows))


ONE_UNIT_WAVES = 32                                       # waves of a grid of one compute unit: 8 workgroups of 4


LATE_EVIDENCE_ROWS = 8                                    # shared_leaf_hubs(stage_pressure_lengths(seg, stage, 8), clique=True): rows of
#   stage / 3 + 1 segments, more than ONE_UNIT_WAVES, so on a grid of one compute unit the wave that scans a row's last segment has
#   scanned an earlier one of the same row before


# ---- reading a finished colouring -----------------------------------------------------------------------------------------------

def uncoloured_at(colours, i):
    c = np.asarray(colours)
    return (c == 0) | (c > 2 * i)


def truncated(want, max_iter):
    """the model's result after max_iter rounds, from its result of a run to the end (a round reads the state at its start only;
    tests/test_coloring_cases_cpu.py compares with the model run that far)"""
    colours, trace, _ = want
    if max_iter <= 0 or max_iter >= len(trace):
        return want
    c = np.where(colours <= 2 * max_iter, colours, 0).astype(np.int32)
    return c, trace[:max_iter], int((c == 0).sum())


def round_rows(ro, colours, rounds, long_min=LONG_MIN, seg=SEG):
    """per round run, what mgx_color_info reports: short rows, long items, long rows uncoloured at the start of the round"""
    deg = np.diff(np.asarray(ro, dtype=np.int64))
    is_long = deg >= long_min
    segs = (deg + seg - 1) // seg
    out = np.zeros((rounds, 3), dtype=np.int64)
    for i in range(rounds):
        u = uncoloured_at(colours, i)
        out[i] = (int((u & ~is_long).sum()), int(segs[u & is_long].sum()), int((u & is_long).sum()))
    return out


def segment_views(ro, ci, colours, seed, i, v, seg=SEG):
    """row v in round i -> (segments holding an uncoloured neighbour of a smaller key, ... of a larger key), two sets"""
    n = len(ro) - 1
    key = model.keys(n, model.salt(seed, i))
    unc = uncoloured_at(colours, i)
    row = np.asarray(ci[ro[v]:ro[v + 1]], dtype=np.int64)
    s = np.arange(len(row)) // seg
    live = unc[row] & (row != v)
    below = set(s[live & (key[row] < key[v])].tolist())
    above = set(s[live & (key[row] > key[v])].tolist())
    return below, above


def split_rows(ro, ci, colours, seed, vertices, seg=SEG):
    """over the rounds >= 1 the given multi-segment rows start uncoloured: (rows whose below- and above-segments are both non-empty
    and disjoint -- only the combined tally tells that they survive --, rows with a segment that sees both), as (round, vertex) lists"""
    disjoint, both = [], []
    last = int(np.asarray(colours).max() + 1) // 2
    for i in range(1, last + 1):
        unc = uncoloured_at(colours, i)
        for v in vertices:
            if not unc[v]:
                continue
            b, a = segment_views(ro, ci, colours, seed, i, int(v), seg)
            if b and a and not (b & a):
                disjoint.append((i, int(v)))
            if b & a:
                both.append((i, int(v)))
    return disjoint, both


HUB_CLIQUE_H = 24
HUB_CLIQUE_SEEDS = (4, 7, 3)                              # colouring seeds hub_clique_seed() tries, in this order


def hub_clique_holds(ro, ci, hubs, colours, seed, seg=SEG):
    """what the hub clique exists for: its rows have at least three segments; some hub is still uncoloured at the start of round
    FIRST_BATCH + 1 (its row crossed the host's first wait); in some round >= 1 some row's below- and above-segments are disjoint;
    some row has a segment that sees both"""
    deg = np.diff(np.asarray(ro, dtype=np.int64))[hubs]
    disjoint, both = split_rows(ro, ci, colours, seed, hubs, seg)
    return bool((deg > 2 * seg).all() and uncoloured_at(colours, FIRST_BATCH + 1)[hubs].any() and disjoint and both)


def hub_clique_seed(ro, ci, hubs, seg=SEG, seeds=HUB_CLIQUE_SEEDS):
    """the first colouring seed of `seeds` under which the hub clique has its property -> (seed, model result); None: none has"""
    for seed in seeds:
        want = model.color(ro, ci, seed, 0)
        if hub_clique_holds(ro, ci, hubs, want[0], seed, seg):
            return seed, want
    return None
