"""The definition of the neighbour sampling (mgx_nsample_*) in numpy: vectorised over a hop's rows, a loop over the
hops and, inside a hop, over the k draws of Floyd's algorithm.  The fused path (include/mgx/nsample_fused.hpp) and the operator path
(include/gunrock/nsample/) give the same six arrays, stats and bins, bit for bit.

  frontiers  V_0 is the ascending set of distinct seeds; every v of V_h is sampled once, at hop h; V_{h+1} is the ascending set of
             the sampled destinations that are in none of V_0 .. V_h.  A vertex's local id is its place in V_0 | V_1 | .. | V_H.
  a row      v at hop h, d entries, k = fanouts[h], key = step_key(walker_key(seed, v), h) of the random walks' draws
             (tests/rw_model.py), from the GLOBAL id.  d == 0: nothing.  k == -1, or not replace and d <= k: positions 0 .. d - 1 in
             stored order (a whole row).  replace: positions hi32(draw(key, j) * d), j = 0 .. k - 1.  Otherwise Floyd's algorithm:
             for j = 0 .. k - 1, i = d - k + j, t = hi32(draw(key, j) * (i + 1)), p_j = i if t is among p_0 .. p_{j-1} (a collision)
             else t; slot j of the row holds p_j (insertion order, no sort)."""
import numpy as np

from tests import row_bodies
from tests.rw_model import draw, index, step_key, walker_key

SHORT_MAX, WAVE_MAX, SEG = 32, 1024, 1024
MAX_HOPS, MAX_FANOUT = 16, 64
STAT_KEYS = ("seeds", "unique_seeds", "hops", "vertices", "rows", "edges", "empty_rows", "whole_rows", "sampled_rows", "draws", "collisions",
             "revisits")
BIN_KEYS = ("none", "short", "wave", "long", "segments")
ARRAYS = ("vertices", "hop_offsets", "row_offsets", "cols", "entry_pos", "seed_local")


def row_keys(seed, v, hop):
    return step_key(walker_key(seed, v), hop)


def floyd(key, d, k):
    """the positions Floyd's algorithm picks in rows of d > k entries -> (int64[rows, k] in insertion order, collisions per row)"""
    key, d = np.asarray(key, dtype=np.uint32), np.asarray(d, dtype=np.int64)
    picks = np.zeros((len(d), k), dtype=np.int64)
    collisions = np.zeros(len(d), dtype=np.int64)
    for j in range(k):
        i = d - k + j
        t = index(draw(key, j), i + 1)
        hit = (picks[:, :j] == t[:, None]).any(axis=1)
        picks[:, j] = np.where(hit, i, t)
        collisions += hit
    return picks, collisions


def with_replacement(key, d, k):
    key, d = np.asarray(key, dtype=np.uint32), np.asarray(d, dtype=np.int64)
    return np.stack([index(draw(key, j), d) for j in range(k)], axis=1) if len(d) else np.zeros((0, k), dtype=np.int64)


def fused_counts(n, seeds, hops, seeds_given):
    """(launches, host_waits) of a fused run: three launches number the seeds, five run a hop, one finishes; a wait for the seeds'
    upload and one for the totals' read-back"""
    if n == 0 or seeds == 0:
        return 0, 0
    return 5 * hops + 4, int(bool(seeds_given)) + 1


def bounds(n, m, seeds, fanouts, replace):
    """the capacities a run allocates: (F_h, E_h)"""
    F, E = [min(n, seeds)], []
    for k in fanouts:
        E.append(m if k < 0 else (F[-1] * k if replace else min(m, F[-1] * k)))
        F.append(min(n, E[-1]))
    return F, E


def sample(ro, ci, seeds=None, fanouts=(15, 10, 5), replace=False, seed=1, short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG):
    """-> dict(vertices, hop_offsets, row_offsets, cols, entry_pos, seed_local, stats, bins)"""
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n, H = len(ro) - 1, len(fanouts)
    deg = np.diff(ro)
    sd = np.arange(n, dtype=np.int64) if seeds is None else np.asarray(seeds, dtype=np.int64).reshape(-1)
    assert ((sd >= 0) & (sd < n)).all() and 0 <= H <= MAX_HOPS and all(k == -1 or 1 <= k <= MAX_FANOUT for k in fanouts)
    local = np.full(n, -1, dtype=np.int64)
    front = np.unique(sd)
    local[front] = np.arange(len(front))
    vertices, hop_offsets = [front], [0, len(front)]
    row_counts, positions = [], []
    c = dict.fromkeys(("empty_rows", "whole_rows", "sampled_rows", "draws", "collisions", "revisits"), 0)
    bins = dict.fromkeys(BIN_KEYS, 0)
    for h, k in enumerate(fanouts):
        d, beg = deg[front], ro[front]
        whole = (d > 0) & ((d <= k) | (k < 0) if not replace else np.full(len(d), k < 0))
        drawn = (d > 0) & ~whole
        cnt = np.where(whole, d, np.where(drawn, k, 0))
        off = np.concatenate([[0], np.cumsum(cnt)])
        pos = np.zeros(off[-1], dtype=np.int64)
        w = np.flatnonzero(whole)
        within = np.arange(cnt[w].sum()) - np.repeat(np.cumsum(cnt[w]) - cnt[w], cnt[w])
        pos[np.repeat(off[w], cnt[w]) + within] = np.repeat(beg[w], cnt[w]) + within
        s = np.flatnonzero(drawn)
        if len(s):
            key = row_keys(seed, front[s], h)
            if replace:
                picks = with_replacement(key, d[s], k)
            else:
                picks, coll = floyd(key, d[s], k)
                c["collisions"] += int(coll.sum())
            pos[off[s][:, None] + np.arange(k)[None, :]] = beg[s][:, None] + picks
        c["empty_rows"] += int((d == 0).sum())
        c["whole_rows"] += len(w)
        c["sampled_rows"] += len(s)
        c["draws"] += len(s) * max(k, 0)
        if k < 0:
            for key_, x in row_bodies.bodies(d, short_max, wave_max, seg).items():
                bins[key_] += x
        dst = ci[pos]
        c["revisits"] += int((local[dst] >= 0).sum())
        new = np.unique(dst[local[dst] < 0])
        local[new] = hop_offsets[-1] + np.arange(len(new))
        row_counts.append(cnt)
        positions.append(pos)
        vertices.append(new)
        hop_offsets.append(hop_offsets[-1] + len(new))
        front = new
    entry_pos = np.concatenate(positions) if positions else np.zeros(0, dtype=np.int64)
    counts = np.concatenate(row_counts) if row_counts else np.zeros(0, dtype=np.int64)
    out = {"vertices": np.concatenate(vertices).astype(np.int32), "hop_offsets": np.array(hop_offsets, dtype=np.int32),
           "row_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), "cols": local[ci[entry_pos]].astype(np.int32),
           "entry_pos": entry_pos.astype(np.int32), "seed_local": local[sd].astype(np.int32), "bins": bins}
    out["stats"] = dict(c, seeds=len(sd), unique_seeds=hop_offsets[1], hops=H, vertices=hop_offsets[-1], rows=hop_offsets[-2] if H else 0,
                        edges=len(entry_pos))
    if n == 0 or len(sd) == 0:
        out["hop_offsets"] = np.zeros(H + 2, dtype=np.int32)
    return out
