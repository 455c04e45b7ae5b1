"""The bit-parallel multi-source BFS in numpy: the statement of the definition (include/mgx/msbfs_fused.hpp) that the
fused path, the operator path and the CPU suite are held against.  It works on the same 64-bit words per vertex, level by level,
and predicts the kind and e_t of every level and the rows per body; it computes every level as an OR over the in-entries of a
transposed copy it builds itself, whatever kind the level is (the kind changes no result)."""
import numpy as np

from tests import cc_model, row_bodies

SHORT_MAX, WAVE_MAX, SEG, PULL_DIV = 32, 1024, 1024, 8
PUSH, PULL = 0, 1
STAT_KEYS = ("sources", "batches", "deepest", "reach", "push_levels", "pull_levels", "csc", "depths")
BIN_KEYS = ("none", "short", "wave", "long", "segments")
U1 = np.uint64(1)


def bodies(lengths, short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG):
    """rows without entries, a lane's, a wave's, segmented rows, the segments of the latter"""
    return row_bodies.bodies(lengths, short_max, wave_max, seg)


def _bits_of(words):
    """uint64[k] -> bool[k, 64], bit b in column b"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").astype(bool)


def traverse(ro, ci, sources=None, symmetric=False, csc=False, short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG, pull_div=PULL_DIV,
             depths=True):
    """-> dict: depths int32[count, n] (None when not asked for), reach / far / ecc int64[count], harm float64[count], reach_in /
    far_in int64[n], kinds, e and long per (batch, level), stats (STAT_KEYS), bins_out / bins_in, launches.  csc: the graph has its
    genuine CSC.  long: the level's PUSH / PULL listed (vertex, segment) items, so a LONG launch follows it: a PUSH meets the
    out-rows of the front's vertices, a PULL the in-rows of every vertex that some source of the batch has not seen.  launches: K
    of the chain (tests/chain_model.py), by the kind rule of k_msbfs_step: RESET and SEED per batch, the PUSH / PULL, the LONG where
    there is one and the FINALIZE per level, and DONE."""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n, m = len(ro) - 1, len(ci)
    src = np.arange(n, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64)
    count = len(src)
    assert count == 0 or (src.min() >= 0 and src.max() < n)
    served = bool(csc) and not symmetric
    have_in = bool(symmetric) or served
    outdeg = np.diff(ro)
    co, ri = cc_model.transpose(ro.astype(np.int32), ci.astype(np.int32))
    co, ri = np.asarray(co, dtype=np.int64), np.asarray(ri, dtype=np.int64)
    has_in = np.diff(co) > 0
    long_out = row_bodies.classes(outdeg, short_max, wave_max) == row_bodies.LONG
    long_in = long_out if symmetric else row_bodies.classes(np.diff(co), short_max, wave_max) == row_bodies.LONG
    heads = co[:-1][has_in]
    depth = np.full((count, n), -1, dtype=np.int32) if depths else None
    reach, far, ecc = (np.zeros(count, dtype=np.int64) for _ in range(3))
    harm = np.zeros(count, dtype=np.float64)
    reach_in, far_in = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    kinds, es, longs, deepest = [], [], [], 0
    ran = n > 0 and count > 0
    batches = (count + 63) // 64 if ran else 0
    for B in range(batches):
        s = src[64 * B:64 * B + 64]
        seen = np.zeros(n, dtype=np.uint64)
        full = np.uint64((1 << len(s)) - 1)
        np.bitwise_or.at(seen, s, U1 << np.arange(len(s), dtype=np.uint64))
        front = seen.copy()
        if depths:
            depth[64 * B + np.arange(len(s)), s] = 0
        t = 0
        while front.any():
            e_t = int(outdeg[front != 0].sum())
            pull = have_in and pull_div > 0 and e_t * pull_div >= m
            kinds.append(PULL if pull else PUSH)
            es.append(e_t)
            longs.append(bool((long_in & ((~seen & full) != 0)).any() if pull else (long_out & (front != 0)).any()))
            nxt = np.zeros(n, dtype=np.uint64)
            if m:
                nxt[has_in] = np.bitwise_or.reduceat(front[ri], heads)
            new = nxt & ~seen
            seen |= new
            front = new
            t += 1
            idx = np.flatnonzero(new)
            if len(idx):
                bits = _bits_of(new[idx])
                pc = bits.sum(axis=1)
                reach_in[idx] += pc
                far_in[idx] += t * pc
                cnt = bits.sum(axis=0)[:len(s)].astype(np.int64)
                got = np.flatnonzero(cnt) + 64 * B
                c = cnt[cnt > 0]
                reach[got] += c
                far[got] += t * c
                ecc[got] = t
                harm[got] += c.astype(np.float64) / np.float64(t)          # ascending depth: the order the device adds in
                if depths:
                    rows, cols = np.nonzero(bits)
                    depth[64 * B + cols, idx[rows]] = t
        deepest = max(deepest, t)
    kinds = np.array(kinds, dtype=np.int32)
    stats = {"sources": count, "batches": batches, "deepest": deepest, "reach": int(reach.sum()), "push_levels": int((kinds == PUSH).sum()),
             "pull_levels": int((kinds == PULL).sum()), "csc": int(served), "depths": int(bool(depths))}
    zero = dict.fromkeys(BIN_KEYS, 0)
    return {"depths": depth, "reach": reach, "far": far, "ecc": ecc, "harm": harm, "reach_in": reach_in, "far_in": far_in,
            "kinds": kinds, "e": es, "long": longs, "stats": stats,
            "launches": 2 * batches + 2 * len(es) + sum(longs) + 1 if ran else 0,
            "bins_out": bodies(outdeg, short_max, wave_max, seg) if ran else dict(zero),
            "bins_in": bodies(outdeg if symmetric else np.diff(co), short_max, wave_max, seg) if ran and have_in else dict(zero)}


def path_from_its_end(n, short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG):
    """what traverse(path of n vertices, [0], symmetric) returns, in closed form, n > 9: vertex v is at depth v, so the run has n
    levels; a front has at most 2 out-entries of the 2 (n - 1), so every level is a PUSH (2 x PULL_DIV < m) and no row is long.
    tests/test_msbfs_cpu.py holds it against traverse on a short path; the GPU suite uses it where traverse would loop 65 536 times"""
    assert n > 1 + PULL_DIV
    v = np.arange(n, dtype=np.int64)
    outdeg = np.where((v == 0) | (v == n - 1), 1, 2)
    harm = np.add.accumulate(np.float64(1.0) / np.arange(1, n, dtype=np.float64))[-1:]       # (one after the other, ascending depth)
    stats = {"sources": 1, "batches": 1, "deepest": n, "reach": n - 1, "push_levels": n, "pull_levels": 0, "csc": 0, "depths": 1}
    bins = bodies(outdeg, short_max, wave_max, seg)
    return {"depths": v.astype(np.int32)[None, :], "reach": np.array([n - 1], dtype=np.int64), "far": np.array([n * (n - 1) // 2], dtype=np.int64),
            "ecc": np.array([n - 1], dtype=np.int64), "harm": harm, "reach_in": (v > 0).astype(np.int64), "far_in": v.copy(),
            "kinds": np.full(n, PUSH, dtype=np.int32), "e": [1] + [2] * (n - 2) + [1], "long": [False] * n, "stats": stats,
            "launches": 2 + 2 * n + 1, "bins_out": bins, "bins_in": dict(bins)}


def closeness(reach, far, n):
    """reach / far * reach / (n - 1) (Wasserman-Faust), 0 where far == 0"""
    reach, far = np.asarray(reach, dtype=np.float64), np.asarray(far, dtype=np.float64)
    out = np.zeros(len(reach), dtype=np.float64)
    ok = far > 0
    out[ok] = reach[ok] / far[ok] * (reach[ok] / (n - 1))
    return out
