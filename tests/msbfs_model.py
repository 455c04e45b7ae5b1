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
    far_in int64[n], kinds and e per (batch, level), stats (STAT_KEYS), bins_out / bins_in.  csc: the graph has its genuine CSC."""
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
    heads = co[:-1][has_in]
    depth = np.full((count, n), -1, dtype=np.int32) if depths else None
    reach, far, ecc = (np.zeros(count, dtype=np.int64) for _ in range(3))
    harm = np.zeros(count, dtype=np.float64)
    reach_in, far_in = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    kinds, es, deepest = [], [], 0
    ran = n > 0 and count > 0
    batches = (count + 63) // 64 if ran else 0
    for B in range(batches):
        s = src[64 * B:64 * B + 64]
        seen = np.zeros(n, dtype=np.uint64)
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
            "kinds": kinds, "e": es, "stats": stats,
            "bins_out": bodies(outdeg, short_max, wave_max, seg) if ran else dict(zero),
            "bins_in": bodies(outdeg if symmetric else np.diff(co), short_max, wave_max, seg) if ran and have_in else dict(zero)}


def closeness(reach, far, n):
    """reach / far * reach / (n - 1) (Wasserman-Faust), 0 where far == 0"""
    reach, far = np.asarray(reach, dtype=np.float64), np.asarray(far, dtype=np.float64)
    out = np.zeros(len(reach), dtype=np.float64)
    ok = far > 0
    out[ok] = reach[ok] / far[ok] * (reach[ok] / (n - 1))
    return out
