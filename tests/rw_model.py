"""The definition of the random walks (mgx_rw_*) in numpy: vectorised over the walkers, a loop over the steps and,
inside a step, over the tries.  The fused path (include/mgx/rw_fused.hpp) and the operator path (include/gunrock/rw/) give the same
paths, ends, lengths, visits, stats and bins, bit for bit: every float is a float32 and every product a single multiply."""
import numpy as np

from tests import row_bodies

TRIES, TILE, SHORT_MAX, WAVE_MAX, SEG = 64, 16, 32, 1024, 1024
STAT_KEYS = ("walkers", "length", "steps", "dead_ends", "restarts", "tries", "fallbacks", "sorted_copy")
BIN_KEYS = ("none", "short", "wave", "long", "segments")
_F = np.float32


def fmix32(h):
    """murmur3's 32-bit finalizer (include/mgx/color_hash.hpp: color_fmix32) on a uint32 array"""
    h = np.array(h, dtype=np.uint32, copy=True, ndmin=1)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _mul(c, k):
    return np.uint32((c * (k + 1)) & 0xFFFFFFFF)


def walker_key(seed, w):
    w1 = (np.asarray(w, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B9) + np.uint64(seed & 0xFFFFFFFF)
    return fmix32((w1 & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def step_key(wkey, t):
    return fmix32(wkey ^ _mul(0x85EBCA6B, t))


def draw(skey, k):
    return fmix32(skey ^ _mul(0xC2B2AE35, k))


def draw_of(seed, w, t, k):
    """draw(seed, w, t, k) of the definition, for one walker"""
    return int(draw(step_key(walker_key(seed, [w]), t), k)[0])


def unit(r):
    """float(r >> 8) * 2^-24: exact, in [0, 1)"""
    return (r >> np.uint32(8)).astype(_F) * _F(2.0 ** -24)


def index(r, d):
    """the high word of r x d"""
    return ((r.astype(np.uint64) * np.asarray(d, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def row_maxima(ro, w):
    """(wmax[v], amax[v]): the maximum weight of every row (0 for a row without entries) and the smallest position that attains it"""
    ro = np.asarray(ro, dtype=np.int64)
    n, deg = len(ro) - 1, np.diff(ro)
    w = np.where(w == 0, _F(0), np.asarray(w, dtype=_F)).astype(_F)              # (-0.0 counts as 0.0)
    wmax, amax = np.zeros(n, dtype=_F), np.zeros(n, dtype=np.int64)
    rows = np.flatnonzero(deg > 0)
    if len(rows):
        wmax[rows] = np.maximum.reduceat(w, ro[rows])
        pos = np.arange(len(w)) - np.repeat(ro[:-1], deg)
        amax[rows] = np.minimum.reduceat(np.where(w == np.repeat(wmax, deg), pos, len(w)), ro[rows])
    return wmax, amax


def rows_ascend(ro, ci):
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    if len(ci) < 2:
        return True
    down = ci[:-1] > ci[1:]
    down[ro[1:-1][(ro[1:-1] > 0) & (ro[1:-1] < len(ci))] - 1] = False              # (a row's last entry and the next row's first)
    return not down.any()


def row_bins(ro, short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG):
    """the rows per body of a setup launch"""
    return row_bodies.bodies(np.diff(np.asarray(ro, dtype=np.int64)), short_max, wave_max, seg)


def fused_counts(walkers, n, starts_given, setup, sort):
    """(launches, host_waits) of a fused run: two launches and a wait for a setup, a launch and two waits for the sorted copy's
    sort, the walk and the counters' read-back, a wait for the starts' upload"""
    if walkers == 0 or n == 0:
        return 0, 0
    return 2 * int(setup) + int(sort) + 1, int(bool(starts_given)) + int(setup) + 2 * int(sort) + 1


def walk(ro, ci, w=None, starts=None, length=80, walks_per_start=1, seed=1, weighted=False, p=1.0, q=1.0, restart=0.0, tries=TRIES,
         short_max=SHORT_MAX, wave_max=WAVE_MAX, seg=SEG):
    """-> dict(paths, ends, lengths, visits, stats, bins).  w: the entries' float32 weights (None: all 1.0)."""
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n, L, R = len(ro) - 1, int(length), int(walks_per_start)
    deg = np.diff(ro)
    wt_all = np.ones(len(ci), dtype=_F) if w is None else np.asarray(w, dtype=_F)
    st = np.arange(n, dtype=np.int64) if starts is None else np.asarray(starts, dtype=np.int64)
    assert ((st >= 0) & (st < n)).all() and L >= 0 and R >= 1 and p > 0 and q > 0 and 0 <= restart < 1
    W = len(st) * R
    start = np.repeat(st, R)
    ip, iq, r32 = _F(1) / _F(p), _F(1) / _F(q), _F(restart)
    big = max(ip, _F(1), iq)
    second_run = not (_F(p) == 1 and _F(q) == 1)
    if weighted:
        if not (wt_all >= 0).all():
            raise ValueError("negative or NaN weight")
        wmax, amax = row_maxima(ro, wt_all)
    else:
        wmax, amax = np.ones(n, dtype=_F), np.zeros(n, dtype=np.int64)
    sorted_copy = bool(second_run and not rows_ascend(ro, ci))
    entries = np.sort(np.repeat(np.arange(n, dtype=np.int64), deg) * max(n, 1) + ci)      # the membership search's answer

    paths = np.full((W, L + 1), -1, dtype=np.int32)
    paths[:, 0] = start
    cur, prev = start.copy(), np.full(W, -1, dtype=np.int64)
    alive = np.ones(W, dtype=bool)
    wkey = walker_key(seed, np.arange(W))
    c = dict(dead_ends=0, restarts=0, tries=0, fallbacks=0)
    with np.errstate(all="ignore"):
        for t in range(L if n else 0):
            ids = np.flatnonzero(alive)
            if not len(ids):
                break
            key = step_key(wkey[ids], t)
            v = cur[ids]
            jump = unit(draw(key, 0)) < r32 if restart > 0 else np.zeros(len(ids), dtype=bool)
            dead = ~jump & ((deg[v] == 0) | (bool(weighted) & ~(wmax[v] > 0)))
            if restart > 0:
                jump, dead = jump | dead, np.zeros(len(ids), dtype=bool)
            c["dead_ends"] += int(dead.sum())
            c["restarts"] += int(jump.sum())
            alive[ids[dead]] = False
            nxt = np.full(len(ids), -1, dtype=np.int64)
            nxt[jump] = start[ids[jump]]
            prev[ids[jump]] = -1
            ch = np.flatnonzero(~jump & ~dead)                                   # the walkers that choose an entry
            if len(ch):
                kc, vc, dc, bc = key[ch], v[ch], deg[v[ch]], ro[v[ch]]
                if not weighted and not second_run:
                    pick = ci[bc + index(draw(kc, 1), dc)]
                    c["tries"] += len(ch)
                else:
                    pv = prev[ids[ch]]
                    second = second_run & (pv >= 0)
                    limit = (wmax[vc] * np.where(second, big, _F(1)).astype(_F)).astype(_F)
                    pick = np.full(len(ch), -1, dtype=np.int64)
                    pend = np.arange(len(ch))
                    for i in range(tries):
                        j = index(draw(kc[pend], 1 + 2 * i), dc[pend])
                        cand = ci[bc[pend] + j]
                        wj = wt_all[bc[pend] + j] if weighted else np.ones(len(pend), dtype=_F)
                        a = unit(draw(kc[pend], 2 + 2 * i))
                        q_ = pv[pend] * max(n, 1) + cand
                        at = np.minimum(np.searchsorted(entries, q_), max(len(entries) - 1, 0))
                        member = (entries[at] == q_) if len(entries) else np.zeros(len(pend), dtype=bool)
                        b = np.where(second[pend], np.where(cand == pv[pend], ip, np.where(member, _F(1), iq)), _F(1)).astype(_F)
                        ok = (a * limit[pend]).astype(_F) < (wj * b).astype(_F)
                        c["tries"] += len(pend)
                        pick[pend[ok]] = cand[ok]
                        pend = pend[~ok]
                        if not len(pend):
                            break
                    c["fallbacks"] += len(pend)
                    pick[pend] = ci[bc[pend] + amax[vc[pend]]]
                nxt[ch] = pick
                prev[ids[ch]] = vc
            go = nxt >= 0
            cur[ids[go]] = nxt[go]
            paths[ids[go], t + 1] = nxt[go]
    lengths = (paths[:, 1:] >= 0).sum(axis=1).astype(np.int32)
    visits = np.bincount(paths[paths >= 0].astype(np.int64), minlength=n).astype(np.int64)
    stats = {"walkers": W, "length": L, "steps": int(lengths.sum()), "dead_ends": c["dead_ends"], "restarts": c["restarts"],
             "tries": c["tries"], "fallbacks": c["fallbacks"], "sorted_copy": int(sorted_copy)}
    if n == 0 or W == 0:
        stats["sorted_copy"] = 0
    return {"paths": paths, "ends": cur.astype(np.int32), "lengths": lengths, "visits": visits, "stats": stats,
            "bins": row_bins(ro, short_max, wave_max, seg), "setup": bool(weighted or second_run), "second": second_run}
