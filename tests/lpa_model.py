"""The definition of label propagation and modularity in numpy: what mgx_lpa_run, mgx_lpa_enact and mgx_modularity
compute, bit for bit.

Votes.  Original ids.  symmetric != 0: every CSR entry (v, u), u != v, gives v one vote for lab[u].  symmetric == 0: every entry
(v, u), u != v, gives v one vote for lab[u] and u one vote for lab[v].  Self-loops never vote, duplicates vote once each.
Iteration.  lab_0[v] = v.  want_t[v] = lab_t[v] if v has no votes or its own label has the most; else the smallest label that has
the most.  unstable_t = #{want_t != lab_t}: 0 stops the run (converged, iterations = t), t == max_iter stops it as well.  Otherwise
lab_{t+1}[v] = want_t[v] where moves(v, t): always (SYNC), or color_key(v, color_salt(seed, t)) & 1 (LAZY).
Active set.  A_0 = the vertices with votes; A_{t+1} = the unstable vertices that did not move, and whoever a mover votes for
(symmetric: the targets of its entries; else those and the sources of its in-entries).  Outside A_t, want_t == lab_t."""
from fractions import Fraction

import numpy as np

from tests import coloring_model, row_bodies

SYNC, LAZY = 0, 1
SEED = coloring_model.SEED
STAT_KEYS = ("communities", "largest", "largest_label", "iterations", "converged", "unstable")
# the defaults of MGX_LPA_SHORT_MAX, MGX_LPA_WAVE_MAX, MGX_LPA_TABLE and MGX_LPA_LIST_DIV (include/mgx/lpa_fused.hpp)
SHORT_MAX, WAVE_MAX, TABLE, LIST_DIV = 16, 256, 2048, 8
# the kinds of the fused path's launches
SETUP, EVAL_DENSE, EVAL_LIST, LONG, APPLY_DENSE, APPLY_LIST, IDLE, MARK = range(1, 9)
APPLY_LANE_MAX = 32           # a mover's rows of more entries go out as items, for a MARK launch behind the APPLY


def votes(ro, ci, symmetric):
    """(receiver, sender) of every vote, int64"""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    cols = np.asarray(ci, dtype=np.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    if symmetric:
        return rows, cols
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


def row_entries(ro, ci, symmetric):
    """entries the kernels walk for every vertex, self-loops included: the out-row, and the in-row when not symmetric"""
    n = len(ro) - 1
    ln = np.diff(ro).astype(np.int64)
    if not symmetric:
        ln = ln + np.bincount(np.asarray(ci, dtype=np.int64), minlength=n)
    return ln


def label_stats(label):
    if len(label) == 0:
        return 0, 0, 0
    ids, sizes = np.unique(label, return_counts=True)
    return len(ids), int(sizes.max()), int(ids[np.argmax(sizes)])


def evaluate(n, rcv, snd, lab):
    """(want, distinct labels per vertex) under lab, for every vertex"""
    want = lab.copy()
    distinct = np.zeros(n, dtype=np.int64)
    if len(rcv) == 0:
        return want, distinct
    uk, cnt = np.unique(rcv * n + lab[snd], return_counts=True)
    rv, rl = uk // n, uk % n
    first = np.flatnonzero(np.diff(rv, prepend=-1))                # (rv ascending: the first pair of every receiver)
    most = np.maximum.reduceat(cnt, first)
    who = rv[first]
    distinct[who] = np.diff(np.append(first, len(rv)))
    m_of = np.zeros(n, dtype=np.int64)
    m_of[who] = most
    own = np.zeros(n, dtype=np.int64)                              # votes for the vertex's own label
    mine = rl == lab[rv]
    own[rv[mine]] = cnt[mine]
    top = cnt == m_of[rv]                                          # the pairs at the maximum, the smallest label of each receiver first
    tv, tl = rv[top], rl[top]
    head = np.flatnonzero(np.diff(tv, prepend=-1))
    smallest = np.zeros(n, dtype=np.int64)
    smallest[tv[head]] = tl[head]
    change = (m_of > 0) & (own != m_of)
    want[change] = smallest[change]
    return want, distinct


def is_dense(n_act, n, list_div):
    """whether an iteration whose active set has n_act vertices runs over all n (include/mgx/lpa_fused.hpp states the same)"""
    return not (list_div > 0 and n_act <= n // list_div)


def propagate(ro, ci, symmetric=False, mode=LAZY, seed=SEED, max_iter=100, active_only=False, short_max=SHORT_MAX,
              wave_max=WAVE_MAX, table=TABLE, list_div=LIST_DIV, check_active=False):
    """-> dict(labels int32, stats (STAT_KEYS), trace [(unstable, changed)], active [|A_t|], evaluated [rows the fused path
    evaluates in iteration t], kinds [the fused path's launches up to its end], overflowed).  active_only: want is computed for A_t alone (the claim: nothing changes)."""
    n = len(ro) - 1
    rcv, snd = votes(ro, ci, symmetric)
    ln = row_entries(ro, ci, symmetric)
    lab = np.arange(n, dtype=np.int64)
    has = np.zeros(n, dtype=bool)
    has[rcv] = True
    act = has.copy()
    trace, active, evaluated, kinds, overflowed = [], [], [], [SETUP], 0
    t = 0
    while True:
        want, distinct = evaluate(n, rcv, snd, lab)
        if check_active:
            assert (want[~act] == lab[~act]).all(), "a vertex outside A_%d wants to move" % t
        if active_only:
            want[~act] = lab[~act]
        n_act = int(act.sum())
        dense = is_dense(n_act, n, list_div)
        seen = np.ones(n, dtype=bool) if dense else act
        evaluated.append(n if dense else n_act)
        long_rows = seen & (row_bodies.classes(ln, short_max, wave_max) == row_bodies.LONG)
        overflowed += int((long_rows & (distinct > table)).sum())
        kinds.append(EVAL_DENSE if dense else EVAL_LIST)
        if long_rows.any():
            kinds.append(LONG)
        active.append(n_act)
        unst = want != lab
        unstable = int(unst.sum())
        if unstable == 0 or t == max_iter:
            trace.append((unstable, 0))
            break
        if mode == SYNC:
            moves = unst
        else:
            moves = unst & ((coloring_model.keys(n, coloring_model.salt(seed, t)) & 1) == 1)
        kinds.append(APPLY_DENSE if dense else APPLY_LIST)
        if (moves & (ln > APPLY_LANE_MAX)).any():
            kinds.append(MARK)
        trace.append((unstable, int(moves.sum())))
        act = unst & ~moves
        act[rcv[moves[snd]]] = True
        lab = np.where(moves, want, lab)
        t += 1
    kinds.append(IDLE)
    labels = lab.astype(np.int32)
    c, big, big_label = label_stats(labels)
    stats = dict(zip(STAT_KEYS, (c, big, big_label, t, int(trace[-1][0] == 0), trace[-1][0])))
    return {"labels": labels, "stats": stats, "trace": trace, "active": active, "evaluated": evaluated, "kinds": kinds,
            "overflowed": overflowed}


def is_equilibrium(ro, ci, symmetric, labels):
    """brute force, vertex by vertex: no label outvotes the one a vertex with votes holds"""
    n = len(ro) - 1
    rcv, snd = votes(ro, ci, symmetric)
    order = np.argsort(rcv, kind="stable")
    rcv, snd = rcv[order], snd[order]
    starts = np.searchsorted(rcv, np.arange(n + 1))
    for v in range(n):
        got = labels[snd[starts[v]:starts[v + 1]]]
        if len(got) == 0:
            continue
        ids, cnt = np.unique(got, return_counts=True)
        own = cnt[ids == labels[v]]
        if len(own) == 0 or own[0] != cnt.max():
            return False
    return True


def modularity(ro, ci, labels, symmetric=False):
    """(Q as a Fraction, S_in, S_sq, W) in Python integers"""
    n = len(ro) - 1
    labels = np.asarray(labels, dtype=np.int64)
    rcv, snd = votes(ro, ci, symmetric)
    w = int(len(rcv))
    s_in = int((labels[rcv] == labels[snd]).sum())
    tot = np.bincount(labels[rcv], minlength=max(n, 1)) if w else np.zeros(max(n, 1), dtype=np.int64)
    s_sq = sum(int(x) * int(x) for x in tot[tot > 0])
    q = Fraction(0) if w == 0 else Fraction(s_in, w) - Fraction(s_sq, w * w)
    return q, s_in, s_sq, w
