"""The definition of the backward of the neighbour feature aggregation (mgx_aggbwd_*) in numpy.  Every step is one
float32 numpy operation, so the order of the arithmetic is the definition's by construction; the fold over a transposed row IS the
forward model's fold (tests/agg_model.py) over the transposed CSR.  The fused path (include/mgx/agg_backward.hpp) and the operator
path (include/gunrock/aggbwd/) give the same float32 bits.

  upstream  g[r, f] = GY[r, f]; for mean GY[r, f] / float32(d_r), one correctly rounded division, before the weight
  L_c       the selected rows' entries e with col_e == c, in ASCENDING e
  term      u_e = g[row_e, f], or w_e * g[row_e, f] rounded once; for max / min that when e == win[row_e, f], else +0.0
  win       the entry whose term the forward's fold kept: the first entry of a segment, then e exactly when t_e > acc (max) or
            t_e < acc (min); the segments' winners combined in segment order by the same test on the segments' values; -1 for a row
            without entries
  fold      segments of seg entries of L_c, acc = u_0 then acc = acc + u_j, the segments' values added in segment order; an empty
            L_c gives +0.0"""
import numpy as np

from tests import agg_model as fwd

STAT_KEYS = ("rows", "entries", "feats", "team_width", "col_tiles", "vector", "seg")       # what mgx_aggbwd_run knows without a wait
BIN_KEYS = fwd.BIN_KEYS
SORT_TILE = 2048                                                                            # segsort.hpp's SEGSORT_TILE


def transpose(ro, ci, x_rows, reverse=False):
    """-> (t_off int32[x_rows + 1], t_row int32[E], t_pos int32[E]) of the entries ro[0] .. ro[-1] - 1: t_pos are absolute places in
    ci, t_row counts from the first selected row.  reverse: every L_c in DESCENDING e (what the definition is not; the tests use it
    to show that the order is visible in the bits)"""
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    e = np.arange(ro[0], ro[-1])
    cols = ci[e]
    assert ((cols >= 0) & (cols < x_rows)).all()
    order = np.argsort(cols, kind="stable")
    t_pos = e[order]
    t_off = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=x_rows))])
    if reverse:
        for c in range(x_rows):
            t_pos[t_off[c]:t_off[c + 1]] = t_pos[t_off[c]:t_off[c + 1]][::-1]
    t_row = np.searchsorted(ro, t_pos, side="right") - 1
    return t_off.astype(np.int32), t_row.astype(np.int32), t_pos.astype(np.int32)


def take(op, acc, win, t, e):
    """the forward's max / min step with its winner: e takes over exactly where the comparison is true (never with a NaN t)"""
    better = (t > acc) if op == "max" else (t < acc)
    return np.where(better, t, acc), np.where(better, e, win)


def winners(ro, ci, x, op, weights=None, seg=fwd.SEG):
    """-> (win int32[R, F], y float32[R, F]): the forward model's fold with the winner beside the value"""
    assert op in ("max", "min")
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    x = np.asarray(x, dtype=np.float32)
    R, F = len(ro) - 1, x.shape[1]
    d = np.diff(ro)
    segs = -(-d // seg)
    first = np.concatenate([[0], np.cumsum(segs)])
    item_row = np.repeat(np.arange(R), segs)
    item_seg = np.arange(first[-1]) - first[item_row]
    item_beg = ro[item_row] + item_seg * seg
    item_len = np.minimum(seg, d[item_row] - item_seg * seg)
    part = np.zeros((len(item_row), F), dtype=np.float32)
    pwin = np.full((len(item_row), F), -1, dtype=np.int64)
    for j in range(int(item_len.max(initial=0))):
        act = np.flatnonzero(item_len > j)
        e = item_beg[act] + j
        t = x[ci[e]]
        if weights is not None:
            t = (np.asarray(weights, dtype=np.float32)[e][:, None] * t).astype(np.float32)
        ee = np.broadcast_to(e[:, None], t.shape)
        if j == 0:
            part[act], pwin[act] = t, ee
        else:
            part[act], pwin[act] = take(op, part[act], pwin[act], t, ee)
    y = np.zeros((R, F), dtype=np.float32)
    win = np.full((R, F), -1, dtype=np.int64)
    for s in range(int(segs.max(initial=0))):
        act = np.flatnonzero(segs > s)
        if s == 0:
            y[act], win[act] = part[first[act]], pwin[first[act]]
        else:
            y[act], win[act] = take(op, y[act], win[act], part[first[act] + s], pwin[first[act] + s])
    return win.astype(np.int32), y


def terms(ro, ci, gy, op, weights, x, seg, t_row, t_pos):
    """u float32[E, F] by slot"""
    gy = np.asarray(gy, dtype=np.float32)
    g = gy
    if op == "mean":
        d = np.diff(np.asarray(ro, dtype=np.int64))
        g = gy.copy()
        full = d > 0
        g[full] = (gy[full] / d[full].astype(np.float32)[:, None]).astype(np.float32)
    u = g[t_row]
    if weights is not None:
        u = (np.asarray(weights, dtype=np.float32)[t_pos][:, None] * u).astype(np.float32)
    win = None
    if op in ("max", "min"):
        win, _ = winners(ro, ci, x, op, weights, seg)
        u = np.where(win[t_row] == t_pos[:, None], u, np.float32(0.0)).astype(np.float32)
    return u, win


def sort_passes(longest):
    p, w = 0, SORT_TILE
    while w < longest:
        w, p = 2 * w, p + 1
    return p


def build_counts(entries, longest):
    """(launches, host_waits) of a transpose's build and its plan: count, scan, fill, the sort's classification and three bands (each
    counted as run) with its merge passes, the slots' rows, the plan's two; no sort below 2 entries, nothing without entries"""
    if entries == 0:
        return 0, 0
    if entries < 2:
        return 6, 1
    p = sort_passes(longest)
    return 10 + p + (p & 1), 2


def fused_counts(x_rows, long_t, builds, entries=0, longest=0, minmax=False, fwd_rows=0, fwd_long=0, builds_fplan=False, mean=False):
    """(launches, host_waits) of a fused run, every case of the header's table"""
    if x_rows == 0:
        return 0, 0
    launches, waits = (3 if long_t else 1), 0
    if mean and fwd_rows > 0:
        launches += 1
    if builds:
        b = build_counts(entries, longest)
        launches, waits = launches + b[0], waits + b[1]
    if minmax and fwd_rows > 0:
        launches += 3 if fwd_long else 1
        if builds_fplan:
            launches, waits = launches + 2, waits + 1
    return launches, waits


def backward(ro, ci, gy, op="sum", weights=None, seg=fwd.SEG, x=None, x_rows=None, vector=None, reverse=False):
    """ro int[R + 1] (absolute places in ci), gy float32[R, F], weights float32 by entry (absolute place) or None, x float32[x_rows, F]
    for max / min -> dict(gx float32[x_rows, F], t_off, t_row, t_pos, win, stats, bins, fwd_long, longest)"""
    assert op in fwd.OPS and seg == fwd.clamp_seg(seg)
    gy = np.asarray(gy, dtype=np.float32)
    if x_rows is None:
        x_rows = x.shape[0] if x is not None else int(np.asarray(ci).max(initial=-1)) + 1
    t_off, t_row, t_pos = transpose(ro, ci, x_rows, reverse)
    u, win = terms(ro, ci, gy, op, weights, x, seg, t_row, t_pos)
    F = gy.shape[1]
    folded = fwd.aggregate(t_off, np.arange(len(t_pos)), u.reshape(len(t_pos), F), "sum", None, seg=seg, vector=vector)
    d = np.diff(np.asarray(ro, dtype=np.int64))
    return dict(gx=folded["y"], t_off=t_off, t_row=t_row, t_pos=t_pos, win=win, stats={k: folded["stats"][k] for k in STAT_KEYS},
                bins=folded["bins"], fwd_long=int((d > seg).sum()), fwd_rows=len(d), longest=int(np.diff(t_off).max(initial=0)))
