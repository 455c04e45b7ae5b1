"""The definition of the neighbour feature aggregation (mgx_agg_*) in numpy: vectorised over the (row, segment) items
and the columns, a loop over the position inside a segment and one over a row's segments -- every step one float32 numpy operation,
so the order of the arithmetic is the definition's by construction.  The fused path (include/mgx/agg_fused.hpp) and the operator
path (include/gunrock/agg/) give the same float32 bits.

  Y[r, f] = (+) over the entries e of row r, in STORED order, of t_e = X[col_e, f], or w_e * X[col_e, f] rounded once to float32
  (the multiply and the add are never fused).
  order   a row's entries are cut into segments of `seg` entries.  Within a segment acc = t_0, then acc = acc (+) t_j, j = 1, 2, ..;
          the row's value is the segments' values combined the same way, in segment order.  (+) is float32 + for sum and mean,
          t > acc ? t : acc for max, t < acc ? t : acc for min.
  mean    the sum divided by float32(d), one correctly rounded division.  A row without entries gives 0.0 for every op."""
import numpy as np

from tests import row_bodies

SEG, SEG_MIN, SEG_MAX = 256, 64, 4096
UNROLL = 8                    # entries whose loads a team issues before the first add
TILE = 64                     # lane-columns a team walks at a time
MAX_FEATS = 65536
OPS = ("sum", "mean", "max", "min")
SOURCES = ("out", "in", "block")
STAT_KEYS = ("rows", "entries", "feats", "empty_rows", "team_rows", "long_rows", "segments", "team_width", "col_tiles", "vector", "seg")
RUN_KEYS = ("rows", "entries", "feats", "team_width", "col_tiles", "vector", "seg")      # what mgx_agg_run knows without a wait
BIN_KEYS = ("none", "team", "long", "segments")


def clamp_seg(value):
    """MGX_AGG_SEG as the library reads it: the smallest power of two in 64 .. 4096 that is >= value"""
    s = SEG_MIN
    while s < SEG_MAX and s < value:
        s *= 2
    return s


def is_vector(feats, ldx, ldy, x_addr=0, y_addr=0):
    """the vector path's gates: a lane owns 4 consecutive columns, one 16-byte load per entry"""
    return feats % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and x_addr % 16 == 0 and y_addr % 16 == 0


def shape(feats, vector):
    """-> (lane-columns C, team width G, column tiles)"""
    c = feats // 4 if vector else feats
    g = 1
    while g < min(c, TILE):
        g *= 2
    return c, g, -(-c // TILE)


def combine(op, acc, t):
    if op in ("sum", "mean"):
        return (acc + t).astype(np.float32)
    return np.where(t > acc, t, acc) if op == "max" else np.where(t < acc, t, acc)


def fused_counts(rows, long_rows, builds_plan):
    """(launches, host_waits) of a fused run: the rows' launch, and with long rows their items' and the fold; a run that builds a
    plan has two launches and one wait more; without rows nothing runs"""
    if rows == 0:
        return 0, 0
    return (3 if long_rows else 1) + (2 if builds_plan else 0), 1 if builds_plan else 0


def aggregate(ro, ci, x, op="sum", weights=None, seg=SEG, vector=None):
    """ro int[R + 1] (absolute places in ci: a hop's rows of a block start where the hop before ends), x float32[x_rows, F],
    weights float32[E] by entry or None -> dict(y float32[R, F], stats, bins).  vector: which path's shape the stats describe
    (None: contiguous arrays, by F alone)."""
    assert op in OPS and seg == clamp_seg(seg)
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    x = np.asarray(x, dtype=np.float32)
    R, F = len(ro) - 1, x.shape[1]
    d = np.diff(ro)
    segs = -(-d // seg)
    first = np.concatenate([[0], np.cumsum(segs)])                               # a row's first item
    item_row = np.repeat(np.arange(R), segs)
    item_seg = np.arange(first[-1]) - first[item_row]
    item_beg = ro[item_row] + item_seg * seg
    item_len = np.minimum(seg, d[item_row] - item_seg * seg)
    part = np.zeros((len(item_row), F), dtype=np.float32)
    for j in range(int(item_len.max(initial=0))):
        act = np.flatnonzero(item_len > j)
        e = item_beg[act] + j
        t = x[ci[e]]
        if weights is not None:
            t = (np.asarray(weights, dtype=np.float32)[e][:, None] * t).astype(np.float32)
        part[act] = t if j == 0 else combine(op, part[act], t)
    y = np.zeros((R, F), dtype=np.float32)
    for s in range(int(segs.max(initial=0))):
        act = np.flatnonzero(segs > s)
        y[act] = part[first[act]] if s == 0 else combine(op, y[act], part[first[act] + s])
    if op == "mean":
        full = d > 0
        y[full] = (y[full] / d[full].astype(np.float32)[:, None]).astype(np.float32)
    b = row_bodies.bodies(d, seg, seg, seg)
    bins = {"none": b["none"], "team": b["short"], "long": b["long"], "segments": b["segments"]}
    vec = (F % 4 == 0) if vector is None else bool(vector)
    c, g, tiles = shape(F, vec)
    stats = dict(rows=R, entries=int(d.sum()), feats=F, empty_rows=bins["none"], team_rows=bins["team"], long_rows=bins["long"],
                 segments=bins["segments"], team_width=g, col_tiles=tiles, vector=int(vec), seg=seg)
    return {"y": y, "stats": stats, "bins": bins}


def left_to_right(ro, ci, x, op="sum", weights=None):
    """the same without the segment tree: one plain left-to-right fold per row (what a row of at most seg entries is)"""
    return aggregate(ro, ci, x, op, weights, seg=SEG_MAX)["y"] if int(np.diff(ro).max(initial=0)) <= SEG_MAX else None
