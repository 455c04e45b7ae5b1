"""The fused BFS's routing rules in Python (include/mgx/bfs_fused*.hpp), and a walk of a traversal's launches that predicts the
counters of mgx_bfs_run_stats from the per-level shapes of a tests/bfs_cases.py graph.

Every constant is read from the headers by regular expression; EXPECTED holds the values the cases were built for, and
tests/test_bfs_cases_cpu.py asserts them: a changed constant fails there instead of moving a case off its edge.

What the walk knows: a level is (nf_short, nf_long, E_short, E_long, units, kids) -- the two queues' sizes, the long rows' 64-entry
units, the discoveries, and the discoveries by queue (slot_marks: what the lazy rule's mark count comes to).  A launch is one of
  ("chain", )   k_bfs_chain_inplace      ("mini", )   k_bfs_mini      ("slot", )   k_bfs_push + the queue build
in the order bfs_fused_run enqueues them for a given number of device-wide slots in its first batch (what the handle has learnt:
bfs_class_slots) and a given tail_from.  predict() walks them for every such number and insists that the counters come out the same:
the cases are built so that the adaptive launch sequence decides nothing."""
import os
import re

import numpy as np

_INC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mgx")


def _read(name):
    with open(os.path.join(_INC, name)) as f:
        return f.read()


def _num(text, pattern):
    m = re.search(pattern, text)
    assert m, "not found in the header: " + pattern
    return int(m.group(1))


def constants():
    fused, chain, mini, run, rt = (_read(f) for f in ("bfs_fused.hpp", "bfs_fused_chain.hpp", "bfs_fused_mini.hpp", "bfs_fused_run.hpp", "runtime.hpp"))
    c = {
        "BFS_MAX_TRACE": _num(fused, r"constexpr int BFS_MAX_TRACE = (\d+);"),
        "BFS_COLD_WORDS": _num(fused, r"constexpr int BFS_COLD_WORDS = (\d+);"),
        "BFS_BUILD_NT": _num(fused, r"constexpr int BFS_BUILD_NT = (\d+);"),
        "BFS_BUILD_VPB": _num(fused, r"constexpr int BFS_BUILD_VPB = (\d+) \* BFS_BUILD_NT;"),
        "BFS_BUILD_LIST": _num(fused, r"constexpr int BFS_BUILD_LIST = (\d+) \* BFS_BUILD_NT;"),
        "BFS_CHAIN_CAP": _num(chain, r"constexpr int BFS_CHAIN_CAP = (\d+);"),
        "BFS_CHAIN_CAP_BIG": _num(chain, r"constexpr int BFS_CHAIN_CAP_BIG = (\d+);"),
        "BFS_CHAIN_EARLY_EDGES": _num(chain, r"constexpr u32 BFS_CHAIN_EARLY_EDGES = (\d+);"),
        "BFS_MINI_WGS": _num(mini, r"constexpr int BFS_MINI_WGS = (\d+);"),
        "BFS_MINI_LCAP": _num(mini, r"constexpr int BFS_MINI_LCAP = (\d+);"),
        "BFS_MINI_WCAP": _num(mini, r"constexpr int BFS_MINI_WCAP = (\d+);"),
        "BFS_MINI_EDGES_LATE": _num(mini, r"constexpr u32 BFS_MINI_EDGES_LATE = (\d+);"),
        "BFS_MINI_EDGES_EARLY": _num(mini, r"constexpr u32 BFS_MINI_EDGES_EARLY = (\d+);"),
        "BFS_MINI_SHORT_ROWS": _num(mini, r"constexpr u32 BFS_MINI_SHORT_ROWS = (\d+);"),
        "BFS_STREAM_HOTW2": _num(run, r"constexpr int BFS_STREAM_HOTW2 = (\d+);"),
        "BFS_WAVE_HOTW": _num(run, r"constexpr int BFS_WAVE_HOTW = (\d+);"),
        "BFS_DENSE_HOTW": _num(run, r"constexpr int BFS_STREAM_HOTW2 = (\d+);") - _num(run, r"constexpr int BFS_DENSE_HOTW = BFS_STREAM_HOTW2 - (\d+);"),
        "LONG_MIN_DEFAULT": _num(rt, r"constexpr int LONG_MIN_DEFAULT = (\d+);"),
        # the handle's defaults (bfs_fused_state_t)
        "chain_max_edges": _num(fused, r"unsigned chain_max_edges = (\d+);"),
        "chain_big_edges": _num(fused, r"unsigned chain_big_edges = (\d+);"),
        "vshort_div": _num(fused, r"unsigned vshort_div = (\d+);"),
        "dense_div": _num(fused, r"unsigned dense_div = (\d+);"),
        "lazy_div": _num(fused, r"unsigned lazy_div = (\d+);"),
        "slots_hint": _num(fused, r"int slots_hint = (\d+);"),
        "levels_per_sync": _num(fused, r"int levels_per_sync = (\d+);"),
        "hot_min_edges": _num(fused, r"unsigned hot_min_edges = (\d+);"),
    }
    c["BFS_BUILD_VPB"] *= c["BFS_BUILD_NT"]
    c["BFS_BUILD_LIST"] *= c["BFS_BUILD_NT"]
    return c


EXPECTED = {"BFS_MAX_TRACE": 4096, "BFS_COLD_WORDS": 20384, "BFS_BUILD_NT": 1024, "BFS_BUILD_VPB": 16384, "BFS_BUILD_LIST": 8192,
            "BFS_CHAIN_CAP": 6144, "BFS_CHAIN_CAP_BIG": 12288, "BFS_CHAIN_EARLY_EDGES": 1536, "BFS_MINI_WGS": 64, "BFS_MINI_LCAP": 4096,
            "BFS_MINI_WCAP": 8192, "BFS_MINI_EDGES_LATE": 131072, "BFS_MINI_EDGES_EARLY": 32768, "BFS_MINI_SHORT_ROWS": 65536,
            "BFS_STREAM_HOTW2": 20400, "BFS_WAVE_HOTW": 18000, "BFS_DENSE_HOTW": 20384, "LONG_MIN_DEFAULT": 32,
            "chain_max_edges": 4096, "chain_big_edges": 4096, "vshort_div": 8, "dense_div": 2, "lazy_div": 4, "slots_hint": 5,
            "levels_per_sync": 2, "hot_min_edges": 65536}
K = constants()


def _atoi(env, key, default):
    return int(env[key]) if key in env else default


class Config:
    """what bfs_fused_plan makes of the switches, the graph and its layout (single GPU, top-down unless mode == 1)"""

    def __init__(self, env, n, layout, ub_units=0, vs_edges=0, cold_pairs=0, mode=0, alpha=0.0):
        self.n, self.mode, self.alpha = int(n), int(mode), np.float32(alpha)
        lm = _atoi(env, "MGX_BFS_LONG_MIN", K["LONG_MIN_DEFAULT"])
        self.long_min = lm if lm > 0 else 0
        chain = _atoi(env, "MGX_BFS_CHAIN_MAX_EDGES", -1)
        do_chain = _atoi(env, "MGX_BFS_DO_CHAIN", 1)
        self.chain_max = 0 if (mode != 0 and not do_chain) else (min(chain, K["BFS_CHAIN_CAP"]) if chain >= 0 else K["chain_max_edges"])
        big = _atoi(env, "MGX_BFS_CHAIN_BIG_EDGES", -1)
        seed = _atoi(env, "MGX_BFS_SEED_CHAIN", 1)
        self.chain_big = (min(big, K["BFS_CHAIN_CAP_BIG"]) if big >= 0 else K["chain_big_edges"]) if (self.chain_max and seed) else 0
        self.hot_min_edges = _atoi(env, "MGX_BFS_HOT_MIN_EDGES", K["hot_min_edges"])
        self.tail_chain = _atoi(env, "MGX_BFS_TAIL_CHAIN", 1) != 0
        self.tail_front = _atoi(env, "MGX_BFS_TAIL_FRONT", 1) != 0
        mini = _atoi(env, "MGX_BFS_MINI", 1)
        merged = _atoi(env, "MGX_BFS_MERGED_PUSH", 1)
        self.minis = mode == 0 and mini != 0 and self.chain_big != 0 and merged != 0 and (n >= (1 << 22) or mini == 2)
        self.src_plan = bool(layout) and self.minis and _atoi(env, "MGX_BFS_SRC_PLAN", 1) != 0 and self.tail_chain
        build_list = _atoi(env, "MGX_BFS_BUILD_LIST", 0)
        # unit blocks, degree classes: the layout's, for the threshold it was built with (the cases set the switches before both)
        units = bool(layout) and self.long_min > 0 and ub_units > 0
        dense = _atoi(env, "MGX_BFS_DENSE", -1)
        packed = _atoi(env, "MGX_BFS_PACK24", 1) != 0 and n <= (1 << 23)
        self.dense_div = 0 if not units else (dense if dense >= 0 else (8 if packed else K["dense_div"]))
        self.ub_units = int(ub_units) if units else 0
        vs = bool(layout) and 0 < self.long_min <= 64 and vs_edges > 0
        vshort = _atoi(env, "MGX_BFS_VSHORT", -1)
        self.vs_div = 0 if not vs else (vshort if vshort >= 0 else K["vshort_div"])
        self.vs_edges = int(vs_edges) if vs else 0
        lazy = min(_atoi(env, "MGX_BFS_LAZY", -1), 1 << 20)
        self.lazy_div = (lazy if lazy >= 0 else K["lazy_div"]) if (self.dense_div and self.vs_div and not build_list) else 0
        self.lazy_pull = mode == 1 and not build_list and lazy != 0
        # cold-edge lists: built by the layout when vertices lie behind the unit-block body's LDS prefix and few of the long rows'
        # entries point there; used by a run with unit blocks, the direct queue build and MGX_BFS_COLD != 0
        hot_n = 32 * K["BFS_COLD_WORDS"]
        lists = units and n > hot_n and cold_pairs > 0 and cold_pairs * 4 <= ub_units * 64 and (n - hot_n + hot_n - 1) // hot_n <= 64
        self.cold = bool(lists and self.dense_div and not build_list and _atoi(env, "MGX_BFS_COLD", 1) != 0)


# ---- the device's rules ---------------------------------------------------------------------------------------------------------
def chain_edge_limit(cfg, reached, max_edges):
    late = reached * 4 >= cfg.n
    return max_edges if (late or max_edges < K["BFS_CHAIN_EARLY_EDGES"]) else K["BFS_CHAIN_EARLY_EDGES"]


def rule_pulls(cfg, reached, nf):
    unvisited = np.float32(cfg.n - reached)
    return bool(unvisited < np.float32(nf) * cfg.alpha)


def level_is_chained(cfg, lv, reached, pull, max_edges, list_cap):
    if max_edges == 0:
        return False
    nf, E = lv[0] + lv[1], lv[2] + lv[3]
    if cfg.mode == 1 and (pull or rule_pulls(cfg, reached, nf)):
        return False
    cap = min(chain_edge_limit(cfg, reached, max_edges), list_cap)
    return nf <= list_cap and E <= cap


def level_is_mini(cfg, lv, reached, lazy_here):
    if cfg.mode != 0 or lazy_here:
        return False
    late = reached * 4 >= cfg.n
    return lv[1] <= K["BFS_MINI_LCAP"] and lv[0] <= K["BFS_MINI_SHORT_ROWS"] and lv[2] + lv[3] <= (K["BFS_MINI_EDGES_LATE"] if late else K["BFS_MINI_EDGES_EARLY"])


def long_is_dense(cfg, lv, fb_here):
    return bool(cfg.ub_units and cfg.dense_div and fb_here and lv[4] * cfg.dense_div >= cfg.ub_units)


def short_is_dense(cfg, lv, fb_here):
    return bool(cfg.vs_div and fb_here and lv[2] * cfg.vs_div >= cfg.vs_edges)


def level_pulls(cfg, lv, reached, pull):
    if cfg.mode != 1:
        return False
    return pull or rule_pulls(cfg, reached, lv[0] + lv[1])


def slot_marks(cfg, lv, dense, vshort, tree):
    """(lo, hi) of the mark stores a device-wide slot's push counts (what bfs_build_is_lazy reads).  The unit-block and the
    vertex-by-vertex body test every entry against their LDS copy of the bitmap: an entry counts when it names an unvisited vertex
    -- exactly the level's discoveries on a tree level, at most every entry otherwise.  The two queue walks copy the prefix only from
    hot_min_edges entries on (the long rows': padded); below that they mark EVERY entry untested (no cold test on these graphs).
    Vertices behind the prefix are marked untested by all four: the cases' entries that lead there lead to unvisited vertices."""
    def part(hot, kids, entries):
        return (kids, kids if tree else entries) if hot else (entries, entries)
    long_lo, long_hi = part(dense or lv[4] * 64 >= cfg.hot_min_edges, lv[7], lv[3])
    short_lo, short_hi = part(vshort or lv[2] >= cfg.hot_min_edges, lv[6], lv[2])
    return long_lo + short_lo, long_hi + short_hi


def build_is_lazy(cfg, marks):
    return bool(cfg.lazy_div and marks * cfg.lazy_div >= cfg.n)


# ---- the host's launch sequence (bfs_fused_run), for `h` device-wide slots in the first batch ------------------------------------
def launches(cfg, h, tail_from, front_mini=True, batches=3000):
    slot = 0
    if cfg.chain_big:
        yield ("chain", slot)
    if cfg.minis and front_mini:
        yield ("mini", slot)
        slot = 1
    for b in range(batches):
        ns = h if b == 0 else K["levels_per_sync"] << min(b - 1, 4)
        ns = min(ns, 32)
        for _ in range(ns):
            if cfg.chain_big and slot > 0 and slot >= tail_from and cfg.tail_chain and cfg.tail_front and not cfg.minis:
                yield ("chain", slot)
            yield ("slot", slot)
            slot += 1
        if cfg.minis and b == 0:
            yield ("mini", slot)
            slot += 1
        if cfg.chain_big and (slot >= tail_from or cfg.minis) and cfg.tail_chain:
            yield ("chain", slot)
        yield ("look", slot)


COUNTERS = ("levels", "reached", "m_t", "frontier_vertices", "push_levels", "small_levels", "dense_slots", "vshort_slots", "lazy_slots",
            "cold_slots", "mini_slots", "pull_edges", "slots_found")


def walk(cfg, shapes, h, tail_from=1 << 30, front_mini=True, tree=True):
    """the counters a traversal over levels `shapes` leaves, and per level which body ran it: ("chain",) / ("chain_inplace",) /
    ("mini",) / ("slot", unit blocks by the rule, vertex by vertex by the rule, cold-edge pass, its build lazy, bottom-up, bottom-up by the
    rule alone).  tree: every entry that
    names an unvisited vertex is that vertex's only one (slot_marks)"""
    L = len(shapes)
    while L and shapes[L - 1][0] + shapes[L - 1][1] == 0:
        L -= 1
    c = dict.fromkeys(COUNTERS, 0)
    ran = []
    lv = 0                       # the level that stands in the slot the next launch works on
    reached, reached_mini, pull = 1, 0, False
    fb_here, lazy_here, done = True, False, False     # (frontier_bits holds this slot's frontier: the init seeds it with the source)

    def kids(k):
        return shapes[k][5]

    def run_chain(inplace, lim_e, cap):
        nonlocal lv, reached, fb_here, lazy_here, done
        first = True
        while True:
            s = shapes[lv]
            c["m_t"] += s[2] + s[3]
            c["frontier_vertices"] += s[0] + s[1]
            c["push_levels"] += 1
            c["small_levels"] += 1
            if first and not inplace:
                c["slots_found"] += 1
            first = False
            ran.append(("chain_inplace" if inplace else "chain",))
            reached += kids(lv)
            lv += 1
            if lv >= L:
                done = True
                c["levels"] = lv
                return
            nxt = shapes[lv]
            max_e = min(chain_edge_limit(cfg, reached, lim_e), cap)
            next_pulls = cfg.mode == 1 and rule_pulls(cfg, reached, nxt[0] + nxt[1])
            if nxt[2] + nxt[3] <= max_e and not next_pulls:
                continue
            fb_here = bool(next_pulls or (cfg.ub_units and cfg.dense_div and nxt[4] * cfg.dense_div >= cfg.ub_units))
            lazy_here = False
            return

    for kind, _slot in launches(cfg, h, tail_from, front_mini):
        if kind == "look":
            if done or lv >= L:
                if not done:
                    c["levels"] = lv
                break
            continue
        if done:
            continue
        if lv >= L:                       # an empty frontier
            if kind != "chain":
                done = True
                c["levels"] = lv
            continue
        s = shapes[lv]
        if kind == "chain":
            if lazy_here or not level_is_chained(cfg, s, reached, pull, cfg.chain_big, K["BFS_CHAIN_CAP_BIG"]):
                continue
            run_chain(True, cfg.chain_big, K["BFS_CHAIN_CAP_BIG"])
        elif kind == "mini":
            if not level_is_mini(cfg, s, reached, lazy_here):
                continue                  # forwarded as it is: the lazy and frontier-bitmap flags move with it
            c["m_t"] += s[2] + s[3]
            c["frontier_vertices"] += s[0] + s[1]
            c["push_levels"] += 1
            c["small_levels"] += 1
            c["mini_slots"] += 1
            c["slots_found"] += 1
            ran.append(("mini",))
            reached_mini += kids(lv)      # NOT in `reached`: the device's later `late` rules do not see an M launch's discoveries
            lv += 1
            fb_here, lazy_here = False, False
        else:
            chained = (not lazy_here) and level_is_chained(cfg, s, reached, pull, cfg.chain_max, K["BFS_CHAIN_CAP"])
            if chained:
                run_chain(False, cfg.chain_max, K["BFS_CHAIN_CAP"])
                continue
            pulls = level_pulls(cfg, s, reached, pull)
            rule_alone = cfg.mode == 1 and rule_pulls(cfg, reached, s[0] + s[1])      # (without what the levels before decided)
            dense = (not pulls) and long_is_dense(cfg, s, fb_here)
            vshort = (not pulls) and short_is_dense(cfg, s, fb_here)
            cold = dense and cfg.cold
            by_rule = (dense, vshort)
            if lazy_here and not pulls:
                dense = vshort = True     # (bfs_slot_plan: whatever the level's size)
            c["m_t"] += s[2] + s[3]
            c["frontier_vertices"] += s[0] + s[1]
            if pulls:
                pull = True
            else:
                c["push_levels"] += 1
            c["slots_found"] += 1
            c["dense_slots"] += int(dense)
            c["vshort_slots"] += int(vshort)
            c["cold_slots"] += int(cold)
            lo, hi = (0, 0) if pulls else slot_marks(cfg, s, dense, vshort, tree)      # (the bottom-up sweep counts no marks)
            if pulls:
                # every vertex still unvisited walks its in-edges up to the first frontier member: on a tree (one in-edge per vertex
                # below the source) that is one entry per vertex of the deeper levels
                assert tree
                c["pull_edges"] += sum(x[5] for x in shapes[lv:])
            lazy_lo, lazy_hi = build_is_lazy(cfg, lo), build_is_lazy(cfg, hi)
            assert lazy_lo == lazy_hi, "the case leaves the lazy rule to the number of duplicate marks"
            lazy = lazy_lo or (cfg.lazy_pull and pull)
            c["lazy_slots"] += int(lazy)
            ran.append(("slot", by_rule[0], by_rule[1], cold, bool(lazy), pulls, rule_alone))
            reached += kids(lv)
            lv += 1
            fb_here, lazy_here = True, bool(lazy)
    else:
        raise AssertionError("the traversal did not end")
    c["reached"] = reached + reached_mini
    return c, ran


def classify_source(cfg, shapes):
    """bfs_classify_source: 0 unknown, 1 the M launch in front absorbs the first level the chain leaves, 2 that launch is not enqueued"""
    if not cfg.src_plan or len(shapes) < 2:
        return 0
    deg = shapes[0][2] + shapes[0][3]
    s1, l1, e1 = shapes[1][0], shapes[1][1], shapes[1][2] + shapes[1][3]
    if deg == 0 or (1 + s1 + l1) * 4 >= cfg.n:
        return 0
    cap = min(min(cfg.chain_big, K["BFS_CHAIN_EARLY_EDGES"]), K["BFS_CHAIN_CAP_BIG"])
    if deg > cap:
        E, rs, rl = deg, shapes[0][0], shapes[0][1]
    elif e1 > cap:
        E, rs, rl = e1, s1, l1
    else:
        return 0
    mini = rl <= K["BFS_MINI_LCAP"] and rs <= K["BFS_MINI_SHORT_ROWS"] and E <= K["BFS_MINI_EDGES_EARLY"]
    return 1 if mini else 2


def outcomes(cfg, shapes, tree=True):
    """every (counters, bodies per level) a traversal can leave, over the launch sequences a handle may have learnt: 1 .. 8 slots in
    the first batch, chain launches in front of the last slots or not, both plans of a source's class"""
    fronts = [True] + ([False] if classify_source(cfg, shapes) == 2 else [])
    out = []
    for front in fronts:
        for h in (1, 2, 3, 5, 8):
            for tf in (h, 1 << 30):
                got = walk(cfg, shapes, h, tf, front, tree)
                if got not in out:
                    out.append(got)
    return out


def predict(cfg, shapes, tree=True):
    """the counters, the same for every launch sequence the handle may have learnt (asserted), and the bodies per level"""
    out = outcomes(cfg, shapes, tree)
    assert len(out) == 1, ("the launch sequence decides a counter", [o[0] for o in out])
    return out[0]


def trace(shapes):
    """level_trace(): (frontier vertices, entries) of every level that holds a queued row, up to the trace's capacity"""
    t = [(s[0] + s[1], s[2] + s[3]) for s in shapes if s[0] + s[1] > 0]
    return t[:K["BFS_MAX_TRACE"]]


def layout_numbers(deg, long_min):
    """what the layout's unit blocks and degree classes hold, from the degrees alone (the layout is a relabelling):
    ub_units = 64-entry units of the rows of at least long_min entries, vs_edges = entries of the shorter rows"""
    deg = np.asarray(deg, dtype=np.int64)
    if long_min <= 0:
        return 0, 0
    lng = deg >= long_min
    return int(((deg[lng] + 63) // 64).sum()), int(deg[~lng].sum())


def vs_classes(deg_layout, long_min):
    """cut_degree_classes on the layout's (descending) degrees: first row below long_min, 17, 5, 1 -- and below 9"""
    d = -np.asarray(deg_layout, dtype=np.int64)                 # ascending for searchsorted
    below = lambda k: int(np.searchsorted(d, -k, side="right"))
    b0 = below(long_min)
    b1 = max(b0, below(17))
    b2 = max(b1, below(5))
    b3 = max(b2, below(1))
    return (b0, b1, b2, b3), min(b2, max(b1, below(9)))


def config_for(env, g, layout, mode=0, alpha=0.0, **kw):
    """the model's view of a run of a tests/bfs_cases.py graph under switches `env`: the layout's numbers follow from the degrees.
    A direction-optimising run of a directed graph leaves the layout aside (it carries no CSC)."""
    lm = Config(env, g.n, False).long_min
    layout = bool(layout) and mode == 0
    ub, vs = layout_numbers(g.deg, lm) if layout else (0, 0)
    return Config(env, g.n, layout, ub_units=ub, vs_edges=vs, mode=mode, alpha=alpha, **kw)


def star_cold_pairs(g):
    """entries of the long rows that point behind the LDS prefix under the layout, for the stars: the hub names every other vertex
    and the layout puts it first, so every id from the prefix's end on is one of its entries"""
    return max(0, g.n - 32 * K["BFS_COLD_WORDS"])
