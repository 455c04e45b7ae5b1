"""Graphs for the fused BFS whose levels are exactly what a case says (numpy only; tests/test_bfs_cases_cpu.py proves it, and
tests/test_gpu_bfs_paths.py runs them).

A graph is given level by level: level k is a list of row groups `rows(count, deg, kids, fill)` -- `count` frontier rows of `deg`
entries each, the LAST `kids` of which lead to `kids` vertices of level k + 1 that no other entry names (tree entries: every vertex
of level k + 1 has exactly one in-edge, so marks stored == claims == discoveries == tree entries, whatever order the device works
in).  The other deg - kids entries are FILLER:
  "visited"    the source -- visited whatever the level; they set a level's entry count without touching the next level's size
  "contested"  by position: a duplicate of the row's own first child, the row itself (a self-loop), the first child of the NEXT row
               of the level -- several rows name one vertex of level k + 1, twice within a row: the claim has losers.  The labels
               do not change: the named vertices are children of the level anyway.
Level k + 1 must hold exactly as many rows as level k has kids; they are dealt in order.  deg == 0 rows are frontier vertices that
are labelled but never queued.  `pad` isolated vertices set n freely.  Ids: "spec" -- the source is 0, then level by level, the
padding last -- or a seeded permutation of that.
The labels come from the construction alone (level k's rows get label k); no search runs here."""
import numpy as np


def rows(count, deg, kids=0, fill="visited"):
    assert 0 <= kids <= deg and count >= 0 and fill in ("visited", "contested")
    return (int(count), int(deg), int(kids), fill)


class Layered:
    def __init__(self, levels, pad=0, ids="spec"):
        assert len(levels[0]) == 1 and levels[0][0][0] == 1, "level 0 is the source's row"
        self.level_rows = []                    # per level: (deg[], kids[], contested[]) of its rows, in spec order
        for lv in levels:
            deg = np.concatenate([np.full(c, d, dtype=np.int64) for c, d, _, _ in lv])
            kid = np.concatenate([np.full(c, k, dtype=np.int64) for c, _, k, _ in lv])
            con = np.concatenate([np.full(c, f == "contested", dtype=bool) for c, _, _, f in lv])
            self.level_rows.append((deg, kid, con))
        for k in range(len(levels) - 1):
            assert int(self.level_rows[k][1].sum()) == len(self.level_rows[k + 1][0]), ("level %d's kids are level %d's rows" % (k, k + 1))
        assert int(self.level_rows[-1][1].sum()) == 0, "the last level has no kids"
        sizes = [len(d) for d, _, _ in self.level_rows]
        base = np.concatenate([[0], np.cumsum(sizes)])
        self.reachable = int(base[-1])
        self.n = self.reachable + int(pad)
        self.src_spec = 0
        deg_all = np.zeros(self.n, dtype=np.int64)
        cols = []
        for k, (deg, kid, con) in enumerate(self.level_rows):
            R = len(deg)
            deg_all[base[k]:base[k] + R] = deg
            T = int(deg.sum())
            if T == 0:
                continue
            row = np.repeat(np.arange(R), deg)
            pos = np.arange(T) - np.repeat(np.cumsum(deg) - deg, deg)
            first_kid = base[k + 1] + np.cumsum(kid) - kid if k + 1 < len(self.level_rows) else np.zeros(R, dtype=np.int64)
            is_kid = pos >= (deg - kid)[row]
            kid_id = first_kid[row] + (pos - (deg - kid)[row])
            fill = np.zeros(T, dtype=np.int64)                   # the source
            if con.any():
                has = np.flatnonzero(kid > 0)
                if len(has):
                    # the first row at or behind r that has a kid (cyclic), and the one behind that
                    nxt = has[np.searchsorted(has, np.arange(R)) % len(has)]
                    nxt2 = has[(np.searchsorted(has, np.arange(R)) + 1) % len(has)]
                    own = first_kid[nxt]
                    other = first_kid[nxt2]
                    me = base[k] + np.arange(R)
                    pick = np.stack([own, me, other])            # by position mod 3
                    cf = pick[pos % 3, row]
                    fill = np.where(con[row], cf, fill)
            cols.append(np.where(is_kid, kid_id, fill))
        ci = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
        ro = np.concatenate([[0], np.cumsum(deg_all)])
        labels = np.full(self.n, -1, dtype=np.int32)
        for k in range(len(sizes)):
            labels[base[k]:base[k + 1]] = k
        if ids == "spec":
            self.new_of_spec = np.arange(self.n, dtype=np.int64)
        else:
            self.new_of_spec = np.random.default_rng(int(ids)).permutation(self.n).astype(np.int64)
        p = self.new_of_spec
        spec_of_new = np.empty(self.n, dtype=np.int64)
        spec_of_new[p] = np.arange(self.n)
        deg_new = deg_all[spec_of_new]
        self.ro = np.concatenate([[0], np.cumsum(deg_new)]).astype(np.int32)
        # row of new id v = the spec row spec_of_new[v], its entries renamed
        start = ro[spec_of_new]
        T = int(deg_new.sum())
        idx = np.repeat(start, deg_new) + (np.arange(T) - np.repeat(self.ro[:-1].astype(np.int64), deg_new))
        self.ci = p[ci[idx]].astype(np.int32) if T else np.zeros(0, dtype=np.int32)
        self.labels = np.empty(self.n, dtype=np.int32)
        self.labels[p] = labels
        self.src = int(p[0])
        self.deg = deg_new
        self.tree = not any(con.any() for _, _, con in self.level_rows)

    def shapes(self, long_min):
        """per level (nf_short, nf_long, E_short, E_long, long-row units, kids, kids of the short rows, kids of the long rows): what
        the device's queues of the level hold -- rows without entries are not queued; long_min <= 0: no long-row queue"""
        out = []
        for deg, kid, _ in self.level_rows:
            q, qk = deg[deg > 0], kid[deg > 0]
            lng = q >= long_min if long_min > 0 else np.zeros(len(q), dtype=bool)
            out.append((int((~lng).sum()), int(lng.sum()), int(q[~lng].sum()), int(q[lng].sum()), int(((q[lng] + 63) // 64).sum()),
                        int(kid.sum()), int(qk[~lng].sum()), int(qk[lng].sum())))
        return out

    def in_neighbour_ok(self):
        """every reached vertex but the source has an in-neighbour one level up (the labels are a BFS's), and no entry skips a level"""
        u = np.repeat(np.arange(self.n), self.deg)
        lu, lv = self.labels[u], self.labels[self.ci]
        if np.any(lu < 0) and np.any(lv[lu < 0] >= 0):
            return False
        if np.any((lu >= 0) & ((lv < 0) | (lv > lu + 1))):
            return False
        has_parent = np.zeros(self.n, dtype=bool)
        has_parent[self.ci[(lu >= 0) & (lv == lu + 1)]] = True
        need = self.labels > 0
        return bool(np.all(has_parent[need]))


def numpy_bfs(ro, ci, src):
    """the ten-line reference: frontier by frontier over the CSR"""
    n = len(ro) - 1
    lab = np.full(n, -1, dtype=np.int32)
    lab[src] = 0
    front = np.array([src])
    k = 0
    while len(front):
        deg = (ro[front + 1] - ro[front]).astype(np.int64)
        idx = np.repeat(ro[front].astype(np.int64), deg) + (np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg))
        nb = np.unique(ci[idx])
        front = nb[lab[nb] < 0]
        k += 1
        lab[front] = k
    return lab


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# name -> dict(env, graph (a function: member -> Layered), members, pair (the level and the counter the members differ in -- by one, or
#              by a third entry: a bottom-up switch holds for the levels behind it too --, or None),
#              layouts (which of False / True the case runs with), doc)
SC0 = {"MGX_BFS_SEED_CHAIN": "0"}                                   # the chain runs inside block 0 of a push launch; no M launches
WIDE = {"MGX_BFS_SEED_CHAIN": "0", "MGX_BFS_CHAIN_MAX_EDGES": "0"}  # every level is a device-wide slot
RULES = {"MGX_BFS_DENSE": "2", "MGX_BFS_VSHORT": "8", "MGX_BFS_LAZY": "4"}   # the three divisors, said out loud
NOLAZY = {"MGX_BFS_DENSE": "2", "MGX_BFS_VSHORT": "8", "MGX_BFS_LAZY": "0"}
HOT_N = 32 * 20384                                                  # vertices of the unit-block body's LDS prefix (asserted by the model)

CASES = {}


def case(name, env, members, graph, pair=None, layouts=(False, True), ids=("spec", 7), doc="", mode=0, alpha=0.0, adaptive=False):
    # adaptive: the handle's learnt launch sequence decides a counter (bfs_model.outcomes lists what a run may report)
    CASES[name] = dict(env=dict(env), members=tuple(members), graph=graph, pair=pair, layouts=tuple(layouts), ids=tuple(ids), doc=doc,
                       mode=mode, alpha=alpha, adaptive=adaptive)


def _two_level(fan, deg, kids_each, extra_deg, pad=0):
    """source -> `fan` rows of `deg` entries (kids_each tree entries each); extra_deg: the first row's length instead"""
    def g(member, ids):
        d0 = deg if member == "at" else extra_deg
        k0 = min(kids_each + (d0 - deg), d0) if kids_each == deg else kids_each
        lv1 = [rows(1, d0, k0), rows(fan - 1, deg, kids_each)]
        nk = k0 + (fan - 1) * kids_each
        return Layered([[rows(1, fan, fan)], lv1, [rows(nk, 0)]], pad=pad, ids=ids)
    return g


# -- chain inside a push launch ---------------------------------------------------------------------------------------------------
case("chain_early", SC0, ("at", "beyond"), _two_level(48, 32, 1, 33, pad=400), pair=(1, "small_levels"),
     doc="level 1 holds 1536 / 1537 entries with reached * 4 < n: BFS_CHAIN_EARLY_EDGES.  Level 0 is chained in both.")
case("chain_late", SC0, ("at", "beyond"), _two_level(64, 64, 1, 65), pair=(1, "small_levels"),
     doc="4096 / 4097 entries with reached * 4 >= n (65 of 129 vertices): chain_max_edges' default")
case("chain_cap", dict(SC0, MGX_BFS_CHAIN_MAX_EDGES="6144"), ("at", "beyond"), _two_level(64, 96, 1, 97), pair=(1, "small_levels"),
     doc="6144 / 6145 entries, late, MGX_BFS_CHAIN_MAX_EDGES=6144: BFS_CHAIN_CAP itself")


def _late_rule(member, ids):
    # 51 vertices reached when level 1 (2000 entries: between the early and the late limit) is looked at: n = 204 is late, 205 is not
    return Layered([[rows(1, 50, 50)], [rows(50, 40, 1)], [rows(50, 0)]], pad=(204 if member == "at" else 205) - 101, ids=ids)


case("chain_late_rule", SC0, ("at", "beyond"), _late_rule, pair=(1, "small_levels"),
     doc="reached * 4 == n / == n - 1 (isolated vertices set n): the `late` rule of bfs_chain_edge_limit")


def _full_list(member, ids):
    # level 0 (2048 entries, early) is a device-wide slot; level 1: 2048 rows x 3 tree entries = 6144 entries that ALL win (the
    # winners' list full), late: 2049 * 4 = 8196 >= n = 8193; level 2: 6144 rows of one entry -- nf == E == BFS_CHAIN_CAP -- or one
    # row of two.  nf = CAP + 1 with E <= CAP cannot be built: a queued row has at least one entry.
    l2 = [rows(6144, 1)] if member == "at" else [rows(1, 2), rows(6143, 1)]
    return Layered([[rows(1, 2048, 2048)], [rows(2048, 3, 3)], l2], ids=ids)


case("chain_full_list", dict(SC0, MGX_BFS_CHAIN_MAX_EDGES="6144"), ("at", "beyond"), _full_list, pair=(2, "small_levels"),
     doc="a tree level whose 6144 entries all win, then 6144 rows of one entry (at) / 6145 entries in 6144 rows (beyond)")
case("chain_three_then_not", SC0, ("at",),
     lambda member, ids: Layered([[rows(1, 4, 4)], [rows(4, 4, 4)], [rows(16, 4, 4)], [rows(64, 32, 32)], [rows(2048, 0)]], ids=ids),
     doc="three chained levels in a row, then 2048 entries before a quarter is reached: the chain stages the level out")

def _entry(member, ids):
    k = 1536 if member == "at" else 1537
    return Layered([[rows(1, k, k)], [rows(k, 0)]], pad=7, ids=ids)


# (the cases above reach their level from a chained level 0: the chain's own "keep going" test decides there.  These two put the edge
#  on the FIRST level a launch looks at, which bfs_level_is_chained itself decides -- as chain_full_list does at BFS_CHAIN_CAP)
case("chain_entry_early", SC0, ("at", "beyond"), _entry, pair=(0, "small_levels"),
     doc="the source's row holds 1536 / 1537 entries: the push launch's own look at level 0")
case("inplace_entry_early", {}, ("at", "beyond"), _entry, pair=(0, "small_levels"),
     doc="the same for the in-place chain launch behind the init")

# -- in-place chain launch --------------------------------------------------------------------------------------------------------
for _nm, _env in (("inplace_default", {}), ("inplace_no_tail", {"MGX_BFS_TAIL_CHAIN": "0"}), ("inplace_no_front", {"MGX_BFS_TAIL_FRONT": "0"})):
    case(_nm, _env, ("at", "beyond"), _two_level(64, 64, 1, 65), pair=(1, "small_levels"),
         doc="4096 / 4097 entries, late: chain_big_edges' default.  The first launch behind the init takes levels 0 and 1 on every run.")
case("inplace_cap", {"MGX_BFS_CHAIN_BIG_EDGES": "12288"}, ("at", "beyond"), _two_level(64, 192, 1, 193), pair=(1, "small_levels"),
     doc="12288 / 12289 entries, late: BFS_CHAIN_CAP_BIG")

# -- M launch (MGX_BFS_MINI=2).  Only the launch in FRONT of the slots meets its level on every run: it works on whatever the
#    in-place chain leaves in slot 0.  The launch behind the slots meets a level or not by how many slots the handle has learnt to
#    enqueue: the cases stand in front, but for mini_short_rows, which cannot and is marked adaptive.
MINI = {"MGX_BFS_MINI": "2"}


def _mini_lcap(member, ids):
    # 1 -> 1400 -> 4096 / 4097 rows of 16 filler entries (long at MGX_BFS_LONG_MIN=16).  Level 1 (4096 / 4097 tree entries) is late
    # (1401 * 4 >= n = 5497 / 5498) and chained in place at MGX_BFS_CHAIN_BIG_EDGES=12288 in both members.
    a, b = (1296, 104) if member == "at" else (1297, 103)
    return Layered([[rows(1, 1400, 1400)], [rows(a, 3, 3), rows(b, 2, 2)], [rows(3 * a + 2 * b, 16)]], ids=ids)


case("mini_lcap", dict(MINI, MGX_BFS_LONG_MIN="16", MGX_BFS_CHAIN_BIG_EDGES="12288"), ("at", "beyond"), _mini_lcap, pair=(2, "mini_slots"),
     doc="4096 / 4097 long rows: BFS_MINI_LCAP")
case("mini_early", MINI, ("at", "beyond"), _two_level(1024, 32, 32, 33), pair=(1, "mini_slots"),
     doc="32768 / 32769 entries, all discoveries, 1025 of 33793 vertices reached: BFS_MINI_EDGES_EARLY")
case("mini_late", MINI, ("at", "beyond"), _two_level(1024, 128, 1, 129), pair=(1, "mini_slots"),
     doc="131072 / 131073 entries, 1025 of 2049 vertices reached: BFS_MINI_EDGES_LATE")
case("mini_behind_lazy", dict(MINI, **RULES), ("at",),
     lambda member, ids: Layered([[rows(1, 40000, 40000)], [rows(40000, 1)]], pad=79999, ids=ids), layouts=(True,),
     doc="level 0 stores 40000 marks of n = 160000: its build is lazy, and level 1 (40000 entries, late: mid-size by its numbers) is "
         "never an M launch's -- whether it meets one (and is forwarded) or a slot, by what the handle has learnt: the counters "
         "are the same")
def _mini_short_rows(member, ids):
    # level 0 (2048 entries, early: not chained) is the M launch's in front of the slots; level 1 (2048 long rows, 65536 / 65537 tree
    # entries, early) is a device-wide slot's; level 2 holds 65536 / 65537 short rows of one filler entry, late by the device's count
    # (65537 of 67585: an M launch's discoveries are not in `reached`) and mid-size by its entries
    l1 = [rows(2048, 32, 32)] if member == "at" else [rows(1, 33, 33), rows(2047, 32, 32)]
    k = 65536 if member == "at" else 65537
    return Layered([[rows(1, 2048, 2048)], l1, [rows(k, 1)]], ids=ids)


case("mini_short_rows", dict(MINI, MGX_BFS_LAZY="0"), ("at", "beyond"), _mini_short_rows, adaptive=True,
     doc="65536 / 65537 short rows: BFS_MINI_SHORT_ROWS.  65536 discoveries need a level of 65536 entries in front, which no chain "
         "takes, so the level stands behind a device-wide slot and meets the M launch BEHIND the slots or another slot by how many "
         "slots the handle has learnt to enqueue: a fresh handle enqueues five and the level meets a slot, a handle that has seen the "
         "traversal enqueues one and `at` meets the M launch.  `beyond` is never an M launch's.  Asserted: labels, reached, m_t, the "
         "trace -- and that the counters are one of those the model's walks give (for `beyond`: the only one)")
# BFS_MINI_WCAP.  The list cannot overflow: bfs_mini_body looks at the workgroup's winner count after EVERY step -- one visit() per
# thread, at most NT = 1024 winners -- and flushes when it exceeds WCAP - NT, so it never holds more than WCAP.  The flush in the
# MIDDLE of a level needs more than WCAP - NT = 7168 winners in ONE of the 64 workgroups.  Units and edge ranks are dealt evenly (a
# level of BFS_MINI_EDGES_LATE entries gives each workgroup 2048): not there.  The row-per-thread walk (Es < 4 * nf_s, an average)
# deals rows in blocks -- workgroup b takes queue entries b * 1024 .. -- so a level whose first 1024 QUEUE ENTRIES carry eight tree
# entries each and the rest one gets there.  But which rows are the queue's first is not the graph's to say: the chain appends its
# winners in the order its waves' claims return, the queue build by the order its workgroups reach the cursor.  A case cannot
# place the heavy rows in workgroup 0, and a level heavy enough for ANY 1024 rows to exceed 7168 breaks Es < 4 * nf_s.  The path is
# reachable on the device and has no deterministic case here; the fuzz test's MGX_BFS_MINI=2 variants are what may meet it.

# -- long-row cut and unit blocks -------------------------------------------------------------------------------------------------
_LENS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def _row_lengths(member, ids):
    # three rows of every length either side of the cuts (long_min 1 / 8 / 32, the 64-entry unit), two tree entries each where they fit
    l1 = [rows(3, d, min(2, d)) for d in _LENS] + [rows(3, 0)]
    nk = sum(3 * min(2, d) for d in _LENS)
    return Layered([[rows(1, 3 * len(_LENS) + 3, 3 * len(_LENS) + 3)], l1, [rows(nk, 0)]], pad=11, ids=ids)


for _nm, _env in (("lengths_default", {}), ("lengths_long0", {"MGX_BFS_LONG_MIN": "0"}), ("lengths_long1", {"MGX_BFS_LONG_MIN": "1"}),
                  ("lengths_long8", {"MGX_BFS_LONG_MIN": "8"}), ("lengths_pack32", {"MGX_BFS_PACK24": "0"}),
                  ("lengths_dense", {"MGX_BFS_DENSE": "1000000", "MGX_BFS_VSHORT": "1000000"}),
                  ("lengths_dense32", {"MGX_BFS_DENSE": "1000000", "MGX_BFS_PACK24": "0"})):
    case(_nm, dict(WIDE, **_env), ("at",), _row_lengths,
         doc="rows of long_min - 1 / long_min / long_min + 1 and of 63 .. 129 entries, their discoveries at the rows' ends")


def _dense_edge(member, ids):
    # ub_units = 40 (at) / 39 (beyond); level 1 holds 20 / 19 units, level 2 holds 20 in both (dense in both)
    l1 = [rows(20, 64, 1)] if member == "at" else [rows(19, 64, 1), rows(1, 31, 1)]
    return Layered([[rows(1, 20, 20)], l1, [rows(20, 64)]], ids=ids)


case("dense_edge", dict(WIDE, **NOLAZY), ("at", "beyond"), _dense_edge, pair=(1, "dense_slots"), layouts=(True,),
     doc="the frontier's units * dense_div == ub_units (20 * 2 == 40) / one unit fewer (19 * 2 < 39)")

# -- short rows vertex by vertex --------------------------------------------------------------------------------------------------


def _vshort_edge(member, ids):
    # vs_edges = 16 + 160 + 1104 = 1280 (at): level 1's 160 entries * 8 == 1280; beyond: 159 * 8 < 1279.  Level 2 qualifies in both.
    l1 = [rows(16, 10, 4)] if member == "at" else [rows(15, 10, 4), rows(1, 9, 4)]
    return Layered([[rows(1, 16, 16)], l1, [rows(16, 18), rows(48, 17)]], ids=ids)


case("vshort_edge", dict(WIDE, **NOLAZY), ("at", "beyond"), _vshort_edge, pair=(1, "vshort_slots"), layouts=(True,),
     doc="E_short * vs_div == vs_edges (160 * 8 == 1280) / one entry fewer")
_VS = (0, 1, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65)


def _vs_classes(member, ids):
    l1 = [rows(70, d, min(1, d)) for d in _VS]      # 70 rows a degree: more than one wave step of every class
    nk = sum(70 * min(1, d) for d in _VS)
    return Layered([[rows(1, 70 * len(_VS), 70 * len(_VS))], l1, [rows(nk, 0)]], pad=5, ids=ids)


for _nm, _env in (("vs_classes_32", {}), ("vs_classes_64", {"MGX_BFS_LONG_MIN": "64"}), ("vs_classes_17", {"MGX_BFS_LONG_MIN": "17"})):
    case(_nm, dict(WIDE, MGX_BFS_VSHORT="1000000", MGX_BFS_LAZY="0", **_env), ("at",), _vs_classes, layouts=(True,),
         doc="rows either side of the 1- / 4- / 16-lane classes (and the 2-lane split at 9, the 8-lane variant at long_min <= 32), "
             "zero-entry rows in the frontier, every level walked vertex by vertex")

# -- lazy build -------------------------------------------------------------------------------------------------------------------


def _lazy_edge(member, ids):
    k = 1000 if member == "at" else 999
    return Layered([[rows(1, k, k)], [rows(k, 1)]], pad=4000 - 1 - k, ids=ids)


case("lazy_edge", dict(WIDE, **RULES), ("at", "beyond"), _lazy_edge, pair=(0, "lazy_slots"), layouts=(True,),
     doc="a tree level of 1000 marks with n = 4000 (marks * 4 == n) / 999 marks.  The slot behind the lazy build takes both queue-less bodies.")
case("lazy_always", dict(WIDE, MGX_BFS_DENSE="2", MGX_BFS_VSHORT="8", MGX_BFS_LAZY="1048576"), ("at",),
     lambda member, ids: Layered([[rows(1, 40, 1)], [rows(1, 70, 3)], [rows(1, 5, 1), rows(2, 0)], [rows(1, 33)]], pad=100, ids=ids),
     layouts=(True,), doc="MGX_BFS_LAZY=1048576: every build behind a mark is lazy; frontiers of one vertex on the queue-less bodies")

# -- queue build ------------------------------------------------------------------------------------------------------------------
for _k in (8191, 8192, 8193, 16382, 16383, 16384):
    for _bl in ("0", "1"):
        case("build_%d_list%s" % (_k, _bl), dict(WIDE, MGX_BFS_BUILD_LIST=_bl), ("at",),
             (lambda k: lambda member, ids: Layered([[rows(1, k, k)], [rows(k, 1)]], pad=3, ids=ids))(_k),
             doc="one level discovering %d vertices (ids 1 .. %d as specified): a batch of BFS_BUILD_LIST discoveries, a whole "
                 "BFS_BUILD_VPB range, and one more; a partial last range" % (_k, _k))

# -- LDS bitmap prefix: a star whose leaves cover every id, so the discoveries at 32 * W - 1 and 32 * W (W = 18000, 20384, 20400)
#    are among them with and without a layout ------------------------------------------------------------------------------------
for _n in (HOT_N, HOT_N + 1, 700001):
    for _nm, _env in (("", {}), ("_hot0", {"MGX_BFS_HOT_MIN_EDGES": "0"}), ("_nocold", {"MGX_BFS_COLD": "0"})):
        case("star_%d%s" % (_n, _nm), dict(WIDE, **_env), ("at",),
             (lambda n: lambda member, ids: Layered([[rows(1, n - 1, n - 1)], [rows(n - 1, 0)]], ids=ids))(_n), ids=("spec",),
             doc="n = %d: one row names every other vertex" % _n)
def _fan(member, ids):
    # source -> 22580 short rows (20 of 31 tree entries, 22560 of 30) -> 677420 leaves: n = 700001, every id from 22581 on is a
    # short row's discovery -- the ids either side of all three prefixes among them, without a layout (ids as specified) and with one
    # (the leaves have no entries: the layout puts them last)
    return Layered([[rows(1, 22580, 22580)], [rows(20, 31, 31), rows(22560, 30, 30)], [rows(677420, 0)]], ids=ids)


for _nm, _env, _lay in (("fan", {}, (False, True)), ("fan_hot0", {"MGX_BFS_HOT_MIN_EDGES": "0"}, (False, True)),
                        ("fan_vshort", {"MGX_BFS_VSHORT": "1000000"}, (True,)), ("fan_novshort", {"MGX_BFS_VSHORT": "0"}, (True,))):
    case(_nm, dict(WIDE, **_env), ("at",), _fan, layouts=_lay, ids=("spec",),
         doc="the SHORT rows' bodies at the prefixes: 677420 entries (>= hot_min_edges) of rows of 30 and 31 entries discover every id up "
             "to 700000 -- the queue walk (BFS_WAVE_HOTW 18000) and, with a layout, the vertex-by-vertex body (BFS_DENSE_HOTW 20384)")
case("star_behind_lazy", dict(WIDE, MGX_BFS_LAZY="1048576"), ("cold", "hot"),
     lambda member, ids: Layered([[rows(1, 1, 1)], [rows(1, (700001 if member == "cold" else 60001) - 2, (700001 if member == "cold" else 60001) - 2)],
                                  [rows((700001 if member == "cold" else 60001) - 2, 0)]], ids=ids), layouts=(True,), ids=("spec",),
     doc="a lazy build behind a level of one mark: the slot behind it reads a frontier of ONE vertex from the bitmap, with cold entries "
         "in its row (n = 700001) and without (n = 60001)")

# -- depth ------------------------------------------------------------------------------------------------------------------------
for _d in (4095, 4096, 4097, 5000):
    for _nm, _env in (("chained", {}), ("wide", WIDE)):
        case("path_%d_%s" % (_d, _nm), _env, ("at",),
             (lambda d: lambda member, ids: Layered([[rows(1, 1, 1)]] * d + [[rows(1, 0)]], pad=2, ids=ids))(_d), ids=(7,),
             doc="a path of %d levels: BFS_MAX_TRACE either side, the slot ring, the batches of launches" % _d)

# -- direction-optimising (mode 1, alpha = 2; the graph is directed: the bottom-up levels read the graph's genuine CSC, and the
#    library runs such a traversal without the layout) ----------------------------------------------------------------------------


def _do_edge(member, ids):
    # level 1 holds 100 / 101 frontier rows (one entry each: the first a tree entry, the others filler) with 200 vertices unvisited:
    # 200 < 100 * 2 is false (top-down), 200 < 101 * 2 holds -- and level 2 (ONE row, ~199 unvisited) stays bottom-up behind it
    k = 100 if member == "at" else 101
    return Layered([[rows(1, k, k)], [rows(1, 1, 1), rows(k - 1, 1)], [rows(1, 1, 1)], [rows(1, 0)]], pad=198, ids=ids)


for _nm, _env in (("do_edge", {}), ("do_edge_no_chain", {"MGX_BFS_DO_CHAIN": "0"}), ("do_edge_own_pull", {"MGX_BFS_MERGED_PULL": "0"}),
                  ("do_edge_push_chain", SC0), ("do_edge_list", {"MGX_BFS_BUILD_LIST": "1"})):
    case(_nm, _env, ("at", "beyond"), _do_edge, pair=(1, "push_levels", 2), layouts=(False,), mode=1, alpha=2.0,
         doc="unvisited == nf * alpha exactly (stays top-down) / one frontier vertex more (bottom-up from there on, also on a level "
             "the rule alone would run top-down); the switch falls on a level the chain would take")

# -- contested claims -------------------------------------------------------------------------------------------------------------


def _contested(fan, deg, kids):
    return lambda member, ids: Layered([[rows(1, fan, fan)], [rows(fan, deg, kids, "contested")], [rows(fan * kids, 0)]], ids=ids)


case("contested_chain", SC0, ("at",), _contested(64, 64, 2), doc="4096 contested entries, late: the chain's claims have losers")
case("contested_mini", MINI, ("at",), _contested(1024, 64, 2), doc="65536 contested entries, late: an M launch's claims")
case("contested_slot", dict(WIDE, MGX_BFS_LAZY="0"), ("at",), _contested(1024, 160, 8), doc="163840 contested entries: a device-wide slot's marks")

# What each edge case promises about the level it is about: member -> [(level, what, value)].  what: "nf" / "E" both queues,
# "nf_s" / "nf_l" / "E_s" / "E_l" one queue (at the case's long_min), "units" the long rows' 64-entry units, "kids" the level's
# discoveries, "late" = 4 * (vertices reached when the level opens) - n.
PROMISE = {
    "chain_early": {"at": [(1, "E", 1536), (1, "late", 4 * 49 - 497)], "beyond": [(1, "E", 1537), (1, "late", 4 * 49 - 497)]},
    "chain_late": {"at": [(1, "E", 4096), (1, "late", 4 * 65 - 129)], "beyond": [(1, "E", 4097), (1, "late", 4 * 65 - 129)]},
    "chain_cap": {"at": [(1, "E", 6144)], "beyond": [(1, "E", 6145)]},
    "chain_late_rule": {"at": [(1, "E", 2000), (1, "late", 0)], "beyond": [(1, "E", 2000), (1, "late", -1)]},
    "chain_full_list": {"at": [(1, "E", 6144), (1, "kids", 6144), (2, "nf", 6144), (2, "E", 6144)],
                        "beyond": [(1, "E", 6144), (1, "kids", 6144), (2, "nf", 6144), (2, "E", 6145)]},
    "chain_entry_early": {"at": [(0, "E", 1536), (0, "late", 4 - 1544)], "beyond": [(0, "E", 1537), (0, "late", 4 - 1545)]},
    "inplace_entry_early": {"at": [(0, "E", 1536)], "beyond": [(0, "E", 1537)]},
    "inplace_default": {"at": [(1, "E", 4096)], "beyond": [(1, "E", 4097)]},
    "inplace_no_tail": {"at": [(1, "E", 4096)], "beyond": [(1, "E", 4097)]},
    "inplace_no_front": {"at": [(1, "E", 4096)], "beyond": [(1, "E", 4097)]},
    "inplace_cap": {"at": [(1, "E", 12288)], "beyond": [(1, "E", 12289)]},
    "mini_lcap": {"at": [(2, "nf_l", 4096), (2, "nf_s", 0), (2, "late", 3 * 5497)], "beyond": [(2, "nf_l", 4097), (2, "E", 4097 * 16)]},
    "mini_early": {"at": [(1, "E", 32768), (1, "kids", 32768)], "beyond": [(1, "E", 32769), (1, "kids", 32769)]},
    "mini_late": {"at": [(1, "E", 131072), (1, "late", 4 * 1025 - 2049)], "beyond": [(1, "E", 131073)]},
    "dense_edge": {"at": [(1, "units", 20)], "beyond": [(1, "units", 19)]},
    "vshort_edge": {"at": [(1, "E_s", 160)], "beyond": [(1, "E_s", 159)]},
    "lazy_edge": {"at": [(0, "kids", 1000)], "beyond": [(0, "kids", 999)]},
}
for _nm in ("do_edge", "do_edge_no_chain", "do_edge_own_pull", "do_edge_push_chain", "do_edge_list"):
    PROMISE[_nm] = {"at": [(1, "nf", 100), (1, "late", 4 * 101 - 301), (2, "nf", 1)], "beyond": [(1, "nf", 101), (1, "late", 4 * 102 - 302), (2, "nf", 1)]}
