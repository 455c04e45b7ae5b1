"""Inputs of the betweenness centrality's edge tests, shared by the CPU suite (tests/test_bc_cases_cpu.py: every case
holds what it claims) and the GPU suite (tests/test_gpu_bc_paths.py: the device computes it and took the launches it should).
numpy only; everything is generated with coloring_model.csr.

A case is a dict: name, group, ro, ci, symmetric (False: the GPU test builds the graph's CSC), sources (int32), env (the switches
the run reads), want ("closed": closed forms, compared bit for bit; "exact": tests/bc_exact.py with the one-implementation bound;
"model": tests/bc_model.py with the two-implementation bound) and the facts it exists for.  expected(case) computes the arrays
once per case and process.

Each group stands on one host decision or kernel edge of include/mgx/bc_fused.hpp:

  key_bits          the radix sort's width: source() sorts keys below K = (D' + 1) * 4 over the smallest end_bit with
                    2^end_bit >= K, D' = levels + 1, and the traversal's `levels` is the depth or the depth - 1.  Paths of n
                    vertices put K just below, on and just above 256 and 4096 for both meanings (symmetric: the last vertex
                    expands its back entry, levels = n; directed: the last vertex is a sink, levels = n - 1 and its key
                    4 n is the largest the width has to hold: n = 64 and 1024 need the ninth and the thirteenth bit for one key).
  bounds_growth     the list bounds' room.  The constructor calls grow_bounds(min(n, 65536) + 2), which makes
                    bound_cap = (min(n, 65536) + 4) * 4 + 1; source() grows behind a wait when (D' + 2) * 4 + 1 > bound_cap,
                    that is D' > min(n, 65536) + 2.  On the symmetric path from vertex 0, D' = n + 1, so for n >= 65536 the
                    bounds grow when n > 65537: the largest n that does not grow them is 65 537, the smallest that does 65 538.
  sigma_limits      sigma = 2^v exactly on the path with every entry twice: the flags at 2^53 and 2^1024, 1 / sigma subnormal.
  class_edges       rows of 16 | 17, 8191 | 8192 | 8193, 16384 | 16385 entries under the default thresholds.
  plan              the two chain-plan loops of source() on level widths of chain | chain + 1.
  behind_the_trace  a level of 3000 wave rows past the 4096 levels the traversal traces: it counts as small.
  parity_back_edges directed entries from level d back onto d - 1, d - 3, d - 5: the levels whose parity level d reads."""
import functools

import numpy as np

from tests import bc_exact as exact
from tests import bc_model as model
from tests import coloring_model as cm

KEY_STRIDE = 4
LANE, WAVE, HUGE = 0, 1, 2
DEFAULTS = {"lane_max": 16, "huge_min": 8192, "seg": 8192, "chain": 1024}
ENV_NAMES = {"lane_max": "MGX_BC_LANE_MAX", "huge_min": "MGX_BC_HUGE_MIN", "seg": "MGX_BC_SEG", "chain": "MGX_BC_CHAIN"}
TRACE = 4096                     # the levels the traversal traces (BFS_MAX_TRACE)
BOUND_LEVELS = 1 << 16           # the constructor's min(n, 65536)

KEY_BITS_N = list(range(60, 67)) + list(range(1020, 1027))
SIGMA_N = [53, 54, 1024, 1025, 1026]
HUB_ROWS = (16, 17, 8191, 8192, 8193, 16384, 16385)
POOL = 16384
WIDTHS = {"a": [1, 1024, 1025, 1024, 1025, 1025, 1024, 1024, 1],
          "b": [1, 1024, 1024, 1025, 1025, 1024, 1025, 1024, 1],       # a, reversed
          "c": [1, 1025, 1024, 1]}


# ---- restatements of the host's decisions ---------------------------------------------------------------------------------------------
def opts(env):
    """the four switches a handle reads under `env`"""
    return {k: int(env.get(ENV_NAMES[k], DEFAULTS[k])) for k in DEFAULTS}


def row_class(length, o):
    """bc_opts_t::row_class"""
    return LANE if length <= o["lane_max"] else (HUGE if length >= o["huge_min"] else WAVE)


def class_counts(offsets, o):
    """(lane rows, wave rows, huge rows, segments of the huge rows) of the rows with these offsets"""
    count, segments = [0, 0, 0], 0
    for length in np.diff(np.asarray(offsets, dtype=np.int64)).tolist():
        k = row_class(length, o)
        count[k] += 1
        if k == HUGE:
            segments += (length + o["seg"] - 1) // o["seg"]
    return count[0], count[1], count[2], segments


def in_offsets(ro, ci):
    n = len(ro) - 1
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(ci, dtype=np.int64), minlength=n))])


def traversal_levels(ro, labels):
    """what the fused traversal reports as `levels`: the levels that expanded at least one entry"""
    has = (np.diff(ro) > 0) & (labels >= 0)
    return int(labels[has].max()) + 1 if has.any() else 0


def key_count(levels):
    """K of source(): the keys 0 .. K - 1 of a traversal that reported `levels`"""
    return (levels + 1 + 1) * KEY_STRIDE


def end_bit(levels):
    K, b = key_count(levels), 1
    while b < 32 and (1 << b) < K:
        b += 1
    return b


def bound_cap(n):
    """bc_state_t's constructor: grow_bounds(min(n, 65536) + 2) -> (levels + 2) * 4 + 1"""
    return (min(n, BOUND_LEVELS) + 2 + 2) * KEY_STRIDE + 1


def grows(levels, cap):
    """the test in source(): D' = levels + 1"""
    return (levels + 1 + 2) * KEY_STRIDE + 1 > cap


def predicted(widths, chain, levels, huge_in=False, huge_out=False, two_sorts=False):
    """The two plan loops of source() for ONE source: (forward chain launches, backward chain launches, all launches of the run).
    widths[d] is the number of vertices on level d, `levels` what the traversal reported (the trace holds min(levels, 4096) levels;
    a level behind it counts as small).  Fixed launches as the code counts them: 5 of begin_run, 3 for clear, seed and keys, 3 per
    sort (clear, sort, bounds), 1 per grid level and 2 more when the direction has a huge row, 1 per chain, 1 for k_bc_finish."""
    D = levels + 1
    traced = min(levels, TRACE)

    def small(d):
        return chain > 0 and (d >= traced or widths[d] <= chain)

    launches = 5 + 3 + 3 * (2 if two_sorts else 1) + 1
    fwd = bwd = 0
    d = 1
    while d <= D - 1:
        e = d
        while e <= D - 1 and small(e):
            e += 1
        if e - d >= 2:
            fwd += 1
            launches += 1
            d = e
            continue
        launches += 3 if huge_in else 1
        d += 1
    d = D - 2
    while d >= 1:
        e = d
        while e >= 1 and small(e):
            e -= 1
        if d - e >= 2:
            bwd += 1
            launches += 1
            d = e
            continue
        launches += 3 if huge_out else 1
        d -= 1
    return fwd, bwd, launches


# ---- builders -------------------------------------------------------------------------------------------------------------------------
def path(n, symmetric=True, copies=1):
    a = np.tile(np.arange(n - 1), copies)
    return cm.csr(n, a, a + 1, symmetric=symmetric)


def caterpillar(p, leaves):
    """a path of p vertices whose last vertex carries `leaves` leaves"""
    a = np.arange(p - 1)
    return cm.csr(p + leaves, np.concatenate([a, np.full(leaves, p - 1)]), np.concatenate([a + 1, p + np.arange(leaves)]))


def hubs(symmetric):
    """root 0, hubs 1 .. 7, a pool of 16 384 vertices from id 8.  Hub k is joined to the root and to the first HUB_ROWS[k] - 1 pool
    vertices.  symmetric: every pair both ways, hub rows of exactly HUB_ROWS entries.  Directed: the downward entries only (root
    -> hub, hub -> pool), so the out-rows of the hubs hold HUB_ROWS - 1 entries (15, 16, 8190, 8191, 8192, 16383, 16384) and every
    in-row at most 7."""
    first = 1 + len(HUB_ROWS)
    s, d = [np.zeros(len(HUB_ROWS), dtype=np.int64)], [1 + np.arange(len(HUB_ROWS))]
    for k, r in enumerate(HUB_ROWS):
        s.append(np.full(r - 1, 1 + k))
        d.append(first + np.arange(r - 1))
    return cm.csr(first + POOL, np.concatenate(s), np.concatenate(d), symmetric=symmetric)


def layered(widths):
    """levels of the given widths, the root alone on level 0; vertex j of a level is joined to the vertices j, j + 1 and j + 7
    (mod the width) of the level before it -- thrice to the same vertex where that level has one --, symmetric.  Every vertex has
    a parent, so the BFS levels from the root are the widths."""
    first = np.concatenate([[0], np.cumsum(widths)])
    s, d = [], []
    for lv in range(1, len(widths)):
        j = np.arange(widths[lv])
        for step in (0, 1, 7):
            s.append(first[lv - 1] + (j + step) % widths[lv - 1])
            d.append(first[lv] + j)
    return cm.csr(int(first[-1]), np.concatenate(s), np.concatenate(d))


def fan_behind_a_path(p=4100, fan=3000, deep=60, each=20):
    """a path of p vertices, its end joined to `fan` vertices, each of those to `each` of `deep` vertices one level deeper"""
    a = np.arange(p - 1)
    f = p + np.arange(fan)
    s = [a, np.full(fan, p - 1), np.repeat(f, each)]
    d = [a + 1, f, p + fan + (np.repeat(np.arange(fan), each) + np.tile(np.arange(each), fan)) % deep]
    return cm.csr(p + fan + deep, np.concatenate(s), np.concatenate(d))


def back_edges(n=41):
    """0 -> 1 -> .. -> n - 1 and, from every v, entries back to v - 1, v - 3 and v - 5 where they exist"""
    v = np.arange(n)
    s, d = [v[:-1]], [v[:-1] + 1]
    for k in (1, 3, 5):
        s.append(v[k:])
        d.append(v[k:] - k)
    return cm.csr(n, np.concatenate(s), np.concatenate(d), symmetric=False)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _case(name, group, graph, symmetric, sources, want, env=None, **facts):
    c = {"name": name, "group": group, "ro": graph[0], "ci": graph[1], "symmetric": symmetric,
         "sources": np.asarray(sources, dtype=np.int32), "want": want, "env": dict(env or {})}
    c.update(facts)
    return c


def _plan_widths(which, chain):
    return [w - 1024 + chain if w >= 1024 else w for w in WIDTHS[which]]


def _builders():
    b = {}
    for n in KEY_BITS_N:
        b["key_bits-sym-%d" % n] = lambda n=n: _case("key_bits-sym-%d" % n, "key_bits", path(n), True, [0], "closed",
                                                     path_n=n, levels=n, copies=1)
        b["key_bits-dir-%d" % n] = lambda n=n: _case("key_bits-dir-%d" % n, "key_bits", path(n, symmetric=False), False, [0], "closed",
                                                     path_n=n, levels=n - 1, copies=1)
    for p in (63, 1023):
        # the leaves' keys are 4 (p + 1) = 256 and 4096: one bit too few sorts them in front of level 0
        b["key_bits-caterpillar-%d" % p] = lambda p=p: _case("key_bits-caterpillar-%d" % p, "key_bits", caterpillar(p, 70), True, [0], "exact",
                                                             env={"MGX_BC_HUGE_MIN": "64", "MGX_BC_SEG": "64"}, path_n=p, leaves=70,
                                                             levels=p + 1)
    for n in (BOUND_LEVELS + 1, BOUND_LEVELS + 2):
        b["bounds_growth-%d" % n] = lambda n=n: _case("bounds_growth-%d" % n, "bounds_growth", path(n), True, [0], "closed",
                                                      path_n=n, levels=n, copies=1, grows=n == BOUND_LEVELS + 2)
    flags = {53: (0, 0), 54: (1, 0), 1024: (1, 0), 1025: (1, 1), 1026: (1, 1)}
    for n in SIGMA_N:
        b["sigma_limits-%d" % n] = lambda n=n: _case("sigma_limits-%d" % n, "sigma_limits", path(n, copies=2), True, [0],
                                                     "closed" if n <= 1024 else "model", path_n=n, levels=n, copies=2, flags=flags[n])
    first = 1 + len(HUB_ROWS)
    b["class_edges-sym"] = lambda: _case("class_edges-sym", "class_edges", hubs(True), True, [0, first, first + 8190, 1 + HUB_ROWS.index(8191)],
                                         "exact", longest_in=16385, entries=114756)
    b["class_edges-dir"] = lambda: _case("class_edges-dir", "class_edges", hubs(False), False, [0, 1 + HUB_ROWS.index(8191)], "exact",
                                         longest_in=7, entries=57378)
    for which in WIDTHS:
        for chain in (1024, 4):
            name = "plan-%s-chain%d" % (which, chain)
            b[name] = lambda which=which, chain=chain, name=name: _case(
                name, "plan", layered(_plan_widths(which, chain)), True, [0], "exact",
                env={} if chain == 1024 else {"MGX_BC_CHAIN": str(chain)}, widths=_plan_widths(which, chain),
                levels=len(WIDTHS[which]))
    b["behind_the_trace"] = lambda: _case("behind_the_trace", "behind_the_trace", fan_behind_a_path(), True, [0], "model",
                                          widths=[1] * 4100 + [3000, 60], levels=4102)
    b["parity_back_edges"] = lambda: _case("parity_back_edges", "parity_back_edges", back_edges(), False, [0], "exact", path_n=41, levels=40)
    return b


_BUILDERS = _builders()
NAMES = list(_BUILDERS)


def names(group):
    return [k for k in NAMES if k == group or k.startswith(group + "-")]


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILDERS[name]()


def _closed_path(c):
    """the path from vertex 0 with every entry `copies` times: sigma[v] = copies^v, delta[v] = n - 1 - v behind the source"""
    n = c["path_n"]
    v = np.arange(n)
    delta = (n - 1.0 - v) * (v > 0)
    two = 2 if c["symmetric"] else 1
    return {"labels": v.astype(np.int32), "sigma": float(c["copies"]) ** v, "delta": delta, "bc": delta.copy(),
            "stats": [1, n, n] + list(c.get("flags", (0, 0))),
            "longest_in": c["copies"] * (two if n > 2 else 1), "longest_out": c["copies"] * (two if n > 2 else 1)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> dict(labels, sigma, delta, bc as the device's arrays should be; stats = [sources, levels, reached, inexact, overflow];
    longest_in, longest_out; rel = the relative bound on delta and bc (0: bit for bit))"""
    c = get(name)
    if c["want"] == "closed":
        w = _closed_path(c)
        w["rel"] = 0.0
    elif c["want"] == "exact":
        e = exact.run(c["ro"], c["ci"], c["sources"], c["symmetric"])
        w = {"labels": e["labels"], "sigma": e["sigma_f"], "delta": e["delta"], "bc": e["bc"], "stats": e["stats"],
             "longest_in": e["longest_in"], "longest_out": e["longest_out"]}
        w["rel"] = exact.bound(e["depth"], max(e["longest_in"], e["longest_out"]), len(c["sources"]))
    else:
        m = model.run(c["ro"], c["ci"], c["sources"], c["symmetric"])
        w = {k: m[k] for k in ("labels", "sigma", "delta", "bc", "stats", "longest_in", "longest_out")}
        w["rel"] = model.rtol(m["stats"][1], max(m["longest_in"], m["longest_out"]), len(c["sources"]))
    for k in ("labels", "sigma", "delta", "bc"):
        w[k].setflags(write=False)
    return w
