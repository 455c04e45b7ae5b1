"""Graphs and pair lists the vertex similarity's suites share (tests/test_sim_cpu.py, tests/test_gpu_sim.py): rows of given lengths
and given contents, so that the pairs sit on every edge of the classification (tests/sim_model.py: classify).  A case is a dict:
name, ro, ci (a symmetric CSR), pairs int32[P, 2], opts (the cuts the handle is to read; {} = the defaults) and need: the (la, lb,
class) triples the case exists for -- tests/test_sim_cpu.py asserts from the model's own classifier that each is there."""
import numpy as np

from tests import sim_model as model
from tests.lpa_cases import clique, path, random_symmetric, star, sym  # noqa: F401

ENV = {"short_max": "MGX_SIM_SHORT_MAX", "probe_ratio": "MGX_SIM_PROBE_RATIO", "wave_max": "MGX_SIM_WAVE_MAX", "stage": "MGX_SIM_STAGE"}
N, L, P, W, B = model.NONE, model.LANE, model.PROBE, model.WAVE, model.BLOCK


def rows_graph(rows, pool, lead=0):
    """row vertex i (ids lead .. lead + len(rows) - 1) is adjacent to the pool members rows[i] names (indices into the pool); the pool
    vertices take the ids before `lead` and behind the row vertices, so that pool index 0 is vertex 0 when lead > 0 and the last pool
    index is vertex n - 1.  Row vertices are adjacent to pool vertices only: d(row i) = len(set(rows[i])) -> (ro, ci, the row ids)"""
    R = len(rows)
    ids = np.concatenate([np.arange(lead), lead + R + np.arange(pool - lead)]).astype(np.int64)
    a = np.concatenate([np.full(len(r), lead + i, dtype=np.int64) for i, r in enumerate(rows)] + [np.zeros(0, dtype=np.int64)])
    b = np.concatenate([ids[np.asarray(r, dtype=np.int64)] for r in rows] + [np.zeros(0, dtype=np.int64)])
    ro, ci = sym(pool + R, a, b)
    return ro, ci, lead + np.arange(R)


def _subset(rng, pool, k):
    return np.sort(rng.permutation(pool)[:k])


def _case(name, rows, pool, pairs_of, need, opts=None, lead=0):
    ro, ci, ids = rows_graph(rows, pool, lead)
    pairs = np.array([(ids[i], ids[j]) for i, j in pairs_of], dtype=np.int32).reshape(-1, 2)
    return {"name": name, "ro": ro, "ci": ci, "pairs": pairs, "opts": dict(opts or {}), "need": need}


def cuts(seed=1):
    """every cut of the default classification, a pair on each side: la in {0, 1, 16, 17, 512, 513}, lb just below and at 16 la"""
    rng = np.random.default_rng(seed)
    s, r, w = model.SHORT_MAX, model.PROBE_RATIO, model.WAVE_MAX
    pool = r * (w + 1) + 8
    lengths = [0, 0, 1, 1, pool, s, s, r * s, s + 1, s + 1, r * (s + 1) - 1, r * (s + 1), w, w, r * w - 1, r * w, w + 1, w + 1, r * (w + 1) - 1,
               r * (w + 1)]
    rows = [_subset(rng, pool, k) for k in lengths]
    at = {}
    for i, k in enumerate(lengths):
        at.setdefault(k, []).append(i)
    pr = [(at[0][0], at[0][1]), (at[0][0], at[s][0]), (at[1][0], at[1][1]), (at[1][0], at[pool][0]), (at[s][0], at[s][1]), (at[s][0], at[r * s][0]),
          (at[s + 1][0], at[s + 1][1]), (at[s + 1][0], at[r * (s + 1) - 1][0]), (at[s + 1][0], at[r * (s + 1)][0]),
          (at[w][0], at[w][1]), (at[w][0], at[r * w - 1][0]), (at[w][0], at[r * w][0]),
          (at[w + 1][0], at[w + 1][1]), (at[w + 1][0], at[r * (w + 1) - 1][0]), (at[w + 1][0], at[r * (w + 1)][0])]
    pr += [(j, i) for i, j in pr] + [pr[4], pr[9], (at[w][0], at[w][0]), (at[0][0], at[0][0]), (at[pool][0], at[pool][0])]
    need = [(0, 0, N), (0, s, N), (1, 1, L), (1, pool, L), (s, s, L), (s, r * s, L), (s + 1, s + 1, W), (s + 1, r * (s + 1) - 1, W),
            (s + 1, r * (s + 1), P), (w, w, W), (w, r * w - 1, W), (w, r * w, P), (w + 1, w + 1, B), (w + 1, r * (w + 1) - 1, B),
            (w + 1, r * (w + 1), P), (pool, pool, B)]
    return _case("cuts", rows, pool, pr, need)


def contents(stage=64):
    """what the rows hold, at a stage of `stage` entries: identical rows, disjoint rows, interleaved rows (evens against odds), and
    a single common element first in its chunk, last in its chunk, equal to vertex 0, equal to vertex n - 1; wave and block pairs"""
    s = stage
    pool = 4 * (model.WAVE_MAX + 2 * s + 8)
    ev, od = np.arange(0, pool, 2), np.arange(1, pool, 2)
    la_w, la_b = 2 * s + 1 + (model.SHORT_MAX if 2 * s + 1 <= model.SHORT_MAX else 0), model.WAVE_MAX + s + 1
    rows, pr, need = [], [], []
    for la in (la_w, la_b):
        base = len(rows)
        a = ev[1:la + 1]                                           # (vertex 0 and the last one are kept out of it)
        first, last = a[s], a[s - 1]                               # the first entry of the second chunk, the last of the first
        others = od[:la + 3]
        rows += [a, a.copy(), od[:la + 2], np.sort(np.concatenate([others, [first]])), np.sort(np.concatenate([others, [last]])),
                 np.concatenate([[0], a]), np.concatenate([[0], others]), np.concatenate([a, [pool - 1]]), np.concatenate([others[:-1], [pool - 2, pool - 1]])]
        pr += [(base, base + 1), (base, base + 2), (base, base + 3), (base, base + 4), (base + 5, base + 6), (base + 7, base + 8), (base + 8, base + 7)]
        cls = W if la <= model.WAVE_MAX else B
        need += [(la, la, cls), (la, la + 2, cls), (la, la + 4, cls), (la + 1, la + 4, cls)]
    return _case("contents_stage_%d" % s, rows, pool, pr, need, {"stage": s}, lead=1)


def stages(stage):
    """la in {stage, stage + 1, 2 stage + 1} staged by a wave and by a workgroup, lb round la and well above it; short_max 0 so
    that rows of 1 .. 3 entries are staged too"""
    rng = np.random.default_rng(stage)
    w = model.WAVE_MAX
    las = [stage, stage + 1, 2 * stage + 1]
    pool = 3 * (w + 2 * stage + 4)
    rows, pr, need = [], [], []
    for la in las + [w + x for x in las]:
        cls = W if la <= w else B
        for lb in (la, la + 1, min(2 * la + 3, pool)):
            if lb >= model.PROBE_RATIO * la:
                continue
            i = len(rows)
            rows += [_subset(rng, min(pool, 3 * lb), la), _subset(rng, min(pool, 3 * lb), lb)]
            pr += [(i, i + 1), (i + 1, i)]
            need.append((la, lb, cls))
    return _case("stages_%d" % stage, rows, pool, pr, need, {"stage": stage, "short_max": 0})


def two_hubs(entries=10000):
    """two hubs of `entries` entries that share half of them (n about 2 entries + 1): a workgroup's pair of several chunks"""
    pool = 2 * entries - 1
    rows = [np.arange(entries), np.arange(entries // 2, entries // 2 + entries), np.arange(0, 40, 2)]
    return _case("two_hubs", rows, pool, [(0, 1), (1, 0), (0, 0), (2, 0), (2, 1)], [(entries, entries, B), (20, entries, P)])


def hub_rows(pairs=1024, hub=100000, seed=5):
    """`pairs` pairs of a row of 16 - 20 entries against one of a few rows of `hub` entries -> (case, the same rows paired with rows of 100)"""
    rng = np.random.default_rng(seed)
    pool = hub + hub // 4
    hubs = [np.sort(rng.permutation(pool)[:hub]) for _ in range(4)]
    plain = [np.sort(rng.permutation(pool)[:100]) for _ in range(4)]
    small = [np.sort(rng.choice(np.unique(rng.integers(0, pool, 64)), 16 + i % 5, replace=False)) for i in range(pairs)]
    rows = hubs + plain + small
    pr = [(8 + i, i % 4) for i in range(pairs)]
    case = _case("hub", rows, pool, pr, [(16, hub, L), (17, hub, P), (20, hub, P)])
    case["plain_pairs"] = np.array([(8 + i, 4 + i % 4) for i in range(pairs)], dtype=np.int32)      # (lead 0: a row's id is its index)
    return case


def small_random(n=300, m=2400, seed=7, pairs=200):
    """a random symmetric graph and random pairs, (u, v) beside (v, u), u == v and a duplicated pair among them"""
    rng = np.random.default_rng(seed)
    ro, ci = random_symmetric(n, m, seed)
    pr = rng.integers(0, n, (pairs, 2))
    pr = np.concatenate([pr, pr[:10, ::-1], np.stack([pr[:5, 0], pr[:5, 0]], axis=1), pr[:3]])
    return {"name": "random_%d" % n, "ro": ro, "ci": ci, "pairs": pr.astype(np.int32), "opts": {}, "need": []}


def all_cases():
    return [cuts(), contents(64), contents(1), stages(64), stages(1), two_hubs(), small_random()]
