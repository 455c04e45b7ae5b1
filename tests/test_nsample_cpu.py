"""CPU suite for the neighbour sampling (mgx_nsample_*, include/mgx/nsample_fused.hpp, include/gunrock/nsample/): the header declares
and the library exports it, NULL handles and invalid parameters are statuses, the switches are in the table, the kernels keep out
of scratch, and the model the GPU tests compare against (tests/nsample_model.py) has the properties of the definition and samples
uniformly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nsample_cases as cases
from tests import nsample_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_nsample_create", "mgx_nsample_free", "mgx_nsample_run", "mgx_nsample_enact", "mgx_nsample_vertices", "mgx_nsample_hop_offsets",
         "mgx_nsample_row_offsets", "mgx_nsample_cols", "mgx_nsample_entry_pos", "mgx_nsample_seed_local", "mgx_nsample_vertices_device",
         "mgx_nsample_row_offsets_device", "mgx_nsample_cols_device", "mgx_nsample_entry_pos_device", "mgx_nsample_bins",
         "mgx_nsample_set_timing", "mgx_nsample_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_ns_%sE" % k,) for k in ("mark", "rank_count", "rank_apply", "rows", "sample", "long", "finish")]
KERNELS += [("7nsample", "sample_functor_t"), ("7nsample", "fresh_functor_t")]
SWITCHES = {"MGX_NSAMPLE_SHORT_MAX", "MGX_NSAMPLE_WAVE_MAX", "MGX_NSAMPLE_SEG"}


def test_header_declares_and_library_exports_nsample(built):
    import mini_amd
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    for name in NAMES:
        assert re.search(r"MGX_API int %s\(" % name, header), name
        assert hasattr(mini_amd.lib, name), name
    sp = mini_amd.NeighborSampleProblem
    assert sp.KEYS == model.STAT_KEYS + ("launches", "host_waits")
    for member in ("run", "enact", "vertices", "hop_offsets", "row_offsets", "cols", "entry_pos", "seed_local", "block", "vertices_device_ptr",
                   "row_offsets_device_ptr", "cols_device_ptr", "entry_pos_device_ptr", "bins", "set_timing", "phase_ms", "close"):
        assert hasattr(sp, member), member
    for word in ("STORED order", "Floyd", "insertion order", "sampled at most once"):
        assert word in sp.__doc__, word


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, d = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 14)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_nsample_create(None, C.byref(h)) == bad
    for go in (lib.mgx_nsample_run, lib.mgx_nsample_enact):
        assert go(None, None, 0, None, 0, 0, 1, st) == bad
        assert b"NULL" in lib.mgx_last_error()
    for fn in (lib.mgx_nsample_vertices, lib.mgx_nsample_hop_offsets, lib.mgx_nsample_row_offsets, lib.mgx_nsample_cols, lib.mgx_nsample_entry_pos,
               lib.mgx_nsample_seed_local, lib.mgx_nsample_bins, lib.mgx_nsample_phase_ms):
        assert fn(None, None) == bad
    for fn in (lib.mgx_nsample_vertices_device, lib.mgx_nsample_row_offsets_device, lib.mgx_nsample_cols_device, lib.mgx_nsample_entry_pos_device):
        assert fn(None, C.byref(d)) == bad
    assert lib.mgx_nsample_set_timing(None, 1) == bad
    assert lib.mgx_nsample_free(None) == 0


@pytest.mark.parametrize("args, word", [
    (dict(hops=-1), "hops"), (dict(hops=17), "hops"), (dict(fanouts=[0]), "fanouts"), (dict(fanouts=[5, 65]), "fanouts"),
    (dict(fanouts=[-2, 3]), "fanouts"), (dict(fanouts=None, hops=2), "fanouts"), (dict(count=-1), "count")])
def test_invalid_parameters_are_statuses(built, args, word):
    """the parameters are checked before anything else: each gives MGX_E_INVALID and a message that names it"""
    import mini_amd
    lib = mini_amd.lib
    a = dict(fanouts=[3, 2], count=1)
    a.update(args)
    fo = None if a["fanouts"] is None else np.array(a["fanouts"] + [0] * 20, dtype=np.int32)
    hops = a.get("hops", 0 if fo is None else len(a["fanouts"]))
    seeds = np.zeros(4, dtype=np.int32)
    for go in (lib.mgx_nsample_run, lib.mgx_nsample_enact):
        status = go(None, seeds.ctypes.data_as(C.c_void_p), a["count"], None if fo is None else fo.ctypes.data_as(C.c_void_p), hops, 0, 1, None)
        assert status == mini_amd.MGX_E_INVALID
        assert word.encode() in lib.mgx_last_error(), lib.mgx_last_error()


def test_nsample_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names


def test_nsample_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the seven kernels of the fused path and the operator path's two functors use
    no scratch and spill nothing"""
    path = os.path.join(ROOT, "mini_amd", "kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resource remarks"
    cur, res = None, {}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key, pat in (("scratch", r"ScratchSize[^:]*: (\d+)"), ("vspill", r"VGPRs Spill[^:]*: (\d+)"),
                         ("sspill", r"SGPRs Spill[^:]*: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                res.setdefault(cur, {})[key] = int(m.group(1))
    for parts in KERNELS:
        found = [k for k in res if all(x in k for x in parts)]
        assert found, parts
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


# ---- the model's properties ----
def _consistent(r, ro, ci, seeds, fanouts, replace):
    """rows, picks and ids are what the definition says, and the arrays agree with each other"""
    ro, ci = np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n, H = len(ro) - 1, len(fanouts)
    V, off, rows, cols, pos = (r[k].astype(np.int64) for k in ("vertices", "hop_offsets", "row_offsets", "cols", "entry_pos"))
    assert len(off) == H + 2 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(V)
    assert len(np.unique(V)) == len(V)                                          # no vertex has two local ids
    sd = np.arange(n) if seeds is None else np.asarray(seeds, dtype=np.int64)
    assert np.array_equal(V[:off[1]], np.unique(sd)) and np.array_equal(V[r["seed_local"]], sd)
    for h in range(H + 1):
        part = V[off[h]:off[h + 1]]
        assert (np.diff(part) > 0).all()                                        # ascending, and so disjoint from the earlier hops
    R = off[H]
    assert len(rows) == R + 1 and rows[0] == 0 and rows[-1] == len(cols) == len(pos)
    assert np.array_equal(ci[pos], V[cols])
    deg = np.diff(ro)
    for h, k in enumerate(fanouts):
        for row in range(off[h], off[h + 1]):
            v, p = V[row], pos[rows[row]:rows[row + 1]] - ro[V[row]]
            d = deg[v]
            assert ((p >= 0) & (p < d)).all()
            if k < 0 or (not replace and d <= k):
                assert np.array_equal(p, np.arange(d))                          # whole, in stored order
            elif replace:
                assert len(p) == (k if d else 0)
            else:
                assert len(p) == k and len(np.unique(p)) == k                   # distinct
        new = V[off[h + 1]:off[h + 2]]
        dst = V[cols[rows[off[h]]:rows[off[h + 1]]]]
        assert np.array_equal(new, np.setdiff1d(dst, V[:off[h + 1]]))
    s = r["stats"]
    assert (s["seeds"], s["unique_seeds"], s["hops"], s["vertices"], s["rows"], s["edges"]) == (len(sd), off[1], H, len(V), R, len(cols))
    assert s["empty_rows"] + s["whole_rows"] + s["sampled_rows"] == R
    assert s["revisits"] == sum(int((cols[rows[off[h]]:rows[off[h + 1]]] < off[h + 1]).sum()) for h in range(H))


@pytest.mark.parametrize("fanouts", [[3], [4, 2], [-1, 2], [2, -1, 1], [15, 10, 5], []])
@pytest.mark.parametrize("replace", [False, True])
def test_rows_picks_and_ids_follow_the_definition(fanouts, replace):
    ro, ci = cases.random_digraph(400, 3000, 3)
    seeds = np.array([7, 7, 399, 0, 120, 64, 7])
    r = model.sample(ro, ci, seeds, fanouts, replace, seed=5)
    _consistent(r, ro, ci, seeds, fanouts, replace)
    again = model.sample(ro, ci, seeds, fanouts, replace, seed=5)
    other = model.sample(ro, ci, seeds, fanouts, replace, seed=6)
    assert all(np.array_equal(again[k], r[k]) for k in model.ARRAYS) and again["stats"] == r["stats"]
    if fanouts and max(fanouts) > 0:
        assert not np.array_equal(other["entry_pos"], r["entry_pos"])
    _consistent(model.sample(ro, ci, None, fanouts[:2], replace, seed=5), ro, ci, None, fanouts[:2], replace)
    _consistent(model.sample(*cases.loops_and_duplicates(), [0, 5], [4, 4], replace, seed=1), *cases.loops_and_duplicates(), [0, 5], [4, 4], replace)


def test_a_vertex_does_not_depend_on_the_batch():
    """a vertex's sampled entries are a function of the graph, the seed, the hop and the vertex: adding seeds changes them only where
    it changes the hop that reaches the vertex"""
    ro, ci = cases.random_digraph(500, 5000, 9)
    few = model.sample(ro, ci, [3, 11], [4, 3], seed=2)
    more = model.sample(ro, ci, [3, 11, 200, 201, 202], [4, 3], seed=2)

    def rows_of(r):
        out = {}
        for h in range(2):
            for row in range(r["hop_offsets"][h], r["hop_offsets"][h + 1]):
                out[(h, int(r["vertices"][row]))] = r["entry_pos"][r["row_offsets"][row]:r["row_offsets"][row + 1]].tolist()
        return out
    a, b = rows_of(few), rows_of(more)
    shared = set(a) & set(b)
    assert len(shared) >= 4 and all(a[key] == b[key] for key in shared)


def test_all_entries_at_every_hop_is_the_bfs_ball():
    ro, ci = cases.random_digraph(600, 1500, 4)
    H, src = 3, [5, 17]
    r = model.sample(ro, ci, src, [-1] * H, seed=1)
    depth = np.full(600, -1)
    depth[src] = 0
    front = np.array(src)
    for h in range(H):
        nxt = np.unique(np.concatenate([ci[ro[v]:ro[v + 1]] for v in front] + [np.zeros(0, dtype=ci.dtype)]))
        nxt = nxt[depth[nxt] < 0]
        depth[nxt] = h + 1
        front = nxt
    off = r["hop_offsets"]
    for h in range(H + 1):
        assert np.array_equal(r["vertices"][off[h]:off[h + 1]], np.flatnonzero(depth == h))
    inner = np.flatnonzero((depth >= 0) & (depth < H))
    assert r["stats"]["edges"] == int(np.diff(ro)[inner].sum()) and r["stats"]["draws"] == 0 and r["stats"]["sampled_rows"] == 0
    assert np.array_equal(np.sort(r["entry_pos"]), np.sort(np.concatenate([np.arange(ro[v], ro[v + 1]) for v in inner])))


def test_revisits_and_one_local_id():
    r = model.sample(*cases.reached_twice(), [0], [-1, -1, -1])
    assert r["vertices"].tolist() == [0, 1, 2, 3] and r["hop_offsets"].tolist() == [0, 1, 3, 4, 4]
    assert r["row_offsets"].tolist() == [0, 2, 4, 5, 5] and r["cols"].tolist() == [1, 2, 2, 3, 3]
    assert r["stats"]["revisits"] == 1 and r["stats"]["empty_rows"] == 1 and r["stats"]["edges"] == 5     # 1 -> 2 finds 2 numbered; 3 has no entries


def test_bounds_and_counts():
    assert model.bounds(100, 1000, 10, [5, -1, 3], False) == ([10, 50, 100, 100], [50, 1000, 300])
    assert model.bounds(100, 40, 10, [5, 5], False) == ([10, 40, 40], [40, 40])
    assert model.bounds(100, 40, 10, [5, 5], True) == ([10, 50, 100], [50, 250])
    assert model.fused_counts(10, 3, 2, True) == (14, 2) and model.fused_counts(10, 10, 0, False) == (4, 1)
    assert model.fused_counts(0, 0, 3, False) == (0, 0) and model.fused_counts(10, 0, 3, True) == (0, 0)


# ---- the distribution Floyd's algorithm samples over the project's draws ----
def _inclusion(picks, d, k):
    S = len(picks)
    assert ((picks >= 0) & (picks < d)).all()
    assert (np.diff(np.sort(picks, axis=1), axis=1) > 0).all()                  # every pick set distinct
    counts = np.bincount(picks.ravel(), minlength=d)
    p = k / d
    dev = np.abs(counts - S * p) / np.sqrt(S * p * (1.0 - p))
    assert dev.max() <= 5.0, (d, k, float(dev.max()))


@pytest.mark.parametrize("d, k", cases.UNIFORM_PAIRS)
def test_floyd_over_the_draws_is_uniform(d, k):
    """every position's inclusion count over 4096 seeds (one vertex), and over 4096 vertices (one seed), within 5 standard
    deviations of Binomial(4096, k / d): 3.7 and 2.8 were measured.  The inputs are fixed, so the test is deterministic."""
    S = 4096
    keys = np.concatenate([model.row_keys(s, [0], 0) for s in range(S)])
    _inclusion(model.floyd(keys, np.full(S, d), k)[0], d, k)
    _inclusion(model.floyd(model.row_keys(1, np.arange(S), 0), np.full(S, d), k)[0], d, k)
