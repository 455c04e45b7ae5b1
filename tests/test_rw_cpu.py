"""CPU suite for the random walks (mgx_rw_*, include/mgx/rw_fused.hpp, include/gunrock/rw/): the header declares and the library
exports them, NULL handles, NULL outputs and invalid parameters are statuses, the switches are in the table, the walk kernels keep
their registers, and the model the GPU tests compare against (tests/rw_model.py) has the properties of the definition and samples
the intended distributions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import rw_cases as cases
from tests import rw_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_rw_create", "mgx_rw_free", "mgx_rw_run", "mgx_rw_enact", "mgx_rw_paths", "mgx_rw_paths_device", "mgx_rw_ends", "mgx_rw_lengths",
         "mgx_rw_visits", "mgx_rw_visits_device", "mgx_rw_bins", "mgx_rw_set_timing", "mgx_rw_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_rw_walkILb%dELb%dE" % (w, s),) for w in (0, 1) for s in (0, 1)]
KERNELS += [("2rw", "step_functor_tILb%dELb%dE" % (w, s)) for w in (0, 1) for s in (0, 1)]
KERNELS += [("k_rw_setupE",), ("k_rw_setup_long",)]
SWITCHES = {"MGX_RW_TRIES", "MGX_RW_TILE", "MGX_RW_SHORT_MAX", "MGX_RW_WAVE_MAX", "MGX_RW_SEG"}


def test_header_declares_and_library_exports_rw(built):
    import mini_amd
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    for name in NAMES:
        assert re.search(r"MGX_API int %s\(" % name, header), name
        assert hasattr(mini_amd.lib, name), name
    rp = mini_amd.RandomWalkProblem
    assert rp.KEYS == model.STAT_KEYS + ("launches", "host_waits")
    for member in ("run", "enact", "paths", "ends", "lengths", "visits", "ppr", "paths_device_ptr", "visits_device_ptr", "bins", "set_timing",
                   "phase_ms", "close"):
        assert hasattr(rp, member), member
    for word in ("STORED order", "2^-32", "fallback", "OUT-entries"):
        assert word in rp.__doc__, word


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, d = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_rw_create(None, C.byref(h)) == bad
    for go in (lib.mgx_rw_run, lib.mgx_rw_enact):
        assert go(None, None, 0, 1, 10, 1, 0, 1.0, 1.0, 0.0, 1, 0, st) == bad
        assert b"NULL" in lib.mgx_last_error()
    for fn in (lib.mgx_rw_paths, lib.mgx_rw_ends, lib.mgx_rw_lengths, lib.mgx_rw_visits, lib.mgx_rw_bins, lib.mgx_rw_phase_ms):
        assert fn(None, None) == bad
    assert lib.mgx_rw_paths_device(None, C.byref(d)) == bad and lib.mgx_rw_visits_device(None, C.byref(d)) == bad
    assert lib.mgx_rw_set_timing(None, 1) == bad
    assert lib.mgx_rw_free(None) == 0


@pytest.mark.parametrize("args, word", [
    (dict(length=-1), "length"), (dict(walks=0), "walks_per_start"), (dict(p=0.0), "p and q"), (dict(p=-1.0), "p and q"),
    (dict(q=0.0), "p and q"), (dict(q=float("inf")), "p and q"), (dict(p=float("nan")), "p and q"), (dict(restart=1.0), "restart"),
    (dict(restart=-0.5), "restart"), (dict(restart=float("nan")), "restart")])
def test_invalid_parameters_are_statuses(built, args, word):
    """the parameters are checked before anything else: each gives MGX_E_INVALID and a message that names it"""
    import mini_amd
    lib = mini_amd.lib
    a = dict(length=10, walks=1, p=1.0, q=1.0, restart=0.0)
    a.update(args)
    for go in (lib.mgx_rw_run, lib.mgx_rw_enact):
        assert go(None, None, 0, a["walks"], a["length"], 1, 0, a["p"], a["q"], a["restart"], 1, 0, None) == mini_amd.MGX_E_INVALID
        assert word.encode() in lib.mgx_last_error(), lib.mgx_last_error()


def test_rw_switches_are_in_the_table(built):
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    names = set()
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert SWITCHES <= names


def test_rw_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the four instantiations of the walk kernel, the operator path's step functors
    and the setup use no scratch and spill nothing"""
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
def _entries(ro, ci):
    n = len(ro) - 1
    return set((np.repeat(np.arange(n), np.diff(ro)) * n + np.asarray(ci, dtype=np.int64)).tolist())


def _consistent(r, ro, ci, starts, R):
    """the pairs of every path are stored entries or counted restarts; lengths, ends, visits and stats are what the paths say"""
    n = len(ro) - 1
    P = r["paths"].astype(np.int64)
    W, L1 = P.shape
    start = np.repeat(np.arange(n) if starts is None else np.asarray(starts), R)
    assert np.array_equal(P[:, 0], start)
    live = P >= 0
    assert (live[:, :-1] | ~live[:, 1:]).all()                                  # -1 only behind the end
    a, b = P[:, :-1][live[:, 1:]], P[:, 1:][live[:, 1:]]
    stored = np.isin(a * n + b, np.fromiter(_entries(ro, ci), dtype=np.int64)) if len(ci) else np.zeros(len(a), dtype=bool)
    home = np.broadcast_to(start[:, None], (W, L1 - 1))[live[:, 1:]]
    assert (stored | (b == home)).all()
    assert (~stored).sum() <= r["stats"]["restarts"]
    assert np.array_equal(r["lengths"], live[:, 1:].sum(axis=1))
    assert np.array_equal(r["ends"], P[np.arange(W), r["lengths"]])
    assert np.array_equal(r["visits"], np.bincount(P[live], minlength=n))
    s = r["stats"]
    assert s["walkers"] == W and s["length"] == L1 - 1 and s["steps"] == int(live[:, 1:].sum())
    assert s["dead_ends"] == int((r["lengths"] < L1 - 1).sum()) and s["tries"] >= s["steps"] - s["restarts"]


MODES = [dict(), dict(weighted=True), dict(p=0.5, q=2.0), dict(weighted=True, p=4.0, q=0.25), dict(restart=0.15),
         dict(weighted=True, p=0.5, q=2.0, restart=0.15)]


@pytest.mark.parametrize("mode", MODES)
def test_paths_follow_entries_and_results_follow_paths(mode):
    ro, ci = cases.with_isolated(*cases.random_digraph(300, 1200, 3), 5)
    w = cases.weights(ci, 4, zeros=0.1)
    r = model.walk(ro, ci, w, None, length=30, walks_per_start=2, seed=7, **mode)
    _consistent(r, ro, ci, None, 2)
    if not mode.get("restart"):
        assert r["stats"]["restarts"] == 0 and r["stats"]["dead_ends"] > 0
    else:
        assert r["stats"]["restarts"] > 0 and r["stats"]["dead_ends"] == 0 and (r["lengths"] == 30).all()
    again = model.walk(ro, ci, w, None, length=30, walks_per_start=2, seed=7, **mode)
    other = model.walk(ro, ci, w, None, length=30, walks_per_start=2, seed=8, **mode)
    assert np.array_equal(again["paths"], r["paths"]) and again["stats"] == r["stats"]
    assert not np.array_equal(other["paths"], r["paths"])


def test_a_walker_does_not_depend_on_the_others():
    """walker w's path is a function of the graph, the seed, w and its start: not of S, of R, or of who else walks"""
    ro, ci = cases.random_symmetric(200, 800, 5)
    w = cases.weights(ci, 6)
    mode = dict(length=25, seed=3, weighted=True, p=0.5, q=2.0, restart=0.1)
    everyone = model.walk(ro, ci, w, None, **mode)
    few = model.walk(ro, ci, w, np.arange(10), **mode)
    assert np.array_equal(few["paths"], everyone["paths"][:10])
    starts = np.array([5, 9, 100, 5, 17])
    twice = model.walk(ro, ci, w, starts, walks_per_start=2, **mode)
    flat = model.walk(ro, ci, w, np.repeat(starts, 2), walks_per_start=1, **mode)
    assert np.array_equal(twice["paths"], flat["paths"]) and twice["stats"] == flat["stats"]
    assert not np.array_equal(twice["paths"][0], twice["paths"][1])           # (two walkers of one start differ)
    assert model.draw_of(3, 4, 5, 6) == model.draw_of(3, 4, 5, 6) != model.draw_of(3, 4, 5, 7)


def test_unweighted_graph_walks_weighted_as_unweighted():
    ro, ci = cases.random_symmetric(150, 500, 8)
    a = model.walk(ro, ci, None, None, length=20, seed=2)
    b = model.walk(ro, ci, None, None, length=20, seed=2, weighted=True)
    assert np.array_equal(a["paths"], b["paths"]) and b["stats"]["fallbacks"] == 0 and a["stats"]["tries"] == b["stats"]["tries"]


def test_the_end_of_a_path_returns_through_the_fallback():
    """ip = 2^-20: a candidate that is prev is accepted when a < 2^-20 only.  On the path of two vertices every step but a walk's
    first has prev as its only candidate: TRIES rejections, then the fallback takes position 0"""
    W, L = 10, 20
    r = model.walk(*cases.path(2), None, np.zeros(W, dtype=np.int64), length=L, seed=11, p=2.0 ** 20, q=1.0)
    assert (r["paths"] == np.tile(np.arange(L + 1) % 2, (W, 1))).all()
    assert r["stats"]["fallbacks"] == W * (L - 1) and r["stats"]["tries"] == W * (1 + model.TRIES * (L - 1))
    n = 6
    r = model.walk(*cases.path(n), None, None, length=40, walks_per_start=4, seed=12, p=2.0 ** 20, q=1.0)
    P = r["paths"]
    at_end, at_start = P[:, 1:-1] == n - 1, P[:, 1:-1] == 0
    assert at_end.any() and (P[:, 2:][at_end] == n - 2).all() and (P[:, 2:][at_start] == 1).all()
    assert r["stats"]["fallbacks"] == int(at_end.sum() + at_start.sum())
    few = model.walk(*cases.path(2), None, np.zeros(W, dtype=np.int64), length=L, seed=11, p=2.0 ** 20, q=1.0, tries=2)
    assert few["stats"]["tries"] == W * (1 + 2 * (L - 1)) and few["stats"]["fallbacks"] == W * (L - 1)


def test_a_row_of_zero_weights_is_a_dead_end():
    ro, ci, w = cases.one_row([0.0, 0.0, 0.0])
    r = model.walk(ro, ci, w, [0, 0, 1], length=5, weighted=True)
    assert r["lengths"].tolist() == [0, 0, 1] and r["stats"]["dead_ends"] == 3 and (r["paths"][:2, 1:] == -1).all()
    assert r["ends"].tolist() == [0, 0, 0]
    r = model.walk(ro, ci, w, [0], length=5, weighted=True, restart=0.5)       # with restarts it jumps to its start instead
    assert r["lengths"].tolist() == [5] and r["stats"]["restarts"] == 5 and (r["paths"] == 0).all()
    with pytest.raises(ValueError):
        model.walk(ro, ci, -w - 1, [0], length=5, weighted=True)
    r = model.walk(ro, ci, w, [0], length=0, weighted=True)
    assert r["paths"].tolist() == [[0]] and r["stats"]["dead_ends"] == 0


def test_row_maxima_and_order():
    ro, ci, w = cases.one_row([1.0, 8.0, 3.0, 8.0])
    wmax, amax = model.row_maxima(ro, w)
    assert wmax[0] == 8.0 and amax[0] == 1 and (wmax[1:] == 1.0).all() and (amax[1:] == 0).all()
    assert model.rows_ascend(ro, ci) and not model.rows_ascend(*cases.descending(ro, ci))
    assert model.rows_ascend(*cases.empty(5)) and model.rows_ascend(*cases.with_isolated(*cases.star(4), 3))
    r = model.walk(*cases.descending(*cases.random_symmetric(50, 300, 1)), None, None, length=5, p=2.0)
    assert r["stats"]["sorted_copy"] == 1
    assert model.walk(*cases.descending(*cases.random_symmetric(50, 300, 1)), None, None, length=5)["stats"]["sorted_copy"] == 0
    b = model.row_bins(cases.fans(cases.cuts(4, 10, 16))[0], 4, 10, 16)
    assert b["long"] == 8 and b["segments"] == 1 + 1 + 1 + 1 + 2 + 2 + 2 + 3


# ---- the distributions the model samples (the GPU equals the model bit for bit) ----
def _within(counts, probs, N):
    """every count within 5 binomial standard deviations of its expectation: a correct sampler fails a cell with probability < 1e-6"""
    for k, pi in zip(counts, probs):
        assert abs(k - N * pi) <= 5.0 * np.sqrt(N * pi * (1.0 - pi)), (counts, probs, N)


def test_uniform_transitions_from_a_star_and_a_clique():
    N = 50000
    for d in (3, 10, 37):
        r = model.walk(*cases.star(d), None, [0], length=1, walks_per_start=N, seed=d)
        assert r["stats"]["fallbacks"] == 0 and r["stats"]["tries"] == N
        _within(np.bincount(r["paths"][:, 1], minlength=d + 1)[1:], [1.0 / d] * d, N)
    k = 9
    r = model.walk(*cases.complete(k), None, [4], length=1, walks_per_start=N, seed=5)
    counts = np.bincount(r["paths"][:, 1], minlength=k)
    assert r["stats"]["fallbacks"] == 0 and counts[4] == 0
    _within(np.delete(counts, 4), [1.0 / (k - 1)] * (k - 1), N)


def test_weighted_transitions():
    N = 50000
    wts = [1.0, 2.0, 4.0, 8.0]
    ro, ci, w = cases.one_row(wts)
    r = model.walk(ro, ci, w, [0], length=1, walks_per_start=N, seed=21, weighted=True)
    assert r["stats"]["fallbacks"] == 0                                        # (a try accepts with 15 / 32: 64 rejections never happen)
    _within(np.bincount(r["paths"][:, 1], minlength=5)[1:], np.array(wts) / sum(wts), N)
    accept = (sum(wts) / 4) / 8.0                                              # tries are geometric: mean wmax M / mean(w b) = 1 / accept
    assert abs(r["stats"]["tries"] / N - 1.0 / accept) <= 5.0 * np.sqrt((1.0 - accept) / accept ** 2 / N)


@pytest.mark.parametrize("weighted", [False, True])
def test_node2vec_transitions_on_the_triangle_with_a_tail(weighted):
    """p = 0.25, q = 4: from prev = 0 at cur = 2 the walk returns to 0, stays near (1, a neighbour of 0) or moves away (3) as
    ip w : 1 w : iq w"""
    N = 100000
    ro, ci = cases.triangle_with_tail()
    w = None
    wt = {0: 1.0, 1: 1.0, 3: 1.0}
    if weighted:                                   # the row of 2 is (0, 1, 3): weights 2, 1, 1 -- a try accepts with 0.39
        w = np.ones(len(ci), dtype=np.float32)
        w[ro[2]:ro[3]] = [2.0, 1.0, 1.0]
        wt = {0: 2.0, 1: 1.0, 3: 1.0}
    r = model.walk(ro, ci, w, [0], length=2, walks_per_start=N, seed=31, weighted=weighted, p=0.25, q=4.0)
    assert r["stats"]["fallbacks"] == 0
    sel = r["paths"][:, 1] == 2
    n_sel = int(sel.sum())
    assert n_sel > N // 4
    counts = np.bincount(r["paths"][sel, 2], minlength=4)
    assert counts[2] == 0
    mass = np.array([4.0 * wt[0], 1.0 * wt[1], 0.25 * wt[3]])
    _within(counts[[0, 1, 3]], mass / mass.sum(), n_sel)
