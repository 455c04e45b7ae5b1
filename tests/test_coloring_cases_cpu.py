"""CPU suite for the colouring's path cases (tests/coloring_cases.py): by the numpy model alone (tests/coloring_model.py), every
case has the property it exists for at the thresholds of include/mgx/color_fused.hpp, which the case module holds by value.  The
GPU suite (tests/test_gpu_coloring_paths.py) runs the same cases with the thresholds the library reports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import coloring_cases as cases
from tests import coloring_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", "mgx", name)).read()


def test_the_case_module_holds_the_headers_thresholds():
    text = _header("color_fused.hpp")
    const = {k: int(v) for k, v in re.findall(r"constexpr int (COLOR_\w+) = (\d+);", text)}
    assert const["COLOR_SEG"] == cases.SEG and const["COLOR_LONG_MIN"] == cases.LONG_MIN
    assert const["COLOR_BATCH_MAX"] == cases.BATCH_MAX
    wave = int(re.search(r"constexpr int WAVE = (\d+);", _header("wave.hpp")).group(1))
    assert re.search(r"constexpr int COLOR_STAGE = 2 \* WAVE;", text) and 2 * wave == cases.STAGE
    assert re.search(r"std::max<long long>\(i, %d\)" % cases.FIRST_BATCH, text), "the first batch's rounds"


def test_library_exports_the_report_and_the_grid_switch(built):
    import mini_amd
    lib = mini_amd.lib
    assert hasattr(mini_amd.ColorProblem, "info")
    consts, rounds = (C.c_int64 * 4)(), C.c_int()
    assert lib.mgx_color_info(None, consts, None, 0, C.byref(rounds)) == mini_amd.MGX_E_INVALID
    names = set()
    name, what = C.c_char_p(), C.c_char_p()
    for i in range(lib.mgx_env_switches(-1, None, None)):
        lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        names.add(name.value.decode())
    assert "MGX_GRID_CUS" in names


def _consistent(ro, want):
    """the predicted row classes add up to the model's active counts"""
    colours, trace, _ = want
    rows = cases.round_rows(ro, colours, len(trace))
    assert np.array_equal(rows[:, 0] + rows[:, 2], trace)
    assert (rows[:, 1] >= rows[:, 2]).all()
    return rows


@pytest.mark.parametrize("tail", cases.EDGE_TAILS)
def test_degree_edges(tail):
    n = 128 * 3 + tail
    ro, ci, by_degree = cases.degree_edges(n)
    deg = np.diff(ro)
    assert sorted(by_degree) == sorted(cases.edge_degrees()) == [0, 1, 31, 32, 33, 2047, 2048, 2049, 4096, 4097]
    want = model.color(ro, ci, model.SEED, 0)
    colours = want[0]
    for d, rows in by_degree.items():
        assert (deg[rows] == d).all() and len(rows) >= 3
        if d >= 1:
            assert (colours[rows] <= 2).any(), "degree %d: no row decided in round 0" % d
        if d >= 2:                                           # (a row of one entry is always decided: its one neighbour is on one side)
            assert (colours[rows] > 2).any(), "degree %d: no row survives round 0" % d
    assert {1, 2} <= set(colours[by_degree[2 * cases.SEG + 1]].tolist())      # a split row decided either way at its first look
    # split rows that survive several rounds: the tally is used, and cleared, round after round
    assert (colours[by_degree[cases.SEG + 1] + by_degree[2 * cases.SEG + 1]] > 6).any()
    assert colours[n - 1] > 2, "vertex n - 1 (the bitmap's last word) is decided in round 0"
    assert n % 128 == tail and (n % 32 != 0)
    rows = _consistent(ro, want)
    assert len(rows) > cases.FIRST_BATCH + 1, "the run ends inside the first batch of rounds"
    for max_iter in (1, cases.FIRST_BATCH, cases.FIRST_BATCH + 1, len(rows), len(rows) + 1):
        got, stopped = cases.truncated(want, max_iter), model.color(ro, ci, model.SEED, max_iter)
        assert np.array_equal(got[0], stopped[0]) and np.array_equal(got[1], stopped[1]) and got[2] == stopped[2]


@pytest.fixture(scope="module")
def hub_clique():
    ro, ci, hubs = cases.hub_clique(cases.HUB_CLIQUE_H, cases.hub_clique_leaves(cases.HUB_CLIQUE_H))
    return ro, ci, hubs


def test_hub_clique(hub_clique):
    ro, ci, hubs = hub_clique
    assert len(ro) - 1 == 144024 and len(ci) == 288552
    found = cases.hub_clique_seed(ro, ci, hubs)
    assert found is not None, "no seed of HUB_CLIQUE_SEEDS gives the hub clique its property"
    seed, want = found
    colours = want[0]
    deg = np.diff(ro)[hubs]
    assert ((deg + cases.SEG - 1) // cases.SEG == 3).all()
    # rows of three segments start FIRST_BATCH + 1 rounds and more uncoloured
    assert (colours[hubs] > 2 * (cases.FIRST_BATCH + 1)).any()
    disjoint, both = cases.split_rows(ro, ci, colours, seed, hubs)
    assert disjoint and all(i >= 1 for i, _ in disjoint)
    for i, v in disjoint:
        below, above = cases.segment_views(ro, ci, colours, seed, i, v)
        assert below and above and not (below & above)
        assert colours[v] > 2 * i + 2                        # the row survives that round, and only the whole tally says so
    assert both
    _consistent(ro, want)


def test_the_seed_matters_for_the_hub_clique(hub_clique):
    """under seed 5 no row ever has its two kinds of neighbours in different segments only: the property is not a given"""
    ro, ci, hubs = hub_clique
    colours = model.color(ro, ci, 5, 0)[0]
    assert not cases.hub_clique_holds(ro, ci, hubs, colours, 5)
    assert cases.hub_clique_seed(ro, ci, hubs, seeds=(5,)) is None


def _hubs_survive_round_0(lengths, segs_want):
    ro, ci = cases.shared_leaf_hubs(lengths)
    assert len(ci) <= 10_000_000
    hubs = len(lengths)
    deg = np.diff(ro)[:hubs]
    assert ((deg + cases.SEG - 1) // cases.SEG).tolist() == list(segs_want)
    want = model.color(ro, ci, model.SEED, 0)
    colours, trace, left = want
    assert (colours[:hubs] == 3).all() and (colours[hubs:] == 1).all() and left == 0
    rows = _consistent(ro, want)
    assert rows.tolist() == [[len(ro) - 1 - hubs, sum(segs_want), hubs], [0, sum(segs_want), hubs]]


def test_hubs_beyond_the_stage():
    lengths = cases.beyond_stage_lengths()
    assert lengths[:2] == (cases.STAGE * cases.SEG, cases.STAGE * cases.SEG + 1) == (262144, 262145)
    _hubs_survive_round_0(lengths, (cases.STAGE, cases.STAGE + 1, 154))


def test_late_evidence():
    """eight hubs of 43 segments that colour each other over several rounds from entries in their last segment alone: a segment
    that gave up because another had already reported would lose the row its evidence"""
    lengths = cases.stage_pressure_lengths(rows=cases.LATE_EVIDENCE_ROWS)
    hubs = len(lengths)
    ro, ci = cases.shared_leaf_hubs(lengths, clique=True)
    segs = (np.diff(ro)[:hubs] + cases.SEG - 1) // cases.SEG
    assert (segs == cases.STAGE // 3 + 1).all() and (segs > cases.ONE_UNIT_WAVES).all()
    wave = int(re.search(r"constexpr int WAVE = (\d+);", _header("wave.hpp")).group(1))
    block = int(re.search(r"constexpr int BLOCK = (\d+);", _header("wave.hpp")).group(1))
    assert cases.ONE_UNIT_WAVES == 8 * block // wave
    want = model.color(ro, ci, model.SEED, 0)
    colours, trace, left = want
    assert left == 0 and (colours[:hubs] > 2).all() and len(trace) == 1 + hubs // 2
    seen = 0
    for i in range(1, len(trace)):
        for v in np.nonzero(cases.uncoloured_at(colours, i)[:hubs])[0]:
            below, above = cases.segment_views(ro, ci, colours, model.SEED, i, int(v))
            assert (below | above) <= {int(segs[v]) - 1}     # the last segment alone
            seen += bool(below and above)
    assert seen >= hubs                                      # rows that survive on that segment's word, round after round
    _consistent(ro, want)


def test_stage_pressure():
    lengths = cases.stage_pressure_lengths()
    segs = cases.STAGE // 3 + 1
    assert len(lengths) == 96 and segs == 43
    assert 2 * segs <= cases.STAGE < 3 * segs                # a wave's third surviving row flushes its stage
    _hubs_survive_round_0(lengths, (segs,) * 96)


def _verdict(below, above):
    return "survives" if below and above else "coloured"


def test_hub_clique_tells_the_combined_tally_from_one_segments_view(hub_clique):
    """a last-arriving wave that kept its own segment's view instead of the tally's would colour every row whose two kinds of
    neighbours lie in different segments only -- whichever segment arrives last -- where the model lets it survive"""
    ro, ci, hubs = hub_clique
    seed, want = cases.hub_clique_seed(ro, ci, hubs)
    disjoint, _ = cases.split_rows(ro, ci, want[0], seed, hubs)
    for i, v in disjoint:
        below, above = cases.segment_views(ro, ci, want[0], seed, i, v)
        assert _verdict(below, above) == "survives"
        for last in range(3):
            assert _verdict(last in below, last in above) == "coloured"


def test_late_evidence_tells_an_early_exit_on_arrivals_alone():
    """on a grid of ONE_UNIT_WAVES waves, item j and item j + ONE_UNIT_WAVES go to the same wave in that order; a wave that skipped a
    segment because the row's tally was non-zero would skip every segment from ONE_UNIT_WAVES on -- the last one with it, which
    holds all the evidence: every surviving hub would be coloured"""
    lengths = cases.stage_pressure_lengths(rows=cases.LATE_EVIDENCE_ROWS)
    hubs = len(lengths)
    ro, ci = cases.shared_leaf_hubs(lengths, clique=True)
    colours = model.color(ro, ci, model.SEED, 0)[0]
    wrong = 0
    for i in range(1, hubs // 2):
        for v in np.nonzero(cases.uncoloured_at(colours, i + 1)[:hubs])[0]:      # survives round i
            below, above = cases.segment_views(ro, ci, colours, model.SEED, i, int(v))
            scanned = set(range(cases.ONE_UNIT_WAVES))
            assert _verdict(below, above) == "survives" and _verdict(below & scanned, above & scanned) == "coloured"
            wrong += 1
    assert wrong >= hubs
