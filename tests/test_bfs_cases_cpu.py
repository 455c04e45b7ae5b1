"""The proof, without a GPU, that the inputs of tests/test_gpu_bfs_paths.py sit on their edges: every graph of tests/bfs_cases.py
has the labels its construction says (two independent searches agree), its levels have the promised shapes, and the device's rules
as tests/bfs_model.py mirrors them put the two members of an edge pair on different sides in exactly the one level the pair is about."""
import numpy as np
import pytest

from tests import bfs_cases as bc
from tests import bfs_model as bm

PAIRS = sorted(k for k, v in bc.CASES.items() if v["pair"])
# (the big stars and the deep paths are built once each here: their second id assignment and their variants change switches only)
CPU_CASES = sorted(k for k in bc.CASES if not (k.startswith("star_") and k.count("_") > 1 and not k.startswith("star_behind"))
                   and k not in ("fan_hot0", "fan_vshort", "fan_novshort"))
FIXED = [k for k in CPU_CASES if not bc.CASES[k]["adaptive"]]
RULE_OF = {"small_levels": lambda r: r[0].startswith("chain"), "mini_slots": lambda r: r[0] == "mini",
           "dense_slots": lambda r: r[0] == "slot" and r[1], "vshort_slots": lambda r: r[0] == "slot" and r[2],
           "lazy_slots": lambda r: r[0] == "slot" and r[4], "push_levels": lambda r: not (r[0] == "slot" and r[6])}


def test_constants_are_what_the_cases_were_built_for():
    assert bm.constants() == bm.EXPECTED
    assert bc.HOT_N == 32 * bm.K["BFS_DENSE_HOTW"] == 32 * bm.K["BFS_COLD_WORDS"]
    # the three LDS prefixes the star cases straddle all lie inside the stars
    assert max(bm.K["BFS_WAVE_HOTW"], bm.K["BFS_DENSE_HOTW"], bm.K["BFS_STREAM_HOTW2"]) * 32 < 700001 and 700001 % 32 == 1


@pytest.mark.parametrize("name", CPU_CASES)
def test_labels_are_a_breadth_first_search(oracle, name):
    case = bc.CASES[name]
    for member in case["members"]:
        for ids in case["ids"]:
            g = case["graph"](member, ids)
            assert g.in_neighbour_ok(), (name, member, ids)
            assert np.array_equal(g.labels, oracle.bfs_cpu(g.ro, g.ci, g.src)), (name, member, ids)
            assert np.array_equal(g.labels, bc.numpy_bfs(g.ro, g.ci, g.src)), (name, member, ids)
            assert int((g.labels >= 0).sum()) == g.reachable


def _value(g, shapes, level, what):
    s = shapes[level]
    if what == "late":
        return 4 * (1 + sum(x[5] for x in shapes[:level])) - g.n
    return {"nf": s[0] + s[1], "E": s[2] + s[3], "nf_s": s[0], "nf_l": s[1], "E_s": s[2], "E_l": s[3], "units": s[4], "kids": s[5]}[what]


@pytest.mark.parametrize("name", sorted(bc.PROMISE))
def test_levels_have_the_promised_shapes(name):
    case = bc.CASES[name]
    for member, promises in bc.PROMISE[name].items():
        for ids in case["ids"]:
            g = case["graph"](member, ids)
            shapes = g.shapes(bm.Config(case["env"], g.n, False).long_min)
            for level, what, value in promises:
                assert _value(g, shapes, level, what) == value, (name, member, level, what)
            # the shapes are the graph's: rows and entries by label, counted from the CSR
            for k, s in enumerate(shapes):
                at = g.labels == k
                assert s[0] + s[1] == int((g.deg[at] > 0).sum()) and s[2] + s[3] == int(g.deg[at].sum())
                assert s[5] == (int((g.labels == k + 1).sum()))


def test_every_pair_has_a_promise():
    assert sorted(bc.PROMISE) == PAIRS


@pytest.mark.parametrize("name", PAIRS)
def test_pair_members_differ_in_exactly_one_level(name):
    case = bc.CASES[name]
    level, counter = case["pair"][:2]
    delta = case["pair"][2] if len(case["pair"]) > 2 else 1
    for layout in case["layouts"]:
        got = {}
        for member in ("at", "beyond"):
            g = case["graph"](member, "spec")
            cfg = bm.config_for(case["env"], g, layout, case["mode"], case["alpha"])
            shapes = g.shapes(cfg.long_min)
            got[member] = bm.predict(cfg, shapes, g.tree)
        (ca, ra), (cb, rb) = got["at"], got["beyond"]
        rule = RULE_OF[counter]
        assert len(ra) == len(rb)
        differ = [k for k in range(len(ra)) if rule(ra[k]) != rule(rb[k])]
        assert differ == [level], (name, layout, differ)
        assert rule(ra[level]) and not rule(rb[level])
        assert ca[counter] == cb[counter] + delta, (name, layout, ca, cb)
        assert ca["levels"] == cb["levels"]


@pytest.mark.parametrize("name", FIXED)
def test_the_launch_sequence_decides_no_counter(name):
    """predict() walks the launches for every number of slots a handle may have learnt and both launch plans of a source's class, and
    raises when a counter depends on it"""
    case = bc.CASES[name]
    for layout in case["layouts"]:
        for member in case["members"]:
            g = case["graph"](member, case["ids"][0])
            cfg = bm.config_for(case["env"], g, layout, case["mode"], case["alpha"], cold_pairs=bm.star_cold_pairs(g) if name.startswith("star") else 0)
            shapes = g.shapes(cfg.long_min)
            c, ran = bm.predict(cfg, shapes, g.tree)
            assert c["reached"] == g.reachable and c["m_t"] == int(g.deg[g.labels >= 0].sum())
            assert c["levels"] == len(ran) == len(bm.trace(shapes)) or c["levels"] > bm.K["BFS_MAX_TRACE"]


def test_the_forced_bodies_are_predicted():
    """spot checks of the walk against what the cases' docstrings say"""
    def run(name, member, layout):
        case = bc.CASES[name]
        g = case["graph"](member, "spec")
        cfg = bm.config_for(case["env"], g, layout, case["mode"], case["alpha"], cold_pairs=bm.star_cold_pairs(g) if name.startswith("star") else 0)
        shapes = g.shapes(cfg.long_min)
        return bm.predict(cfg, shapes, g.tree)
    c, ran = run("chain_three_then_not", "at", False)
    assert [r[0] for r in ran] == ["chain", "chain", "chain", "slot"] and c["small_levels"] == 3
    c, ran = run("mini_behind_lazy", "at", True)
    assert c["mini_slots"] == 0 and c["lazy_slots"] == 1 and c["dense_slots"] == 2 and c["vshort_slots"] == 1
    c, ran = run("lazy_always", "at", True)
    assert c["lazy_slots"] == 3 and c["levels"] == 4
    c, ran = run("lazy_edge", "at", True)
    assert (c["lazy_slots"], c["dense_slots"], c["vshort_slots"]) == (1, 2, 1)
    c, ran = run("lazy_edge", "beyond", True)
    assert (c["lazy_slots"], c["dense_slots"], c["vshort_slots"]) == (0, 1, 1)
    for n, cold in ((bc.HOT_N, 0), (bc.HOT_N + 1, 1), (700001, 1)):
        c, ran = run("star_%d" % n, "at", True)
        assert (c["dense_slots"], c["cold_slots"], c["levels"]) == (1, cold, 1)
        assert run("star_%d_nocold" % n, "at", True)[0]["cold_slots"] == 0
        assert run("star_%d" % n, "at", False)[0]["dense_slots"] == 0
    c, ran = run("star_behind_lazy", "cold", True)
    assert (c["lazy_slots"], c["dense_slots"], c["vshort_slots"], c["cold_slots"]) == (2, 1, 2, 1)
    c, ran = run("path_5000_wide", "at", False)
    assert c["levels"] == 5000 and c["small_levels"] == 0
    c, ran = run("path_5000_chained", "at", False)
    assert c["levels"] == 5000 and c["small_levels"] == 5000


def test_short_rows_of_an_m_launch_stand_on_their_edge():
    """mini_short_rows, the one case the launch sequence decides: level 2 holds 65536 / 65537 short rows and is late and mid-size by
    its entries in both members; `at` is an M launch's in some of the sequences a handle may enqueue, `beyond` in none"""
    case = bc.CASES["mini_short_rows"]
    for layout in case["layouts"]:
        seen = {}
        for member in case["members"]:
            g = case["graph"](member, "spec")
            cfg = bm.config_for(case["env"], g, layout)
            shapes = g.shapes(cfg.long_min)
            assert shapes[2][0] == (bm.K["BFS_MINI_SHORT_ROWS"] if member == "at" else bm.K["BFS_MINI_SHORT_ROWS"] + 1) and shapes[2][1] == 0
            assert shapes[2][2] <= bm.K["BFS_MINI_EDGES_LATE"] and 4 * (1 + shapes[1][5]) >= g.n       # (level 0's discoveries are an M launch's)
            seen[member] = bm.outcomes(cfg, shapes, g.tree)
            for c, ran in seen[member]:
                assert ran[0] == ("mini",) and ran[1][0] == "slot" and c["levels"] == 3 and c["reached"] == g.reachable
        assert sorted({ran[2][0] for _, ran in seen["at"]}) == ["mini", "slot"]
        assert {ran[2][0] for _, ran in seen["beyond"]} == {"slot"} and len(seen["beyond"]) == 1


@pytest.mark.parametrize("name,long_min", [("vs_classes_17", 17), ("vs_classes_32", 32), ("vs_classes_64", 64)])
def test_lane_class_rows_stand_either_side_of_every_cut(name, long_min):
    """the layout sorts by degree, so its class boundaries (cut_degree_classes) follow from the degrees: every cut -- long_min, 17, 9,
    5, 1 -- has rows of the degree just above it and just below it on its two sides"""
    g = bc.CASES[name]["graph"]("at", "spec")
    deg = np.sort(g.deg)[::-1]
    (b0, b1, b2, b3), b9 = bm.vs_classes(deg, long_min)
    for cut, at in ((long_min, b0), (17, b1), (9, b9), (5, b2), (1, b3)):
        assert deg[at - 1] >= cut > deg[at]
        if cut <= long_min:
            assert deg[at - 1] == cut and deg[at] == cut - 1, (name, cut)
    assert b3 - b2 >= 128 and b2 - b9 >= 128 and b9 - b1 >= 128 and (b1 - b0 >= 128 or long_min == 17)     # more than one wave step a class
