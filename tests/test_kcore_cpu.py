"""CPU suite for the fused k-core (mgx_kcore_run, include/mgx/kcore_fused.hpp): the library exports it, refuses NULL arguments, its
kernels keep their registers, and the numpy worklist model the GPU tests compare against (tests/kcore_model.py) computes what
the oracle's restatement of kcore_enactor_t::enact computes -- stranded vertices and the k <= n cap included.  The model's launch
plan (which kind every launch of the fused run is) computes the same again, holds the header's thresholds by value, and on
every case of tests/kcore_cases.py is what the case was built for."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import kcore_cases as cases
from tests import kcore_model as model
from tests.golden_inputs import case_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [c for c in json.load(open(os.path.join(GOLD, "reference_goldens.json")))["cases"] if "kcore_largest" in c]


def test_library_exports_kcore_run(built):
    import mini_amd
    assert hasattr(mini_amd.lib, "mgx_kcore_run")
    assert hasattr(mini_amd.KcoreProblem, "run")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    largest = C.c_int()
    st = (C.c_int64 * 6)()
    assert lib.mgx_kcore_run(None, C.byref(largest), st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_kcore_run(None, None, None) == mini_amd.MGX_E_INVALID
    # (a NULL largest_k_core on a live handle is refused by the same test before any device work: checked on the GPU suite)


def test_kcore_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the k-core kernels use no scratch and spill nothing"""
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
    found = [k for k in res if "k_kcore_" in k]
    assert found, sorted(k for k in res if "kcore" in k)
    for k in found:
        assert res[k].get("scratch", 0) == 0, (k, res[k])
        assert res[k].get("vspill", 0) == 0, (k, res[k])
        assert res[k].get("sspill", 0) == 0, (k, res[k])


def _check(oracle, ro, ci, symmetric=False):
    """the model against the enactor's restatement; on symmetric graphs also against the CPU validator"""
    cores, largest, deg, st = model.decompose(ro, ci)
    ecores, elargest, est = oracle.kcore_enact(ro, ci)
    assert np.array_equal(cores, ecores)
    assert largest == elargest
    assert model.check_against_enactor(st, est), (st, est.tolist())
    assert st["levels"] <= int(est[0])
    assert not ((deg > 0) & (cores > 0)).any()               # whoever left is at 0 or below
    if symmetric:
        want, wlargest = oracle.kcore_cpu(ro, ci)
        assert np.array_equal(cores, want)
        assert wlargest == largest or (len(ci) == 0 and wlargest == 0 and largest == -1)
    return cores, largest, deg, st


def test_model_path3_strands_the_middle(oracle):
    cores, largest, deg, st = _check(oracle, *model.path3(), symmetric=True)
    assert cores.tolist() == [1, 0, 1] and st["stranded"] == 1 and st["removed"] == 2
    assert deg.tolist() == [0, 0, 0] and largest == 1


def test_model_graph_without_entries(oracle):
    cores, largest, deg, st = _check(oracle, *model.no_entries(), symmetric=True)
    assert largest == -1 and not cores.any() and st == dict.fromkeys(model.STAT_NAMES, 0)


def test_model_cap_at_n(oracle):
    ro, ci = model.capped_multigraph()
    assert np.diff(ro).max() >= 6
    cores, largest, deg, st = _check(oracle, ro, ci)
    assert largest == -1 and not cores.any() and np.array_equal(deg, np.diff(ro))
    cores, largest, deg, st = _check(oracle, *model.tripled_clique())
    assert largest == -1 and not cores.any()


def test_model_star_forest(oracle):
    ro, ci = model.star_forest()
    cores, largest, deg, st = _check(oracle, ro, ci, symmetric=True)
    # a hub with two or more leaves falls from its degree to 0 in the one pass its leaves leave in; a hub with one leaf leaves
    # with it (8 of the 50 stars)
    assert st["stranded"] == 42 and st["levels"] == 1 and st["passes"] == 1 and largest == 1


@pytest.mark.parametrize("loop", [False, True])
def test_model_single_vertex(oracle, loop):
    _check(oracle, *model.single(loop), symmetric=True)


def test_model_grid(oracle):
    cores, largest, deg, st = _check(oracle, *model.grid(64, 64), symmetric=True)
    assert st["passes"] >= 63


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_golden_fixtures(oracle, case, tmp_path):
    n, ro, ci, w, _ = oracle.load_mtx(case_path(case, oracle, tmp_path, GOLD), undir=True)
    _check(oracle, ro, ci, symmetric=True)


@pytest.mark.parametrize("seed", range(12))
def test_model_directed_ragged_multigraphs(oracle, seed):
    n = [5, 8, 13, 30, 60, 100, 200, 300, 400, 500, 600, 37][seed]
    _check(oracle, *model.ragged_directed(seed, n))


@pytest.mark.parametrize("seed", range(6))
def test_model_sparse_symmetric_graphs(oracle, seed):
    cores, largest, deg, st = _check(oracle, *model.sparse_symmetric(100 + seed), symmetric=True)
    assert st["stranded"] > 0


@pytest.mark.parametrize("scale,ef,seed", [(10, 16, 10), (12, 8, 12), (14, 4, 14), (16, 16, 16)])
def test_model_rmat(oracle, scale, ef, seed):
    n, ro, ci, w = oracle.rmat_csr(scale, ef, seed)
    _check(oracle, ro, ci, symmetric=True)


# ---- the launch plan ----
def _header_constants():
    """the constexpr ints of include/mgx/kcore_fused.hpp, launch_chain.hpp and wave.hpp by name, products of names and numbers evaluated"""
    vals = {}
    for name in ("wave.hpp", "launch_chain.hpp", "kcore_fused.hpp"):
        text = open(os.path.join(ROOT, "include", "mgx", name)).read()
        for m in re.finditer(r"constexpr int (\w+) = ([^;]+);", text):
            total = 1
            for factor in m.group(2).split("*"):
                factor = factor.strip()
                if factor not in vals and not factor.isdigit():
                    break                                            # (something else than a product: not one of ours)
                total *= int(factor) if factor.isdigit() else vals[factor]
            else:
                vals[m.group(1)] = total
    return vals


def test_plan_constants_are_the_headers(built):
    import mini_amd
    c = _header_constants()
    assert c["KCORE_MINI_MAX"] == model.MINI_MAX == 2048
    assert c["KCORE_LONG_MIN"] == model.LONG_MIN == 32
    assert c["KCORE_SEG"] == model.SEG == 256
    assert (c["CHAIN_BATCH_MIN"], c["CHAIN_BATCH_MAX"]) == (model.BATCH_MIN, model.BATCH_MAX) == (64, 256)
    # what the cases' sizes lean on: the stages flush at 128 short and 64 long rows, a scan covers 256 ids a wave
    assert c["KCORE_STAGE"] == 128 and c["WAVE"] == 64 and c["BLOCK"] == 256
    text = open(os.path.join(ROOT, "include", "mgx", "kcore_fused.hpp")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"KCORE_(\w+) = (\d+)", re.search(r"enum kcore_kind_t[^{]*\{([^}]*)\}", text).group(1)))
    assert enum == {"INIT": 0, "MIN": model.MIN, "LIST": model.LIST, "EXPAND": model.EXPAND, "FILTER": model.FILTER,
                    "DONE": model.IDLE, "MINI": model.MINI}
    assert mini_amd.KcoreProblem.STEP_KINDS == model.KIND_NAMES


def test_plan_batches():
    assert [model.host_waits_and_launches(k) for k in (1, 2, 64, 65, 192, 193, 448, 449, 704, 705)] == \
        [(1, 64), (1, 64), (1, 64), (2, 192), (2, 192), (3, 448), (3, 448), (4, 704), (4, 704), (5, 960)]


def _check_plan(oracle, ro, ci):
    """launch_plan against decompose and against the enactor's restatement"""
    plan = model.launch_plan(ro, ci)
    cores, largest, deg, st = model.decompose(ro, ci)
    assert np.array_equal(plan.cores, cores) and plan.cores.dtype == cores.dtype
    assert plan.largest == largest
    assert np.array_equal(plan.degrees, deg)
    assert plan.stats == st
    ecores, elargest, est = oracle.kcore_enact(ro, ci)
    assert np.array_equal(plan.cores, ecores) and plan.largest == elargest
    assert model.check_against_enactor(plan.stats, est), (plan.stats, est.tolist())
    # the plan's own book-keeping: a working launch of every counted kind, one idle launch, at the end
    assert plan.kinds[0] == model.MIN and plan.kinds[-1] == model.IDLE and plan.kinds.count(model.IDLE) == 1
    assert len(plan.fronts) == st["passes"] == len(plan.lists)
    assert sum(w for _, w, _ in plan.fronts) == st["expanded"]
    assert sum(kind == model.EXPAND for _, _, kind in plan.fronts) == plan.kinds.count(model.EXPAND)
    assert all((w <= model.MINI_MAX) == (kind == model.MINI) for _, w, kind in plan.fronts)
    return plan


MODEL_GRAPHS = {
    "path3": model.path3, "no_entries": model.no_entries, "capped_multigraph": model.capped_multigraph,
    "star_forest": model.star_forest, "tripled_clique": model.tripled_clique, "grid64": lambda: model.grid(64, 64),
    "ragged_directed": model.ragged_directed, "ragged_directed_37": lambda: model.ragged_directed(11, 37),
    "sparse_symmetric": lambda: model.sparse_symmetric(100), "single": lambda: model.single(False),
    "single_loop": lambda: model.single(True),
}


@pytest.mark.parametrize("name", list(MODEL_GRAPHS))
def test_plan_equals_models_on_the_models_graphs(oracle, name):
    _check_plan(oracle, *MODEL_GRAPHS[name]())


@pytest.mark.parametrize("scale,ef,seed", [(10, 16, 10), (13, 16, 13)])
def test_plan_equals_models_on_rmat(oracle, scale, ef, seed):
    n, ro, ci, w = oracle.rmat_csr(scale, ef, seed)
    _check_plan(oracle, ro, ci)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_plan_equals_models_on_the_cases(oracle, name):
    ro, ci = cases.get(name)
    if name not in cases.DIRECTED:
        src = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        assert np.array_equal(*[np.sort(a.astype(np.int64) * len(ro) + b) for a, b in ((src, ci), (ci, src))]), "symmetric"
    plan = _check_plan(oracle, ro, ci)
    assert plan.kinds == cases.plan(name).kinds


def _kinds(text):
    codes = {v: k for k, v in model.KIND_NAMES.items()}
    return [codes[w] for w in text.split()]


BROOM_TAIL = "min list mini min idle"
# (K44, 1892 entries, is the last front of one workgroup; K45 has 1980 and K46 2070)
CASE_KINDS = {
    "broom2047": "min list mini " + BROOM_TAIL,
    "broom2048": "min list mini expand " + BROOM_TAIL,
    "broom2049": "min list expand filter expand " + BROOM_TAIL,
    "multi_broom": "min list expand filter expand " + BROOM_TAIL,
    "cliques32x5_33x4": "min list expand min expand min idle",
    "stairs2_40": "min list mini " + "min mini " * 38 + "min idle",
    "stairs2_100": "min list mini " + "min mini " * 43 + "min expand " * 55 + "min idle",
    "stairs_even2_80": "min list mini " * 22 + "min list expand " * 18 + "min idle",
    "stairs_even2_300": "min list mini " * 22 + "min list expand " * 128 + "min idle",
    "star3000": "min list expand filter min idle",
    "star100": "min list mini min idle",
    "funnel1500": "min list expand filter min idle",
    "funnel3001": "min list expand filter expand min idle",
    "funnel3002": "min list expand min expand min idle",
    "clique5": "min list mini min idle",
    "clique2": "min list mini min idle",
    "cap_row5": "min list mini min idle",
}
CASE_KINDS.update({"tail%d" % n: "min list mini " + BROOM_TAIL for n in cases.TAIL_NS})
# (largest k-core, levels, passes, stranded) where the case names them
CASE_NUMBERS = {
    "broom2047": (3, 2, 3, 0), "broom2048": (3, 2, 3, 0), "broom2049": (3, 2, 3, 0),
    "multi_broom": (3, 2, 3, 0), "cliques32x5_33x4": (32, 2, 2, 0),
    "stairs2_40": (39, 39, 39, 0), "stairs2_100": (99, 99, 99, 0), "stairs_even2_80": (79, 40, 40, 0),
    "stairs_even2_300": (299, 150, 150, 0),
    "star3000": (1, 1, 1, 1), "star100": (1, 1, 1, 1),
    "funnel1500": (1, 1, 1, 1), "funnel3001": (1, 1, 2, 0), "funnel3002": (2, 2, 2, 0),
    "clique5": (4, 1, 1, 0), "clique2": (1, 1, 1, 0), "cap_row5": (-1, 1, 1, 0),
}
CASE_NUMBERS.update({"tail%d" % n: (3, 2, 2, 0) for n in cases.TAIL_NS})
# (kinds up to the first idle launch, launches enqueued, host waits)
CASE_LAUNCHES = {"stairs2_40": (81, 192, 2), "stairs2_100": (201, 448, 3), "stairs_even2_80": (122, 192, 2),
                 "stairs_even2_300": (452, 704, 4)}


def test_every_case_is_pinned():
    assert set(CASE_KINDS) == set(cases.CASES) == set(CASE_NUMBERS)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_plan_is_what_the_case_was_built_for(name):
    plan = cases.plan(name)
    assert plan.kinds == _kinds(CASE_KINDS[name]), plan.names()
    st = plan.stats
    assert (plan.largest, st["levels"], st["passes"], st["stranded"]) == CASE_NUMBERS[name]
    waits, launches = model.host_waits_and_launches(len(plan.kinds))
    assert (len(plan.kinds), launches, waits) == CASE_LAUNCHES.get(name, (len(plan.kinds), 64, 1))


def test_case_fronts_sit_on_the_thresholds():
    M, E = model.MINI, model.EXPAND
    fronts = {name: cases.plan(name).fronts for name in cases.CASES}
    lists = {name: cases.plan(name).lists for name in cases.CASES}
    # KCORE_MINI_MAX from both sides, at the launch's choice and at the hand-on inside a MINI
    assert fronts["broom2047"][:2] == [(2, 2047, M), (2, 2048, M)]
    assert fronts["broom2048"][:2] == [(2, 2048, M), (2, 2049, E)]
    assert fronts["broom2049"][:2] == [(2, 2049, E), (2, 2050, E)]
    assert (45, 1980, M) in fronts["stairs2_100"] and (46, 2070, E) in fronts["stairs2_100"]
    # KCORE_LONG_MIN and KCORE_SEG from both sides: one short row and 1 + 1 + 1 + 1 + 2 + 2 + 3 + 4 + 5 items
    assert cases.HUB_ROWS == (31, 32, 33, 255, 256, 257, 512, 513, 1024, 1025)
    assert fronts["multi_broom"][:2] == [(2, 3928, E), (2, 3938, E)] and lists["multi_broom"][:2] == [(3928, 0), (1, 20)]
    ro, ci = cases.get("multi_broom")
    assert tuple(np.diff(ro)[:10]) == cases.HUB_ROWS
    # every entry of a hub's row is a leaf (final degree -1) or the K4: nothing a lost or doubled segment could hide behind
    deg = cases.plan("multi_broom").degrees
    assert (deg[10:-4] == -1).all() and (deg[:10] == -1).all() and (deg[-4:] == -3).all()       # (a hub: its K4 vertex left after it)
    # the stages: 160 short rows in one wave's scan range (ids 0 .. 255; flush at 128), 132 long rows of exactly 32 entries (64 staged)
    assert fronts["cliques32x5_33x4"] == [(32, 4960, E), (33, 4224, E)] and lists["cliques32x5_33x4"] == [(160, 0), (0, 132)]
    # a vertex every wave decrements: candidate once, and then stranded / leaving / listed by the MIN
    assert fronts["funnel1500"] == [(2, 3000, E)] and cases.plan("funnel1500").degrees[cases.FUNNEL_SOURCES] == -1500
    assert fronts["funnel3001"] == [(2, 3000, E), (2, 3001, E)] and cases.plan("funnel3001").cores[cases.FUNNEL_SOURCES] == 1
    assert fronts["funnel3002"] == [(2, 3000, E), (3, 3002, E)] and cases.plan("funnel3002").cores[cases.FUNNEL_SOURCES] == 2
    # the stranded hub keeps core number 0
    for name in ("star3000", "star100"):
        assert cases.plan(name).cores[0] == 0 and (cases.plan(name).cores[1:] == 1).all()
    # k == n: level n runs, nobody leaves behind it -- in cap_row5 somebody IS at degree n then
    assert fronts["clique5"] == [(5, 20, M)] and fronts["clique2"] == [(2, 2, M)]
    assert fronts["cap_row5"] == [(5, 4, M)] and cases.plan("cap_row5").degrees.tolist() == [5, 0, 0, 0, -4]
    assert cases.plan("cap_row5").cores.tolist() == [0, 4, 0, 0, 0]
    # the first level's only vertex is the scan's last id
    for n in cases.TAIL_NS:
        assert fronts["tail%d" % n] == [(2, 1, M), (4, 13, M)]
        assert np.nonzero(cases.plan("tail%d" % n).cores == 1)[0].tolist() == [n - 1]


def test_cases_reach_every_kind_and_every_transition():
    seen, pairs = set(), set()
    for name in cases.CASES:
        kinds = cases.plan(name).kinds
        seen.update(kinds)
        pairs.update(zip(kinds, kinds[1:]))
    assert seen == {model.MIN, model.LIST, model.EXPAND, model.FILTER, model.MINI, model.IDLE}
    for pair in ((model.MIN, model.EXPAND), (model.MIN, model.MINI), (model.MINI, model.EXPAND), (model.FILTER, model.EXPAND),
                 (model.FILTER, model.MIN), (model.EXPAND, model.MIN), (model.LIST, model.MINI), (model.LIST, model.EXPAND)):
        assert pair in pairs, pair
