"""The launch chain's host loop and its edge cases, on the CPU: tests/chain_model.py against the constants of
include/mgx/launch_chain.hpp, and every case of tests/chain_cases.py against its algorithm's model -- its pinned K is the K the
model predicts, so a case that drifts off its seam fails here."""
import os
import re

import numpy as np
import pytest

from tests import chain_cases as cases
from tests import chain_model, kcore_model, ktruss_cases, ktruss_model, lpa_model, msbfs_cases, msbfs_model, scc_cases, scc_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", "mgx", name)).read()


def test_constants_are_the_headers():
    text = _header("launch_chain.hpp")
    c = dict((k, v) for k, v in re.findall(r"constexpr int (CHAIN_\w+) = ([^;]+);", text))
    assert (int(c["CHAIN_BATCH_MIN"]), int(c["CHAIN_BATCH_MAX"])) == (chain_model.BATCH_MIN, chain_model.BATCH_MAX) == (64, 256)
    assert c["CHAIN_LOG_CAP"].replace(" ", "") == "1<<16" and chain_model.LOG_CAP == 1 << 16
    assert re.search(r"batch = std::min\(batch \* 2, CHAIN_BATCH_MAX\)", text), "the batches double"
    assert kcore_model.host_waits_and_launches is not chain_model.waits_and_launches          # (a wrapper, so its callers stay)
    assert (kcore_model.BATCH_MIN, kcore_model.BATCH_MAX) == (64, 256)
    api = open(os.path.join(ROOT, "mini_amd", "api.py")).read()
    assert re.search(r"^CHAIN_LOG_CAP = 1 << 16\b", api, re.M), "the Python side's cap"


def test_waits_and_launches():
    w = chain_model.waits_and_launches
    assert [w(k) for k in (1, 2, 63, 64)] == [(1, 64)] * 4
    assert [w(k) for k in (65, 192)] == [(2, 192)] * 2 and [w(k) for k in (193, 448)] == [(3, 448)] * 2
    assert [w(k) for k in (449, 704, 705)] == [(4, 704), (4, 704), (5, 960)]
    assert [w(k) for k in (1, 64, 65, 449)] == [kcore_model.host_waits_and_launches(k) for k in (1, 64, 65, 449)]
    # a seam is where one launch more costs a wait more; every seam value of SEAMS stands at one, below it or above it
    turns = [k for k in range(1, 500) if w(k + 1)[0] > w(k)[0]]
    assert turns == [64, 192, 448] and chain_model.SEAMS == tuple(k + d for k in turns for d in (-1, 0, 1))
    for k in (65535, 65536, 65537):                              # 64 + 128 + 256 x 255 = 65 472 < 65 535: the same batch holds all three
        assert w(k) == (258, 64 + 128 + 256 * 256)


def test_logged():
    assert chain_model.logged([1, 2, 9], 9) == [1, 2, 9] + [9] * 61
    assert chain_model.logged([1] * 64 + [9], 9) == [1] * 64 + [9] * 128
    long = chain_model.logged([1] * 65536 + [9], 9)
    assert len(long) == chain_model.LOG_CAP and set(long) == {1}


def test_every_algorithm_stands_on_every_seam():
    for algo in cases.ALGOS:
        ks = sorted({c.K for c in cases.SEAM_CASES if c.algo == algo})
        if algo == "louvain":                                    # (3 t + 2 or 5 t + 2: see tests/chain_cases.py)
            assert ks == [62, 65, 191, 192, 194, 447, 449]
            for k in (63, 64, 193, 448):
                assert (k - 2) % 3 and (k - 2) % 5
        else:
            assert ks == list(chain_model.SEAMS), algo
        assert any(k <= 64 for k in ks) and 65 in ks, algo      # both sides of the first seam
    assert len({cases.case_id(c) for c in cases.SEAM_CASES + cases.CAP_CASES}) == len(cases.SEAM_CASES + cases.CAP_CASES)


@pytest.mark.parametrize("case", cases.SEAM_CASES, ids=cases.case_id)
def test_seam_case_has_its_k(case):
    assert cases.predicted_k(case) == case.K
    w = cases.wanted(case)
    if case.algo == "lpa":
        assert w["kinds"][-1] == lpa_model.IDLE and w["stats"]["converged"] == 0 and w["stats"]["iterations"] == case.args["max_iter"]
    if case.algo == "ktruss":
        assert len(ktruss_model.peel_kinds(w)) == case.K
    if case.algo == "msbfs":
        assert (w["kinds"] == msbfs_model.PUSH).all() and sum(w["long"]) == 1 - case.K % 2
    if case.algo == "scc":
        n = len(cases.graph(case)[0]) - 1
        st = w["stats"]
        if case.name.startswith("path"):
            assert scc_model.path_launches(n) == case.K and st["trimmed"] == n and st["pivot_size"] == 0
        else:
            assert scc_model.ring_launches(n) == case.K and st["trimmed"] == 0 and st["pivot_size"] == n and st["rounds"] == 0
    if case.algo == "louvain":
        assert w["levels"][0][2] == case.args["max_iter"]           # the level ran to max_iter, not to its second rejection


def test_lpa_cap_cases_by_their_closed_forms():
    """the models of the cap cases take seconds and run once, in the GPU suite; here their K by the families' formulas, and the
    formulas against the model at small max_iter"""
    for c in cases.LPA_CAP:
        i = c.args["max_iter"]
        assert c.K == (2 * i + 8 if c.args["opts"] else 2 * i + 3)
    for i in (3, 4, 9):
        assert len(lpa_model.propagate(*cases.lpa_pair(), True, lpa_model.SYNC, max_iter=i)["kinds"]) == 2 * i + 3
        w = lpa_model.propagate(*cases.lpa_pair_and_clique(), True, lpa_model.SYNC, max_iter=i, **cases.LPA_EVEN_OPTS)
        assert len(w["kinds"]) == 2 * i + 8 and w["kinds"].count(lpa_model.MARK) == 2 and w["kinds"].count(lpa_model.LONG) == 3
    assert [c.K for c in cases.LPA_CAP] == [chain_model.LOG_CAP - 1, chain_model.LOG_CAP, chain_model.LOG_CAP + 1]


def test_ktruss_launches_and_kinds():
    w = ktruss_model.decompose(*ktruss_cases.grid(100, 40, True), True)
    assert (w["stats"]["levels"], w["stats"]["passes"]) == (1, 40) and ktruss_model.peel_launches(w["stats"]) == 83 + 2
    M, L, E, S, D = ktruss_model.MIN, ktruss_model.LIST, ktruss_model.EXPAND, ktruss_model.SEAL, ktruss_model.IDLE
    assert ktruss_model.peel_kinds(w) == [M, L, S] + [E, S] * 40 + [M, D]
    w = ktruss_model.decompose(*ktruss_cases.clique_chain(3, 6), True)            # four levels of one pass
    assert ktruss_model.peel_kinds(w) == [M, L, S, E, S] * 4 + [M, D] and ktruss_model.peel_launches(w["stats"]) == 22
    w = ktruss_model.decompose(np.zeros(4, np.int32), np.zeros(0, np.int32), True)
    assert ktruss_model.peel_kinds(w) == [M, D] and ktruss_model.peel_launches(w["stats"]) == 2
    text = _header("ktruss_fused.hpp")
    enum = dict((k, int(v)) for k, v in re.findall(r"KTRUSS_(\w+) = (\d+)", re.search(r"enum ktruss_kind_t[^{]*\{([^}]*)\}", text).group(1)))
    assert enum == {"INIT": 0, "MIN": M, "LIST": L, "EXPAND": E, "SEAL": S, "DONE": D}


def test_scc_formulas():
    text = _header("scc_fused.hpp")
    enum = dict((k, int(v)) for k, v in re.findall(r"SCC_(\w+) = (\d+)", re.search(r"enum scc_kind_t[^{]*\{([^}]*)\}", text).group(1)))
    m = scc_model
    assert enum == {"INIT": 0, "DEGINIT": m.DEGINIT, "LIST": m.LIST, "EXPAND": m.EXPAND, "PMAX": m.PMAX, "PPICK": m.PPICK, "RINIT": m.RINIT,
                    "FWD": m.FWD, "ROOTS": m.ROOTS, "BWD": m.BWD, "SEAL": m.SEAL, "DONE": m.DONE}
    for n in (1, 2, 3, 4, 5, 120, 121):
        assert len(m.path_kinds(n)) == m.path_launches(n)
        # the fronts of the trim, from the definition: both ends, then the next two ... ceil(n / 2) of them
        alive, fronts = np.ones(n, bool), 0
        src, dst = m.arcs(*scc_cases.path(n))
        while alive.any():
            keep = alive[src] & alive[dst]
            go = alive & ((np.bincount(src[keep], minlength=n) == 0) | (np.bincount(dst[keep], minlength=n) == 0))
            assert go.any()
            alive &= ~go
            fronts += 1
        assert m.path_kinds(n).count(m.EXPAND) == fronts
    for n in (2, 3, 27, 28):
        assert len(m.ring_kinds(n)) == m.ring_launches(n) and m.ring_kinds(n).count(m.FWD) == m.ring_kinds(n).count(m.BWD) == n
    n = cases.SCC_CAP_RING
    assert m.ring_launches(n - 1) <= chain_model.LOG_CAP < m.ring_launches(n) == chain_model.LOG_CAP + 1


def test_msbfs_path_closed_form_is_the_model():
    for n in (10, 300):
        w = msbfs_model.traverse(*msbfs_cases.path(n), [0], True, False)
        c = msbfs_model.path_from_its_end(n)
        assert sorted(w) == sorted(c)
        for k in w:
            if isinstance(w[k], np.ndarray):
                assert w[k].dtype == c[k].dtype and np.array_equal(w[k], c[k]), k
            else:
                assert w[k] == c[k], k
    assert msbfs_model.path_from_its_end(65537)["launches"] == 2 * 65537 + 3


def test_msbfs_launches_count_the_long_levels():
    """a star from its centre (one long PUSH row) and from a leaf, pushed; the fans pulled: LONG wherever a long in-row is unseen"""
    ro, ci = msbfs_cases.star(2000)
    w = msbfs_model.traverse(ro, ci, [0], False, False)
    assert w["kinds"].tolist() == [0, 0] and w["long"] == [True, False] and w["launches"] == 2 + 5 + 1
    w = msbfs_model.traverse(ro, ci, [5], True, False, pull_div=1 << 30)
    assert w["kinds"].tolist() == [1, 1, 1] and w["long"] == [True, False, False] and w["launches"] == 2 + 7 + 1
    w = msbfs_model.traverse(ro, ci, [], True, False)
    assert w["launches"] == 0 and w["long"] == []
    w = msbfs_model.traverse(ro, ci, np.arange(70), True, False, pull_div=0)
    assert w["stats"]["batches"] == 2 and w["launches"] == 4 + 2 * len(w["kinds"]) + sum(w["long"]) + 1
