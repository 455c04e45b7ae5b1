"""CPU suite for the sparsification's path cases (tests/lspar_cases.py): by the numpy model alone (tests/lspar_model.py), every
case has the property it exists for at the thresholds of include/mgx/lspar_fused.hpp, which the case module holds by value.  The
GPU suite (tests/test_gpu_lspar_paths.py) runs the same cases with the thresholds the library reports."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import lspar_cases as cases
from tests import lspar_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_module_holds_the_headers_thresholds():
    text = open(os.path.join(ROOT, "include", "mgx", "lspar_fused.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (LSPAR_\w+) = (\d+);", text)}
    assert (const["LSPAR_SHORT_MAX"], const["LSPAR_SEG"], const["LSPAR_K_MAX"]) == (cases.SHORT_MAX, cases.SEG, cases.K_MAX)
    assert const["LSPAR_SHORT_MAX"] // const["LSPAR_SEL_GROUP"] == cases.SEL_ROUNDS
    assert "return k <= 2 ? k : (k + 3) & ~3;" in text
    assert [cases.stride(k) for k in (1, 2, 3, 4, 5, 8, 9, 31, 32)] == [1, 2, 4, 4, 8, 8, 12, 32, 32]


def test_library_exports_the_report(built):
    import mini_amd
    assert hasattr(mini_amd.LsparProblem, "info")
    out = (C.c_int64 * 5)()
    assert mini_amd.lib.mgx_lspar_info(None, out) == mini_amd.MGX_E_INVALID


def test_the_k_sweep_covers_both_sim_bodies_every_padding_and_partial_chunks():
    ks = cases.KS
    assert 2 in ks and 1 in ks                                                # the scalar body, one and two columns
    assert {cases.stride(k) - k for k in ks if k > 2} == {0, 1, 2, 3}         # every number of padding columns
    assert {k % 8 for k in ks if k > 8} >= {1, 4, 7}                          # partial last chunks of the 8-wide minhash loop
    assert max(ks) == cases.K_MAX


def test_length_edges():
    ro, ci, by_length = cases.length_edges()
    d = np.diff(ro)
    assert sorted(by_length) == [0, 63, 64, 65, 4095, 4096, 4097, 8192, 8193]
    for length, rows in by_length.items():
        assert len(rows) >= 2 and (d[rows] == length).all()
    assert cases.long_items(ro) == 2 * (1 + 1 + 1 + 2 + 2 + 3)
    assert len(ci) < 100000


@pytest.mark.parametrize("k", cases.KS)
def test_graded_long(k):
    """every level 0 .. k occurs on the hub's row, and there is an e for each place of the cut among the segments"""
    ro, ci = cases.graded_long(k)
    d = int(ro[1])
    assert d == 3 * cases.SEG + 5 and (np.diff(ro)[1:] <= k).all()
    sims = cases.row_sims(ro, ci, model.SEED, k)
    assert set(sims.tolist()) == set(range(k + 1))
    for place, e in cases.graded_params(ro, ci, model.SEED, k, cases.SEG):
        if place is None:
            assert k == 1
            continue
        assert e is not None, "k=%d: no e of the grid cuts the hub's row at the %s segment of its level" % (k, place)
        t = int(model.keep_count(d, e))
        c, q, at = cases.cut_of(sims, t)
        assert 0 < c < k and 0 < q < len(at)
        segs = at // cases.SEG
        mine = segs[q - 1]
        assert len(set(segs.tolist())) >= 2
        assert {"first": not (segs < mine).any() and (segs > mine).any(),
                "middle": (segs < mine).any() and (segs > mine).any(),
                "last": (segs < mine).any() and not (segs > mine).any()}[place]


def test_graded_long_k32_is_the_case_the_arithmetic_was_checked_on():
    ro, ci = cases.graded_long(32, seed=7)
    assert int(ro[1]) == 12293 and len(ci) == 29547
    sims = cases.row_sims(ro, ci, 7, 32)
    c, q, at = cases.cut_of(sims, int(model.keep_count(12293, 0.5)))
    assert c == 22 and np.bincount(at // cases.SEG).tolist() == [3, 4, 3]


@pytest.mark.parametrize("k", cases.KS)
def test_graded_short(k):
    """a row of exactly short_max entries: every level recurs in each of the four register rounds, and there is an e per place"""
    ro, ci = cases.graded_short(k)
    assert int(ro[1]) == cases.SHORT_MAX
    sims = cases.row_sims(ro, ci, model.SEED, k)
    chunk = cases.SHORT_MAX // cases.SEL_ROUNDS
    levels = set(sims.tolist())
    assert len(levels) >= min(k, 3) + 1
    for lv in levels:
        assert set((np.nonzero(sims == lv)[0] // chunk).tolist()) == set(range(cases.SEL_ROUNDS))
    for place, e in cases.graded_params(ro, ci, model.SEED, k, chunk):
        if place is None:
            assert k == 1
            continue
        assert e is not None, (k, place)
        t = int(model.keep_count(cases.SHORT_MAX, e))
        assert cases.cut_place(sims, t, k, chunk) == place


def test_graded_model_equals_the_definition():
    """the vectorised model on a graded case against the plain loop (rows not sorted, a row of ties)"""
    ro, ci = cases.graded_short(5)
    e = cases.graded_params(ro, ci, model.SEED, 5, 16)[1][1]
    got = model.sparsify(ro, ci, model.SEED, 5, e)
    want = model.brute_force(ro, ci, model.SEED, 5, e)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(a, np.asarray(b))
    assert np.array_equal(got[4], np.asarray(want[4], dtype=np.uint32))


def test_keep_count_edges():
    deg = cases.keep_degrees()
    ro, ci = cases.keep_count_edges()
    assert np.array_equal(np.diff(ro), deg) and len(ci) < 5_000_000
    for p, top in ((2, 128), (3, 40), (4, 16)):
        for j in (2, top):
            assert {j ** p - 1, j ** p, j ** p + 1} <= set(deg.tolist())
    for e in cases.KEEP_ES + (Fraction(1, 10), Fraction(9, 10)):
        exact = cases.exact_keep(deg, e)
        a, b = e.numerator, e.denominator
        for x, t in zip(deg.tolist(), exact.tolist()):
            assert t ** b <= x ** a < (t + 1) ** b
        assert np.array_equal(model.keep_count(deg, float(e)), exact), e
    # the perfect powers are where a floating pow lands on either side of the integer
    assert cases.exact_keep(np.array([40 ** 3 - 1, 40 ** 3, 40 ** 3 + 1]), Fraction(1, 3)).tolist() == [39, 40, 40]
    assert cases.exact_keep(np.array([16 ** 4 - 1, 16 ** 4]), Fraction(3, 4)).tolist() == [4095, 4096]


def _write_kernel(sims, t, seg, k, carry):
    """k_lspar_select_write's arithmetic on one row, segment by segment as its waves run it: the row's and the earlier segments'
    histograms, the cut level c, the quota q, `kept = pge(c) - pc + carry(pc, q)` entries before the segment, then the segment's
    entries in order.  -> the positions written to the row's t output slots (a slot written twice keeps the later write, -1: never)"""
    d = len(sims)
    segs = (d + seg - 1) // seg
    hist = np.array([np.bincount(sims[i * seg:(i + 1) * seg], minlength=k + 1) for i in range(segs)])
    H = hist.sum(axis=0)
    ge = np.cumsum(H[::-1])[::-1]
    c = max(level for level in range(k + 1) if ge[level] >= t)
    q = t - (ge[c] - H[c])
    out = {}
    for y in range(segs):
        P = hist[:y].sum(axis=0)
        pc = int(P[c])
        kept, at_c = int(P[c:].sum()) - pc + carry(pc, q), pc
        for p in range(y * seg, min(d, (y + 1) * seg)):
            keep = sims[p] > c or (sims[p] == c and at_c < q)
            at_c += sims[p] == c
            if keep:
                out[kept] = p
                kept += 1
    return [out.get(i, -1) for i in range(t)]


@pytest.mark.parametrize("k", [k for k in cases.KS if k >= 2])
def test_graded_long_tells_a_wrong_carry_from_the_right_one(k):
    """the write kernel's arithmetic restated: with min(pc, q) it gives the model's kept entries on the hub's row, with 0 in its
    place it does not -- at every place of the cut.  The case is sharp enough to see that term."""
    ro, ci = cases.graded_long(k)
    sims = cases.row_sims(ro, ci, model.SEED, k)
    for place, e in cases.graded_params(ro, ci, model.SEED, k, cases.SEG):
        t = int(model.keep_count(len(sims), e))
        want = model.sparsify(ro, ci, model.SEED, k, e)[2][:t].tolist()          # (row 0's kept positions: its eids)
        assert _write_kernel(sims, t, cases.SEG, k, min) == want, (k, place)
        assert _write_kernel(sims, t, cases.SEG, k, lambda pc, q: 0) != want, (k, place)
