"""CPU suite for the backward of the neighbour feature aggregation (mgx_aggbwd_*, include/mgx/agg_backward.hpp,
include/gunrock/aggbwd/): the header declares and the library exports and binds it, NULL handles and invalid parameters are
statuses, the kernels keep out of scratch, the model the GPU tests compare against (tests/aggbwd_model.py) is within the summation
bound of a float64 A^T g and its winners are the forward model's, and every case of tests/aggbwd_cases.py tells apart what it is
there to tell apart."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import agg_model as fwd
from tests import aggbwd_cases as cases
from tests import aggbwd_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_aggbwd_create", "mgx_aggbwd_free", "mgx_aggbwd_run", "mgx_aggbwd_enact", "mgx_aggbwd_upload", "mgx_aggbwd_output", "mgx_aggbwd_result",
         "mgx_aggbwd_transpose", "mgx_aggbwd_bins", "mgx_aggbwd_set_timing", "mgx_aggbwd_phase_ms"]
# (parts of the mangled names and the instances expected: float and float4; two walks or two combines)
KERNELS = [(("k_aggb_rowsI",), 4), (("k_aggb_itemsI",), 4), (("k_aggb_foldI",), 2), (("k_aggb_scaleI",), 2), (("k_aggb_win_rowsI",), 4), (("k_aggb_win_itemsI",), 4),
           (("k_aggb_win_foldI",), 4), (("k_aggb_tr_countE",), 1), (("k_aggb_tr_fillE",), 1), (("k_aggb_tr_rowsE",), 1),
           (("6aggbwd", "win_functor_t"), None), (("6aggbwd", "col_functor_t"), None)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_header_declares_and_library_exports_and_binds_aggbwd(built):
    import mini_amd
    from mini_amd import _lib
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    declared = sorted(set(re.findall(r"MGX_API int (mgx_aggbwd_\w+)\(", header)))
    assert declared == sorted(NAMES)
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
        assert name in _lib.SIGNATURES, name
    gp = mini_amd.AggregateGradProblem
    assert gp.KEYS == model.STAT_KEYS + ("launches", "host_waits", "built") and gp.OPS == fwd.OPS and gp.BINS == model.BIN_KEYS + ("seg",)
    assert gp.PHASES == ("transpose", "winners", "rows", "items", "fold")
    for member in ("run", "enact", "result", "transpose", "bins", "set_timing", "phase_ms", "close"):
        assert hasattr(gp, member), member
    for word in ("ASCENDING entry order", "never fused", "edge weights is not built", "+0.0", "padding columns"):
        assert word in gp.__doc__, word
    assert "edge weights is not built" in header
    import mini_amd.autograd                                                    # imports torch inside, and nothing of it at package import
    assert hasattr(mini_amd.autograd, "aggregate")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, d = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 10)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_aggbwd_create(None, C.byref(h)) == bad
    for go in (lib.mgx_aggbwd_run, lib.mgx_aggbwd_enact):
        assert go(None, 0, None, -1, None, 4, 4, 0, 0, None, 4, 0, None, 4, st) == bad
        assert b"NULL" in lib.mgx_last_error()
    assert lib.mgx_aggbwd_upload(None, 0, None, 0, 1, C.byref(d)) == bad
    assert lib.mgx_aggbwd_output(None, 0, 1, C.byref(d)) == bad
    for fn in (lib.mgx_aggbwd_result, lib.mgx_aggbwd_bins, lib.mgx_aggbwd_phase_ms):
        assert fn(None, None) == bad
    assert lib.mgx_aggbwd_transpose(None, None, None, None) == bad
    assert lib.mgx_aggbwd_set_timing(None, 1) == bad
    assert lib.mgx_aggbwd_free(None) == 0


@pytest.mark.parametrize("args, word", [
    (dict(feats=0), "feats"), (dict(feats=65537), "feats"), (dict(ldgy=3), "ldgy"), (dict(ldgx=3), "ldgx"), (dict(op=4), "op"), (dict(op=-1), "op"),
    (dict(op=2, ldx=3), "ldx"), (dict(op=3, ldx=3), "ldx"), (dict(source=3), "source"), (dict(source=-1), "source"), (dict(x_rows=-1), "x_rows"),
    (dict(x_rows=2 ** 31), "x_rows")])
def test_invalid_parameters_are_statuses(built, args, word):
    """the parameters are checked before anything else, the handle included: each gives MGX_E_INVALID and a message that names it"""
    import mini_amd
    lib = mini_amd.lib
    a = dict(source=0, x_rows=0, ldgy=4, ldx=4, ldgx=4, feats=4, op=0)
    a.update(args)
    for go in (lib.mgx_aggbwd_run, lib.mgx_aggbwd_enact):
        assert go(None, a["source"], None, -1, None, a["ldgy"], a["feats"], a["op"], 0, None, a["ldx"], a["x_rows"], None, a["ldgx"], None) == mini_amd.MGX_E_INVALID
        assert word.encode() in lib.mgx_last_error(), lib.mgx_last_error()


def test_aggbwd_kernels_do_not_spill(built):
    """every instance of the backward's, the winners' and the transpose's kernels and the operator path's functors uses no scratch
    and spills nothing; the forward's three still have their six instances each"""
    path = os.path.join(ROOT, "mini_amd", "kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resource remarks"
    cur, res = None, {}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key, pat in (("scratch", r"ScratchSize[^:]*: (\d+)"), ("vspill", r"VGPRs Spill[^:]*: (\d+)"), ("sspill", r"SGPRs Spill[^:]*: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                res.setdefault(cur, {})[key] = int(m.group(1))
    for parts, count in KERNELS:
        found = [k for k in res if all(x in k for x in parts)]
        assert found, parts
        if count is not None:
            assert len(found) == count, (parts, found)
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])
    for name in ("rows", "items", "fold"):
        assert len([k for k in res if "k_agg_%sI" % name in k]) == 6, name


# ---- the model's properties ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("seg", [64, 256])
def test_the_model_is_within_the_summation_bound_of_a_float64_transposed_product(seg, op, weighted):
    """per element |model - float64 sum of the same float32 terms u_e| <= L u sum|u_e|, u = 2^-24, L the fold length |L_c|: any order
    of L - 1 float32 additions is within (L - 1) u / (1 - (L - 1) u) sum|u|, which L u sum|u| covers while L (L - 1) u <= 1, up to
    L = 4096 (tests/test_agg_cpu.py derives the same bound for the forward).  The terms themselves are checked against float64
    beside it: each is the float64 value w g / d within one rounding per operation, |u_e - exact| <= 2 u |exact| (1 + u)."""
    ro, ci = cases.graph_cols([0, 1, 2, 63, 64, 65, 300, 1000, 4000], seed=seg, rows=40)
    n = len(ro) - 1
    gy = cases.features(n, 5, seed=seg)
    w = cases.weights(len(ci), seg) if weighted else None
    got = model.backward(ro, ci, gy, op, w, seg=seg, x_rows=n)
    u32, _ = model.terms(ro, ci, gy, op, w, None, seg, got["t_row"], got["t_pos"])
    u = 2.0 ** -24
    d = np.diff(ro).astype(np.float64)
    exact = gy.astype(np.float64)[got["t_row"]]
    if op == "mean":
        exact = exact / d[got["t_row"]][:, None]
    if weighted:
        exact = exact * w.astype(np.float64)[got["t_pos"]][:, None]
    assert (np.abs(u32.astype(np.float64) - exact) <= 2 * u * np.abs(exact) * (1 + u)).all()
    t = u32.astype(np.float64)
    off = got["t_off"]
    assert sorted(set(np.diff(off))) == [0, 1, 2, 63, 64, 65, 300, 1000, 4000]
    for c in range(n):
        rows = t[off[c]:off[c + 1]]
        L = len(rows)
        assert (np.abs(got["gx"][c].astype(np.float64) - rows.sum(axis=0)) <= L * u * np.abs(rows).sum(axis=0)).all(), (c, L)
        if L == 0:
            assert (_bits(got["gx"][c]) == 0).all()                                # +0.0


def test_the_transpose_is_ascending_and_complete():
    ro, ci = cases.graph_cols(cases.IN_DEGREES, seed=1, long_rows=(3, 9))
    n = len(ro) - 1
    off, row, pos = model.transpose(ro, ci, n + 5)                                # x_rows above n: the rows behind are empty
    assert len(off) == n + 6 and off[-1] == len(ci) and (off[n:] == len(ci)).all()
    assert sorted(pos) == list(range(len(ci)))
    for c in range(n):
        p = pos[off[c]:off[c + 1]]
        assert (np.diff(p) > 0).all() and (ci[p] == c).all()
    assert ((ro[row] <= pos) & (pos < ro[row + 1])).all()
    # a hop's rows of a block: offsets that do not start at 0 keep absolute places and count the rows from the hop's first
    off, row, pos = model.transpose(ro[10:31], ci, n)
    assert off[-1] == ro[30] - ro[10] and pos.min(initial=ro[10]) >= ro[10] and pos.max(initial=0) < ro[30]
    assert ((ro[10 + row] <= pos) & (pos < ro[11 + row])).all()


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("weighted", [False, True])
def test_the_models_winners_are_the_forward_models(op, weighted):
    """t[win[r, f]] equals the forward model's Y[r, f] bit for bit (no NaN here); the winner is the FIRST entry with that value"""
    ro, ci = cases.graph_rows([0, 1, 2, 7, 63, 64, 65, 129, 321, 1000], seed=5, n=50)      # (50 columns: equal values are frequent)
    x = cases.features(50, 4, seed=5)
    w = cases.weights(len(ci), 5) if weighted else None
    for seg in (64, 256):
        win, y = model.winners(ro, ci, x, op, w, seg)
        want = fwd.aggregate(ro, ci, x, op, w, seg=seg)["y"]
        assert np.array_equal(_bits(y), _bits(want))
        t = x[ci] if w is None else (w[:, None] * x[ci]).astype(np.float32)
        for r in range(len(ro) - 1):
            if ro[r] == ro[r + 1]:
                assert (win[r] == -1).all()
                continue
            for f in range(4):
                assert ro[r] <= win[r, f] < ro[r + 1]
                assert _bits(t[win[r, f], f]) == _bits(want[r, f])
                same = np.flatnonzero(t[ro[r]:ro[r + 1], f] == want[r, f])
                assert win[r, f] == ro[r] + same[0]


# ---- the cases tell apart what they are there to tell apart ----
def test_case_a_the_order_of_a_column_shows_in_the_bits():
    ro, ci, gy = cases.stability_case(4)
    n = len(ro) - 1
    good = model.backward(ro, ci, gy, "sum", seg=64, x_rows=n)
    bad = model.backward(ro, ci, gy, "sum", seg=64, x_rows=n, reverse=True)
    mags = np.abs(gy[good["t_row"][good["t_off"][1]:good["t_off"][2]]])
    assert good["t_off"][2] - good["t_off"][1] == 48 and mags.max() / mags.min() > 2.0 ** 30
    assert (_bits(good["gx"][1]) != _bits(bad["gx"][1])).any()


def test_case_b_the_division_comes_before_the_weight():
    ro, ci, w, gy = cases.mean_case(8)
    for r, d in ((0, 3), (1, 7)):
        first = (w[ro[r]:ro[r + 1], None] * (gy[r] / np.float32(d)).astype(np.float32)).astype(np.float32)
        after = ((w[ro[r]:ro[r + 1], None] * gy[r]).astype(np.float32) / np.float32(d)).astype(np.float32)
        assert (_bits(first) != _bits(after)).any(), d
    got = model.backward(ro, ci, gy, "mean", w, x_rows=3)
    by_hand = np.zeros((3, 8), dtype=np.float32)
    seen = set()
    for r, d in ((0, 3), (1, 7)):
        g = (gy[r] / np.float32(d)).astype(np.float32)
        for e in range(ro[r], ro[r + 1]):
            u = (w[e] * g).astype(np.float32)
            by_hand[ci[e]] = u if ci[e] not in seen else (by_hand[ci[e]] + u).astype(np.float32)
            seen.add(ci[e])
    assert np.array_equal(_bits(got["gx"]), _bits(by_hand))


def test_case_c_no_fused_multiply_add():
    ro, ci, w, gy = cases.fma_case(3)
    got = model.backward(ro, ci, gy, "sum", w, x_rows=2)
    assert (_bits(got["gx"][0]) == 0).all() and (_bits(got["gx"][1]) == 0).all()
    fused = np.float32(float(w[1]) * float(gy[1, 0]) + float(gy[0, 0]))
    assert fused == np.float32(2.0 ** -24)


@pytest.mark.parametrize("op", ["max", "min"])
def test_case_d_ties_zeros_and_nans(op):
    ro, ci, x = cases.tie_case(4, op)
    win, y = model.winners(ro, ci, x, op, None, 64)
    assert (win[0] == 10).all()                                                   # inside segment 0, across the boundary (70) and the last (129)
    one_seg, _ = model.winners(ro, ci, x, op, None, 256)
    assert (one_seg[0] == 10).all()
    assert (win[1] == 130).all() and (_bits(y[1]) == 0).all()                      # +0.0 against -0.0: neither t > acc nor t < acc
    assert (win[2] == 132).all() and np.isnan(y[2]).all()                          # a leading NaN keeps the win
    assert ((win[3] == 135) | (win[3] == 137)).all() and not np.isnan(y[3]).any()  # a later NaN never wins
    assert np.isin(win[4], [138, 140]).all()                                       # column 5 three times: its first entry, or the self-loop
    assert (win[5:] == -1).all()
    gy = cases.features(len(ro) - 1, 4, seed=3)
    got = model.backward(ro, ci, gy, op, None, seg=64, x=x)
    assert np.array_equal(_bits(got["gx"][10]), _bits(gy[0]))
    for c in (20, 70, 129, 131):
        assert (_bits(got["gx"][c]) == 0).all(), c                                # the losers of a tie get +0.0
    assert np.array_equal(_bits(got["gx"][132]), _bits(gy[2]))                    # the NaN's column gets row 2's gradient, nothing of row 3's


def test_counts_of_every_case_of_the_table():
    assert model.fused_counts(10, 0, False) == (1, 0)
    assert model.fused_counts(10, 2, False) == (3, 0)
    assert model.fused_counts(10, 2, False, mean=True, fwd_rows=5) == (4, 0)
    assert model.fused_counts(10, 0, False, minmax=True, fwd_rows=5, fwd_long=0) == (2, 0)
    assert model.fused_counts(10, 2, False, minmax=True, fwd_rows=5, fwd_long=1) == (6, 0)
    assert model.fused_counts(10, 2, False, minmax=True, fwd_rows=5, fwd_long=1, builds_fplan=True) == (8, 1)
    assert model.fused_counts(10, 0, True, entries=100, longest=40) == (11, 2)
    assert model.fused_counts(10, 1, True, entries=100000, longest=100000) == (3 + 10 + 6, 2)          # 6 merge passes from 2048 to 100 000
    assert model.fused_counts(10, 0, True, entries=1, longest=1) == (7, 1)
    assert model.fused_counts(10, 0, True, entries=0) == (1, 0)
    assert model.fused_counts(0, 0, True) == (0, 0)
    assert [model.sort_passes(x) for x in (0, 2048, 2049, 4096, 4097)] == [0, 0, 1, 1, 2]
