"""CPU suite for the neighbour feature aggregation (mgx_agg_*, include/mgx/agg_fused.hpp, include/gunrock/agg/): the header declares
and the library exports and binds it, NULL handles and invalid parameters are statuses, the switch is in the table, the kernels
keep out of scratch, and the model the GPU tests compare against (tests/agg_model.py) has the properties of the definition: it is
within the summation bound of a float64 sum of the same terms, it implements the segment tree, and its ops treat empty rows, +-0
and the mean's division as the definition says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import agg_cases as cases
from tests import agg_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_agg_create", "mgx_agg_free", "mgx_agg_run", "mgx_agg_enact", "mgx_agg_upload", "mgx_agg_output", "mgx_agg_result", "mgx_agg_bins",
         "mgx_agg_set_timing", "mgx_agg_phase_ms"]
# (parts of the mangled names: a kernel matches when it holds all of its parts)
KERNELS = [("k_agg_%sI" % k,) for k in ("rows", "items", "fold")] + [("k_agg_plan_countE",), ("k_agg_plan_fillE",), ("3agg", "row_functor_t")]


def test_header_declares_and_library_exports_and_binds_agg(built):
    import mini_amd
    from mini_amd import _lib
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    declared = sorted(set(re.findall(r"MGX_API int (mgx_agg_\w+)\(", header)))
    assert declared == sorted(NAMES)
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
        assert name in _lib.SIGNATURES, name
    for k, name in enumerate(("MGX_AGG_SUM", "MGX_AGG_MEAN", "MGX_AGG_MAX", "MGX_AGG_MIN")):
        assert getattr(mini_amd, name) == k and re.search(r"#define %s %d\b" % (name, k), header)
    ap = mini_amd.AggregateProblem
    assert ap.KEYS == model.RUN_KEYS + ("launches", "host_waits") and ap.OPS == model.OPS and ap.BINS == model.BIN_KEYS + ("seg",)
    for member in ("run", "enact", "result", "bins", "set_timing", "phase_ms", "close"):
        assert hasattr(ap, member), member
    for word in ("STORED order", "never fused", "local id", "0.0 for every op", "padding columns"):
        assert word in ap.__doc__, word


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h, d = C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 9)()
    bad = mini_amd.MGX_E_INVALID
    assert lib.mgx_agg_create(None, C.byref(h)) == bad
    for go in (lib.mgx_agg_run, lib.mgx_agg_enact):
        assert go(None, 0, None, -1, None, 0, 4, 4, 0, 0, None, 4, st) == bad
        assert b"NULL" in lib.mgx_last_error()
    assert lib.mgx_agg_upload(None, None, 0, 1, C.byref(d)) == bad
    assert lib.mgx_agg_output(None, 0, 1, C.byref(d)) == bad
    for fn in (lib.mgx_agg_result, lib.mgx_agg_bins, lib.mgx_agg_phase_ms):
        assert fn(None, None) == bad
    assert lib.mgx_agg_set_timing(None, 1) == bad
    assert lib.mgx_agg_free(None) == 0


@pytest.mark.parametrize("args, word", [
    (dict(feats=0), "feats"), (dict(feats=65537), "feats"), (dict(ldx=3), "ldx"), (dict(ldy=3), "ldy"), (dict(op=4), "op"), (dict(op=-1), "op"),
    (dict(source=3), "source"), (dict(source=-1), "source"), (dict(x_rows=-1), "x_rows")])
def test_invalid_parameters_are_statuses(built, args, word):
    """the parameters are checked before anything else, the handle included: each gives MGX_E_INVALID and a message that names it"""
    import mini_amd
    lib = mini_amd.lib
    a = dict(source=0, x_rows=0, ldx=4, feats=4, op=0, ldy=4)
    a.update(args)
    for go in (lib.mgx_agg_run, lib.mgx_agg_enact):
        assert go(None, a["source"], None, -1, None, a["x_rows"], a["ldx"], a["feats"], a["op"], 0, None, a["ldy"], None) == mini_amd.MGX_E_INVALID
        assert word.encode() in lib.mgx_last_error(), lib.mgx_last_error()


def _env_table():
    import mini_amd
    name, what = C.c_char_p(), C.c_char_p()
    n = mini_amd.lib.mgx_env_switches(-1, None, None)
    out = {}
    for i in range(n):
        mini_amd.lib.mgx_env_switches(i, C.byref(name), C.byref(what))
        out[name.value.decode()] = what.value.decode()
    return out


def test_the_switch_is_in_the_table_and_clamps(built):
    table = _env_table()
    assert "MGX_AGG_SEG" in table and "power of two" in table["MGX_AGG_SEG"] and "[64, 4096]" in table["MGX_AGG_SEG"]
    header = open(os.path.join(ROOT, "include", "mgx", "agg_fused.hpp")).read()
    for name, value in (("AGG_SEG_DEFAULT", model.SEG), ("AGG_SEG_MIN", model.SEG_MIN), ("AGG_SEG_MAX", model.SEG_MAX), ("AGG_UNROLL", model.UNROLL),
                        ("AGG_MAX_FEATS", model.MAX_FEATS)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), header), name          # the model mirrors the header's constants
    assert re.search(r"constexpr int AGG_TILE = WAVE;", header) and model.TILE == 64
    for value, want in ((-5, 64), (0, 64), (1, 64), (64, 64), (65, 128), (200, 256), (256, 256), (257, 512), (4096, 4096), (4097, 4096), (10 ** 9, 4096)):
        assert model.clamp_seg(value) == want


def test_agg_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: every instance of the three fused kernels, the two plan kernels and the operator
    path's functor use no scratch and spill nothing"""
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
    for parts in KERNELS:
        found = [k for k in res if all(x in k for x in parts)]
        assert found, parts
        if parts[0].endswith("I"):
            assert len(found) == 6, (parts, found)                              # float and float4, three combines
        for k in found:
            assert res[k].get("scratch", 0) == 0, (k, res[k])
            assert res[k].get("vspill", 0) == 0, (k, res[k])
            assert res[k].get("sspill", 0) == 0, (k, res[k])


# ---- the model's properties ----
def _terms(ro, ci, x, w):
    t = x[ci].astype(np.float32)
    return t if w is None else (w[:, None] * t).astype(np.float32)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("seg", [64, 256])
def test_the_model_is_within_the_summation_bound_of_a_float64_sum(seg, weighted):
    """per element |model - float64 sum of the same float32 terms| <= d u sum|t|, u = 2^-24: any order of d - 1 float32 additions
    is within (d - 1) u / (1 - (d - 1) u) sum|t|, which d u sum|t| covers while d (d - 1) u <= 1, that is up to d = 4096 -- the
    rows here stay below.  (The float64 sum's own error, d 2^-53 sum|t|, is 2^-29 of that.)  The mean adds one rounding of the
    quotient: |fl(S / d) - E / d| <= |S - E| / d + u |S / d| <= u sum|t| (1 + u) + u |E / d|"""
    ro, ci = cases.graph_rows([0, 1, 2, 63, 64, 65, 300, 1000, 4000], seed=seg, n=400)
    x = cases.features(400, 6, seed=seg)
    w = cases.weights(len(ci), seg) if weighted else None
    t = _terms(ro, ci, x, w).astype(np.float64)
    got = model.aggregate(ro, ci, x, "sum", w, seg=seg)["y"].astype(np.float64)
    mean = model.aggregate(ro, ci, x, "mean", w, seg=seg)["y"].astype(np.float64)
    u = 2.0 ** -24
    for r in range(len(ro) - 1):
        rows = t[ro[r]:ro[r + 1]]
        d = len(rows)
        exact, mass = rows.sum(axis=0), np.abs(rows).sum(axis=0)
        assert (np.abs(got[r, :] - exact) <= d * u * mass).all(), (r, d)
        if d:
            assert (np.abs(mean[r, :] - exact / d) <= u * mass * (1.0 + u) + u * np.abs(exact / d)).all(), (r, d)
    assert (got[9:] == 0).all()


def test_the_model_implements_the_segment_tree():
    """a row of 2 seg + 1 entries of mixed magnitudes: the tree's bits differ from the plain left-to-right fold's (the same entries
    under a seg that holds the whole row), and equal a hand-written tree"""
    seg = 64
    ro, ci = cases.graph_rows([2 * seg + 1], seed=1, n=200)
    x = cases.features(200, 5, seed=1)
    tree = model.aggregate(ro, ci, x, "sum", seg=seg)["y"]
    plain = model.aggregate(ro, ci, x, "sum", seg=256)["y"]
    assert tree.shape == plain.shape == (200, 5)
    assert (tree[0].view(np.uint32) != plain[0].view(np.uint32)).any()
    t = x[ci]
    parts = []
    for s in range(3):
        acc = t[s * seg].copy()
        for k in range(s * seg + 1, min((s + 1) * seg, len(t))):
            acc = (acc + t[k]).astype(np.float32)
        parts.append(acc)
    by_hand = ((parts[0] + parts[1]).astype(np.float32) + parts[2]).astype(np.float32)
    assert np.array_equal(tree[0].view(np.uint32), by_hand.view(np.uint32))
    left = t[0].copy()
    for k in range(1, len(t)):
        left = (left + t[k]).astype(np.float32)
    assert np.array_equal(plain[0].view(np.uint32), left.view(np.uint32))
    st = model.aggregate(ro, ci, x, "sum", seg=seg)["stats"]
    assert (st["long_rows"], st["segments"], st["team_rows"], st["empty_rows"]) == (1, 3, 0, 199)


def test_the_models_ops():
    ro, ci, x = cases.zeros_case(3)
    pos, neg = np.float32(0.0).view(np.uint32), np.float32(-0.0).view(np.uint32)
    for op in model.OPS:
        y = model.aggregate(ro, ci, x, op)["y"]
        assert (y[3].view(np.uint32) == pos).all(), op                          # a row without entries: +0.0
    for op in ("max", "min"):
        y = model.aggregate(ro, ci, x, op)["y"].view(np.uint32)
        assert (y[0] == pos).all() and (y[1] == neg).all(), op                  # the first of equal values stays
    y = model.aggregate(ro, ci, x, "sum")["y"].view(np.uint32)
    assert (y[0] == pos).all() and (y[1] == pos).all()                          # +0 + -0 = +0 either way
    two = np.array([0, 2], dtype=np.int32), np.array([1, 1], dtype=np.int32)
    assert (model.aggregate(*two, x, "sum")["y"].view(np.uint32) == neg).all()  # -0 + -0 = -0: the fold starts from t_0, not from 0.0
    # max and min pick elements; the mean is ONE division of the sum by float32(d)
    ro, ci = cases.graph_rows([3, 7], seed=2, n=20)
    x = cases.features(20, 4, seed=2)
    for r in range(2):
        t = x[ci[ro[r]:ro[r + 1]]]
        assert np.array_equal(model.aggregate(ro, ci, x, "max")["y"][r], t.max(axis=0))
        assert np.array_equal(model.aggregate(ro, ci, x, "min")["y"][r], t.min(axis=0))
        s = model.aggregate(ro, ci, x, "sum")["y"][r]
        want = (s.astype(np.float64) / float(len(t))).astype(np.float32)        # (float64 quotient of two float32, rounded once: exact)
        assert np.array_equal(model.aggregate(ro, ci, x, "mean")["y"][r].view(np.uint32), want.view(np.uint32))
    # the weighted term is rounded once, before the add
    ro, ci, w, x = cases.fma_case(2)
    assert (model.aggregate(ro, ci, x, "sum", w)["y"][0] == 0.0).all()


def test_shapes_and_fused_counts():
    assert [model.shape(f, True)[1] for f in (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    assert [model.shape(f, True)[2] for f in (256, 260, 512, 516)] == [1, 2, 2, 3]
    assert [model.shape(f, False)[1:] for f in (1, 2, 3, 5, 63, 64, 65, 129)] == [(1, 1), (2, 1), (4, 1), (8, 1), (64, 1), (64, 1), (64, 2), (64, 3)]
    assert model.is_vector(8, 8, 12) and not model.is_vector(8, 9, 8) and not model.is_vector(8, 8, 10) and not model.is_vector(6, 8, 8)
    assert not model.is_vector(8, 8, 8, x_addr=4) and not model.is_vector(8, 8, 8, y_addr=4) and model.is_vector(8, 8, 8, 32, 48)
    # every case of a run: a block without a -1 hop / a planned CSR without and with long rows / the run that builds a plan / no rows
    assert model.fused_counts(10, 0, False) == (1, 0)
    assert model.fused_counts(10, 2, False) == (3, 0)
    assert model.fused_counts(10, 0, True) == (3, 1)
    assert model.fused_counts(10, 2, True) == (5, 1)
    assert model.fused_counts(0, 0, True) == (0, 0) and model.fused_counts(0, 0, False) == (0, 0)
    st = model.aggregate(*cases.graph_rows([0, 1, 256, 257, 1000], n=8), cases.features(8, 12), seg=256)
    assert st["bins"] == {"none": 4, "team": 2, "long": 2, "segments": 2 + 4}
    assert st["stats"]["team_width"] == 4 and st["stats"]["col_tiles"] == 1 and st["stats"]["vector"] == 1 and st["stats"]["entries"] == 1514
