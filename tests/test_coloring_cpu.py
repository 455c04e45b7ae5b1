"""CPU suite for the graph colouring (mgx_color_*, include/mgx/color_fused.hpp, include/gunrock/coloring/): the library
exports it, refuses NULL handles, its kernels keep their registers, and the numpy model the GPU tests compare against
(tests/coloring_model.py) holds the properties DESIGN 8 states."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import coloring_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgx_color_create", "mgx_color_free", "mgx_color_run", "mgx_color_enact", "mgx_color_colors",
         "mgx_color_colors_device", "mgx_color_round_trace"]


def test_library_exports_coloring(built):
    import mini_amd
    for name in NAMES:
        assert hasattr(mini_amd.lib, name), name
    assert hasattr(mini_amd, "ColorProblem")


def test_null_arguments_are_invalid(built):
    import mini_amd
    lib = mini_amd.lib
    h = C.c_void_p()
    assert lib.mgx_color_create(None, C.byref(h)) == mini_amd.MGX_E_INVALID
    st = (C.c_int64 * 4)()
    assert lib.mgx_color_run(None, 1, 0, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_color_enact(None, 1, 0, st) == mini_amd.MGX_E_INVALID
    assert lib.mgx_color_colors(None, None) == mini_amd.MGX_E_INVALID
    p = C.c_void_p()
    assert lib.mgx_color_colors_device(None, C.byref(p)) == mini_amd.MGX_E_INVALID
    r = C.c_int()
    assert lib.mgx_color_round_trace(None, None, 0, C.byref(r)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_color_free(None) == 0


def test_coloring_kernels_do_not_spill(built):
    """build() keeps the compiler's resource remarks: the colouring kernels use no scratch and spill nothing"""
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
    kernels = [k for k in res if "k_color_first" in k or "k_color_round" in k]
    assert len(kernels) == 3, sorted(kernels)
    for k in kernels:
        assert res[k].get("scratch", 0) == 0, (k, res[k])
        assert res[k].get("vspill", 0) == 0, (k, res[k])
        assert res[k].get("sspill", 0) == 0, (k, res[k])


def test_model_fmix32_is_a_bijection_on_a_sample():
    for s in (0, model.salt(model.SEED, 0), model.salt(31, 5)):
        k = model.keys(1 << 20, s)
        assert len(np.unique(k)) == 1 << 20
    # the reference constants of the finaliser
    assert int(model.fmix32(0)) == 0
    assert int(model.fmix32(1)) == 0x514E28B7


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 33])
def test_model_clique_takes_half_n_rounds_and_n_colours(n):
    ro, ci = model.clique(n)
    c, trace, left = model.color(ro, ci, seed=7, max_iter=0)
    assert len(trace) == math.ceil(n / 2) and left == 0
    assert len(np.unique(c)) == n and c.min() >= 1
    assert model.conflicts(ro, ci, c) == 0


@pytest.mark.parametrize("seed", [1, 31, model.SEED])
def test_model_colours_small_symmetric_graphs_properly(seed):
    rng = np.random.default_rng(seed)
    for n, m in ((10, 20), (100, 400), (500, 3000), (64, 2000)):
        s, d = rng.integers(0, n, m), rng.integers(0, n, m)           # self-loops and duplicates kept
        ro, ci = model.csr(n, s, d)
        c, trace, left = model.color(ro, ci, seed=seed, max_iter=0)
        assert left == 0 and (c > 0).all()
        assert model.conflicts(ro, ci, c) == 0
        assert trace[0] == n and (np.diff(trace) < 0).all()           # every round colours its smallest and largest key
        assert len(trace) <= math.ceil(n / 2)
        # max_iter stops early with exactly the later rounds' vertices left
        c3, t3, left3 = model.color(ro, ci, seed=seed, max_iter=3)
        assert np.array_equal(t3, trace[:3])
        assert np.array_equal(c3, np.where(c <= 6, c, 0))
        assert left3 == int((c > 6).sum())


def test_model_self_loops_and_parallel_entries_change_nothing():
    rng = np.random.default_rng(3)
    n = 300
    s, d = rng.integers(0, n, 900), rng.integers(0, n, 900)
    keep = s != d
    ro, ci = model.csr(n, s[keep], d[keep])
    extra_s = np.concatenate([s[keep], np.arange(n), s[keep][:100]])
    extra_d = np.concatenate([d[keep], np.arange(n), d[keep][:100]])
    ro2, ci2 = model.csr(n, extra_s, extra_d)
    a = model.color(ro, ci, seed=9, max_iter=0)
    b = model.color(ro2, ci2, seed=9, max_iter=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_model_edge_cases():
    c, trace, left = model.color(np.zeros(6, np.int32), np.zeros(0, np.int32), max_iter=0)
    assert list(trace) == [5] and left == 0 and (c == 1).all()
    c, trace, left = model.color(np.zeros(1, np.int32), np.zeros(0, np.int32), max_iter=0)
    assert len(trace) == 0 and left == 0 and len(c) == 0
    ro, ci = np.array([0, 1], np.int32), np.array([0], np.int32)     # one vertex, one self-loop
    c, trace, left = model.color(ro, ci, max_iter=0)
    assert list(c) == [1] and list(trace) == [1]
