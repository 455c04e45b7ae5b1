"""GPU suite (-m gpu): betweenness centrality on its thresholds ("BC: which test stands on which edge").  The inputs are
tests/bc_cases.py's, each built for one host decision or kernel edge of include/mgx/bc_fused.hpp; tests/test_bc_cases_cpu.py proves
without a GPU that each case stands where it claims.

What a case is compared with (bc_cases.expected):
  closed   closed forms; every operation on the way is exact, so the fused path must match BIT FOR BIT;
  exact    tests/bc_exact.py (integers and fractions, rounded once): zeros exact, elsewhere
           |got - exact| <= (rtol(L, R, S) / 2 + 2^-53) * exact -- ONE implementation's share of 3.11's bound plus the reference's
           rounding;
  model    tests/bc_model.py by test_gpu_bc.py's rule (two implementations), NaN and inf at the same vertices.
Per case: fused against the expectation, two fused runs bit-equal, chain off on a fresh handle bit-equal to chain on, the stats, the
class counts and switches of info(), one host wait; the operator path too where a host round trip per level is affordable."""
import numpy as np
import pytest

from tests import bc_cases as cases
from tests import bc_exact as exact
from tests import bc_model as model
from tests.test_gpu_bc import _arrays, _bit_equal, _close, _graph

pytestmark = pytest.mark.gpu

STATS = ("sources", "levels", "reached", "inexact", "overflow")


def _against(tag, got, w, c, rel=None):
    """one path's arrays against the case's expectation"""
    assert got["labels"].dtype == np.int32 and got["sigma"].dtype == np.float64
    assert np.array_equal(got["labels"], w["labels"]), tag + ": labels"
    assert np.array_equal(got["sigma"], w["sigma"], equal_nan=True), tag + ": sigma"
    for k in ("delta", "bc"):
        if c["want"] == "model":
            _close("%s: %s" % (tag, k), got[k], w[k], w["rel"])
        elif rel is None and c["want"] == "closed":
            assert np.array_equal(got[k], w[k]), "%s: %s differs from the closed form at %d vertices" % (tag, k, int((got[k] != w[k]).sum()))
        else:
            exact.close("%s: %s" % (tag, k), got[k], w[k], rel if rel is not None else w["rel"])


def _check(ctx, monkeypatch, name, operator=True, sigma_below_two53=True, host_waits=1, chain_off=True):
    """fused (twice), chain off, the operator path; returns (fused arrays, fused stats, info)"""
    import mini_amd
    c = cases.get(name)
    w = cases.expected(name)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    o = cases.opts(c["env"])
    sym = c["symmetric"]
    if sigma_below_two53:
        assert float(w["sigma"].max()) < model.TWO53                          # the sigma sums are exact in any order
    L, R, S = w["stats"][1], max(w["longest_in"], w["longest_out"]), len(c["sources"])
    g = _graph(ctx, c["ro"], c["ci"], csc=not sym)
    bp = mini_amd.BcProblem(g)
    sf = bp.run(c["sources"], sym)
    af = _arrays(bp)
    info = bp.info()
    sf2 = bp.run(c["sources"], sym)
    _bit_equal(name + ": two fused runs", _arrays(bp), af)
    _against(name + ": fused", af, w, c)
    assert [sf[k] for k in STATS] == w["stats"] == [sf2[k] for k in STATS], (sf, sf2, w["stats"])
    assert sf["host_waits"] == host_waits and sf2["host_waits"] == 1, (sf, sf2)
    assert sf["used_csc"] == int(not sym)
    assert (info["longest_in"], info["longest_out"]) == (w["longest_in"], w["longest_out"]), info
    rin = cases.class_counts(c["ro"] if sym else cases.in_offsets(c["ro"], c["ci"]), o)
    rout = cases.class_counts(c["ro"], o)
    assert (info["in_lane"], info["in_wave"], info["in_huge"], info["in_segments"]) == rin, (info, rin)
    assert (info["out_lane"], info["out_wave"], info["out_huge"], info["out_segments"]) == rout, (info, rout)
    assert (info["lane_max"], info["huge_min"], info["seg"], info["chain"]) == (o["lane_max"], o["huge_min"], o["seg"], o["chain"]), info
    assert info["levels"] == int(w["labels"].max()) + 1, info                 # (info: the LAST source's depth and chain launches)
    if S == 1:
        assert info["chain_launches"] == sf["chain_launches"], (info, sf)
    if operator:
        so = bp.enact(c["sources"], sym)
        ao = _arrays(bp)
        # (the operator path adds with atomics in the hardware's order: never bit for bit, one implementation's bound where the
        #  truth is finite)
        _against(name + ": operator", ao, w, c, rel=None if c["want"] == "model" else exact.bound(L, R, S))
        if np.isfinite(w["delta"]).all():
            _close(name + ": operator against fused: bc", ao["bc"], af["bc"], model.rtol(L, R, S))
        assert [so[k] for k in STATS] == w["stats"], (so, w["stats"])
    bp.close()
    if chain_off:
        with monkeypatch.context() as m:
            m.setenv("MGX_BC_CHAIN", "0")
            off = mini_amd.BcProblem(g)
            s0 = off.run(c["sources"], sym)                                   # (the handle reads the switches at its first run)
        _bit_equal(name + ": chain off against chain on", _arrays(off), af)
        assert s0["chain_launches"] == 0 and off.info()["chain"] == 0 and s0["host_waits"] == host_waits, s0
        if "widths" in c and len(c["sources"]) == 1:
            assert s0["launches"] == cases.predicted(c["widths"], 0, c["levels"], rin[2] > 0, rout[2] > 0, not sym)[2], s0
        off.close()
    g.close()
    return af, sf, info


@pytest.mark.parametrize("name", cases.names("key_bits"))
def test_key_bits(gpu_ctx, monkeypatch, name):
    """K = (levels + 2) * 4 on both sides of 256 and 4096: one bit too few in the sort puts the deepest level in front of level 0"""
    af, sf, info = _check(gpu_ctx, monkeypatch, name)
    c = cases.get(name)
    assert sf["levels"] == c["levels"] + (0 if c["symmetric"] else 1)
    if "leaves" in c:
        assert info["in_huge"] == 1 and info["in_segments"] == 2 and (af["labels"][c["path_n"]:] == sf["levels"] - 1).all()


@pytest.mark.parametrize("name", cases.names("sigma_limits"))
def test_sigma_limits(gpu_ctx, monkeypatch, name):
    """sigma = 2^v: the flags at 2^53 and 2^1024, Q = 1 / sigma subnormal at n = 1024 (flushed, delta[1022] is 0 in place of 1)"""
    af, sf, info = _check(gpu_ctx, monkeypatch, name, sigma_below_two53=False)
    c = cases.get(name)
    assert (sf["inexact"], sf["overflow"]) == c["flags"]
    n = c["path_n"]
    if n <= 1024:
        assert af["sigma"][n - 1] == 2.0 ** (n - 1) and af["delta"][n - 2] == 1.0 and af["delta"][1] == n - 2
    elif n == 1025:
        assert np.isinf(af["sigma"][1024]) and not np.isnan(af["delta"]).any() and af["delta"][1022] == 1.0
    else:
        assert np.isnan(af["delta"][1:1025]).all() and af["delta"][0] == 0 and af["delta"][1025] == 0


@pytest.mark.parametrize("name", cases.names("class_edges"))
def test_class_edges(gpu_ctx, monkeypatch, name):
    """rows of 16 | 17, 8191 | 8192 | 8193, 16384 | 16385 entries under the default thresholds, against the exact reference"""
    af, sf, info = _check(gpu_ctx, monkeypatch, name)
    c = cases.get(name)
    assert info["longest_in"] == c["longest_in"]
    if c["symmetric"]:
        assert (info["in_wave"], info["in_huge"], info["in_segments"]) == (2, 4, 1 + 2 + 2 + 3), info
    else:
        assert (info["in_wave"], info["in_huge"], info["out_wave"], info["out_huge"], info["out_segments"]) == (0, 0, 2, 3, 5), info


@pytest.mark.parametrize("name", cases.names("plan"))
def test_plan(gpu_ctx, monkeypatch, name):
    """level widths of chain | chain + 1: the launches of both plan loops are the predicted ones"""
    af, sf, info = _check(gpu_ctx, monkeypatch, name)
    c = cases.get(name)
    fwd, bwd, launches = cases.predicted(c["widths"], cases.opts(c["env"])["chain"], c["levels"])
    assert sf["chain_launches"] == fwd + bwd and info["chain_launches"] == fwd + bwd, (sf, info, fwd, bwd)
    assert sf["launches"] == launches, (sf, launches)
    assert np.bincount(af["labels"]).tolist() == c["widths"]


def test_behind_the_trace(gpu_ctx, monkeypatch):
    """3000 wave rows on level 4100, past the traced 4096 levels: one workgroup's chain takes them, forward and backward"""
    af, sf, info = _check(gpu_ctx, monkeypatch, "behind_the_trace", operator=False)
    c = cases.get("behind_the_trace")
    assert sf["chain_launches"] > 0
    fwd, bwd, launches = cases.predicted(c["widths"], 1024, c["levels"])
    assert (sf["chain_launches"], sf["launches"]) == (fwd + bwd, launches), sf
    assert (af["sigma"][-60:] == 1000).all() and (af["labels"][4100:7100] == 4100).all()


def test_parity_back_edges(gpu_ctx, monkeypatch):
    """directed entries from level d onto d - 1, d - 3, d - 5 contribute exactly nothing"""
    af, sf, info = _check(gpu_ctx, monkeypatch, "parity_back_edges")
    assert np.array_equal(af["delta"], (40.0 - np.arange(41)) * (np.arange(41) > 0))


def test_bounds_growth(gpu_ctx, monkeypatch):
    """the symmetric path of 65 537 vertices fits the bounds the constructor made; 65 538 grows them behind a second host wait, once
    per handle; another graph's handle has bounds of its own"""
    import mini_amd
    small, big = cases.names("bounds_growth")
    assert not cases.get(small)["grows"] and cases.get(big)["grows"]
    _check(gpu_ctx, monkeypatch, small, operator=False, host_waits=1)
    af, sf, info = _check(gpu_ctx, monkeypatch, big, operator=False, host_waits=2)      # (the repeat inside: 1; chain off, a fresh handle: 2)
    assert sf["levels"] == 65538 and af["delta"][1] == 65536.0
    # a shallow source on a different small graph's handle
    c = cases.get("key_bits-sym-60")
    g = _graph(gpu_ctx, c["ro"], c["ci"])
    bp = mini_amd.BcProblem(g)
    st = bp.run(c["sources"], True)
    assert st["host_waits"] == 1 and st["levels"] == 60
    assert np.array_equal(bp.centrality(), cases.expected(c["name"])["bc"])
    bp.close()
    g.close()
