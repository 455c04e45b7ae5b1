"""GPU suite (-m gpu): the backward of the neighbour feature aggregation (mgx_aggbwd_*).  Every check asserts that the
fused path (mgx_aggbwd_run), the operator path (mgx_aggbwd_enact) and the numpy model (tests/aggbwd_model.py) agree on the float32
BITS, that transpose() is the model's arrays, the stats, launches and host waits of the header's table, a repeat run that allocates
nothing, and a sentinel-filled GX whose padding columns stay untouched."""
import os

import numpy as np
import pytest

from tests import agg_model as fwd
from tests import aggbwd_cases as cases
from tests import aggbwd_model as model
from tests.grid_cus import one_cu_context

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["bfs_test.mtx", "kcore_test.mtx", "pr_test.mtx", "sssp_test.mtx", "synthetic_dup.mtx"]
SENTINEL = np.float32(-12345.678)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, who):
    assert got.dtype == np.float32 and got.shape == want.shape, (who, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d of %d elements differ in their bits" % (who, int((_bits(got) != _bits(want)).sum()), want.size)


class _Device:
    """GY, X and GX as torch tensors with leading dimensions and base offsets of the test's choosing; GX pre-filled with a sentinel"""

    def __init__(self, torch, gy, x_rows, x=None, ldgy=None, ldgx=None, gyoff=0, gxoff=0):
        F = gy.shape[1]
        self.F, self.T, self.ldgy, self.ldgx, self.gxoff = F, x_rows, ldgy or F, ldgx or F, gxoff
        h = np.zeros((max(gy.shape[0], 1), self.ldgy), dtype=np.float32)
        h[:gy.shape[0], :F] = gy
        self.gybuf = torch.zeros(gyoff + h.size + 4, dtype=torch.float32, device="cuda")
        self.gybuf[gyoff:gyoff + h.size] = torch.from_numpy(h.ravel()).cuda()
        self.gy = self.gybuf[gyoff:]
        self.gxbuf = torch.full((gxoff + max(x_rows, 1) * self.ldgx + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
        self.gx = self.gxbuf[gxoff:]
        self.x = None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.torch = torch

    def kwargs(self):
        return dict(gy=self.gy, x=self.x, out=self.gx, ldgy=self.ldgy, ldx=self.F, ldgx=self.ldgx, x_rows=self.T, feats=self.F)

    def vector(self):
        return fwd.is_vector(self.F, self.ldgy, self.ldgx, self.gy.data_ptr(), self.gx.data_ptr())

    def check_padding(self, who):
        """everything of GX's buffer but GX[:x_rows, :F] still holds the sentinel; then the sentinel goes back everywhere"""
        self.torch.cuda.synchronize()
        all_ = self.gxbuf.cpu().numpy()
        body = all_[self.gxoff:self.gxoff + self.T * self.ldgx].reshape(self.T, self.ldgx) if self.T else np.zeros((0, self.ldgx), np.float32)
        assert (all_[:self.gxoff] == SENTINEL).all() and (all_[self.gxoff + self.T * self.ldgx:] == SENTINEL).all(), who
        assert (body[:, self.F:] == SENTINEL).all(), who
        self.gxbuf.fill_(float(SENTINEL))


def _check(gp, want, gy, builds, dev=None, x=None, operator=True, fplan=(False, False), **how):
    """builds: (this run builds a transpose, the repeat run builds one); fplan: the same for the forward rows' plan (max / min).
    how: op, weighted, rows, block, hop"""
    import mini_amd
    ws = want["stats"]
    op = how.get("op", "sum")
    args = dict(dev.kwargs(), **how) if dev else dict(gy=gy, x=x, x_rows=ws["rows"], **how)
    vec = dev.vector() if dev else fwd.is_vector(gy.shape[1], gy.shape[1], gy.shape[1])
    c, g, tiles = fwd.shape(gy.shape[1], vec)
    known = dict(rows=ws["rows"], entries=ws["entries"], feats=ws["feats"], team_width=g, col_tiles=tiles, vector=int(vec), seg=ws["seg"])

    def after(who, s, fused=None):
        _same(gp.result(), want["gx"], who)
        off, row, pos = gp.transpose()
        assert np.array_equal(off, want["t_off"]) and np.array_equal(pos, want["t_pos"]) and np.array_equal(row, want["t_row"]), who
        if dev:
            dev.check_padding(who)
        assert {k: s[k] for k in model.STAT_KEYS} == known, (who, s, known)
        if fused is not None:
            b, f = fused
            expect = model.fused_counts(ws["rows"], want["bins"]["long"], b, ws["entries"], want["longest"], op in ("max", "min"), want["fwd_rows"],
                                        want["fwd_long"], f, op == "mean")
            assert (s["launches"], s["host_waits"], s["built"]) == expect + (int(b and ws["rows"] > 0),), (who, s, expect)       # (no rows: nothing runs)
            bins = gp.bins()
            assert {k: bins[k] for k in model.BIN_KEYS} == want["bins"] and bins["seg"] == ws["seg"], (who, bins, want["bins"])

    s1 = gp.run(**args)
    print("fused", s1)
    after("fused", s1, (builds[0], fplan[0]))
    before = mini_amd.lib.mgx_device_allocations()
    s2 = gp.run(**args)                                          # a repeat run: the same bits and stats, nothing allocated
    assert mini_amd.lib.mgx_device_allocations() == before
    after("fused, repeated", s2, (builds[1], fplan[1]))
    if operator:
        so = gp.enact(**args)
        print("operator", so)
        after("operator path", so)
        assert so["launches"] == (2 if op in ("max", "min") and want["fwd_rows"] else 1) * (ws["rows"] > 0)
        s3 = gp.run(**args)                                      # fused behind the operator path on one handle
        after("fused behind the operator path", s3, (builds[1], fplan[1]))
        assert s3 == s2
    return s1


def _graph_check(ctx, ro, ci, feats, op="sum", w=None, seg=fwd.SEG, torch=None, layout=None, seed=0, gy=None, x=None, x_rows=None, **kw):
    """a fresh graph and handle over (ro, ci[, w]): out-rows; layout: _Device's ldgy / ldgx / gyoff / gxoff (needs torch)"""
    import mini_amd
    n = len(ro) - 1
    x_rows = n if x_rows is None else x_rows
    gy = cases.features(n, feats, seed) if gy is None else gy
    if op in ("max", "min") and x is None:
        x = cases.features(x_rows, feats, seed + 500)
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    gp = mini_amd.AggregateGradProblem(g)
    dev = _Device(torch, gy, x_rows, x, **(layout or {})) if torch is not None else None
    want = model.backward(ro, ci, gy, op, w, seg=seg, x=x, x_rows=x_rows, vector=dev.vector() if dev else None)
    minmax = op in ("max", "min") and n > 0
    s = _check(gp, want, gy, (True, False), dev, x=x, fplan=(minmax, False), op=op, weighted=w is not None, **kw)
    gp.close()
    g.close()
    return want, s


@pytest.mark.parametrize("op", ["sum", "max"])
def test_transposed_row_lengths(gpu_ctx, monkeypatch, op):
    """in-degrees 0 .. 321 at MGX_AGG_SEG=64, each between a column without entries and a column of one; forward rows both short
    and long, so that the winners' items and fold run too"""
    monkeypatch.setenv("MGX_AGG_SEG", "64")
    ro, ci = cases.graph_cols(cases.IN_DEGREES, seed=1, long_rows=(3, 9))
    want, s = _graph_check(gpu_ctx, ro, ci, 8, op, cases.weights(len(ci), 1), seg=64, seed=1)
    assert want["fwd_long"] >= 2 and want["bins"]["long"] == 4 and s["seg"] == 64
    assert sorted(set(np.diff(want["t_off"][:3 * len(cases.IN_DEGREES)])[1::3])) == sorted(cases.IN_DEGREES)
    want, s = _graph_check(gpu_ctx, ro, ci, 5, op, None, seg=64, seed=2)
    plain = model.backward(ro, ci, cases.features(len(ro) - 1, 5, 2), "sum", None, seg=512, x_rows=len(ro) - 1)
    if op == "sum":
        assert not np.array_equal(_bits(want["gx"]), _bits(plain["gx"]))          # a kernel without the segment tree gives other bits


@pytest.mark.parametrize("op", ["sum", "mean", "min"])
def test_star_pointing_inward(gpu_ctx, op):
    """one column of 100 000 in-entries: 391 items at the default seg, six merge passes of the sort; row 1 is a long forward row"""
    ro, ci = cases.star_in()
    want, s = _graph_check(gpu_ctx, ro, ci, 4, op, cases.weights(len(ci), 4), seed=4, operator=op != "mean")
    assert want["longest"] == 100000 and want["bins"]["long"] == 1 and want["fwd_long"] == 1
    assert s["launches"] == 3 + 10 + 6 + {"sum": 0, "mean": 1, "min": 5}[op]


def test_stability(monkeypatch, gpu_ctx, torch_mod, built):
    """case (a) twice on fresh handles and once on one compute unit: the same bits and the same t_pos each time"""
    monkeypatch.setenv("MGX_AGG_SEG", "64")
    ro, ci, gy = cases.stability_case(4)
    w1, _ = _graph_check(gpu_ctx, ro, ci, 4, gy=gy, seg=64)
    w2, _ = _graph_check(gpu_ctx, ro, ci, 4, gy=gy, seg=64, operator=False)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        w3, _ = _graph_check(ctx, ro, ci, 4, gy=gy, seg=64, operator=False)
        lengths = np.random.default_rng(7).integers(0, 6, 20000)                 # and the grid-stride loops on 8 workgroups
        lengths[[5, 777]] = [300, 257]
        big = cases.graph_rows(lengths, seed=7)
        _graph_check(ctx, *big, 4, "max", seg=64, operator=False, seed=1)
        _graph_check(ctx, *big, 3, "mean", seg=64, operator=False, seed=2)
    assert np.array_equal(_bits(w1["gx"]), _bits(w3["gx"])) and np.array_equal(w1["t_pos"], w2["t_pos"])


@pytest.mark.parametrize("feats", cases.FEATS)
def test_team_widths(gpu_ctx, torch_mod, feats):
    ro, ci = cases.graph_cols([0, 1, 2, 7, 70], seed=feats, rows=20)
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", cases.weights(len(ci), feats), seed=feats)
    c, g, tiles = fwd.shape(feats, feats % 4 == 0)
    assert (s["vector"], s["team_width"], s["col_tiles"]) == (int(feats % 4 == 0), g, tiles)
    _graph_check(gpu_ctx, ro, ci, feats, "max", None, torch=torch_mod, layout=dict(ldgy=feats + 4, ldgx=feats + 8), seed=feats, operator=False)
    _graph_check(gpu_ctx, ro, ci, feats, "mean", None, torch=torch_mod, layout=dict(ldgy=feats + 4, ldgx=feats + 8), seed=feats, operator=False)


@pytest.mark.parametrize("layout, vector", [(dict(ldgy=9), 0), (dict(ldgx=10), 0), (dict(gyoff=1), 0), (dict(gxoff=1), 0), (dict(ldgy=12), 1),
                                            (dict(ldgy=12, ldgx=16, gyoff=4, gxoff=8), 1), (dict(), 1)])
def test_alignment_gates(gpu_ctx, torch_mod, layout, vector):
    """each gate failing alone sends the run to the scalar path, with the same bits"""
    ro, ci = cases.graph_cols([0, 1, 2, 7, 70, 9, 300], seed=3, rows=30)
    for op in ("sum", "mean", "max"):
        want, s = _graph_check(gpu_ctx, ro, ci, 8, op, cases.weights(len(ci), 3), torch=torch_mod, layout=layout, seed=3, operator=op == "sum")
        assert s["vector"] == vector and s["team_width"] == (2 if vector else 8)
        plain = model.backward(ro, ci, cases.features(len(ro) - 1, 8, 3), op, cases.weights(len(ci), 3), x=cases.features(len(ro) - 1, 8, 503),
                               x_rows=len(ro) - 1)
        assert np.array_equal(_bits(want["gx"]), _bits(plain["gx"]))              # the path does not enter the definition


@pytest.mark.parametrize("x_rows", cases.X_ROWS)
def test_x_row_counts(gpu_ctx, x_rows):
    """the last partial team group of a wave at G = 16 (4 transposed rows a pass) and G = 1 (64 a pass)"""
    n = x_rows
    lengths = np.random.default_rng(x_rows).integers(0, 10, n)
    ro, ci = cases.graph_rows(lengths, seed=x_rows)
    for feats in (64, 1):
        want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", seed=x_rows, operator=feats == 1)
        assert s["team_width"] == (16 if feats == 64 else 1) and s["rows"] == x_rows
    want, s = _graph_check(gpu_ctx, ro, ci, 4, "sum", seed=x_rows, x_rows=n + 3, operator=False)      # X had more rows than the graph: +0.0 behind
    assert (_bits(want["gx"][n:]) == 0).all() and s["rows"] == n + 3


@pytest.mark.parametrize("op", fwd.OPS)
@pytest.mark.parametrize("weighted", [False, True])
def test_ops(gpu_ctx, op, weighted):
    ro, ci = cases.graph_rows([0, 1, 2, 7, 70, 300, 5, 513, 64, 0, 33], seed=11, n=120)
    w = cases.weights(len(ci), 11) if weighted else None
    for feats in (8, 3):
        want, s = _graph_check(gpu_ctx, ro, ci, feats, op, w, seed=11)
        assert want["fwd_long"] == 2
    if op == "mean":                                                              # (b): the division comes before the weight
        ro, ci, wb, gy = cases.mean_case(8)
        _graph_check(gpu_ctx, ro, ci, 8, "mean", wb if weighted else None, gy=gy)
    if op == "sum" and weighted:                                                  # (c): no fused multiply-add
        for feats in (4, 1, 7):
            ro, ci, wc, gy = cases.fma_case(feats)
            want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", wc, gy=gy)
            assert (_bits(want["gx"]) == 0).all()
    # a graph uploaded without weights holds 1.0 for every entry: weighted is legal and gives the unweighted bits
    import mini_amd
    ro, ci = cases.graph_rows([3, 9, 0, 70], seed=12, n=80)
    gy, x = cases.features(80, 8, 12), cases.features(80, 8, 13)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    gp = mini_amd.AggregateGradProblem(g)
    gp.run(gy, op, weighted=True, x=x)
    _same(gp.result(), model.backward(ro, ci, gy, op, x=x, x_rows=80)["gx"], "weights of 1.0")
    gp.close()
    g.close()


@pytest.mark.parametrize("op", ["max", "min"])
def test_winners(gpu_ctx, monkeypatch, op):
    """(d) at seg 64: ties inside a segment and across the boundary, +0 against -0, a NaN first and a NaN later, duplicate entries
    and a self-loop"""
    monkeypatch.setenv("MGX_AGG_SEG", "64")
    for feats in (4, 3):
        ro, ci, x = cases.tie_case(feats, op)
        want, s = _graph_check(gpu_ctx, ro, ci, feats, op, None, seg=64, x=x, seed=3)
        assert (want["win"][0] == 10).all() and (_bits(want["gx"][[20, 70, 129, 131]]) == 0).all()
        _graph_check(gpu_ctx, ro, ci, feats, op, np.abs(cases.weights(len(ci), 5)), seg=64, x=x, seed=3, operator=False)


def test_sources(gpu_ctx):
    """out-rows; in-rows after build_csc() against the model on the CSC's own arrays and row values; without a CSC refused"""
    import mini_amd
    ro, ci = cases.fwd_cases.random_digraph(500, 6000, 21)
    w = cases.weights(len(ci), 21)
    gy, x = cases.features(500, 12, 21), cases.features(500, 12, 22)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    gp = mini_amd.AggregateGradProblem(g)
    for go in (gp.run, gp.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go(gy, rows="in")
        assert err.value.status == mini_amd.MGX_E_INVALID and "CSC" in str(err.value)
    _check(gp, model.backward(ro, ci, gy, "sum", w, x_rows=500), gy, (True, False), op="sum", weighted=True, rows="out")
    g.build_csc()
    co, ri, rv = g.csc_arrays()
    for k, (op, weighted) in enumerate((("sum", True), ("mean", False), ("max", True))):
        want = model.backward(co, ri, gy, op, rv if weighted else None, x=x, x_rows=500)
        _check(gp, want, gy, (k == 0, False), x=x, fplan=(op == "max", False), op=op, weighted=weighted, rows="in")    # the in-rows' own, built once
    want = model.backward(ro, ci, gy, "min", w, x=x, x_rows=500)
    _check(gp, want, gy, (False, False), x=x, fplan=(True, False), op="min", weighted=True, rows="out")       # the out-rows' is still there
    gp.close()
    g.close()


def _block_check(ctx, ro, ci, w, seeds, fanouts, feats, seed, sampler="run", seg=fwd.SEG, ops=(("sum", True), ("mean", False), ("max", True))):
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    gp = mini_amd.AggregateGradProblem(g)
    st = getattr(sp, sampler)(seeds, fanouts, seed=seed)
    off, rows, cols, pos = sp.hop_offsets(), sp.row_offsets(), sp.cols(), sp.entry_pos()
    V = st["vertices"]
    x = cases.features(V, feats, seed + 1)
    whole = -1 in fanouts
    for k, hop in enumerate([None] + list(range(len(fanouts)))):
        part = rows if hop is None else rows[off[hop]:off[hop + 1] + 1]
        if V == 0:
            part = np.zeros(1, dtype=np.int32)
        gy = cases.features(len(part) - 1, feats, seed + k)
        for op, weighted in ops:
            want = model.backward(part, cols, gy, op, w[pos] if weighted else None, seg=seg, x=x, x_rows=V)
            named = np.zeros(V, dtype=bool)
            named[cols[part[0]:part[-1]]] = True
            assert (_bits(want["gx"][~named]) == 0).all()                       # a vertex that is nobody's neighbour gets +0.0
            minmax = op in ("max", "min") and whole and len(part) > 1
            _check(gp, want, gy, (True, True), x=x, fplan=(minmax, minmax), op=op, weighted=weighted, block=sp, hop=hop, operator=k < 2)
    gp.close()
    sp.close()
    g.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_blocks(gpu_ctx, oracle, name):
    """a sampling run's rows read on the device: every hop and all rows, GX by local id, the weights through entry_pos"""
    n, ro, ci, w, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=True, random_w=True)
    for fanouts, sampler in (([3, 2], "run"), ([-1, 1], "run"), ([3, 2], "enact")):
        _block_check(gpu_ctx, ro, ci, np.asarray(w, dtype=np.float32), np.arange(0, n, 2), fanouts, 8, seed=5, sampler=sampler)


def test_blocks_rmat(gpu_ctx, oracle, monkeypatch):
    import mini_amd
    monkeypatch.setenv("MGX_AGG_SEG", "64")                                     # R-MAT-12's hubs are long rows then, both ways
    n, ro, ci, w = oracle.rmat_csr(12, 16, 512, undir=False)
    w = cases.weights(len(ci), 12)
    seeds = np.random.default_rng(12).integers(0, n, 200)
    for fanouts, sampler in (([3, 2], "run"), ([-1, 1], "enact"), ([-1, 1], "run")):
        _block_check(gpu_ctx, ro, ci, w, seeds, fanouts, 16, seed=3, sampler=sampler, seg=64, ops=(("sum", True), ("max", False)))
    # a block of another graph, a hop the run does not have, too few rows
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    g2 = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    sp, gp, other = mini_amd.NeighborSampleProblem(g), mini_amd.AggregateGradProblem(g), mini_amd.AggregateGradProblem(g2)
    st = sp.run(seeds, [2, 2], seed=1)
    gy = cases.features(st["rows"], 4, 1)
    for call, word in ((lambda: other.run(gy, block=sp), "another graph"), (lambda: gp.run(gy, block=sp, hop=2), "hop"),
                       (lambda: gp.run(gy, block=sp, hop=-2), "hop"), (lambda: gp.run(gy, block=sp, x_rows=st["vertices"] - 1), "x_rows")):
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and word in str(err.value), str(err.value)
    for h in (other, gp, sp):
        h.close()
    g2.close()
    g.close()


def test_transpose_is_kept_across_feats_and_ops(gpu_ctx):
    import mini_amd
    ro, ci = cases.graph_cols([300, 0, 5, 1000, 256, 257], seed=31, rows=300, long_rows=(2,))
    n = len(ro) - 1
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    gp = mini_amd.AggregateGradProblem(g)
    gy8, gy5, x5 = cases.features(n, 8, 31), cases.features(n, 5, 32), cases.features(n, 5, 33)
    s = gp.run(gy8)
    assert (s["launches"], s["host_waits"], s["built"]) == (3 + 10, 2, 1)
    s = gp.run(gy5, "max", x=x5)                                                  # another F and op find it; the forward rows' plan is new
    assert (s["launches"], s["host_waits"], s["built"]) == (3 + 1 + 2, 1, 0)
    _same(gp.result(), model.backward(ro, ci, gy5, "max", x=x5, x_rows=n)["gx"], "another F and op on the kept transpose")
    s = gp.run(gy5, "min", x=x5)
    assert (s["launches"], s["host_waits"], s["built"]) == (4, 0, 0)
    s = gp.run(gy8, "mean")
    assert (s["launches"], s["host_waits"], s["built"]) == (4, 0, 0)
    _same(gp.result(), model.backward(ro, ci, gy8, "mean", x_rows=n)["gx"], "mean on the kept transpose")
    s = gp.run(gy8, x_rows=n + 2)                                                 # another x_rows is another transpose
    assert s["built"] == 1 and s["rows"] == n + 2
    gp.close()
    g.close()


def test_handle_reuse_and_the_forward_beside_it(gpu_ctx):
    """on ONE handle a large block, a small one and the large one again, each what a fresh handle gives; the forward handle's
    result() is unchanged by the backward runs between"""
    import mini_amd
    ro, ci = cases.fwd_cases.random_digraph(3000, 40000, 41)
    w = cases.weights(len(ci), 41)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    one, ap = mini_amd.AggregateGradProblem(g), mini_amd.AggregateProblem(g)
    large, small = np.arange(0, 2000, 2), np.arange(2001, 2100, 7)
    for seeds, fanouts, feats in ((large, [-1, 3], 32), (small, [2, 2], 5), (large, [-1, 3], 32), (small, [-1], 64)):
        st = sp.run(seeds, fanouts, seed=9)
        x = cases.features(st["vertices"], feats, 9)
        gy = cases.features(st["rows"], feats, 10)
        ap.run(x, "max", weighted=True, block=sp)
        y = ap.result()
        want = model.backward(sp.row_offsets(), sp.cols(), gy, "max", w[sp.entry_pos()], x=x, x_rows=st["vertices"])
        s = one.run(gy, "max", weighted=True, block=sp, x=x)
        _same(one.result(), want["gx"], "one handle")
        _same(ap.result(), y, "the forward's result behind a backward run")
        _same(y, model.winners(sp.row_offsets(), sp.cols(), x, "max", w[sp.entry_pos()])[1], "the forward is the model's")
        fresh = mini_amd.AggregateGradProblem(g)
        assert fresh.run(gy, "max", weighted=True, block=sp, x=x) == s
        _same(fresh.result(), want["gx"], "fresh handle")
        fresh.enact(gy, "max", weighted=True, block=sp, x=x)
        _same(fresh.result(), want["gx"], "operator behind fused")
        fresh.close()
    one.close()
    one.close()
    ap.close()
    sp.close()
    g.close()


def test_edges_and_refusals(gpu_ctx, torch_mod):
    import mini_amd
    want, s = _graph_check(gpu_ctx, *cases.fwd_cases.empty(0), 4)                 # n = 0
    assert (s["launches"], s["host_waits"], s["rows"]) == (0, 0, 0)
    want, s = _graph_check(gpu_ctx, *cases.fwd_cases.empty(50), 4, "mean")        # m = 0: zeros, nothing to transpose
    assert (_bits(want["gx"]) == 0).all() and (s["launches"], s["host_waits"]) == (2, 0)
    ro, ci = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)     # one self-loop: no sort
    want, s = _graph_check(gpu_ctx, ro, ci, 4, "max", np.array([2.5], np.float32))
    assert (s["launches"], s["host_waits"]) == (1 + 6 + 1 + 2, 2)
    ro, ci = np.array([0, 6, 6, 9], dtype=np.int32), np.array([1, 1, 1, 2, 1, 1, 0, 0, 0], dtype=np.int32)     # duplicate entries
    _graph_check(gpu_ctx, ro, ci, 5, "sum")
    _graph_check(gpu_ctx, ro, ci, 5, "min")
    # every refusal, before any device work; the getters after a refusal
    ro, ci = cases.fwd_cases.random_digraph(100, 600, 51)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    gp = mini_amd.AggregateGradProblem(g)
    lib, h = mini_amd.lib, gp._h
    buf = torch_mod.zeros(4 * 100 * 8 + 64, dtype=torch_mod.float32, device="cuda")
    gyp = buf.data_ptr()
    xp, gxp = gyp + 4 * 800, gyp + 4 * 1600                                       # touching ranges are legal
    ok = dict(source=0, block=None, hop=-1, gy=gyp, ldgy=8, feats=8, op=2, weighted=0, x=xp, ldx=8, x_rows=100, gx=gxp, ldgx=8)
    bad = [(dict(feats=0), "feats"), (dict(feats=65537, ldgy=65537, ldx=65537, ldgx=65537), "feats"), (dict(ldgy=7), "ldgy"), (dict(ldgx=7), "ldgx"),
           (dict(ldx=7), "ldx"), (dict(gy=None), "NULL"), (dict(gx=None), "NULL"), (dict(x=None), "d_x"), (dict(op=4), "op"), (dict(source=3), "source"),
           (dict(source=1), "CSC"), (dict(source=2), "block"), (dict(x_rows=99), "x_rows"), (dict(gx=gyp), "GY and GX"), (dict(gx=xp + 4 * 8 * 99), "X and GX"),
           (dict(x=gyp + 4 * 7), "GY and X"), (dict(gy=gxp + 4 * 7), "GY and GX")]

    def call(go, a):
        return go(h, a["source"], a["block"], a["hop"], a["gy"], a["ldgy"], a["feats"], a["op"], a["weighted"], a["x"], a["ldx"], a["x_rows"], a["gx"],
                  a["ldgx"], None)

    for go in (lib.mgx_aggbwd_run, lib.mgx_aggbwd_enact):
        assert call(go, ok) == 0
        assert call(go, dict(ok, op=0, x=None)) == 0                              # d_x may be NULL for sum
        assert call(go, dict(ok, op=1, x=gyp)) == 0                               # and is ignored where it is not read, overlapping or not
        assert lib.mgx_aggbwd_bins(h, (mini_amd._lib._i64 * 5)()) == (0 if go is lib.mgx_aggbwd_run else mini_amd.MGX_E_INVALID)
        before = mini_amd.lib.mgx_device_allocations()
        for change, word in bad:
            status = call(go, dict(ok, **change))
            assert status == mini_amd.MGX_E_INVALID and word.encode() in lib.mgx_last_error(), (change, lib.mgx_last_error())
            for getter in (gp.result, gp.bins, gp.phase_ms, gp.transpose):         # a refused call leaves nothing to the getters
                with pytest.raises(mini_amd.MgxError) as err:
                    getter()
                assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
        assert mini_amd.lib.mgx_device_allocations() == before                   # refused before any device work
    gp.close()
    g.close()


def test_timing_changes_nothing(gpu_ctx):
    import mini_amd
    ro, ci = cases.graph_cols([300, 0, 5, 1000, 7, 257] * 5, seed=61, rows=100, long_rows=(1,))
    n = len(ro) - 1
    gy, x = cases.features(n, 16, 61), cases.features(n, 16, 62)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    gp = mini_amd.AggregateGradProblem(g)
    with pytest.raises(mini_amd.MgxError):
        gp.phase_ms()
    gp.run(gy, "max", x=x)
    plain, gx = gp.run(gy, "max", x=x), gp.result()
    assert gp.phase_ms() == dict.fromkeys(mini_amd.AggregateGradProblem.PHASES, 0.0)
    gp.set_timing(True)
    timed = gp.run(gy, "max", x=x)
    assert timed == plain
    _same(gp.result(), gx, "timed")
    ms = gp.phase_ms()
    assert set(ms) == set(mini_amd.AggregateGradProblem.PHASES) and min(ms["winners"], ms["rows"], ms["items"], ms["fold"]) > 0.0
    _same(gx, model.backward(ro, ci, gy, "max", x=x, x_rows=n)["gx"], "model")
    gp.close()
    g.close()


def test_another_stream(gpu_ctx, torch_mod):
    import mini_amd
    ro, ci = cases.graph_cols([300, 0, 5, 70, 7, 257], seed=71, rows=60)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _graph_check(ctx, ro, ci, 12, "sum", cases.weights(len(ci), 71), seed=71)
        _graph_check(ctx, ro, ci, 12, "max", cases.weights(len(ci), 71), seed=72, operator=False)
    finally:
        ctx.close()
