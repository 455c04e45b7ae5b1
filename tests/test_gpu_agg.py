"""GPU suite (-m gpu): neighbour feature aggregation (mgx_agg_*).  The fused path (mgx_agg_run), the operator path
(mgx_agg_enact) and the numpy model (tests/agg_model.py) agree on the float32 BITS -- every team width and column tile of both
paths, each alignment gate, row counts round the last team group of a wave and past one grid, the segment cut and the unroll's edges,
a row of 100 000 entries, four ops weighted and not, +-0, a row that tells a fused multiply-add, out-rows, in-rows and sampled blocks.
The run's stats, the bins, the launches and the host waits are exact; a repeat run gives the same and allocates nothing; padding
columns stay untouched."""
import os

import numpy as np
import pytest

from tests import agg_cases as cases
from tests import agg_model as model
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
    """X and Y as torch tensors with leading dimensions and base offsets of the test's choosing; Y pre-filled with a sentinel"""

    def __init__(self, torch, x, rows, ldx=None, ldy=None, xoff=0, yoff=0):
        F = x.shape[1]
        self.F, self.R, self.ldx, self.ldy, self.yoff = F, rows, ldx or F, ldy or F, yoff
        hx = np.zeros((max(x.shape[0], 1), self.ldx), dtype=np.float32)
        hx[:x.shape[0], :F] = x
        self.xbuf = torch.zeros(xoff + hx.size + 4, dtype=torch.float32, device="cuda")
        self.xbuf[xoff:xoff + hx.size] = torch.from_numpy(hx.ravel()).cuda()
        self.x = self.xbuf[xoff:]
        self.ybuf = torch.full((yoff + max(rows, 1) * self.ldy + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
        self.y = self.ybuf[yoff:]
        self.x_rows = x.shape[0]
        self.torch = torch

    def kwargs(self):
        return dict(x=self.x, out=self.y, ldx=self.ldx, ldy=self.ldy, x_rows=self.x_rows, feats=self.F)

    def vector(self):
        return model.is_vector(self.F, self.ldx, self.ldy, self.x.data_ptr(), self.y.data_ptr())

    def check_padding(self, who):
        """everything of Y's buffer but Y[:R, :F] still holds the sentinel; then the sentinel goes back everywhere"""
        self.torch.cuda.synchronize()
        all_ = self.ybuf.cpu().numpy()
        body = all_[self.yoff:self.yoff + self.R * self.ldy].reshape(self.R, self.ldy) if self.R else np.zeros((0, self.ldy), np.float32)
        assert (all_[:self.yoff] == SENTINEL).all() and (all_[self.yoff + self.R * self.ldy:] == SENTINEL).all(), who
        assert (body[:, self.F:] == SENTINEL).all(), who
        self.ybuf.fill_(float(SENTINEL))


def _check(ap, want, x, plan, dev=None, operator=True, operator_first=False, **how):
    """fused == operator path == model on the bits; stats, bins, launches and waits; the repeat run and its allocations; padding.
    plan: (this run builds a plan, the repeat run builds one).  how: op, weighted, rows, block, hop."""
    import mini_amd
    ws = want["stats"]
    args = dict(dev.kwargs(), **how) if dev else dict(x=x, **how)
    vec = dev.vector() if dev else model.is_vector(x.shape[1], x.shape[1], x.shape[1])
    c, g, tiles = model.shape(x.shape[1], vec)
    known = dict(rows=ws["rows"], entries=ws["entries"], feats=ws["feats"], team_width=g, col_tiles=tiles, vector=int(vec), seg=ws["seg"])

    def after(who, s=None, builds=None):
        _same(ap.result(), want["y"], who)
        if dev:
            dev.check_padding(who)
        if s is not None:
            assert {k: s[k] for k in model.RUN_KEYS} == known, (who, s, known)
        if builds is not None:
            assert (s["launches"], s["host_waits"]) == model.fused_counts(ws["rows"], ws["long_rows"], builds), (who, s, ws)
            b = ap.bins()
            assert {k: b[k] for k in model.BIN_KEYS} == want["bins"] and b["seg"] == ws["seg"], (who, b, want["bins"])

    if operator_first:
        after("operator path first", ap.enact(**args))
    s1 = ap.run(**args)
    print("fused", s1)
    after("fused", s1, plan[0])
    before = mini_amd.lib.mgx_device_allocations()
    s2 = ap.run(**args)                                          # a repeat run: the same bits and stats, nothing allocated
    assert mini_amd.lib.mgx_device_allocations() == before
    after("fused, repeated", s2, plan[1])
    if operator:
        so = ap.enact(**args)
        print("operator", so)
        after("operator path", so)
        s3 = ap.run(**args)                                      # fused behind the operator path on one handle
        after("fused behind the operator path", s3, plan[1])
        assert s3 == s2
    return s1


def _graph_check(ctx, ro, ci, feats, op="sum", w=None, seg=model.SEG, torch=None, layout=None, seed=0, x=None, **kw):
    """a fresh graph and handle over (ro, ci[, w]): out-rows; layout: _Device's ldx / ldy / xoff / yoff (needs torch)"""
    import mini_amd
    n = len(ro) - 1
    x = cases.features(n, feats, seed) if x is None else x
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    ap = mini_amd.AggregateProblem(g)
    dev = _Device(torch, x, n, **(layout or {})) if torch is not None else None
    vec = dev.vector() if dev else None
    want = model.aggregate(ro, ci, x, op, w, seg=seg, vector=vec)
    s = _check(ap, want, x, (True, False), dev, op=op, weighted=w is not None, **kw)
    ap.close()
    g.close()
    return want, s


@pytest.mark.parametrize("feats", cases.VECTOR_FEATS + cases.SCALAR_FEATS)
def test_team_widths(gpu_ctx, torch_mod, feats):
    """rows of 0, 1, 2, 7 and 70 entries at every team width and column tile of both paths, from host arrays and from tensors"""
    ro, ci = cases.graph_rows(cases.TEAM_ROWS * 3, seed=feats, n=80)
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", cases.weights(len(ci), feats), seed=feats)
    c, g, tiles = model.shape(feats, feats % 4 == 0)
    assert (s["vector"], s["team_width"], s["col_tiles"]) == (int(feats % 4 == 0), g, tiles)
    _graph_check(gpu_ctx, ro, ci, feats, "mean", None, torch=torch_mod, layout=dict(ldx=feats + 4, ldy=feats + 8), seed=feats, operator=False)


@pytest.mark.parametrize("layout, vector", [(dict(ldx=9), 0), (dict(ldy=10), 0), (dict(xoff=1), 0), (dict(yoff=1), 0), (dict(ldx=12), 1),
                                            (dict(ldx=12, ldy=16, xoff=4, yoff=8), 1), (dict(), 1)])
def test_alignment_gates(gpu_ctx, torch_mod, layout, vector):
    """each gate failing alone sends the run to the scalar path, with the same bits"""
    ro, ci = cases.graph_rows([0, 1, 2, 7, 70, 9, 300], seed=3, n=90)
    want, s = _graph_check(gpu_ctx, ro, ci, 8, "sum", cases.weights(len(ci), 3), torch=torch_mod, layout=layout, seed=3)
    assert s["vector"] == vector and s["team_width"] == (2 if vector else 8)
    plain = model.aggregate(ro, ci, cases.features(90, 8, 3), "sum", cases.weights(len(ci), 3))
    assert np.array_equal(_bits(want["y"]), _bits(plain["y"]))                  # the path does not enter the definition


@pytest.mark.parametrize("rows", [1, 3, 5, 63, 64, 65, 255, 256, 257])
def test_row_counts(gpu_ctx, rows):
    """the last partial team group of a wave at G = 16 (4 rows a pass) and G = 1 (64 rows a pass)"""
    lengths = np.random.default_rng(rows).integers(0, 10, rows)
    ro, ci = cases.graph_rows(lengths, seed=rows)
    for feats in (64, 1):
        want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", seed=rows, operator=feats == 1)
        assert s["team_width"] == (16 if feats == 64 else 1) and s["rows"] == rows


def test_grid_stride_on_one_compute_unit(monkeypatch, torch_mod, built):
    """8 workgroups: 20 000 rows are 313 passes of 64 rows at G = 1 and 5 000 passes at G = 16 for 32 waves"""
    lengths = np.random.default_rng(7).integers(0, 6, 20000)
    lengths[[5, 777, 19999]] = [300, 257, 600]                                  # and the items' and the fold's loops
    ro, ci = cases.graph_rows(lengths, seed=7)
    with one_cu_context(monkeypatch, torch_mod) as ctx:
        _graph_check(ctx, ro, ci, 4, "sum", seed=1, operator=False)
        _graph_check(ctx, ro, ci, 64, "max", seed=2, operator=False)
        _graph_check(ctx, ro, ci, 3, "mean", seed=3)


@pytest.mark.parametrize("feats", [1, 8, 5])
def test_segment_edges(gpu_ctx, monkeypatch, feats):
    """MGX_AGG_SEG=64: rows at the cut (63, 64, 65), at two segments (127, 128, 129) and of 64 x 5 + 1 entries, each between a row
    without entries and a row of one; the unroll's edges U - 1, U, U + 1, 2 U + 1"""
    monkeypatch.setenv("MGX_AGG_SEG", "64")
    ro, ci = cases.interleaved(cases.SEG_EDGE_ROWS, seed=feats)
    wants = {}
    for op in ("sum", "max"):
        # (sum: the handle's first successful call is the operator path's; the fused run behind it still builds its plan)
        wants[op], s = _graph_check(gpu_ctx, ro, ci, feats, op, cases.weights(len(ci), feats), seg=64, seed=feats, operator_first=op == "sum")
        assert (s["launches"], s["host_waits"]) == (5, 1)
        assert s["seg"] == 64 and wants[op]["bins"] == {"none": 50, "team": 7 + 2, "long": 5, "segments": 2 + 2 + 2 + 3 + 6}
    plain = model.aggregate(ro, ci, cases.features(len(ro) - 1, feats, feats), "sum", cases.weights(len(ci), feats), seg=512)
    assert not np.array_equal(_bits(wants["sum"]["y"]), _bits(plain["y"]))         # a kernel without the tree gives other bits
    U = model.UNROLL
    ro, ci = cases.interleaved([U - 1, U, U + 1, 2 * U + 1], seed=9)
    _graph_check(gpu_ctx, ro, ci, feats, "sum", cases.weights(len(ci), 9), seg=64, seed=9)
    monkeypatch.setenv("MGX_AGG_SEG", "100")                                    # clamps to 128: 127 and 128 are one fold, 129 is cut
    ro, ci = cases.interleaved(cases.SEG_EDGE_ROWS, seed=feats)
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", None, seg=128, seed=feats, operator=False)
    assert s["seg"] == 128 and want["bins"]["long"] == 2


def test_seg_is_read_once_per_handle(gpu_ctx, monkeypatch):
    """seg is part of the result: a handle keeps the MGX_AGG_SEG of its first call for both of its paths"""
    import mini_amd
    ro, ci = cases.interleaved(cases.SEG_EDGE_ROWS, seed=2)
    x = cases.features(len(ro) - 1, 8, 2)
    want = model.aggregate(ro, ci, x, "sum", seg=64)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    for first, second in (("enact", "run"), ("run", "enact")):
        monkeypatch.setenv("MGX_AGG_SEG", "64")
        ap = mini_amd.AggregateProblem(g)
        s = getattr(ap, first)(x)
        _same(ap.result(), want["y"], first)
        monkeypatch.setenv("MGX_AGG_SEG", "1024")
        for go in (second, first):
            s = getattr(ap, go)(x)
            assert s["seg"] == 64, (go, s)
            _same(ap.result(), want["y"], go + " behind a changed switch")
        fresh = mini_amd.AggregateProblem(g)
        assert fresh.run(x)["seg"] == 1024
        fresh.close()
        ap.close()
    g.close()


@pytest.mark.parametrize("feats", [8, 5])
def test_one_huge_row(gpu_ctx, feats):
    """a row of 100 000 entries at the default seg: 391 items and one fold"""
    ro, ci = cases.huge_row()
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", cases.weights(len(ci), 4), seed=4)
    assert want["bins"]["long"] == 1 and want["bins"]["segments"] == -(-100000 // model.SEG) and s["launches"] == 5
    _graph_check(gpu_ctx, ro, ci, feats, "mean", None, seed=5, operator=False)


@pytest.mark.parametrize("op", model.OPS)
@pytest.mark.parametrize("weighted", [False, True])
def test_ops(gpu_ctx, op, weighted):
    ro, ci = cases.graph_rows([0, 1, 2, 7, 70, 300, 5, 513, 64, 0, 33], seed=11, n=120)
    w = cases.weights(len(ci), 11) if weighted else None
    for feats in (8, 3):
        want, s = _graph_check(gpu_ctx, ro, ci, feats, op, w, seed=11, operator_first=feats == 3)
        assert want["bins"]["long"] == 2 and (s["launches"], s["host_waits"]) == (5, 1)      # operator first or not: the first fused run plans
    ro, ci, x = cases.zeros_case(4)                                             # +-0: the first of equal values, -0 + -0 = -0
    want, s = _graph_check(gpu_ctx, ro, ci, 4, op, np.ones(len(ci), np.float32) if weighted else None, x=x)
    if op in ("max", "min"):
        assert (_bits(want["y"][0]) == 0).all() and (_bits(want["y"][1]) == 0x80000000).all()
    # a graph uploaded without weights holds 1.0 for every entry: weighted is legal and gives the unweighted bits
    import mini_amd
    ro, ci = cases.graph_rows([3, 9, 0, 70], seed=12, n=80)
    x = cases.features(80, 8, 12)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    ap = mini_amd.AggregateProblem(g)
    ap.run(x, op, weighted=True)
    _same(ap.result(), model.aggregate(ro, ci, x, op)["y"], "weights of 1.0")
    ap.close()
    g.close()


@pytest.mark.parametrize("feats", [4, 1, 7])
def test_no_fused_multiply_add(gpu_ctx, feats):
    """w x rounds to 1 + 2^-11 and the sum is 0.0; a fused multiply-add keeps the product's 2^-24 (asserted in tests/agg_cases.py)"""
    ro, ci, w, x = cases.fma_case(feats)
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "sum", w, x=x)
    assert (_bits(want["y"][0]) == 0).all()
    want, s = _graph_check(gpu_ctx, ro, ci, feats, "mean", w, x=x, operator=False)


def test_sources(gpu_ctx):
    """out-rows; in-rows after build_csc() against the model on the transposed CSR with the CSC's own row values; without a CSC"""
    import mini_amd
    ro, ci = cases.random_digraph(500, 6000, 21)
    w = cases.weights(len(ci), 21)
    x = cases.features(500, 12, 21)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    ap = mini_amd.AggregateProblem(g)
    for go in (ap.run, ap.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go(x, rows="in")
        assert err.value.status == mini_amd.MGX_E_INVALID and "CSC" in str(err.value)
    _check(ap, model.aggregate(ro, ci, x, "sum", w), x, (True, False), op="sum", weighted=True, rows="out")
    g.build_csc()
    co, ri, rv = g.csc_arrays()
    assert not np.array_equal(co, ro)
    for op, weighted in (("sum", True), ("mean", False), ("max", True)):
        want = model.aggregate(co, ri, x, op, rv if weighted else None)
        _check(ap, want, x, (op == "sum", False), op=op, weighted=weighted, rows="in")       # the in-rows' own plan, built once
    _check(ap, model.aggregate(ro, ci, x, "min", w), x, (False, False), op="min", weighted=True, rows="out")   # the out-rows' is still there
    ap.close()
    g.close()


def _block_check(ctx, ro, ci, w, seeds, fanouts, feats, seed, sampler="run"):
    """sampler: which of the sampler's paths left the block (each keeps its own results and entry offsets)"""
    import mini_amd
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    ap = mini_amd.AggregateProblem(g)
    st = getattr(sp, sampler)(seeds, fanouts, seed=seed)
    off, rows, cols, pos = sp.hop_offsets(), sp.row_offsets(), sp.cols(), sp.entry_pos()
    x = cases.features(st["vertices"], feats, seed)
    whole = -1 in fanouts
    for k, hop in enumerate([None] + list(range(len(fanouts)))):
        part = rows if hop is None else rows[off[hop]:off[hop + 1] + 1]
        if st["vertices"] == 0:
            part = np.zeros(1, dtype=np.int32)
        for op, weighted in (("sum", True), ("mean", False)):
            want = model.aggregate(part, cols, x, op, w[pos] if weighted else None)
            assert whole or want["bins"]["long"] == 0
            s = _check(ap, want, x, (whole, whole), op=op, weighted=weighted, block=sp, hop=hop, operator=k < 2,
                       operator_first=k == 0 and op == "sum")             # (the handle's very first call is mgx_agg_enact)
            if not whole and want["stats"]["rows"]:
                assert (s["launches"], s["host_waits"]) == (1, 0)
    ap.close()
    sp.close()
    g.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_blocks(gpu_ctx, oracle, name):
    """a sampling run's rows read on the device: every hop and all rows, X by local id, the weights through entry_pos"""
    n, ro, ci, w, _ = oracle.load_mtx(os.path.join(GOLD, name), undir=True, random_w=True)
    for fanouts in ([3, 2], [-1, 1]):
        for sampler in ("run", "enact"):
            _block_check(gpu_ctx, ro, ci, np.asarray(w, dtype=np.float32), np.arange(0, n, 2), fanouts, 8, seed=5, sampler=sampler)


def test_blocks_rmat(gpu_ctx, oracle, monkeypatch):
    import mini_amd
    monkeypatch.setenv("MGX_AGG_SEG", "64")                                     # R-MAT-12's hubs are long rows then
    n, ro, ci, w = oracle.rmat_csr(12, 16, 512, undir=False)
    w = cases.weights(len(ci), 12)
    seeds = np.random.default_rng(12).integers(0, n, 200)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    ap = mini_amd.AggregateProblem(g)
    for fanouts, sample in (([3, 2], sp.run), ([-1, 1], sp.enact), ([-1, 1], sp.run)):
        st = sample(seeds, fanouts, seed=3)
        off, rows, cols, pos = sp.hop_offsets(), sp.row_offsets(), sp.cols(), sp.entry_pos()
        x = cases.features(st["vertices"], 16, 12)
        whole = -1 in fanouts
        for hop in (None, 0, 1):
            part = rows if hop is None else rows[off[hop]:off[hop + 1] + 1]
            want = model.aggregate(part, cols, x, "sum", w[pos], seg=64)
            assert want["bins"]["long"] > 0 if (whole and hop != 1) else want["bins"]["long"] == 0
            _check(ap, want, x, (whole, whole), op="sum", weighted=True, block=sp, hop=hop, operator=hop is None)
    # a block handle after a refused sampling run, of another graph, a hop the run does not have
    with pytest.raises(mini_amd.MgxError):
        sp.run([n], [2])
    x = cases.features(n, 4, 1)
    for go in (ap.run, ap.enact):
        with pytest.raises(mini_amd.MgxError) as err:
            go(x, block=sp)
        assert err.value.status == mini_amd.MGX_E_INVALID and "successful" in str(err.value)
    sp.run(seeds, [2, 2], seed=1)
    g2 = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    other = mini_amd.AggregateProblem(g2)
    for call, word in ((lambda: other.run(x, block=sp), "another graph"), (lambda: ap.run(x, block=sp, hop=2), "hop"), (lambda: ap.run(x, block=sp, hop=-2), "hop"),
                       (lambda: ap.run(x[:sp._last["vertices"] - 1], block=sp), "x_rows")):
        with pytest.raises(mini_amd.MgxError) as err:
            call()
        assert err.value.status == mini_amd.MGX_E_INVALID and word in str(err.value), str(err.value)
    for h in (other, ap, sp):
        h.close()
    g2.close()
    g.close()


def test_plan_is_kept(gpu_ctx):
    """the first run on the out-rows builds their plan (+2 launches, +1 wait); another F and op find it; the in-rows have their own"""
    import mini_amd
    ro, ci = cases.graph_rows([300, 0, 5, 1000, 256, 257], seed=31, n=300)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None).build_csc()
    co, ri, rv = g.csc_arrays()
    ap = mini_amd.AggregateProblem(g)
    x8, x5 = cases.features(300, 8, 31), cases.features(300, 5, 32)
    s = ap.run(x8)
    assert (s["launches"], s["host_waits"]) == (5, 1) == model.fused_counts(300, 3, True)
    s = ap.run(x5, "max")
    assert (s["launches"], s["host_waits"]) == (3, 0) == model.fused_counts(300, 3, False)
    _same(ap.result(), model.aggregate(ro, ci, x5, "max")["y"], "another F and op on the kept plan")
    s = ap.run(x8, rows="in")
    long_in = model.aggregate(co, ri, x8)["stats"]["long_rows"]
    assert (s["launches"], s["host_waits"]) == model.fused_counts(300, long_in, True)
    s = ap.run(x8, "mean", rows="in")
    assert (s["launches"], s["host_waits"]) == model.fused_counts(300, long_in, False)
    _same(ap.result(), model.aggregate(co, ri, x8, "mean")["y"], "the in-rows' plan")
    s = ap.run(x8)
    assert (s["launches"], s["host_waits"]) == (3, 0)
    _same(ap.result(), model.aggregate(ro, ci, x8)["y"], "back on the out-rows")
    ap.close()
    g.close()


def test_handle_reuse(gpu_ctx):
    """on ONE handle a large block, a small one and the large one again, each what a fresh handle gives; the partials only grow"""
    import mini_amd
    ro, ci = cases.random_digraph(3000, 40000, 41)
    w = cases.weights(len(ci), 41)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    one = mini_amd.AggregateProblem(g)
    large, small = np.arange(0, 2000, 2), np.arange(2001, 2100, 7)
    for seeds, fanouts, feats in ((large, [-1, 3], 32), (small, [2, 2], 5), (large, [-1, 3], 32), (small, [-1], 64)):
        st = sp.run(seeds, fanouts, seed=9)
        x = cases.features(st["vertices"], feats, 9)
        want = model.aggregate(sp.row_offsets(), sp.cols(), x, "sum", w[sp.entry_pos()])
        s = one.run(x, weighted=True, block=sp)
        _same(one.result(), want["y"], "one handle")
        fresh = mini_amd.AggregateProblem(g)
        assert fresh.run(x, weighted=True, block=sp) == s
        _same(fresh.result(), want["y"], "fresh handle")
        so = fresh.enact(x, weighted=True, block=sp)                           # operator behind fused on one handle
        _same(fresh.result(), want["y"], "operator behind fused")
        fresh.close()
    one.close()
    one.close()
    sp.close()
    g.close()


def test_edges_and_refusals(gpu_ctx, torch_mod):
    import mini_amd
    want, s = _graph_check(gpu_ctx, *cases.empty(0), 4)                          # n = 0
    assert (s["launches"], s["host_waits"], s["rows"]) == (0, 0, 0)
    want, s = _graph_check(gpu_ctx, *cases.empty(50), 4, "mean")                 # m = 0: zeros
    assert (want["y"] == 0).all() and s["launches"] == 3
    ro, ci = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)    # R = 1 with a self-loop
    want, s = _graph_check(gpu_ctx, ro, ci, 4, "sum", np.array([2.5], np.float32))
    ro, ci = np.array([0, 6, 6, 9], dtype=np.int32), np.array([1, 1, 1, 2, 1, 1, 0, 0, 0], dtype=np.int32)     # duplicate entries
    want, s = _graph_check(gpu_ctx, ro, ci, 5, "sum")
    # every refusal, before any device work; the getters after a refusal
    ro, ci = cases.random_digraph(100, 600, 51)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    ap = mini_amd.AggregateProblem(g)
    lib, h = mini_amd.lib, ap._h
    x = torch_mod.zeros(2 * 100 * 8 + 64, dtype=torch_mod.float32, device="cuda")
    y = torch_mod.zeros(100 * 8 + 64, dtype=torch_mod.float32, device="cuda")
    xp, yp = x.data_ptr(), y.data_ptr()
    ok = dict(source=0, block=None, hop=-1, x=xp, x_rows=100, ldx=8, feats=8, op=0, weighted=0, y=yp, ldy=8)
    bad = [(dict(feats=0), "feats"), (dict(feats=65537, ldx=65537, ldy=65537), "feats"), (dict(ldx=7), "ldx"), (dict(ldy=7), "ldy"), (dict(x=None), "NULL"),
           (dict(y=None), "NULL"), (dict(op=4), "op"), (dict(source=3), "source"), (dict(source=1), "CSC"), (dict(source=2), "block"),
           (dict(x_rows=99), "x_rows"), (dict(y=xp), "overlap"), (dict(y=xp + 4 * 8 * 99), "overlap"), (dict(x=yp + 4 * 7, x_rows=100), "overlap")]
    for go in (lib.mgx_agg_run, lib.mgx_agg_enact):
        assert go(h, 0, None, -1, xp, 100, 8, 8, 0, 0, yp, 8, None) == 0
        assert lib.mgx_agg_bins(h, (mini_amd._lib._i64 * 5)()) == (0 if go is lib.mgx_agg_run else mini_amd.MGX_E_INVALID)
        before = mini_amd.lib.mgx_device_allocations()
        for change, word in bad:
            a = dict(ok, **change)
            status = go(h, a["source"], a["block"], a["hop"], a["x"], a["x_rows"], a["ldx"], a["feats"], a["op"], a["weighted"], a["y"], a["ldy"], None)
            assert status == mini_amd.MGX_E_INVALID and word.encode() in lib.mgx_last_error(), (change, lib.mgx_last_error())
            for getter in (ap.result, ap.bins, ap.phase_ms):                    # a refused call leaves nothing to the getters
                with pytest.raises(mini_amd.MgxError) as err:
                    getter()
                assert err.value.status == mini_amd.MGX_E_INVALID and "no run yet" in str(err.value)
        assert mini_amd.lib.mgx_device_allocations() == before                 # refused before any device work
    # touching ranges are legal: Y starts where X ends (x holds both)
    assert lib.mgx_agg_run(h, 0, None, -1, xp, 100, 8, 8, 0, 0, xp + 4 * 800, 8, None) == 0
    ap.close()
    g.close()


def test_timing_changes_nothing(gpu_ctx):
    import mini_amd
    ro, ci = cases.graph_rows([300, 0, 5, 1000, 7, 257] * 20, seed=61, n=300)
    x = cases.features(300, 16, 61)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    ap = mini_amd.AggregateProblem(g)
    with pytest.raises(mini_amd.MgxError):
        ap.phase_ms()
    ap.run(x)
    plain, y = ap.run(x), ap.result()
    assert ap.phase_ms() == {"rows": 0.0, "items": 0.0, "fold": 0.0}
    ap.set_timing(True)
    timed = ap.run(x)
    assert timed == plain
    _same(ap.result(), y, "timed")
    ms = ap.phase_ms()
    assert set(ms) == {"rows", "items", "fold"} and min(ms.values()) > 0.0
    _same(y, model.aggregate(ro, ci, x)["y"], "model")
    ap.close()
    g.close()


def test_another_stream(gpu_ctx, torch_mod):
    import mini_amd
    ro, ci = cases.graph_rows([300, 0, 5, 70, 7, 257] * 10, seed=71, n=200)
    s = torch_mod.cuda.Stream()
    ctx = mini_amd.Context(0, s.cuda_stream)
    try:
        _graph_check(ctx, ro, ci, 12, "sum", cases.weights(len(ci), 71), seed=71)
    finally:
        ctx.close()
