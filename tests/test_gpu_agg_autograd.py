"""GPU suite (-m gpu): mini_amd.autograd.aggregate, the torch.autograd.Function on top of AggregateProblem / AggregateGradProblem
(DESIGN 3.24).  x.grad equals the numpy model's bits (tests/aggbwd_model.py) for each op on a graph and on a block, a two-hop chain
equals the composed model, on the default context and on a context whose stream is not torch's current one; a block sampled again
between forward and backward raises; without requires_grad no backward work runs."""
import numpy as np
import pytest

from tests import agg_model as fwd
from tests import aggbwd_cases as cases
from tests import aggbwd_model as model

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, who):
    assert got.shape == want.shape, (who, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d of %d elements differ in their bits" % (who, int((_bits(got) != _bits(want)).sum()), want.size)


@pytest.fixture(params=["default", "other_stream"])
def ctx(request, gpu_ctx, torch_mod):
    """the suite's context (on torch's current stream), and a context on a stream of its own while torch stays on its default"""
    import mini_amd
    if request.param == "default":
        yield gpu_ctx
        return
    s = torch_mod.cuda.Stream()
    c = mini_amd.Context(0, s.cuda_stream)
    assert c.stream == s.cuda_stream != torch_mod.cuda.current_stream().cuda_stream
    yield c
    torch_mod.cuda.synchronize()
    c.close()


@pytest.mark.parametrize("op", fwd.OPS)
def test_grad_on_a_graph(ctx, torch_mod, op):
    import mini_amd
    from mini_amd.autograd import aggregate
    ro, ci = cases.graph_rows([0, 1, 2, 7, 70, 300, 5, 33], seed=3, n=90)
    w = cases.weights(len(ci), 3)
    hx, hgy = cases.features(90, 8, 3), cases.features(90, 8, 4)
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    # (the inputs are made by torch kernels queued right before the call: on the other stream only the events order them)
    x = (torch_mod.from_numpy(hx).cuda() * 1.0).requires_grad_(True)
    gy = torch_mod.from_numpy(hgy).cuda() * 1.0
    y = aggregate(g, x, op=op, weighted=True)
    _same(y.detach().cpu().numpy(), fwd.aggregate(ro, ci, hx, op, w)["y"], "forward")
    y.backward(gy)
    _same(x.grad.cpu().numpy(), model.backward(ro, ci, hgy, op, w, x=hx, x_rows=90)["gx"], "x.grad")
    g.close()


@pytest.mark.parametrize("op", fwd.OPS)
def test_grad_on_a_block(ctx, torch_mod, op):
    import mini_amd
    from mini_amd.autograd import aggregate
    ro, ci = cases.fwd_cases.random_digraph(400, 4000, 5)
    w = cases.weights(len(ci), 5)
    g = mini_amd.Graph.from_host(ctx, ro, ci, w)
    sp = mini_amd.NeighborSampleProblem(g)
    st = sp.run(np.arange(0, 60, 2), [3, 2], seed=7)
    rows, cols, pos = sp.row_offsets(), sp.cols(), sp.entry_pos()
    hx, hgy = cases.features(st["vertices"], 12, 5), cases.features(st["rows"], 12, 6)
    x = (torch_mod.from_numpy(hx).cuda() * 1.0).requires_grad_(True)
    y = aggregate(g, x, op=op, weighted=True, block=sp)
    y.backward(torch_mod.from_numpy(hgy).cuda() * 1.0)
    _same(x.grad.cpu().numpy(), model.backward(rows, cols, hgy, op, w[pos], x=hx, x_rows=st["vertices"])["gx"], "x.grad")
    sp.close()
    g.close()


def test_two_hop_chain(ctx, torch_mod):
    """hop 1's aggregate feeds hop 0's through a slice (a block's vertices start with hop 0's rows, then hop 1's): x.grad is the
    composed model's"""
    import mini_amd
    from mini_amd.autograd import aggregate
    ro, ci = cases.fwd_cases.random_digraph(400, 4000, 8)
    g = mini_amd.Graph.from_host(ctx, ro, ci, None)
    sp = mini_amd.NeighborSampleProblem(g)
    st = sp.run(np.arange(0, 40), [3, 3], seed=2)
    off, rows, cols = sp.hop_offsets(), sp.row_offsets(), sp.cols()
    V, R0, R1 = st["vertices"], int(off[1] - off[0]), int(off[2] - off[1])
    hx, hgy = cases.features(V, 8, 8), cases.features(R0, 8, 9)
    x = (torch_mod.from_numpy(hx).cuda() * 1.0).requires_grad_(True)
    h1 = aggregate(g, x, op="mean", block=sp, hop=1)                              # the rows of hop 1: the vertices R0 .. R0 + R1 - 1
    mid = torch_mod.cat([x[:R0], h1, x[R0 + R1:]])                                # their new features beside everybody else's
    y = aggregate(g, mid, op="sum", block=sp, hop=0)
    y.backward(torch_mod.from_numpy(hgy).cuda() * 1.0)
    r0, r1 = rows[off[0]:off[1] + 1], rows[off[1]:off[2] + 1]
    gmid = model.backward(r0, cols, hgy, "sum", x_rows=V)["gx"]
    g1 = model.backward(r1, cols, gmid[R0:R0 + R1], "mean", x_rows=V)["gx"]
    want = g1.copy()
    want[:R0] = (want[:R0] + gmid[:R0]).astype(np.float32)                        # (torch accumulates the slices' gradients onto h1's)
    want[R0 + R1:] = (want[R0 + R1:] + gmid[R0 + R1:]).astype(np.float32)
    got = x.grad.cpu().numpy()
    # (an element gets at most two non-zero contributions, so torch's order of accumulation does not show; the zeros it adds for the
    #  other slices can turn a -0.0 into +0.0, which compares equal)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    sp.close()
    g.close()


def test_a_block_sampled_again_raises(gpu_ctx, torch_mod):
    import mini_amd
    from mini_amd.autograd import aggregate
    ro, ci = cases.fwd_cases.random_digraph(400, 4000, 5)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    sp = mini_amd.NeighborSampleProblem(g)
    st = sp.run(np.arange(0, 60, 2), [3, 2], seed=7)
    x = torch_mod.from_numpy(cases.features(st["vertices"], 4, 1)).cuda().requires_grad_(True)
    y = aggregate(g, x, block=sp)
    sp.run(np.arange(1, 80, 2), [2, 2], seed=8)
    with pytest.raises(RuntimeError, match="sampled again"):
        y.sum().backward()
    assert x.grad is None
    sp.close()
    g.close()


def test_without_requires_grad_no_backward_work_runs(gpu_ctx, torch_mod):
    import mini_amd
    from mini_amd import autograd
    ro, ci = cases.graph_rows([3, 9, 0, 70], seed=12, n=80)
    g = mini_amd.Graph.from_host(gpu_ctx, ro, ci, None)
    hx = cases.features(80, 8, 12)
    y = autograd.aggregate(g, torch_mod.from_numpy(hx).cuda())
    assert not y.requires_grad
    _same(y.cpu().numpy(), fwd.aggregate(ro, ci, hx)["y"], "forward")
    pair = autograd.handles(g)
    assert pair is autograd.handles(g) and pair[1]._last is None                 # one pair per graph; its backward handle never ran
    # a second input that does not ask for a gradient beside one that does: only the one that asks gets the work
    x = torch_mod.from_numpy(hx).cuda().requires_grad_(True)
    autograd.aggregate(g, x).sum().backward()
    assert pair[1]._last is not None and pair[1]._last["built"] == 1
    g.close()
