"""torch.autograd on top of the neighbour feature aggregation: aggregate(graph, x, ...) is AggregateProblem.run in
the forward and AggregateGradProblem.run in the backward, so that sample -> aggregate -> dense layers -> loss.backward() trains.
torch is imported here and nowhere else in the package.

  * the gradient is with respect to x alone; the gradient with respect to the edge weights is not built;
  * one pair of handles is kept per graph (weakly: it goes with the graph);
  * the library runs on its context's stream.  Where that is not torch's current stream the two are ordered with events, in both
    directions, around every call; the tensors the library touches are recorded on its stream;
  * a block must still hold the sampling run it held at forward time when backward runs: the run's sizes (seeds, vertices, rows,
    edges, draws, collisions, ...) are kept at forward time and compared, and a re-run sampler raises rather than computing on other rows."""
import weakref

import torch

from .api import AggregateGradProblem, AggregateProblem

_handles = weakref.WeakKeyDictionary()          # graph -> (AggregateProblem, AggregateGradProblem)
_BLOCK_KEYS = ("seeds", "unique_seeds", "hops", "vertices", "rows", "edges", "empty_rows", "whole_rows", "sampled_rows", "draws", "collisions", "revisits")


def handles(graph):
    """the graph's pair of handles, made at first use"""
    pair = _handles.get(graph)
    if pair is None:
        pair = (AggregateProblem(graph), AggregateGradProblem(graph))
        _handles[graph] = pair
    return pair


class _on_context_stream:
    """orders torch's current stream and the context's stream around the library's calls"""

    def __init__(self, ctx, tensors):
        self.cur = torch.cuda.current_stream()
        self.own = None
        if int(ctx.stream) != int(self.cur.cuda_stream):
            self.own = torch.cuda.ExternalStream(int(ctx.stream)) if ctx.stream else torch.cuda.default_stream()
        self.tensors = tensors

    def __enter__(self):
        if self.own is not None:
            self.own.wait_stream(self.cur)                 # what torch has queued for the inputs comes first
            for t in self.tensors:
                t.record_stream(self.own)
        return self

    def __exit__(self, *exc):
        if self.own is not None:
            self.cur.wait_stream(self.own)                 # and torch's next kernels wait for the library's
        return False


def _block_state(block):
    last = getattr(block, "_last", None)
    if not last:
        raise ValueError("the block has no successful sampling run")
    return tuple(int(last.get(k, -1)) for k in _BLOCK_KEYS)


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, op, weighted, rows, block, hop):
        fwd, _ = handles(graph)
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("x must be a two-dimensional float32 tensor on the device")
        x = x if x.stride(1) == 1 or x.shape[1] == 1 else x.contiguous()
        R = fwd._rows_of(block, hop)
        y = torch.empty((R, x.shape[1]), dtype=torch.float32, device=x.device)
        with _on_context_stream(graph.ctx, (x, y)):
            fwd.run(x, op=op, weighted=weighted, rows=rows, block=block, hop=hop, out=y, ldx=max(int(x.stride(0)), x.shape[1]), ldy=x.shape[1],
                    x_rows=x.shape[0], feats=x.shape[1])
        ctx.how = (graph, op, weighted, rows, block, hop, x.shape[0], None if block is None else _block_state(block))
        if op in ("max", "min"):
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        graph, op, weighted, rows, block, hop, x_rows, state = ctx.how
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        if block is not None and _block_state(block) != state:
            raise RuntimeError("the block was sampled again between forward and backward: its rows are no longer the forward's")
        _, bwd = handles(graph)
        gy = gy.contiguous()
        x = ctx.saved_tensors[0] if op in ("max", "min") else None
        gx = torch.empty((x_rows, gy.shape[1]), dtype=torch.float32, device=gy.device)
        with _on_context_stream(graph.ctx, (gy, gx) + (() if x is None else (x,))):
            bwd.run(gy, op=op, weighted=weighted, rows=rows, block=block, hop=hop, x=x, out=gx, ldgy=gy.shape[1],
                    ldx=None if x is None else max(int(x.stride(0)), x.shape[1]), ldgx=gy.shape[1], x_rows=x_rows, feats=gy.shape[1])
        return (gx,) + (None,) * 6


def aggregate(graph, x, op="sum", weighted=False, rows="out", block=None, hop=None):
    """Y = the aggregation of x over the graph's out-rows (rows="out"), its in-rows ("in") or a NeighborSampleProblem's last run
    (block=, hop=), as AggregateProblem.run computes it, differentiable with respect to x"""
    return _Aggregate.apply(x, graph, op, weighted, rows, block, hop)
