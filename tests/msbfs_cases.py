"""Graphs the multi-source BFS's suites share (tests/test_msbfs_cpu.py, tests/test_gpu_msbfs.py): the label propagation's builders
(tests/lpa_cases.py) and what is particular to a traversal -- rows of exact lengths on the out- and on the in-side."""
import numpy as np

from tests.lpa_cases import (directed, empty, grid, path, random_digraph, random_symmetric, star, sym, clique)  # noqa: F401


def complete(k):
    return sym(k, *clique(k))


def fans(lengths):
    """a directed graph with, for every length L, a hub whose out-row has exactly L entries (to leaves of its own) and a sink
    whose in-row has exactly L entries (from those same leaves); a root reaches every hub -> (ro, ci, root, hubs, sinks).
    Forced PUSH meets the hubs' out-rows in its lists, forced PULL the sinks' in-rows."""
    src, dst, hubs, sinks = [], [], [], []
    nxt = 1                                       # vertex 0 is the root
    for ln in lengths:
        hub, sink = nxt, nxt + 1
        leaves = nxt + 2 + np.arange(ln)
        nxt += 2 + ln
        hubs.append(hub)
        sinks.append(sink)
        src += [np.array([0]), np.full(ln, hub), leaves]
        dst += [np.array([hub]), leaves, np.full(ln, sink)]
    ro, ci = directed(nxt, np.concatenate(src), np.concatenate(dst))
    return ro, ci, 0, hubs, sinks


def cuts(short_max, wave_max, seg):
    """the row lengths one below, at and one above every cut: short_max, wave_max, one segment and two segments"""
    out = set()
    for c in (short_max, wave_max, seg, 2 * seg):
        out.update((c - 1, c, c + 1))
    return sorted(x for x in out if x >= 1)


def with_isolated(ro, ci, extra):
    """the same graph with `extra` vertices without entries behind it"""
    ro = np.asarray(ro)
    return np.concatenate([ro, np.full(extra, ro[-1], dtype=ro.dtype)]), ci
