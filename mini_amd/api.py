"""Host-side mirror of the reference's data model and operator interface over the C-ABI.

Names follow the reference (gunrock/src/*.hxx): Graph ~ graph_device_t, Frontier ~ frontier_t<int>,
BfsProblem ~ bfs_problem_t + bfs_enactor_t, SsspProblem ~ sssp_problem_t + sssp_enactor_t,
PrProblem ~ pr_problem_t + pr_enactor_t, KcoreProblem ~ kcore_problem_t + kcore_enactor_t,
ColorProblem ~ coloring_problem_t + coloring_enactor_t, LsparProblem ~ lspar_problem_t + lspar_enactor_t,
CcProblem ~ cc_problem_t + cc_enactor_t, TcProblem ~ tc_problem_t + tc_enactor_t, BcProblem ~ bc_problem_t + bc_enactor_t, MstProblem ~ mst_problem_t + mst_enactor_t, KtrussProblem ~ ktruss_problem_t + ktruss_enactor_t, PageRankProblem ~ pagerank_problem_t + pagerank_enactor_t.  Every method is one C-ABI call; nothing is computed here but TcProblem.clustering() / transitivity(), one numpy division on the counts, BcProblem.centrality()'s two scalings, and KtrussProblem's canonical edge order (u < v, sorted by (u, v): one lexsort of what the library returns in its own edge order).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev_ptr(x):
    """int device address, or an object with data_ptr() (torch tensor), or None"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


CHAIN_LOG_CAP = 1 << 16     # include/mgx/launch_chain.hpp: the launches (MsBfsProblem: levels) of a run whose kind is kept


class _StepKinds:
    """A fused path that is a chain of launches (include/mgx/launch_chain.hpp).  `_C` is the handle's C prefix; the class says what
    its STEP_KINDS are."""

    def step_kinds(self):
        """what every launch of the last run() was, in order (the first CHAIN_LOG_CAP): codes of STEP_KINDS"""
        n = C.c_int64()
        out = np.empty(CHAIN_LOG_CAP, dtype=np.int32)
        check(getattr(lib, self._C + "_step_kinds")(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:min(n.value, len(out))].copy()


class _Timed:
    """A fused path that times its phases on the device when asked.  `_C` is the handle's C prefix; the class says what its PHASES
    are."""

    def set_timing(self, on):
        """measurement tools: every run() keeps the time of each of PHASES"""
        check(getattr(lib, self._C + "_set_timing")(self._h, int(bool(on))))

    def phase_ms(self):
        """ms per entry of PHASES of the last timed run()"""
        out = (C.c_double * len(self.PHASES))()
        check(getattr(lib, self._C + "_phase_ms")(self._h, out))
        return dict(zip(self.PHASES, (float(x) for x in out)))


class Context:
    """standard_context_t: one device, one stream, scratch arena (tests/bfs/test_bfs.cu:22)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib.mgx_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(h)))
        self._h = h
        self.device = device
        self.stream = int(stream or 0)         # the stream's address as given (0: the default stream), for callers that order work against it

    def set_stream(self, stream):
        check(lib.mgx_ctx_set_stream(self._h, C.c_void_p(stream or 0)))
        self.stream = int(stream or 0)

    def synchronize(self):
        check(lib.mgx_ctx_synchronize(self._h))

    @property
    def num_cus(self):
        v = C.c_int()
        check(lib.mgx_ctx_num_cus(self._h, C.byref(v)))
        return v.value

    def close(self):
        if self._h:
            lib.mgx_ctx_destroy(self._h)
            self._h = None


class Graph:
    """graph_device_t (graph.hxx:37-83).  CSC slots mirror the CSR unless a CSC is given."""

    def __init__(self, ctx, handle, keepalive=None):
        self.ctx, self._h, self._keep = ctx, handle, keepalive
        n, m = C.c_int(), C.c_int64()
        check(lib.mgx_graph_dims(self._h, C.byref(n), C.byref(m)))
        self.num_nodes, self.num_edges = n.value, m.value

    @classmethod
    def from_host(cls, ctx, row_offsets, col_indices, weights=None, col_offsets=None, row_indices=None,
                  row_weights=None):
        ro, ci = _np_i32(row_offsets), _np_i32(col_indices)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        co = None if col_offsets is None else _np_i32(col_offsets)
        ri = None if row_indices is None else _np_i32(row_indices)
        rw = None if row_weights is None else np.ascontiguousarray(row_weights, dtype=np.float32)
        h = C.c_void_p()
        check(lib.mgx_graph_upload(ctx._h, len(ro) - 1, len(ci), _ptr(ro), _ptr(ci), _ptr(w), _ptr(co), _ptr(ri),
                                   _ptr(rw), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_device(cls, ctx, num_nodes, num_edges, row_offsets, col_indices, weights=None, col_offsets=None,
                    row_indices=None, row_weights=None):
        """Borrow device arrays (torch tensors or raw addresses); they are kept alive by the Graph."""
        h = C.c_void_p()
        check(lib.mgx_graph_wrap_device(ctx._h, int(num_nodes), int(num_edges), _dev_ptr(row_offsets),
                                        _dev_ptr(col_indices), _dev_ptr(weights), _dev_ptr(col_offsets),
                                        _dev_ptr(row_indices), _dev_ptr(row_weights), C.byref(h)))
        return cls(ctx, h, keepalive=(row_offsets, col_indices, weights, col_offsets, row_indices, row_weights))

    def attach_layout(self, layout_row_offsets, layout_col_indices, new_of_old, old_of_new, layout_weights=None):
        """Hub-first (degree-descending) relabelled CSR + id maps for the fused traversals (device tensors);
        layout_weights (optional, the layout's edge order) lets the fused SSSP loop run in layout space too."""
        check(lib.mgx_graph_attach_layout(self._h, _dev_ptr(layout_row_offsets), _dev_ptr(layout_col_indices),
                                          _dev_ptr(new_of_old), _dev_ptr(old_of_new)))
        if layout_weights is not None:
            check(lib.mgx_graph_attach_layout_weights(self._h, _dev_ptr(layout_weights)))
        self._layout = (layout_row_offsets, layout_col_indices, new_of_old, old_of_new, layout_weights)
        return self

    def build_layout(self, weights=False):
        """The same layout, built by the library from the graph's own CSR (mgx_graph_build_layout) and owned by it."""
        check(lib.mgx_graph_build_layout(self._h, int(bool(weights))))
        return self

    def layout_info(self):
        """what the layout holds (mgx_graph_layout_info): unit blocks, cold-edge lists, device bytes"""
        out = (C.c_int64 * 8)()
        check(lib.mgx_graph_layout_info(self._h, out))
        keys = ("has_layout", "units", "units_24bit", "cold_pairs", "cold_slices", "hot_units", "cold_majority", "device_bytes")
        return dict(zip(keys, (int(x) for x in out)))

    def nr_slices_info(self):
        """the long rows by slice of their destinations (mgx_graph_nr_slices_info; built at the first full-frontier reduce)"""
        out = (C.c_int64 * 5)()
        check(lib.mgx_graph_nr_slices_info(self._h, out))
        keys = ("mini_units", "hot_slices", "long_rows", "multi_lane_fold_rows", "tail_mini_units")
        return dict(zip(keys, (int(x) for x in out)))

    def nr_last_call(self):
        """what the last neighbourhood reduce on this graph's context did (mgx_graph_nr_last_call; MgxError before any): body 0 the
        general kernel / 1 the layout's unit blocks / 2 the layout's sliced long rows, frontier 0 other / 1 full / 2 subset, rejected
        1 if the device's verdict on the frontier sent a layout call to the general kernel, and the edges the call returned"""
        out = (C.c_int64 * 4)()
        check(lib.mgx_graph_nr_last_call(self._h, out))
        return dict(zip(("body", "frontier", "rejected", "edges"), (int(x) for x in out)))

    def build_csc(self):
        """Genuine CSC (transpose) built by the library on the device (mgx_graph_build_csc): in-edges for the bottom-up
        levels on directed graphs."""
        check(lib.mgx_graph_build_csc(self._h))
        return self

    def csc_arrays(self):
        """(col_offsets, row_indices, row_values) of the CSC slots as host numpy arrays"""
        n, m = self.num_nodes, self.num_edges
        co, ri = np.empty(n + 1, dtype=np.int32), np.empty(max(m, 1), dtype=np.int32)
        rv = np.empty(max(m, 1), dtype=np.float32)
        check(lib.mgx_graph_csc_read(self._h, co.ctypes.data_as(C.c_void_p), ri.ctypes.data_as(C.c_void_p),
                                     rv.ctypes.data_as(C.c_void_p)))
        return co, ri[:m], rv[:m]

    def layout_arrays(self, weights=False):
        """(layout_row_offsets, layout_col_indices, new_of_old, old_of_new[, layout_weights]) as host numpy arrays"""
        n, m = self.num_nodes, self.num_edges
        lro, lci = np.empty(n + 1, dtype=np.int32), np.empty(max(m, 1), dtype=np.int32)
        n2o, o2n = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        lw = np.empty(max(m, 1), dtype=np.float32) if weights else None
        check(lib.mgx_graph_layout_read(self._h, lro.ctypes.data_as(C.c_void_p), lci.ctypes.data_as(C.c_void_p),
                                        n2o.ctypes.data_as(C.c_void_p), o2n.ctypes.data_as(C.c_void_p),
                                        lw.ctypes.data_as(C.c_void_p) if weights else None))
        out = (lro, lci[:m], n2o, o2n)
        return out + (lw[:m],) if weights else out

    def close(self):
        if self._h:
            lib.mgx_graph_free(self._h)
            self._h = None


def load_mtx(path, undir=False, random_edge_value=False, genuine_csc=None):
    """load_graph (graph.hxx:96-223) -> (n, row_offsets, col_indices, weights) on the host; with genuine_csc given
    (True / False) also the loader's CSC slots: (..., col_offsets, row_indices, row_weights)."""
    n, m = C.c_int(), C.c_int64()
    ptrs = [C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()]
    if genuine_csc is None:
        check(lib.mgx_load_mtx(str(path).encode(), int(undir), int(random_edge_value), C.byref(n), C.byref(m),
                               *[C.byref(p) for p in ptrs]))
    else:
        ptrs += [C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()]
        check(lib.mgx_load_mtx_csc(str(path).encode(), int(undir), int(random_edge_value), int(bool(genuine_csc)),
                                   C.byref(n), C.byref(m), *[C.byref(p) for p in ptrs]))
    N, M = n.value, m.value
    try:
        out = []
        for i, p in enumerate(ptrs):
            cnt = N + 1 if i % 3 == 0 else M
            out.append(np.ctypeslib.as_array(p, (max(cnt, 1),))[:cnt].copy())
    finally:
        for p in ptrs:
            lib.mgx_host_free(p)
    return (N,) + tuple(out)


def save_csr_cache(path, row_offsets, col_indices, weights=None, csc=None, undirected=False):
    """binary CSR cache (mgx_graph_save_csr); csc = (col_offsets, row_indices, row_weights) to store a genuine CSC too"""
    ro, ci = _np_i32(row_offsets), _np_i32(col_indices)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    co = ri = rw = None
    if csc is not None:
        co, ri = _np_i32(csc[0]), _np_i32(csc[1])
        rw = None if csc[2] is None else np.ascontiguousarray(csc[2], dtype=np.float32)
    check(lib.mgx_graph_save_csr(str(path).encode(), len(ro) - 1, len(ci), int(bool(undirected)), _ptr(ro), _ptr(ci), _ptr(w),
                                 _ptr(co), _ptr(ri), _ptr(rw)))


def load_csr_cache(path):
    """-> dict(n, undirected, row_offsets, col_indices, weights, csc = (col_offsets, row_indices, row_weights) | None)"""
    n, m, u = C.c_int(), C.c_int64(), C.c_int()
    ptrs = [C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)(), C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()]
    check(lib.mgx_graph_load_csr(str(path).encode(), C.byref(n), C.byref(m), C.byref(u), *[C.byref(p) for p in ptrs]))
    N, M = n.value, m.value
    try:
        arrs = []
        for i, p in enumerate(ptrs):
            cnt = N + 1 if i % 3 == 0 else M
            arrs.append(np.ctypeslib.as_array(p, (max(cnt, 1),))[:cnt].copy() if p else None)
    finally:
        for p in ptrs:
            if p:
                lib.mgx_host_free(p)
    return {"n": N, "undirected": bool(u.value), "row_offsets": arrs[0], "col_indices": arrs[1], "weights": arrs[2],
            "csc": None if arrs[3] is None else (arrs[3], arrs[4], arrs[5])}


class Frontier:
    """frontier_t<int> (frontier.hxx:12-99)."""

    def __init__(self, ctx, capacity):
        h = C.c_void_p()
        check(lib.mgx_frontier_create(ctx._h, int(capacity), C.byref(h)))
        self.ctx, self._h = ctx, h

    def load(self, ids):
        a = _np_i32(ids)
        check(lib.mgx_frontier_load(self._h, _ptr(a), len(a)))
        return self

    def fill_iota(self, n):
        check(lib.mgx_frontier_fill_iota(self._h, int(n)))
        return self

    def fill(self, value, n):
        check(lib.mgx_frontier_fill(self._h, int(value), int(n)))
        return self

    def resize(self, n):
        check(lib.mgx_frontier_resize(self._h, int(n)))

    @property
    def size(self):
        v = C.c_int64()
        check(lib.mgx_frontier_size(self._h, C.byref(v)))
        return v.value

    @property
    def capacity(self):
        v = C.c_int64()
        check(lib.mgx_frontier_capacity(self._h, C.byref(v)))
        return v.value

    @property
    def device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_frontier_device_ptr(self._h, C.byref(p)))
        return p.value

    def read(self):
        n = self.size
        out = np.empty(max(n, 1), dtype=np.int32)
        got = C.c_int64()
        check(lib.mgx_frontier_read(self._h, _ptr(out), len(out), C.byref(got)))
        return out[:got.value]

    def close(self):
        if self._h:
            lib.mgx_frontier_free(self._h)
            self._h = None


def _i64():
    return C.c_int64()


class BfsProblem:
    """bfs_problem_t + bfs_enactor_t (gunrock/src/bfs/)."""

    def __init__(self, graph, src=0):
        h = C.c_void_p()
        check(lib.mgx_bfs_create(graph._h, int(src), C.byref(h)))
        self.graph, self._h = graph, h

    def reset(self, src):
        check(lib.mgx_bfs_reset(self._h, int(src)))

    def labels(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_bfs_labels(self._h, _ptr(out)))
        return out

    def preds(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_bfs_preds(self._h, _ptr(out)))
        return out

    @property
    def labels_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_bfs_labels_device(self._h, C.byref(p)))
        return p.value

    # operators ------------------------------------------------------------------------------
    def advance(self, fin, fout, iteration):
        v = _i64()
        check(lib.mgx_bfs_advance(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def filter(self, fin, fout, iteration):
        v = _i64()
        check(lib.mgx_bfs_filter(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def advance_filter_fused(self, fin, fout, iteration):
        v = _i64()
        check(lib.mgx_bfs_advance_filter_fused(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def gen_unvisited(self, indices, unvisited, iteration=0):
        v = _i64()
        check(lib.mgx_bfs_gen_unvisited(self._h, indices._h, unvisited._h, int(iteration), C.byref(v)))
        return v.value

    def sparse_to_dense(self, sparse, dense, iteration):
        check(lib.mgx_bfs_sparse_to_dense(self._h, sparse._h, dense._h, int(iteration)))

    def advance_backward(self, unvisited, bitmap, bitmap_out, iteration):
        v = _i64()
        check(lib.mgx_bfs_advance_backward(self._h, unvisited._h, bitmap._h, bitmap_out._h, int(iteration),
                                           C.byref(v)))
        return v.value

    # enactors -------------------------------------------------------------------------------
    def enact_pushpull(self, threshold=None):
        """bfs_enactor_t::enact_pushpull; default threshold 1/n like test_bfs.cu:30."""
        if threshold is None:
            threshold = 1.0 / max(self.graph.num_nodes, 1)
        st = (C.c_int64 * 4)()
        check(lib.mgx_bfs_enact_pushpull(self._h, C.c_float(threshold), st))
        return {"pushed_iterations": st[0], "total_iterations": st[1], "pushed_edges": st[2], "pulled_edges": st[3]}

    def enact_idempotent(self):
        """the reference's idempotent mode as a loop: advance<idempotence> (every neighbour, no atomics) + uniquify"""
        st = (C.c_int64 * 2)()
        check(lib.mgx_bfs_enact_idempotent(self._h, st))
        return {"iterations": st[0], "edges": st[1]}

    def advance_idempotent(self, fin, fout, iteration):
        v = C.c_int64()
        check(lib.mgx_bfs_advance_idempotent(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def uniquify(self, fin, fout, iteration):
        v = C.c_int64()
        check(lib.mgx_bfs_uniquify(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    STATS_LEN = 24

    @staticmethod
    def new_stats():
        """a buffer for run_into()"""
        return (C.c_int64 * BfsProblem.STATS_LEN)()

    def run_into(self, src, mode, alpha, st):
        """Fused device-resident traversal, counters into a caller-made buffer (new_stats()): the call a timing loop
        makes -- nothing is allocated or converted between two traversals; stats_dict(st) reads the buffer afterwards."""
        rc = lib.mgx_bfs_run_stats(self._h, src, mode, alpha, st, BfsProblem.STATS_LEN)
        if rc:
            check(rc)

    def run_many(self, sources, mode=_lib.MGX_BFS_PUSH, alpha=0.0, prepared=None):
        """A batch of sources enqueued back to back, one host wait (mgx_bfs_run_many).  Returns (list of stats dicts,
        reruns); labels() are the last source's.  prepared = prepare_many(sources): buffers made beforehand, for timing loops
        (then only the ctypes call happens here and the raw buffer is returned instead of dicts)."""
        if prepared is None:
            srcs, st, rr, count = self.prepare_many(sources)
        else:
            srcs, st, rr, count = prepared
        rc = lib.mgx_bfs_run_many(self._h, srcs, count, int(mode), float(alpha), st, BfsProblem.STATS_LEN, C.byref(rr))
        if rc:
            check(rc)
        if prepared is not None:
            return st, rr.value
        L = BfsProblem.STATS_LEN
        return [self.stats_dict(st[i * L:(i + 1) * L]) for i in range(count)], rr.value

    @staticmethod
    def prepare_many(sources):
        n = len(sources)
        return (C.c_int * max(n, 1))(*[int(s) for s in sources]), (C.c_int64 * (max(n, 1) * BfsProblem.STATS_LEN))(), C.c_int(0), n

    @staticmethod
    def stats_dict(st):
        return {"levels": st[0], "reached": st[1], "m_t": st[2], "push_edges": st[3], "pull_edges": st[4],
                "push_levels": st[5], "kernel_launches": st[6], "kernel_ns": st[7], "frontier_vertices": st[8],
                "claims": st[9], "dom_launches": st[10], "dom_ns": st[11], "dom_edges": st[12],
                "dom_vertices": st[13],
                "dom_kernel": "k_bfs_push (long rows / merged launch)" if st[14] else "k_bfs_push (short rows)",
                "small_levels": st[15], "slots": st[16], "dense_slots": st[17], "vshort_slots": st[18], "lazy_slots": st[19],
                "cold_slots": st[20], "mini_slots": st[21], "level_byte_slot": st[22]}

    def run(self, src, mode=_lib.MGX_BFS_PUSH, alpha=0.0):
        """Fused device-resident traversal."""
        st = self.new_stats()
        self.run_into(int(src), int(mode), float(alpha), st)
        return self.stats_dict(st)

    def level_trace(self, cap=4096):
        nf, ne, lv = (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int()
        check(lib.mgx_bfs_level_trace(self._h, cap, nf, ne, C.byref(lv)))
        L = min(lv.value, cap)
        return [(nf[i], ne[i]) for i in range(L)]

    def set_kernel_timing(self, on=True):
        """events around every push-kernel launch (costs ~6 us of stream gap per event: profiling runs only).
        True / 1: the parts of a slot's push as separate launches; 2: the one merged launch a traversal really runs"""
        check(lib.mgx_bfs_set_kernel_timing(self._h, int(on)))

    def kernel_times(self):
        """per-launch timing of the two push kernels of the last run()"""
        c = (C.c_int64 * 8)()
        check(lib.mgx_bfs_kernel_times(self._h, c))
        keys = ("launches", "ns", "edges", "vertices")
        return {"stream": dict(zip(keys, c[0:4])), "wave": dict(zip(keys, c[4:8]))}

    def level_times_ms(self, cap=63):
        """per-level duration from device-side timestamps (no host synchronisation per level)"""
        ms, lv = (C.c_float * cap)(), C.c_int()
        check(lib.mgx_bfs_level_times(self._h, cap, ms, C.byref(lv)))
        return [ms[i] for i in range(min(lv.value, cap))]

    def level_kernel_times_ms(self, cap=64):
        a, b = (C.c_float * cap)(), (C.c_float * cap)()
        check(lib.mgx_bfs_level_kernel_times(self._h, cap, a, b))
        return [(a[i], b[i]) for i in range(cap)]

    def level_claims(self, cap=64):
        c = (C.c_int64 * cap)()
        check(lib.mgx_bfs_level_claims(self._h, cap, c))
        return [c[i] for i in range(cap)]

    def batch_times_ms(self, cap=256):
        ms, nb = (C.c_float * cap)(), C.c_int()
        check(lib.mgx_bfs_batch_times(self._h, cap, ms, C.byref(nb)))
        return [ms[i] for i in range(min(nb.value, cap))]

    def close(self):
        if self._h:
            lib.mgx_bfs_free(self._h)
            self._h = None


class SsspProblem:
    """sssp_problem_t + sssp_enactor_t (gunrock/src/sssp/)."""

    def __init__(self, graph, src=0):
        h = C.c_void_p()
        check(lib.mgx_sssp_create(graph._h, int(src), C.byref(h)))
        self.graph, self._h = graph, h

    def reset(self, src):
        check(lib.mgx_sssp_reset(self._h, int(src)))

    def distances(self):
        out = np.empty(self.graph.num_nodes, dtype=np.float32)
        check(lib.mgx_sssp_distances(self._h, _ptr(out)))
        return out

    def preds(self):
        """after enact(): the functor's preds; after run(): a shortest-path tree built from the distances (mgx/sssp_preds.hpp)"""
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_sssp_preds(self._h, _ptr(out)))
        return out

    def build_preds(self):
        """builds the predecessors of the last run()'s distances on the device (no copy) -> {ties, rounds}"""
        st = (C.c_int64 * 2)()
        check(lib.mgx_sssp_build_preds(self._h, st))
        return {"ties": st[0], "rounds": st[1]}

    @property
    def distances_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_sssp_distances_device(self._h, C.byref(p)))
        return p.value

    def advance(self, fin, fout, iteration):
        v = _i64()
        check(lib.mgx_sssp_advance(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def filter(self, fin, fout, iteration):
        v = _i64()
        check(lib.mgx_sssp_filter(self._h, fin._h, fout._h, int(iteration), C.byref(v)))
        return v.value

    def enact(self, queue_sizing=1.0):
        st = (C.c_int64 * 3)()
        check(lib.mgx_sssp_enact(self._h, C.c_float(queue_sizing), st))
        return {"iterations": st[0], "relaxations": st[1], "frontier_total": st[2]}

    def set_kernel_timing(self, on=True):
        check(lib.mgx_sssp_set_kernel_timing(self._h, int(bool(on))))

    def iteration_trace(self, cap=63):
        """[(frontier vertices, edges relaxed, ms)] of the last run()'s iterations (device-side timestamps)"""
        nf, ne, ms, it = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_float * cap)(), C.c_int()
        check(lib.mgx_sssp_iteration_trace(self._h, cap, nf, ne, ms, C.byref(it)))
        return [(nf[i], ne[i], ms[i]) for i in range(min(it.value, cap))]

    def kernel_times(self):
        """{launches, ns} of k_sssp_relax in the last run() (after set_kernel_timing)"""
        c = (C.c_int64 * 2)()
        check(lib.mgx_sssp_kernel_times(self._h, c))
        return {"launches": c[0], "ns": c[1]}

    SWEEP_VARIANTS = {0: "none", 1: "ids32+f32", 2: "ids24+f32", 3: "ids24+f16"}

    def path_info(self):
        """which paths the last run() took (mgx_sssp_path_info; MgxError before the first run): swept + walked_with_bounds +
        walked_without_bounds + threshold_moves == iterations"""
        o = (C.c_int64 * 8)()
        check(lib.mgx_sssp_path_info(self._h, o))
        return {"sweep_available": bool(o[0]), "sweep_variant": int(o[1]), "swept": int(o[2]), "walked_with_bounds": int(o[3]),
                "walked_without_bounds": int(o[4]), "queue_build": "list" if o[5] else "direct", "threshold_moves": int(o[6]),
                "layout_space": bool(o[7])}

    def run(self, src, delta=None):
        """fused device-resident loop; delta: near / far bucket width (None / 0: plain frontier Bellman-Ford)"""
        st = (C.c_int64 * 3)()
        if delta is None:
            check(lib.mgx_sssp_run(self._h, int(src), st))
        else:
            check(lib.mgx_sssp_run_delta(self._h, int(src), C.c_float(delta), st))
        return {"iterations": st[0], "relaxations": st[1], "frontier_total": st[2]}

    def close(self):
        if self._h:
            lib.mgx_sssp_free(self._h)
            self._h = None


class PrProblem:
    """pr_problem_t + pr_enactor_t (gunrock/src/pr/)."""

    def __init__(self, graph, max_iter=10):
        h = C.c_void_p()
        check(lib.mgx_pr_create(graph._h, int(max_iter), C.byref(h)))
        self.graph, self._h, self.max_iter = graph, h, max_iter

    def enact(self):
        lens = (C.c_int64 * max(self.max_iter, 1))()
        it = C.c_int()
        check(lib.mgx_pr_enact(self._h, lens, C.byref(it)))
        return [lens[i] for i in range(it.value)]

    def ranks(self):
        out = np.empty(self.graph.num_nodes, dtype=np.float32)
        check(lib.mgx_pr_ranks(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h:
            lib.mgx_pr_free(self._h)
            self._h = None


class KcoreProblem(_StepKinds):
    """kcore_problem_t + kcore_enactor_t (gunrock/src/kcore/)."""

    _C = "mgx_kcore"

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_kcore_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    def reset(self):
        check(lib.mgx_kcore_reset(self._h))

    def enact(self):
        """-> (largest_k_core, {"rounds", "passes", "expanded", "removed"})"""
        largest = C.c_int()
        st = (C.c_int64 * 4)()
        check(lib.mgx_kcore_enact(self._h, C.byref(largest), st))
        return largest.value, {"rounds": st[0], "passes": st[1], "expanded": st[2], "removed": st[3]}

    def run(self):
        """The fused path (worklist peeling): the same core numbers, degrees and largest k-core as enact(), from a fresh start
        of its own (no reset() needed).  -> (largest_k_core, {"levels", "passes", "expanded", "removed", "stranded", "host_waits"})"""
        largest = C.c_int()
        st = (C.c_int64 * 6)()
        check(lib.mgx_kcore_run(self._h, C.byref(largest), st))
        return largest.value, {"levels": st[0], "passes": st[1], "expanded": st[2], "removed": st[3], "stranded": st[4],
                               "host_waits": st[5]}

    STEP_KINDS = {1: "min", 2: "list", 3: "expand", 4: "filter", 5: "idle", 6: "mini"}

    def num_cores(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_kcore_num_cores(self._h, _ptr(out)))
        return out

    def degrees(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_kcore_degrees(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h:
            lib.mgx_kcore_free(self._h)
            self._h = None


class ColorProblem:
    """coloring_problem_t + coloring_enactor_t (gunrock/src/coloring/), and the fused path beside them.  Every run starts
    from all-uncoloured; colors() / round_trace() describe the last run of either path."""

    SEED = 15485863        # the reference driver's defaults (tests/coloring/test_coloring.cu)
    MAX_ITER = 10

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_color_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    @staticmethod
    def _stats(st):
        return {"rounds": st[0], "uncolored": st[1], "max_color": st[2], "host_waits": st[3]}

    def run(self, seed=SEED, max_iter=MAX_ITER):
        """fused path -> {"rounds", "uncolored", "max_color", "host_waits"}; max_iter <= 0: until none is left"""
        st = (C.c_int64 * 4)()
        check(lib.mgx_color_run(self._h, C.c_uint(seed & 0xFFFFFFFF), int(max_iter), st))
        return self._stats(st)

    def enact(self, seed=SEED, max_iter=MAX_ITER):
        """operator path (neighbourhood reduce + filter); the same stats"""
        st = (C.c_int64 * 4)()
        check(lib.mgx_color_enact(self._h, C.c_uint(seed & 0xFFFFFFFF), int(max_iter), st))
        return self._stats(st)

    def colors(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_color_colors(self._h, _ptr(out)))
        return out

    @property
    def colors_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_color_colors_device(self._h, C.byref(p)))
        return p.value

    def round_trace(self):
        """active vertices at the start of every round of the last run (int64 array)"""
        rounds = C.c_int()
        check(lib.mgx_color_round_trace(self._h, None, 0, C.byref(rounds)))
        out = np.zeros(max(rounds.value, 1), dtype=np.int64)
        check(lib.mgx_color_round_trace(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), rounds.value, C.byref(rounds)))
        return out[:rounds.value]

    def info(self):
        """the fused path's row classes and the last fused run: {"long_min", "seg", "stage", "batch_max", "rounds": int64 (rounds, 3):
        short rows, long items, long rows at the start of every round run}"""
        consts, rounds = (C.c_int64 * 4)(), C.c_int()
        check(lib.mgx_color_info(self._h, consts, None, 0, C.byref(rounds)))
        out = np.zeros((max(rounds.value, 1), 3), dtype=np.int64)
        check(lib.mgx_color_info(self._h, consts, out.ctypes.data_as(C.POINTER(C.c_int64)), rounds.value, C.byref(rounds)))
        d = dict(zip(("long_min", "seg", "stage", "batch_max"), (int(x) for x in consts)))
        d["rounds"] = out[:rounds.value]
        return d

    def close(self):
        if self._h:
            lib.mgx_color_free(self._h)
            self._h = None


class LsparProblem:
    """lspar_problem_t + lspar_enactor_t (gunrock/src/lspar/), and the fused path beside them.  result() / minhashes() /
    graph() describe the last run of either path; `source` is the input graph."""

    SEED = 15485863        # the reference driver's defaults
    K = 1
    E = 0.5

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_lspar_create(graph._h, C.byref(h)))
        self.source, self._h = graph, h
        self._kept, self._k = None, None

    def _go(self, fn, seed, k, e):
        st = (C.c_int64 * 3)()
        self._kept = None
        check(fn(self._h, C.c_uint(seed & 0xFFFFFFFF), int(k), float(e), st))
        self._kept, self._k = st[0], int(k)
        return {"kept": st[0], "rows_cut": st[1], "host_waits": st[2]}

    def run(self, seed=SEED, k=K, e=E):
        """fused path -> {"kept", "rows_cut", "host_waits"}"""
        return self._go(lib.mgx_lspar_run, seed, k, e)

    def enact(self, seed=SEED, k=K, e=E):
        """operator path (neighbourhood reduce, advance, segmented sort, advance, compaction, segmented sort); the same stats"""
        return self._go(lib.mgx_lspar_enact, seed, k, e)

    def result(self):
        """(out_ro int32[n + 1], out_ci, out_eid, out_sim int32[kept])"""
        if self._kept is None:
            check(lib.mgx_lspar_result(self._h, None, None, None, None))       # raises: no run yet
        n, m = self.source.num_nodes, self._kept
        ro = np.empty(n + 1, dtype=np.int32)
        ci, eid, sim = (np.empty(max(m, 1), dtype=np.int32) for _ in range(3))
        check(lib.mgx_lspar_result(self._h, _ptr(ro), _ptr(ci), _ptr(eid), _ptr(sim)))
        return ro, ci[:m], eid[:m], sim[:m]

    def result_device_ptrs(self):
        p = [C.c_void_p() for _ in range(4)]
        check(lib.mgx_lspar_result_device(self._h, *(C.byref(x) for x in p)))
        return tuple(x.value for x in p)

    def minhashes(self):
        """(n, k) uint32, vertex-major"""
        if self._kept is None:
            check(lib.mgx_lspar_minhashes(self._h, None))                      # raises
        out = np.empty((self.source.num_nodes, self._k), dtype=np.uint32)
        check(lib.mgx_lspar_minhashes(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def info(self):
        """the fused path's row classes and the last fused run: {"short_max", "seg", "k_max", "stride", "items"}"""
        out = (C.c_int64 * 5)()
        check(lib.mgx_lspar_info(self._h, out))
        return dict(zip(("short_max", "seg", "k_max", "stride", "items"), (int(x) for x in out)))

    def graph(self):
        """a new Graph owning a device copy of the last result"""
        h = C.c_void_p()
        check(lib.mgx_lspar_graph(self._h, C.byref(h)))
        return Graph(self.source.ctx, h)

    def close(self):
        if self._h:
            lib.mgx_lspar_free(self._h)
            self._h = None


class CcProblem:
    """Connected components: cc_problem_t + cc_enactor_t, and the fused path beside them.  labels() describes the last
    run of either path: label[v] = the smallest vertex id of v's weakly connected component."""

    SEED = 15485863

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_cc_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    @staticmethod
    def _stats(st):
        return {"components": st[0], "largest": st[1], "largest_label": st[2], "skipped": st[3], "host_waits": st[4]}

    def run(self, symmetric=False, seed=SEED):
        """fused path -> {"components", "largest", "largest_label", "skipped", "host_waits"}.  symmetric=True is the caller's word
        that every entry has its reverse (the final pass then skips the sampled largest set); False is right on any graph."""
        st = (C.c_int64 * 5)()
        check(lib.mgx_cc_run(self._h, int(bool(symmetric)), C.c_uint(seed & 0xFFFFFFFF), st))
        return self._stats(st)

    def enact(self):
        """operator path (hook advances, pointer-jumping filters); the same stats, skipped = 0"""
        st = (C.c_int64 * 5)()
        check(lib.mgx_cc_enact(self._h, st))
        return self._stats(st)

    def labels(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_cc_labels(self._h, _ptr(out)))
        return out

    def labels_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_cc_labels_device(self._h, C.byref(p)))
        return p.value

    def close(self):
        if self._h:
            lib.mgx_cc_free(self._h)
            self._h = None


class MstProblem:
    """Minimum spanning forest: mst_problem_t + mst_enactor_t, and the fused path beside them.  Every CSR entry
    (v, u, w) is the undirected edge {v, u}; edges are ordered by (key(w), min, max), so the forest is unique.  edges(), weight() and
    labels() describe the last run of either path."""

    KEYS = ("edges", "components", "largest", "largest_label", "rounds", "host_waits", "cursor_steps", "entries")
    INFO = ("long_items", "short_items", "long_min", "seg", "merge_passes", "setup_reused")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_mst_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._edges = None

    def _go(self, fn, symmetric):
        st = (C.c_int64 * 8)()
        self._edges = None
        check(fn(self._h, int(bool(symmetric)), st))
        self._edges = int(st[0])
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self, symmetric=False):
        """fused path -> the stats dict.  symmetric=True is the caller's word that every entry has its reverse with the same weight;
        False needs the graph's genuine CSC (Graph.build_csc)."""
        return self._go(lib.mgx_mst_run, symmetric)

    def enact(self, symmetric=False):
        """operator path (two advances and a hook filter per round); the same stats, cursor_steps = 0"""
        return self._go(lib.mgx_mst_enact, symmetric)

    def edges(self):
        """(a int32, b int32, w float32) of the forest's edges, a < b"""
        if self._edges is None:
            check(lib.mgx_mst_edges(self._h, None, None, None))                # raises: no run yet
        k = self._edges
        a, b = (np.empty(max(k, 1), dtype=np.int32) for _ in range(2))
        w = np.empty(max(k, 1), dtype=np.float32)
        check(lib.mgx_mst_edges(self._h, _ptr(a), _ptr(b), _ptr(w)))
        return a[:k], b[:k], w[:k]

    def edges_device_ptrs(self):
        p = [C.c_void_p() for _ in range(3)]
        check(lib.mgx_mst_edges_device(self._h, *(C.byref(x) for x in p)))
        return tuple(x.value for x in p)

    def weight(self):
        t = C.c_double()
        check(lib.mgx_mst_weight(self._h, C.byref(t)))
        return float(t.value)

    def labels(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_mst_labels(self._h, _ptr(out)))
        return out

    def labels_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_mst_labels_device(self._h, C.byref(p)))
        return p.value

    def info(self):
        """the last fused run: which path its rows took and the switches in effect"""
        out = (C.c_int64 * 8)()
        check(lib.mgx_mst_info(self._h, out))
        return dict(zip(self.INFO, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_mst_free(self._h)
            self._h = None


class TcProblem:
    """Triangle counting: tc_problem_t + tc_enactor_t, and the fused path beside them.  triangles(), simple_degrees()
    and dag() describe the last run of either path, on the underlying simple undirected graph, in original ids."""

    KEYS = ("triangles", "edges", "max_row", "wedges", "rows_sorted", "built", "host_waits", "launches")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_tc_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    def _go(self, fn, symmetric):
        st = (C.c_int64 * 8)()
        check(fn(self._h, int(bool(symmetric)), st))
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self, symmetric=False):
        """fused path -> {"triangles", "edges", "max_row", "wedges", "rows_sorted", "built", "host_waits", "launches"}.
        symmetric=True is the caller's word that every entry has its reverse; False is right on any graph."""
        return self._go(lib.mgx_tc_run, symmetric)

    def enact(self, symmetric=False):
        """operator path (one advance over the oriented graph, a thread per entry); the same stats"""
        return self._go(lib.mgx_tc_enact, symmetric)

    def triangles(self):
        """tri[v]: the triangles that contain v (int64)"""
        out = np.empty(self.graph.num_nodes, dtype=np.int64)
        check(lib.mgx_tc_triangles(self._h, _ptr(out)))
        return out

    def simple_degrees(self):
        """sdeg[v]: the distinct neighbours of v other than v (int32)"""
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_tc_simple_degrees(self._h, _ptr(out)))
        return out

    def dag(self):
        """(row_offsets, col_indices) of the oriented graph the last run counted on"""
        ro = np.empty(self.graph.num_nodes + 1, dtype=np.int32)
        check(lib.mgx_tc_dag(self._h, _ptr(ro), None))
        ci = np.empty(max(int(ro[-1]), 1), dtype=np.int32)
        check(lib.mgx_tc_dag(self._h, _ptr(ro), _ptr(ci)))
        return ro, ci[:int(ro[-1])]

    def bins(self):
        """which kernel the last run's rows go to on the fused path, and the switches in effect"""
        out = (C.c_int64 * 7)()
        check(lib.mgx_tc_bins(self._h, out))
        return dict(zip(("short_rows", "wave_rows", "block_rows", "block_stage", "wave_stage", "short_max", "wave_max"),
                        (int(x) for x in out)))

    def clustering(self):
        """local clustering coefficient 2 tri / (sdeg (sdeg - 1)) as float64, 0 where sdeg < 2"""
        tri, d = self.triangles().astype(np.float64), self.simple_degrees().astype(np.float64)
        out = np.zeros(len(tri), dtype=np.float64)
        ok = d >= 2
        out[ok] = 2.0 * tri[ok] / (d[ok] * (d[ok] - 1.0))
        return out

    def transitivity(self):
        """3 triangles / connected triples: sum of tri / sum of sdeg (sdeg - 1) / 2"""
        tri, d = self.triangles(), self.simple_degrees().astype(np.int64)
        triples = int((d * (d - 1) // 2).sum())
        return float(int(tri.sum())) / triples if triples else 0.0

    def triangles_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_tc_triangles_device(self._h, C.byref(p)))
        return p.value

    def simple_degrees_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_tc_simple_degrees_device(self._h, C.byref(p)))
        return p.value

    def close(self):
        if self._h:
            lib.mgx_tc_free(self._h)
            self._h = None


class KtrussProblem(_StepKinds, _Timed):
    """k-truss decomposition: ktruss_problem_t + ktruss_enactor_t, and the fused path beside them, on the underlying
    simple undirected graph, in original ids.  The getters describe the last run of either path.  step_kinds() are the launches of
    the last run()'s peel; a timed run() records events round its support launches and its peel."""

    _C = "mgx_ktruss"
    KEYS = ("max_truss", "edges", "triangles", "levels", "passes", "built", "host_waits", "launches")
    STEP_KINDS = {1: "min", 2: "list", 3: "expand", 4: "seal", 5: "idle"}
    PHASES = ("support", "peel")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_ktruss_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._m = None

    def _go(self, fn, symmetric):
        st = (C.c_int64 * 8)()
        self._m = None
        check(fn(self._h, int(bool(symmetric)), st))
        self._m = int(st[1])
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self, symmetric=True):
        """fused path -> the stats dict of KEYS.  symmetric=True is the caller's word that every entry has its reverse; False is
        right on any graph."""
        return self._go(lib.mgx_ktruss_run, symmetric)

    def enact(self, symmetric=True):
        """operator path (one advance for the supports, three filters over edge ids per pass); the same stats"""
        return self._go(lib.mgx_ktruss_enact, symmetric)

    def _edge_count(self):
        if self._m is None:
            check(lib.mgx_ktruss_edges(self._h, None, None, None))            # raises: no run yet
        return self._m

    def _raw_edges(self):
        m = self._edge_count()
        a, b, t = (np.empty(max(m, 1), dtype=np.int32) for _ in range(3))
        check(lib.mgx_ktruss_edges(self._h, _ptr(a), _ptr(b), _ptr(t)))
        return a[:m], b[:m], t[:m]

    def _canonical(self):
        """(u, v, permutation): the edges with u < v, sorted by (u, v) -- the same whatever orientation the run used"""
        a, b, _ = self._raw_edges()
        u, v = np.minimum(a, b), np.maximum(a, b)
        perm = np.lexsort((v, u))
        return u[perm], v[perm], perm

    def edges(self):
        """(u int32, v int32, truss int32) with u < v, sorted by (u, v)"""
        u, v, perm = self._canonical()
        return u, v, self._raw_edges()[2][perm]

    def support(self):
        """the triangles that contain each edge (int32), in the order of edges()"""
        m = self._edge_count()
        out = np.empty(max(m, 1), dtype=np.int32)
        check(lib.mgx_ktruss_support(self._h, _ptr(out)))
        return out[:m][self._canonical()[2]]

    def vertex_truss(self):
        """vtruss[v]: the largest trussness of an edge at v, 0 if there is none (int32)"""
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_ktruss_vertex_truss(self._h, _ptr(out)))
        return out

    def histogram(self):
        """hist[k]: the edges of trussness k (int64), k = 0 .. the largest trussness"""
        cap = self.graph.num_nodes + 1
        out = (C.c_int64 * cap)()
        check(lib.mgx_ktruss_histogram(self._h, out, cap))
        h = np.array(out[:], dtype=np.int64)
        top = int(np.flatnonzero(h).max()) if h.any() else 0
        return h[:top + 1]

    def order(self):
        """the peel order of the last run(): edge ids (positions of the oriented graph's entries); every front is a range of it"""
        m = self._edge_count()
        out = np.empty(max(m, 1), dtype=np.int32)
        check(lib.mgx_ktruss_order(self._h, _ptr(out)))
        return out[:m]

    def adjacency(self):
        """(row_offsets, col_indices, edge_ids): row v = the simple neighbours of v ascending, each with its edge's id"""
        m = self._edge_count()
        ro = np.empty(self.graph.num_nodes + 1, dtype=np.int32)
        ci, eid = (np.empty(max(2 * m, 1), dtype=np.int32) for _ in range(2))
        check(lib.mgx_ktruss_adjacency(self._h, _ptr(ro), _ptr(ci), _ptr(eid)))
        return ro, ci[:2 * m], eid[:2 * m]

    def raw_edges(self):
        """(src, dst, truss) in the order of the oriented graph's entries: what the edge ids of order() and adjacency() index"""
        return self._raw_edges()

    def truss_edges(self, k):
        """(u, v) of the edges of trussness >= k: the k-truss with its isolated vertices dropped"""
        u, v, t = self.edges()
        keep = t >= k
        return u[keep], v[keep]

    def truss_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_ktruss_truss_device(self._h, C.byref(p)))
        return p.value

    def vertex_truss_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_ktruss_vertex_truss_device(self._h, C.byref(p)))
        return p.value

    def close(self):
        if self._h:
            lib.mgx_ktruss_free(self._h)
            self._h = None


class SccProblem(_StepKinds, _Timed):
    """Strongly connected components: scc_problem_t + scc_enactor_t, and the fused path beside them, on the directed
    graph of the CSR entries, which needs its genuine CSC (Graph.build_csc, or one uploaded with the graph).  labels() describes
    the last run of either path: label[v] = the smallest vertex id of v's strongly connected component.  PHASES: the degree init,
    the trims, the pivot phase and the rounds, by the device's wall clock in every launch of a timed run()."""

    _C = "mgx_scc"
    KEYS = ("components", "largest", "largest_label", "trimmed", "pivot_size", "rounds", "host_waits", "launches")
    STEP_KINDS = {1: "degrees", 2: "list", 3: "expand", 4: "pivot_max", 5: "pivot_pick", 6: "round_init", 7: "forward", 8: "roots",
                  9: "backward", 10: "seal", 11: "idle"}
    PHASES = ("init", "trim", "pivot", "rounds")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_scc_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    def _go(self, fn):
        st = (C.c_int64 * 8)()
        check(fn(self._h, st))
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self):
        """fused path -> the stats dict of KEYS"""
        return self._go(lib.mgx_scc_run)

    def enact(self):
        """operator path (recounting filters for the trims and the pivot, advances forward and over the transposed graph); the
        same stats"""
        return self._go(lib.mgx_scc_enact)

    def labels(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_scc_labels(self._h, _ptr(out)))
        return out

    def labels_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_scc_labels_device(self._h, C.byref(p)))
        return p.value

    def close(self):
        if self._h:
            lib.mgx_scc_free(self._h)
            self._h = None


class LpaProblem(_StepKinds, _Timed):
    """Label propagation: lpa_problem_t + lpa_enactor_t, and the fused path beside them.  Every vertex takes the label
    most of its votes carry; labels() describes the last run of either path.  symmetric=True is the caller's word that every
    entry has its reverse; symmetric=False counts every entry at both of its ends and needs the graph's genuine CSC.  PHASES are
    timed by the device's wall clock in every launch of a timed run()."""

    _C = "mgx_lpa"
    SYNC, LAZY = _lib.MGX_LPA_SYNC, _lib.MGX_LPA_LAZY
    SEED = 15485863
    KEYS = ("communities", "largest", "largest_label", "iterations", "converged", "unstable", "evaluated", "overflowed", "host_waits",
            "launches")
    STEP_KINDS = {1: "setup", 2: "evaluate_dense", 3: "evaluate_list", 4: "long_rows", 5: "apply_dense", 6: "apply_list", 7: "idle",
                  8: "mark_long_rows"}
    PHASES = ("setup", "evaluate", "long_rows", "apply")
    BINS = ("rows_none", "rows_short", "rows_wave", "rows_long", "short_max", "wave_max", "table", "list_div", "overflowed")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_lpa_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._symmetric = False

    def _go(self, fn, symmetric, mode, seed, max_iter):
        st = (C.c_int64 * 10)()
        check(fn(self._h, int(bool(symmetric)), int(mode), int(seed) & 0xFFFFFFFF, int(max_iter), st))
        self._symmetric = bool(symmetric)
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self, symmetric=False, mode=LAZY, seed=SEED, max_iter=100):
        """fused path -> the stats dict of KEYS"""
        return self._go(lib.mgx_lpa_run, symmetric, mode, seed, max_iter)

    def enact(self, symmetric=False, mode=LAZY, seed=SEED, max_iter=100):
        """operator path (gathering advances, the segmented sort, a scanning and an applying filter); the same stats"""
        return self._go(lib.mgx_lpa_enact, symmetric, mode, seed, max_iter)

    def labels(self):
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_lpa_labels(self._h, _ptr(out)))
        return out

    def labels_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_lpa_labels_device(self._h, C.byref(p)))
        return p.value

    def trace(self):
        """int64[iterations + 1, 3] of the last run: unstable, changed, evaluated per iteration"""
        n = C.c_int64()
        check(lib.mgx_lpa_trace(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.int64)
        check(lib.mgx_lpa_trace(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def bins(self):
        """the last run(): vertices per body, the switches as read, rows that overflowed their table"""
        out = (C.c_int64 * 9)()
        check(lib.mgx_lpa_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def modularity(self):
        """(Q, S_in, S_sq, W) of the last run's labels, with the votes of that run's `symmetric`"""
        return modularity(self.graph, self.labels_device_ptr() or 0, self._symmetric)

    def close(self):
        if self._h:
            lib.mgx_lpa_free(self._h)
            self._h = None


class LouvainProblem(_Timed):
    """Louvain community detection: levels of local moves that raise the modularity, each contracted into the next
    level's weighted graph.  Integer arithmetic throughout: the run agrees with tests/louvain_model.py bit for bit.
    symmetric=True is the caller's word that every entry has its reverse; symmetric=False counts every entry at both of its ends
    and needs the graph's genuine CSC.  PHASES are timed by the device's wall clock in every launch of a timed run(), the
    aggregation by the host's."""

    _C = "mgx_louvain"
    SEED = 0x9E3779B9
    KEYS = ("communities", "largest", "largest_id", "levels", "s_in", "s_sq", "w", "host_waits", "launches", "iterations")
    LEVEL_KEYS = ("vertices", "entries", "iterations", "accepted", "communities", "qnum")
    STEP_KINDS = {1: "setup", 2: "evaluate", 3: "long_fill", 4: "long_scan", 5: "apply", 6: "qnum", 7: "done"}
    PHASES = ("setup", "evaluate", "long_rows", "apply", "qnum", "aggregate")
    BINS = ("rows_none", "rows_short", "rows_wave", "rows_long", "short_max", "wave_max", "seg", "long_items")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_louvain_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._stats = None

    def _go(self, fn, symmetric, seed, max_iter, max_levels, tol):
        st = (C.c_int64 * 10)()
        self._stats = None
        check(fn(self._h, int(bool(symmetric)), int(seed) & 0xFFFFFFFF, int(max_iter), int(max_levels), float(tol), st))
        self._stats = dict(zip(self.KEYS, (int(x) for x in st)))
        return dict(self._stats)

    def run(self, symmetric=True, seed=SEED, max_iter=100, max_levels=32, tol=0.0):
        """fused path -> the stats dict of KEYS"""
        return self._go(lib.mgx_louvain_run, symmetric, seed, max_iter, max_levels, tol)

    def enact(self, symmetric=True, seed=SEED, max_iter=100, max_levels=32, tol=0.0):
        """operator path (gathering advances, the segmented sort, a scanning and an applying filter per iteration); the same
        stats, `launches` being its operator calls"""
        return self._go(lib.mgx_louvain_enact, symmetric, seed, max_iter, max_levels, tol)

    def levels(self):
        """the levels that ran, the last one that accepted nothing included: a dict of LEVEL_KEYS each"""
        n = C.c_int64()
        check(lib.mgx_louvain_levels(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 6), dtype=np.int64)
        check(lib.mgx_louvain_levels(self._h, _ptr(out), n.value, C.byref(n)))
        return [dict(zip(self.LEVEL_KEYS, (int(x) for x in row))) for row in out]

    def labels(self, level=None):
        """level=None: the final communities of the n vertices; else the map of that aggregated level's vertices"""
        if level is None:
            count, level = self.graph.num_nodes, -1
        else:
            count = self.levels()[level]["vertices"]
        out = np.empty(count, dtype=np.int32)
        check(lib.mgx_louvain_labels(self._h, int(level), _ptr(out)))
        return out

    def labels_device_ptr(self, level=None):
        p = C.c_void_p()
        check(lib.mgx_louvain_labels_device(self._h, -1 if level is None else int(level), C.byref(p)))
        return p.value

    def dendrogram(self):
        """the aggregated levels' maps, bottom up: composing them gives labels()"""
        return [self.labels(level) for level in range(self._stats["levels"])] if self._stats else []

    def modularity(self):
        """Q of the last run's final labels; the division is done here"""
        s = self._stats
        if not s or s["w"] == 0:
            return 0.0
        return s["s_in"] / s["w"] - s["s_sq"] / (s["w"] * s["w"])

    def trace(self):
        """int64[iterations, 3] of the last run, the levels one behind the other: moved, accepted, Qnum of the moved labelling"""
        n = C.c_int64()
        check(lib.mgx_louvain_trace(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.int64)
        check(lib.mgx_louvain_trace(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def step_kinds(self):
        """what every launch of the last run's chains was, each level up to its first `done`: codes of STEP_KINDS"""
        n = C.c_int64()
        check(lib.mgx_louvain_step_kinds(self._h, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.int32)
        check(lib.mgx_louvain_step_kinds(self._h, _ptr(out), len(out), C.byref(n)))
        return out

    def bins(self):
        """the last run: vertices per body over the levels, the switches as read, the long rows' items over all iterations"""
        out = (C.c_int64 * 8)()
        check(lib.mgx_louvain_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_louvain_free(self._h)
            self._h = None


class MsBfsProblem(_Timed):
    """Bit-parallel multi-source BFS: BFS depths from many sources at once, 64 traversals to a 64-bit word per vertex,
    and what follows from them -- reach, farness, eccentricity, harmonic and closeness centrality per source, and per vertex how
    many sources reach it and the sum of their depths.  run() is the fused path, enact() the operator path; the getters describe
    the last run of either.  Depths follow the out-entries: on a directed graph closeness() and harmonic() are the OUT-closeness
    and the out-harmonic centrality of the sources (networkx's closeness_centrality is the in-closeness: run on the reversed graph
    to get that).  symmetric=True is the caller's word that every entry has its reverse, which lets the dense levels pull over
    the rows themselves; symmetric=False pulls over the graph's genuine CSC where it has one and pushes every level where not."""

    _C = "mgx_msbfs"
    KEYS = ("sources", "batches", "deepest", "reach", "push_levels", "pull_levels", "host_waits", "launches", "csc", "depths")
    PUSH, PULL = _lib.MGX_MSBFS_PUSH, _lib.MGX_MSBFS_PULL
    PHASES = ("push", "pull", "long_rows", "finalize")
    BINS = ("out_none", "out_short", "out_wave", "out_long", "out_segments", "in_none", "in_short", "in_wave", "in_long", "in_segments",
            "short_max", "wave_max", "seg", "pull_div")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_msbfs_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._count = 0

    def _go(self, fn, sources, symmetric, depths):
        st = (C.c_int64 * 10)()
        if sources is None:
            src, ptr, count = None, None, 0
        else:
            src = _np_i32(np.asarray(sources))
            ptr, count = _ptr(src), len(src)
            if count == 0:
                src = np.zeros(1, dtype=np.int32)                # (NULL would mean every vertex)
                ptr = _ptr(src)
        check(fn(self._h, ptr, count, int(bool(symmetric)), int(bool(depths)), st))
        out = dict(zip(self.KEYS, (int(x) for x in st)))
        self._count = out["sources"]
        return out

    def run(self, sources=None, symmetric=False, depths=False):
        """fused path from `sources` (None: every vertex) -> the stats dict of KEYS"""
        return self._go(lib.mgx_msbfs_run, sources, symmetric, depths)

    def enact(self, sources=None, symmetric=False, depths=False):
        """operator path (an advance that ORs and a filter that finalizes per level; it always pushes); the same results"""
        return self._go(lib.mgx_msbfs_enact, sources, symmetric, depths)

    def _per_source(self, fn, dtype):
        out = np.zeros(max(self._count, 1), dtype=dtype)
        check(fn(self._h, _ptr(out)))
        return out[:self._count]

    def reach(self):
        """int64[count]: the vertices every source reaches, itself not counted"""
        return self._per_source(lib.mgx_msbfs_reach, np.int64)

    def farness(self):
        """int64[count]: the sum of the depths of the vertices every source reaches"""
        return self._per_source(lib.mgx_msbfs_far, np.int64)

    def eccentricity(self):
        """int64[count]: the depth of the deepest vertex every source reaches"""
        return self._per_source(lib.mgx_msbfs_ecc, np.int64)

    def harmonic(self):
        """float64[count]: the sum of 1 / depth over the vertices every source reaches (out-entries: see the class)"""
        return self._per_source(lib.mgx_msbfs_harmonic, np.float64)

    def closeness(self):
        """float64[count]: reach / far * reach / (n - 1) (Wasserman-Faust; networkx's wf_improved=True), 0 where far == 0; the
        OUT-closeness on a directed graph"""
        reach, far = self.reach().astype(np.float64), self.farness().astype(np.float64)
        n = self.graph.num_nodes
        out = np.zeros(len(reach), dtype=np.float64)
        ok = far > 0
        out[ok] = reach[ok] / far[ok] * (reach[ok] / (n - 1))
        return out

    def vertex_sums(self):
        """(reach_in, far_in), int64[n] each: the run's sources that reach every vertex and the sum of their depths there"""
        n = self.graph.num_nodes
        r, f = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        check(lib.mgx_msbfs_vertex_sums(self._h, _ptr(r), _ptr(f)))
        return r[:n], f[:n]

    def vertex_sums_device_ptrs(self):
        r, f = C.c_void_p(), C.c_void_p()
        check(lib.mgx_msbfs_vertex_sums_device(self._h, C.byref(r), C.byref(f)))
        return r.value, f.value

    def depths(self):
        """int32[count, n] of the last run with depths=True: -1 where the source does not reach the vertex"""
        n = self.graph.num_nodes
        out = np.zeros(max(self._count * n, 1), dtype=np.int32)
        check(lib.mgx_msbfs_depths(self._h, _ptr(out)))
        return out[:self._count * n].reshape(self._count, n)

    def level_kinds(self):
        """PUSH or PULL per (batch, level) of the last run(), the batches behind each other (the first 65536)"""
        n = C.c_int64()
        check(lib.mgx_msbfs_level_kinds(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(min(n.value, CHAIN_LOG_CAP), 1), dtype=np.int32)
        check(lib.mgx_msbfs_level_kinds(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:min(n.value, CHAIN_LOG_CAP)].copy()

    def bins(self):
        """the last run(): out- and in-rows per body, their segments, the switches as read"""
        out = (C.c_int64 * 14)()
        check(lib.mgx_msbfs_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_msbfs_free(self._h)
            self._h = None


class RandomWalkProblem(_Timed):
    """Random walks and node2vec sampling: DeepWalk / node2vec corpora, Monte-Carlo personalised PageRank, walk-based
    sampling.  run() is the fused path (one launch, a lane per walker), enact() the operator path (a filter per step); the getters
    describe the last run of either, and both give the same results bit for bit.  Every draw is a pure function of (seed, walker,
    step, draw): walker w's path does not depend on which other walkers run.  The fine print of the definition:
      * a pick is a position in the row's STORED order: two uploads of one graph with differently ordered rows walk differently;
      * a position in a row of d entries is the high word of a 32-bit draw times d: a position's probability is off 1 / d by at
        most 2^-32, a row's total bias at most d / 2^32;
      * weighted and second-order (p, q) steps sample by rejection; after MGX_RW_TRIES (64) rejected candidates a step takes the
        row's first maximum-weight entry and counts a fallback: the sampled distribution is the intended one exactly where
        stats["fallbacks"] == 0; the expected tries per step are wmax * max(1/p, 1, 1/q) / mean(w * b);
      * walks follow the OUT-entries: on a directed graph "prev has an entry to c" is asked of prev's out-row, and a vertex without
        out-entries ends the walk (restart > 0: it jumps to its start instead)."""

    _C = "mgx_rw"
    KEYS = ("walkers", "length", "steps", "dead_ends", "restarts", "tries", "fallbacks", "sorted_copy", "launches", "host_waits")
    PHASES = ("setup", "walk")
    BINS = ("none", "short", "wave", "long", "segments", "short_max", "wave_max", "seg", "tries", "tile")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_rw_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._walkers = self._length = 0

    def _go(self, fn, starts, length, walks_per_start, seed, weighted, p, q, restart, paths, visits):
        st = (C.c_int64 * 10)()
        if starts is None:
            src, ptr, count = None, None, 0
        else:
            src = _np_i32(np.asarray(starts))
            ptr, count = _ptr(src), len(src)
            if count == 0:
                src = np.zeros(1, dtype=np.int32)                # (NULL would mean every vertex)
                ptr = _ptr(src)
        check(fn(self._h, ptr, count, int(walks_per_start), int(length), int(seed) & 0xFFFFFFFF, int(bool(weighted)), float(p), float(q),
                 float(restart), int(bool(paths)), int(bool(visits)), st))
        out = dict(zip(self.KEYS, (int(x) for x in st)))
        self._walkers, self._length = out["walkers"], out["length"]
        return out

    def run(self, starts=None, length=80, walks_per_start=1, seed=1, weighted=False, p=1.0, q=1.0, restart=0.0, paths=True, visits=False):
        """fused path from `starts` (None: every vertex) -> the stats dict of KEYS"""
        return self._go(lib.mgx_rw_run, starts, length, walks_per_start, seed, weighted, p, q, restart, paths, visits)

    def enact(self, starts=None, length=80, walks_per_start=1, seed=1, weighted=False, p=1.0, q=1.0, restart=0.0, paths=True, visits=False):
        """operator path (a filter over the live walkers per step); the same results"""
        return self._go(lib.mgx_rw_enact, starts, length, walks_per_start, seed, weighted, p, q, restart, paths, visits)

    def paths(self):
        """int32[walkers, length + 1] of the last run with paths=True: slot 0 the start, -1 behind a walk's end"""
        w, k = self._walkers, self._length + 1
        out = np.zeros(max(w * k, 1), dtype=np.int32)
        check(lib.mgx_rw_paths(self._h, _ptr(out)))
        return out[:w * k].reshape(w, k)

    def _per_walker(self, fn):
        out = np.zeros(max(self._walkers, 1), dtype=np.int32)
        check(fn(self._h, _ptr(out)))
        return out[:self._walkers]

    def ends(self):
        """int32[walkers]: the last vertex of every walk"""
        return self._per_walker(lib.mgx_rw_ends)

    def lengths(self):
        """int32[walkers]: the steps every walk took"""
        return self._per_walker(lib.mgx_rw_lengths)

    def visits(self):
        """int64[n] of the last run with visits=True: the path slots that hold every vertex, the starts included"""
        n = self.graph.num_nodes
        out = np.zeros(max(n, 1), dtype=np.int64)
        check(lib.mgx_rw_visits(self._h, _ptr(out)))
        return out[:n]

    def ppr(self):
        """float64[n]: visits / visits.sum(), the Monte-Carlo personalised PageRank estimate of a run with restart > 0"""
        v = self.visits().astype(np.float64)
        total = v.sum()
        return v / total if total > 0 else v

    def paths_device_ptr(self):
        d = C.c_void_p()
        check(lib.mgx_rw_paths_device(self._h, C.byref(d)))
        return d.value

    def visits_device_ptr(self):
        d = C.c_void_p()
        check(lib.mgx_rw_visits_device(self._h, C.byref(d)))
        return d.value

    def bins(self):
        """rows per body of the handle's last setup launch (zeros before any), their segments, the switches as read"""
        out = (C.c_int64 * 10)()
        check(lib.mgx_rw_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_rw_free(self._h)
            self._h = None


class NeighborSampleProblem(_Timed):
    """Fan-out neighbour sampling for GNN mini-batches, the GraphSAGE / NeighborLoader shape: from a batch of seeds up
    to fanouts[h] out-neighbours of every newly reached vertex at hop h, the result one renumbered subgraph.  run() is the fused
    path (5 H + 4 launches, nothing read back between the hops), enact() the operator path; the getters describe the last run of
    either, and both give the same results bit for bit.  The fine print of the definition:
      * V_0 is the ascending set of distinct seeds, V_{h+1} the ascending set of hop h's sampled destinations that are in none of
        V_0 .. V_h; a vertex's local id is its place in V_0 | V_1 | ... | V_H.  A vertex is sampled at most once in a run, at the
        hop that reached it first;
      * a pick is a position in the row's STORED order: two uploads of one graph with differently ordered rows sample differently;
      * a row's key comes from (seed, the vertex's GLOBAL id, the hop): its sample does not depend on who else is in the batch;
      * a row of d entries at fan-out k: all of them, in stored order, when k == -1 or d <= k (replace=False); with replace=True k
        positions drawn independently; otherwise Floyd's algorithm, exactly k draws and no retries: t uniform in [0, d - k + j] for
        j = 0 .. k - 1, and d - k + j instead when t was picked before (a collision).  The picks stay in insertion order;
      * self-loops and duplicate entries are entries like any other; weights do not bias the sample (gather them with entry_pos())."""

    _C = "mgx_nsample"
    KEYS = ("seeds", "unique_seeds", "hops", "vertices", "rows", "edges", "empty_rows", "whole_rows", "sampled_rows", "draws", "collisions",
            "revisits", "launches", "host_waits")
    PHASES = ("sample", "dedup")
    BINS = ("none", "short", "wave", "long", "segments", "short_max", "wave_max", "seg")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_nsample_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._last = None

    def _go(self, fn, seeds, fanouts, replace, seed):
        st = (C.c_int64 * 14)()
        if seeds is None:
            src, ptr, count = None, None, 0
        else:
            src = _np_i32(np.asarray(seeds))
            ptr, count = _ptr(src), len(src)
            if count == 0:
                src = np.zeros(1, dtype=np.int32)                # (NULL would mean every vertex)
                ptr = _ptr(src)
        fo = _np_i32(np.asarray(list(fanouts) + [0]))            # (never an empty array)
        self._last = None
        check(fn(self._h, ptr, count, _ptr(fo), len(fo) - 1, int(bool(replace)), int(seed) & 0xFFFFFFFF, st))
        self._last = dict(zip(self.KEYS, (int(x) for x in st)))
        return dict(self._last)

    def run(self, seeds=None, fanouts=(15, 10, 5), replace=False, seed=1):
        """fused path from `seeds` (None: every vertex) -> the stats dict of KEYS"""
        return self._go(lib.mgx_nsample_run, seeds, fanouts, replace, seed)

    def enact(self, seeds=None, fanouts=(15, 10, 5), replace=False, seed=1):
        """operator path (a filter over the frontier per hop, a filter over all vertices for the next one); the same results"""
        return self._go(lib.mgx_nsample_enact, seeds, fanouts, replace, seed)

    def _get(self, fn, count):
        out = np.zeros(max(count, 1), dtype=np.int32)
        check(fn(self._h, _ptr(out)))
        return out[:count]

    def _size(self, key, extra=0):
        return (self._last[key] + extra) if self._last else 1

    def vertices(self):
        """int32[N]: local id -> global id"""
        return self._get(lib.mgx_nsample_vertices, self._size("vertices"))

    def hop_offsets(self):
        """int32[H + 2]: V_h = vertices()[hop_offsets[h]:hop_offsets[h + 1]]"""
        return self._get(lib.mgx_nsample_hop_offsets, self._size("hops", 2))

    def row_offsets(self):
        """int32[R + 1]: the sampled subgraph as a CSR over the local rows 0 .. R - 1, R = hop_offsets[H]"""
        return self._get(lib.mgx_nsample_row_offsets, self._size("rows", 1))

    def cols(self):
        """int32[E]: the sampled entries' destinations, local ids"""
        return self._get(lib.mgx_nsample_cols, self._size("edges"))

    def entry_pos(self):
        """int32[E]: the index into the graph's col_indices / weights of every sampled entry"""
        return self._get(lib.mgx_nsample_entry_pos, self._size("edges"))

    def seed_local(self):
        """int32[len(seeds)]: the local id of every seed, duplicates included"""
        return self._get(lib.mgx_nsample_seed_local, self._size("seeds"))

    def block(self, h):
        """(row_offsets, cols) of hop h's rows: row_offsets starts at 0, cols are local ids"""
        off, ro = self.hop_offsets(), self.row_offsets()
        if not 0 <= h < len(off) - 2:
            raise IndexError("hop %d of %d" % (h, len(off) - 2))
        part = ro[off[h]:off[h + 1] + 1]
        return part - part[0], self.cols()[part[0]:part[-1]]

    def _device(self, fn):
        d = C.c_void_p()
        check(fn(self._h, C.byref(d)))
        return d.value

    def vertices_device_ptr(self):
        return self._device(lib.mgx_nsample_vertices_device)

    def row_offsets_device_ptr(self):
        return self._device(lib.mgx_nsample_row_offsets_device)

    def cols_device_ptr(self):
        return self._device(lib.mgx_nsample_cols_device)

    def entry_pos_device_ptr(self):
        return self._device(lib.mgx_nsample_entry_pos_device)

    def bins(self):
        """rows per copy body of the last fused run's hops with fan-out -1, their segments, the switches as read"""
        out = (C.c_int64 * 8)()
        check(lib.mgx_nsample_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_nsample_free(self._h)
            self._h = None


class AggregateProblem(_Timed):
    """Neighbour feature aggregation for GNN layers: Y[r, :] = the reduction over row r's entries of the neighbours'
    feature rows X[col_e, :], optionally times the entry's weight -- the memory-bound step of a GraphSAGE / GCN layer.  run() is the
    fused path (a team of lanes per row, one launch; three with rows longer than seg), enact() the operator path (a lane per row);
    both give the same float32 bits as tests/agg_model.py, on every run.  The fine print of the definition:
      * the rows are the graph's out-rows (rows="out"), its in-rows (rows="in", after graph.build_csc()) or, with block=a
        NeighborSampleProblem, the rows of its last sampling run: hop h's, or all sampled rows with hop=None.  A block's columns are
        local ids: x is then indexed by local id (x[i] belongs to block.vertices()[i]);
      * a term is x[col, f], or weight * x[col, f] rounded once to float32 (weighted=True: the graph's weights, a block's through
        entry_pos, the CSC's row values for in-rows); the multiply and the add are never fused;
      * a row's entries are folded in STORED order, left to right, from its first term (not from zero); a row of more than seg
        entries (MGX_AGG_SEG, default 256) in segments of seg whose values are combined in segment order.  max and min are
        t > acc ? t : acc and t < acc ? t : acc, which fixes +-0 and NaN by the order;
      * mean is the sum divided by float32(d), correctly rounded; a row without entries gives 0.0 for every op;
      * every element of the result is written on every run, padding columns (ldy > feats) never.
    x and out may be numpy arrays (x is uploaded into the handle's buffer, the result stays in the handle's: result()), torch
    tensors, or device addresses (then with x_rows= and feats=)."""

    _C = "mgx_agg"
    KEYS = ("rows", "entries", "feats", "team_width", "col_tiles", "vector", "seg", "launches", "host_waits")
    PHASES = ("rows", "items", "fold")
    BINS = ("none", "team", "long", "segments", "seg")
    OPS = ("sum", "mean", "max", "min")
    ROWS = ("out", "in")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_agg_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._last = None

    def _rows_of(self, block, hop):
        if block is None:
            return self.graph.num_nodes
        if not block._last:
            return 0                                             # (the library refuses the block)
        if hop is None:
            return block._last["rows"]
        off = block.hop_offsets()
        return int(off[hop + 1] - off[hop]) if 0 <= hop < len(off) - 2 else 0

    def _go(self, fn, x, op, weighted, rows, block, hop, out, ldx, ldy, x_rows, feats):
        if op not in self.OPS or rows not in self.ROWS:
            raise ValueError("op must be one of %s and rows one of %s" % (self.OPS, self.ROWS))
        self._last = None
        if isinstance(x, np.ndarray):
            hx = np.ascontiguousarray(x, dtype=np.float32)
            if hx.ndim != 2:
                raise ValueError("x must be two-dimensional (x_rows, feats)")
            x_rows, feats = hx.shape
            d = C.c_void_p()
            check(lib.mgx_agg_upload(self._h, _ptr(hx), x_rows, max(feats, 1), C.byref(d)))
            d_x, ldx = d, feats
        else:
            if (x_rows is None or feats is None) and hasattr(x, "shape"):
                x_rows, feats = (int(s) for s in x.shape)          # a two-dimensional tensor
                if ldx is None and x_rows > 1:
                    ldx = int(x.stride(0))
            if x_rows is None or feats is None:
                raise ValueError("a device address needs x_rows= and feats=")
            d_x, ldx = _dev_ptr(x), feats if ldx is None else ldx
        R = self._rows_of(block, hop)
        if out is None:
            ldy = feats if ldy is None else ldy
            d = C.c_void_p()
            check(lib.mgx_agg_output(self._h, R, max(ldy, 1), C.byref(d)))
            d_y = d
        else:
            if ldy is None:
                ldy = int(out.stride(0)) if hasattr(out, "stride") and len(out.shape) == 2 and out.shape[0] > 1 else feats
            d_y = _dev_ptr(out)
        st = (C.c_int64 * 9)()
        source = 2 if block is not None else self.ROWS.index(rows)
        check(fn(self._h, source, None if block is None else block._h, -1 if hop is None else int(hop), d_x, int(x_rows), int(ldx), int(feats),
                 self.OPS.index(op), int(bool(weighted)), d_y, int(ldy), st))
        self._last = dict(zip(self.KEYS, (int(v) for v in st)))
        return dict(self._last)

    def run(self, x, op="sum", weighted=False, rows="out", block=None, hop=None, out=None, ldx=None, ldy=None, x_rows=None, feats=None):
        """fused path -> the stats dict of KEYS; only enqueues on the context's stream (a run that builds a plan waits once)"""
        return self._go(lib.mgx_agg_run, x, op, weighted, rows, block, hop, out, ldx, ldy, x_rows, feats)

    def enact(self, x, op="sum", weighted=False, rows="out", block=None, hop=None, out=None, ldx=None, ldy=None, x_rows=None, feats=None):
        """operator path (one filter over the rows, a lane per row); the same bits"""
        return self._go(lib.mgx_agg_enact, x, op, weighted, rows, block, hop, out, ldx, ldy, x_rows, feats)

    def result(self):
        """float32[R, feats]: the last call's result, from wherever it was written (waits)"""
        R, F = (self._last["rows"], self._last["feats"]) if self._last else (0, 1)
        y = np.zeros((max(R, 1), F), dtype=np.float32)
        check(lib.mgx_agg_result(self._h, _ptr(y)))
        return y[:R]

    def bins(self):
        """the last fused run's rows without entries, of at most seg entries (a team's), longer ones, their segments, and seg (waits)"""
        out = (C.c_int64 * 5)()
        check(lib.mgx_agg_bins(self._h, out))
        return dict(zip(self.BINS, (int(v) for v in out)))

    def close(self):
        if self._h:
            lib.mgx_agg_free(self._h)
            self._h = None


class AggregateGradProblem(_Timed):
    """The backward of AggregateProblem: GX[c, :] = the sum over the selected rows' entries e with col_e == c of the
    upstream gradient's rows gy[row_e, :], optionally times the entry's weight -- the gradient with respect to the features x.
    run() is the fused path (a team of lanes per TRANSPOSED row, no atomics on GX), enact() the operator path; both give the same
    float32 bits as tests/aggbwd_model.py, on every run.  The fine print:
      * rows=, block=, hop=, weighted= and op= say which forward is differentiated, as AggregateProblem takes them; gy has that
        forward's rows, the result has x_rows rows (default: the graph's n, or the block's vertices);
      * mean divides gy[r, f] by float32(d_r) first, one correctly rounded division, then the weight is applied, rounded once;
        the multiply and the add are never fused;
      * max and min need x= (the forward's x): the gradient goes to the entry whose term the forward's fold kept (the first of
        equal values), every other entry contributes +0.0;
      * a column's terms are added in ASCENDING entry order, the forward's stored order, in segments of seg (MGX_AGG_SEG) whose
        values are added in segment order; a vertex that is nobody's neighbour gets +0.0;
      * every element of the result is written on every run, padding columns (ldgx > feats) never;
      * the gradient with respect to the edge weights is not built.
    The transposed CSR is built on the device by the first run on the out-rows / in-rows and kept; for a block by every run.
    gy, x and out may be numpy arrays (uploaded into the handle's buffers, the result stays in the handle's: result()), torch
    tensors, or device addresses (then with rows_gy= / x_rows= and feats=)."""

    _C = "mgx_aggbwd"
    KEYS = ("rows", "entries", "feats", "team_width", "col_tiles", "vector", "seg", "launches", "host_waits", "built")
    PHASES = ("transpose", "winners", "rows", "items", "fold")
    BINS = ("none", "team", "long", "segments", "seg")
    OPS = AggregateProblem.OPS
    ROWS = AggregateProblem.ROWS

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_aggbwd_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._last = None

    def _device(self, a, which, ld, feats):
        """-> (device address, leading dimension, rows, feats) of gy (which 0) or x (which 1)"""
        if isinstance(a, np.ndarray):
            ha = np.ascontiguousarray(a, dtype=np.float32)
            if ha.ndim != 2:
                raise ValueError("gy and x must be two-dimensional (rows, feats)")
            d = C.c_void_p()
            check(lib.mgx_aggbwd_upload(self._h, which, _ptr(ha), ha.shape[0], max(ha.shape[1], 1), C.byref(d)))
            return d, ha.shape[1], ha.shape[0], ha.shape[1]
        rows = None
        if hasattr(a, "shape") and len(a.shape) == 2:
            rows, feats = (int(s) for s in a.shape)
            if ld is None and rows > 1:
                ld = int(a.stride(0))
        return _dev_ptr(a), ld, rows, feats

    def _go(self, fn, gy, op, weighted, rows, block, hop, x, out, ldgy, ldx, ldgx, x_rows, feats):
        if op not in self.OPS or rows not in self.ROWS:
            raise ValueError("op must be one of %s and rows one of %s" % (self.OPS, self.ROWS))
        self._last = None
        d_gy, ldgy, _, feats = self._device(gy, 0, ldgy, feats)
        if feats is None:
            raise ValueError("a device address needs feats=")
        ldgy = feats if ldgy is None else ldgy
        d_x, have = None, None
        if x is not None and op in ("max", "min"):
            d_x, ldx, have, _ = self._device(x, 1, ldx, feats)
            ldx = feats if ldx is None else ldx
        if x_rows is None:
            x_rows = have if have is not None else (self.graph.num_nodes if block is None else (block._last or {}).get("vertices", 0))
        if out is None:
            ldgx = feats if ldgx is None else ldgx
            d = C.c_void_p()
            check(lib.mgx_aggbwd_output(self._h, x_rows, max(ldgx, 1), C.byref(d)))
            d_gx = d
        else:
            if ldgx is None:
                ldgx = int(out.stride(0)) if hasattr(out, "stride") and len(out.shape) == 2 and out.shape[0] > 1 else feats
            d_gx = _dev_ptr(out)
        st = (C.c_int64 * 10)()
        source = 2 if block is not None else self.ROWS.index(rows)
        check(fn(self._h, source, None if block is None else block._h, -1 if hop is None else int(hop), d_gy, int(ldgy), int(feats),
                 self.OPS.index(op), int(bool(weighted)), d_x, int(ldx or feats), int(x_rows), d_gx, int(ldgx), st))
        self._last = dict(zip(self.KEYS, (int(v) for v in st)))
        return dict(self._last)

    def run(self, gy, op="sum", weighted=False, rows="out", block=None, hop=None, x=None, out=None, ldgy=None, ldx=None, ldgx=None, x_rows=None,
            feats=None):
        """fused path -> the stats dict of KEYS; a repeat run on a kept transpose only enqueues on the context's stream"""
        return self._go(lib.mgx_aggbwd_run, gy, op, weighted, rows, block, hop, x, out, ldgy, ldx, ldgx, x_rows, feats)

    def enact(self, gy, op="sum", weighted=False, rows="out", block=None, hop=None, x=None, out=None, ldgy=None, ldx=None, ldgx=None, x_rows=None,
              feats=None):
        """operator path (one filter over the result's rows, a lane per transposed row); the same bits"""
        return self._go(lib.mgx_aggbwd_enact, gy, op, weighted, rows, block, hop, x, out, ldgy, ldx, ldgx, x_rows, feats)

    def result(self):
        """float32[x_rows, feats]: the last call's result, from wherever it was written (waits)"""
        R, F = (self._last["rows"], self._last["feats"]) if self._last else (0, 1)
        gx = np.zeros((max(R, 1), F), dtype=np.float32)
        check(lib.mgx_aggbwd_result(self._h, _ptr(gx)))
        return gx[:R]

    def transpose(self):
        """(offsets int32[x_rows + 1], rows int32[E], pos int32[E]): the transposed CSR the last call ran on (waits)"""
        R, E = (self._last["rows"], self._last["entries"]) if self._last else (0, 0)
        off, row, pos = np.zeros(R + 1, dtype=np.int32), np.zeros(max(E, 1), dtype=np.int32), np.zeros(max(E, 1), dtype=np.int32)
        check(lib.mgx_aggbwd_transpose(self._h, _ptr(off), _ptr(row), _ptr(pos)))
        return off, row[:E], pos[:E]

    def bins(self):
        """the last fused run's transposed rows without entries, of at most seg entries, longer ones, their segments, and seg (waits)"""
        out = (C.c_int64 * 5)()
        check(lib.mgx_aggbwd_bins(self._h, out))
        return dict(zip(self.BINS, (int(v) for v in out)))

    def close(self):
        if self._h:
            lib.mgx_aggbwd_free(self._h)
            self._h = None


class SimilarityProblem(_Timed):
    """Vertex similarity for link prediction: how alike are two vertices' neighbourhoods, exactly, for arbitrary pairs
    or for every edge.  The graph is the underlying simple undirected graph of the triangle count: N(v) = the distinct neighbours of
    v other than v, d(v) = |N(v)|, original ids; symmetric as in TcProblem.run.  run() is the fused path (one classifying launch,
    pair kernels by row lengths, one scoring launch), enact() the operator path (one filter, a merge per thread); the getters
    describe the last run of either.  With c = |N(u) & N(v)|:
      common   c                          jaccard  c / (d(u) + d(v) - c)       overlap  c / min(d(u), d(v))
      sorensen 2 c / (d(u) + d(v))        cosine   c / sqrt(d(u) d(v))         (each 0 where its denominator is 0)
      weighted the sum of weights[w] over the common neighbours w: weights="adamic_adar" is 1 / ln d (0 where d < 2),
               "resource_allocation" 1 / d (0 where d == 0), built here with numpy from degrees(); or any float64[n]
    pairs=None is edges mode: the pairs are the simple graph's edges in the order of KtrussProblem.edges().  u == v and duplicate
    pairs are legal; an id outside [0, n) raises MgxError(MGX_E_INVALID).  The ratios are bit-equal to numpy's division; the weighted
    sum uses a fixed order (two runs are bit-equal) and score(u, v) == score(v, u) bit for bit."""

    _C = "mgx_sim"
    KEYS = ("pairs", "common", "positive", "entries", "longest_row", "built", "host_waits", "launches")
    MEASURES = {"common": _lib.MGX_SIM_COMMON, "jaccard": _lib.MGX_SIM_JACCARD, "overlap": _lib.MGX_SIM_OVERLAP,
                "sorensen": _lib.MGX_SIM_SORENSEN, "cosine": _lib.MGX_SIM_COSINE, "weighted": _lib.MGX_SIM_WEIGHTED}
    PHASES = ("build", "classify", "pairs")
    BINS = ("none", "lane", "probe", "wave", "block", "short_max", "probe_ratio", "wave_max", "stage", "entries_read")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_sim_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._pairs = None

    def degrees(self, symmetric=True):
        """int32[n]: d(v) of the simple graph (builds the adjacency of `symmetric` when the handle does not have it)"""
        check(lib.mgx_sim_prepare(self._h, int(bool(symmetric))))
        n = self.graph.num_nodes
        out = np.zeros(max(n, 1), dtype=np.int32)
        check(lib.mgx_sim_degrees(self._h, _ptr(out)))
        return out[:n]

    def weights(self, kind, symmetric=True):
        """float64[n] for measure="weighted": "adamic_adar" 1 / ln d (0 where d < 2), "resource_allocation" 1 / d (0 where d == 0)"""
        d = self.degrees(symmetric).astype(np.float64)
        x = np.zeros(len(d), dtype=np.float64)
        if kind == "adamic_adar":
            ok = d >= 2
            x[ok] = 1.0 / np.log(d[ok])
        elif kind == "resource_allocation":
            ok = d > 0
            x[ok] = 1.0 / d[ok]
        else:
            raise ValueError("weights: 'adamic_adar', 'resource_allocation' or an array of n doubles")
        return x

    def _go(self, fn, pairs, measure, weights, symmetric):
        st = (C.c_int64 * 8)()
        if weights is not None:
            measure = "weighted"                                 # (weights given: the measure is their sum over the common neighbours)
        code = self.MEASURES[measure] if isinstance(measure, str) else int(measure)
        x = None
        if code == _lib.MGX_SIM_WEIGHTED:
            if weights is None:
                raise ValueError("measure 'weighted' needs weights")
            x = self.weights(weights, symmetric) if isinstance(weights, str) else np.ascontiguousarray(weights, dtype=np.float64)
            if len(x) != self.graph.num_nodes:
                raise ValueError("weights: %d values for %d vertices" % (len(x), self.graph.num_nodes))
            if len(x) == 0:
                x = np.zeros(1, dtype=np.float64)
        if pairs is None:
            u = v = None
            pu = pv = None
            count = 0
        else:
            pr = np.asarray(pairs).reshape(-1, 2)
            u, v = _np_i32(pr[:, 0]), _np_i32(pr[:, 1])
            count = len(u)
            if count == 0:
                u = v = np.zeros(1, dtype=np.int32)              # (NULL would mean edges mode)
            pu, pv = _ptr(u), _ptr(v)
        self._pairs = None
        check(fn(self._h, int(bool(symmetric)), pu, pv, count, code, None if x is None else _ptr(x), st))
        out = dict(zip(self.KEYS, (int(s) for s in st)))
        self._pairs = out["pairs"]
        return out

    def run(self, pairs=None, measure="jaccard", weights=None, symmetric=True):
        """fused path over `pairs` (anything that reshapes to (P, 2); None: every edge) -> the stats dict of KEYS"""
        return self._go(lib.mgx_sim_run, pairs, measure, weights, symmetric)

    def enact(self, pairs=None, measure="jaccard", weights=None, symmetric=True):
        """operator path (one filter over the pair indices, a two-pointer merge per thread); the same results and stats"""
        return self._go(lib.mgx_sim_enact, pairs, measure, weights, symmetric)

    def _count(self):
        if self._pairs is None:
            check(lib.mgx_sim_common(self._h, None))             # raises: no run yet
        return self._pairs or 0

    def common(self):
        """int32[P]: the common neighbours of every pair"""
        p = self._count()
        out = np.zeros(max(p, 1), dtype=np.int32)
        check(lib.mgx_sim_common(self._h, _ptr(out)))
        return out[:p]

    def scores(self):
        """float64[P]: the chosen measure of every pair"""
        p = self._count()
        out = np.zeros(max(p, 1), dtype=np.float64)
        check(lib.mgx_sim_scores(self._h, _ptr(out)))
        return out[:p]

    def pairs(self):
        """int32[P, 2]: the last run's pairs (edges mode: the edges it generated, (src, dst) of KtrussProblem.edges())"""
        p = self._count()
        u, v = np.zeros(max(p, 1), dtype=np.int32), np.zeros(max(p, 1), dtype=np.int32)
        check(lib.mgx_sim_pairs(self._h, _ptr(u), _ptr(v)))
        return np.stack([u[:p], v[:p]], axis=1)

    def common_device_ptr(self):
        d = C.c_void_p()
        check(lib.mgx_sim_common_device(self._h, C.byref(d)))
        return d.value

    def scores_device_ptr(self):
        d = C.c_void_p()
        check(lib.mgx_sim_scores_device(self._h, C.byref(d)))
        return d.value

    def bins(self):
        """the last run(): pairs per class, the cuts as read, the adjacency entries the pair kernels loaded"""
        out = (C.c_int64 * 10)()
        check(lib.mgx_sim_bins(self._h, out))
        return dict(zip(self.BINS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_sim_free(self._h)
            self._h = None


def modularity(graph, labels, symmetric=False):
    """Modularity of any labelling (labels in [0, n): a numpy array, a torch tensor on the device or a device address) ->
    (Q, S_in, S_sq, W); Q = S_in / W - S_sq / W^2 in double from the three integers the library returns (0.0 when W == 0)."""
    keep = None
    if isinstance(labels, np.ndarray):
        import torch
        keep = torch.from_numpy(_np_i32(labels)).cuda()
        torch.cuda.synchronize()
        labels = keep
    out = (C.c_uint64 * 3)()
    check(lib.mgx_modularity(graph._h, _dev_ptr(labels), int(bool(symmetric)), out))
    s_in, s_sq, w = int(out[0]), int(out[1]), int(out[2])
    q = 0.0 if w == 0 else float(s_in) / float(w) - float(s_sq) / (float(w) * float(w))
    return q, s_in, s_sq, w


class BcProblem:
    """Betweenness centrality: bc_problem_t + bc_enactor_t, and the fused path beside them.  centrality() is the sum
    over the last run's sources; sigma(), delta() and labels() describe its LAST source; original ids."""

    KEYS = ("sources", "levels", "reached", "inexact", "overflow", "host_waits", "traversal_waits", "launches", "chain_launches",
            "used_csc")
    INFO = ("in_lane", "in_wave", "in_huge", "out_lane", "out_wave", "out_huge", "in_segments", "out_segments", "lane_max", "huge_min",
            "seg", "chain", "levels", "chain_launches", "longest_in", "longest_out")

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_bc_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h
        self._all = False

    def _go(self, fn, sources, symmetric):
        st = (C.c_int64 * 10)()
        if sources is None:
            check(fn(self._h, None, 0, int(bool(symmetric)), st))
        else:
            src = np.ascontiguousarray(sources, dtype=np.int32)
            check(fn(self._h, _ptr(src), len(src), int(bool(symmetric)), st))
        self._all = sources is None
        return dict(zip(self.KEYS, (int(x) for x in st)))

    def run(self, sources=None, symmetric=False):
        """fused path -> the stats dict.  sources=None: every vertex.  symmetric=True is the caller's word that every entry has its
        reverse; False needs the graph's genuine CSC (Graph.build_csc)."""
        return self._go(lib.mgx_bc_run, sources, symmetric)

    def enact(self, sources=None, symmetric=False):
        """operator path (advance + filter per level, atomic adds); the same stats"""
        return self._go(lib.mgx_bc_enact, sources, symmetric)

    def _f64(self, fn):
        out = np.empty(self.graph.num_nodes, dtype=np.float64)
        check(fn(self._h, _ptr(out)))
        return out

    def centrality(self, normalized=False, undirected=False):
        """bc[v] of the last run (float64).  normalized / undirected: networkx's two scalings for a run over all sources -- 1 / ((n - 1)
        (n - 2)) and the halving of a graph whose every edge is stored in both directions."""
        out = self._f64(lib.mgx_bc_centrality)
        if normalized or undirected:
            if not self._all:
                raise ValueError("BcProblem.centrality: the scalings are defined for a run over all sources")
            n = self.graph.num_nodes
            if undirected:
                out *= 0.5
            if normalized:
                out *= (2.0 if undirected else 1.0) / ((n - 1) * (n - 2)) if n > 2 else 0.0
        return out

    def sigma(self):
        """shortest entry-paths from the last source (float64, 0 where unreached)"""
        return self._f64(lib.mgx_bc_sigma)

    def delta(self):
        """the last source's dependencies (float64)"""
        return self._f64(lib.mgx_bc_delta)

    def labels(self):
        """BFS depths from the last source (int32, -1 where unreached)"""
        out = np.empty(self.graph.num_nodes, dtype=np.int32)
        check(lib.mgx_bc_labels(self._h, _ptr(out)))
        return out

    def info(self):
        """row classes, segments, switches as read, levels and chain launches of the last source"""
        out = (C.c_int64 * 16)()
        check(lib.mgx_bc_info(self._h, out))
        return dict(zip(self.INFO, (int(x) for x in out)))

    def set_timing(self, on=True):
        """HIP events around the phases of the next fused runs (measurement only)"""
        check(lib.mgx_bc_set_timing(self._h, int(bool(on))))

    def phase_ms(self):
        """ms per source of the last timed fused run: traversal, list build, forward, backward; and the sources timed"""
        out = (C.c_double * 5)()
        check(lib.mgx_bc_phase_ms(self._h, out))
        return {"traversal": out[0], "lists": out[1], "forward": out[2], "backward": out[3], "sources_timed": int(out[4])}

    def centrality_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_bc_centrality_device(self._h, C.byref(p)))
        return p.value

    def close(self):
        if self._h:
            lib.mgx_bc_free(self._h)
            self._h = None


class PageRankProblem:
    """PageRank to convergence: pagerank_problem_t + pagerank_enactor_t, and the fused path beside them.  Not PrProblem,
    which is the reference's loop.  ranks() / residuals() describe the last run of either path."""

    def __init__(self, graph):
        h = C.c_void_p()
        check(lib.mgx_pagerank_create(graph._h, C.byref(h)))
        self.graph, self._h = graph, h

    def _go(self, fn, alpha, tol, max_iter, symmetric):
        st, res = (C.c_int64 * 6)(), C.c_double()
        check(fn(self._h, C.c_double(alpha), C.c_double(tol), int(max_iter), int(bool(symmetric)), st, C.byref(res)))
        return {"iterations": st[0], "converged": st[1], "dangling": st[2], "layout_path": st[3], "host_waits": st[4],
                "launches": st[5], "residual": res.value}

    def run(self, alpha=0.85, tol=1e-6, max_iter=100, symmetric=False):
        """fused path -> {"iterations", "converged", "dangling", "layout_path", "host_waits", "launches", "residual"}.
        symmetric=True is the caller's word that every entry has its reverse; False needs the graph's genuine CSC (build_csc)."""
        return self._go(lib.mgx_pagerank_run, alpha, tol, max_iter, symmetric)

    def enact(self, alpha=0.85, tol=1e-6, max_iter=100, symmetric=False):
        """operator path (neighbourhood-reduce, update, two host waits per iteration); the same stats, layout_path = 0"""
        return self._go(lib.mgx_pagerank_enact, alpha, tol, max_iter, symmetric)

    def ranks(self):
        out = np.empty(self.graph.num_nodes, dtype=np.float32)
        check(lib.mgx_pagerank_ranks(self._h, _ptr(out)))
        return out

    def ranks_device_ptr(self):
        p = C.c_void_p()
        check(lib.mgx_pagerank_ranks_device(self._h, C.byref(p)))
        return p.value

    def residuals(self, cap=65536):
        """e_1 .. e_T of the last run (at most 65 536 are kept)"""
        out, it = np.empty(max(int(cap), 1), dtype=np.float64), C.c_int()
        check(lib.mgx_pagerank_residuals(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), int(cap), C.byref(it)))
        return out[:min(int(cap), it.value)].copy()

    def bins(self):
        """which class of the general reduce took the in-rows of the last run() (huge_rows is 0 after a layout run), and the constants
        that draw the classes"""
        out = (C.c_int64 * 4)()
        check(lib.mgx_pagerank_bins(self._h, out))
        return dict(zip(("huge_rows", "lane_max", "huge_min", "huge_blocks"), (int(x) for x in out)))

    def close(self):
        if self._h:
            lib.mgx_pagerank_free(self._h)
            self._h = None


# building blocks ------------------------------------------------------------------------------
def scan_exclusive_i32(ctx, d_in, n, d_out):
    v = _i64()
    check(lib.mgx_scan_exclusive_i32(ctx._h, _dev_ptr(d_in), int(n), _dev_ptr(d_out), C.byref(v)))
    return v.value


def segmented_sort(ctx, keys, segments, values=None, descending=False):
    """mgpu::segmented_sort on int32 device tensors, in place on the context's stream: stable within the segments whose heads
    `segments` lists (ascending; what lies before the first head is a segment too).  Returns (keys, values)."""
    check(lib.mgx_segmented_sort_i32(ctx._h, _dev_ptr(keys), _dev_ptr(values), int(keys.numel()), _dev_ptr(segments),
                                     int(segments.numel()), int(bool(descending))))
    return keys, values


def scan_frontier_degrees(graph, frontier, use_csc=False):
    v = _i64()
    check(lib.mgx_scan_frontier_degrees(graph._h, frontier._h, int(use_csc), C.byref(v)))
    return v.value


def lbs_expand_debug(graph, frontier, total):
    seg = np.empty(max(total, 1), dtype=np.int32)
    rank = np.empty(max(total, 1), dtype=np.int32)
    check(lib.mgx_lbs_expand_debug(graph._h, frontier._h, int(total), _ptr(seg), _ptr(rank)))
    return seg[:total], rank[:total]


def compact_i32(ctx, d_in, n, drop_value, d_out):
    v = _i64()
    check(lib.mgx_compact_i32(ctx._h, _dev_ptr(d_in), int(n), int(drop_value), _dev_ptr(d_out), C.byref(v)))
    return v.value


def segreduce(graph, frontier, d_vertex_value, identity, d_reduced, op="f32_plus", push=True):
    v = _i64()
    if op == "f32_plus":
        check(lib.mgx_segreduce_f32_plus(graph._h, frontier._h, int(push), _dev_ptr(d_vertex_value),
                                         C.c_float(identity), _dev_ptr(d_reduced), C.byref(v)))
    elif op == "i32_min":
        check(lib.mgx_segreduce_i32_min(graph._h, frontier._h, int(push), _dev_ptr(d_vertex_value), int(identity),
                                        _dev_ptr(d_reduced), C.byref(v)))
    elif op == "i32_max":
        check(lib.mgx_segreduce_i32_max(graph._h, frontier._h, int(push), _dev_ptr(d_vertex_value), int(identity),
                                        _dev_ptr(d_reduced), C.byref(v)))
    else:
        raise ValueError(op)
    return v.value


def rmat_edges(ctx, scale, first_edge, count, seed, scramble, d_src, d_dst, d_weight=None):
    check(lib.mgx_rmat_edges(ctx._h, int(scale), int(first_edge), int(count), C.c_uint64(seed), int(bool(scramble)),
                             _dev_ptr(d_src), _dev_ptr(d_dst), _dev_ptr(d_weight)))
