"""numpy / scipy model of the triangle count (include/mgx/tc_fused.hpp): the definition the fused path and the
operator path must both reproduce bit for bit.

    graph:      the underlying simple undirected graph: a CSR entry (v, u), v != u, is the pair {v, u}; self-loops and duplicate
                entries change nothing
    tri[v]:     the triangles that contain v (int64); total = sum(tri) / 3
    sdeg[v]:    the distinct neighbours of v other than v (int32)
    rank:       symmetric: (row length, id), only the entries with rank(v) < rank(u) are kept;
                otherwise: (row length + entries that name v, id), every entry oriented from its lower-ranked end
    DAG:        dag_ro[n + 1], dag_ci[m_dag]: row a = the distinct neighbours of a of higher rank, ascending by id
    stats:      [0] triangles, [1] m_dag, [2] the longest oriented row, [3] oriented wedges sum d+(d+ - 1) / 2,
                [4] 1 if symmetric and every CSR row is ascending (the rows are used as they are), else 0

A triangle of ranks a < b < c is counted once.  With L the DAG's 0/1 matrix, ((L L^T) o L)[a, b] is the support of entry (a, b)
(the common elements of rows a and b: where the GPU paths count) and the column sums of ((L L) o L) are the third corners.  L L^T
costs the sum of the squared IN-degrees, though -- 10^10 on a star of 10^5 leaves, whose oriented rows all name the centre --, so
count() takes the same triangles at entry (b, c) instead: ((L^T L) o L)[b, c] = the a with a -> b and a -> c, which costs the
oriented wedges; its row sums are the middle corners, its column sums the third corners, the row sums of ((L L) o L) the first.
supports() is the (L L^T) form, for the inputs that can afford it (tests/test_tc_cpu.py holds the two against each other).
A A of the unoriented graph is never formed.
"""
import numpy as np

STAT_KEYS = ("triangles", "edges", "max_row", "wedges", "rows_sorted")


def _rank_less(deg, v, u):
    return (deg[v] < deg[u]) | ((deg[v] == deg[u]) & (v < u))


def dag(row_offsets, col_indices, symmetric):
    """-> (dag_ro int32[n + 1], dag_ci int32[m_dag], rows_sorted)"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    n = len(ro) - 1
    length = np.diff(ro)
    rows = np.repeat(np.arange(n, dtype=np.int64), length)
    if symmetric:
        keep = (rows != ci) & _rank_less(length, rows, ci)
        a, b = rows[keep], ci[keep]
    else:
        deg = length + np.bincount(ci, minlength=n)
        fwd = _rank_less(deg, rows, ci)
        ne = rows != ci
        a, b = np.where(fwd, rows, ci)[ne], np.where(fwd, ci, rows)[ne]
    key = np.unique(a * n + b)
    a, b = key // max(n, 1), key % max(n, 1)
    dag_ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=dag_ro[1:])
    ascending = True
    if len(ci) > 1:
        inner = np.ones(len(ci), dtype=bool)
        inner[ro[:-1][length > 0]] = False                     # the first entry of a row has no entry before it
        ascending = not bool(((ci[1:] < ci[:-1]) & inner[1:]).any())
    return dag_ro.astype(np.int32), b.astype(np.int32), int(bool(symmetric) and ascending)


def count(row_offsets, col_indices, symmetric):
    """-> {"tri": int64[n], "sdeg": int32[n], "dag_ro", "dag_ci", "stats": {STAT_KEYS}}"""
    import scipy.sparse as sp
    dag_ro, dag_ci, rows_sorted = dag(row_offsets, col_indices, symmetric)
    n = len(dag_ro) - 1
    L = sp.csr_matrix((np.ones(len(dag_ci), dtype=np.int64), dag_ci.astype(np.int64), dag_ro.astype(np.int64)), shape=(n, n))
    closing = (L.T @ L).multiply(L).tocsr()                     # [b, c]: the a with a -> b and a -> c, at the entries only
    third = (L @ L).multiply(L).tocsr()                         # [a, c]: the b with a -> b -> c, at the entries only
    tri = (np.asarray(third.sum(axis=1)).ravel() + np.asarray(closing.sum(axis=1)).ravel()
           + np.asarray(closing.sum(axis=0)).ravel()).astype(np.int64)
    d = np.diff(dag_ro.astype(np.int64))
    sdeg = (d + np.bincount(dag_ci, minlength=n)).astype(np.int32)
    stats = {"triangles": int(closing.sum()), "edges": int(len(dag_ci)), "max_row": int(d.max()) if n else 0,
             "wedges": int((d * (d - 1) // 2).sum()), "rows_sorted": rows_sorted}
    return {"tri": tri, "sdeg": sdeg, "dag_ro": dag_ro, "dag_ci": dag_ci, "stats": stats}


def supports(dag_ro, dag_ci):
    """((L L^T) o L) as a scipy CSR matrix: [a, b] = the common elements of rows a and b, at the DAG's entries only"""
    import scipy.sparse as sp
    n = len(dag_ro) - 1
    L = sp.csr_matrix((np.ones(len(dag_ci), dtype=np.int64), np.asarray(dag_ci, dtype=np.int64), np.asarray(dag_ro, dtype=np.int64)),
                      shape=(n, n))
    return (L @ L.T).multiply(L).tocsr()


def simple_graph(row_offsets, col_indices):
    """the underlying simple undirected graph as a networkx Graph (every vertex a node)"""
    import networkx as nx
    ro = np.asarray(row_offsets, dtype=np.int64)
    n = len(ro) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    g = nx.Graph()
    g.add_nodes_from(range(n))
    ci = np.asarray(col_indices, dtype=np.int64)
    ne = rows != ci
    g.add_edges_from(zip(rows[ne].tolist(), ci[ne].tolist()))
    return g
