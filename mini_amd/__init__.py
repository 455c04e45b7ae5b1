"""mini_amd -- MI355X-native frontier traversal engine (advance / filter / neighbourhood-reduce and
the BFS / SSSP / PR loops that drive them), behind mini-gunrock's operator API, plus k-core, graph colouring, local
sparsification and connected components (CcProblem: label[v] = the smallest vertex id of v's weakly connected component) and PageRank to convergence
(PageRankProblem; PrProblem is the reference's loop of that name) and triangle counting (TcProblem: per-vertex and total counts of the
underlying simple undirected graph, clustering coefficients) and betweenness centrality (BcProblem: Brandes per source on the fused BFS,
atomic-free pull sweeps, double precision) and k-truss decomposition (KtrussProblem: the trussness of every edge of the underlying simple
undirected graph, by peeling edges on their triangle supports) and strongly connected components (SccProblem: label[v] = the smallest
vertex id of v's strongly connected component, on the directed graph with its genuine CSC) and community detection by label
propagation (LpaProblem) with the modularity of any labelling (modularity) and bit-parallel multi-source BFS (MsBfsProblem: depths
from 64 sources per pass over the graph; closeness, harmonic centrality and eccentricity of the sources) and random walks (RandomWalkProblem: uniform, weighted and node2vec
walks with restarts, counter-based draws; paths, visit counts, Monte-Carlo personalised PageRank) and Louvain community detection
(LouvainProblem: levels of modularity-raising moves and graph contraction in integer arithmetic; labels, dendrogram, modularity) and
fan-out neighbour sampling for GNN mini-batches (NeighborSampleProblem: up to k_h out-neighbours per newly reached vertex and hop,
without replacement, one renumbered subgraph) and vertex similarity for link prediction (SimilarityProblem: the common neighbours of
arbitrary vertex pairs or of every edge, exactly; Jaccard, overlap, Sorensen, cosine, Adamic-Adar, resource allocation) and neighbour
feature aggregation for GNN layers (AggregateProblem: sum, mean, max or min of the neighbours' feature rows over out-rows, in-rows or
sampled blocks, optionally weighted, in a fixed order of arithmetic: bit-equal on every run) with its backward (AggregateGradProblem:
the gradient with respect to the features over the transposed rows, no atomics, bit-equal as well; mini_amd.autograd.aggregate is the
torch.autograd.Function on top of the two).

Layout: csrc/ (HIP sources of libmgx.so), _lib.py (ctypes binding of include/mgx.h),
api.py (host mirror of the reference's data model), autograd.py (the only module that imports torch), rmat.py (synthetic inputs,
device-side).
Importing the package loads libmgx.so and raises ImportError if it has not been built.
"""
from ._lib import (LIB_PATH, MGX_AGG_BLOCK, MGX_AGG_IN_ROWS, MGX_AGG_MAX, MGX_AGG_MEAN, MGX_AGG_MIN, MGX_AGG_OUT_ROWS, MGX_AGG_SUM,
                   MGX_BFS_DIRECTION_OPT, MGX_BFS_PUSH, MGX_E_FRONTIER_OVERFLOW, MGX_E_INVALID, MGX_LPA_LAZY, MGX_LPA_SYNC,
                   MGX_SIM_COMMON, MGX_SIM_COSINE, MGX_SIM_JACCARD, MGX_SIM_OVERLAP, MGX_SIM_SORENSEN, MGX_SIM_WEIGHTED,
                   MGX_E_NEGATIVE_WEIGHT, MgxError, lib)
from .api import (AggregateGradProblem, AggregateProblem, BcProblem, BfsProblem, CcProblem, ColorProblem, Context, Frontier, Graph, KcoreProblem, KtrussProblem, LouvainProblem, LpaProblem, LsparProblem, MsBfsProblem, MstProblem, NeighborSampleProblem, PageRankProblem, PrProblem, RandomWalkProblem, SccProblem, SimilarityProblem, SsspProblem, TcProblem, compact_i32,
                  lbs_expand_debug, load_csr_cache, load_mtx, rmat_edges, save_csr_cache, scan_exclusive_i32, scan_frontier_degrees,
                  modularity, segmented_sort, segreduce)

__all__ = [n for n in dir() if not n.startswith("_")]
