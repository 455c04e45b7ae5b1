/*
 * mgx.h -- C-ABI of the MI355X-native frontier traversal engine (libmgx.so).
 *
 * The reference (gunrock/mini) has no FFI: its boundary is a set of C++ function
 * templates parameterised by device functors.  Device functors cannot
 * cross a C ABI, so this header carries the operators PRE-INSTANTIATED for the
 * in-scope functors (BFS, SSSP, PR), the building blocks (scan, load-balanced
 * search, compaction, segmented reduce) and whole-algorithm runs.  The
 * source-compatible template API itself lives in include/gunrock/ (*.hxx).
 *
 * Conventions: every entry point returns an int status (MGX_OK == 0, negative ==
 * error), never calls exit() (the reference does: frontier.hxx:53-59,83-93,
 * graph.hxx:107-110), never throws across the boundary.  Handles are opaque.
 * Host buffers are caller-owned.  `stream` arguments are hipStream_t passed as
 * void* (NULL == legacy default stream, which is what the reference uses).
 * All ids/offsets are 32-bit like the reference (graph.hxx:19-26); counts that
 * can exceed 2^31 are int64_t.
 */
#ifndef MGX_H_
#define MGX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_API __attribute__((visibility("default")))

/* status codes */
#define MGX_OK 0
#define MGX_E_INVALID (-1)           /* bad argument                                         */
#define MGX_E_HIP (-2)               /* a HIP runtime call failed (see mgx_last_error)        */
#define MGX_E_FRONTIER_OVERFLOW (-4) /* frontier.hxx:53-59,83-93: the reference exit(0)s here */
#define MGX_E_NEGATIVE_WEIGHT (-5)   /* SSSP relaxes on the int view of non-negative floats   */
#define MGX_E_NO_DEVICE (-6)

typedef struct mgx_ctx_s* mgx_ctx_t;
typedef struct mgx_graph_s* mgx_graph_t;
typedef struct mgx_frontier_s* mgx_frontier_t;
typedef struct mgx_bfs_s* mgx_bfs_t;
typedef struct mgx_sssp_s* mgx_sssp_t;
typedef struct mgx_pr_s* mgx_pr_t;
typedef struct mgx_kcore_s* mgx_kcore_t;
typedef struct mgx_color_s* mgx_color_t;
typedef struct mgx_lspar_s* mgx_lspar_t;
typedef struct mgx_cc_s* mgx_cc_t;
typedef struct mgx_tc_s* mgx_tc_t;
typedef struct mgx_bc_s* mgx_bc_t;
typedef struct mgx_pagerank_s* mgx_pagerank_t;
typedef struct mgx_mst_s* mgx_mst_t;
typedef struct mgx_ktruss_s* mgx_ktruss_t;
typedef struct mgx_scc_s* mgx_scc_t;
typedef struct mgx_lpa_s* mgx_lpa_t;
typedef struct mgx_msbfs_s* mgx_msbfs_t;
typedef struct mgx_rw_s* mgx_rw_t;
typedef struct mgx_nsample_s* mgx_nsample_t;
typedef struct mgx_agg_s* mgx_agg_t;
typedef struct mgx_aggbwd_s* mgx_aggbwd_t;
typedef struct mgx_louvain_s* mgx_louvain_t;
typedef struct mgx_dbfs_s* mgx_dbfs_t;
typedef struct mgx_dbfs2_s* mgx_dbfs2_t;
typedef struct mgx_dsssp_s* mgx_dsssp_t;
typedef struct mgx_comm_s* mgx_comm_t;

MGX_API int mgx_version(void);
/* The environment switches the library reads (include/mgx/env.hpp: the one table, the one reader): returns how many there are; for
 * 0 <= index < that, *name / *what (either may be NULL) point at the switch's name and a line about it (static strings).  Every switch
 * selects between product paths the thresholds pick by size; none changes a result.  An empty value counts as unset. */
MGX_API int mgx_env_switches(int index, const char** name, const char** what);
MGX_API int mgx_build_is_lab(void); /* 1: built with -DMGX_LAB (experiment shapes and instrumented kernels compiled in: never the product) */
MGX_API const char* mgx_strerror(int status);
MGX_API const char* mgx_last_error(void); /* thread-local detail of the last failure */

/* ---- context: replaces mgpu::standard_context_t (tests/bfs/test_bfs.cu:22) ---- */
MGX_API int mgx_ctx_create(int device, void* stream, mgx_ctx_t* out);
MGX_API int mgx_ctx_set_stream(mgx_ctx_t ctx, void* stream);
MGX_API int mgx_ctx_synchronize(mgx_ctx_t ctx);
MGX_API int mgx_ctx_destroy(mgx_ctx_t ctx);
MGX_API int mgx_ctx_num_cus(mgx_ctx_t ctx, int* out);

/* ---- graph: replaces graph_device_t + graph_to_device (graph.hxx:37-83) ----
 * col_offsets/row_indices/row_weights == NULL mirrors the CSR into the "CSC" slots, which
 * is what the reference always ends up doing.  weights == NULL means all 1.0f
 * (graph.hxx:126).  upload copies from host; wrap_device borrows device pointers (e.g.
 * torch tensors) that must outlive the graph.                                           */
MGX_API int mgx_graph_upload(mgx_ctx_t ctx, int num_nodes, int64_t num_edges,
                             const int* row_offsets, const int* col_indices, const float* weights,
                             const int* col_offsets, const int* row_indices, const float* row_weights,
                             mgx_graph_t* out);
MGX_API int mgx_graph_wrap_device(mgx_ctx_t ctx, int num_nodes, int64_t num_edges,
                                  const int* d_row_offsets, const int* d_col_indices, const float* d_weights,
                                  const int* d_col_offsets, const int* d_row_indices, const float* d_row_weights,
                                  mgx_graph_t* out);
/* Optional hub-first layout used by mgx_bfs_run (not in the reference): the same graph with vertex
 * ids renumbered by DESCENDING DEGREE (layout id 0 = highest degree), as CSR, plus the two id maps
 * (new_of_old[old] = layout id, old_of_new = inverse).  With it the hot prefix of the visited
 * bitmap (the vertices that receive most edges) is kept in LDS.  Device pointers are borrowed.
 * Results (labels) are always in original ids; the operator entry points ignore the layout.   */
MGX_API int mgx_graph_attach_layout(mgx_graph_t g, const int* d_layout_row_offsets, const int* d_layout_col_indices,
                                    const int* d_new_of_old, const int* d_old_of_new);
/* weights of the layout's edges, in the layout's order (optional): mgx_sssp_run then relaxes in layout space, where
 * the distances of the high-degree vertices -- the targets of most relaxations -- sit together in L2 */
MGX_API int mgx_graph_attach_layout_weights(mgx_graph_t g, const float* d_layout_weights);
/* The same layout built by the library from the graph's own CSR (device-side degree sort, renumbering, rows sorted by
 * neighbour; one-time setup, rocPRIM sort / scan) and owned by the graph; with_weights != 0 carries the edge weights
 * along for the fused SSSP loop.  mgx_graph_layout_read copies the pieces to host buffers (NULL: skip; sizes n + 1,
 * m, n, n, m) -- what the tests compare with the torch construction in mini_amd/rmat.py. */
MGX_API int mgx_graph_build_layout(mgx_graph_t g, int with_weights);
/* What the layout holds: out8 = { 1 if the graph has one, unit blocks (64-entry units of the long rows), 1 if their 24-bit copy
 * exists, pairs of the cold-edge lists, slices that hold pairs, units of the blocks WITHOUT the lists' entries (the fused BFS reads
 * those when it runs the cold-edge pass), 1 if the long rows' entries were mostly cold (no lists: a flat graph), bytes of device
 * memory the library allocated for the layout and everything cut from it (arrays the caller attached are not counted) }. */
MGX_API int mgx_graph_layout_info(mgx_graph_t g, int64_t* out8);
/* The long rows regrouped by slice of their destinations for the full-frontier neighbour-reduce (mgx/nreduce.hpp: k_nrs_edges; replaces
 * the gather of value(u) per edge of the reference's neighborhood_kernel, neighborhood.hxx:39-58, by LDS reads): built by the library
 * at the graph's first full-frontier reduce (mgx_segreduce_*, mgx_pr_enact) on a graph with the library's layout.  out5 = { 16-byte
 * mini-units (0: not built), hot slices of 40 000 vertices, long rows, rows whose partials more than one lane folds, mini-units of the tail }. */
MGX_API int mgx_graph_nr_slices_info(mgx_graph_t g, int64_t* out5);
MGX_API int mgx_graph_layout_read(mgx_graph_t g, int* h_row_offsets, int* h_col_indices, int* h_new_of_old,
                                  int* h_old_of_new, float* h_weights);
/* Genuine CSC (the transpose) built by the library from the graph's own CSR, device-side (one stable radix sort of the
 * edges by destination), owned by the graph: col_offsets / row_indices (sources of every vertex's in-edges, ascending) /
 * row_values.  What bottom-up BFS levels need on DIRECTED inputs (BASELINE config 4); the reference's load_graph means to
 * build it (graph.hxx:176-222) but returns the CSR in the CSC slots.  mgx_graph_csc_read copies the CSC slots
 * to host buffers (NULL: skip; sizes n + 1, m, m) -- whatever they hold, alias or transpose. */
MGX_API int mgx_graph_build_csc(mgx_graph_t g);
MGX_API int mgx_graph_csc_read(mgx_graph_t g, int* h_col_offsets, int* h_row_indices, float* h_row_values);
MGX_API int mgx_graph_free(mgx_graph_t g);
MGX_API int mgx_graph_dims(mgx_graph_t g, int* num_nodes, int64_t* num_edges);
/* host-side MTX text loader, bug-compatible with load_graph (graph.hxx:96-223): row = 2nd
 * field, neighbour = 1st field, multi-edges and self loops kept, undir appends the swapped
 * copies.  Returns malloc'd arrays to be released with mgx_host_free.                    */
MGX_API int mgx_load_mtx(const char* path, int undir, int random_edge_value,
                         int* num_nodes, int64_t* num_edges,
                         int** row_offsets, int** col_indices, float** weights);
/* The same plus the loader's CSC slots: the CSR again (what the reference always returns) or, with
 * genuine_csc != 0 and undir == 0, the transpose (load_graph's _genuine_csc option: what graph.hxx:176-222 means to
 * build).  Six malloc'd arrays to be released with mgx_host_free.                                  */
MGX_API int mgx_load_mtx_csc(const char* path, int undir, int random_edge_value, int genuine_csc,
                             int* num_nodes, int64_t* num_edges, int** row_offsets, int** col_indices, float** weights,
                             int** col_offsets, int** row_indices, float** row_weights);
/* Binary CSR cache: the loader's output as raw arrays behind a header with a checksum, so that a big
 * MatrixMarket file is parsed and sorted once (mgx_load_mtx / mgx_load_mtx_csc, then mgx_graph_save_csr) and mapped
 * back without parsing afterwards (mgx_graph_load_csr).  col_offsets / row_indices / row_weights: a genuine CSC to store
 * with it, or all NULL.  load: a file that is missing, truncated, of another format or fails its checksum or the
 * structural checks (monotone offsets, ids in range) is MGX_E_INVALID -- a cache is never trusted; the CSC outputs are
 * NULL when the file holds none.  Arrays are malloc'd: release with mgx_host_free. */
MGX_API int mgx_graph_save_csr(const char* path, int num_nodes, int64_t num_edges, int undirected, const int* row_offsets,
                               const int* col_indices, const float* weights, const int* col_offsets, const int* row_indices,
                               const float* row_weights);
MGX_API int mgx_graph_load_csr(const char* path, int* num_nodes, int64_t* num_edges, int* undirected, int** row_offsets,
                               int** col_indices, float** weights, int** col_offsets, int** row_indices, float** row_weights);
MGX_API void mgx_host_free(void* p);

/* ---- frontier: replaces frontier_t<int> (frontier.hxx:12-99) ---- */
MGX_API int mgx_frontier_create(mgx_ctx_t ctx, int64_t capacity, mgx_frontier_t* out);
MGX_API int mgx_frontier_free(mgx_frontier_t f);
MGX_API int mgx_frontier_load(mgx_frontier_t f, const int* host, int64_t n);   /* load(vector)  :65-79 */
MGX_API int mgx_frontier_fill_iota(mgx_frontier_t f, int64_t n);              /* enactor.hxx:29-34   */
MGX_API int mgx_frontier_fill(mgx_frontier_t f, int value, int64_t n);        /* fill + load(mem_t)  */
MGX_API int mgx_frontier_read(mgx_frontier_t f, int* host, int64_t cap, int64_t* n);
MGX_API int mgx_frontier_resize(mgx_frontier_t f, int64_t n);                 /* resize :82-93       */
MGX_API int mgx_frontier_size(mgx_frontier_t f, int64_t* n);
MGX_API int mgx_frontier_capacity(mgx_frontier_t f, int64_t* n);
MGX_API int mgx_frontier_device_ptr(mgx_frontier_t f, int** d_ptr);

/* ---- building blocks (moderngpu call sites: advance.hxx:40,62; filter.hxx:18-29;
 *      neighborhood.hxx:35,58).  Device pointers in, counts out.                       */
/* out[i] = sum_{j<i} in[j]; *total = sum of all (transform_scan<int>, plus_t)          */
MGX_API int mgx_scan_exclusive_i32(mgx_ctx_t ctx, const int* d_in, int64_t n, int* d_out, int64_t* total);
/* degree scan of a frontier over the graph's row offsets (push) or col offsets (pull):
 * d_scanned_row_offsets[i] = sum_{j<i} deg(in[j])   (advance.hxx:32-43)                 */
MGX_API int mgx_scan_frontier_degrees(mgx_graph_t g, mgx_frontier_t in, int use_csc, int64_t* total);
/* transform_lbs made visible: (seg, rank) of every work item of the last degree scan  */
MGX_API int mgx_lbs_expand_debug(mgx_graph_t g, mgx_frontier_t in, int64_t total,
                                 int* host_seg, int* host_rank);
/* stable compaction of d_in by (d_in[i] != drop_value) -- transform_compact            */
MGX_API int mgx_compact_i32(mgx_ctx_t ctx, const int* d_in, int64_t n, int drop_value, int* d_out, int64_t* kept);
/* neighborhood_kernel (neighborhood.hxx:12-70) with get_value_to_reduce = d_vertex_value[nbr]:
 * d_reduced[seg] = op over the segment's neighbours, identity for empty segments.
 * The identity contract: a segment WITH neighbours receives the pure fold of their values -- `identity` is never mixed in,
 * it need not be the operator's neutral element (a sentinel such as -1.0 for "no neighbours" under f32_plus is fine) --
 * and a segment without neighbours receives `identity` itself.  The answer does not depend on which kernels ran.
 * push != 0 walks the CSR, 0 the CSC slots.                                             */
MGX_API int mgx_segreduce_f32_plus(mgx_graph_t g, mgx_frontier_t in, int push,
                                   const float* d_vertex_value, float identity, float* d_reduced, int64_t* nonzeros);
MGX_API int mgx_segreduce_i32_min(mgx_graph_t g, mgx_frontier_t in, int push,
                                  const int* d_vertex_value, int identity, int* d_reduced, int64_t* nonzeros);
MGX_API int mgx_segreduce_i32_max(mgx_graph_t g, mgx_frontier_t in, int push,
                                  const int* d_vertex_value, int identity, int* d_reduced, int64_t* nonzeros);
/* What the last neighbourhood reduce on the graph's context did (mgx_segreduce_*, and the operator calls of mgx_pr_enact,
 * the colouring and lspar enactors); MGX_E_INVALID before any such call.
 *   out4[0]  body: 0 the general LBS kernel, 1 the layout with its unit blocks, 2 the layout with the sliced long rows
 *   out4[1]  the frontier as the host classified it: 0 other, 1 full (n ids), 2 subset (n / 8 <= ids < n)
 *   out4[2]  1 if the layout's kernels were entered but the device's verdict on the frontier (not 0 .. n - 1, not strictly
 *            ascending) sent the call to the general kernel; out4[0] is then 0
 *   out4[3]  edges returned                                                              */
MGX_API int mgx_graph_nr_last_call(mgx_graph_t g, int64_t* out4);

/* ---- BFS: bfs_problem_t / bfs_functor_t / bfs_enactor_t (gunrock/src/bfs/) ---- */
MGX_API int mgx_bfs_create(mgx_graph_t g, int src, mgx_bfs_t* out);       /* bfs_problem.hxx:34-46 */
MGX_API int mgx_bfs_reset(mgx_bfs_t p, int src);
MGX_API int mgx_bfs_free(mgx_bfs_t p);
MGX_API int mgx_bfs_labels(mgx_bfs_t p, int* host_labels);                /* extract() :48-50      */
MGX_API int mgx_bfs_preds(mgx_bfs_t p, int* host_preds);                  /* stay -1   */
MGX_API int mgx_bfs_labels_device(mgx_bfs_t p, int** d_labels);
/* advance_forward_kernel<bfs_problem_t,bfs_functor_t,false,true>  (bfs_enactor.hxx:52-57) */
MGX_API int mgx_bfs_advance(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front);
/* filter_kernel<bfs_problem_t,bfs_functor_t>                      (bfs_enactor.hxx:60-65) */
MGX_API int mgx_bfs_filter(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept);
/* the two above in one pass over the edges: out = ids whose label this call set          */
MGX_API int mgx_bfs_advance_filter_fused(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept);
/* The reference's IDEMPOTENT mode (no upstream enactor uses it):
 * advance_forward_kernel<bfs_problem_t, F, idempotence = true, true> (advance.hxx:60): out = EVERY neighbour of the
 * frontier, duplicates and visited vertices included, no atomics on labels; front = edges expanded.
 * uniquify_kernel<bfs_problem_t, F> (filter.hxx:95-119): out = the vertices of `in` not seen before in this traversal,
 * one copy each, stable (wave64 intra-wave cull, then an exact visited-bitmask cull: the mask, (n + 31) / 32 words,
 * belongs to the problem handle and is reset by mgx_bfs_reset with the source's bit set), labelled iteration + 1 by
 * F::cond_uniq.  F = bfs_idempotent_functor_t (include/gunrock/bfs/bfs_functor.hxx).
 * mgx_bfs_enact_idempotent: the superstep loop over the two from the problem's source (labels as mgx_bfs_reset left
 * them); stats[0] = iterations, [1] = edges expanded.  Labels equal enact_pushpull's. */
MGX_API int mgx_bfs_advance_idempotent(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front);
MGX_API int mgx_bfs_uniquify(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept);
MGX_API int mgx_bfs_enact_idempotent(mgx_bfs_t p, int64_t* stats);
/* gen_unvisited_kernel / sparse_to_dense_kernel / advance_backward_kernel (advance.hxx:69-160) */
MGX_API int mgx_bfs_gen_unvisited(mgx_bfs_t p, mgx_frontier_t indices, mgx_frontier_t unvisited, int iteration, int64_t* kept);
MGX_API int mgx_bfs_sparse_to_dense(mgx_bfs_t p, mgx_frontier_t sparse, mgx_frontier_t dense, int iteration);
MGX_API int mgx_bfs_advance_backward(mgx_bfs_t p, mgx_frontier_t unvisited, mgx_frontier_t bitmap,
                                     mgx_frontier_t bitmap_out, int iteration, int64_t* front);
/* bfs_enactor_t::enact_pushpull (bfs_enactor.hxx:41-117) on the operator-per-superstep path.
 * stats[0]=pushed iterations, [1]=total iterations, [2]=edges expanded by push,
 * [3]=in-edges inspected by pull.                                                        */
MGX_API int mgx_bfs_enact_pushpull(mgx_bfs_t p, float threshold, int64_t* stats);

/* Whole traversal on the fused device-resident path (no per-level host round trip):
 * labels identical to enact_pushpull's.  mode: MGX_BFS_PUSH (config 2) or
 * MGX_BFS_DIRECTION_OPT (config 4; needs a genuine CSC for directed graphs).
 * A traversal is enqueued as batches of launch slots (mgx/bfs_fused_run.hpp); the host waits once per batch
 * (first batch: as many slots as the previous traversal of the graph needed, then MGX_BFS_LEVELS_PER_SYNC).
 * stats (may be NULL):
 *   [0] levels run  [1] vertices reached (incl. source)  [2] m_t = sum of out-degrees of
 *   reached vertices (the TEPS numerator)  [3] edges inspected by push levels
 *   [4] edges inspected by pull levels [5] push levels [6] level-kernel launches (incl. the
 *   empty ones behind the last level) [7] device time of those launches in ns (HIP events on
 *   the context's stream) [8] frontier vertices expanded (sum of per-level frontier sizes)
 *   [9] visited-bit claims (atomicOr) issued.
 *   Timed push kernel (only with mgx_bfs_set_kernel_timing; mode 2: the merged k_bfs_push launch, mode 1: the part
 *   with more device time in this run):
 *   [10] its launches (incl. the ones that find nothing to do) [11] their device time in ns (HIP events
 *   around every launch) [12] edges and [13] frontier vertices it processed
 *   [14] which one (1 = long-row part or the merged launch, 0 = short-row part)
 *   [15] levels run inside a push launch's block 0 (chains of small levels, bfs_fused_chain.hpp)
 *   [16] launch slots used [17] slots whose long rows were read from the unit blocks (bfs_fused_dense.hpp)
 *   [18] slots whose short rows were walked vertex by vertex (bfs_fused_vshort.hpp)
 *   [19] slots that ran without queues (the build before them wrote none, bfs_build_is_lazy)
 *   [20] slots that ran the cold-edge pass (bfs_fused_cold.hpp) [21] mid-size levels expanded by M launches (bfs_fused_mini.hpp)
 *   [22] 1 + the last slot whose queue build stored level bytes (mgx/bfs_fused.hpp: lvl8; 0: none did).
 *   mgx_bfs_run writes entries [0] .. [15] (stats must hold 16: the contract of the first release, kept so that a
 *   caller built against it is not overrun); mgx_bfs_run_stats is the same call with an explicit capacity and writes
 *   min(cap, 24) entries.                                                                       */
#define MGX_BFS_PUSH 0
#define MGX_BFS_DIRECTION_OPT 1
MGX_API int mgx_bfs_run(mgx_bfs_t p, int src, int mode, float alpha, int64_t* stats);
MGX_API int mgx_bfs_run_stats(mgx_bfs_t p, int src, int mode, float alpha, int64_t* stats, int cap);
/* A batch of sources: `count` complete traversals (each as mgx_bfs_run: labels re-initialised, every level run, counters
 * taken) enqueued back to back on the context's stream with ONE host wait at the end -- the reference's one-call-per-
 * source driver (test_bfs.cu:32-42) pays a host round trip per traversal, ~18 us of a 0.35 ms RMAT-22 traversal here.
 * stats: count x cap entries, row i = the counters of sources[i] (the layout of mgx_bfs_run_stats; timing entries are 0);
 * the labels (mgx_bfs_labels) are those of the LAST source.  *reruns (optional): traversals that did not finish inside the
 * batch and were run again on their own (a source whose level structure needed more launch slots than its predecessors). */
MGX_API int mgx_bfs_run_many(mgx_bfs_t p, const int* sources, int count, int mode, float alpha, int64_t* stats, int cap, int* reruns);
/* per-level trace of the last mgx_bfs_run: level_nf[i], level_edges[i] for i < *levels  */
MGX_API int mgx_bfs_level_trace(mgx_bfs_t p, int cap, int64_t* level_nf, int64_t* level_edges, int* levels);

/* device time (ms, HIP events) of each launch batch of the last mgx_bfs_run; with the environment
 * variable MGX_BFS_LEVELS_PER_SYNC=1 a batch is exactly one level kernel                   */
/* Per-launch timing of the push kernels is OFF by default: every hipEventRecord between two kernels leaves a
 * ~6 us gap on the stream (measured, rocprofv3 kernel trace).  on == 1: following mgx_bfs_run calls launch the parts of
 * a slot's push (long rows, short rows) separately with events around each and fill mgx_bfs_kernel_times /
 * mgx_bfs_level_kernel_times; on == 2: events around the ONE merged push launch of every slot (k_bfs_push, the kernel a
 * traversal actually runs): its launches and time are reported in the "stream" half of mgx_bfs_kernel_times with ALL
 * push edges and frontier vertices; the "wave" half then holds the launches and time of the slots' queue builds
 * (k_bfs_build2 -- the filter half of advance + filter), edges and vertices zero. */
MGX_API int mgx_bfs_set_kernel_timing(mgx_bfs_t p, int on);
/* the two push kernels of the last mgx_bfs_run, timed per launch with HIP events on the context's stream:
 * out8 = { stream launches, ns, edges, frontier vertices,  wave launches, ns, edges, frontier vertices }
 * ("stream": the long-row part of k_bfs_push -- rows of >= MGX_BFS_LONG_MIN edges, unit blocks or queue walk, with the
 *  cold-edge pass -- or, in timing mode 2, the whole merged launch; "wave": the short-row part)               */
MGX_API int mgx_bfs_kernel_times(mgx_bfs_t p, int64_t* out8);
/* duration of each level of the last run (ms), from device-side timestamps taken when a level is opened: no host
 * synchronisation involved; first min(cap, 63) levels */
MGX_API int mgx_bfs_level_times(mgx_bfs_t p, int cap, float* ms, int* levels);
/* the same per launch slot (ms), first min(cap, 64) slots of the last run; a slot = one k_bfs_push launch
 * and its queue build (include/mgx/bfs_fused_run.hpp) */
MGX_API int mgx_bfs_level_kernel_times(mgx_bfs_t p, int cap, float* stream_ms, float* wave_ms);
/* atomicOr claims issued per level of the last run (first 64 levels) */
MGX_API int mgx_bfs_level_claims(mgx_bfs_t p, int cap, int64_t* claims);
MGX_API int mgx_bfs_batch_times(mgx_bfs_t p, int cap, float* ms, int* batches);

/* ---- vertex-range partitioned BFS: the per-rank pieces (the reference has no
 *      multi-GPU path, README.md:4).  Rank r of `ranks` owns global ids [r*chunk, (r+1)*chunk),
 *      chunk = ceil(n_global/ranks): their CSR rows (local row_offsets, GLOBAL col_indices) and
 *      labels.  Per superstep the host calls expand (-> per-owner bins of neighbour ids, each id at
 *      most once per traversal per rank), exchanges bin r of every rank to rank r (all-to-all over
 *      RCCL/xGMI), calls receive for what arrived (and for its own bin) and swap.  Labels equal the
 *      single-GPU depths bit for bit.  Device pointers are borrowed.                          */
/* d_bins: optional caller-owned send buffer of ranks*bin_capacity ints (bin_capacity >= chunk), so the
 * host can hand slices of it straight to its collective; NULL = library-owned.                  */
MGX_API int mgx_dbfs_create(mgx_ctx_t ctx, int n_global, int ranks, int rank, int64_t m_local,
                            const int* d_row_offsets_local, const int* d_col_indices_global,
                            int* d_bins, int64_t bin_capacity, mgx_dbfs_t* out);
MGX_API int mgx_dbfs_free(mgx_dbfs_t h);
MGX_API int mgx_dbfs_range(mgx_dbfs_t h, int* v_lo, int* v_hi);
MGX_API int mgx_dbfs_reset(mgx_dbfs_t h, int src_global);
MGX_API int mgx_dbfs_expand(mgx_dbfs_t h, int64_t* host_counts_per_rank, int64_t* edges_expanded);
MGX_API int mgx_dbfs_bins(mgx_dbfs_t h, int** d_bins, int64_t* bin_capacity); /* bin r at d_bins + r*capacity */
MGX_API int mgx_dbfs_receive(mgx_dbfs_t h, const int* d_global_ids, int64_t count, int label);
MGX_API int mgx_dbfs_swap(mgx_dbfs_t h, int64_t* next_frontier_size);
MGX_API int mgx_dbfs_labels(mgx_dbfs_t h, int* host_labels_local);

/* ---- vertex-range partitioned SSSP: the per-rank pieces ("(dst, dist) pairs with min-combining"; the
 *      reference has no multi-GPU path).  Same partition as mgx_dbfs_*: rank r owns [r*chunk, (r+1)*chunk), their rows
 *      (local row_offsets, GLOBAL col_indices, weights) and distances.  A superstep is frontier Bellman-Ford
 *      (sssp_enactor.hxx:40-72): expand relaxes the local frontier's edges -- local targets at once, remote ones into
 *      per-owner bins of 8-byte pairs (vertex << 32 | float bits), ONE pair per target vertex and superstep carrying the
 *      minimum over all of this rank's edges to it (min-combining before send) and only if it beats everything this
 *      rank sent for that vertex before; the host exchanges bin r of every rank to rank r (all-to-all-v); receive keeps
 *      the minimum and queues the vertices whose distance dropped; swap returns the next local frontier size (the host
 *      all-reduces it: zero everywhere ends the run).  Distances equal the single-GPU ones bit for bit; unreachable
 *      vertices hold FLT_MAX.  Device pointers are borrowed. */
MGX_API int mgx_dsssp_create(mgx_ctx_t ctx, int n_global, int ranks, int rank, int64_t m_local, const int* d_row_offsets_local,
                             const int* d_col_indices_global, const float* d_weights, mgx_dsssp_t* out);
MGX_API int mgx_dsssp_free(mgx_dsssp_t h);
MGX_API int mgx_dsssp_reset(mgx_dsssp_t h, int src_global);
MGX_API int mgx_dsssp_expand(mgx_dsssp_t h, int64_t* host_counts_per_rank, int64_t* edges_relaxed);
MGX_API int mgx_dsssp_bins(mgx_dsssp_t h, uint64_t** d_bins, int64_t* bin_capacity); /* bin r at d_bins + r*capacity */
MGX_API int mgx_dsssp_receive(mgx_dsssp_t h, const uint64_t* d_pairs, int64_t count);
MGX_API int mgx_dsssp_swap(mgx_dsssp_t h, int64_t* next_frontier_size);
MGX_API int mgx_dsssp_distances(mgx_dsssp_t h, float* host_dist_local);
/* The whole superstep loop from `src_global` with the library's communicator (mgx_comm_create; NULL for one rank): expand,
 * bin counts by all-gather, the all-to-all-v of the pairs as one group of sends and receives, receive, swap, global
 * frontier size -- until it is zero.  out4: supersteps, edges relaxed here, pairs sent from here, pairs received here.
 * Every rank of the communicator must make the call.  No reference counterpart (README.md:4); SURVEY 8e. */
MGX_API int mgx_dsssp_run(mgx_dsssp_t h, mgx_comm_t comm, int src_global, int64_t* out4);

/* ---- partitioned BFS, generation 2 (include/mgx/bfs_dist2.hpp): every rank runs the FUSED level
 *      kernels on its rows and ranks exchange dense "newly visited" bitmaps (one all-gather of n/8 bytes
 *      per rank and level) instead of id lists.  Ids are global and hub-first (descending global degree);
 *      vertex v belongs to rank v % ranks, local row v / ranks.  d_newbits: caller-owned buffer of
 *      mgx_dbfs2_words(n_global) words that mgx_dbfs2_push fills with the rank's discoveries of the level;
 *      mgx_dbfs2_merge takes the all-gathered ranks x words array, ORs it into every rank's visited
 *      bitmap, labels the owned vertices and builds the rank's next frontier (returns its size/edges). */
MGX_API int mgx_dbfs2_create(mgx_ctx_t ctx, int n_global, int ranks, int rank, const int* d_row_offsets_local,
                             const int* d_col_indices_global, unsigned* d_newbits, mgx_dbfs2_t* out);
/* Unit blocks of the rank's long rows (64-entry units, one owner each, as mgx_graph_build_layout makes them for the
 * single-GPU path): levels that hold a large share of the rank's long rows are then read from them, 16 bytes per lane,
 * with the level's merged discoveries as the frontier bitmap, instead of walking the long-row queue.  On a graph that
 * outgrows the LDS prefix of the visited bitmap (652 288 vertices) the call also builds the rows' cold-edge lists -- the
 * entries behind the prefix as (owner, destination) pairs by slice of the destination: workgroups of the push launch take
 * them with THEIR slice of the bitmap in LDS and leave a bitmap, no byte marks (needs rows sorted by neighbour id, as the
 * library's shard builder makes them).  Once per engine, optional; *units (may be NULL) <- units built (0: the rows are
 * all short).  Needs row_offsets / col_indices to stay valid and unchanged.  No reference counterpart.
 * Round 4: with cold-edge lists the unit blocks hold the rows' entries INSIDE the prefix only, three bytes each, and the pairs
 * are kept a second time at four bytes each; when the rank's rows come by non-increasing degree (the shard builder's order) the
 * call also prepares the vertex-by-vertex walk of its short rows -- a copy of col_indices with readable entries behind it
 * (m_local + 8 ints of device memory) and a bitmap of the rank's local frontier.  mgx_dbfs2_path_levels says what a traversal used. */
MGX_API int mgx_dbfs2_build_units(mgx_dbfs2_t h, int64_t* units);
/* levels of the traversal whose long rows were read from the unit blocks, as of the last mgx_dbfs2_status / mgx_dbfs2_run */
MGX_API int mgx_dbfs2_dense_levels(mgx_dbfs2_t h, int64_t* levels);
/* ... and how many of them ran the cold-edge pass (the long rows' entries behind the LDS prefix as (owner, destination) pairs by
 * slice of the destination, built with the unit blocks when the graph is big enough to have any: *pairs, may be NULL) */
MGX_API int mgx_dbfs2_cold_levels(mgx_dbfs2_t h, int64_t* levels, int64_t* pairs);
/* which of round 4's paths the last traversal took on this rank (as of the last mgx_dbfs2_status / mgx_dbfs2_run): out4 = { levels
 * whose push appended its discoveries to the id list itself (no sweep over the marks), levels whose short rows were walked vertex
 * by vertex, 1 if a sweep declared its list overflowed from the push's mark count, slices of the cold-edge lists stored at four
 * bytes per pair }.  Tests and tools. */
MGX_API int mgx_dbfs2_path_levels(mgx_dbfs2_t h, int64_t* out4);
MGX_API int mgx_dbfs2_free(mgx_dbfs2_t h);
/* All of reset / push / merge are asynchronous on the context's stream: a level is
 *   push(level) -> all-gather of d_newbits into d_gathered (the caller's collective, stream-ordered) -> merge(level)
 * and several levels can be enqueued before mgx_dbfs2_status synchronises.  Levels enqueued after the traversal has
 * ended are no-ops on every rank (their new-bit maps are empty).  Bitmaps are mgx_dbfs2_words(n) 32-bit words long
 * (padded to 16 bytes). */
MGX_API int mgx_dbfs2_words(int n_global, int64_t* words);
MGX_API int mgx_dbfs2_reset(mgx_dbfs2_t h, int src_global);
MGX_API int mgx_dbfs2_push(mgx_dbfs2_t h, int level);
MGX_API int mgx_dbfs2_merge(mgx_dbfs2_t h, int level, const unsigned* d_gathered);
/* The same for `maps` new-bit maps that lie `stride_words` apart (a multiple of 4, >= mgx_dbfs2_words): the padded
 * buffers of an all-gather, or ONE map that already is the OR of every rank's -- what a caller has after a
 * reduce-scatter (all-to-all of slices + OR) followed by an all-gather of the merged slices, which moves
 * 2 (R-1)/R bitmaps per rank and level instead of R-1. */
MGX_API int mgx_dbfs2_merge_maps(mgx_dbfs2_t h, int level, const unsigned* d_maps, int maps, int64_t stride_words);
/* The reduce step of that exchange: d_out[w] = OR over r < maps of d_maps[r * stride_words + w], w < words (words and
 * stride multiples of 4; d_out may be d_maps itself).  Asynchronous on the context's stream. */
MGX_API int mgx_dbfs2_or_maps(mgx_dbfs2_t h, const unsigned* d_maps, int maps, int64_t stride_words, int64_t words,
                              unsigned* d_out);
/* Synchronises.  next_level = number of levels enqueued so far.  out6: [0] traversal over (a level discovered nothing
 * on ANY rank -- the same on every rank, no reduction needed) [1] levels that hold vertices [2] edges this rank has
 * expanded [3] vertices discovered by all ranks in the level merged last [4] size and [5] edges of this rank's next
 * queues */
/* Sparse levels (lists on sparse levels, bitmaps on dense ones).  With a list set (mgx_dbfs2_set_list: a device
 * buffer of mgx_dbfs2_list_words(n, ranks) words -- 4 header words, [0] = count, then ids), mgx_dbfs2_push also writes the
 * rank's discoveries of the level there as vertex ids; a count above the capacity means "did not fit".  The caller all-gathers
 * the lists and hands them to mgx_dbfs2_apply_lists, which answers out3 = { 1: some list overflowed, NOTHING was applied,
 * exchange the bitmaps and call mgx_dbfs2_merge* as before | 0: the level is merged (every listed vertex decided once on
 * every rank, the owner's labels and next queues written); sum of the counts (0: no rank discovered anything -- the
 * traversal is over); 0 }.  It waits for that verdict only (a spin on pinned memory), not for the stream.             */
/* A rank's shard of the symmetrised R-MAT graph (scale, edgefactor, seed) under this layout, built inside the library on
 * the rank's GPU with no communication (every rank derives the same hub-first permutation from the same counter-based pair
 * stream): mgx_dbfs2_shard_plan makes the permutation and says how many rows and entries the rank holds; the caller
 * allocates; mgx_dbfs2_shard_fill writes local row offsets (n_local + 1), global neighbour ids (m_local) and, where not
 * NULL, new_of_old / old_of_new / degree_of_new (n each); mgx_dbfs2_shard_free releases the plan.  Untimed setup.     */
MGX_API int mgx_dbfs2_shard_plan(mgx_ctx_t ctx, int scale, int edgefactor, uint64_t seed, int ranks, int rank, void** plan, int* n_local, int64_t* m_local);
MGX_API int mgx_dbfs2_shard_fill(mgx_ctx_t ctx, void* plan, int* d_row_offsets_local, int* d_col_indices, int* d_new_of_old, int* d_old_of_new, int* d_degree_of_new);
MGX_API int mgx_dbfs2_shard_free(void* plan);
MGX_API int mgx_dbfs2_list_words(int n_global, int ranks, int64_t* words);
MGX_API int mgx_dbfs2_set_list(mgx_dbfs2_t h, unsigned* d_list, int64_t words);
MGX_API int mgx_dbfs2_apply_lists(mgx_dbfs2_t h, int level, const unsigned* d_lists, int lists, int64_t stride_words, int64_t* out3);
MGX_API int mgx_dbfs2_status(mgx_dbfs2_t h, int next_level, int64_t* out6);
MGX_API int mgx_dbfs2_labels(mgx_dbfs2_t h, int* host_labels_local);
/* this rank's copy of the visited bitmap over ALL vertices (mgx_dbfs2_words words, bit v = vertex v in hub-first global ids):
 * after a traversal every rank holds the same one -- what the tests check */
MGX_API int mgx_dbfs2_visited(mgx_dbfs2_t h, unsigned* host_words);

/* ---- the partitioned traversal driven from C++ over RCCL (include/mgx/comm.hpp, bfs_dist2.hpp: d2_run) ----
 * A communicator of the library's own: rank 0 calls mgx_comm_unique_id, the 128 bytes travel to the other ranks by any
 * means (the Python layer broadcasts them over torch.distributed), every rank calls mgx_comm_create (collective:
 * ncclCommInitRank).  RCCL is resolved at run time from the copy already in the process (PyTorch's librccl.so.1) or the
 * system's; mgx_comm_library says which.  mgx_dbfs2_run then runs a WHOLE traversal: reset, and per level push -> the
 * exchange of the new-bit maps (0: one ncclAllGather; 1: grouped ncclSend/ncclRecv of slices + OR + ncclAllGather of the
 * merged slices) -> merge, enqueued for a batch of levels at a time on the context's stream, one synchronisation per
 * batch; no host code runs between levels.  exchange_words: length of the exchanged map, >= mgx_dbfs2_words(n) and a
 * multiple of 4 * ranks -- the d_newbits buffer given to mgx_dbfs2_create must be that long.  comm may be NULL for
 * ranks == 1.  out6 as mgx_dbfs2_status. */
MGX_API int mgx_comm_unique_id(unsigned char* out128);
MGX_API int mgx_comm_create(mgx_ctx_t ctx, int ranks, int rank, const unsigned char* id128, mgx_comm_t* out);
MGX_API int mgx_comm_free(mgx_comm_t comm);
MGX_API const char* mgx_comm_library(void);
MGX_API int mgx_comm_available(void); /* 1: RCCL is in the process or could be loaded with every entry point the library needs */
/* The in-process stand-in for RCCL (include/mgx/comm_loopback.hpp): G host THREADS of one process as G ranks -- any devices, the
 * tests use one GPU, where RCCL itself refuses a second rank -- so that mgx_dbfs2_run / mgx_dsssp_run themselves can be run and
 * checked with 2 .. 64 ranks on a one-GPU box.  Since round 6 it is a library of its own, mini_amd/libmgx_loopback.so (built by
 * __graft_entry__.build()): libmgx.so only recognises an id that names it and loads the stand-in from next to itself then; without
 * that file both calls below return MGX_E_INVALID.  mgx_comm_loopback_id makes such an id; mgx_comm_create on it blocks until `ranks` threads have joined (or
 * MGX_LOOPBACK_TIMEOUT_S seconds, default 120, have passed: MGX_E_HIP, as every later call on that communicator).  Collectives
 * are host-synchronous device copies with the group semantics of ncclGroupStart / End.  Test infrastructure for the multi-rank
 * loops: nothing selects it by default.  mgx_comm_info: *is_loopback, and the collective rounds its world has completed. */
MGX_API int mgx_comm_loopback_id(unsigned char* out128);
MGX_API int mgx_comm_info(mgx_comm_t comm, int* is_loopback, int64_t* rounds);
/* A communicator's pre-flight, through the very function table the loops use (collective: every rank calls it): all-gather of the
 * first `words` words of d_send into d_gathered (ranks * words), then the slice exchange's pattern -- grouped send of slice r of
 * d_send (ranks * words) to rank r / receive from rank r into slice r of d_alltoall -- and a wait for the stream. */
MGX_API int mgx_comm_selftest(mgx_comm_t comm, const unsigned* d_send, unsigned* d_gathered, unsigned* d_alltoall, int64_t words);
MGX_API int mgx_dbfs2_run(mgx_dbfs2_t h, mgx_comm_t comm, int src_global, int exchange, int64_t exchange_words, int64_t* out6);
/* With id lists, mgx_dbfs2_run enqueues a WHOLE traversal ahead -- per level the push and either the lists or the bitmaps, as the
 * engine's last traversals went (the first one, and MGX_DIST_SPEC=0, look once per level) -- and waits once.  A list that overflows
 * against the plan freezes the traversal at that level on every rank alike; the host then sends that level through the bitmaps
 * and goes on level by level.  out5 = { traversals planned ahead, of those frozen, of those longer than planned, levels and
 * lists-mask (bit L: level L from id lists) of the last plan }. */
MGX_API int mgx_dbfs2_spec_stats(mgx_dbfs2_t h, int64_t* out5);
/* Level 0 of every traversal runs with a host look on every rank, and its all-gathered id-list headers carry each rank's plan: the
 * rest is enqueued ahead only when ALL ranks announced the same plan (round 6) -- a rank whose history differs (its engine handle was
 * recreated, MGX_DIST_SPEC is set in its environment only, a traversal threw there) makes every rank go level by level instead of
 * issuing different RCCL collectives.  mgx_dbfs2_forget_plan drops this engine's history (what a recreated handle starts with). */
MGX_API int mgx_dbfs2_forget_plan(mgx_dbfs2_t h);
/* The engines of ALL ranks of one partition, made on one context, driven in turn by the calling thread: the collectives are device
 * copies into one shared buffer, the level plan is mgx_dbfs2_run's.  A measurement and test entry (wall time / ranks = what one
 * rank's GPU spends per traversal, no exchange time); out6_each: ranks x 6, as mgx_dbfs2_status per engine. */
MGX_API int mgx_dbfs2_run_group(mgx_dbfs2_t* engines, int count, int src_global, int64_t exchange_words, int64_t* out6_each);

/* ---- SSSP: sssp_problem_t / sssp_functor_t / sssp_enactor_t (gunrock/src/sssp/) ---- */
MGX_API int mgx_sssp_create(mgx_graph_t g, int src, mgx_sssp_t* out);     /* sssp_problem.hxx:40-52 */
MGX_API int mgx_sssp_reset(mgx_sssp_t p, int src);
MGX_API int mgx_sssp_free(mgx_sssp_t p);
MGX_API int mgx_sssp_distances(mgx_sssp_t p, float* host_dist);           /* extract() :54-57       */
/* After mgx_sssp_enact: the functor's preds (sssp_functor.hxx:31-34; racy as the reference's).  After mgx_sssp_run (the fused loop
 * keeps none): a shortest-path TREE built from the final distances the first time it is asked for (include/mgx/sssp_preds.hpp) --
 * pred[v] = the largest u with a tight edge u -> v from a strictly nearer vertex; equal-distance ties (zero weights) are resolved in
 * rounds so that no cycle can form; pred[source] = pred[unreached] = -1.  mgx_sssp_build_preds builds them without copying:
 * stats2 = { equal-distance tight edges found, rounds }. */
MGX_API int mgx_sssp_preds(mgx_sssp_t p, int* host_preds);
MGX_API int mgx_sssp_build_preds(mgx_sssp_t p, int64_t* stats2);
MGX_API int mgx_sssp_distances_device(mgx_sssp_t p, float** d_dist);
/* advance_forward_kernel<sssp_problem_t,sssp_functor_t,false,true> (sssp_enactor.hxx:49-54) */
MGX_API int mgx_sssp_advance(mgx_sssp_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front);
/* filter_kernel<sssp_problem_t,sssp_functor_t>                     (sssp_enactor.hxx:60-65) */
MGX_API int mgx_sssp_filter(mgx_sssp_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept);
/* sssp_enactor_t::enact (sssp_enactor.hxx:40-72).  stats[0]=iterations, [1]=edge relaxations,
 * [2]=sum of input frontier lengths.                                                      */
MGX_API int mgx_sssp_enact(mgx_sssp_t p, float queue_sizing, int64_t* stats);
/* fused device-resident SSSP (same fixed point): stats as above                          */
MGX_API int mgx_sssp_run(mgx_sssp_t p, int src, int64_t* stats);
/* the same with near / far buckets of width delta (the delta-stepping BASELINE config 3 names): improved vertices whose
 * distance lies at or above the current threshold wait until the queue of nearer ones has run dry, then the threshold
 * moves to the bucket of the smallest waiting distance.  Same fixed point, fewer relaxations, more (cheap) iterations.
 * delta == 0: off (plain frontier Bellman-Ford, what mgx_sssp_run does); delta < 0: the default (off).  stats as above ([0] counts
 * the iterations incl. the bucket changes). */
MGX_API int mgx_sssp_run_delta(mgx_sssp_t p, int src, float delta, int64_t* stats);
/* per-launch timing of the relax kernel of mgx_sssp_run (k_sssp_relax: sssp_functor.hxx:20-29 over every edge of the
 * frontier): on != 0 brackets each launch with HIP events on the context's stream (each costs ~6 us of stream gap: measurement
 * runs only); mgx_sssp_kernel_times: out2 = { launches, device ns } of the last run                                        */
MGX_API int mgx_sssp_set_kernel_timing(mgx_sssp_t p, int on);
/* per-iteration trace of the last mgx_sssp_run (first min(cap, 63) iterations): frontier vertices, edges relaxed, duration in
 * ms from device-side timestamps taken when an iteration is opened (0 for the last one); *iterations = how many there were */
MGX_API int mgx_sssp_iteration_trace(mgx_sssp_t p, int cap, int64_t* frontier, int64_t* edges, float* ms, int* iterations);
MGX_API int mgx_sssp_kernel_times(mgx_sssp_t p, int64_t* out2);
/* which paths the last mgx_sssp_run / mgx_sssp_run_delta took (include/mgx/sssp_fused.hpp); MGX_E_INVALID before the first run.
 *   out8[0]  1: the heavy iterations' sweep over the unit blocks was available to the run (a weighted layout the library built
 *            with a long-row threshold of 17 .. 64 and at least 16 units, the direct queue build, no near / far buckets,
 *            MGX_SSSP_DENSE not 0)
 *   out8[1]  the sweep's variant: 0 none (out8[0] == 0); 1 32-bit ids + float weights; 2 24-bit ids + float weights;
 *            3 24-bit ids + half weights (every weight of the unit blocks survives the round trip through IEEE half)
 *   out8[2]  iterations the sweep relaxed
 *   out8[3]  iterations the queue walk relaxed with the hubs' distance bounds in LDS (MGX_SSSP_HOT_MIN_EDGES)
 *   out8[4]  iterations the queue walk relaxed without them
 *   out8[5]  queue build: 0 direct (k_sssp_build2), 1 list (k_sssp_build: MGX_SSSP_BUILD_LIST=1 or row offsets off 16 bytes)
 *   out8[6]  iterations that only moved the near / far threshold (0 in a plain run)
 *   out8[7]  1: the run relaxed in layout space
 * out8[2] + out8[3] + out8[4] + out8[6] == stats[0] of the run.  Counted on the host, when asked, from the per-iteration trace
 * the device keeps, with the very predicates the kernels select by; the trace holds 4096 iterations: MGX_E_INVALID for a
 * longer run.
 * The sweep never runs on a layout attached with mgx_graph_attach_layout / _attach_layout_weights: its short-row walk loads 16
 * bytes from a row's start whatever the row's length, and borrowed arrays end at exactly num_edges entries (a layout the library
 * builds carries 8 entries of slack).  out8[0] is 0 there. */
MGX_API int mgx_sssp_path_info(mgx_sssp_t p, int64_t* out8);

/* ---- PR: pr_problem_t / pr_functor_t / pr_enactor_t (gunrock/src/pr/) ---- */
MGX_API int mgx_pr_create(mgx_graph_t g, int max_iter, mgx_pr_t* out);    /* pr_problem.hxx:33-44   */
MGX_API int mgx_pr_free(mgx_pr_t p);
MGX_API int mgx_pr_enact(mgx_pr_t p, int64_t* frontier_len_per_iter, int* iterations); /* pr_enactor.hxx:41-79 */
MGX_API int mgx_pr_ranks(mgx_pr_t p, float* host_ranks);

/* ---- k-core: kcore_problem_t / kcore_functor.hxx / kcore_enactor_t (gunrock/src/kcore/) ---- */
MGX_API int mgx_kcore_create(mgx_graph_t g, mgx_kcore_t* out);             /* kcore_problem.hxx:37-49 */
MGX_API int mgx_kcore_reset(mgx_kcore_t p);                                /* core numbers 0, degrees = row lengths */
MGX_API int mgx_kcore_free(mgx_kcore_t p);
/* kcore_enactor_t::enact (kcore_enactor.hxx:40-86): peeling on filter<deg_less_than_k> / advance<update_deg, false, false> /
 * filter<deg_atleast_k>.  *largest_k_core: what the enactor found (-1 if no k <= n ended the run: only a graph without
 * entries, an upstream quirk that is kept).  stats[0] = k values tried, [1] = passes, [2] = entries expanded,
 * [3] = vertices removed (stats may be NULL).  The run consumes the working degrees: mgx_kcore_reset before another one. */
MGX_API int mgx_kcore_enact(mgx_kcore_t p, int* largest_k_core, int64_t* stats);
/* the fused path (mgx/kcore_fused.hpp): the same peeling as worklists -- a pass looks only at the vertices whose degree the
 * pass before took below k, and the next k is 1 + the smallest positive working degree.  Core numbers, working degrees and
 * *largest_k_core equal mgx_kcore_enact's on every graph (stranded vertices and the k <= n cap included), on the
 * plain CSR in original ids.  It starts afresh by itself, on the context's stream: no mgx_kcore_reset before or after, and it may
 * follow an enact directly.  stats (may be NULL): [0] levels (values of k at which somebody left), [1] removing passes,
 * [2] entries expanded, [3] vertices removed, [4] stranded vertices (degree from >= k to <= 0 within one pass: core 0),
 * [5] host waits.  Against mgx_kcore_enact's stats e: [1] = e[1] - e[0], [2] = e[2], [3] = e[3]. */
MGX_API int mgx_kcore_run(mgx_kcore_t p, int* largest_k_core, int64_t* stats);
/* what every launch of the last fused run was, in order (for joining a kernel trace with the run's steps): 1 smallest degree,
 * 2 list the level's first front, 3 expand, 4 filter, 6 one workgroup's own passes on a small front, 5 behind the end.
 * *launches: how many the run enqueued; min(*launches, cap, 65536) kinds are written.  MGX_E_INVALID before any fused run. */
MGX_API int mgx_kcore_step_kinds(mgx_kcore_t p, int* host_kinds, int cap, int64_t* launches);
MGX_API int mgx_kcore_num_cores(mgx_kcore_t p, int* host_num_cores);       /* extract() :51-53        */
MGX_API int mgx_kcore_degrees(mgx_kcore_t p, int* host_degrees);           /* the working degrees (<= 0 once a run is over) */

/* ---- graph colouring: coloring_problem_t / coloring_functor.hxx / coloring_enactor_t (gunrock/src/coloring/) ----
 * Two colours per round from local minima and maxima of a per-round key: salt_i = fmix32(seed + 0x9E3779B9 * (i + 1)),
 * key_i(v) = fmix32(v ^ salt_i), unsigned.  Round i, every v uncoloured at its start: key_i(v) <= min of its uncoloured
 * neighbours' keys -> colour 2i + 1, else >= their max -> 2i + 2 (0: uncoloured).  Keys are distinct, so self-loops and parallel
 * entries change nothing.  Stops after max_iter rounds or when none is left; max_iter <= 0: until none is left (at most
 * ceil(n / 2) rounds).  Proper on a symmetric graph; a directed one is coloured by its out-rows, not necessarily properly.
 * Every run starts from all-uncoloured, on the context's stream.  stats (may be NULL): [0] rounds run, [1] vertices left
 * uncoloured, [2] largest colour (0: none), [3] host waits the run made. */
MGX_API int mgx_color_create(mgx_graph_t g, mgx_color_t* out);
MGX_API int mgx_color_free(mgx_color_t p);
/* the fused path (mgx/color_fused.hpp): one launch per round, rounds enqueued in batches, one host wait per batch */
MGX_API int mgx_color_run(mgx_color_t p, unsigned seed, int max_iter, int64_t* stats);
/* the operator path (coloring_enactor.hxx): neighbourhood max / min reduce over the iota frontier, filter over the active */
MGX_API int mgx_color_enact(mgx_color_t p, unsigned seed, int max_iter, int64_t* stats);
/* colours of the last run of either path (MGX_E_INVALID before any run); the device pointer stays valid until the next run or free */
MGX_API int mgx_color_colors(mgx_color_t p, int* host_colors);
MGX_API int mgx_color_colors_device(mgx_color_t p, const int** d_colors);
/* active vertices at the start of each round of the last run: *rounds gets the round count, at most cap are written */
MGX_API int mgx_color_round_trace(mgx_color_t p, int64_t* active_at_round_start, int cap, int* rounds);
/* the fused path's row classes (all host-side): consts4 = { long_min: rows of at least this many entries are long, seg: entries of a
 * long row one wave scans, stage: segments a wave's LDS stage holds -- a surviving row of more goes out on its own --, batch_max:
 * rounds per host wait at most }; and per round the LAST FUSED run ran, three values at the start of the round: short rows, long
 * items (segments), long rows still uncoloured (round 0: short rows = vertices of fewer than long_min entries).  *rounds gets the
 * round count, at most cap triples are written (round_triples may be NULL with cap <= 0).  MGX_E_INVALID before any fused run. */
MGX_API int mgx_color_info(mgx_color_t p, int64_t* consts4, int64_t* round_triples, int cap, int* rounds);

/* ---- local graph sparsification: lspar_problem_t / lspar_functor.hxx / lspar_enactor_t (gunrock/src/lspar/) ----
 * One definition, rows read as they stand (duplicates and self-loops count):
 *   salt_j = fmix32(seed + 0x9E3779B9 * (j + 1)), h_j(u) = fmix32(u ^ salt_j), j = 0 .. k - 1 (colouring's keys)
 *   mh_j(v) = unsigned min of h_j over the entries of row v (0xFFFFFFFF: empty row)
 *   sim of entry (v, u) = number of j with mh_j(v) == mh_j(u), 0 .. k
 *   t(v) = min(d, floor(pow(d, e) * (1 + 2^-40))) in double, d = the row's length
 *   row v keeps its first t(v) entries in the order (sim descending, position ascending), written in row order.
 * The result is a CSR of the same n: out_ro (n + 1), out_ci (kept neighbours), out_eid (index into the input col_indices),
 * out_sim.  k must be 1 .. 32 and e finite and >= 0 (else MGX_E_INVALID before any device work); the reference driver's
 * defaults are seed 15485863, k = 1, e = 0.5.  Everything runs on the context's stream.  stats (may be NULL): [0] kept
 * entries, [1] rows cut (t < d), [2] host waits the run made. */
MGX_API int mgx_lspar_create(mgx_graph_t g, mgx_lspar_t* out);
MGX_API int mgx_lspar_free(mgx_lspar_t p);
/* the fused path (mgx/lspar_fused.hpp): a minhash pass and a select pass, one host wait */
MGX_API int mgx_lspar_run(mgx_lspar_t p, unsigned seed, int k, double e, int64_t* stats);
/* the operator path (lspar_enactor.hxx): neighbourhood reduce, advance, segmented sort, advance, compaction, segmented sort */
MGX_API int mgx_lspar_enact(mgx_lspar_t p, unsigned seed, int k, double e, int64_t* stats);
/* the last run's result (MGX_E_INVALID before any run); NULL skips an array.  Sizes: n + 1 and stats[0] */
MGX_API int mgx_lspar_result(mgx_lspar_t p, int* h_ro, int* h_ci, int* h_eid, int* h_sim);
/* the same on the device, valid until the next run or free (NULL skips one) */
MGX_API int mgx_lspar_result_device(mgx_lspar_t p, const int** d_ro, const int** d_ci, const int** d_eid, const int** d_sim);
/* the last run's minhash table, n x k, vertex-major */
MGX_API int mgx_lspar_minhashes(mgx_lspar_t p, unsigned* h_minhashes);
/* the fused path's row classes (all host-side): out5 = { short_max: rows of at most this many entries take the group kernels, seg:
 * entries of a longer row one wave item covers, k_max, and of the LAST FUSED run: the minhash table's stride (k <= 2: k, else k
 * rounded up to a multiple of 4) and its items (segments of the rows longer than short_max) }.  MGX_E_INVALID before any fused run. */
MGX_API int mgx_lspar_info(mgx_lspar_t p, int64_t* out5);
/* a NEW graph that owns a device copy of the last result (weights: the kept entries' input weights, gathered by eid);
 * free it with mgx_graph_free */
MGX_API int mgx_lspar_graph(mgx_lspar_t p, mgx_graph_t* out);

/* ---- connected components ----
 * Weakly connected components: every CSR entry (v, u) is read as the undirected pair {v, u}; self-loops and duplicate entries
 * change nothing, a vertex without entries is a component of its own.  label[v] = the smallest vertex id of v's component, in
 * original ids (an attached hub-first layout is ignored).  stats (may be NULL): [0] components (v with label[v] == v), [1] size of
 * the largest, [2] its label (on a tie in size, the smallest label), [3] vertices whose rows the fused final pass skipped (always
 * 0 on the operator path), [4] host waits the run made.  Every run starts afresh, on the context's stream. */
MGX_API int mgx_cc_create(mgx_graph_t g, mgx_cc_t* out);
MGX_API int mgx_cc_free(mgx_cc_t p);
/* the fused path (mgx/cc_fused.hpp): Afforest-style union-find, one host wait.  symmetric != 0 is the caller's word that every
 * entry has its reverse: the labels are right on a symmetric graph; on a directed one only with symmetric = 0, which is right on
 * any graph (the final pass then uses the graph's genuine CSC if it has one, else skips nothing).  seed picks the 1024 sampled
 * vertices; the labels do not depend on it.  stats[3]: vertices in the sampled largest set after the two neighbour rounds that
 * had entries left to link (out-entries from the third on, or in-entries of the genuine CSC) */
MGX_API int mgx_cc_run(mgx_cc_t p, int symmetric, unsigned seed, int64_t* stats);
/* the operator path (include/gunrock/cc/): Shiloach-Vishkin hook advances and pointer-jumping filters; right on any graph */
MGX_API int mgx_cc_enact(mgx_cc_t p, int64_t* stats);
/* labels of the last run of either path (MGX_E_INVALID before any run); the device pointer stays valid until the next run or free */
MGX_API int mgx_cc_labels(mgx_cc_t p, int* host_labels);
MGX_API int mgx_cc_labels_device(mgx_cc_t p, const int** d_labels);

/* ---- triangle counting ----
 * Triangles of the underlying simple undirected graph: every CSR entry (v, u) with v != u is read as the pair {v, u}; self-loops
 * and duplicate entries change nothing; original ids (an attached hub-first layout is ignored).  tri[v] = the triangles that
 * contain v (64 bits), total = sum of tri / 3, sdeg[v] = the distinct neighbours of v other than v.  Both paths count on the same
 * oriented graph (DAG), built on the device at the first run and kept on the handle per `symmetric` value: dag_ro[n + 1],
 * dag_ci[m_dag], row a = the distinct neighbours of a of higher rank, ascending by id; a triangle of ranks a < b < c is counted
 * once, at entry (a, b).  symmetric != 0 is the caller's word that every entry has its reverse: rank = (row length, id) and only
 * the entries with rank(v) < rank(u) are kept -- the counts are right on a symmetric graph; symmetric = 0 is right on any graph
 * (deg(v) = row length + entries that name v, every entry oriented from its lower-ranked end).  stats (int64, may be NULL):
 * [0] triangles, [1] m_dag (the simple undirected edges), [2] the longest oriented row, [3] oriented wedges (sum of d+(d+ - 1)/2),
 * [4] 1 if the rows were found ascending and used as they are (symmetric != 0 only), 0 if a sorted copy was made, [5] 1 if this
 * run built the DAG, 0 if it reused an earlier run's, [6] host waits the run made, [7] launches it enqueued.  [0] - [4] are equal
 * between the two paths; [7] counts kernel launches and clears (the read-back copies are not in it).  A CSR of more than 2^30
 * entries is refused with MGX_E_FRONTIER_OVERFLOW at the first run (the sort's merge passes keep run widths in ints; m_dag <= m, so
 * m_dag < 2^31 always holds), no memory is MGX_E_HIP.  Every run starts afresh, on the
 * context's stream. */
MGX_API int mgx_tc_create(mgx_graph_t g, mgx_tc_t* out);
MGX_API int mgx_tc_free(mgx_tc_t p);
/* the fused path (mgx/tc_fused.hpp): rows binned by oriented length; short rows an entry a lane, longer ones staged in LDS by a
 * wave or a workgroup while the rows of their entries are streamed; one host wait (the stats) */
MGX_API int mgx_tc_run(mgx_tc_t p, int symmetric, int64_t* stats);
/* the operator path (include/gunrock/tc/): one advance over the DAG's entries, a thread intersects the two rows of an entry */
MGX_API int mgx_tc_enact(mgx_tc_t p, int symmetric, int64_t* stats);
/* results of the last run of either path (MGX_E_INVALID before any run); the device pointers stay valid until the next run or free */
MGX_API int mgx_tc_triangles(mgx_tc_t p, int64_t* host_tri);
MGX_API int mgx_tc_triangles_device(mgx_tc_t p, const int64_t** d_tri);
MGX_API int mgx_tc_simple_degrees(mgx_tc_t p, int* host_sdeg);
MGX_API int mgx_tc_simple_degrees_device(mgx_tc_t p, const int** d_sdeg);
/* which kernel the rows of the last run's DAG go to on the fused path, and the switches in effect (MGX_E_INVALID before any run):
 * out[7] = rows counted an entry a lane, rows a wave stages, rows a workgroup stages (rows of fewer than two entries are in no
 * list), entries of a workgroup's stage, entries of a wave's stage, MGX_TC_SHORT_MAX, MGX_TC_WAVE_MAX as read */
MGX_API int mgx_tc_bins(mgx_tc_t p, int64_t* out);
/* the last run's DAG: h_ro[n + 1], h_ci[stats[1]]; h_ci may be NULL to fetch the offsets only */
MGX_API int mgx_tc_dag(mgx_tc_t p, int* h_ro, int* h_ci);

/* ---- betweenness centrality (mgx/bc_fused.hpp, include/gunrock/bc/) ----
 * Brandes on the unweighted graph: a CSR entry (u, v) is an edge u -> v, every entry counts once (duplicate entries are parallel
 * edges and distinct shortest paths, as for mgx_pagerank_*), self-loops lie on no shortest path; original ids (an attached hub-first
 * layout serves the traversal underneath, the centrality kernels ignore it).  For a source s: label = BFS depth (-1 unreached),
 * sigma[v] = the shortest s -> v entry-paths (sigma[s] = 1), delta[v] = sum over the entries (v, w) with label[w] = label[v] + 1 of
 * sigma[v] / sigma[w] * (1 + delta[w]), bc[v] = sum over the given sources s != v of delta_s[v] -- networkx.betweenness_centrality(
 * DiGraph, normalized=False) when there are no duplicate entries and the sources are all vertices.  sigma, delta, bc are double;
 * sigma is exact below 2^53.  sources == NULL: all n vertices (count is ignored); count < 0 or a source out of range: MGX_E_INVALID
 * before any device work; count == 0: a valid run that leaves bc all zero.  symmetric != 0 is the caller's word that every entry has
 * its reverse (the in-entries of v are then row v); symmetric = 0 takes the in-entries from the graph's genuine CSC
 * (mgx_graph_build_csc, or one uploaded) and is MGX_E_INVALID without one (mgx_bc_run only: the operator path reads out-entries alone).
 * stats (int64[10], may be NULL): [0] sources run, [1] the deepest traversal in levels, [2] vertices reached summed over the sources,
 * [3] inexact: some sigma reached 2^53, [4] overflow: some sigma is not finite (neither is an error status), [5] host waits of the
 * run's own, [6] the traversals' host waits (fused path), [7] launches of the run's own (kernels, clears, a sort as one; fused path),
 * [8] chain launches, [9] 1 if the in-entries came from the CSC.  Every run starts afresh, on the context's stream. */
MGX_API int mgx_bc_create(mgx_graph_t g, mgx_bc_t* out);
MGX_API int mgx_bc_free(mgx_bc_t p);
/* the fused path: per source the fused BFS (push mode), the level lists by one radix sort, then pull sweeps level by level -- no
 * atomic, results bit-equal from run to run; ONE host wait of its own, at the end */
MGX_API int mgx_bc_run(mgx_bc_t p, const int* sources, int count, int symmetric, int64_t* stats);
/* the operator path: advance + filter per level with a CAS on the label and a double atomicAdd per shortest-path entry, one advance
 * per level backwards */
MGX_API int mgx_bc_enact(mgx_bc_t p, const int* sources, int count, int symmetric, int64_t* stats);
/* results of the last run of either path (MGX_E_INVALID before any run): the centrality summed over the run's sources; sigma, delta
 * and labels of its LAST source.  The device pointer stays valid until the next run or free */
MGX_API int mgx_bc_centrality(mgx_bc_t p, double* host_bc);
MGX_API int mgx_bc_centrality_device(mgx_bc_t p, const double** d_bc);
MGX_API int mgx_bc_sigma(mgx_bc_t p, double* host_sigma);
MGX_API int mgx_bc_delta(mgx_bc_t p, double* host_delta);
MGX_API int mgx_bc_labels(mgx_bc_t p, int* host_labels);
/* what the fused path did with the graph (MGX_E_INVALID before any run): out[16] = [0..2] vertices whose in-row is folded by a lane /
 * a wave / in segments, [3..5] the same for the out-rows, [6] [7] segments of the huge in- / out-rows, [8..11] MGX_BC_LANE_MAX,
 * MGX_BC_HUGE_MIN, MGX_BC_SEG, MGX_BC_CHAIN as read, [12] levels of the last source, [13] its chain launches, [14] [15] the longest
 * in- / out-row.  [0..7], [14], [15] describe the last fused run's tables (0 before one) */
MGX_API int mgx_bc_info(mgx_bc_t p, int64_t* out);
/* measurement (tools/bc_bench.py): with timing on, a fused run puts HIP events around the phases of its first 64 sources (a few
 * microseconds of stream gap each); mgx_bc_phase_ms then gives out[5] = ms per source of the traversal, the list build (clears, keys,
 * sort, bounds), the forward launches, the backward launches (with the final sigma launch), and the number of sources timed */
MGX_API int mgx_bc_set_timing(mgx_bc_t p, int on);
MGX_API int mgx_bc_phase_ms(mgx_bc_t p, double* out);

/* ---- PageRank to convergence (mgx/pagerank_fused.hpp, include/gunrock/pagerank/) ----
 * Not mgx_pr_*: that is the reference's pr_enactor_t loop, kept quirk for quirk.  This is PageRank: CSR entry (u, v) is an edge
 * u -> v (duplicates count once each, self-loops count), d(u) the length of row u, r_0 = 1 / n,
 *   r_{t+1}[v] = (1 - alpha) / n + alpha * (sum of r_t[u] / d(u) over the in-entries (u, v) + D_t / n),  D_t = the ranks of the
 * vertices without out-entries, e_{t+1} = |r_{t+1} - r_t|_1; the run stops after the first iteration with e <= tol (converged) or
 * after max_iter iterations.  Ranks are float, D and e double; the ranks sum to 1.
 * symmetric != 0 is the caller's word that every entry has its reverse: the in-entries of v are then row v of the CSR.
 * symmetric == 0: the in-entries come from the graph's genuine CSC (mgx_graph_build_csc, or one uploaded); a graph without one gets
 * MGX_E_INVALID.  Every run starts afresh, on the context's stream. */
MGX_API int mgx_pagerank_create(mgx_graph_t g, mgx_pagerank_t* out);
MGX_API int mgx_pagerank_free(mgx_pagerank_t p);
/* alpha in [0, 1), tol >= 0 and finite, max_iter >= 1: else MGX_E_INVALID before any device work.
 * stats (may be NULL): [0] iterations run, [1] converged (0 / 1), [2] vertices without out-entries,
 * [3] reduce path (1: the layout's sliced kernels, 0: general; always 0 from mgx_pagerank_enact, whose operator chooses for itself),
 * [4] host waits the run made, [5] launches the path enqueued (mgx_pagerank_enact: without the operator's own).
 * *residual (may be NULL): e of the last iteration.
 * mgx_pagerank_run: the fused path -- the iterations end on the device, the host looks once per batch of them; two runs with the same
 * arguments give bit-equal ranks and residuals.  mgx_pagerank_enact: the operator path (neighbourhood-reduce + update, two host
 * waits per iteration), right on any graph under the same rule for symmetric. */
MGX_API int mgx_pagerank_run  (mgx_pagerank_t p, double alpha, double tol, int max_iter, int symmetric, int64_t* stats, double* residual);
MGX_API int mgx_pagerank_enact(mgx_pagerank_t p, double alpha, double tol, int max_iter, int symmetric, int64_t* stats, double* residual);
/* ranks of the last run of either path by original id (MGX_E_INVALID before any run); the device pointer stays valid until the next
 * run or free */
MGX_API int mgx_pagerank_ranks(mgx_pagerank_t p, float* host_ranks);
MGX_API int mgx_pagerank_ranks_device(mgx_pagerank_t p, const float** d_ranks);
/* e_1 .. of the last run: min(cap, iterations, 65536) values into host_e; *iterations (may be NULL) = iterations run */
MGX_API int mgx_pagerank_residuals(mgx_pagerank_t p, double* host_e, int cap, int* iterations);
/* which class of the general reduce took the in-rows of the last mgx_pagerank_run (MGX_E_INVALID before any): out[4] = rows in the
 * huge list (a workgroup each; 0 after a run on the layout), PGR_LANE_MAX (rows of at most so many entries a lane each),
 * PGR_HUGE_MIN (rows of at least so many a workgroup each; the others a wave each), PGR_HUGE_BLOCKS (workgroups that stride over
 * the huge list).  Reports; steers nothing. */
MGX_API int mgx_pagerank_bins(mgx_pagerank_t p, int64_t* out);

/* ---- minimum spanning forest (include/mgx/mst_fused.hpp, include/gunrock/mst/) ----
 * Every CSR entry (v, u, w) is the undirected edge {v, u} of the graph's float weight w (1.0f when none were uploaded); self-loops
 * are ignored, parallel entries are parallel edges, a vertex without entries is a tree of its own.  Weights are ordered by
 * key(w) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) of their IEEE bits b, -0.0 read as +0.0 (and reported as +0.0); negative weights
 * are allowed; a NaN weight makes the run MGX_E_INVALID, found at the run's host wait, and leaves no result.  Edges are ordered by
 * (key(w), min(v, u), max(v, u)), entries with the same triple are the same edge: the minimum spanning forest is unique and both
 * paths return the same set of (a, b, w), a < b.  The fused path's list order is a function of the graph alone (ascending position
 * in its sorted incident arrays), list and total are bit-equal from run to run; the operator path's list order is not specified.
 * symmetric != 0 is the caller's word that every entry has its reverse with the same weight; symmetric == 0 takes the in-entries
 * from the graph's genuine CSC (mgx_graph_build_csc, or one uploaded; row values included) and is MGX_E_INVALID without one, on both
 * paths.  A false word may give a wrong forest; it never hangs or faults.
 * stats (may be NULL), int64[8]: [0] edges (n - components), [1] components, [2] size of the largest, [3] its label, [4] rounds that
 * chose something, [5] host waits the run made (fused: counted where the host waits; operator path: one per operator call, each
 * reads its count back, plus the read-backs at the end), [6] cursor steps summed (fused: entries a lane looked at plus 64-entry steps of a
 * wave; 0 on the operator path), [7] incident entries after dropping self-loops (both ends' when symmetric == 0).  A graph of more
 * than 2^29 entries is MGX_E_FRONTIER_OVERFLOW.  Every run starts afresh, on the context's stream; the fused path keeps its sorted
 * incident arrays per `symmetric` on the handle. */
MGX_API int mgx_mst_create(mgx_graph_t g, mgx_mst_t* out);
MGX_API int mgx_mst_free(mgx_mst_t p);
/* the fused path: Boruvka rounds with a monotone cursor per vertex; one host wait whatever the number of rounds */
MGX_API int mgx_mst_run(mgx_mst_t p, int symmetric, int64_t* stats);
/* the operator path: two advances and a hook filter per round over all entries, pointer-jumping filters; the host loops */
MGX_API int mgx_mst_enact(mgx_mst_t p, int symmetric, int64_t* stats);
/* results of the last run of either path (MGX_E_INVALID before any run, and after one that failed): stats[0] entries each, any of
 * the arrays may be NULL; the total weight, summed in double in an order fixed by the list; labels[v] = the smallest vertex id of
 * v's component.  Device pointers stay valid until the next run or free. */
MGX_API int mgx_mst_edges(mgx_mst_t p, int* h_a, int* h_b, float* h_w);
MGX_API int mgx_mst_edges_device(mgx_mst_t p, const int** d_a, const int** d_b, const float** d_w);
MGX_API int mgx_mst_weight(mgx_mst_t p, double* total);
MGX_API int mgx_mst_labels(mgx_mst_t p, int* host_labels);
MGX_API int mgx_mst_labels_device(mgx_mst_t p, const int** d_labels);
/* the last fused run (MGX_E_INVALID before one): out8 = [0] long-row items processed over all rounds (a wave each), [1] short-row
 * items (a lane each), [2] MGX_MST_LONG_MIN in effect, [3] MGX_MST_SEG in effect, [4] merge passes of the setup sort, [5] 1 if the
 * setup was reused, [6] [7] 0 */
MGX_API int mgx_mst_info(mgx_mst_t p, int64_t* out8);

/* ---- k-truss decomposition (include/mgx/ktruss_fused.hpp, include/gunrock/ktruss/) ----
 * The graph is the underlying simple undirected graph of the triangle count (self-loops and duplicate entries change nothing,
 * original ids, `symmetric` as in mgx_tc_run).  Its edges are the entries of the oriented graph that count builds: edge e joins
 * src[e] to dst[e], stats[1] of them.  sup0[e] = the triangles that contain e; truss[e] = the largest k such that e lies in a
 * subgraph whose every edge is in at least k - 2 of its triangles (an edge without triangles: 2); vtruss[v] = the largest trussness
 * of an edge at v (0: none); hist[k] = edges of trussness k.  Both paths and tests/ktruss_model.py peel by the same simultaneous
 * rule, so supports after every pass, levels and passes are unique.
 * stats (may be NULL), int64[8]: [0] largest trussness (0 without edges), [1] edges, [2] triangles, [3] levels (values of k that had
 * a front), [4] passes, [5] 1 if this run built the oriented graph and the adjacency with edge ids (kept per `symmetric` on the
 * handle), [6] host waits the run made, counted where the host waits (the first run's include the builds': the oriented graph's
 * stats, the adjacency's size check, the two of the sort's host side; operator path: one per operator call), [7] launches (fused:
 * the idle ones behind the run's end included; the sort's counted as if every band ran; operator path: two per operator call).
 * A graph of more than 2^30 entries is MGX_E_FRONTIER_OVERFLOW at the first run, no memory is MGX_E_HIP.  Every run starts
 * afresh, on the context's stream. */
MGX_API int mgx_ktruss_create(mgx_graph_t g, mgx_ktruss_t* out);
MGX_API int mgx_ktruss_free(mgx_ktruss_t p);
/* the fused path: supports by the triangle count's kernels with the adds sent to the entries; the peel as a chain of launches
 * whose kind is decided on the device, one host wait per batch of launches (64, 128, 256, 256 ...) */
MGX_API int mgx_ktruss_run(mgx_ktruss_t p, int symmetric, int64_t* stats);
/* the operator path: one advance for the supports, three filters over edge ids per pass; the host loops */
MGX_API int mgx_ktruss_enact(mgx_ktruss_t p, int symmetric, int64_t* stats);
/* results of the last run of either path (MGX_E_INVALID before any run); any array of _edges and _adjacency may be NULL.
 * _edges, _support: stats[1] entries in the order of the oriented graph's entries; _vertex_truss: n; _histogram: min(cap, n + 1)
 * counts; _adjacency: ro[n + 1], ci and eid[2 stats[1]]: row v = the simple neighbours of v ascending, each with its edge's id.
 * _order: the peel order of the last FUSED run (every front is a range of it; MGX_E_INVALID when the last run was not fused).
 * Device pointers stay valid until the next run or free. */
MGX_API int mgx_ktruss_edges(mgx_ktruss_t p, int* h_src, int* h_dst, int* h_truss);
MGX_API int mgx_ktruss_support(mgx_ktruss_t p, int* h_sup0);
MGX_API int mgx_ktruss_vertex_truss(mgx_ktruss_t p, int* h_vtruss);
MGX_API int mgx_ktruss_histogram(mgx_ktruss_t p, int64_t* h_hist, int cap);
MGX_API int mgx_ktruss_order(mgx_ktruss_t p, int* h_order);
MGX_API int mgx_ktruss_adjacency(mgx_ktruss_t p, int* h_ro, int* h_ci, int* h_eid);
MGX_API int mgx_ktruss_truss_device(mgx_ktruss_t p, const int** d_truss);
MGX_API int mgx_ktruss_vertex_truss_device(mgx_ktruss_t p, const int** d_vtruss);
/* what every launch of the last fused run's peel was, in order: 1 smallest support, 2 list the level's first front, 3 expand,
 * 4 seal, 5 behind the end.  *launches: how many the peel enqueued; min(*launches, cap, 65536) kinds are written.  MGX_E_INVALID
 * before any fused run. */
MGX_API int mgx_ktruss_step_kinds(mgx_ktruss_t p, int* host_kinds, int cap, int64_t* launches);
/* timing (measurement tools; off by default): on != 0 makes every fused run record events round its support launches and its
 * peel (one more host wait at the run's end, not counted in stats[6]); mgx_ktruss_phase_ms then gives out[2] = ms of the support
 * launches and of the peel (its clears and idle launches included) of the last fused run */
MGX_API int mgx_ktruss_set_timing(mgx_ktruss_t p, int on);
MGX_API int mgx_ktruss_phase_ms(mgx_ktruss_t p, double* out);

/* ---- strongly connected components (include/mgx/scc_fused.hpp, include/gunrock/scc/) ----
 * The graph is the directed graph whose arcs are the CSR entries (v -> u), in original ids; an attached layout is ignored,
 * self-loops and duplicate entries change no label.  label[v] = the smallest vertex id of v's strongly connected component (a
 * vertex on no cycle is a component of its own).  Both runs need the graph's genuine CSC for the in-entries: without it they
 * return MGX_E_INVALID.  Both paths and tests/scc_model.py run the same scheme -- trim to the fixpoint, one pivot reach, colouring
 * rounds, a trim behind each -- whose alive set after every phase is unique.
 * stats (may be NULL), int64[8]: [0] components, [1] the largest one's size, [2] its label (ties: the smaller), [3] vertices the
 * trims removed over the whole run, [4] size of the pivot's component (0: nobody was alive after the first trim), [5] rounds,
 * [6] host waits (fused: one per batch of launches and one for [0] - [2]; operator path: one per operator call and that one),
 * [7] launches (fused: the idle ones behind the run's end included; operator path: operator calls).  Every run starts afresh, on
 * the context's stream; a second run allocates nothing.  A run that fails leaves no result: the getters, mgx_scc_step_kinds and
 * mgx_scc_phase_ms included, return MGX_E_INVALID until a run succeeds.  MGX_E_HIP "a fixpoint did not end": more than n + 2
 * launches of one kind in a row, which the definition rules out -- a fault of the library, reported instead of run on. */
MGX_API int mgx_scc_create(mgx_graph_t g, mgx_scc_t* out);
MGX_API int mgx_scc_free(mgx_scc_t p);
/* the fused path: a chain of launches whose kind is decided on the device, one host wait per batch of launches (64, 128, 256,
 * 256 ...) */
MGX_API int mgx_scc_run(mgx_scc_t p, int64_t* stats);
/* the operator path: filters that recount for the trims and the pivot, advances with an atomicMin functor forward and a claiming
 * functor over the transposed graph backward; the host loops */
MGX_API int mgx_scc_enact(mgx_scc_t p, int64_t* stats);
/* the labels of the last run of either path (MGX_E_INVALID before any run); the device pointer stays valid until the next run or
 * free */
MGX_API int mgx_scc_labels(mgx_scc_t p, int* host_labels);
MGX_API int mgx_scc_labels_device(mgx_scc_t p, const int** d_labels);
/* what every launch of the last fused run was, in order: 1 degrees, 2 list the first trim front, 3 expand (take the degrees down
 * for who left), 4 pivot: largest product, 5 pivot: smallest id, 6 round init, 7 forward sweep, 8 roots, 9 backward sweep, 10 seal,
 * 11 behind the end.  *launches: how many the run enqueued; min(*launches, cap, 65536) kinds are written.  MGX_E_INVALID before
 * any fused run. */
MGX_API int mgx_scc_step_kinds(mgx_scc_t p, int* host_kinds, int cap, int64_t* launches);
/* timing (measurement tools; off by default): on != 0 makes every launch of a fused run add the device's wall clock since the
 * launch before it to that launch's phase; mgx_scc_phase_ms then gives out[4] = ms of the last fused run's degree init, trims
 * (all of them), pivot phase and rounds */
MGX_API int mgx_scc_set_timing(mgx_scc_t p, int on);
MGX_API int mgx_scc_phase_ms(mgx_scc_t p, double* out);

/* ---- label propagation and modularity (include/mgx/lpa_fused.hpp, include/gunrock/lpa/) ----
 * Community detection by label propagation, in original ids; an attached layout is ignored.  symmetric != 0 is the caller's word
 * that every entry has its reverse: each CSR entry (v, u), u != v, gives v one vote for label[u].  symmetric == 0 is right on any
 * graph: each entry (v, u), u != v, gives v one vote for label[u] and u one vote for label[v]; it needs the graph's genuine CSC
 * and is MGX_E_INVALID without one.  Self-loops never vote, duplicate entries vote once each, edge weights are not used.
 * label_0[v] = v; in iteration t every vertex with votes wants the label most of its votes carry (its current one on a tie, else
 * the smallest); unstable_t counts those that want another.  unstable_t == 0 ends the run (converged, iterations = t), t ==
 * max_iter ends it too.  mode MGX_LPA_SYNC: every unstable vertex moves; MGX_LPA_LAZY: those with color_key(v, color_salt(seed,
 * t)) & 1 (include/mgx/color_hash.hpp) -- the synchronous rule oscillates on anything bipartite.  Both paths and
 * tests/lpa_model.py compute the same labels bit for bit.
 * mode must be 0 or 1 and max_iter in [0, 2^20], else MGX_E_INVALID before any device work; more than 2^30 entries:
 * MGX_E_FRONTIER_OVERFLOW (mgx_lpa_enact with symmetric == 0: 2^30 entries or more, its 2 m vote slots are addressed by ints).
 * stats (may be NULL), int64[10]: [0] communities (distinct labels), [1] the largest one's size, [2] its label (ties: the
 * smaller), [3] iterations, [4] converged (0 / 1), [5] unstable of the last iteration evaluated, [6] rows evaluated over the run
 * (operator path: n x (iterations + 1)), [7] rows that overflowed their LDS table, [8] host waits (fused: one per batch of
 * launches and one for [0] - [2]), [9] launches (fused: the idle ones behind the run's end included; operator path: operator
 * calls).  Every run starts afresh, on the context's stream; a second run allocates nothing.  A run that fails leaves no result:
 * the getters return MGX_E_INVALID until a run succeeds. */
#define MGX_LPA_SYNC 0
#define MGX_LPA_LAZY 1
MGX_API int mgx_lpa_create(mgx_graph_t g, mgx_lpa_t* out);
MGX_API int mgx_lpa_free(mgx_lpa_t p);
/* the fused path: a chain of launches whose kind is decided on the device, one host wait per batch of launches (64, 128, 256,
 * 256 ...) */
MGX_API int mgx_lpa_run(mgx_lpa_t p, int symmetric, int mode, uint32_t seed, int max_iter, int64_t* stats);
/* the operator path: advances that gather every vote's label, the segmented sort, a filter that scans every vertex's sorted votes
 * and one that applies the moves; every vertex every iteration */
MGX_API int mgx_lpa_enact(mgx_lpa_t p, int symmetric, int mode, uint32_t seed, int max_iter, int64_t* stats);
/* the labels of the last run of either path; the device pointer stays valid until the next run or free */
MGX_API int mgx_lpa_labels(mgx_lpa_t p, int* host_labels);
MGX_API int mgx_lpa_labels_device(mgx_lpa_t p, const int** d_labels);
/* per iteration of the last run (iterations + 1 of them), three values: unstable_t, the vertices whose label changed, the vertices
 * evaluated.  *iterations: how many triples the run has; min(*iterations, cap) are written. */
MGX_API int mgx_lpa_trace(mgx_lpa_t p, int64_t* host_triples, int cap, int64_t* iterations);
/* what every launch of the last fused run was, in order: 1 setup, 2 evaluate all vertices, 3 evaluate the active list, 4 the long
 * rows, 5 apply over all vertices, 6 apply over the list, 7 behind the end, 8 mark the voters of the movers' long rows.  *launches: how many the run enqueued;
 * min(*launches, cap, 65536) kinds are written.  MGX_E_INVALID before any fused run. */
MGX_API int mgx_lpa_step_kinds(mgx_lpa_t p, int* host_kinds, int cap, int64_t* launches);
/* the last fused run, int64[9]: [0] - [3] vertices whose rows have no entries / take a lane / a wave / a workgroup, [4] - [7]
 * MGX_LPA_SHORT_MAX, _WAVE_MAX, _TABLE and _LIST_DIV as read, [8] rows that overflowed their table over the whole run */
MGX_API int mgx_lpa_bins(mgx_lpa_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_lpa_phase_ms gives out[4] = ms of the last fused run's setup, evaluations,
 * long rows and applies */
MGX_API int mgx_lpa_set_timing(mgx_lpa_t p, int on);
MGX_API int mgx_lpa_phase_ms(mgx_lpa_t p, double* out);
/* Modularity of any labelling (d_labels: n labels in [0, n) on the device): out[3] = {S_in, S_sq, W} with S_in the votes whose two
 * ends carry equal labels, S_sq the sum over the labels of (the votes of their vertices)^2, W all votes; Q = S_in / W - S_sq /
 * W^2 (0 when W == 0) is the caller's division.  A label outside [0, n): MGX_E_INVALID, found at the call's host wait.  The n
 * sums the call needs are allocated at the graph's first call and kept with it: a second call allocates nothing. */
MGX_API int mgx_modularity(mgx_graph_t g, const int* d_labels, int symmetric, uint64_t* out);

/* ---- bit-parallel multi-source BFS and closeness (include/mgx/msbfs_fused.hpp, include/gunrock/msbfs/) ----
 * BFS depths from many sources at once, in original ids; an attached layout is ignored.  A CSR entry (u, v) is an edge u -> v;
 * duplicates and self-loops change nothing.  depth_s[v] is the BFS depth from s along out-entries, 0 at s, -1 when unreached: what
 * mgx_bfs_labels gives for every source.  sources[count] is cut into batches of 64 in the given order (source 64 B + b is bit b
 * of batch B: one 64-bit word per vertex serves the batch's traversals); duplicates are allowed and give equal rows; sources ==
 * NULL means all n vertices (count is ignored); count < 0 or an id out of range is MGX_E_INVALID before any device work; count
 * == 0 is a valid empty run.  A batch whose deepest vertex is at depth D runs D + 1 levels.
 * Level t is a PULL (every vertex some source has not seen ORs its in-neighbours' front words, no atomics but for segmented huge
 * rows) iff in-entries are available and MGX_MSBFS_PULL_DIV > 0 and e_t x MGX_MSBFS_PULL_DIV >= m, e_t the out-entries of the
 * level's front; else a PUSH over the front's list (a 64-bit atomicOr per entry that brings new bits).  In-entries are the rows
 * themselves when symmetric != 0 (the caller's word that every entry has its reverse), else the graph's genuine CSC; with
 * symmetric == 0 and no CSC the run is valid and every level pushes.  mgx_msbfs_enact always pushes.
 * Results of a run, over all its sources: per source reach (vertices at depth >= 1), far (the sum of their depths), ecc (the
 * deepest level), exact, and harm = the sum of cnt_d / d over d = 1, 2 ... in double, added in ascending d (bit-equal from run
 * to run); per vertex reach_in (the sources, with their multiplicity, that have it at depth >= 1) and far_in (the sum of those
 * depths); with want_depths != 0 the depths, int32[count][n].  Depths that do not fit in memory: MGX_E_HIP.  Closeness is the
 * caller's division: reach / far x reach / (n - 1).
 * stats (may be NULL), int64[10]: [0] sources, [1] batches, [2] levels of the deepest batch, [3] the sum of reach, [4] PUSH
 * levels, [5] PULL levels, [6] host waits (fused: one per batch of launches of the chain -- 64, 128, 256, 256 ... -- and one for
 * the read-back of the per-source results), [7] launches (fused: the idle ones behind the run's end included; operator path:
 * operator calls), [8] 1 if the genuine CSC served as the in-entries (operator path: 0), [9] 1 if depths were kept.  Every run
 * starts afresh, on the context's stream; a repeat run allocates nothing.  A run that fails leaves no result: the getters return
 * MGX_E_INVALID until a run succeeds, as they do before any run. */
#define MGX_MSBFS_PUSH 0
#define MGX_MSBFS_PULL 1
MGX_API int mgx_msbfs_create(mgx_graph_t g, mgx_msbfs_t* out);
MGX_API int mgx_msbfs_free(mgx_msbfs_t p);
/* the fused path: a chain of launches whose kind is decided on the device; batches of sources follow each other without a host wait */
MGX_API int mgx_msbfs_run(mgx_msbfs_t p, const int* sources, int count, int symmetric, int want_depths, int64_t* stats);
/* the operator path: per level an advance that ORs, a filter that dedups and finalizes, a host wait */
MGX_API int mgx_msbfs_enact(mgx_msbfs_t p, const int* sources, int count, int symmetric, int want_depths, int64_t* stats);
/* the last run's per-source results, host arrays of its count */
MGX_API int mgx_msbfs_reach(mgx_msbfs_t p, int64_t* host);
MGX_API int mgx_msbfs_far(mgx_msbfs_t p, int64_t* host);
MGX_API int mgx_msbfs_ecc(mgx_msbfs_t p, int64_t* host);
MGX_API int mgx_msbfs_harmonic(mgx_msbfs_t p, double* host);
/* the last run's per-vertex sums, n each; the device pointers stay valid until the next run or free */
MGX_API int mgx_msbfs_vertex_sums(mgx_msbfs_t p, int64_t* reach_in, int64_t* far_in);
MGX_API int mgx_msbfs_vertex_sums_device(mgx_msbfs_t p, const int64_t** d_reach_in, const int64_t** d_far_in);
/* the last run's depths, int32[count][n]; MGX_E_INVALID when it kept none */
MGX_API int mgx_msbfs_depths(mgx_msbfs_t p, int* host);
/* MGX_MSBFS_PUSH or _PULL per (batch, level) of the last fused run, the batches behind each other.  *levels: how many it ran;
 * min(*levels, cap, 65536) kinds are written */
MGX_API int mgx_msbfs_level_kinds(mgx_msbfs_t p, int* host_kinds, int cap, int64_t* levels);
/* the last fused run, int64[14]: [0] - [3] out-rows without entries / a lane's / a wave's / segmented, [4] the segments of the
 * latter, [5] - [9] the same of the in-rows (zeros when every level pushes), [10] - [13] MGX_MSBFS_SHORT_MAX, _WAVE_MAX, _SEG
 * and _PULL_DIV as read */
MGX_API int mgx_msbfs_bins(mgx_msbfs_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_msbfs_phase_ms gives out[4] = ms of the last fused run's PUSH, PULL, LONG and
 * FINALIZE launches (RESET and SEED count as FINALIZE) */
MGX_API int mgx_msbfs_set_timing(mgx_msbfs_t p, int on);
MGX_API int mgx_msbfs_phase_ms(mgx_msbfs_t p, double* out);

/* ---- random walks and node2vec sampling (include/mgx/rw_fused.hpp, include/gunrock/rw/) ----
 * Walks along out-entries, in original ids; an attached layout is ignored.  A CSR entry (u, v) is a step u -> v, duplicates count
 * as often as they are stored.  starts is a host int32[count], NULL means every vertex in order (count is ignored); walker w of
 * [0, count x walks_per_start) starts at starts[w / walks_per_start] and takes up to `length` steps.  Its path has length + 1
 * slots: slot 0 the start, -1 behind the walk's end.  A start outside [0, n), count < 0, length < 0, walks_per_start < 1, p or q
 * not finite or <= 0, restart outside [0, 1): MGX_E_INVALID before any device work; count x walks_per_start >= 2^31:
 * MGX_E_FRONTIER_OVERFLOW; the path matrix is addressed in 64 bits.
 * Every draw is draw(seed, w, t, k) = fmix32(fmix32(fmix32(seed + 0x9E3779B9 (w + 1)) ^ 0x85EBCA6B (t + 1)) ^ 0xC2B2AE35 (k + 1))
 * (fmix32: murmur3's 32-bit finalizer), t the step, k the draw within it: a walker's path depends on the graph, the seed and w
 * alone.  u(r) = float(r >> 8) 2^-24; a position in a row of d entries is the high word of r x d (a position's probability is off
 * 1 / d by at most 2^-32, a row's total bias at most d / 2^32).  Step t from cur (prev: the vertex before it, none at the start
 * and behind a restart):
 *   1. restart > 0 and u(draw(k = 0)) < restart: to the walker's start; a step and a restart.
 *   2. cur's row is dead (no entries; weighted: its maximum weight is <= 0): the walk ends, a dead end -- with restart > 0 it
 *      jumps to the start as in 1 instead.
 *   3. tries i = 0 .. MGX_RW_TRIES - 1 (64): position j = hi(draw(k = 1 + 2 i) x d) in the row's STORED order, c its vertex, a =
 *      u(draw(k = 2 + 2 i)); accepted iff a * (wmax * M) < w_j * b in float32 products.  weighted == 0: w = wmax = 1.  First order
 *      (p == q == 1 or no prev): b = M = 1.  Second order (node2vec): b = 1 / p when c == prev, 1 when prev has an entry to c,
 *      1 / q otherwise; M = max(1 / p, 1, 1 / q).  The unweighted first-order step takes try 0.
 *   4. after MGX_RW_TRIES rejections: the row's first entry of maximum weight, a fallback.  The sampled distribution is the
 *      intended one exactly where stats[6] == 0; the expected tries per step are wmax M / mean(w b).
 * Setup, per handle, redone when a run's mode needs what is missing: weighted runs the rows' maxima (a negative or NaN weight is
 * MGX_E_NEGATIVE_WEIGHT; a graph without uploaded weights has all 1.0f), second-order runs a check that every row ascends, and
 * a sorted copy of col_indices for the membership search where one does not (stats[7]).
 * stats (may be NULL), int64[10]: [0] walkers, [1] length, [2] steps taken, [3] dead ends, [4] restarts, [5] tries (candidates
 * drawn), [6] fallbacks, [7] 1 if the membership search ran on a sorted copy, [8] launches (fused: two for a setup, one for a
 * sorted copy's sort, one walk; operator path: operator calls on top of the setup's), [9] host waits (fused: one for the starts'
 * upload when given, one for a setup and two for a sort, one for the counters).  Every run starts afresh, on the context's stream;
 * a repeat run allocates nothing.  A run that fails leaves no result: the getters return MGX_E_INVALID until a run succeeds. */
MGX_API int mgx_rw_create(mgx_graph_t g, mgx_rw_t* out);
MGX_API int mgx_rw_free(mgx_rw_t p);
/* the fused path: one launch walks every walker, a lane each; the paths leave through an LDS tile of MGX_RW_TILE slots */
MGX_API int mgx_rw_run(mgx_rw_t p, const int* starts, int count, int walks_per_start, int length, uint32_t seed, int weighted, float p_ret,
                       float q_inout, float restart, int want_paths, int want_visits, int64_t* stats);
/* the operator path: a filter over the live walkers per step, a host wait each; the same results, bit for bit */
MGX_API int mgx_rw_enact(mgx_rw_t p, const int* starts, int count, int walks_per_start, int length, uint32_t seed, int weighted, float p_ret,
                         float q_inout, float restart, int want_paths, int want_visits, int64_t* stats);
/* the last run's paths, int32[walkers][length + 1]; MGX_E_INVALID when it kept none.  The device pointer stays valid until the
 * next run or free */
MGX_API int mgx_rw_paths(mgx_rw_t p, int* host);
MGX_API int mgx_rw_paths_device(mgx_rw_t p, const int** d_paths);
/* the last run's last vertex and steps taken per walker, host int32[walkers] */
MGX_API int mgx_rw_ends(mgx_rw_t p, int* host);
MGX_API int mgx_rw_lengths(mgx_rw_t p, int* host);
/* the last run's visits, int64[n]: the path slots that hold every vertex, slot 0 included; MGX_E_INVALID when it kept none */
MGX_API int mgx_rw_visits(mgx_rw_t p, int64_t* host);
MGX_API int mgx_rw_visits_device(mgx_rw_t p, const int64_t** d_visits);
/* int64[10]: [0] - [3] the rows without entries / a lane's / a wave's / segmented of the handle's last setup launch, [4] the
 * segments of the latter (zeros before any setup), [5] - [9] MGX_RW_SHORT_MAX, _WAVE_MAX, _SEG, _TRIES and _TILE as read */
MGX_API int mgx_rw_bins(mgx_rw_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_rw_phase_ms gives out[2] = ms of the last fused run's setup and walk */
MGX_API int mgx_rw_set_timing(mgx_rw_t p, int on);
MGX_API int mgx_rw_phase_ms(mgx_rw_t p, double* out);

/* ---- Louvain community detection (include/mgx/louvain_fused.hpp, include/mgx/louvain_aggregate.hpp) ----
 * Levels of local moves that raise the modularity, each followed by a contraction of the communities into the next level's
 * weighted graph.  Level 0 takes the votes of mgx_lpa_* and mgx_modularity: symmetric != 0 (the caller's word that every entry has
 * its reverse): every CSR entry (v, u), u != v, is weight 1 from v to u; symmetric == 0: every entry gives weight 1 to both ends,
 * which needs the graph's genuine CSC (mgx_graph_build_csc, or one uploaded) and is MGX_E_INVALID without one.  Self-loops are
 * dropped, duplicate entries add, float edge values are not used, an attached layout is ignored.
 * An iteration scores for every vertex its own label and its neighbours' (s(c) = k_vc W - (Sigma_c - [c is its own] k_v) k_v),
 * takes the best (ties: the current label, then the smaller color_key(c, seed)) and moves there when the key falls (even
 * iterations) or rises (odd ones); the moved labelling is accepted iff a vertex moved and Qnum = S_in W - S_sq grew by more than
 * (int64) ceil(tol * W * W).  A level ends after two consecutive rejected iterations or at max_iter; a level that accepted nothing
 * ends the run, as does max_levels.  All of it is integer arithmetic: the run and tests/louvain_model.py agree bit for bit.
 * max_iter in [0, 2^20], max_levels in [0, 64], tol in [0, 1] and not NaN, else MGX_E_INVALID before any device work; more than
 * 2^30 entries, or 2^30 - 1 and more with symmetric == 0 (the contraction addresses the votes by int32): MGX_E_FRONTIER_OVERFLOW,
 * before any device work as well.
 * stats, int64[10] (may be NULL): [0] communities, [1] the largest one's vertices, [2] its id, [3] levels aggregated, [4] S_in,
 * [5] S_sq, [6] W of the final labels (Q = S_in / W - S_sq / W^2 is the caller's division; 0 when W == 0), [7] host waits,
 * [8] launches of the levels' chains, [9] iterations over all levels.
 * The state is allocated at the first run, bounded by the graph's vertices and entries: a repeat run allocates nothing (a later
 * run does only when it asks for more iterations than any before, or is the handle's first with symmetric == 0).  A run that fails leaves no result: the getters return MGX_E_INVALID until
 * a run succeeds.  mgx_louvain_enact is the operator path (include/gunrock/louvain/): the same results and stats, [8] being its
 * operator calls; every vertex every iteration, a host wait per operator.  _step_kinds, _bins and _phase_ms describe fused runs
 * only (MGX_E_INVALID behind an operator run). */
/* how many device arrays the library has allocated in this process so far: equal before and after a call that allocates nothing */
MGX_API long long mgx_device_allocations(void);
MGX_API int mgx_louvain_create(mgx_graph_t g, mgx_louvain_t* out);
MGX_API int mgx_louvain_free(mgx_louvain_t p);
MGX_API int mgx_louvain_run(mgx_louvain_t p, int symmetric, uint32_t seed, int max_iter, int max_levels, double tol, int64_t* stats);
MGX_API int mgx_louvain_enact(mgx_louvain_t p, int symmetric, uint32_t seed, int max_iter, int max_levels, double tol, int64_t* stats);
/* labels of the last run.  level == -1: the composition of the levels' maps, n labels in [0, communities).  0 <= level < levels:
 * that level's map, as many labels as the level has vertices (mgx_louvain_levels), in [0, its communities).  The device pointer
 * stays valid until the next run or free. */
MGX_API int mgx_louvain_labels(mgx_louvain_t p, int level, int* host_labels);
MGX_API int mgx_louvain_labels_device(mgx_louvain_t p, int level, const int** d_labels);
/* the levels that ran, the last one that accepted nothing included: (vertices, entries, iterations, accepted iterations,
 * communities, Qnum) each; *levels_run: how many there are, at most cap sextuples are written */
MGX_API int mgx_louvain_levels(mgx_louvain_t p, int64_t* host_sextuples, int cap, int64_t* levels_run);
/* (moved, accepted, Qnum of the moved labelling) per iteration, the levels one behind the other */
MGX_API int mgx_louvain_trace(mgx_louvain_t p, int64_t* host_triples, int cap, int64_t* iterations);
/* the launches of the levels' chains, each level up to its first DONE: 1 setup, 2 evaluate, 3 long rows into their tables, 4 long
 * rows' tables scored, 5 apply, 6 Qnum, 7 done.  *launches: how many there are; min(*launches, cap) kinds are written.  Of a
 * level of more than 65 536 launches only the first 65 536 are kept: its list then ends without its 7. */
MGX_API int mgx_louvain_step_kinds(mgx_louvain_t p, int* host_kinds, int cap, int64_t* launches);
/* int64[8]: [0] - [3] vertices without entries / a lane's / a wave's / long, summed over the levels; [4] - [6]
 * MGX_LOUVAIN_SHORT_MAX, _WAVE_MAX and _SEG as read; [7] the long rows' (vertex, segment) items over all iterations */
MGX_API int mgx_louvain_bins(mgx_louvain_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_louvain_phase_ms gives out[6] = ms of the last run's setup, evaluations, long
 * rows, applies, Qnum launches (device clock) and aggregation (host clock, waits included) */
MGX_API int mgx_louvain_set_timing(mgx_louvain_t p, int on);
MGX_API int mgx_louvain_phase_ms(mgx_louvain_t p, double* out);

/* ---- neighbour sampling for GNN mini-batches (include/mgx/nsample_fused.hpp, include/gunrock/nsample/) ----
 * Fan-out sampling in the GraphSAGE / NeighborLoader shape along out-entries, in original ids; an attached layout is ignored.  seeds
 * is a host int32[count], duplicates allowed, NULL means every vertex (count is ignored); fanouts is a host int32[hops], every
 * entry -1 (all of a row's entries) or 1 .. 64.
 *   frontiers   V_0 is the ascending set of distinct seeds.  For h = 0 .. hops - 1 every v of V_h is sampled once; V_{h+1} is the
 *               ascending set of the sampled destinations that are in none of V_0 .. V_h: a vertex is sampled at most once in a
 *               run.  A vertex's local id is its place in V_0 | V_1 | ... | V_hops.
 *   a row       v at hop h, d entries, k = fanouts[h], key = step_key(walker_key(seed, v), h) of the random walks' draws (above),
 *               from the GLOBAL id: a vertex's sample depends on the graph, seed, h and v, never on who else is in the batch.
 *               d == 0: nothing.  k == -1, or replace == 0 and d <= k: positions 0 .. d - 1 in the row's STORED order (a whole row).
 *               replace != 0: k positions hi(draw(key, j) x d), j = 0 .. k - 1.  Otherwise Floyd's algorithm, exactly k draws, no
 *               retries: for j = 0 .. k - 1, i = d - k + j, t = hi(draw(key, j) x (i + 1)), p_j = i when t is among p_0 .. p_{j-1}
 *               (a collision), else t.  Slot j of the row holds p_j: insertion order, no sort.  Self-loops and duplicate entries
 *               are entries like any other.
 * Results: vertices int32[N] (local -> global), hop_offsets int32[hops + 2] (V_h = vertices[hop_offsets[h], hop_offsets[h + 1])),
 * row_offsets int32[R + 1], R = hop_offsets[hops] (the sampled subgraph as a CSR over the local rows; {0} when hops == 0), cols
 * int32[E] (local ids), entry_pos int32[E] (the index into the graph's col_indices / weights of every sampled entry), seed_local
 * int32[count].
 * hops outside [0, 16], a fan-out that is neither -1 nor in 1 .. 64, count < 0, a seed outside [0, n): MGX_E_INVALID before any
 * device work, the message names the parameter.  The arrays are sized before the first launch by bounds: F_0 = min(n, count), E_h =
 * F_h x k_h (clamped to m unless replace; k = -1: m), F_{h+1} = min(n, E_h); a bound of 2^31 or more is MGX_E_FRONTIER_OVERFLOW,
 * before any device work as well.  They live on the handle and only grow: a repeat run of the same or a smaller shape allocates
 * nothing.
 * stats (may be NULL), int64[14]: [0] seeds, [1] distinct seeds, [2] hops, [3] vertices N, [4] rows R, [5] entries E, [6] rows
 * without entries, [7] whole rows, [8] sampled rows, [9] draws, [10] collisions, [11] revisits (sampled entries whose destination
 * had a local id before its hop's new vertices were numbered), [12] launches (fused: 5 hops + 4; operator path: operator calls),
 * [13] host waits (fused: one for the seeds' upload when given, one for the totals).  Without vertices or without seeds a run
 * does no device work: launches and waits are 0.  Every run starts afresh, on the context's stream.  A run that fails leaves no
 * result: the getters return MGX_E_INVALID until a run succeeds. */
MGX_API int mgx_nsample_create(mgx_graph_t g, mgx_nsample_t* out);
MGX_API int mgx_nsample_free(mgx_nsample_t p);
/* the fused path: per hop a launch that counts, one that samples (a group of lanes per row, membership by one ballot), one for
 * the segments of long copied rows and two that rank the new vertices' bits; nothing is read back between the hops */
MGX_API int mgx_nsample_run(mgx_nsample_t p, const int* seeds, int count, const int* fanouts, int hops, int replace, uint32_t seed,
                            int64_t* stats);
/* the operator path: a filter over the frontier, a lane per row, and a filter over all vertices for the next frontier; the same
 * results, bit for bit */
MGX_API int mgx_nsample_enact(mgx_nsample_t p, const int* seeds, int count, const int* fanouts, int hops, int replace, uint32_t seed,
                              int64_t* stats);
/* the last run's arrays to the host (sizes: stats [3], hops + 2, [4] + 1, [5], [5], [0]); the device pointers stay valid until the
 * next run or free (NULL where the array is empty) */
MGX_API int mgx_nsample_vertices(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_hop_offsets(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_row_offsets(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_cols(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_entry_pos(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_seed_local(mgx_nsample_t p, int* host);
MGX_API int mgx_nsample_vertices_device(mgx_nsample_t p, const int** d_vertices);
MGX_API int mgx_nsample_row_offsets_device(mgx_nsample_t p, const int** d_row_offsets);
MGX_API int mgx_nsample_cols_device(mgx_nsample_t p, const int** d_cols);
MGX_API int mgx_nsample_entry_pos_device(mgx_nsample_t p, const int** d_entry_pos);
/* int64[8]: [0] - [3] the rows without entries / a lane's / a wave's / segmented among the rows the last fused run copied in its
 * hops with fan-out -1, [4] the segments of the latter, [5] - [7] MGX_NSAMPLE_SHORT_MAX, _WAVE_MAX and _SEG as read */
MGX_API int mgx_nsample_bins(mgx_nsample_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_nsample_phase_ms gives out[2] = ms of the last fused run's sampling launches
 * and of its deduplication (marks, ranks, renumbering) */
MGX_API int mgx_nsample_set_timing(mgx_nsample_t p, int on);
MGX_API int mgx_nsample_phase_ms(mgx_nsample_t p, double* out);

/* ---- neighbour feature aggregation for GNN layers (include/mgx/agg_fused.hpp, include/gunrock/agg/) ----
 * For every row r of a CSR the reduction of its neighbours' feature rows, Y[r, f] = (+) over the entries e of row r of t_e, the
 * memory-bound step of a GraphSAGE / GCN layer, in a FIXED order of arithmetic: both paths and tests/agg_model.py give the same
 * float32 bits, on every run.
 *   the CSR   source 0: the graph's out-rows; 1: its in-rows (needs the genuine CSC, mgx_graph_build_csc); 2: the rows of `block`'s
 *             last successful sampling run, read on the device without a copy: hop h's rows, or all R sampled rows with hop = -1.
 *             A block's columns are local ids: X is then indexed by local id and needs the run's `vertices` rows.  Original ids; an
 *             attached layout is ignored.
 *   X, Y      float32 device arrays, row-major: X is x_rows x feats with leading dimension ldx >= feats, Y is R x feats with ldy >=
 *             feats.  Their ranges must not overlap.  Every element of Y[:R, :feats] is written on every run, the padding columns
 *             feats .. ldy - 1 never.
 *   a term    t_e = X[col_e, f], or with weighted != 0 w_e * X[col_e, f] rounded once to float32: the multiply and the add are never
 *             fused.  w_e is the graph's weight of the entry (out-rows; a block's through entry_pos) or the CSC's row value (in-rows).
 *   the order a row's entries are cut into segments of seg entries in STORED order (MGX_AGG_SEG, a power of two in 64 .. 4096,
 *             default 256).  Within a segment acc = t_0, then acc = acc (+) t_j, j = 1, 2, ..; the row's value is the segments' values
 *             combined the same way, in segment order: a row of at most seg entries is one plain left-to-right fold.  (+) is float32 +
 *             for MGX_AGG_SUM and MGX_AGG_MEAN, t > acc ? t : acc for MGX_AGG_MAX, t < acc ? t : acc for MGX_AGG_MIN, which fixes +-0
 *             and NaN by the order.  MEAN divides the sum by float(d), one correctly rounded division.  A row without entries gives
 *             0.0 for every op.
 * MGX_E_INVALID before any device work, the message names the parameter: feats outside [1, 65536], ldx or ldy below feats, an unknown
 * op or source, weighted without weights, in-rows without a CSC, a block of another graph or without a successful run, hop outside
 * [-1, the run's hops), x_rows below n (the graph's rows) or below the run's vertices (a block), NULL d_x or d_y with R > 0,
 * overlapping X and Y.
 * stats (may be NULL), int64[9]: [0] rows R, [1] entries, [2] feats, [3] team width G (lanes a row takes), [4] column tiles, [5] 1
 * on the vector path (feats, ldx, ldy multiples of 4 and both bases 16-byte aligned: a lane owns 4 columns), [6] seg, [7] launches
 * (mgx_agg_enact: operator calls), [8] host waits.  mgx_agg_run only enqueues on the context's stream: 1 launch (3 with rows longer
 * than seg) and no wait; the run that builds a plan of the long rows has 2 launches and 1 wait more: the first run on the out-rows
 * and on the in-rows (kept for the handle's life), and every run on a block whose sampling run had a fan-out of -1.  R == 0: nothing.
 * Partials and plans live on the handle and only grow: a repeat run of the same or a smaller shape allocates nothing.  A call that
 * is refused leaves no result: the getters return MGX_E_INVALID until a call succeeds. */
#define MGX_AGG_SUM 0
#define MGX_AGG_MEAN 1
#define MGX_AGG_MAX 2
#define MGX_AGG_MIN 3
#define MGX_AGG_OUT_ROWS 0
#define MGX_AGG_IN_ROWS 1
#define MGX_AGG_BLOCK 2
MGX_API int mgx_agg_create(mgx_graph_t g, mgx_agg_t* out);
MGX_API int mgx_agg_free(mgx_agg_t p);
/* the fused path: a team of lanes per row, the loads of 8 entries in flight, one launch; rows longer than seg as (row, segment)
 * items and a fold of their partials in segment order */
MGX_API int mgx_agg_run(mgx_agg_t p, int source, mgx_nsample_t block, int hop, const float* d_x, int64_t x_rows, int64_t ldx, int feats, int op,
                        int weighted, float* d_y, int64_t ldy, int64_t* stats);
/* the operator path: one filter over the rows, a lane per row, column by column; the same bits */
MGX_API int mgx_agg_enact(mgx_agg_t p, int source, mgx_nsample_t block, int hop, const float* d_x, int64_t x_rows, int64_t ldx, int feats, int op,
                          int weighted, float* d_y, int64_t ldy, int64_t* stats);
/* for callers with host arrays: mgx_agg_upload copies host_x (rows x feats, contiguous) into an array the handle owns and gives its
 * device address (leading dimension feats); mgx_agg_output gives a handle-owned device array of rows x ld floats to pass as d_y.
 * Both grow only and stay valid until a larger request or free. */
MGX_API int mgx_agg_upload(mgx_agg_t p, const float* host_x, int64_t rows, int feats, float** d_x);
MGX_API int mgx_agg_output(mgx_agg_t p, int64_t rows, int64_t ld, float** d_y);
/* the last call's Y[:R, :feats] to the host, contiguous (R x feats), from wherever the call wrote it; waits */
MGX_API int mgx_agg_result(mgx_agg_t p, float* host_y);
/* int64[5] of the last fused run, counted by its own launches (waits): [0] rows without entries, [1] rows of at most seg entries (a
 * team's), [2] longer rows, [3] the segments of the latter, [4] seg */
MGX_API int mgx_agg_bins(mgx_agg_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_agg_phase_ms gives out[3] = ms of the last fused run's rows, items and fold
 * launches (waits for them) */
MGX_API int mgx_agg_set_timing(mgx_agg_t p, int on);
MGX_API int mgx_agg_phase_ms(mgx_agg_t p, double* out);

/* ---- the backward of the neighbour feature aggregation (include/mgx/agg_backward.hpp, include/gunrock/aggbwd/) ----
 * The gradient of mgx_agg_* with respect to the features: GX[c, f] = (+) over the selected rows' entries e with col_e == c of u_e,
 * in a FIXED order of arithmetic: both paths and tests/aggbwd_model.py give the same float32 bits, on every run.  A handle of its
 * own: the forward handle's state is never touched.  source, block, hop, op, weighted and MGX_AGG_SEG mean what they mean to
 * mgx_agg_run (seg is read once per handle).
 *   GY, X, GX float32 device arrays, row-major: GY is R x feats with ldgy (the gradient with respect to the forward's Y), X is the
 *             forward's X, x_rows x feats with ldx, read by MAX and MIN only (d_x may be NULL for SUM and MEAN, and is then ignored),
 *             GX is x_rows x feats with ldgx.  x_rows is at least n (the graph's rows) or the run's vertices (a block).  No two of
 *             the three may overlap.  Every element of GX[:x_rows, :feats] is written on every run, the padding columns never.
 *   upstream  g[r, f] = GY[r, f]; for MEAN GY[r, f] / float(d_r), one correctly rounded division BEFORE the weight
 *   a term    u_e = g[row_e, f], or with weighted != 0 w_e * g[row_e, f] rounded once to float32, never fused with the add.  For MAX
 *             and MIN u_e is that when e is the entry whose term the forward's fold kept for (row_e, f), and +0.0 otherwise
 *             (selected, not multiplied).  The winner is recomputed from X in the forward's order: the first of equal values wins, a
 *             leading NaN keeps the win, a later NaN never wins, a row without entries has none.
 *   the order L_c, the entries with col_e == c, in ASCENDING e (the forward's stored order), cut into segments of seg entries: within
 *             a segment acc = u_0, then acc = acc + u_j; the segments' values are added in segment order.  An empty L_c gives +0.0.
 * The gradient with respect to the edge weights is not built.
 * The transposed CSR (offsets, the forward row and the forward entry of every slot) is built on the device -- count by column, scan,
 * cursor fill, a segmented sort of every transposed row by entry, so that no result depends on the order in which atomics land --
 * by the first run on the out-rows and on the in-rows (kept for the handle's life, keyed by x_rows) and by every run on a block.
 * MGX_E_INVALID before any device work, the message names the parameter: everything mgx_agg_run refuses, for its counterparts (feats,
 * ldgy, ldgx, ldx with MAX / MIN, op, source, weighted without weights, in-rows without a CSC, the block, hop, x_rows below what the
 * columns name, NULL d_gy or d_gx), d_x NULL with MAX or MIN, any two of GY, X and GX overlapping.
 * stats (may be NULL), int64[10]: [0] transposed rows (x_rows), [1] entries, [2] feats, [3] team width G, [4] column tiles, [5] 1 on
 * the vector path (feats, ldgy, ldgx multiples of 4 and both bases 16-byte aligned), [6] seg, [7] launches (mgx_aggbwd_enact:
 * operator calls), [8] host waits, [9] 1 when this call built a transpose.  Launches and host waits of mgx_aggbwd_run, by case (L: 2
 * more launches where transposed rows are longer than seg; W: the winners' 1 launch, 3 where forward rows are longer than seg):
 *   repeat run on a kept transpose, SUM                                                 1 + L launches, 0 waits
 *   repeat run on a kept transpose, MEAN                                                2 + L launches, 0 waits (the division is a pass
 *       of its own that writes g = GY / d into a buffer of the handle's, R x feats)
 *   repeat run on a kept transpose, MAX or MIN                                          1 + L + W launches, 0 waits
 *   ... its first MAX or MIN on a source whose forward rows may be long                 + 2 launches, + 1 wait (the forward rows' plan)
 *   the run that builds (first on out-rows / in-rows; every run on a block)             + 10 + P launches, + 2 waits: count, scan, fill,
 *       the sort's classification and its three bands (each counted as run) and P = passes + (passes & 1) merge launches, with
 *       passes = ceil(log2(longest transposed row / 2048)) where one is longer than 2048, the slots' rows, the plan's two; the waits
 *       are the sort's and the plan's.  With fewer than 2 entries there is no sort (4 launches and 1 wait less), with none nothing.
 *   a block                                                                              as the run that builds: at most 3 waits
 *       (2, and the forward rows' plan for MAX / MIN where the sampling run had a fan-out of -1)
 * A repeat run on a kept transpose does no host wait and allocates nothing; every array lives on the handle and only grows.  A call
 * that is refused leaves no result: the getters return MGX_E_INVALID until a call succeeds. */
MGX_API int mgx_aggbwd_create(mgx_graph_t g, mgx_aggbwd_t* out);
MGX_API int mgx_aggbwd_free(mgx_aggbwd_t p);
/* the fused path: a team of lanes per transposed row, the loads of 8 slots in flight, no atomics on GX */
MGX_API int mgx_aggbwd_run(mgx_aggbwd_t p, int source, mgx_nsample_t block, int hop, const float* d_gy, int64_t ldgy, int feats, int op,
                           int weighted, const float* d_x, int64_t ldx, int64_t x_rows, float* d_gx, int64_t ldgx, int64_t* stats);
/* the operator path: one filter over GX's rows, a lane per transposed row (for MAX / MIN a filter over the forward rows first); the
 * same transposed arrays, the same bits */
MGX_API int mgx_aggbwd_enact(mgx_aggbwd_t p, int source, mgx_nsample_t block, int hop, const float* d_gy, int64_t ldgy, int feats, int op,
                             int weighted, const float* d_x, int64_t ldx, int64_t x_rows, float* d_gx, int64_t ldgx, int64_t* stats);
/* for callers with host arrays: mgx_aggbwd_upload copies host (rows x feats, contiguous) into the handle's array `which` (0: GY, 1:
 * X) and gives its device address; mgx_aggbwd_output gives a handle-owned device array of rows x ld floats to pass as d_gx.  They
 * grow only and stay valid until a larger request or free. */
MGX_API int mgx_aggbwd_upload(mgx_aggbwd_t p, int which, const float* host, int64_t rows, int feats, float** d_out);
MGX_API int mgx_aggbwd_output(mgx_aggbwd_t p, int64_t rows, int64_t ld, float** d_gx);
/* the last call's GX[:x_rows, :feats] to the host, contiguous, from wherever the call wrote it; waits */
MGX_API int mgx_aggbwd_result(mgx_aggbwd_t p, float* host_gx);
/* the transposed arrays the last call ran on, to the host (each may be NULL): offsets int32[x_rows + 1], rows int32[entries] (the
 * forward row of every slot, counted from the first selected row), pos int32[entries] (its forward entry, a place in the CSR's
 * columns); waits */
MGX_API int mgx_aggbwd_transpose(mgx_aggbwd_t p, int* offsets, int* rows, int* pos);
/* int64[5] of the last fused run, counted by its own launches (waits): [0] transposed rows without entries, [1] of at most seg
 * entries (a team's), [2] longer ones, [3] the segments of the latter, [4] seg */
MGX_API int mgx_aggbwd_bins(mgx_aggbwd_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_aggbwd_phase_ms gives out[5] = ms of the last fused run's transpose, winners,
 * rows, items and fold (waits for them) */
MGX_API int mgx_aggbwd_set_timing(mgx_aggbwd_t p, int on);
MGX_API int mgx_aggbwd_phase_ms(mgx_aggbwd_t p, double* out);

/* ---- vertex similarity for link prediction (include/mgx/sim_fused.hpp, include/gunrock/sim/) ----
 * How alike are two vertices' neighbourhoods, exactly, for arbitrary pairs.  The graph is the underlying simple undirected graph of
 * the triangle count: N(v) = the distinct neighbours of v other than v, original ids, d(v) = |N(v)|; symmetric as in mgx_tc_run.
 * A run takes `pairs` pairs (h_u[p], h_v[p]), host int32; both NULL selects EDGES MODE: the pairs are the simple graph's m_dag edges
 * in the order of mgx_ktruss_edges (`pairs` is ignored).  With c = |N(u) & N(v)|, common[p] = c (int32) always, and score[p]
 * (double) by `measure`:
 *   MGX_SIM_COMMON    c
 *   MGX_SIM_JACCARD   c / (d(u) + d(v) - c)        MGX_SIM_OVERLAP   c / min(d(u), d(v))
 *   MGX_SIM_SORENSEN  2 c / (d(u) + d(v))         MGX_SIM_COSINE    c / sqrt(d(u) d(v))          (each 0 where its denominator is 0)
 *   MGX_SIM_WEIGHTED  the sum of h_x[w] over the common neighbours w; h_x is a host double[n], required for this measure and read
 *                     by no other (Adamic-Adar: x = 1 / ln d, resource allocation: x = 1 / d; the caller builds x from
 *                     mgx_sim_degrees, no logarithm runs on the device)
 * u == v is legal (c = d(u)), duplicate pairs are legal, pairs == 0 is a valid run.  An id outside [0, n) is found on the device by
 * the classifying launch: the run returns MGX_E_INVALID and leaves no result.  The four ratios are one round-to-nearest division
 * of exact integers; the weighted sum uses no float atomics and a fixed reduction order: two runs are bit-equal, and (u, v) and
 * (v, u) score bit-equal (of two equally long rows the smaller id's plays the shorter).
 * stats (may be NULL), int64[8]: [0] pairs, [1] the sum of c, [2] pairs with c > 0, [3] adjacency entries (2 m_dag), [4] the longest
 * simple row, [5] 1 if this run built the adjacency, [6] host waits, [7] launches (mgx_sim_enact: two per operator call).  The
 * adjacency is built once per `symmetric` value and kept on the handle; a repeat run waits once, for its stats, and allocates
 * nothing while pairs does not exceed the largest seen. */
#define MGX_SIM_COMMON 0
#define MGX_SIM_JACCARD 1
#define MGX_SIM_OVERLAP 2
#define MGX_SIM_SORENSEN 3
#define MGX_SIM_COSINE 4
#define MGX_SIM_WEIGHTED 5
typedef struct mgx_sim_s* mgx_sim_t;
MGX_API int mgx_sim_create(mgx_graph_t g, mgx_sim_t* out);
MGX_API int mgx_sim_free(mgx_sim_t p);
/* builds the adjacency of `symmetric` unless the handle has it, so that mgx_sim_degrees can be read before a run */
MGX_API int mgx_sim_prepare(mgx_sim_t p, int symmetric);
/* the fused path: one classifying launch, four pair kernels by row lengths (a lane, a group of 16 lanes, a wave's LDS stage, a
 * workgroup's), one scoring launch; nothing is read back between them */
MGX_API int mgx_sim_run(mgx_sim_t p, int symmetric, const int* h_u, const int* h_v, int pairs, int measure, const double* h_x, int64_t* stats);
/* the operator path: one filter over the pair indices, a two-pointer merge per thread; the same results (WEIGHTED: within the
 * summation bound, its order is the merge's) */
MGX_API int mgx_sim_enact(mgx_sim_t p, int symmetric, const int* h_u, const int* h_v, int pairs, int measure, const double* h_x, int64_t* stats);
/* the last run's results to the host (stats [0] entries each); the device pointers stay valid until the next run or free */
MGX_API int mgx_sim_common(mgx_sim_t p, int* host);
MGX_API int mgx_sim_scores(mgx_sim_t p, double* host);
MGX_API int mgx_sim_common_device(mgx_sim_t p, const int** d_common);
MGX_API int mgx_sim_scores_device(mgx_sim_t p, const double** d_scores);
/* the last run's pairs (edges mode: the edges it generated); either may be NULL */
MGX_API int mgx_sim_pairs(mgx_sim_t p, int* h_u, int* h_v);
/* d(v) of the n vertices, of the adjacency the handle prepared or ran on last */
MGX_API int mgx_sim_degrees(mgx_sim_t p, int* host);
/* int64[10] of the last fused run: [0] - [4] pairs without a possible common neighbour (a row is empty) / a lane's / a group's / a
 * wave's / a workgroup's, [5] - [8] MGX_SIM_SHORT_MAX, _PROBE_RATIO, _WAVE_MAX and _STAGE as read, [9] the adjacency entries the
 * pair kernels loaded */
MGX_API int mgx_sim_bins(mgx_sim_t p, int64_t* out);
/* timing (measurement tools; off by default): mgx_sim_phase_ms gives out[3] = ms of the last fused run's build, classifying
 * launch and pair kernels (the scoring launch with them) */
MGX_API int mgx_sim_set_timing(mgx_sim_t p, int on);
MGX_API int mgx_sim_phase_ms(mgx_sim_t p, double* out);

/* ---- segmented sort (mgpu::segmented_sort, lspar_enactor.hxx:85; mgx/segsort.hpp) ----
 * Sorts d_keys[0, count) (and d_vals with them; NULL: keys only) in place, stably, ascending or descending, within segments:
 * d_segments holds num_segments heads, ascending, duplicates allowed; whatever lies before the first head is a segment too,
 * the last ends at count.  On the context's stream; returns when the sort is done. */
MGX_API int mgx_segmented_sort_i32(mgx_ctx_t ctx, int* d_keys, int* d_vals, int64_t count, const int* d_segments, int num_segments,
                                   int descending);

/* ---- synthetic input: counter-based R-MAT (the reference ships none, F4) ----
 * Writes edges [first_edge, first_edge+count) of the (scale, seed) stream to device arrays. */
MGX_API int mgx_rmat_edges(mgx_ctx_t ctx, int scale, int64_t first_edge, int64_t count, uint64_t seed,
                           int scramble, int* d_src, int* d_dst, float* d_weight);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H_ */
