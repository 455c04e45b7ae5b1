// mgx_capi.hip -- implementation of the C-ABI declared in include/mgx.h.
// Pre-instantiates the operator templates of include/gunrock/*.hxx for the in-scope functors (BFS, SSSP, PR, k-core, colouring,
// lspar, CC, TC, BC, PageRank, MST, random walks), exposes the building blocks and runs the fused paths of include/mgx/*_fused.hpp.
// Every algorithm's handle is an mgx_problem_s (its graph) plus what its two paths keep; the entry points share enter() (device
// and stream current, context and graph), create_handle / free_handle, require_run ("no run yet"), read_back (a result to the
// host) and put_stats.  Built with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Iinclude
// into mini_amd/libmgx.so (see __graft_entry__.build()).
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "gunrock/bc/bc_enactor.hxx"
#include "gunrock/bfs/bfs_enactor.hxx"
#include "gunrock/cc/cc_enactor.hxx"
#include "gunrock/coloring/coloring_enactor.hxx"
#include "gunrock/lspar/lspar_enactor.hxx"
#include "gunrock/ktruss/ktruss_enactor.hxx"
#include "gunrock/scc/scc_enactor.hxx"
#include "gunrock/louvain/louvain_enactor.hxx"
#include "gunrock/lpa/lpa_enactor.hxx"
#include "gunrock/msbfs/msbfs_enactor.hxx"
#include "gunrock/mst/mst_enactor.hxx"
#include "gunrock/pagerank/pagerank_enactor.hxx"
#include "gunrock/pr/pr_enactor.hxx"
#include "gunrock/nsample/nsample_enactor.hxx"
#include "gunrock/agg/agg_enactor.hxx"
#include "gunrock/aggbwd/aggbwd_enactor.hxx"
#include "gunrock/sim/sim_enactor.hxx"
#include "gunrock/rw/rw_enactor.hxx"
#include "gunrock/kcore/kcore_enactor.hxx"
#include "gunrock/sssp/sssp_enactor.hxx"
#include "gunrock/tc/tc_enactor.hxx"
#include "mgx/bc_fused.hpp"
#include "mgx/bfs_dist.hpp"
#include "mgx/bfs_dist2.hpp"
#include "mgx/cc_fused.hpp"
#include "mgx/kcore_fused.hpp"
#include "mgx/color_fused.hpp"
#include "mgx/lspar_fused.hpp"
#include "mgx/ktruss_fused.hpp"
#include "mgx/scc_fused.hpp"
#include "mgx/louvain_fused.hpp"
#include "mgx/lpa_fused.hpp"
#include "mgx/msbfs_fused.hpp"
#include "mgx/mst_fused.hpp"
#include "mgx/pagerank_fused.hpp"
#include "mgx/env.hpp"
#include "mgx/sssp_dist.hpp"
#include "mgx/rmat.hpp"
#include "mgx/nsample_fused.hpp"
#include "mgx/agg_backward.hpp"
#include "mgx/agg_fused.hpp"
#include "mgx/sim_fused.hpp"
#include "mgx/rw_fused.hpp"
#include "mgx/sssp_fused.hpp"
#include "mgx/sssp_preds.hpp"
#include "mgx/tc_fused.hpp"
#include "mgx.h"

using namespace gunrock;

// ------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------
struct mgx_ctx_s {
  int device;
  std::unique_ptr<standard_context_t> ctx;
};
struct mgx_graph_s {
  mgx_ctx_s* c;
  std::shared_ptr<graph_device_t> g;
  bool weights_checked = false;
  bool weights_ok = true;
  std::unique_ptr<mgx::modularity_state_t> mod;        // lazily: mgx_modularity's sums, kept for the next call on this graph
};
struct mgx_frontier_s {
  mgx_ctx_s* c;
  std::shared_ptr<frontier_t<int>> f;
};
// what every algorithm's handle starts with: the graph it was made for
struct mgx_problem_s {
  mgx_graph_s* g = nullptr;
  standard_context_t& ctx() const { return *g->c->ctx; }
  graph_device_t& graph() const { return *g->g; }
  size_t n() const { return (size_t)g->g->num_nodes; }
};
struct mgx_bfs_s : mgx_problem_s {
  std::shared_ptr<bfs::bfs_problem_t> p;
  std::unique_ptr<bfs::bfs_enactor_t> e;              // lazily: holds two m-capacity buffers
  std::unique_ptr<bfs::bfs_fused_enactor_t> fe;       // lazily: O(n)
  int64_t last_stats[24] = {0};
  mem_t<unsigned> visited_mask;                       // lazily: the idempotent mode's bitmask ((n + 31) / 32 words)
  int time_kernels = -1;                              // -1: environment default
};
struct mgx_sssp_s : mgx_problem_s {
  std::shared_ptr<sssp::sssp_problem_t> p;
  std::unique_ptr<sssp::sssp_enactor_t> e;
  float e_sizing = 0.f;
  std::unique_ptr<mgx::sssp_fused_state_t> fused;     // lazily: O(n)
  // predecessors of the fused loop's distances (mgx/sssp_preds.hpp): built when somebody asks for them
  mgx::sssp_pred_state_t pred_state;
  bool preds_stale = false;
  int preds_src = 0;
};
struct mgx_pr_s : mgx_problem_s {
  std::shared_ptr<pr::pr_problem_t> p;
  std::unique_ptr<pr::pr_enactor_t> e;
};
struct mgx_kcore_s : mgx_problem_s {
  std::shared_ptr<kcore::kcore_problem_t> p;
  std::unique_ptr<kcore::kcore_enactor_t> e;
  std::unique_ptr<mgx::kcore_fused_state_t> fused;                // lazily: the fused path's worklists and state words
};

struct mgx_color_s : mgx_problem_s {
  std::unique_ptr<mgx::color_fused_state_t> fused;                // lazily: the fused path's O(n) state
  std::shared_ptr<coloring::coloring_problem_t> p;                // lazily: the operator path's
  std::unique_ptr<coloring::coloring_enactor_t> e;
  const int* colors = nullptr;                                    // the last run's colours (nullptr: no run yet)
  std::vector<long long> trace;                                   // its active vertices per round
};

struct mgx_lspar_s : mgx_problem_s {
  std::unique_ptr<mgx::lspar_fused_state_t> fused;                // lazily: the fused path's state
  std::shared_ptr<lspar::lspar_problem_t> p;                      // lazily: the operator path's
  std::unique_ptr<lspar::lspar_enactor_t> e;
  // the last run's result (ro == nullptr: no run yet) and minhash table (n x mh_stride, k columns used)
  const int* ro = nullptr;
  const int* ci = nullptr;
  const int* eid = nullptr;
  const int* sim = nullptr;
  const unsigned* mh = nullptr;
  int mh_stride = 0, k = 0;
  long long kept = 0;
};

struct mgx_cc_s : mgx_problem_s {
  std::unique_ptr<mgx::cc_fused_state_t> fused;                   // lazily: the fused path's O(n + m / 32) state
  std::shared_ptr<cc::cc_problem_t> p;                            // lazily: the operator path's
  std::unique_ptr<cc::cc_enactor_t> e;
  std::unique_ptr<mgx::cc_label_stats_t> label_stats;             // lazily: the operator path's stats
  const int* labels = nullptr;                                    // the last run's labels (nullptr: no run yet)
};

struct mgx_tc_s : mgx_problem_s {
  std::unique_ptr<mgx::tc_state_t> st;                            // lazily: the DAGs (per `symmetric`), their work lists, tri
  std::shared_ptr<tc::tc_problem_t> p[2];                         // lazily: the operator path's view of dag[symmetric]
  std::unique_ptr<tc::tc_enactor_t> e;
};

struct mgx_bc_s : mgx_problem_s {
  std::unique_ptr<mgx::bc_state_t> st;                            // lazily: the row classes, the level lists, P / Q, sigma, delta, bc
  std::shared_ptr<bfs::bfs_problem_t> bp;                         // lazily: the traversal's labels (both paths write them)
  std::unique_ptr<bfs::bfs_fused_enactor_t> fe;                   // lazily: the fused path's traversal
  std::shared_ptr<bc::bc_problem_t> p;                            // lazily: the operator path's view of the same arrays
  std::unique_ptr<bc::bc_enactor_t> e;
  int last_sym = -1;                                              // `symmetric` of the last fused run (-1: none yet)
  int last_levels = 0;                                            // levels of the last source of the last run
};

struct mgx_pagerank_s : mgx_problem_s {
  std::shared_ptr<pagerank::pagerank_problem_t> p;                // lazily: the O(n) state both paths run on
  std::unique_ptr<pagerank::pagerank_enactor_t> e;                // lazily: the operator path's iota frontier
};

struct mgx_mst_s : mgx_problem_s {
  std::unique_ptr<mgx::mst_fused_state_t> fused;                  // lazily: the fused path's state and its sorted incident arrays
  std::shared_ptr<mst::mst_problem_t> p;                          // lazily: the operator path's
  std::unique_ptr<mst::mst_enactor_t> e;
  std::unique_ptr<mgx::cc_label_stats_t> label_stats;             // lazily: the operator path's stats
  mem_t<double> tile_sum;                                         // lazily: the operator path's list total
  mem_t<mgx::u64> stat;
  bool ready = false;                                             // a run of either path has left a result
  const int* labels = nullptr;
  const int* a = nullptr;
  const int* b = nullptr;
  const float* w = nullptr;
  long long edges = 0;
  double total = 0.0;
};

struct mgx_ktruss_s : mgx_problem_s {
  std::unique_ptr<mgx::ktruss_state_t> st;                        // lazily: the DAGs and adjacencies (per `symmetric`), the run's arrays
  std::shared_ptr<ktruss::ktruss_problem_t> p[2];                 // lazily: the operator path's view of them
  std::unique_ptr<ktruss::ktruss_enactor_t> e[2];
};

struct mgx_scc_s : mgx_problem_s {
  std::unique_ptr<mgx::scc_fused_state_t> fused;                  // lazily: the fused path's state, lists and state words
  std::unique_ptr<scc::scc_state_t> op_state;                     // lazily: the operator path's arrays, its two views of them
  std::shared_ptr<scc::scc_problem_t> fwd, bwd;
  std::unique_ptr<scc::scc_enactor_t> e;
  std::unique_ptr<mgx::cc_label_stats_t> label_stats;             // lazily: the operator path's stats
  const int* labels = nullptr;                                    // the last run's labels (nullptr: no run yet)
};

struct mgx_lpa_s : mgx_problem_s {
  std::unique_ptr<mgx::lpa_fused_state_t> fused;                  // lazily: the fused path's labels, lists and state words
  std::unique_ptr<lpa::lpa_state_t> op_state;                     // lazily: the operator path's arrays, its two views of them
  std::shared_ptr<lpa::lpa_problem_t> fwd, bwd;
  std::unique_ptr<lpa::lpa_enactor_t> e;
  std::unique_ptr<mgx::lpa_label_stats_t> label_stats;            // lazily: the operator path's stats
  const int* labels = nullptr;                                    // the last run's labels (nullptr: no run yet)
  bool last_fused = false;                                        // which path the trace is read from
};

struct mgx_msbfs_s : mgx_problem_s {
  std::unique_ptr<mgx::msbfs_fused_state_t> fused;                // lazily: the fused path's words, lists and state words
  std::unique_ptr<msbfs::msbfs_state_t> op_state;                 // lazily: the operator path's arrays
  std::shared_ptr<msbfs::msbfs_problem_t> p;
  msbfs::msbfs_problem_t::data_slice_t p_slice = {};              // what p points at
  std::unique_ptr<msbfs::msbfs_enactor_t> e;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's results; 2: the operator path's
  long long count = 0;                                            // sources of the last run
};

struct mgx_rw_s : mgx_problem_s {
  std::unique_ptr<mgx::rw_setup_state_t> setup;                   // lazily: the rows' maxima and the sorted copy, shared by both paths
  std::unique_ptr<mgx::rw_fused_state_t> fused;                   // lazily: the fused path's results
  std::unique_ptr<rw::rw_state_t> op_state;                       // lazily: the operator path's arrays
  std::shared_ptr<rw::rw_problem_t> p;
  std::unique_ptr<rw::rw_enactor_t> e;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's results; 2: the operator path's
  long long walkers = 0, length = 0;                              // of the last run
  bool kept_paths = false, kept_visits = false;
  bool timing = false;
};

struct mgx_nsample_s : mgx_problem_s {
  std::unique_ptr<mgx::ns_fused_state_t> fused;                   // lazily: the fused path's bitmaps, map and results
  std::unique_ptr<nsample::nsample_state_t> op_state;             // lazily: the operator path's arrays
  std::shared_ptr<nsample::nsample_problem_t> p;
  std::unique_ptr<nsample::nsample_enactor_t> e;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's results; 2: the operator path's
  bool timing = false;
};

struct mgx_sim_s : mgx_problem_s {
  std::unique_ptr<mgx::sim_state_t> st;                           // lazily: the adjacencies (per `symmetric`), the fused path's lists and results
  mgx::sim_results_t op_res;                                      // the operator path's pairs and results
  mem_t<unsigned long long> op_sums;
  std::shared_ptr<sim::sim_problem_t> p;
  std::unique_ptr<sim::sim_enactor_t> e;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's results; 2: the operator path's
  int sym = -1;                                                   // the adjacency prepared or run on last (-1: none yet)
  bool timing = false;
};

struct mgx_agg_s : mgx_problem_s {
  std::unique_ptr<mgx::agg_fused_state_t> fused;                  // lazily: the fused path's plans, partials and control words
  std::shared_ptr<agg::agg_problem_t> p;                          // lazily: the operator path's slice
  std::unique_ptr<agg::agg_enactor_t> e;
  mem_t<float> xbuf, ybuf;                                        // mgx_agg_upload's and mgx_agg_output's arrays, growing only
  size_t xcap = 0, ycap = 0;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's result; 2: the operator path's
  const float* last_y = nullptr;                                  // where the last run wrote: rows x feats, leading dimension ldy
  long long last_ldy = 0;
  int last_rows = 0, last_feats = 0;
  bool timing = false;
  int seg = 0;                                                    // MGX_AGG_SEG as read at the handle's first call, for both paths (0: not yet)
};

struct mgx_aggbwd_s : mgx_problem_s {
  std::unique_ptr<mgx::aggb_state_t> st;                          // lazily: the transposes, their plans, the winners, partials and control words
  std::shared_ptr<aggbwd::aggbwd_problem_t> p;                    // lazily: the operator path's slice
  std::unique_ptr<aggbwd::aggbwd_enactor_t> e;
  mem_t<float> inbuf[2], outbuf;                                  // mgx_aggbwd_upload's (GY, X) and mgx_aggbwd_output's arrays, growing only
  size_t incap[2] = {0, 0}, outcap = 0;
  int last = 0;                                                   // 0: no run yet; 1: the fused path's result; 2: the operator path's
  const float* last_gx = nullptr;                                 // where the last run wrote: rows x feats, leading dimension ldgx
  long long last_ldgx = 0;
  int last_rows = 0, last_feats = 0;
  bool timing = false;
};

struct mgx_louvain_s : mgx_problem_s {
  std::unique_ptr<mgx::louvain_fused_state_t> fused;              // lazily: the fused path's labels, tables, level graphs and state words
  std::unique_ptr<louvain::louvain_state_t> op_state;             // lazily: the operator path's arrays, its contraction, its stats
  std::unique_ptr<mgx::louvain_aggregate_t> op_agg;
  std::unique_ptr<louvain::louvain_enactor_t> e;
  std::unique_ptr<mgx::lpa_label_stats_t> label_stats;
  long long op_entries = 0;                                       // what op_state is sized for
  int last = 0;                                                   // 0: no result; 1: the fused path's; 2: the operator path's
};

struct mgx_dbfs_s {
  mgx_ctx_s* c;
  mgx::dbfs_state_t st;
};

struct mgx_dsssp_s {
  mgx_ctx_s* c;
  mgx::dsssp_state_t st;
  mgx::dsssp_run_bufs_t run_bufs;
};

struct mgx_dbfs2_s {
  mgx_ctx_s* c;
  mgx::d2_state_t st;
  mgx::d2_run_bufs_t run_bufs;
  mgx::d2_group_bufs_t group_bufs;     // (rank 0's handle holds the group run's shared buffers: mgx_dbfs2_run_group)
};
struct mgx_comm_s {
  mgx_ctx_s* c;
  mgx::comm_t cm;
};

static thread_local std::string g_last_error;

#define MGX_TRY try {
#define MGX_CATCH                                                  \
  }                                                                \
  catch (const mgx::mgx_error& e) {                                \
    g_last_error = e.what();                                       \
    return e.code;                                                 \
  }                                                                \
  catch (const mgx::hip_error& e) {                                \
    g_last_error = e.what();                                       \
    return MGX_E_HIP;                                              \
  }                                                                \
  catch (const std::exception& e) {                                \
    g_last_error = e.what();                                       \
    return MGX_E_INVALID;                                          \
  }                                                                \
  return MGX_OK;

#define MGX_REQUIRE(cond, msg)                                    \
  do {                                                             \
    if (!(cond)) throw mgx::mgx_error(MGX_E_INVALID, msg);         \
  } while (0)

// every entry point: the handle's device, and its stream as the one the context-less copies are ordered on
static inline void use_device(mgx_ctx_s* c) { MGX_HIP(hipSetDevice(c->device)); c->ctx->make_current(); }

// ---- what the algorithms' entry points share (the handles are mgx_problem_s) ----
// An entry point's prologue: the handle checked, its device and stream current; `auto [ctx, g] = enter(p);`
struct entered_t {
  standard_context_t& ctx;
  graph_device_t& g;
};
static entered_t enter(const mgx_problem_s* p) {
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  return {p->ctx(), p->graph()};
}
template <typename H>
static int create_handle(mgx_graph_t g, H** out) {
  MGX_TRY
  MGX_REQUIRE(g && out, "NULL argument");
  auto* h = new H();
  h->g = g;
  *out = h;
  MGX_CATCH
}
// Whatever the handle's last run enqueued on the context's stream is over before its memory goes.
template <typename H>
static int free_handle(H* p) {
  MGX_TRY
  if (p) { use_device(p->g->c); p->ctx().synchronize(); delete p; }
  MGX_CATCH
}
static void require_run(bool ran, const char* who) {
  if (!ran) throw mgx::mgx_error(MGX_E_INVALID, std::string(who) + ": no run yet");
}
// `count` values of a result to the host, behind a wait for the context's stream (the copy alone is ordered on that stream as
// well; of the two things the getters did the wait is the stricter one, and every getter does it now)
template <typename T>
static void read_back(const mgx_problem_s* p, T* host, const T* src, size_t count) {
  use_device(p->g->c);
  p->ctx().synchronize();
  if (count) MGX_HIP(mgx::dtoh(host, src, count));
}
// the `count` words an entry point's header promises, when the caller wants them (a run that returns another number of them
// is refused, not written past the caller's array)
static void put_stats(int64_t* stats, size_t count, const std::vector<long long>& v) {
  MGX_REQUIRE(v.size() == count, "internal: a run's stats do not have the size the header states");
  if (stats) std::copy(v.begin(), v.end(), stats);
}
// What the chains of launches (mgx/launch_chain.hpp) share at this boundary.  `state`: the handle's lazily made state; `ran`: its
// count of the last run's launches, below 0 while the log holds no run.
// the kinds of the last run's launches: all of them counted, the first min(cap, CHAIN_LOG_CAP) written
template <typename H, typename S>
static int chain_step_kinds(H* p, std::unique_ptr<S> H::*state, long long S::*ran, const char* who, int* host_kinds, int cap,
                            int64_t* launches) {
  MGX_TRY
  MGX_REQUIRE(p && launches && cap >= 0 && (host_kinds || cap == 0), "bad argument");
  const S* st = (p->*state).get();
  require_run(st && st->*ran >= 0, who);
  *launches = st->*ran;
  read_back(p, host_kinds, (const int*)st->ctl.data()->log, (size_t)std::min<long long>({st->*ran, (long long)cap, (long long)mgx::CHAIN_LOG_CAP}));
  MGX_CATCH
}
template <typename H, typename S>
static int chain_set_timing(H* p, std::unique_ptr<S> H::*state, int on) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  if (!(p->*state)) (p->*state).reset(new S(g.num_nodes, g.num_edges, ctx));
  (p->*state)->timing = on != 0;
  MGX_CATCH
}
template <typename H, typename S, int K>
static int chain_phase_ms(H* p, std::unique_ptr<S> H::*state, long long S::*ran, double (S::*ms)[K], const char* who, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  const S* st = (p->*state).get();
  require_run(st && st->*ran >= 0, who);
  std::copy(st->*ms, st->*ms + K, out);
  MGX_CATCH
}

// neighbourhood reduce with a plain per-vertex gather as the functor
namespace {
template <typename V>
struct gather_problem_t : problem_t {
  struct data_slice_t { const V* values; };
  mem_t<data_slice_t> d_data_slice;
  gather_problem_t(std::shared_ptr<graph_device_t> g, const V* values, standard_context_t& ctx) : problem_t(g) {
    std::vector<data_slice_t> h(1);
    h[0].values = values;
    d_data_slice = to_mem(h, ctx);
  }
};
template <typename V>
struct gather_functor_t {
  typedef typename gather_problem_t<V>::data_slice_t slice_t;
  static constexpr bool mgx_pure_gather = true;      // cond / apply are trivially true, the value is a pure read (neighborhood.hxx)
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, slice_t*, int) { return true; }
  static __device__ __forceinline__ V get_value_to_reduce(int idx, slice_t* d, int) { return d->values[idx]; }
};

extern "C" int mgx_nrs_build_device(const int* ro, const int* ci, int rows, unsigned slice_n, int slices, void** mu, unsigned** off,
                                    unsigned* first, long long* total, hipStream_t stream);   // mgx_layout.hip
// The long rows by slice of their destinations (mgx/nreduce.hpp: k_nrs_edges), once per graph at its first neighbour-reduce
// through the library: needs the layout with its degree classes (the long rows are [0, vs_v[0])); MGX_NR_SLICED=0 skips it.
// 16 bytes per mini-unit -- RMAT-22: 17.5 M of them, 280 MB -- and a partial per mini-unit in the context's arena; left out
// (the unit blocks serve) when the memory is not there.
static void ensure_nr_slices(mgx_graph_s* g) {
  graph_device_t& G = *g->g;
  if (G.nrs_tried) return;
  G.nrs_tried = true;
  if (const char* e = mgx::env("MGX_NR_SLICED")) if (atoi(e) == 0) return;
  if (!mgx::nr_units_valid(G) || G.rows.vs_v[0] == 0) return;                  // (no fast path on this graph, or no long rows)
  standard_context_t& ctx = *g->c->ctx;
  const unsigned S = (unsigned)mgx::NR_HOTV;
  const long long n = G.num_nodes;
  const int all = (int)std::min<long long>((n + S - 1) / S, (long long)mgx::NRS_MAX_SLICES);      // (slices the id range has)
  int slices = std::min(all, mgx::nrs_default_slices(n));
  if (const char* e = mgx::env("MGX_NR_SLICES")) { const int v = atoi(e); if (v >= 1) slices = std::min(v, all); }   // (tests: a tail on small graphs, many slices on mid-size ones)
  const int rows = (int)G.rows.vs_v[0];
  void* mu = nullptr;
  unsigned* off = nullptr;
  unsigned first[mgx::NRS_MAX_SLICES + 2] = {0};
  long long total = 0;
  ctx.synchronize();
  const int rc = mgx_nrs_build_device(G.d_layout_row_offsets.data(), G.d_layout_col_indices.data(), rows, S, slices, &mu, &off, first, &total,
                                      ctx.stream());
  // (the builder hands arrays back only when it succeeds with total > 0: NULL in both on every other way out)
  if (rc != 0) { (void)hipGetLastError(); return; }      // (the memory is not there: the unit blocks serve -- the call that asked is not failed for it)
  if (total <= 0 || !mu || !off) return;
  G.d_nrs_mu = mem_t<unsigned>::adopt((unsigned*)mu, ((size_t)total + 4) * 4);
  G.d_nrs_off = mem_t<unsigned>::adopt(off, (size_t)(slices + 1) * (size_t)rows + 1);
  // rows of more than NRS_BIG_DEG entries (the layout is sorted by degree: a prefix), from the first rows' offsets
  {
    std::vector<int> h((size_t)rows + 1);
    MGX_HIP(mgx::dtoh(h.data(), G.d_layout_row_offsets.data(), (size_t)rows + 1));
    auto first_at_most = [&](int d) {            // first row of at most d entries (degrees are non-increasing)
      size_t lo = 0, hi = (size_t)rows;
      while (lo < hi) { const size_t mid = (lo + hi) / 2; if (h[mid + 1] - h[mid] > d) lo = mid + 1; else hi = mid; }
      return (unsigned)lo;
    };
    int degs[3] = {mgx::NRS_FOLD_DEG[0], mgx::NRS_FOLD_DEG[1], mgx::NRS_FOLD_DEG[2]};
    if (const char* e = mgx::env("MGX_NR_FOLD_DEGS")) {            // (tests: every tier on small graphs)
      int d0 = 0, d1 = 0, d2 = 0;
      if (sscanf(e, "%d/%d/%d", &d0, &d1, &d2) == 3 && d0 >= d1 && d1 >= d2 && d2 >= 0) { degs[0] = d0; degs[1] = d1; degs[2] = d2; }
    }
    unsigned prev = 0;
    for (int i = 0; i < 3; ++i) { G.nrs_tier[i] = std::max(prev, first_at_most(degs[i])); prev = G.nrs_tier[i]; }
  }
  try {
    ctx.reserve_scratch(mgx::nr_scratch_bytes(G.num_nodes, total, 8));    // (a partial per mini-unit)
  } catch (const mgx::mgx_error&) {                                       // no room for the partials: give the slices back, the unit blocks serve
    (void)hipGetLastError();
    G.d_nrs_mu = mem_t<unsigned>();
    G.d_nrs_off = mem_t<unsigned>();
    return;
  }
  for (int k = 0; k < mgx::NRS_MAX_SLICES + 2; ++k) G.nrs_first[k] = k <= slices + 1 ? first[k] : first[slices + 1];
  G.nrs_slices = (unsigned)slices; G.nrs_rows = (unsigned)rows; G.nrs_units = total;
}

template <typename V, typename Op>
int segreduce_impl(mgx_graph_t g, mgx_frontier_t in, int push, const V* vals, V identity, V* reduced, int64_t* nz) {
  MGX_TRY
  MGX_REQUIRE(g && in && vals && reduced, "segreduce: NULL argument");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  if (in->f && (long long)in->f->size() * 8 >= (long long)g->g->num_nodes) ensure_nr_slices(g);     // (a full frontier, or a large ascending subset, may take mgx/nreduce.hpp)
  auto prob = std::make_shared<gather_problem_t<V>>(g->g, vals, ctx);
  std::shared_ptr<frontier_t<int>> dummy;
  int r;
  if (push)
    r = oprtr::neighborhood::neighborhood_kernel<gather_problem_t<V>, gather_functor_t<V>, V, Op, false, true>(
        prob, in->f, dummy, reduced, identity, 0, ctx);
  else
    r = oprtr::neighborhood::neighborhood_kernel<gather_problem_t<V>, gather_functor_t<V>, V, Op, false, false>(
        prob, in->f, dummy, reduced, identity, 0, ctx);
  ctx.synchronize();
  if (nz) *nz = r;
  MGX_CATCH
}
}  // namespace


extern "C" {

int mgx_version(void) { return 100; }

const char* mgx_strerror(int status) {
  switch (status) {
    case MGX_OK: return "ok";
    case MGX_E_INVALID: return "invalid argument";
    case MGX_E_HIP: return "HIP runtime error";
    case MGX_E_FRONTIER_OVERFLOW: return "frontier capacity overflow";
    case MGX_E_NEGATIVE_WEIGHT: return "negative edge weight";
    case MGX_E_NO_DEVICE: return "no HIP device";
    default: return "unknown status";
  }
}
const char* mgx_last_error(void) { return g_last_error.c_str(); }

// ---- context -------------------------------------------------------------------------------
int mgx_ctx_create(int device, void* stream, mgx_ctx_t* out) {
  MGX_TRY
  MGX_REQUIRE(out, "mgx_ctx_create: out is NULL");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    g_last_error = "no HIP device visible";
    return MGX_E_NO_DEVICE;
  }
  MGX_REQUIRE(device >= 0 && device < count, "mgx_ctx_create: device ordinal out of range");
  MGX_HIP(hipSetDevice(device));
  auto* c = new mgx_ctx_s();
  c->device = device;
  c->ctx.reset(new standard_context_t(false, (hipStream_t)stream));
  *out = c;
  MGX_CATCH
}
int mgx_ctx_set_stream(mgx_ctx_t c, void* stream) {
  MGX_TRY
  MGX_REQUIRE(c, "ctx is NULL");
  c->ctx->set_stream((hipStream_t)stream);
  MGX_CATCH
}
int mgx_ctx_synchronize(mgx_ctx_t c) {
  MGX_TRY
  MGX_REQUIRE(c, "ctx is NULL");
  use_device(c);
  c->ctx->synchronize();
  MGX_CATCH
}
int mgx_ctx_destroy(mgx_ctx_t c) {
  MGX_TRY
  if (c) { use_device(c); delete c; }
  MGX_CATCH
}
int mgx_ctx_num_cus(mgx_ctx_t c, int* out) {
  MGX_TRY
  MGX_REQUIRE(c && out, "NULL argument");
  *out = c->ctx->num_cus;
  MGX_CATCH
}

// ---- graph ---------------------------------------------------------------------------------
static void finish_graph(mgx_ctx_s* c, graph_device_t& g) {
  g.d_scanned_row_offsets = mem_t<int>((size_t)g.num_nodes + 1, *c->ctx);
  c->ctx->reserve_scratch((size_t)g.num_edges / 2 + ((size_t)g.num_nodes + 4096) * 2 + (1 << 20));
}

int mgx_graph_upload(mgx_ctx_t c, int n, int64_t m, const int* ro, const int* ci, const float* w, const int* co,
                     const int* ri, const float* rw, mgx_graph_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && ro && (ci || m == 0), "mgx_graph_upload: NULL argument");
  MGX_REQUIRE(n >= 0 && m >= 0 && m <= 2147483647LL, "mgx_graph_upload: sizes must fit int32 (graph.hxx:19-26)");
  MGX_REQUIRE((co == nullptr) == (ri == nullptr), "mgx_graph_upload: col_offsets and row_indices go together");
  // host arrays: cheap to validate (the kernels index with them unchecked)
  MGX_REQUIRE(ro[0] == 0 && (int64_t)ro[n] == m, "mgx_graph_upload: row_offsets must start at 0 and end at num_edges");
  for (int v = 0; v < n; ++v) MGX_REQUIRE(ro[v] <= ro[v + 1], "mgx_graph_upload: row_offsets must be non-decreasing");
  for (int64_t e = 0; e < m; ++e) MGX_REQUIRE(ci[e] >= 0 && ci[e] < n, "mgx_graph_upload: col_indices outside [0, num_nodes)");
  if (co) {
    MGX_REQUIRE(co[0] == 0 && (int64_t)co[n] == m, "mgx_graph_upload: col_offsets must start at 0 and end at num_edges");
    for (int v = 0; v < n; ++v) MGX_REQUIRE(co[v] <= co[v + 1], "mgx_graph_upload: col_offsets must be non-decreasing");
    for (int64_t e = 0; e < m; ++e) MGX_REQUIRE(ri[e] >= 0 && ri[e] < n, "mgx_graph_upload: row_indices outside [0, num_nodes)");
  }
  use_device(c);
  auto g = std::make_shared<graph_device_t>();
  g->num_nodes = n;
  g->num_edges = (int)m;
  g->d_row_offsets = mem_t<int>((size_t)n + 1, *c->ctx);
  MGX_HIP(mgx::htod(g->d_row_offsets.data(), ro, (size_t)n + 1));
  g->d_col_indices = mem_t<int>((size_t)m, *c->ctx);
  MGX_HIP(mgx::htod(g->d_col_indices.data(), ci, (size_t)m));
  if (w) {
    g->d_col_values = mem_t<float>((size_t)m, *c->ctx);
    MGX_HIP(mgx::htod(g->d_col_values.data(), w, (size_t)m));
  } else {
    g->d_col_values = mgx::fill(1.0f, (size_t)m, *c->ctx);
  }
  if (co) {
    g->d_col_offsets = mem_t<int>((size_t)n + 1, *c->ctx);
    MGX_HIP(mgx::htod(g->d_col_offsets.data(), co, (size_t)n + 1));
    g->d_row_indices = mem_t<int>((size_t)m, *c->ctx);
    MGX_HIP(mgx::htod(g->d_row_indices.data(), ri, (size_t)m));
    if (rw) {
      g->d_row_values = mem_t<float>((size_t)m, *c->ctx);
      MGX_HIP(mgx::htod(g->d_row_values.data(), rw, (size_t)m));
    } else {
      g->d_row_values = mgx::fill(1.0f, (size_t)m, *c->ctx);
    }
    g->csc_is_csr = false;
  } else {
    g->d_col_offsets = mem_t<int>::borrow(g->d_row_offsets.data(), g->d_row_offsets.size());
    g->d_row_indices = mem_t<int>::borrow(g->d_col_indices.data(), g->d_col_indices.size());
    g->d_row_values = mem_t<float>::borrow(g->d_col_values.data(), g->d_col_values.size());
    g->csc_is_csr = true;
  }
  finish_graph(c, *g);
  c->ctx->synchronize();
  auto* h = new mgx_graph_s();
  h->c = c;
  h->g = g;
  *out = h;
  MGX_CATCH
}

int mgx_graph_wrap_device(mgx_ctx_t c, int n, int64_t m, const int* ro, const int* ci, const float* w, const int* co,
                          const int* ri, const float* rw, mgx_graph_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && ro && (ci || m == 0), "mgx_graph_wrap_device: NULL argument");
  MGX_REQUIRE(n >= 0 && m >= 0 && m <= 2147483647LL, "mgx_graph_wrap_device: sizes must fit int32");
  MGX_REQUIRE((co == nullptr) == (ri == nullptr), "mgx_graph_wrap_device: col_offsets and row_indices go together");
  use_device(c);
  auto g = std::make_shared<graph_device_t>();
  g->num_nodes = n;
  g->num_edges = (int)m;
  g->d_row_offsets = mem_t<int>::borrow((int*)ro, (size_t)n + 1);
  g->d_col_indices = mem_t<int>::borrow((int*)ci, (size_t)m);
  if (w) g->d_col_values = mem_t<float>::borrow((float*)w, (size_t)m);
  else g->d_col_values = mgx::fill(1.0f, (size_t)m, *c->ctx);
  if (co) {
    g->d_col_offsets = mem_t<int>::borrow((int*)co, (size_t)n + 1);
    g->d_row_indices = mem_t<int>::borrow((int*)ri, (size_t)m);
    if (rw) g->d_row_values = mem_t<float>::borrow((float*)rw, (size_t)m);
    else g->d_row_values = mgx::fill(1.0f, (size_t)m, *c->ctx);
    g->csc_is_csr = false;
  } else {
    g->d_col_offsets = mem_t<int>::borrow(g->d_row_offsets.data(), (size_t)n + 1);
    g->d_row_indices = mem_t<int>::borrow(g->d_col_indices.data(), (size_t)m);
    g->d_row_values = mem_t<float>::borrow(g->d_col_values.data(), (size_t)m);
    g->csc_is_csr = true;
  }
  finish_graph(c, *g);
  c->ctx->synchronize();
  auto* h = new mgx_graph_s();
  h->c = c;
  h->g = g;
  *out = h;
  MGX_CATCH
}
static void build_unit_blocks(mgx_graph_s* g);
int mgx_graph_attach_layout(mgx_graph_t g, const int* d_row_offsets, const int* d_col_indices, const int* d_new_of_old,
                            const int* d_old_of_new) {
  MGX_TRY
  MGX_REQUIRE(g && d_row_offsets && (d_col_indices || g->g->num_edges == 0) && d_new_of_old && d_old_of_new,
              "mgx_graph_attach_layout: NULL argument");
  graph_device_t& G = *g->g;
  G.d_layout_row_offsets = mem_t<int>::borrow((int*)d_row_offsets, (size_t)G.num_nodes + 1);
  G.d_layout_col_indices = mem_t<int>::borrow((int*)d_col_indices, (size_t)G.num_edges);
  G.d_new_of_old = mem_t<int>::borrow((int*)d_new_of_old, (size_t)G.num_nodes);
  G.d_old_of_new = mem_t<int>::borrow((int*)d_old_of_new, (size_t)G.num_nodes);
  G.has_layout = true;
  mgx::row_layout_t& R = G.rows;
  R.vs_edges = 0; R.vs_dummy = 0; R.vs_long_min = 0;      // (borrowed arrays: no padding behind them, sortedness not checked)
  R.cold_owner = mem_t<int>(); R.cold_dst = mem_t<int>(); R.colds_owner = mem_t<int>(); R.colds_dst = mem_t<int>();
  R.cold_pk = mem_t<unsigned>(); R.cold_cbase = mem_t<unsigned>(); R.cold_pk_mask = 0;
  R.cold_pairs = R.colds_pairs = 0; R.cold_slices = 0;
  use_device(g->c);
  g->c->ctx->synchronize();
  build_unit_blocks(g);
  MGX_CATCH
}
int mgx_graph_attach_layout_weights(mgx_graph_t g, const float* d_layout_weights) {
  MGX_TRY
  MGX_REQUIRE(g && d_layout_weights, "mgx_graph_attach_layout_weights: NULL argument");
  MGX_REQUIRE(g->g->has_layout, "mgx_graph_attach_layout_weights: attach the layout first");
  graph_device_t& G = *g->g;
  G.d_layout_col_values = mem_t<float>::borrow((float*)d_layout_weights, (size_t)G.num_edges);
  G.has_layout_weights = true;
  MGX_CATCH
}
extern "C" int mgx_layout_build_device(const int* ro, const int* ci, const float* w, int n, long long m, int* lro, int* lci,
                                       float* lw, int* new_of_old, int* old_of_new, hipStream_t stream);   // mgx_layout.hip
// Unit blocks of the layout's long rows (mgx/bfs_fused_dense.hpp; built by mgx_layout.hip: mgx::build_unit_blocks).  The threshold is
// the fused traversal's long-row threshold at build time (MGX_BFS_LONG_MIN, default mgx::LONG_MIN_DEFAULT; a unit is 64 entries
// whatever the threshold); a run with another threshold ignores the blocks.
static void build_unit_blocks(mgx_graph_s* g) {
  graph_device_t& G = *g->g;
  mgx::row_layout_t& R = G.rows;
  R.ub = mgx::unit_blocks_t(); R.ub_min_degree = 0;
  G.nr_big_rows = 0; G.d_ub_w = mem_t<float>(); G.d_ub_w16 = mem_t<unsigned short>(); G.ub_w_tried = false;
  G.d_nrs_mu = mem_t<unsigned>(); G.d_nrs_off = mem_t<unsigned>(); G.nrs_units = 0; G.nrs_slices = G.nrs_rows = 0; G.nrs_tier[0] = G.nrs_tier[1] = G.nrs_tier[2] = 0; G.nrs_tried = false;
  int long_min = mgx::LONG_MIN_DEFAULT;
  if (const char* e = mgx::env("MGX_BFS_LONG_MIN")) long_min = atoi(e);
  if (long_min <= 0 || !G.has_layout || G.num_edges <= 0) return;
  // 24-bit copy for the fused BFS (ids below 2^23: bit 23 of an entry is free, so a sign-extending unpack turns 0xFFFFFF back into -1).
  // Round 6 (memory): every reader of the unit blocks takes the 24-bit copy when there is one -- the fused BFS, the neighbour-reduce,
  // the fused SSSP's sweep (with half or float weights) -- so the 32-bit entries go: 493 MB of RMAT-22's 2.03 GB of layout.
  // (MGX_BFS_PACK24=0 at layout time keeps them and builds no copy.)
  bool pack = (long long)G.num_nodes <= (1ll << 23);
  if (const char* e = mgx::env("MGX_BFS_PACK24")) pack = pack && atoi(e) != 0;
  mgx::build_unit_blocks(R.ub, G.d_layout_row_offsets.data(), G.d_layout_col_indices.data(), G.num_nodes, long_min, 0u, mgx::owner_remap_t(), true,
                         g->c->ctx->stream());
  if (R.ub.units <= 0) return;
  // the neighbour-reduce over the unit blocks (mgx/nreduce.hpp) keeps its values and per-unit partials in the context's arena
  g->c->ctx->reserve_scratch(mgx::nr_scratch_bytes(G.num_nodes, R.ub.units_pad, 8));
  R.ub_min_degree = long_min;
  if (pack) mgx::pack_unit_blocks24(R.ub, false, g->c->ctx->stream());
}
// Cold-edge lists of the layout (mgx/bfs_fused_cold.hpp); MGX_BFS_COLD_LISTS=0 skips them.  Needs the unit blocks and the
// degree classes (a degree-sorted layout: the long rows are [0, vs_v[0]), the short ones [vs_v[0], vs_v[3])); built only
// when the cold entries are a small share of the long rows' entries (a skewed graph under the hub-first order) and few
// slices hold any.  One list for the long rows, one for the short rows, the same slices.
static void build_cold_lists(mgx_graph_s* g) {
  graph_device_t& G = *g->g;
  mgx::row_layout_t& R = G.rows;
  R.cold_owner = mem_t<int>(); R.cold_dst = mem_t<int>(); R.colds_owner = mem_t<int>(); R.colds_dst = mem_t<int>();
  R.cold_pairs = R.colds_pairs = 0; R.cold_slices = 0; R.cold_hot_n = 0; R.cold_long_min = 0; R.cold_majority = false; R.cold_all = false;
  R.ubh = mgx::unit_blocks_t();
  // the short rows' list too on graphs of more than 2^23 vertices (equal to marking those entries on RMAT-22, where 6 % of the entries
  // are cold; RMAT-24 -2 %, RMAT-25 -9 % of a traversal); MGX_BFS_COLD_LISTS: 0 no lists at all, 1 the long rows' only, 2 both
  bool with_short = (long long)G.num_nodes > (1ll << 23);
  if (const char* e = mgx::env("MGX_BFS_COLD_LISTS")) {
    if (atoi(e) == 0) return;
    with_short = atoi(e) == 2;
  }
  if (R.ub.units <= 0 || R.vs_long_min <= 0 || R.vs_long_min != R.ub_min_degree || R.vs_v[0] == 0) return;
  const unsigned hot_n = (unsigned)mgx::BFS_COLD_WORDS * 32u, slice_n = hot_n;
  const unsigned n = (unsigned)G.num_nodes;
  if (n <= hot_n) return;                                          // everything is inside the prefix
  const long long slices_ll = ((long long)n - hot_n + slice_n - 1) / slice_n;
  if (slices_ll > 64) return;
  int slices = (int)slices_ll;
  unsigned list_hot_n = hot_n;          // first vertex the lists cover (0: a FLAT graph's lists hold every entry, below)
  bool flat = false;
  const int *ro = G.d_layout_row_offsets.data(), *ci = G.d_layout_col_indices.data();
  hipStream_t s = g->c->ctx->stream();
  std::vector<int> off_l;
  mem_t<int> d_owner, d_dst;
  long long pairs = mgx::build_cold_pairs(d_owner, d_dst, off_l, ro, ci, (int)n, 0, (int)R.vs_v[0], R.vs_long_min, hot_n, slice_n, slices, s);
  if (pairs <= 0) return;
  const long long long_entries = R.ub.units * 64;                  // (padded: an upper bound of the long rows' entries)
  if (pairs * 4 > long_entries) {
    // A FLAT graph (a uniform random graph: six entries in seven point behind the LDS prefix).  Round 5 left it to the bodies that PROBE
    // the bitmap in L2 -- 134 M probes at what the L2s deliver, 1.34 ms per RMAT-22-sized traversal, whatever the kernel around them
    // does.  Round 6: EVERY entry of every row as a pair by slice of its destination, slices from vertex 0 on (the first is the LDS
    // prefix itself); a level that holds an eighth of the graph's entries is then ONE sweep of the packed pairs by the cold-edge
    // pass's workgroups, each with its slice of the bitmap in LDS -- no probe leaves the compute unit, no mark is stored -- and the
    // other levels walk their queues and mark untested (few entries: few marks).  MGX_BFS_FLAT_LISTS=0: the probes, as in round 5.
    R.cold_majority = true;
    bool want = (long long)G.num_edges < (1ll << 31) - 512 && (n + (long long)slice_n - 1) / slice_n <= 64;
    if (const char* e = mgx::env("MGX_BFS_FLAT_LISTS")) want = want && atoi(e) != 0;
    if (!want || R.vs_v[3] == 0) return;
    slices = (int)((n + (long long)slice_n - 1) / slice_n);         // (the long rows' cold entries: superseded; no memory for 8 bytes per entry: the probes serve)
    pairs = mgx::build_cold_pairs(d_owner, d_dst, off_l, ro, ci, (int)n, 0, (int)R.vs_v[3], 1, 0u, slice_n, slices, s, true);
    if (pairs <= 0) return;
    list_hot_n = 0u; flat = true; with_short = false;
    R.cold_majority = false;
  }
  // the short rows' cold entries
  std::vector<int> off_s((size_t)slices + 1, 0);
  mem_t<int> d_owner_s, d_dst_s;
  long long pairs_s = 0;
  if (with_short && R.vs_v[3] > R.vs_v[0]) {
    pairs_s = mgx::build_cold_pairs(d_owner_s, d_dst_s, off_s, ro, ci, (int)n, (int)R.vs_v[0], (int)(R.vs_v[3] - R.vs_v[0]), 1, hot_n, slice_n, slices, s);
    if (pairs_s * 2 > (long long)R.vs_edges) { d_owner_s = mem_t<int>(); d_dst_s = mem_t<int>(); pairs_s = 0; }    // (mostly cold: leave them to the marks)
  }
  if (pairs_s <= 0) std::fill(off_s.begin(), off_s.end(), 0);
  // workgroups: one per 131 072 pairs, 64 .. 1024
  long long nwg = (pairs + pairs_s + 131071) / 131072;
  nwg = std::max<long long>(nwg, mgx::BFS_COLD_WGS);
  nwg = std::min<long long>(nwg, mgx::BFS_COLD_WGS_MAX);
  R.cold_owner = std::move(d_owner); R.cold_dst = std::move(d_dst); R.cold_pairs = pairs;
  R.colds_owner = std::move(d_owner_s); R.colds_dst = std::move(d_dst_s); R.colds_pairs = pairs_s;
  if (!mgx::cut_cold_lists(R, off_l, off_s, list_hot_n, slice_n, nwg, mgx::owner_remap_t(), true, s)) return;
  // Round 6 (memory): with EVERY slice packed nobody reads the 8-byte pairs of the long rows again (bfs_cold_body takes the packed
  // words slice by slice): they go -- 53 MB on RMAT-22.  (MGX_BFS_COLD_PACK=0 at layout time keeps them and packs nothing.)
  const int used = R.cold_slices;
  const unsigned long long every = used >= 64 ? ~0ull : ((1ull << used) - 1ull);
  if (R.cold_pk.size() && (R.cold_pk_mask & every) == every) {
    g->c->ctx->synchronize();
    R.cold_owner = mem_t<int>(); R.cold_dst = mem_t<int>();
  }
  R.cold_hot_n = list_hot_n; R.cold_long_min = R.vs_long_min;
  R.cold_all = flat;
  if (flat && (!R.cold_pk.size() || R.cold_owner.size())) {        // (a flat graph's lists are only worth their bytes when EVERY slice is packed: 4 per entry, what the CSR costs)
    R.cold_owner = mem_t<int>(); R.cold_dst = mem_t<int>(); R.cold_pk = mem_t<unsigned>(); R.cold_cbase = mem_t<unsigned>();
    R.cold_pairs = 0; R.cold_slices = 0; R.cold_all = false; R.cold_majority = true;
    return;
  }
  if (flat) return;                          // (no blocks "without the lists' entries": the lists hold everything)
  // The unit blocks once more for the fused BFS, WITHOUT the entries that now live in the lists (its unit-block body reads them only to
  // skip them) -- and what is left points into the LDS prefix, ids below 2^20: 24 bits per entry do at every graph size (the full
  // blocks' 24-bit copy stops at 2^23 vertices).  MGX_BFS_HOT_UNITS=0: not built.  The full blocks stay: the neighbour-reduce and the
  // fused SSSP read them, and so does a traversal that is told to run without the cold-edge pass.
  bool hot_units = true;
  if (const char* e = mgx::env("MGX_BFS_HOT_UNITS")) hot_units = atoi(e) != 0;
  if (const char* e = mgx::env("MGX_BFS_PACK24")) hot_units = hot_units && atoi(e) != 0;
  if (!hot_units) return;
  // Their ids lie below hot_n = 652 288 < 2^20 - 1: 20 bits per entry (mgx/pack20.hpp) INSTEAD of 24 -- a sixth off the stream that
  // dominates the push kernel and off the blocks' memory.  MGX_BFS_PACK20=0: 24 bits, as before.
  bool pack20 = hot_n < 0xFFFFFu;
  if (const char* e = mgx::env("MGX_BFS_PACK20")) pack20 = pack20 && atoi(e) != 0;
  mgx::build_unit_blocks(R.ubh, ro, ci, G.num_nodes, R.vs_long_min, hot_n, mgx::owner_remap_t(), false, s);
  if (R.ubh.units > 0) {
    if (pack20) mgx::pack_unit_blocks20(R.ubh, s);
    else mgx::pack_unit_blocks24(R.ubh, false, s);
  }
}
int mgx_graph_build_layout(mgx_graph_t g, int with_weights) {
  MGX_TRY
  MGX_REQUIRE(g, "graph is NULL");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  graph_device_t& G = *g->g;
  const size_t n = (size_t)G.num_nodes, m = (size_t)G.num_edges;
  MGX_REQUIRE(!with_weights || G.d_col_values.size() >= m, "mgx_graph_build_layout: the graph has no weights");
  ctx.synchronize();
  mem_t<int> lro(n + 1, ctx), lci(m + 8, ctx), n2o(n, ctx), o2n(n, ctx);     // (+8: slack and four -1 for bfs_fused_vshort.hpp)
  MGX_HIP(hipMemsetAsync(lci.data() + m, 0xFF, 8 * sizeof(int), ctx.stream()));
  mem_t<float> lw;
  if (with_weights) lw = mem_t<float>(m + 8, ctx);          // (+8: the short rows' 16-byte weight loads of sssp_dense_short may reach past the last entry)
  const int rc = mgx_layout_build_device(G.d_row_offsets.data(), G.d_col_indices.data(),
                                         with_weights ? G.d_col_values.data() : (const float*)nullptr, (int)n, (long long)m,
                                         lro.data(), lci.data(), with_weights ? lw.data() : (float*)nullptr, n2o.data(),
                                         o2n.data(), ctx.stream());
  if (rc != 0) throw mgx::mgx_error(MGX_E_HIP, std::string("mgx_graph_build_layout: ") + hipGetErrorString((hipError_t)rc));
  G.d_layout_row_offsets = std::move(lro);
  G.d_layout_col_indices = std::move(lci);
  G.d_new_of_old = std::move(n2o);
  G.d_old_of_new = std::move(o2n);
  G.has_layout = true;
  if (with_weights) { G.d_layout_col_values = std::move(lw); G.has_layout_weights = true; }
  build_unit_blocks(g);
  // degree classes of the short rows (the layout is sorted by degree): boundaries by binary search on a host copy
  mgx::row_layout_t& R = G.rows;
  R.vs_edges = 0; R.vs_dummy = 0; R.vs_long_min = 0;
  {
    int long_min = mgx::LONG_MIN_DEFAULT;
    if (const char* e = mgx::env("MGX_BFS_LONG_MIN")) long_min = atoi(e);
    if (long_min > 0 && long_min <= 64 && n > 0 && m > 0) {
      std::vector<int> h(n + 1);
      MGX_HIP(mgx::dtoh(h.data(), G.d_layout_row_offsets.data(), n + 1));
      mgx::cut_degree_classes(R, h, n, long_min);
      G.nr_big_rows = mgx::first_row_below(h, n, 64 * mgx::NR_BIG_UNITS + 1);       // rows of more than NR_BIG_UNITS units (mgx/nreduce.hpp)
      R.vs_dummy = (unsigned)m + 4u;
      R.vs_long_min = long_min;
    }
  }
build_cold_lists(g);
  // (the sources' shapes -- mgx/src_shapes.hpp -- are resolved per call since round 6; what the cache held belongs to the old layout's threshold)
  G.src_shape_cache.clear();
  G.src_shapes_enabled = true;
  MGX_CATCH
}
extern "C" int mgx_csc_build_device(const int* ro, const int* ci, const float* w, int n, long long m, int* co, int* ri, float* rv,
                                    hipStream_t stream);   // mgx_layout.hip
int mgx_graph_build_csc(mgx_graph_t g) {
  MGX_TRY
  MGX_REQUIRE(g, "graph is NULL");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  graph_device_t& G = *g->g;
  const size_t n = (size_t)G.num_nodes, m = (size_t)G.num_edges;
  ctx.synchronize();
  mem_t<int> co(n + 1, ctx), ri(m, ctx);
  mem_t<float> rv(m, ctx);
  const int rc = mgx_csc_build_device(G.d_row_offsets.data(), G.d_col_indices.data(), G.d_col_values.data(), (int)n, (long long)m,
                                      co.data(), ri.data(), rv.data(), ctx.stream());
  if (rc != 0) throw mgx::mgx_error(MGX_E_HIP, std::string("mgx_graph_build_csc: ") + hipGetErrorString((hipError_t)rc));
  G.d_col_offsets = std::move(co);
  G.d_row_indices = std::move(ri);
  G.d_row_values = std::move(rv);
  G.csc_is_csr = false;
  MGX_CATCH
}
int mgx_graph_csc_read(mgx_graph_t g, int* h_col_offsets, int* h_row_indices, float* h_row_values) {
  MGX_TRY
  MGX_REQUIRE(g, "graph is NULL");
  use_device(g->c);
  g->c->ctx->synchronize();
  graph_device_t& G = *g->g;
  const size_t n = (size_t)G.num_nodes, m = (size_t)G.num_edges;
  if (h_col_offsets) MGX_HIP(mgx::dtoh(h_col_offsets, G.d_col_offsets.data(), n + 1));
  if (h_row_indices && m) MGX_HIP(mgx::dtoh(h_row_indices, G.d_row_indices.data(), m));
  if (h_row_values && m) MGX_HIP(mgx::dtoh(h_row_values, G.d_row_values.data(), m));
  MGX_CATCH
}
int mgx_graph_layout_info(mgx_graph_t g, int64_t* out8) {
  MGX_TRY
  MGX_REQUIRE(g && out8, "NULL argument");
  const graph_device_t& G = *g->g;
  for (int i = 0; i < 8; ++i) out8[i] = 0;
  if (!G.has_layout) return MGX_OK;
  out8[0] = 1;
  const mgx::row_layout_t& R = G.rows;
  out8[1] = (int64_t)R.ub.units;
  out8[2] = R.ub.col24.size() ? 1 : 0;
  out8[3] = (int64_t)R.cold_pairs;
  out8[4] = (int64_t)R.cold_slices;
  out8[5] = (int64_t)R.ubh.units;
  out8[6] = R.cold_majority ? 1 : 0;
  auto bytes = [](auto& m) -> int64_t { return m.owned() ? (int64_t)(m.size() * sizeof(*m.data())) : 0; };
  out8[7] = bytes(G.d_layout_row_offsets) + bytes(G.d_layout_col_indices) + bytes(G.d_layout_col_values) + bytes(G.d_new_of_old) + bytes(G.d_old_of_new) +
            bytes(R.ub.col) + bytes(R.ub.col24) + bytes(R.ub.owner) + bytes(R.ubh.col24) + bytes(R.ubh.col20) + bytes(R.ubh.owner) + bytes(G.d_ub_w) + bytes(G.d_ub_w16) +
            bytes(R.ub.cnt) + bytes(R.ub.first) + bytes(R.cold_owner) + bytes(R.cold_dst) + bytes(R.cold_pk) + bytes(R.cold_cbase) +
            bytes(R.colds_owner) + bytes(R.colds_dst) + bytes(G.d_nrs_mu) + bytes(G.d_nrs_off) + bytes(G.d_nr_pos);
  MGX_CATCH
}
int mgx_graph_nr_slices_info(mgx_graph_t g, int64_t* out5) {
  MGX_TRY
  MGX_REQUIRE(g && out5, "NULL argument");
  const graph_device_t& G = *g->g;
  out5[0] = (int64_t)G.nrs_units;
  out5[1] = (int64_t)G.nrs_slices;
  out5[2] = (int64_t)G.nrs_rows;
  out5[3] = (int64_t)G.nrs_tier[2];
  out5[4] = G.nrs_units > 0 ? (int64_t)(G.nrs_first[G.nrs_slices + 1] - G.nrs_first[G.nrs_slices]) : 0;
  MGX_CATCH
}
int mgx_graph_nr_last_call(mgx_graph_t g, int64_t* out4) {
  MGX_TRY
  MGX_REQUIRE(g && out4, "NULL argument");
  const auto& last = g->c->ctx->nr_last_call;
  MGX_REQUIRE(last.valid, "mgx_graph_nr_last_call: no neighbourhood reduce on this context yet");
  out4[0] = last.body; out4[1] = last.frontier; out4[2] = last.rejected; out4[3] = (int64_t)last.edges;
  MGX_CATCH
}
int mgx_graph_layout_read(mgx_graph_t g, int* h_row_offsets, int* h_col_indices, int* h_new_of_old, int* h_old_of_new,
                          float* h_weights) {
  MGX_TRY
  MGX_REQUIRE(g, "graph is NULL");
  MGX_REQUIRE(g->g->has_layout, "mgx_graph_layout_read: the graph has no layout");
  use_device(g->c);
  g->c->ctx->synchronize();
  graph_device_t& G = *g->g;
  const size_t n = (size_t)G.num_nodes, m = (size_t)G.num_edges;
  if (h_row_offsets) MGX_HIP(mgx::dtoh(h_row_offsets, G.d_layout_row_offsets.data(), n + 1));
  if (h_col_indices && m) MGX_HIP(mgx::dtoh(h_col_indices, G.d_layout_col_indices.data(), m));
  if (h_new_of_old) MGX_HIP(mgx::dtoh(h_new_of_old, G.d_new_of_old.data(), n));
  if (h_old_of_new) MGX_HIP(mgx::dtoh(h_old_of_new, G.d_old_of_new.data(), n));
  if (h_weights && m) {
    MGX_REQUIRE(G.has_layout_weights, "mgx_graph_layout_read: the layout carries no weights");
    MGX_HIP(mgx::dtoh(h_weights, G.d_layout_col_values.data(), m));
  }
  MGX_CATCH
}
int mgx_graph_free(mgx_graph_t g) {
  MGX_TRY
  if (g) { use_device(g->c); delete g; }
  MGX_CATCH
}
int mgx_graph_dims(mgx_graph_t g, int* n, int64_t* m) {
  MGX_TRY
  MGX_REQUIRE(g, "graph is NULL");
  if (n) *n = g->g->num_nodes;
  if (m) *m = g->g->num_edges;
  MGX_CATCH
}

int mgx_load_mtx(const char* path, int undir, int random_w, int* n, int64_t* m, int** ro, int** ci, float** w) {
  MGX_TRY
  MGX_REQUIRE(path && n && m && ro && ci && w, "mgx_load_mtx: NULL argument");
  auto g = load_graph(path, undir != 0, random_w != 0);
  MGX_REQUIRE(g != nullptr, std::string("mgx_load_mtx: cannot read ") + path);
  *n = g->num_nodes;
  *m = g->num_edges;
  *ro = (int*)malloc(((size_t)g->num_nodes + 1) * sizeof(int));
  *ci = (int*)malloc(((size_t)g->num_edges + 1) * sizeof(int));
  *w = (float*)malloc(((size_t)g->num_edges + 1) * sizeof(float));
  memcpy(*ro, g->csr->offsets.data(), ((size_t)g->num_nodes + 1) * sizeof(int));
  memcpy(*ci, g->csr->indices.data(), (size_t)g->num_edges * sizeof(int));
  memcpy(*w, g->csr->edge_weights.data(), (size_t)g->num_edges * sizeof(float));
  MGX_CATCH
}
int mgx_load_mtx_csc(const char* path, int undir, int random_w, int genuine_csc, int* n, int64_t* m, int** ro, int** ci,
                     float** w, int** co, int** ri, float** rw) {
  MGX_TRY
  MGX_REQUIRE(path && n && m && ro && ci && w && co && ri && rw, "mgx_load_mtx_csc: NULL argument");
  auto g = load_graph(path, undir != 0, random_w != 0, genuine_csc != 0);
  MGX_REQUIRE(g != nullptr, std::string("mgx_load_mtx_csc: cannot read ") + path);
  *n = g->num_nodes;
  *m = g->num_edges;
  const size_t N = (size_t)g->num_nodes, M = (size_t)g->num_edges;
  auto dup_i = [](const std::vector<int>& v, size_t cnt) { int* p = (int*)malloc((cnt + 1) * sizeof(int)); memcpy(p, v.data(), cnt * sizeof(int)); return p; };
  auto dup_f = [](const std::vector<float>& v, size_t cnt) { float* p = (float*)malloc((cnt + 1) * sizeof(float)); memcpy(p, v.data(), cnt * sizeof(float)); return p; };
  *ro = dup_i(g->csr->offsets, N + 1); *ci = dup_i(g->csr->indices, M); *w = dup_f(g->csr->edge_weights, M);
  *co = dup_i(g->csc->offsets, N + 1); *ri = dup_i(g->csc->indices, M); *rw = dup_f(g->csc->edge_weights, M);
  MGX_CATCH
}
// binary CSR cache (include/gunrock/graph.hxx: save_graph_cache / load_graph_cache)
int mgx_graph_save_csr(const char* path, int num_nodes, int64_t num_edges, int undirected, const int* ro, const int* ci,
                       const float* w, const int* co, const int* ri, const float* rw) {
  MGX_TRY
  MGX_REQUIRE(path && ro && (ci || num_edges == 0) && num_nodes >= 0 && num_edges >= 0 && num_edges <= 2147483647LL,
              "mgx_graph_save_csr: bad argument");
  MGX_REQUIRE((co == nullptr) == (ri == nullptr), "mgx_graph_save_csr: col_offsets and row_indices go together");
  graph_t g;
  g.num_nodes = num_nodes; g.num_edges = (int)num_edges; g.undirected = undirected != 0;
  auto mk = [&](const int* o, const int* i, const float* v) {
    auto c = std::make_shared<csr_t>();
    c->num_nodes = num_nodes; c->num_edges = (int)num_edges;
    c->offsets.assign(o, o + num_nodes + 1);
    c->indices.assign(i, i + num_edges);
    if (v) c->edge_weights.assign(v, v + num_edges); else c->edge_weights.assign((size_t)num_edges, 1.0f);
    return c;
  };
  g.csr = mk(ro, ci, w);
  g.csc = co ? mk(co, ri, rw) : g.csr;
  MGX_REQUIRE(save_graph_cache(path, g), std::string("mgx_graph_save_csr: cannot write ") + path);
  MGX_CATCH
}
int mgx_graph_load_csr(const char* path, int* n, int64_t* m, int* undirected, int** ro, int** ci, float** w, int** co, int** ri,
                       float** rw) {
  MGX_TRY
  MGX_REQUIRE(path && n && m && ro && ci && w, "mgx_graph_load_csr: NULL argument");
  auto g = load_graph_cache(path);
  MGX_REQUIRE(g != nullptr, std::string("mgx_graph_load_csr: not a valid CSR cache (missing, truncated, or checksum mismatch): ") + path);
  *n = g->num_nodes; *m = g->num_edges;
  if (undirected) *undirected = g->undirected ? 1 : 0;
  const size_t N = (size_t)g->num_nodes, M = (size_t)g->num_edges;
  auto dup_i = [](const std::vector<int>& v, size_t cnt) { int* p = (int*)malloc((cnt + 1) * sizeof(int)); memcpy(p, v.data(), cnt * sizeof(int)); return p; };
  auto dup_f = [](const std::vector<float>& v, size_t cnt) { float* p = (float*)malloc((cnt + 1) * sizeof(float)); memcpy(p, v.data(), cnt * sizeof(float)); return p; };
  *ro = dup_i(g->csr->offsets, N + 1); *ci = dup_i(g->csr->indices, M); *w = dup_f(g->csr->edge_weights, M);
  const bool has_csc = g->csc != g->csr;
  if (co) *co = has_csc ? dup_i(g->csc->offsets, N + 1) : nullptr;
  if (ri) *ri = has_csc ? dup_i(g->csc->indices, M) : nullptr;
  if (rw) *rw = has_csc ? dup_f(g->csc->edge_weights, M) : nullptr;
  MGX_CATCH
}
void mgx_host_free(void* p) { free(p); }

// ---- frontier ------------------------------------------------------------------------------
int mgx_frontier_create(mgx_ctx_t c, int64_t capacity, mgx_frontier_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && capacity >= 0, "mgx_frontier_create: bad argument");
  use_device(c);
  auto* h = new mgx_frontier_s();
  h->c = c;
  h->f = std::make_shared<frontier_t<int>>(*c->ctx, (size_t)capacity);
  *out = h;
  MGX_CATCH
}
int mgx_frontier_free(mgx_frontier_t f) {
  MGX_TRY
  if (f) { use_device(f->c); delete f; }
  MGX_CATCH
}
int mgx_frontier_load(mgx_frontier_t f, const int* host, int64_t n) {
  MGX_TRY
  MGX_REQUIRE(f && (host || n == 0) && n >= 0, "mgx_frontier_load: bad argument");
  use_device(f->c);
  f->f->resize((size_t)n);   // throws MGX_E_FRONTIER_OVERFLOW
  mgx::frontier_touched();
  MGX_HIP(mgx::htod(f->f->data()->data(), host, (size_t)n));
  MGX_CATCH
}
int mgx_frontier_fill_iota(mgx_frontier_t f, int64_t n) {
  MGX_TRY
  MGX_REQUIRE(f && n >= 0, "mgx_frontier_fill_iota: bad argument");
  use_device(f->c);
  f->f->resize((size_t)n);
  mgx::frontier_touched();
  int* p = f->f->data()->data();
  mgx::transform([=] __device__(int i) { p[i] = i; }, n, *f->c->ctx);
  MGX_CATCH
}
int mgx_frontier_fill(mgx_frontier_t f, int value, int64_t n) {
  MGX_TRY
  MGX_REQUIRE(f && n >= 0, "mgx_frontier_fill: bad argument");
  use_device(f->c);
  f->f->resize((size_t)n);
  mgx::frontier_touched();
  int* p = f->f->data()->data();
  mgx::transform([=] __device__(int i) { p[i] = value; }, n, *f->c->ctx);
  MGX_CATCH
}
int mgx_frontier_read(mgx_frontier_t f, int* host, int64_t cap, int64_t* n) {
  MGX_TRY
  MGX_REQUIRE(f && n, "mgx_frontier_read: bad argument");
  use_device(f->c);
  f->c->ctx->synchronize();
  *n = (int64_t)f->f->size();
  if (host) {
    MGX_REQUIRE(cap >= *n, "mgx_frontier_read: host buffer too small");
    MGX_HIP(mgx::dtoh(host, f->f->data()->data(), f->f->size()));
  }
  MGX_CATCH
}
int mgx_frontier_resize(mgx_frontier_t f, int64_t n) {
  MGX_TRY
  MGX_REQUIRE(f && n >= 0, "mgx_frontier_resize: bad argument");
  f->f->resize((size_t)n);
  MGX_CATCH
}
int mgx_frontier_size(mgx_frontier_t f, int64_t* n) {
  MGX_TRY
  MGX_REQUIRE(f && n, "NULL argument");
  *n = (int64_t)f->f->size();
  MGX_CATCH
}
int mgx_frontier_capacity(mgx_frontier_t f, int64_t* n) {
  MGX_TRY
  MGX_REQUIRE(f && n, "NULL argument");
  *n = (int64_t)f->f->capacity();
  MGX_CATCH
}
int mgx_frontier_device_ptr(mgx_frontier_t f, int** p) {
  MGX_TRY
  MGX_REQUIRE(f && p, "NULL argument");
  *p = f->f->data()->data();
  f->f->mark_exposed();
  MGX_CATCH
}

// ---- building blocks -----------------------------------------------------------------------
int mgx_scan_exclusive_i32(mgx_ctx_t c, const int* d_in, int64_t n, int* d_out, int64_t* total) {
  MGX_TRY
  MGX_REQUIRE(c && (d_in || n == 0) && (d_out || n == 0) && n >= 0, "mgx_scan_exclusive_i32: bad argument");
  use_device(c);
  c->ctx->reserve_scratch(mgx::scan_scratch_bytes(n));
  long long t = 0;
  mgx::transform_scan([=] __device__(long long i) { return d_in[i]; }, n, d_out, *c->ctx, &t);
  if (total) *total = t;
  MGX_CATCH
}

int mgx_scan_frontier_degrees(mgx_graph_t g, mgx_frontier_t in, int use_csc, int64_t* total) {
  MGX_TRY
  MGX_REQUIRE(g && in, "NULL argument");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  g->g->ensure_scanned(in->f->capacity(), ctx);
  const int* input_data = in->f->data()->data();
  const int* offsets = use_csc ? g->g->d_col_offsets.data() : g->g->d_row_offsets.data();
  long long t = 0;
  mgx::transform_scan(
      [=] __device__(long long i) {
        const int v = input_data[i];
        return offsets[v + 1] - offsets[v];
      },
      (long long)in->f->size(), g->g->d_scanned_row_offsets.data(), ctx, &t);
  if (total) *total = t;
  MGX_CATCH
}

int mgx_lbs_expand_debug(mgx_graph_t g, mgx_frontier_t in, int64_t total, int* host_seg, int* host_rank) {
  MGX_TRY
  MGX_REQUIRE(g && in && total >= 0 && (total == 0 || (host_seg && host_rank)), "bad argument");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  if (total == 0) return MGX_OK;
  mem_t<int> seg((size_t)total, ctx), rank((size_t)total, ctx);
  int* ps = seg.data();
  int* pr = rank.data();
  mgx::transform_lbs([=] __device__(int idx, int s, int r) { ps[idx] = s; pr[idx] = r; }, total,
                     g->g->d_scanned_row_offsets.data(), (long long)in->f->size(), ctx);
  ctx.synchronize();
  MGX_HIP(mgx::dtoh(host_seg, ps, (size_t)total));
  MGX_HIP(mgx::dtoh(host_rank, pr, (size_t)total));
  MGX_CATCH
}

int mgx_compact_i32(mgx_ctx_t c, const int* d_in, int64_t n, int drop_value, int* d_out, int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(c && (d_in || n == 0) && n >= 0, "mgx_compact_i32: bad argument");
  use_device(c);
  c->ctx->reserve_scratch(mgx::scan_scratch_bytes(n));
  auto compact = mgx::transform_compact(n, *c->ctx);
  const long long k = compact.upsweep([=] __device__(long long i) { return d_in[i] != drop_value; });
  compact.downsweep([=] __device__(long long d, long long s) { d_out[d] = d_in[s]; });
  c->ctx->synchronize();
  if (kept) *kept = k;
  MGX_CATCH
}

int mgx_segreduce_f32_plus(mgx_graph_t g, mgx_frontier_t in, int push, const float* v, float id, float* red,
                           int64_t* nz) {
  return segreduce_impl<float, mgx::plus_t<float>>(g, in, push, v, id, red, nz);
}
int mgx_segreduce_i32_min(mgx_graph_t g, mgx_frontier_t in, int push, const int* v, int id, int* red, int64_t* nz) {
  return segreduce_impl<int, mgx::minimum_t<int>>(g, in, push, v, id, red, nz);
}
int mgx_segreduce_i32_max(mgx_graph_t g, mgx_frontier_t in, int push, const int* v, int id, int* red, int64_t* nz) {
  return segreduce_impl<int, mgx::maximum_t<int>>(g, in, push, v, id, red, nz);
}

// ---- BFS -----------------------------------------------------------------------------------
static bfs::bfs_enactor_t& bfs_enactor(mgx_bfs_t p) {
  if (!p->e) p->e.reset(new bfs::bfs_enactor_t(*p->g->c->ctx, p->g->g->num_nodes, p->g->g->num_edges));
  return *p->e;
}

int mgx_bfs_create(mgx_graph_t g, int src, mgx_bfs_t* out) {
  MGX_TRY
  MGX_REQUIRE(g && out, "NULL argument");
  MGX_REQUIRE(src >= 0 && src < g->g->num_nodes, "mgx_bfs_create: src out of range");
  use_device(g->c);
  auto* h = new mgx_bfs_s();
  h->g = g;
  h->p = std::make_shared<bfs::bfs_problem_t>(g->g, (size_t)src, *g->c->ctx);
  *out = h;
  MGX_CATCH
}
int mgx_bfs_reset(mgx_bfs_t p, int src) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(src >= 0 && src < p->g->g->num_nodes, "mgx_bfs_reset: src out of range");
  use_device(p->g->c);
  p->p->reset((size_t)src, *p->g->c->ctx);
  if (p->visited_mask.size()) {        // the idempotent mode's bitmask: only the source seen
    unsigned* const mask = p->visited_mask.data();
    MGX_HIP(hipMemsetAsync(mask, 0, p->visited_mask.size() * sizeof(unsigned), p->g->c->ctx->stream()));
    mgx::transform([=] __device__(int) { mask[src >> 5] = 1u << (src & 31); }, 1, *p->g->c->ctx);
  }
  MGX_CATCH
}
int mgx_bfs_free(mgx_bfs_t p) {
  MGX_TRY
  if (p) { use_device(p->g->c); delete p; }
  MGX_CATCH
}
int mgx_bfs_labels(mgx_bfs_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_labels.data(), p->n());
  MGX_CATCH
}
int mgx_bfs_preds(mgx_bfs_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_preds.data(), p->n());
  MGX_CATCH
}
int mgx_bfs_labels_device(mgx_bfs_t p, int** d) {
  MGX_TRY
  MGX_REQUIRE(p && d, "NULL argument");
  *d = p->p->d_labels.data();
  MGX_CATCH
}

int mgx_bfs_advance(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::advance_forward_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t, false, true>(
      p->p, in->f, out->f, iteration, *p->g->c->ctx);
  if (front) *front = r;
  MGX_CATCH
}
int mgx_bfs_filter(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::filter::filter_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t>(p->p, in->f, out->f, iteration,
                                                                                   *p->g->c->ctx);
  if (kept) *kept = r;
  MGX_CATCH
}
int mgx_bfs_advance_filter_fused(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::advance_filter_fused_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t>(
      p->p, in->f, out->f, iteration, *p->g->c->ctx);
  if (kept) *kept = r;
  MGX_CATCH
}
int mgx_bfs_gen_unvisited(mgx_bfs_t p, mgx_frontier_t indices, mgx_frontier_t unvisited, int iteration,
                          int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(p && indices && unvisited, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::gen_unvisited_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t>(
      p->p, indices->f, unvisited->f, iteration, *p->g->c->ctx);
  if (kept) *kept = r;
  MGX_CATCH
}
int mgx_bfs_sparse_to_dense(mgx_bfs_t p, mgx_frontier_t sparse, mgx_frontier_t dense, int iteration) {
  MGX_TRY
  MGX_REQUIRE(p && sparse && dense, "NULL argument");
  use_device(p->g->c);
  oprtr::advance::sparse_to_dense_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t>(p->p, sparse->f, dense->f,
                                                                                iteration, *p->g->c->ctx);
  MGX_CATCH
}
int mgx_bfs_advance_backward(mgx_bfs_t p, mgx_frontier_t unvisited, mgx_frontier_t bitmap, mgx_frontier_t bitmap_out,
                             int iteration, int64_t* front) {
  MGX_TRY
  MGX_REQUIRE(p && unvisited && bitmap && bitmap_out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::advance_backward_kernel<bfs::bfs_problem_t, bfs::bfs_functor_t>(
      p->p, unvisited->f, bitmap->f, bitmap_out->f, iteration, *p->g->c->ctx);
  if (front) *front = r;
  MGX_CATCH
}
int mgx_bfs_enact_pushpull(mgx_bfs_t p, float threshold, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  bfs::bfs_enactor_t& e = bfs_enactor(p);
  e.enact_pushpull(p->p, threshold, *p->g->c->ctx);
  p->g->c->ctx->synchronize();
  if (stats) {
    stats[0] = e.pushed_iterations;
    stats[1] = e.total_iterations;
    stats[2] = e.pushed_edges;
    stats[3] = e.pulled_edges;
  }
  MGX_CATCH
}

static mem_t<unsigned>& bfs_mask(mgx_bfs_t p) {
  if (!p->visited_mask.size()) {
    const size_t words = ((size_t)p->g->g->num_nodes + 31) / 32 + 1;
    p->visited_mask = mem_t<unsigned>(words, *p->g->c->ctx);
    unsigned* const mask = p->visited_mask.data();
    const int src = p->p->src;           // the state mgx_bfs_reset leaves: only the source seen
    MGX_HIP(hipMemsetAsync(mask, 0, words * sizeof(unsigned), p->g->c->ctx->stream()));
    mgx::transform([=] __device__(int) { mask[src >> 5] = 1u << (src & 31); }, 1, *p->g->c->ctx);
  }
  return p->visited_mask;
}
int mgx_bfs_advance_idempotent(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::advance_forward_kernel<bfs::bfs_problem_t, bfs::bfs_idempotent_functor_t, true, true>(
      p->p, in->f, out->f, iteration, *p->g->c->ctx);
  if (front) *front = r;
  MGX_CATCH
}
int mgx_bfs_uniquify(mgx_bfs_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  mem_t<unsigned>& mask = bfs_mask(p);
  oprtr::filter::uniquify_kernel<bfs::bfs_problem_t, bfs::bfs_idempotent_functor_t>(p->p, (unsigned char*)mask.data(), in->f,
                                                                                    out->f, iteration, *p->g->c->ctx);
  if (kept) *kept = (int64_t)out->f->size();
  MGX_CATCH
}
int mgx_bfs_enact_idempotent(mgx_bfs_t p, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  bfs::bfs_enactor_t& e = bfs_enactor(p);
  e.enact_idempotent(p->p, bfs_mask(p), *p->g->c->ctx);
  p->g->c->ctx->synchronize();
  if (stats) {
    stats[0] = e.total_iterations;
    stats[1] = e.idempotent_edges;
  }
  MGX_CATCH
}

static void fill_bfs_stats(int64_t* out24, const bfs::bfs_run_stats_t& L) {
  out24[0] = L.levels;
  out24[1] = L.reached;
  out24[2] = L.m_t;
  out24[3] = L.push_edges;
  out24[4] = L.pull_edges;
  out24[5] = L.push_levels;
  out24[6] = L.kernel_launches;
  out24[7] = L.kernel_ns;
  out24[8] = L.frontier_vertices;
  out24[9] = L.claims;
  const bfs::bfs_kernel_stats_t& D = L.dominant ? L.stream : L.wave;
  out24[10] = D.launches;
  out24[11] = D.ns;
  out24[12] = D.edges;
  out24[13] = D.vertices;
  out24[14] = L.dominant;
  out24[15] = L.small_levels;
  out24[16] = L.slots;
  out24[17] = L.dense_slots;
  out24[18] = L.vshort_slots;
  out24[19] = L.lazy_slots;
  out24[20] = L.cold_slots;
  out24[21] = L.mini_slots;
  out24[22] = L.level_byte_slot;
}
int mgx_bfs_run(mgx_bfs_t p, int src, int mode, float alpha, int64_t* stats) { return mgx_bfs_run_stats(p, src, mode, alpha, stats, 16); }
int mgx_bfs_run_stats(mgx_bfs_t p, int src, int mode, float alpha, int64_t* stats, int cap) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(cap >= 0, "mgx_bfs_run_stats: negative capacity");
  MGX_REQUIRE(src >= 0 && src < p->g->g->num_nodes, "mgx_bfs_run: src out of range");
  MGX_REQUIRE(mode == MGX_BFS_PUSH || mode == MGX_BFS_DIRECTION_OPT, "mgx_bfs_run: unknown mode");
  use_device(p->g->c);
  standard_context_t& ctx = *p->g->c->ctx;
  if (!p->fe) p->fe.reset(new bfs::bfs_fused_enactor_t(ctx, p->g->g->num_nodes));
  if (p->time_kernels >= 0) p->fe->fused->time_kernels = p->time_kernels;
  p->p->src = src;
  p->fe->enact(p->p, ctx, mode == MGX_BFS_DIRECTION_OPT, alpha);
  fill_bfs_stats(p->last_stats, p->fe->last);
  constexpr int have = (int)(sizeof(p->last_stats) / sizeof(p->last_stats[0]));
  if (stats) memcpy(stats, p->last_stats, sizeof(int64_t) * (size_t)(cap < have ? cap : have));
  MGX_CATCH
}
int mgx_bfs_run_many(mgx_bfs_t p, const int* sources, int count, int mode, float alpha, int64_t* stats, int cap, int* reruns) {
  MGX_TRY
  MGX_REQUIRE(p && (sources || count == 0), "NULL argument");
  MGX_REQUIRE(count >= 0 && count <= (1 << 20), "mgx_bfs_run_many: count out of range");
  MGX_REQUIRE(cap >= 0, "mgx_bfs_run_many: negative capacity");
  MGX_REQUIRE(mode == MGX_BFS_PUSH || mode == MGX_BFS_DIRECTION_OPT, "mgx_bfs_run_many: unknown mode");
  for (int i = 0; i < count; ++i) MGX_REQUIRE(sources[i] >= 0 && sources[i] < p->g->g->num_nodes, "mgx_bfs_run_many: src out of range");
  if (reruns) *reruns = 0;
  if (count == 0) return MGX_OK;
  use_device(p->g->c);
  standard_context_t& ctx = *p->g->c->ctx;
  if (!p->fe) p->fe.reset(new bfs::bfs_fused_enactor_t(ctx, p->g->g->num_nodes));
  p->fe->fused->time_kernels = 0;                       // (per-launch events belong to mgx_bfs_run)
  std::vector<bfs::bfs_run_stats_t> all;
  const int rr = p->fe->enact_many(p->p, ctx, sources, count, all, mode == MGX_BFS_DIRECTION_OPT, alpha);
  if (reruns) *reruns = rr;
  constexpr int have = (int)(sizeof(p->last_stats) / sizeof(p->last_stats[0]));
  const int take = cap < have ? cap : have;
  for (int i = 0; i < count; ++i) {
    fill_bfs_stats(p->last_stats, all[(size_t)i]);
    if (stats && take > 0) memcpy(stats + (size_t)i * (size_t)cap, p->last_stats, sizeof(int64_t) * (size_t)take);
  }
  MGX_CATCH
}
int mgx_bfs_level_trace(mgx_bfs_t p, int cap, int64_t* level_nf, int64_t* level_edges, int* levels) {
  MGX_TRY
  MGX_REQUIRE(p && levels, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_level_trace: no mgx_bfs_run yet");
  const auto& tr = p->fe->last.trace;
  *levels = (int)tr.size();
  for (int i = 0; i < (int)tr.size() && i < cap; ++i) {
    if (level_nf) level_nf[i] = tr[i].first;
    if (level_edges) level_edges[i] = tr[i].second;
  }
  MGX_CATCH
}
int mgx_bfs_set_kernel_timing(mgx_bfs_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->time_kernels = on < 0 ? 0 : on;
  MGX_CATCH
}
int mgx_bfs_kernel_times(mgx_bfs_t p, int64_t* out8) {
  MGX_TRY
  MGX_REQUIRE(p && out8, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_kernel_times: no mgx_bfs_run yet");
  const bfs::bfs_run_stats_t& L = p->fe->last;
  out8[0] = L.stream.launches; out8[1] = L.stream.ns; out8[2] = L.stream.edges; out8[3] = L.stream.vertices;
  out8[4] = L.wave.launches; out8[5] = L.wave.ns; out8[6] = L.wave.edges; out8[7] = L.wave.vertices;
  MGX_CATCH
}
int mgx_bfs_level_kernel_times(mgx_bfs_t p, int cap, float* stream_ms, float* wave_ms) {
  MGX_TRY
  MGX_REQUIRE(p && stream_ms && wave_ms, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_level_kernel_times: no mgx_bfs_run yet");
  for (int i = 0; i < cap && i < 64; ++i) {
    stream_ms[i] = p->fe->fused->level_stream_ms[i];
    wave_ms[i] = p->fe->fused->level_wave_ms[i];
  }
  MGX_CATCH
}
int mgx_bfs_level_times(mgx_bfs_t p, int cap, float* ms, int* levels) {
  MGX_TRY
  MGX_REQUIRE(p && levels, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_level_times: no mgx_bfs_run yet");
  const auto& t = p->fe->last.level_ms;
  *levels = (int)t.size();
  for (int i = 0; i < (int)t.size() && i < cap; ++i)
    if (ms) ms[i] = t[i];
  MGX_CATCH
}
int mgx_bfs_level_claims(mgx_bfs_t p, int cap, int64_t* claims) {
  MGX_TRY
  MGX_REQUIRE(p && claims, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_level_claims: no mgx_bfs_run yet");
  for (int i = 0; i < cap && i < 64; ++i) claims[i] = p->fe->last.claims_level[i];
  MGX_CATCH
}
int mgx_bfs_batch_times(mgx_bfs_t p, int cap, float* ms, int* batches) {
  MGX_TRY
  MGX_REQUIRE(p && batches, "NULL argument");
  MGX_REQUIRE(p->fe != nullptr, "mgx_bfs_batch_times: no mgx_bfs_run yet");
  const auto& b = p->fe->last.batch_ms;
  *batches = (int)b.size();
  for (int i = 0; i < (int)b.size() && i < cap; ++i)
    if (ms) ms[i] = b[i];
  MGX_CATCH
}

// ---- vertex-range partitioned BFS (per-rank pieces; the exchange is the host's job) -----------
int mgx_dbfs_create(mgx_ctx_t c, int n_global, int ranks, int rank, int64_t m_local, const int* d_row_offsets,
                    const int* d_col_indices, int* d_bins, int64_t bin_capacity, mgx_dbfs_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && d_row_offsets && (d_col_indices || m_local == 0), "mgx_dbfs_create: NULL argument");
  MGX_REQUIRE(n_global > 0 && ranks >= 1 && ranks <= mgx::DBFS_MAX_RANKS && rank >= 0 && rank < ranks,
              "mgx_dbfs_create: bad partition");
  use_device(c);
  const int chunk = (n_global + ranks - 1) / ranks;
  const int lo = rank * chunk < n_global ? rank * chunk : n_global;
  const int hi = (rank + 1) * chunk < n_global ? (rank + 1) * chunk : n_global;
  auto* h = new mgx_dbfs_s();
  h->c = c;
  MGX_REQUIRE(d_bins == nullptr || bin_capacity >= chunk, "mgx_dbfs_create: bin capacity must be >= ceil(n/ranks)");
  h->st.init(*c->ctx, n_global, lo, hi, ranks, rank, d_row_offsets, d_col_indices, m_local, d_bins, bin_capacity);
  *out = h;
  MGX_CATCH
}
int mgx_dbfs_free(mgx_dbfs_t h) {
  MGX_TRY
  if (h) { use_device(h->c); delete h; }
  MGX_CATCH
}
int mgx_dbfs_range(mgx_dbfs_t h, int* lo, int* hi) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  if (lo) *lo = h->st.v_lo;
  if (hi) *hi = h->st.v_hi;
  MGX_CATCH
}
int mgx_dbfs_reset(mgx_dbfs_t h, int src_global) {
  MGX_TRY
  MGX_REQUIRE(h && src_global >= 0 && src_global < h->st.n_global, "mgx_dbfs_reset: bad argument");
  use_device(h->c);
  mgx::dbfs_reset(h->st, src_global, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs_expand(mgx_dbfs_t h, int64_t* counts, int64_t* edges) {
  MGX_TRY
  MGX_REQUIRE(h && counts, "NULL argument");
  use_device(h->c);
  long long e = 0;
  mgx::dbfs_expand(h->st, *h->c->ctx, &e);
  for (int r = 0; r < h->st.ranks; ++r) {
    counts[r] = (int64_t)h->st.host_counters[r];
    if (counts[r] > h->st.bin_cap) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx_dbfs_expand: send bin overflow");
  }
  if (edges) *edges = e;
  MGX_CATCH
}
int mgx_dbfs_bins(mgx_dbfs_t h, int** d_bins, int64_t* bin_cap) {
  MGX_TRY
  MGX_REQUIRE(h && d_bins && bin_cap, "NULL argument");
  *d_bins = h->st.bins.data();
  *bin_cap = h->st.bin_cap;
  MGX_CATCH
}
int mgx_dbfs_receive(mgx_dbfs_t h, const int* d_ids, int64_t count, int label) {
  MGX_TRY
  MGX_REQUIRE(h && (d_ids || count == 0) && count >= 0, "bad argument");
  use_device(h->c);
  mgx::dbfs_receive(h->st, d_ids, count, label, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs_swap(mgx_dbfs_t h, int64_t* frontier_size) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  use_device(h->c);
  const long long f = mgx::dbfs_swap(h->st, *h->c->ctx);
  if (frontier_size) *frontier_size = f;
  MGX_CATCH
}
int mgx_dbfs_labels(mgx_dbfs_t h, int* host_labels) {
  MGX_TRY
  MGX_REQUIRE(h && host_labels, "NULL argument");
  use_device(h->c);
  h->c->ctx->synchronize();
  MGX_HIP(mgx::dtoh(host_labels, h->st.labels.data(), (size_t)h->st.n_local));
  MGX_CATCH
}

// ---- vertex-range partitioned SSSP (per-rank pieces; mgx/sssp_dist.hpp) -----------------------------------------
int mgx_dsssp_create(mgx_ctx_t c, int n_global, int ranks, int rank, int64_t m_local, const int* d_row_offsets,
                     const int* d_col_indices, const float* d_weights, mgx_dsssp_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && d_row_offsets && ((d_col_indices && d_weights) || m_local == 0), "mgx_dsssp_create: NULL argument");
  MGX_REQUIRE(n_global > 0 && ranks >= 1 && ranks <= mgx::DBFS_MAX_RANKS && rank >= 0 && rank < ranks, "mgx_dsssp_create: bad partition");
  use_device(c);
  const int chunk = (n_global + ranks - 1) / ranks;
  const int lo = rank * chunk < n_global ? rank * chunk : n_global;
  const int hi = (rank + 1) * chunk < n_global ? (rank + 1) * chunk : n_global;
  auto* h = new mgx_dsssp_s();
  h->c = c;
  h->st.init(*c->ctx, n_global, lo, hi, ranks, rank, d_row_offsets, d_col_indices, d_weights, m_local);
  *out = h;
  MGX_CATCH
}
int mgx_dsssp_free(mgx_dsssp_t h) {
  MGX_TRY
  if (h) { use_device(h->c); delete h; }
  MGX_CATCH
}
int mgx_dsssp_reset(mgx_dsssp_t h, int src_global) {
  MGX_TRY
  MGX_REQUIRE(h && src_global >= 0 && src_global < h->st.n_global, "mgx_dsssp_reset: bad argument");
  use_device(h->c);
  mgx::dsssp_reset(h->st, src_global, *h->c->ctx);
  MGX_CATCH
}
int mgx_dsssp_expand(mgx_dsssp_t h, int64_t* counts, int64_t* edges) {
  MGX_TRY
  MGX_REQUIRE(h && counts, "NULL argument");
  use_device(h->c);
  long long e = 0;
  mgx::dsssp_expand(h->st, *h->c->ctx, &e);
  for (int r = 0; r < h->st.ranks; ++r) {
    counts[r] = (int64_t)h->st.host_counters[r];
    if (counts[r] > h->st.bin_cap) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx_dsssp_expand: send bin overflow");
  }
  if (edges) *edges = e;
  MGX_CATCH
}
int mgx_dsssp_bins(mgx_dsssp_t h, uint64_t** d_bins, int64_t* bin_cap) {
  MGX_TRY
  MGX_REQUIRE(h && d_bins && bin_cap, "NULL argument");
  *d_bins = (uint64_t*)h->st.bins.data();
  *bin_cap = h->st.bin_cap;
  MGX_CATCH
}
int mgx_dsssp_receive(mgx_dsssp_t h, const uint64_t* d_pairs, int64_t count) {
  MGX_TRY
  MGX_REQUIRE(h && (d_pairs || count == 0) && count >= 0, "bad argument");
  use_device(h->c);
  mgx::dsssp_receive(h->st, (const unsigned long long*)d_pairs, count, *h->c->ctx);
  MGX_CATCH
}
int mgx_dsssp_swap(mgx_dsssp_t h, int64_t* frontier_size) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  use_device(h->c);
  const long long f = mgx::dsssp_swap(h->st, *h->c->ctx);
  if (frontier_size) *frontier_size = f;
  MGX_CATCH
}
int mgx_dsssp_distances(mgx_dsssp_t h, float* host_dist_local) {
  MGX_TRY
  MGX_REQUIRE(h && host_dist_local, "NULL argument");
  use_device(h->c);
  h->c->ctx->synchronize();
  MGX_HIP(mgx::dtoh((unsigned*)host_dist_local, h->st.dist.data(), (size_t)h->st.n_local));
  MGX_CATCH
}

int mgx_dsssp_run(mgx_dsssp_t h, mgx_comm_t comm, int src_global, int64_t* out4) {
  MGX_TRY
  MGX_REQUIRE(h && out4 && src_global >= 0 && src_global < h->st.n_global, "mgx_dsssp_run: bad argument");
  MGX_REQUIRE(comm || h->st.ranks == 1, "mgx_dsssp_run: a communicator is needed for more than one rank");
  MGX_REQUIRE(!comm || (comm->cm.ranks == h->st.ranks && comm->cm.rank == h->st.rank), "mgx_dsssp_run: communicator and engine disagree on the partition");
  use_device(h->c);
  mgx::comm_t none;
  long long o[4];
  mgx::dsssp_run(h->st, comm ? comm->cm : none, h->run_bufs, src_global, *h->c->ctx, o);
  for (int i = 0; i < 4; ++i) out4[i] = o[i];
  MGX_CATCH
}

// ---- partitioned BFS, generation 2: fused kernels per rank + bitmap exchange (mgx/bfs_dist2.hpp) ----
int mgx_dbfs2_create(mgx_ctx_t c, int n_global, int ranks, int rank, const int* d_row_offsets_local,
                     const int* d_col_indices_global, unsigned* d_newbits, mgx_dbfs2_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && out && d_row_offsets_local && d_newbits, "mgx_dbfs2_create: NULL argument");
  MGX_REQUIRE(n_global > 0 && ranks >= 1 && ranks <= 64 && rank >= 0 && rank < ranks, "mgx_dbfs2_create: bad partition");
  use_device(c);
  auto* h = new mgx_dbfs2_s();
  h->c = c;
  h->st.init(*c->ctx, n_global, ranks, rank, d_row_offsets_local, d_col_indices_global, d_newbits);
  c->ctx->synchronize();
  *out = h;
  MGX_CATCH
}
int mgx_dbfs2_build_units(mgx_dbfs2_t h, int64_t* units) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  use_device(h->c);
  mgx::d2_state_t& st = h->st;
  mgx::row_layout_t& R = st.rows;
  standard_context_t& ctx = *h->c->ctx;
  if (units) *units = 0;
  if (st.blocks().col.size()) { if (units) *units = st.blocks().units; return MGX_OK; }
  const int long_min = st.fs->long_min;
  if (long_min != 64 || st.n_local <= 0) return MGX_OK;     // (a unit is 64 entries: only with the default long-row threshold)
  ctx.synchronize();
  const mgx::owner_remap_t global{st.ranks, st.rank, st.n_local, st.n_global};
  mgx::build_unit_blocks(R.ub, st.row_offsets, st.col_indices, st.n_local, long_min, 0u, global, false, ctx.stream());
  const long long U = R.ub.units;
  if (U <= 0) return MGX_OK;
  ctx.synchronize();
  if (const char* e = mgx::env("MGX_DIST_DENSE_DIV")) { const int d = atoi(e); if (d >= 0) st.dense_div = (unsigned)d; }
  // the short rows vertex by vertex (MGX_DIST_VSHORT=0: never; N: when a level holds 1 / N of their edges): needs rows by
  // non-increasing degree (hub-first global ids, cyclic ownership: they are) -- checked here, on the host
  {
    int vdiv = 8;
    if (const char* e = mgx::env("MGX_DIST_VSHORT")) vdiv = atoi(e);
    const int n = st.n_local;
    if (n > 0) {
      // deferred hot marks only on a shard big enough to pay for their bitmaps (d2_state_t::defer_pays)
      int m_last = 0;
      MGX_HIP(mgx::dtoh(&m_last, st.row_offsets + n, 1));
      int defer_mode = 1;
      if (const char* e = mgx::env("MGX_DIST_DEFER")) defer_mode = atoi(e);
      st.defer_pays = defer_mode == 2 || (long long)m_last >= mgx::d2_state_t::D2_DEFER_MIN_ENTRIES;
    }
    if (vdiv > 0 && n > 0) {
      std::vector<int> hro((size_t)n + 1);
      MGX_HIP(mgx::dtoh(hro.data(), st.row_offsets, (size_t)n + 1));
      bool sorted = true;
      for (int i = 1; i < n && sorted; ++i) sorted = hro[i + 1] - hro[i] <= hro[i] - hro[i - 1];
      const long long m_local = hro[n];
      if (sorted && m_local > 0) {
        mgx::cut_degree_classes(R, hro, (size_t)n, long_min);
        st.col_pad = mem_t<int>((size_t)m_local + 8, ctx);
        MGX_HIP(hipMemcpyAsync(st.col_pad.data(), st.col_indices, (size_t)m_local * sizeof(int), hipMemcpyDeviceToDevice, ctx.stream()));
        MGX_HIP(hipMemsetAsync(st.col_pad.data() + m_local, 0xFF, 8 * sizeof(int), ctx.stream()));
        st.front_local = mem_t<unsigned>((size_t)n / 32 + 64, ctx);
        MGX_HIP(hipMemsetAsync(st.front_local.data(), 0, st.front_local.size() * sizeof(unsigned), ctx.stream()));
        ctx.synchronize();
        st.vs_div = R.vs_edges ? (unsigned)vdiv : 0u;
      }
    }
  }
  if (units) *units = U;
  // cold-edge lists of the same rows (bfs_fused_cold.hpp; MGX_DIST_COLD=0: none): as build_cold_lists does for a graph's layout --
  // only when the destinations behind the LDS prefix span at most 128 slices of which at most BFS_COLD_MAX_SLICES hold pairs,
  // and the cold entries are at most half of the long rows' entries
  bool want_cold = true;
  if (const char* e = mgx::env("MGX_DIST_COLD")) want_cold = atoi(e) != 0;
  const unsigned hot_n = (unsigned)mgx::BFS_COLD_WORDS * 32u, slice_n = hot_n;
  const long long slices_ll = (unsigned)st.n_global > hot_n ? ((long long)st.n_global - hot_n + slice_n - 1) / slice_n : 0;
  if (!want_cold || slices_ll < 1 || slices_ll > 128) return MGX_OK;
  mem_t<int> d_long = mgx::fill<int>(0, 1, ctx), d_sorted = mgx::fill<int>(1, 1, ctx);
  hipLaunchKernelGGL(mgx::k_d2_row_facts, dim3(ctx.num_cus * 8), dim3(mgx::BLOCK), 0, ctx.stream(), st.row_offsets, st.col_indices, st.n_local, long_min,
                     d_long.data(), d_sorted.data());
  ctx.synchronize();
  const int long_rows = mgx::from_mem(d_long)[0];
  const bool rows_sorted = mgx::from_mem(d_sorted)[0] == 1;
  if (!rows_sorted || long_rows <= 0) return MGX_OK;
  std::vector<int> off;
  const long long pairs = mgx::build_cold_pairs(R.cold_owner, R.cold_dst, off, st.row_offsets, st.col_indices, st.n_local, 0, long_rows, long_min, hot_n,
                                                slice_n, (int)slices_ll, ctx.stream());
  long long nwg = (pairs + 131071) / 131072;
  nwg = std::max<long long>(nwg, mgx::BFS_COLD_WGS);
  // (at most 512 on a rank: every cold workgroup costs a copy of its slice into LDS and an 80 KB bitmap to write and to reduce --
  //  RMAT-26 / 8 with 1 024 of them: push 584 us and reduce 87 us per traversal, with 512: 552 and 57, with 256: 575 and 46)
  nwg = std::min<long long>(nwg, 512);
  if (const char* e = mgx::env("MGX_DIST_COLD_WGS")) if (atoi(e) > 0) nwg = std::min<long long>(atoi(e), mgx::BFS_COLD_WGS_MAX);      // (measurements)
  // the pairs once more, four bytes each
  bool pack_pairs = true;
  if (const char* e = mgx::env("MGX_BFS_COLD_PACK")) pack_pairs = atoi(e) != 0;
  R.cold_pairs = pairs;
  // (RMAT-25 / 8: a quarter of the entries, RMAT-26 / 8: a third)
  if (pairs <= 0 || pairs * 2 > U * 64 ||
      !mgx::cut_cold_lists(R, off, std::vector<int>(off.size(), 0), hot_n, slice_n, nwg, global, pack_pairs, ctx.stream())) {
    R.cold_owner = mem_t<int>(); R.cold_dst = mem_t<int>(); R.cold_pairs = 0;
    return MGX_OK;
  }
  st.cold_flush = mem_t<u32>((size_t)R.cold_wgs[R.cold_slices] * mgx::BFS_COLD_WORDS, ctx);
  MGX_HIP(hipMemsetAsync(st.cold_flush.data(), 0, st.cold_flush.size() * sizeof(unsigned), ctx.stream()));
  // a launch of its own ORs a slice's bitmaps together in front of the sweep (MGX_DIST_COLD_REDUCE=0: k_d2_newbits reads them all)
  if (const char* e = mgx::env("MGX_DIST_COLD_REDUCE")) st.cold_reduce = atoi(e);
  ctx.synchronize();
  // The unit blocks again, WITHOUT the entries that now live in the pair lists (the unit-block body read them only to skip
  // them: a third of its stream on RMAT-26 / 8) -- and what is left points into the LDS prefix, ids below 2^20: three bytes
  // per entry do (bfs_fused_dense.hpp: ub_col24).  MGX_DIST_HOT_UNITS=0: the full blocks stay.
  bool hot_units = true;
  if (const char* e = mgx::env("MGX_DIST_HOT_UNITS")) hot_units = atoi(e) != 0;
  if (hot_units) {
    mgx::build_unit_blocks(R.ubh, st.row_offsets, st.col_indices, st.n_local, long_min, hot_n, global, false, ctx.stream());
    ctx.synchronize();
    if (R.ubh.units > 0) {
      R.ub = mgx::unit_blocks_t();
      if (units) *units = R.ubh.units;
      bool pack = true;
      if (const char* e = mgx::env("MGX_BFS_PACK24")) pack = atoi(e) != 0;
      if (pack) mgx::pack_unit_blocks24(R.ubh, true, ctx.stream());
    }
  }
  MGX_CATCH
}
int mgx_dbfs2_dense_levels(mgx_dbfs2_t h, int64_t* levels) {
  MGX_TRY
  MGX_REQUIRE(h && levels, "NULL argument");
  *levels = (int64_t)h->st.fs->host_ctrl->dense_slots;     // (as of the last mgx_dbfs2_status / mgx_dbfs2_run)
  MGX_CATCH
}
int mgx_dbfs2_cold_levels(mgx_dbfs2_t h, int64_t* levels, int64_t* pairs) {
  MGX_TRY
  MGX_REQUIRE(h && levels, "NULL argument");
  *levels = (int64_t)h->st.fs->host_ctrl->cold_slots;
  if (pairs) *pairs = (int64_t)h->st.rows.cold_pairs;
  MGX_CATCH
}
int mgx_dbfs2_path_levels(mgx_dbfs2_t h, int64_t* out4) {
  MGX_TRY
  MGX_REQUIRE(h && out4, "NULL argument");
  const mgx::bfs_ctrl_t* hc = h->st.fs->host_ctrl.data();          // (as of the last mgx_dbfs2_status / mgx_dbfs2_run)
  out4[0] = (int64_t)hc->small_levels;                       // levels whose push appended its discoveries to the id list itself
  out4[1] = (int64_t)hc->vshort_slots;                       // levels whose short rows were walked vertex by vertex
  out4[2] = (int64_t)hc->d2_declared_level >= 0 ? 1 : 0;     // a sweep declared its list overflowed (the last such level is kept, not a count)
  out4[3] = (int64_t)(h->st.rows.cold_pk.data() ? __builtin_popcountll(h->st.rows.cold_pk_mask) : 0);   // slices whose pairs are packed to 4 bytes
  MGX_CATCH
}
int mgx_dbfs2_free(mgx_dbfs2_t h) {
  MGX_TRY
  if (h) { use_device(h->c); delete h; }
  MGX_CATCH
}
int mgx_dbfs2_reset(mgx_dbfs2_t h, int src) {
  MGX_TRY
  MGX_REQUIRE(h && src >= 0 && src < h->st.n_global, "mgx_dbfs2_reset: bad argument");
  use_device(h->c);
  mgx::d2_reset(h->st, src, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs2_push(mgx_dbfs2_t h, int level) {
  MGX_TRY
  MGX_REQUIRE(h && level >= 0, "bad argument");
  use_device(h->c);
  mgx::d2_push(h->st, level, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs2_merge(mgx_dbfs2_t h, int level, const unsigned* d_gathered) {
  MGX_TRY
  MGX_REQUIRE(h && d_gathered && level >= 0, "bad argument");
  use_device(h->c);
  mgx::d2_merge(h->st, level, d_gathered, h->st.ranks, h->st.nwords, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs2_merge_maps(mgx_dbfs2_t h, int level, const unsigned* d_maps, int maps, int64_t stride_words) {
  MGX_TRY
  MGX_REQUIRE(h && d_maps && level >= 0, "bad argument");
  MGX_REQUIRE(maps >= 1 && maps <= 64 && stride_words >= h->st.nwords && stride_words % 4 == 0,
              "mgx_dbfs2_merge_maps: maps must be 1..64 and the stride a multiple of 4 words, at least a bitmap long");
  use_device(h->c);
  mgx::d2_merge(h->st, level, d_maps, maps, (long long)stride_words, *h->c->ctx);
  MGX_CATCH
}
int mgx_dbfs2_or_maps(mgx_dbfs2_t h, const unsigned* d_maps, int maps, int64_t stride_words, int64_t words,
                      unsigned* d_out) {
  MGX_TRY
  MGX_REQUIRE(h && d_maps && d_out, "NULL argument");
  MGX_REQUIRE(maps >= 1 && maps <= 64 && words >= 0 && words % 4 == 0 && stride_words % 4 == 0 && stride_words >= words,
              "mgx_dbfs2_or_maps: maps must be 1..64, words and stride multiples of 4, stride >= words");
  use_device(h->c);
  if (words)
    hipLaunchKernelGGL(mgx::k_d2_or_maps, dim3(mgx::grid_for(words / 4, mgx::BLOCK, 1024)), dim3(mgx::BLOCK), 0,
                       h->c->ctx->stream(), (const uint4*)d_maps, maps, (long long)(stride_words / 4), (long long)(words / 4),
                       (uint4*)d_out);
  MGX_CATCH
}
extern "C" int mgx_shard_plan_device(int scale, int edgefactor, unsigned long long seed, int ranks, int rank, void** handle, int* n_local,
                                     long long* m_local, hipStream_t stream);
extern "C" int mgx_shard_fill_device(void* handle, int* row_offsets, int* col, int* new_of_old, int* old_of_new, int* deg_of_new,
                                     hipStream_t stream);
extern "C" void mgx_shard_free_device(void* handle);
int mgx_dbfs2_shard_plan(mgx_ctx_t c, int scale, int edgefactor, uint64_t seed, int ranks, int rank, void** plan, int* n_local, int64_t* m_local) {
  MGX_TRY
  MGX_REQUIRE(c && plan && n_local && m_local, "NULL argument");
  MGX_REQUIRE(scale >= 1 && scale <= 30 && edgefactor >= 1 && ranks >= 1 && ranks <= 64 && rank >= 0 && rank < ranks,
              "mgx_dbfs2_shard_plan: bad argument");
  use_device(c);
  long long m = 0;
  const int rc = mgx_shard_plan_device(scale, edgefactor, (unsigned long long)seed, ranks, rank, plan, n_local, &m, c->ctx->stream());
  if (rc != 0) throw mgx::mgx_error(MGX_E_HIP, std::string("mgx_dbfs2_shard_plan: ") + hipGetErrorString((hipError_t)rc));
  MGX_REQUIRE(m < (1ll << 31), "mgx_dbfs2_shard_plan: more than 2^31 - 1 entries on one rank (int32 local offsets)");
  *m_local = m;
  MGX_CATCH
}
int mgx_dbfs2_shard_fill(mgx_ctx_t c, void* plan, int* d_row_offsets_local, int* d_col_indices, int* d_new_of_old, int* d_old_of_new,
                         int* d_degree_of_new) {
  MGX_TRY
  MGX_REQUIRE(c && plan && d_row_offsets_local, "NULL argument");
  use_device(c);
  const int rc = mgx_shard_fill_device(plan, d_row_offsets_local, d_col_indices, d_new_of_old, d_old_of_new, d_degree_of_new, c->ctx->stream());
  if (rc != 0) throw mgx::mgx_error(MGX_E_HIP, std::string("mgx_dbfs2_shard_fill: ") + hipGetErrorString((hipError_t)rc));
  MGX_CATCH
}
int mgx_dbfs2_shard_free(void* plan) {
  MGX_TRY
  mgx_shard_free_device(plan);
  MGX_CATCH
}
int mgx_dbfs2_list_words(int n_global, int ranks, int64_t* words) {
  MGX_TRY
  MGX_REQUIRE(words && n_global > 0 && ranks >= 1 && ranks <= 64, "mgx_dbfs2_list_words: bad argument");
  *words = (int64_t)mgx::D2_LIST_HEAD + (int64_t)mgx::d2_state_t::default_list_cap(n_global, ranks);
  MGX_CATCH
}
int mgx_dbfs2_set_list(mgx_dbfs2_t h, unsigned* d_list, int64_t words) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  MGX_REQUIRE(!d_list || (words > mgx::D2_LIST_HEAD && words % 4 == 0 && words < (1ll << 31)),
              "mgx_dbfs2_set_list: the list must hold its 4 header words and a multiple of 4 words in all");
  use_device(h->c);
  h->c->ctx->synchronize();
  h->st.set_list(d_list, d_list ? (unsigned)(words - mgx::D2_LIST_HEAD) : 0u);
  MGX_CATCH
}
int mgx_dbfs2_apply_lists(mgx_dbfs2_t h, int level, const unsigned* d_lists, int lists, int64_t stride_words, int64_t* out3) {
  MGX_TRY
  MGX_REQUIRE(h && d_lists && out3 && level >= 0, "bad argument");
  MGX_REQUIRE(h->st.mylist != nullptr, "mgx_dbfs2_apply_lists: no list was set (mgx_dbfs2_set_list)");
  MGX_REQUIRE(lists >= 1 && lists <= 64 && stride_words >= h->st.list_words(), "mgx_dbfs2_apply_lists: 1..64 lists, each at least a list long");
  use_device(h->c);
  long long o[3];
  mgx::d2_apply_lists(h->st, level, d_lists, lists, (long long)stride_words, *h->c->ctx, o);
  for (int i = 0; i < 3; ++i) out3[i] = o[i];
  MGX_CATCH
}
int mgx_dbfs2_status(mgx_dbfs2_t h, int next_level, int64_t* out6) {
  MGX_TRY
  MGX_REQUIRE(h && out6 && next_level >= 0, "bad argument");
  use_device(h->c);
  long long o[6];
  mgx::d2_status(h->st, next_level, *h->c->ctx, o);
  for (int i = 0; i < 6; ++i) out6[i] = o[i];
  MGX_CATCH
}
// ---- RCCL communicator of the library's own (mgx/comm.hpp) and the traversal driven from C++ ----
// (MGX_COMM=loopback, an environment route to the in-process stand-in, is gone since round 6: a loopback world is asked for by id,
//  mgx_comm_loopback_id -- the tests' way)
int mgx_comm_unique_id(unsigned char* out128) {
  MGX_TRY
  MGX_REQUIRE(out128, "NULL argument");
  mgx::rccl_api_t& api = mgx::rccl_api_t::get();
  MGX_REQUIRE(api.ok(), "mgx_comm_unique_id: no RCCL in this process and none could be loaded (librccl.so.1)");
  ncclUniqueId id;
  MGX_RCCL(api.GetUniqueId(&id));
  memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
  MGX_CATCH
}
int mgx_comm_loopback_id(unsigned char* out128) {
  MGX_TRY
  MGX_REQUIRE(out128, "NULL argument");
  const mgx::rccl_api_t& api = mgx::rccl_api_t::loopback();
  MGX_REQUIRE(api.ok(), "mgx_comm_loopback_id: the in-process stand-in for RCCL is a test library of its own (mini_amd/libmgx_loopback.so, built by __graft_entry__.build()): not found next to this library");
  ncclUniqueId id;
  MGX_RCCL(api.GetUniqueId(&id));
  memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
  MGX_CATCH
}
int mgx_comm_create(mgx_ctx_t c, int ranks, int rank, const unsigned char* id128, mgx_comm_t* out) {
  MGX_TRY
  MGX_REQUIRE(c && id128 && out && ranks >= 1 && rank >= 0 && rank < ranks, "mgx_comm_create: bad argument");
  // (a loopback id -- mgx_comm_loopback_id -- names the in-process stand-in: a test library of its own since round 6)
  const bool loop = mgx::loopback::is_loopback_id(id128);
  const mgx::rccl_api_t& api = loop ? mgx::rccl_api_t::loopback() : mgx::rccl_api_t::get();
  MGX_REQUIRE(api.ok(), loop ? "mgx_comm_create: a loopback id, but mini_amd/libmgx_loopback.so (the test double) is not next to this library"
                             : "mgx_comm_create: no RCCL in this process and none could be loaded (librccl.so.1)");
  use_device(c);
  ncclUniqueId id;
  memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
  auto* h = new mgx_comm_s();
  h->c = c;
  h->cm.ranks = ranks; h->cm.rank = rank; h->cm.api = &api;
  ncclResult_t r = api.CommInitRank(&h->cm.comm, ranks, id, rank);
  if (r != ncclSuccess) {
    h->cm.comm = nullptr;
    delete h;
    throw mgx::mgx_error(MGX_E_HIP, std::string("ncclCommInitRank: ") + (api.GetErrorString ? api.GetErrorString(r) : "RCCL error"));
  }
  *out = h;
  MGX_CATCH
}
int mgx_comm_info(mgx_comm_t h, int* is_loopback, int64_t* rounds) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  const bool loop = h->cm.api == &mgx::rccl_api_t::loopback();
  if (is_loopback) *is_loopback = loop ? 1 : 0;
  if (rounds) *rounds = (loop && h->cm.api->rounds) ? (int64_t)h->cm.api->rounds(h->cm.comm) : 0;
  MGX_CATCH
}
int mgx_comm_selftest(mgx_comm_t h, const unsigned* d_send, unsigned* d_gathered, unsigned* d_alltoall, int64_t words) {
  MGX_TRY
  MGX_REQUIRE(h && d_send && d_gathered && d_alltoall && words > 0, "mgx_comm_selftest: bad argument");
  use_device(h->c);
  const mgx::rccl_api_t& api = h->cm.table();
  hipStream_t s = h->c->ctx->stream();
  const int R = h->cm.ranks;
  MGX_RCCL(api.AllGather(d_send, d_gathered, (size_t)words, ncclUint32, h->cm.comm, s));
  {
    mgx::rccl_group_t group(api);
    for (int r = 0; r < R; ++r) {
      MGX_RCCL(api.Send(d_send + (size_t)r * words, (size_t)words, ncclUint32, r, h->cm.comm, s));
      MGX_RCCL(api.Recv(d_alltoall + (size_t)r * words, (size_t)words, ncclUint32, r, h->cm.comm, s));
    }
    group.end();
  }
  MGX_HIP(hipStreamSynchronize(s));
  MGX_CATCH
}
int mgx_comm_free(mgx_comm_t h) {
  MGX_TRY
  if (h) { use_device(h->c); delete h; }
  MGX_CATCH
}
const char* mgx_comm_library(void) { return mgx::rccl_api_t::get().where.c_str(); }
int mgx_env_switches(int index, const char** name, const char** what) {
  int n = 0;
  const mgx::env_switch_t* t = mgx::env_switches(&n);
  if (index >= 0 && index < n) { if (name) *name = t[index].name; if (what) *what = t[index].what; }
  return n;
}
int mgx_build_is_lab(void) {
#ifdef MGX_LAB
  return 1;
#else
  return 0;
#endif
}
int mgx_comm_available(void) { return mgx::rccl_api_t::get().ok() ? 1 : 0; }
int mgx_dbfs2_run(mgx_dbfs2_t h, mgx_comm_t comm, int src_global, int exchange, int64_t exchange_words, int64_t* out6) {
  MGX_TRY
  MGX_REQUIRE(h && out6 && src_global >= 0 && src_global < h->st.n_global, "mgx_dbfs2_run: bad argument");
  MGX_REQUIRE(exchange == 0 || exchange == 1, "mgx_dbfs2_run: exchange is 0 (all-gather) or 1 (slices + all-gather)");
  MGX_REQUIRE(comm || h->st.ranks == 1, "mgx_dbfs2_run: a communicator is needed for more than one rank");
  MGX_REQUIRE(!comm || (comm->cm.ranks == h->st.ranks && comm->cm.rank == h->st.rank), "mgx_dbfs2_run: communicator and engine disagree on the partition");
  MGX_REQUIRE(exchange_words >= h->st.nwords && exchange_words % (4 * h->st.ranks) == 0,
              "mgx_dbfs2_run: exchange_words must cover the bitmap and be a multiple of 4 * ranks");
  use_device(h->c);
  mgx::comm_t none;
  long long o[6];
  mgx::d2_run(h->st, comm ? comm->cm : none, h->run_bufs, src_global, exchange, (long long)exchange_words, *h->c->ctx, o);
  for (int i = 0; i < 6; ++i) out6[i] = o[i];
  MGX_CATCH
}
int mgx_dbfs2_spec_stats(mgx_dbfs2_t h, int64_t* out5) {
  MGX_TRY
  MGX_REQUIRE(h && out5, "NULL argument");
  out5[0] = h->run_bufs.spec_runs; out5[1] = h->run_bufs.spec_frozen; out5[2] = h->run_bufs.spec_short;
  out5[3] = h->run_bufs.last_plan_levels; out5[4] = (int64_t)h->run_bufs.last_plan_sparse;
  MGX_CATCH
}
int mgx_dbfs2_forget_plan(mgx_dbfs2_t h) {
  MGX_TRY
  MGX_REQUIRE(h, "NULL argument");
  h->run_bufs.hist_n = 0;
  MGX_CATCH
}
int mgx_dbfs2_run_group(mgx_dbfs2_t* hs, int count, int src_global, int64_t exchange_words, int64_t* out6_each) {
  MGX_TRY
  MGX_REQUIRE(hs && out6_each && count >= 1 && count <= 64, "mgx_dbfs2_run_group: 1..64 engines");
  mgx_dbfs2_t h0 = hs[0];
  MGX_REQUIRE(h0 && count == h0->st.ranks, "mgx_dbfs2_run_group: one engine per rank of the partition");
  MGX_REQUIRE(src_global >= 0 && src_global < h0->st.n_global, "mgx_dbfs2_run_group: bad source");
  MGX_REQUIRE(exchange_words >= h0->st.nwords && exchange_words % 4 == 0, "mgx_dbfs2_run_group: exchange_words must cover the bitmap");
  std::vector<mgx::d2_state_t*> sts((size_t)count);
  std::vector<mgx::d2_run_bufs_t*> bufs((size_t)count);
  for (int r = 0; r < count; ++r) {
    MGX_REQUIRE(hs[r] && hs[r]->c == h0->c && hs[r]->st.ranks == count && hs[r]->st.rank == r && hs[r]->st.n_global == h0->st.n_global &&
                (hs[r]->st.mylist != nullptr) == (h0->st.mylist != nullptr),
                "mgx_dbfs2_run_group: the engines must be ranks 0 .. count - 1 of one partition, on one context, all with or all without id lists");
    sts[(size_t)r] = &hs[r]->st; bufs[(size_t)r] = &hs[r]->run_bufs;
  }
  use_device(h0->c);
  std::vector<long long> o((size_t)count * 6, 0);
  mgx::d2_group_run(sts.data(), bufs.data(), h0->group_bufs, count, src_global, (long long)exchange_words, *h0->c->ctx, o.data());
  for (size_t i = 0; i < o.size(); ++i) out6_each[i] = o[i];
  MGX_CATCH
}
int mgx_dbfs2_words(int n_global, int64_t* words) {
  MGX_TRY
  MGX_REQUIRE(words && n_global > 0, "bad argument");
  *words = (((long long)n_global + 31) / 32 + 3) / 4 * 4;
  MGX_CATCH
}
int mgx_dbfs2_labels(mgx_dbfs2_t h, int* host_labels_local) {
  MGX_TRY
  MGX_REQUIRE(h && host_labels_local, "NULL argument");
  use_device(h->c);
  h->c->ctx->synchronize();
  MGX_HIP(mgx::dtoh(host_labels_local, h->st.labels.data(), (size_t)h->st.n_local));
  MGX_CATCH
}
int mgx_dbfs2_visited(mgx_dbfs2_t h, unsigned* host_words) {
  MGX_TRY
  MGX_REQUIRE(h && host_words, "NULL argument");
  use_device(h->c);
  h->c->ctx->synchronize();
  MGX_HIP(mgx::dtoh(host_words, h->st.fs->visited.data(), (size_t)h->st.nwords));
  MGX_CATCH
}

// ---- SSSP ----------------------------------------------------------------------------------
static void check_weights(mgx_graph_t g) {
  if (g->weights_checked) return;
  standard_context_t& ctx = *g->c->ctx;
  mem_t<int> flag = mgx::fill<int>(0, 1, ctx);
  int* pf = flag.data();
  const float* w = g->g->d_col_values.data();
  mgx::transform([=] __device__(int i) { if (!(w[i] >= 0.0f)) *pf = 1; }, g->g->num_edges, ctx);
  ctx.synchronize();
  g->weights_ok = (mgx::from_mem(flag)[0] == 0);
  g->weights_checked = true;
}

int mgx_sssp_create(mgx_graph_t g, int src, mgx_sssp_t* out) {
  MGX_TRY
  MGX_REQUIRE(g && out, "NULL argument");
  MGX_REQUIRE(src >= 0 && src < g->g->num_nodes, "mgx_sssp_create: src out of range");
  use_device(g->c);
  check_weights(g);
  if (!g->weights_ok) throw mgx::mgx_error(MGX_E_NEGATIVE_WEIGHT, "mgx_sssp_create: negative or NaN edge weight");
  auto* h = new mgx_sssp_s();
  h->g = g;
  h->p = std::make_shared<sssp::sssp_problem_t>(g->g, (size_t)src, *g->c->ctx);
  *out = h;
  MGX_CATCH
}
int mgx_sssp_reset(mgx_sssp_t p, int src) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(src >= 0 && src < p->g->g->num_nodes, "mgx_sssp_reset: src out of range");
  use_device(p->g->c);
  p->p->reset((size_t)src, *p->g->c->ctx);
  p->preds_stale = false;          // (-1 everywhere: what the operator path starts from)
  MGX_CATCH
}
int mgx_sssp_free(mgx_sssp_t p) {
  MGX_TRY
  if (p) { use_device(p->g->c); delete p; }
  MGX_CATCH
}
int mgx_sssp_distances(mgx_sssp_t p, float* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_labels.data(), p->n());
  MGX_CATCH
}
// the fused loop keeps no predecessors (sssp_fused.hpp); they are built from its distances the first time they are asked for
static void sssp_preds_if_stale(mgx_sssp_t p) {
  if (!p->preds_stale) return;
  graph_device_t& G = *p->g->g;
  mgx::sssp_build_preds(p->pred_state, G.d_row_offsets.data(), G.d_col_indices.data(), G.d_col_values.data(), p->p->d_labels.data(),
                        p->p->d_preds.data(), G.num_nodes, (long long)G.num_edges, p->preds_src, 3.402823466e+38f, *p->g->c->ctx);
  p->preds_stale = false;
}
int mgx_sssp_build_preds(mgx_sssp_t p, int64_t* stats2) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  sssp_preds_if_stale(p);
  if (stats2) { stats2[0] = p->pred_state.last_ties; stats2[1] = p->pred_state.last_rounds; }
  MGX_CATCH
}
int mgx_sssp_preds(mgx_sssp_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  use_device(p->g->c);
  sssp_preds_if_stale(p);
  read_back(p, host, p->p->d_preds.data(), p->n());
  MGX_CATCH
}
int mgx_sssp_distances_device(mgx_sssp_t p, float** d) {
  MGX_TRY
  MGX_REQUIRE(p && d, "NULL argument");
  *d = p->p->d_labels.data();
  MGX_CATCH
}
int mgx_sssp_advance(mgx_sssp_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* front) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::advance::advance_forward_kernel<sssp::sssp_problem_t, sssp::sssp_functor_t, false, true>(
      p->p, in->f, out->f, iteration, *p->g->c->ctx);
  if (front) *front = r;
  MGX_CATCH
}
int mgx_sssp_filter(mgx_sssp_t p, mgx_frontier_t in, mgx_frontier_t out, int iteration, int64_t* kept) {
  MGX_TRY
  MGX_REQUIRE(p && in && out, "NULL argument");
  use_device(p->g->c);
  const int r = oprtr::filter::filter_kernel<sssp::sssp_problem_t, sssp::sssp_functor_t>(p->p, in->f, out->f,
                                                                                       iteration, *p->g->c->ctx);
  if (kept) *kept = r;
  MGX_CATCH
}
int mgx_sssp_enact(mgx_sssp_t p, float queue_sizing, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p && queue_sizing > 0, "bad argument");
  use_device(p->g->c);
  standard_context_t& ctx = *p->g->c->ctx;
  if (!p->e || p->e_sizing != queue_sizing) {
    p->e.reset();
    p->e.reset(new sssp::sssp_enactor_t(ctx, p->g->g->num_nodes, p->g->g->num_edges, queue_sizing));
    p->e_sizing = queue_sizing;
  }
  p->e->enact(p->p, ctx);
  ctx.synchronize();
  if (stats) {
    stats[0] = p->e->iterations;
    stats[1] = p->e->relaxations;
    stats[2] = p->e->frontier_total;
  }
  MGX_CATCH
}
// Weights of the unit blocks' entries (mgx/sssp_fused.hpp: sssp_dense_long), once per graph at its first fused SSSP run:
// 4 bytes per padded long-row entry; skipped (the queue walk serves every iteration) when the memory is not there.
static void ensure_unit_weights(mgx_graph_s* g) {
  graph_device_t& G = *g->g;
  if (G.ub_w_tried) return;
  G.ub_w_tried = true;
  // (the sweep reads the long rows from the unit blocks and walks the short ones by degree class: any threshold the two were cut by together)
  if (!G.has_layout || !G.has_layout_weights || G.rows.ub.units <= 0 || !G.rows.ub.first.size() || G.rows.vs_long_min != G.rows.ub_min_degree || G.rows.vs_long_min < 17 || G.rows.vs_long_min > 64) return;
  if (const char* e = mgx::env("MGX_SSSP_DENSE")) if (atoi(e) == 0) return;
  standard_context_t& ctx = *g->c->ctx;
  float* w = nullptr;
  const size_t entries = ((size_t)G.rows.ub.units_pad << 6) + 4;
  if (hipMalloc((void**)&w, entries * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return; }
  G.d_ub_w = mem_t<float>::adopt(w, entries);
  MGX_HIP(hipMemsetAsync(w, 0, entries * sizeof(float), ctx.stream()));
  hipLaunchKernelGGL(mgx::k_sssp_unit_weights, dim3(4096), dim3(mgx::BLOCK), 0, ctx.stream(), G.d_layout_row_offsets.data(),
                     G.d_layout_col_values.data(), G.rows.ub.first.data(), G.num_nodes, w);
  MGX_CHECK_LAUNCH("unit-block weights");
  // ... and as halves, for the sweep's packed stream: only with the 24-bit entries, only when every weight survives the round trip
  G.d_ub_w16 = mem_t<unsigned short>();
  if (G.rows.ub.col24.size()) {
    mem_t<unsigned short> w16(entries + 8, ctx);
    mem_t<int> exact = mgx::fill<int>(1, 1, ctx);
    hipLaunchKernelGGL(mgx::k_sssp_unit_weights16, dim3(4096), dim3(mgx::BLOCK), 0, ctx.stream(), (const float*)w, (long long)entries, w16.data(), exact.data());
    int ok = 0;
    MGX_HIP(mgx::dtoh(&ok, exact.data(), 1));
    if (ok) G.d_ub_w16 = std::move(w16);
  }
}
int mgx_sssp_run(mgx_sssp_t p, int src, int64_t* stats) { return mgx_sssp_run_delta(p, src, -1.0f, stats); }
int mgx_sssp_run_delta(mgx_sssp_t p, int src, float delta, int64_t* stats) {
  // device-resident loop (include/mgx/sssp_fused.hpp): distances identical to mgx_sssp_enact's; predecessors are
  // left at -1 (the reference's are racy, the operator path keeps them)
  int rc = mgx_sssp_reset(p, src);
  if (rc != MGX_OK) return rc;
  MGX_TRY
  use_device(p->g->c);
  standard_context_t& ctx = *p->g->c->ctx;
  graph_device_t& G = *p->g->g;
  MGX_REQUIRE(G.d_col_values.size() >= (size_t)G.num_edges, "mgx_sssp_run: the graph has no weights");
  check_weights(p->g);
  MGX_REQUIRE(p->g->weights_ok, "mgx_sssp_run: negative or NaN weight");
  if (!p->fused) p->fused.reset(new mgx::sssp_fused_state_t(G.num_nodes, ctx));
  MGX_REQUIRE(!(delta != delta) && delta < 3e38f, "mgx_sssp_run_delta: delta must be a finite number (< 0: the default)");
  p->fused->delta = delta < 0.f ? 0.f : delta;
  mgx::sssp_layout_t layout;
  if (G.has_layout && G.has_layout_weights) {
    layout.row_offsets = G.d_layout_row_offsets.data();
    layout.col_indices = G.d_layout_col_indices.data();
    layout.weights = G.d_layout_col_values.data();
    layout.new_of_old = G.d_new_of_old.data();
    layout.old_of_new = G.d_old_of_new.data();
    ensure_unit_weights(p->g);
    if (G.d_ub_w.size()) {
      layout.ub_col = G.rows.ub.col.size() ? G.rows.ub.col.data() : nullptr; layout.ub_w = G.d_ub_w.data(); layout.ub_cnt = G.rows.ub.cnt.data(); layout.ub_owner = G.rows.ub.owner.data();
      if (G.rows.ub.col24.size()) layout.ub_col24 = G.rows.ub.col24.data();
      if (G.rows.ub.col24.size() && G.d_ub_w16.size()) layout.ub_w16 = G.d_ub_w16.data();
      layout.ub_units_pad = (unsigned)G.rows.ub.units_pad;
      for (int i = 0; i < 4; ++i) layout.vs_v[i] = G.rows.vs_v[i];
      layout.m_edges = (long long)G.num_edges;
    }
  }
  mgx::sssp_fused_run(*p->fused, G.d_row_offsets.data(), G.d_col_indices.data(), G.d_col_values.data(),
                      p->p->d_labels.data(), src, ctx, layout.row_offsets ? &layout : nullptr);
  p->preds_stale = true;           // (mgx_sssp_preds / mgx_sssp_build_preds: from these distances, mgx/sssp_preds.hpp)
  p->preds_src = src;
  if (stats) {
    stats[0] = p->fused->host_ctrl->levels;
    stats[1] = (int64_t)p->fused->host_ctrl->sum_edges;
    stats[2] = (int64_t)p->fused->host_ctrl->sum_frontier;
  }
  MGX_CATCH
}
int mgx_sssp_iteration_trace(mgx_sssp_t p, int cap, int64_t* frontier, int64_t* edges, float* ms, int* iterations) {
  MGX_TRY
  MGX_REQUIRE(p && iterations, "NULL argument");
  MGX_REQUIRE(p->fused != nullptr, "mgx_sssp_iteration_trace: no mgx_sssp_run yet");
  const mgx::bfs_ctrl_t* hc = p->fused->host_ctrl.data();
  const int it = hc->levels < 63 ? hc->levels : 63;
  *iterations = hc->levels;
  for (int i = 0; i < it && i < cap; ++i) {
    if (frontier) frontier[i] = (int64_t)(hc->trace[i] >> mgx::BFS_VSHIFT);
    if (edges) edges[i] = (int64_t)(hc->trace[i] & mgx::BFS_EMASK);
    if (ms) ms[i] = (hc->stamp[i + 1] >= hc->stamp[i] && hc->stamp[i + 1] != 0) ? (float)((double)(hc->stamp[i + 1] - hc->stamp[i]) / 1e5) : 0.f;
  }
  MGX_CATCH
}
int mgx_sssp_path_info(mgx_sssp_t p, int64_t* out8) {
  MGX_TRY
  MGX_REQUIRE(p && out8, "NULL argument");
  MGX_REQUIRE(p->fused != nullptr && p->fused->path.valid, "mgx_sssp_path_info: no mgx_sssp_run yet");
  use_device(p->g->c);
  MGX_REQUIRE(mgx::sssp_count_paths(*p->fused, *p->g->c->ctx), "mgx_sssp_path_info: the run had more iterations than the trace holds (4096)");
  const mgx::sssp_path_t& P = p->fused->path;
  out8[0] = P.sweep ? 1 : 0;
  out8[1] = P.variant;
  out8[2] = P.swept;
  out8[3] = P.walked_bounds;
  out8[4] = P.walked_plain;
  out8[5] = P.build_list ? 1 : 0;
  out8[6] = P.thr_moves;
  out8[7] = P.layout_space ? 1 : 0;
  MGX_CATCH
}
int mgx_sssp_set_kernel_timing(mgx_sssp_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  if (!p->fused) p->fused.reset(new mgx::sssp_fused_state_t(p->g->g->num_nodes, *p->g->c->ctx));
  p->fused->time_kernels = on != 0;
  MGX_CATCH
}
int mgx_sssp_kernel_times(mgx_sssp_t p, int64_t* out2) {
  MGX_TRY
  MGX_REQUIRE(p && out2, "NULL argument");
  MGX_REQUIRE(p->fused != nullptr, "mgx_sssp_kernel_times: no mgx_sssp_run yet");
  out2[0] = p->fused->relax_launches;
  out2[1] = (int64_t)(p->fused->relax_ms * 1e6);
  MGX_CATCH
}

// ---- PR ------------------------------------------------------------------------------------
int mgx_pr_create(mgx_graph_t g, int max_iter, mgx_pr_t* out) {
  MGX_TRY
  MGX_REQUIRE(g && out && max_iter >= 0, "bad argument");
  use_device(g->c);
  auto* h = new mgx_pr_s();
  h->g = g;
  h->p = std::make_shared<pr::pr_problem_t>(g->g, max_iter, *g->c->ctx);
  // the enactor with its frontiers (2 x num_edges ints, enactor.hxx:22-28) and the layout's sliced long rows belong to the set-up, as
  // in the reference's driver (tests/pr/test_pr.cu:32 constructs pr_enactor_t before the timer around enact starts, :34-37)
  h->e.reset(new pr::pr_enactor_t(*g->c->ctx, g->g->num_nodes, g->g->num_edges));
  ensure_nr_slices(g);
  *out = h;
  MGX_CATCH
}
int mgx_pr_free(mgx_pr_t p) {
  MGX_TRY
  if (p) { use_device(p->g->c); delete p; }
  MGX_CATCH
}
int mgx_pr_enact(mgx_pr_t p, int64_t* lens, int* iterations) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  use_device(p->g->c);
  standard_context_t& ctx = *p->g->c->ctx;
  if (!p->e) p->e.reset(new pr::pr_enactor_t(ctx, p->g->g->num_nodes, p->g->g->num_edges));
  ensure_nr_slices(p->g);
  p->e->enact(p->p, ctx);
  ctx.synchronize();
  if (iterations) *iterations = (int)p->e->frontier_lengths.size();
  if (lens)
    for (size_t i = 0; i < p->e->frontier_lengths.size(); ++i) lens[i] = p->e->frontier_lengths[i];
  MGX_CATCH
}
int mgx_pr_ranks(mgx_pr_t p, float* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_current_ranks.data(), p->n());
  MGX_CATCH
}


// ---- k-core ----------------------------------------------------------------------------------
int mgx_kcore_create(mgx_graph_t g, mgx_kcore_t* out) {
  MGX_TRY
  MGX_REQUIRE(g && out, "bad argument");
  use_device(g->c);
  auto* h = new mgx_kcore_s();
  h->g = g;
  h->p = std::make_shared<kcore::kcore_problem_t>(g->g, *g->c->ctx);
  *out = h;
  MGX_CATCH
}
int mgx_kcore_reset(mgx_kcore_t p) {
  MGX_TRY
  standard_context_t& ctx = enter(p).ctx;
  p->p->reset(ctx);
  MGX_CATCH
}
int mgx_kcore_free(mgx_kcore_t p) { return free_handle(p); }
int mgx_kcore_enact(mgx_kcore_t p, int* largest_k_core, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p && largest_k_core, "NULL argument");
  auto [ctx, g] = enter(p);
  if (!p->e) p->e.reset(new kcore::kcore_enactor_t(ctx, g.num_nodes, g.num_edges));
  p->e->enact(p->p, ctx);
  ctx.synchronize();
  *largest_k_core = p->p->largest_k_core;
  put_stats(stats, 4, {p->e->rounds, p->e->passes, p->e->expanded, p->e->removed});
  MGX_CATCH
}
int mgx_kcore_run(mgx_kcore_t p, int* largest_k_core, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p && largest_k_core, "NULL argument");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::kcore_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->p->reset(ctx);                               // every run starts afresh: core numbers 0, degrees = row lengths
  int largest = -1;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), p->p->d_degrees.data(),
                                                  p->p->d_num_cores.data(), ctx, largest);
  p->p->largest_k_core = largest;
  *largest_k_core = largest;
  put_stats(stats, 6, st);
  MGX_CATCH
}
int mgx_kcore_step_kinds(mgx_kcore_t p, int* host_kinds, int cap, int64_t* launches) {
  return chain_step_kinds(p, &mgx_kcore_s::fused, &mgx::kcore_fused_state_t::launches, "mgx_kcore_step_kinds", host_kinds, cap, launches);
}
int mgx_kcore_num_cores(mgx_kcore_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_num_cores.data(), p->n());
  MGX_CATCH
}
int mgx_kcore_degrees(mgx_kcore_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, p->p->d_degrees.data(), p->n());
  MGX_CATCH
}


// ---- graph colouring -------------------------------------------------------------------------
int mgx_color_create(mgx_graph_t g, mgx_color_t* out) { return create_handle(g, out); }
int mgx_color_free(mgx_color_t p) { return free_handle(p); }
int mgx_color_run(mgx_color_t p, unsigned seed, int max_iter, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::color_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->colors = nullptr;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), seed, max_iter, ctx, p->trace);
  p->colors = p->fused->colour.data();
  put_stats(stats, 4, st);
  MGX_CATCH
}
int mgx_color_enact(mgx_color_t p, unsigned seed, int max_iter, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  if (!p->p) p->p = std::make_shared<coloring::coloring_problem_t>(p->g->g, seed, max_iter, ctx);
  if (!p->e) p->e.reset(new coloring::coloring_enactor_t(ctx, g.num_nodes, g.num_edges));
  p->p->seed = seed;
  p->p->max_iter = max_iter;
  p->colors = nullptr;
  p->e->enact(p->p, ctx);
  ctx.synchronize();
  p->colors = p->p->d_colors.data();
  p->trace = p->e->trace;
  put_stats(stats, 4, {p->e->rounds, p->e->left, p->e->largest, p->e->waits});
  MGX_CATCH
}
int mgx_color_colors(mgx_color_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->colors, "mgx_color_colors");
  read_back(p, host, p->colors, p->n());
  MGX_CATCH
}
int mgx_color_colors_device(mgx_color_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->colors, "mgx_color_colors_device");
  *out = p->colors;
  MGX_CATCH
}
int mgx_color_round_trace(mgx_color_t p, int64_t* active_at_round_start, int cap, int* rounds) {
  MGX_TRY
  MGX_REQUIRE(p && rounds && (active_at_round_start || cap <= 0), "NULL argument");
  *rounds = (int)p->trace.size();
  for (int i = 0; i < cap && i < (int)p->trace.size(); ++i) active_at_round_start[i] = p->trace[i];
  MGX_CATCH
}
int mgx_color_info(mgx_color_t p, int64_t* consts4, int64_t* round_triples, int cap, int* rounds) {
  MGX_TRY
  MGX_REQUIRE(p && consts4 && rounds && (round_triples || cap <= 0), "NULL argument");
  MGX_REQUIRE(p->fused && p->fused->has_run, "mgx_color_info: no fused run yet");
  consts4[0] = mgx::COLOR_LONG_MIN;
  consts4[1] = mgx::COLOR_SEG;
  consts4[2] = mgx::COLOR_STAGE;
  consts4[3] = mgx::COLOR_BATCH_MAX;
  const std::vector<long long>& v = p->fused->round_rows;
  *rounds = (int)(v.size() / 3);
  for (int i = 0; i < cap && i < *rounds; ++i)
    for (int j = 0; j < 3; ++j) round_triples[3 * i + j] = v[3 * (size_t)i + j];
  MGX_CATCH
}


// ---- local graph sparsification ----------------------------------------------------------------
int mgx_lspar_create(mgx_graph_t g, mgx_lspar_t* out) { return create_handle(g, out); }
int mgx_lspar_free(mgx_lspar_t p) { return free_handle(p); }
static void lspar_check_params(int k, double e) {
  MGX_REQUIRE(k >= 1 && k <= mgx::LSPAR_K_MAX, "lspar: k must be 1 .. 32");
  MGX_REQUIRE(std::isfinite(e) && e >= 0.0, "lspar: e must be finite and >= 0");
}
int mgx_lspar_run(mgx_lspar_t p, unsigned seed, int k, double e, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  lspar_check_params(k, e);
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::lspar_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->ro = nullptr;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), seed, k, e, ctx);
  mgx::lspar_fused_state_t& f = *p->fused;
  p->ro = f.oro.data(); p->ci = f.oci.data(); p->eid = f.oeid.data(); p->sim = f.osim.data();
  p->mh = f.mh.data(); p->mh_stride = f.S; p->k = k; p->kept = st[0];
  put_stats(stats, 3, st);
  MGX_CATCH
}
int mgx_lspar_enact(mgx_lspar_t p, unsigned seed, int k, double e, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  lspar_check_params(k, e);
  auto [ctx, g] = enter(p);
  if (!p->p) p->p = std::make_shared<lspar::lspar_problem_t>(p->g->g, seed, k, e, ctx);
  else p->p->reset(seed, k, e, ctx);
  if (!p->e) p->e.reset(new lspar::lspar_enactor_t(ctx, g.num_nodes, g.num_edges));
  p->ro = nullptr;
  p->e->enact(p->p, ctx);
  ctx.synchronize();
  lspar::lspar_enactor_t& E = *p->e;
  p->ro = E.d_out_ro.data(); p->ci = E.d_out_ci.data(); p->eid = E.d_out_eid.data(); p->sim = E.d_out_sim.data();
  p->mh = p->p->d_minwise_hashs.data(); p->mh_stride = k; p->k = k; p->kept = E.kept;
  put_stats(stats, 3, {E.kept, E.cut, E.waits});
  MGX_CATCH
}
int mgx_lspar_result(mgx_lspar_t p, int* h_ro, int* h_ci, int* h_eid, int* h_sim) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->ro, "mgx_lspar_result");
  enter(p).ctx.synchronize();
  const size_t m = (size_t)p->kept;
  if (h_ro) MGX_HIP(mgx::dtoh(h_ro, p->ro, p->n() + 1));
  if (m) {
    if (h_ci) MGX_HIP(mgx::dtoh(h_ci, p->ci, m));
    if (h_eid) MGX_HIP(mgx::dtoh(h_eid, p->eid, m));
    if (h_sim) MGX_HIP(mgx::dtoh(h_sim, p->sim, m));
  }
  MGX_CATCH
}
int mgx_lspar_result_device(mgx_lspar_t p, const int** d_ro, const int** d_ci, const int** d_eid, const int** d_sim) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->ro, "mgx_lspar_result_device");
  if (d_ro) *d_ro = p->ro;
  if (d_ci) *d_ci = p->ci;
  if (d_eid) *d_eid = p->eid;
  if (d_sim) *d_sim = p->sim;
  MGX_CATCH
}
int mgx_lspar_minhashes(mgx_lspar_t p, unsigned* h) {
  MGX_TRY
  MGX_REQUIRE(p && h, "NULL argument");
  require_run(p->ro, "mgx_lspar_minhashes");
  enter(p).ctx.synchronize();
  const size_t n = p->n();
  if (n)
    MGX_HIP(hipMemcpy2D(h, (size_t)p->k * sizeof(unsigned), p->mh, (size_t)p->mh_stride * sizeof(unsigned), (size_t)p->k * sizeof(unsigned),
                        n, hipMemcpyDeviceToHost));
  MGX_CATCH
}
int mgx_lspar_info(mgx_lspar_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  MGX_REQUIRE(p->fused && p->fused->last_items >= 0, "mgx_lspar_info: no fused run yet");
  out[0] = mgx::LSPAR_SHORT_MAX;
  out[1] = mgx::LSPAR_SEG;
  out[2] = mgx::LSPAR_K_MAX;
  out[3] = p->fused->S;
  out[4] = p->fused->last_items;
  MGX_CATCH
}
int mgx_lspar_graph(mgx_lspar_t p, mgx_graph_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->ro, "mgx_lspar_graph");
  mgx_ctx_s* const c = p->g->c;
  use_device(c);
  standard_context_t& ctx = *c->ctx;
  const graph_device_t& in = *p->g->g;
  const int n = in.num_nodes;
  const long long m = p->kept;
  auto g = std::make_shared<graph_device_t>();
  g->num_nodes = n;
  g->num_edges = (int)m;
  g->d_row_offsets = mem_t<int>((size_t)n + 1, ctx);
  MGX_HIP(mgx::dtod(g->d_row_offsets.data(), p->ro, (size_t)n + 1, ctx.stream()));
  g->d_col_indices = mem_t<int>((size_t)m, ctx);
  g->d_col_values = mem_t<float>((size_t)m, ctx);
  if (m) {
    MGX_HIP(mgx::dtod(g->d_col_indices.data(), p->ci, (size_t)m, ctx.stream()));
    const float* const w = in.d_col_values.data();
    const int* const eid = p->eid;
    float* const kw = g->d_col_values.data();
    transform([=] __device__(int i) { kw[i] = w[eid[i]]; }, m, ctx);
  }
  g->d_col_offsets = mem_t<int>::borrow(g->d_row_offsets.data(), g->d_row_offsets.size());
  g->d_row_indices = mem_t<int>::borrow(g->d_col_indices.data(), g->d_col_indices.size());
  g->d_row_values = mem_t<float>::borrow(g->d_col_values.data(), g->d_col_values.size());
  g->csc_is_csr = true;
  finish_graph(c, *g);
  ctx.synchronize();
  auto* h = new mgx_graph_s();
  h->c = c;
  h->g = g;
  *out = h;
  MGX_CATCH
}

// ---- segmented sort ----------------------------------------------------------------------------
int mgx_segmented_sort_i32(mgx_ctx_t c, int* d_keys, int* d_vals, int64_t count, const int* d_segments, int num_segments,
                           int descending) {
  MGX_TRY
  MGX_REQUIRE(c && (d_keys || count == 0) && (d_segments || num_segments == 0) && count >= 0 && num_segments >= 0,
              "mgx_segmented_sort_i32: bad argument");
  MGX_REQUIRE(count <= 2147483647LL, "mgx_segmented_sort_i32: count must fit int32");
  use_device(c);
  standard_context_t& ctx = *c->ctx;
  auto up = [] __device__(int a, int b) { return a < b; };
  auto down = [] __device__(int a, int b) { return a > b; };
  if (d_vals) {
    if (descending) mgx::segmented_sort(d_keys, d_vals, count, d_segments, num_segments, down, ctx);
    else mgx::segmented_sort(d_keys, d_vals, count, d_segments, num_segments, up, ctx);
  } else {
    if (descending) mgx::segmented_sort(d_keys, count, d_segments, num_segments, down, ctx);
    else mgx::segmented_sort(d_keys, count, d_segments, num_segments, up, ctx);
  }
  MGX_CATCH
}


// ---- connected components ----------------------------------------------------------------------
int mgx_cc_create(mgx_graph_t g, mgx_cc_t* out) { return create_handle(g, out); }
int mgx_cc_free(mgx_cc_t p) { return free_handle(p); }
int mgx_cc_run(mgx_cc_t p, int symmetric, unsigned seed, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::cc_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->labels = nullptr;
  const bool csc = !g.csc_is_csr;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), csc ? g.d_col_offsets.data() : nullptr,
                                                  csc ? g.d_row_indices.data() : nullptr, symmetric != 0, seed, ctx);
  p->labels = p->fused->comp.data();
  put_stats(stats, 5, st);
  MGX_CATCH
}
int mgx_cc_enact(mgx_cc_t p, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  if (!p->p) p->p = std::make_shared<cc::cc_problem_t>(p->g->g, ctx);
  if (!p->e) p->e.reset(new cc::cc_enactor_t(ctx, g.num_nodes, g.num_edges));
  if (!p->label_stats) p->label_stats.reset(new mgx::cc_label_stats_t(g.num_nodes, ctx));
  p->labels = nullptr;
  p->e->enact(p->p, ctx);
  const std::vector<long long> st = p->label_stats->run(p->p->d_comp.data(), g.num_nodes, ctx);
  p->labels = p->p->d_comp.data();
  put_stats(stats, 5, {st[0], st[1], st[2], 0, p->e->waits + 1});
  MGX_CATCH
}
int mgx_cc_labels(mgx_cc_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->labels, "mgx_cc_labels");
  read_back(p, host, p->labels, p->n());
  MGX_CATCH
}
int mgx_cc_labels_device(mgx_cc_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->labels, "mgx_cc_labels_device");
  *out = p->labels;
  MGX_CATCH
}

// ---- triangle counting -------------------------------------------------------------
int mgx_tc_create(mgx_graph_t g, mgx_tc_t* out) { return create_handle(g, out); }
int mgx_tc_free(mgx_tc_t p) { return free_handle(p); }
static mgx::tc_state_t& tc_state(mgx_tc_t p) {
  if (!p->st) p->st.reset(new mgx::tc_state_t(p->graph().num_nodes, p->graph().num_edges, p->ctx()));
  return *p->st;
}
int mgx_tc_run(mgx_tc_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  put_stats(stats, 8, tc_state(p).run(g.d_row_offsets.data(), g.d_col_indices.data(), symmetric != 0, ctx));
  MGX_CATCH
}
int mgx_tc_enact(mgx_tc_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  mgx::tc_state_t& st = tc_state(p);
  const int sym = symmetric != 0 ? 1 : 0;
  st.launches = st.waits = 0;
  st.last = -1;
  if (st.n <= 0) { put_stats(stats, 8, {0, 0, 0, 0, sym, 0, 0, 0}); return MGX_OK; }
  mgx::tc_dag_t& d = st.dag[sym];
  bool built_now = false;
  {
    mgx::tc_build_tmp_t tmp;
    built_now = st.ensure_dag(sym != 0, g.d_row_offsets.data(), g.d_col_indices.data(), tmp, ctx);
    if (built_now) st.read_stats(d, true, ctx);        // (the operator needs m_dag on the host; the build's scratch goes behind the wait)
  }
  const hipStream_t s = ctx.stream();
  // the operator's view of the DAG borrows its arrays: a new one whenever they are not the ones it holds (either path may have rebuilt)
  std::shared_ptr<tc::tc_problem_t>& view = p->p[sym];
  if (!view || view->gslice->d_row_offsets.data() != d.ro.data() || view->gslice->d_col_indices.data() != d.ci.data()) {
    view = std::make_shared<tc::tc_problem_t>(d.ro.data(), d.ci.data(), st.n, (int)d.h[mgx::TC_S_MDAG], st.tri.data(), ctx);
    ++st.waits;                                        // (its data slice goes up with a blocking copy)
  }
  if (!p->e) p->e.reset(new tc::tc_enactor_t(ctx, st.n));
  MGX_HIP(hipMemsetAsync(st.tri.data(), 0, (size_t)st.n * sizeof(mgx::u64), s));
  MGX_HIP(hipMemsetAsync(d.stat.data() + mgx::TC_S_TOTAL, 0, sizeof(mgx::u64), s));
  p->e->enact(view, ctx);
  st.waits += p->e->waits;
  hipLaunchKernelGGL(mgx::k_tc_sum, dim3(grid_for(st.n, mgx::BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(mgx::BLOCK), 0, s,
                     (const mgx::u64*)st.tri.data(), st.n, d.stat.data());
  MGX_CHECK_LAUNCH("mgx tc enact");
  // two clears, the degree scan over the n rows (one launch, or three above the look-back's tile limit), the expansion, the sum
  st.launches += 2 + (mgx::scan_num_tiles(st.n) <= mgx::SCAN_LOOKBACK_MAX_TILES ? 1 : 3) + 1 + 1;
  st.read_stats(d, false, ctx);
  st.last = sym;
  put_stats(stats, 8, st.result(d, d.h[mgx::TC_S_TOTAL] / 3, built_now));
  MGX_CATCH
}
static mgx::tc_dag_t& tc_last(mgx_tc_t p, const char* who) {
  require_run(p->st && p->st->last >= 0, who);
  return p->st->dag[p->st->last];
}
int mgx_tc_triangles(mgx_tc_t p, int64_t* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  tc_last(p, "mgx_tc_triangles");
  read_back(p, (mgx::u64*)host, (const mgx::u64*)p->st->tri.data(), (size_t)p->st->n);
  MGX_CATCH
}
int mgx_tc_triangles_device(mgx_tc_t p, const int64_t** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  tc_last(p, "mgx_tc_triangles_device");
  *out = (const int64_t*)p->st->tri.data();
  MGX_CATCH
}
int mgx_tc_simple_degrees(mgx_tc_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  read_back(p, host, (const int*)tc_last(p, "mgx_tc_simple_degrees").sdeg.data(), (size_t)p->st->n);
  MGX_CATCH
}
int mgx_tc_simple_degrees_device(mgx_tc_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  *out = tc_last(p, "mgx_tc_simple_degrees_device").sdeg.data();
  MGX_CATCH
}
int mgx_tc_bins(mgx_tc_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  tc_last(p, "mgx_tc_bins");
  put_stats(out, 7, p->st->bins(enter(p).ctx));
  MGX_CATCH
}
int mgx_tc_dag(mgx_tc_t p, int* h_ro, int* h_ci) {
  MGX_TRY
  MGX_REQUIRE(p && h_ro, "NULL argument");
  mgx::tc_dag_t& d = tc_last(p, "mgx_tc_dag");
  read_back(p, h_ro, (const int*)d.ro.data(), (size_t)p->st->n + 1);
  if (h_ci) read_back(p, h_ci, (const int*)d.ci.data(), (size_t)d.h[mgx::TC_S_MDAG]);
  MGX_CATCH
}

// ---- betweenness centrality --------------------------------------------------------
int mgx_bc_create(mgx_graph_t g, mgx_bc_t* out) { return create_handle(g, out); }
int mgx_bc_free(mgx_bc_t p) { return free_handle(p); }
// the checks both paths make before any device work; the sources as a list
static std::vector<int> bc_sources(mgx_bc_t p, const int* sources, int count, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  const int n = p->g->g->num_nodes;
  MGX_REQUIRE(count >= 0, std::string(who) + ": negative count");
  std::vector<int> s;
  if (!sources) {
    s.resize((size_t)n);
    for (int i = 0; i < n; ++i) s[(size_t)i] = i;
  } else {
    for (int i = 0; i < count; ++i) MGX_REQUIRE(sources[i] >= 0 && sources[i] < n, std::string(who) + ": source out of range");
    s.assign(sources, sources + count);
  }
  return s;
}
static mgx::bc_state_t& bc_state(mgx_bc_t p) {
  if (!p->st) p->st.reset(new mgx::bc_state_t(p->graph().num_nodes, p->ctx()));
  if (!p->bp) p->bp = std::make_shared<bfs::bfs_problem_t>(p->g->g, 0, p->ctx());
  return *p->st;
}
static void bc_stats(int64_t* stats, const mgx::bc_state_t& st, const mgx::bc_ctrl_t& c, long long traversal_waits) {
  put_stats(stats, 10, {st.sources, c.deepest, st.reached, c.inexact ? 1 : 0, c.overflow ? 1 : 0, st.waits, traversal_waits, st.launches,
                    st.chain_launches, st.used_csc});
}
int mgx_bc_run(mgx_bc_t p, const int* sources, int count, int symmetric, int64_t* stats) {
  MGX_TRY
  const std::vector<int> srcs = bc_sources(p, sources, count, "mgx_bc_run");
  MGX_REQUIRE(symmetric || !p->g->g->csc_is_csr, "mgx_bc_run: symmetric = 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  auto [ctx, G] = enter(p);
  mgx::bc_state_t& st = bc_state(p);
  const bool sym = symmetric != 0;
  st.ensure_rows(sym, G.d_row_offsets.data(), G.d_col_indices.data(), G.d_col_offsets.data(), G.d_row_indices.data(), ctx);
  if (!p->fe && G.num_edges > 0) p->fe.reset(new bfs::bfs_fused_enactor_t(ctx, G.num_nodes));
  st.begin_run(sym, ctx);
  long long traversal_waits = 0;
  const std::vector<std::pair<long long, long long>> no_trace;
  int* const labels = p->bp->d_labels.data();
  for (size_t i = 0; i < srcs.size(); ++i) {
    const int src = srcs[i];
    st.mark(0, ctx.stream());
    if (G.num_edges > 0) {
      // the fused BFS in push mode; it waits for the host as it always does (and with that for the launches of the source before)
      p->bp->src = src;
      p->fe->fused->time_kernels = 0;
      p->fe->enact(p->bp, ctx, false, 0.f);
      traversal_waits += p->fe->fused->batches + (p->fe->last.levels > 64 ? 1 : 0);
      st.reached += p->fe->last.reached;
      st.source(labels, src, p->fe->last.levels, p->fe->last.trace, sym, ctx);
    } else {                                                       // a graph without entries: the source alone
      MGX_HIP(hipMemsetAsync(labels, 0xFF, (size_t)G.num_nodes * sizeof(int), ctx.stream()));
      MGX_HIP(hipMemsetAsync(labels + src, 0, sizeof(int), ctx.stream()));
      st.reached += 1;
      st.source(labels, src, 0, no_trace, sym, ctx);
    }
  }
  mgx::bc_ctrl_t c = {};
  if (!srcs.empty()) c = st.end_run(ctx);
  st.ran = true;
  st.last_chain_launches = srcs.empty() ? 0 : st.last_chain_launches;
  p->last_sym = sym ? 1 : 0;
  p->last_levels = c.last_levels;
  bc_stats(stats, st, c, traversal_waits);
  MGX_CATCH
}
int mgx_bc_enact(mgx_bc_t p, const int* sources, int count, int symmetric, int64_t* stats) {
  MGX_TRY
  const std::vector<int> srcs = bc_sources(p, sources, count, "mgx_bc_enact");
  (void)symmetric;                                                 // (the operator path reads the out-entries alone)
  auto [ctx, G] = enter(p);
  mgx::bc_state_t& st = bc_state(p);
  const int n = G.num_nodes;
  if (!p->p) p->p = std::make_shared<bc::bc_problem_t>(p->g->g, p->bp->d_labels.data(), st.sigma.data(), const_cast<double*>(st.delta()), ctx);
  if (!p->e) p->e.reset(new bc::bc_enactor_t(ctx, n, G.num_edges));
  st.begin_run(true, ctx);
  const bool was_timing = st.timing;
  st.timing = false;                                               // (the phase events belong to the fused path)
  st.launches = 0;                                                 // (the operators' launches are not counted)
  p->e->waits = 0;
  int deepest = 0, levels = 0;
  double* const bcv = st.bc.data();
  const double* const delta = st.delta();
  const double* const sigma = st.sigma.data();
  mgx::bc_ctrl_t* const dc = st.ctrl.data();
  for (size_t i = 0; i < srcs.size(); ++i) {
    levels = p->e->enact(p->p, srcs[i], ctx);
    deepest = std::max(deepest, levels);
    st.reached += (long long)p->e->level_off.back();
    mgx::transform([=] __device__(int v) {
      bcv[v] += delta[v];
      const double s = sigma[v];
      if (s >= mgx::BC_TWO53) dc->inexact = 1u;
      if (!(s <= 1.7976931348623157e308)) dc->overflow = 1u;
    }, n, ctx);
    ++st.sources;
  }
  MGX_CHECK_LAUNCH("mgx bc enact");
  mgx::bc_ctrl_t c = {};
  if (!srcs.empty()) c = st.end_run(ctx);
  st.ran = true;
  st.timing = was_timing;
  c.deepest = deepest;
  p->last_levels = levels;
  st.waits += p->e->waits;
  bc_stats(stats, st, c, 0);
  MGX_CATCH
}
static mgx::bc_state_t& bc_last(mgx_bc_t p, const char* who) {
  require_run(p->st && p->st->ran, who);
  return *p->st;
}
int mgx_bc_centrality(mgx_bc_t p, double* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_centrality");
  read_back(p, host, (const double*)st.bc.data(), (size_t)st.n);
  MGX_CATCH
}
int mgx_bc_centrality_device(mgx_bc_t p, const double** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  *out = bc_last(p, "mgx_bc_centrality_device").bc.data();
  MGX_CATCH
}
int mgx_bc_sigma(mgx_bc_t p, double* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_sigma");
  read_back(p, host, (const double*)st.sigma.data(), (size_t)st.n);
  MGX_CATCH
}
int mgx_bc_delta(mgx_bc_t p, double* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_delta");
  read_back(p, host, (const double*)st.delta(), (size_t)st.n);
  MGX_CATCH
}
int mgx_bc_labels(mgx_bc_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_labels");
  read_back(p, host, (const int*)p->bp->d_labels.data(), (size_t)st.n);
  MGX_CATCH
}
int mgx_bc_set_timing(mgx_bc_t p, int on) {
  MGX_TRY
  enter(p);
  bc_state(p).timing = on != 0;
  MGX_CATCH
}
int mgx_bc_phase_ms(mgx_bc_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_phase_ms");
  for (int k = 0; k < 4; ++k) out[k] = st.timed > 0 ? st.phase_ms[k] / st.timed : 0.0;
  out[4] = (double)st.timed;
  MGX_CATCH
}
int mgx_bc_info(mgx_bc_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  mgx::bc_state_t& st = bc_last(p, "mgx_bc_info");
  for (int i = 0; i < mgx::BC_INFO_WORDS; ++i) out[i] = 0;
  if (p->last_sym >= 0) {
    const mgx::bc_rows_t& rin = p->last_sym ? st.rows_sym : st.rows[0];
    const mgx::bc_rows_t& rout = p->last_sym ? st.rows_sym : st.rows[1];
    for (int k = 0; k < 3; ++k) { out[k] = rin.count[k]; out[3 + k] = rout.count[k]; }
    out[6] = rin.segments; out[7] = rout.segments;
    out[14] = rin.longest; out[15] = rout.longest;
  }
  out[8] = st.opts.lane_max; out[9] = st.opts.huge_min; out[10] = st.opts.seg; out[11] = st.opts.chain;
  out[12] = p->last_levels; out[13] = st.last_chain_launches;
  MGX_CATCH
}

// ---- PageRank to convergence --------------------------------------------------------
int mgx_pagerank_create(mgx_graph_t g, mgx_pagerank_t* out) { return create_handle(g, out); }
int mgx_pagerank_free(mgx_pagerank_t p) { return free_handle(p); }
// the arguments both paths refuse before any device work
static void pagerank_check(mgx_pagerank_t p, double alpha, double tol, int max_iter, int symmetric, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(alpha >= 0.0 && alpha < 1.0, std::string(who) + ": alpha must be in [0, 1)");
  MGX_REQUIRE(tol >= 0.0 && std::isfinite(tol), std::string(who) + ": tol must be finite and >= 0");
  MGX_REQUIRE(max_iter >= 1, std::string(who) + ": max_iter must be >= 1");
  MGX_REQUIRE(symmetric != 0 || !p->g->g->csc_is_csr,
              std::string(who) + ": symmetric = 0 needs the graph's genuine CSC for the in-entries (mgx_graph_build_csc, or upload one); "
                                 "pass symmetric = 1 only if every entry has its reverse");
}
static void pagerank_stats(int64_t* stats, double* residual, const mgx::pagerank_stats_t& s) {
  put_stats(stats, 6, {s.iterations, s.converged, s.dangling, s.layout_path, s.waits, s.launches});
  if (residual) *residual = s.residual;
}
int mgx_pagerank_run(mgx_pagerank_t p, double alpha, double tol, int max_iter, int symmetric, int64_t* stats, double* residual) {
  MGX_TRY
  pagerank_check(p, alpha, tol, max_iter, symmetric, "mgx_pagerank_run");
  auto [ctx, G] = enter(p);
  if (!p->p) p->p = std::make_shared<pagerank::pagerank_problem_t>(p->g->g, ctx);
  mgx::pagerank_graph_t pg;
  mgx::nr_layout_t L;
  pg.out_off = G.d_row_offsets.data();
  pg.in_off = symmetric ? G.d_row_offsets.data() : G.d_col_offsets.data();
  pg.in_idx = symmetric ? G.d_col_indices.data() : G.d_row_indices.data();
  pg.in_entries = G.num_edges;
  // the layout reduce only with the long rows by slice (and 4-byte values); otherwise the general reduce serves
  if (symmetric && G.has_layout && G.num_edges > 0) {
    ensure_nr_slices(p->g);
    if (mgx::nr_units_valid(G)) L = mgx::nr_layout_of(G, ctx, sizeof(float), true);
    if (L.nrs_mu) {
      pg.layout = &L;
      pg.old_of_new = G.d_old_of_new.data();
    }
  }
  pagerank_stats(stats, residual, p->p->state.run(pg, alpha, tol, max_iter, ctx));
  MGX_CATCH
}
int mgx_pagerank_enact(mgx_pagerank_t p, double alpha, double tol, int max_iter, int symmetric, int64_t* stats, double* residual) {
  MGX_TRY
  pagerank_check(p, alpha, tol, max_iter, symmetric, "mgx_pagerank_enact");
  auto [ctx, G] = enter(p);
  if (!p->p) p->p = std::make_shared<pagerank::pagerank_problem_t>(p->g->g, ctx);
  if (!p->e) p->e.reset(new pagerank::pagerank_enactor_t(ctx, G.num_nodes, G.num_edges));
  if (G.has_layout && G.csc_is_csr) ensure_nr_slices(p->g);      // (the operator's full-frontier reduce may take them)
  pagerank_stats(stats, residual, p->e->enact(p->p, alpha, tol, max_iter, ctx));
  MGX_CATCH
}
int mgx_pagerank_ranks(mgx_pagerank_t p, float* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->p && p->p->state.result, "mgx_pagerank_ranks");
  read_back(p, host, (const float*)p->p->state.result, p->n());
  MGX_CATCH
}
int mgx_pagerank_ranks_device(mgx_pagerank_t p, const float** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->p && p->p->state.result, "mgx_pagerank_ranks_device");
  *out = p->p->state.result;
  MGX_CATCH
}
int mgx_pagerank_residuals(mgx_pagerank_t p, double* host_e, int cap, int* iterations) {
  MGX_TRY
  MGX_REQUIRE(p && cap >= 0 && (host_e || cap == 0), "bad argument");
  require_run(p->p && p->p->state.result, "mgx_pagerank_residuals");
  mgx::pagerank_state_t& s = p->p->state;
  if (iterations) *iterations = s.last_iterations;
  read_back(p, host_e, (const double*)s.trace.data(), (size_t)std::max(std::min(std::min(cap, s.last_iterations), s.trace_cap), 0));
  MGX_CATCH
}
int mgx_pagerank_bins(mgx_pagerank_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->p && p->p->state.last_huge_rows >= 0, "mgx_pagerank_bins");
  put_stats(out, 4, p->p->state.bins());
  MGX_CATCH
}


// ---- minimum spanning forest -----------------------------------------------------------
int mgx_mst_create(mgx_graph_t g, mgx_mst_t* out) { return create_handle(g, out); }
int mgx_mst_free(mgx_mst_t p) { return free_handle(p); }
int mgx_mst_run(mgx_mst_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  p->ready = false;
  const bool csc = !g.csc_is_csr;
  MGX_REQUIRE(symmetric || csc, "mgx_mst_run: symmetric == 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  MGX_REQUIRE(g.d_col_values.size() >= (size_t)g.num_edges && (!csc || g.d_row_values.size() >= (size_t)g.num_edges), "mgx_mst_run: the graph has no weights");
  if (!p->fused) p->fused.reset(new mgx::mst_fused_state_t(g.num_nodes, g.num_edges, ctx));
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_values.data(),
                                                  csc ? g.d_col_offsets.data() : nullptr, csc ? g.d_row_indices.data() : nullptr,
                                                  csc ? g.d_row_values.data() : nullptr, symmetric != 0, ctx);
  p->labels = p->fused->comp.data();
  p->a = p->fused->out_a.data(); p->b = p->fused->out_b.data(); p->w = p->fused->out_w.data();
  p->edges = st[0];
  p->total = p->fused->total();
  p->ready = true;
  put_stats(stats, 8, st);
  MGX_CATCH
}
int mgx_mst_enact(mgx_mst_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  p->ready = false;
  MGX_REQUIRE(symmetric || !g.csc_is_csr, "mgx_mst_enact: symmetric == 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  MGX_REQUIRE(g.d_col_values.size() >= (size_t)g.num_edges, "mgx_mst_enact: the graph has no weights");
  const int n = g.num_nodes;
  if (n <= 0) {
    p->labels = nullptr; p->a = p->b = nullptr; p->w = nullptr; p->edges = 0; p->total = 0.0;
    p->ready = true;
    put_stats(stats, 8, {0, 0, 0, 0, 0, 0, 0, 0});
    return MGX_OK;
  }
  if (!p->p) p->p = std::make_shared<mst::mst_problem_t>(p->g->g, ctx);
  if (!p->e) p->e.reset(new mst::mst_enactor_t(ctx, n, g.num_edges));
  if (!p->label_stats) p->label_stats.reset(new mgx::cc_label_stats_t(n, ctx));
  if (!p->stat.size()) {
    p->stat = mem_t<mgx::u64>(mgx::MST_S_WORDS, ctx);
    p->tile_sum = mem_t<double>((size_t)n / mgx::MST_SUM_TILE + 2, ctx);
  }
  p->e->enact(p->p, symmetric != 0, ctx);
  const hipStream_t s = ctx.stream();
  mgx::mst_sum_list(p->p->d_w_out.data(), (const long long*)p->p->d_counters.data(), (long long)n, p->tile_sum.data(), nullptr,
                    (const mgx::u64*)(p->p->d_counters.data() + 2), nullptr, n, p->stat.data(), s);
  MGX_CHECK_LAUNCH("mgx mst enact");
  mgx::u64 h[mgx::MST_S_WORDS];
  mgx::u64 counters[4];
  long long waits = p->e->waits;                                  // the operators' read-backs, one a call
  MGX_HIP(mgx::dtoh(h, (const mgx::u64*)p->stat.data(), (size_t)mgx::MST_S_WORDS, s));
  ++waits;
  MGX_HIP(mgx::dtoh(counters, (const mgx::u64*)p->p->d_counters.data(), (size_t)4, s));
  ++waits;
  MGX_REQUIRE(h[mgx::MST_S_NAN] == 0, "mgx_mst_enact: a NaN edge weight");
  const std::vector<long long> ls = p->label_stats->run(p->p->d_root.data(), n, ctx);
  ++waits;
  p->labels = p->p->d_root.data();
  p->a = p->p->d_a.data(); p->b = p->p->d_b.data(); p->w = p->p->d_w_out.data();
  p->edges = (long long)h[mgx::MST_S_EDGES];
  std::memcpy(&p->total, &h[mgx::MST_S_TOTAL], sizeof(double));
  p->ready = true;
  put_stats(stats, 8, {p->edges, ls[0], ls[1], ls[2], p->e->rounds, waits, 0, (long long)counters[1]});
  MGX_CATCH
}
int mgx_mst_edges(mgx_mst_t p, int* h_a, int* h_b, float* h_w) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->ready, "mgx_mst_edges");
  enter(p).ctx.synchronize();
  const size_t k = (size_t)p->edges;
  if (h_a && k) MGX_HIP(mgx::dtoh(h_a, p->a, k));
  if (h_b && k) MGX_HIP(mgx::dtoh(h_b, p->b, k));
  if (h_w && k) MGX_HIP(mgx::dtoh(h_w, p->w, k));
  MGX_CATCH
}
int mgx_mst_edges_device(mgx_mst_t p, const int** d_a, const int** d_b, const float** d_w) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->ready, "mgx_mst_edges_device");
  if (d_a) *d_a = p->a;
  if (d_b) *d_b = p->b;
  if (d_w) *d_w = p->w;
  MGX_CATCH
}
int mgx_mst_weight(mgx_mst_t p, double* total) {
  MGX_TRY
  MGX_REQUIRE(p && total, "NULL argument");
  require_run(p->ready, "mgx_mst_weight");
  *total = p->total;
  MGX_CATCH
}
int mgx_mst_labels(mgx_mst_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->ready, "mgx_mst_labels");
  read_back(p, host, p->labels, (size_t)std::max(p->graph().num_nodes, 0));
  MGX_CATCH
}
int mgx_mst_labels_device(mgx_mst_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->ready, "mgx_mst_labels_device");
  *out = p->labels;
  MGX_CATCH
}
int mgx_mst_info(mgx_mst_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  MGX_REQUIRE(p->fused, "mgx_mst_info: no fused run yet");
  put_stats(out, 8, p->fused->info());
  MGX_CATCH
}

// ---- k-truss decomposition -----------------------------------------------------------
int mgx_ktruss_create(mgx_graph_t g, mgx_ktruss_t* out) { return create_handle(g, out); }
int mgx_ktruss_free(mgx_ktruss_t p) { return free_handle(p); }
static mgx::ktruss_state_t& ktruss_state(mgx_ktruss_t p) {
  if (!p->st) p->st.reset(new mgx::ktruss_state_t(p->graph().num_nodes, p->graph().num_edges, p->ctx()));
  return *p->st;
}
int mgx_ktruss_run(mgx_ktruss_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  put_stats(stats, 8, ktruss_state(p).run(g.d_row_offsets.data(), g.d_col_indices.data(), symmetric != 0, ctx));
  MGX_CATCH
}
int mgx_ktruss_enact(mgx_ktruss_t p, int symmetric, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  mgx::ktruss_state_t& st = ktruss_state(p);
  const int sym = symmetric != 0 ? 1 : 0;
  st.start_run();
  if (st.n <= 0) { put_stats(stats, 8, {0, 0, 0, 0, 0, 0, 0, 0}); return MGX_OK; }
  const bool built_now = st.ensure_graph(sym != 0, g.d_row_offsets.data(), g.d_col_indices.data(), ctx);
  mgx::ktruss_graph_t& kg = st.gr[sym];
  mgx::tc_dag_t& d = st.tc.dag[sym];
  const hipStream_t s = ctx.stream();
  // the operator's view borrows the arrays: a new one whenever they are not the ones it holds (either path may have rebuilt)
  std::shared_ptr<ktruss::ktruss_problem_t>& view = p->p[sym];
  if (!view || view->gslice->d_row_offsets.data() != d.ro.data() || view->gslice->d_col_indices.data() != d.ci.data()) {
    const ktruss::ktruss_problem_t::data_slice_t slice = {d.ro.data(), d.ci.data(), kg.src.data(), kg.adj_ro.data(), kg.adj_ci.data(),
                                                          kg.adj_eid.data(), kg.sup0.data(), kg.sup.data(), kg.state.data(),
                                                          kg.truss.data(), st.vtruss.data(), st.hist.data()};
    view = std::make_shared<ktruss::ktruss_problem_t>(slice, st.n, kg.m, ctx);
    ++st.tc.waits;                                     // (its data slice goes up with a blocking copy)
    p->e[sym].reset(new ktruss::ktruss_enactor_t(ctx, std::max(std::max(st.n, kg.m), 1)));
  }
  ktruss::ktruss_enactor_t& e = *p->e[sym];
  e.waits = e.calls = 0;
  MGX_HIP(hipMemsetAsync(kg.sup0.data(), 0, (size_t)std::max(kg.m, 1) * sizeof(int), s));
  MGX_HIP(hipMemsetAsync(d.stat.data() + mgx::TC_S_TOTAL, 0, sizeof(mgx::u64), s));
  e.supports(view, ctx);
  hipLaunchKernelGGL(mgx::k_ktruss_sum, dim3(grid_for(std::max(kg.m, 1), mgx::BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(mgx::BLOCK), 0, s,
                     (const int*)kg.sup0.data(), kg.m, d.stat.data());
  MGX_CHECK_LAUNCH("mgx ktruss enact");
  st.begin_peel(kg, ctx);
  e.peel(view, ctx);
  st.tc.waits += e.waits;
  st.tc.launches += 3 + 2 * e.calls;                   // (two clears, the sum; a scan and an expansion, or the two sweeps of a compaction, per call)
  st.tc.read_stats(d, false, ctx);
  st.res[0] = e.largest; st.res[1] = kg.m; st.res[2] = d.h[mgx::TC_S_TOTAL] / 3; st.res[3] = e.levels; st.res[4] = e.passes;
  put_stats(stats, 8, st.finish_run(sym, built_now));
  MGX_CATCH
}
static mgx::ktruss_graph_t& ktruss_last(mgx_ktruss_t p, const char* who) {
  require_run(p->st && p->st->last >= 0, who);
  return p->st->gr[p->st->last];
}
int mgx_ktruss_edges(mgx_ktruss_t p, int* h_src, int* h_dst, int* h_truss) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  mgx::ktruss_graph_t& kg = ktruss_last(p, "mgx_ktruss_edges");
  if (h_src) read_back(p, h_src, (const int*)kg.src.data(), (size_t)kg.m);
  if (h_dst) read_back(p, h_dst, (const int*)p->st->tc.dag[p->st->last].ci.data(), (size_t)kg.m);
  if (h_truss) read_back(p, h_truss, (const int*)kg.truss.data(), (size_t)kg.m);
  MGX_CATCH
}
int mgx_ktruss_support(mgx_ktruss_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::ktruss_graph_t& kg = ktruss_last(p, "mgx_ktruss_support");
  read_back(p, host, (const int*)kg.sup0.data(), (size_t)kg.m);
  MGX_CATCH
}
int mgx_ktruss_vertex_truss(mgx_ktruss_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  ktruss_last(p, "mgx_ktruss_vertex_truss");
  read_back(p, host, (const int*)p->st->vtruss.data(), (size_t)p->st->n);
  MGX_CATCH
}
int mgx_ktruss_histogram(mgx_ktruss_t p, int64_t* host, int cap) {
  MGX_TRY
  MGX_REQUIRE(p && host && cap >= 0, "bad argument");
  ktruss_last(p, "mgx_ktruss_histogram");
  std::vector<int> h((size_t)std::min<long long>(cap, (long long)p->st->n + 1));
  read_back(p, h.data(), (const int*)p->st->hist.data(), h.size());
  std::copy(h.begin(), h.end(), host);
  MGX_CATCH
}
int mgx_ktruss_order(mgx_ktruss_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  mgx::ktruss_graph_t& kg = ktruss_last(p, "mgx_ktruss_order");
  MGX_REQUIRE(p->st->last_fused, "mgx_ktruss_order: the last run was not a fused run");
  read_back(p, host, (const int*)kg.order.data(), (size_t)kg.m);
  MGX_CATCH
}
int mgx_ktruss_adjacency(mgx_ktruss_t p, int* h_ro, int* h_ci, int* h_eid) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  mgx::ktruss_graph_t& kg = ktruss_last(p, "mgx_ktruss_adjacency");
  if (h_ro) read_back(p, h_ro, (const int*)kg.adj_ro.data(), (size_t)p->st->n + 1);
  if (h_ci) read_back(p, h_ci, (const int*)kg.adj_ci.data(), 2 * (size_t)kg.m);
  if (h_eid) read_back(p, h_eid, (const int*)kg.adj_eid.data(), 2 * (size_t)kg.m);
  MGX_CATCH
}
int mgx_ktruss_truss_device(mgx_ktruss_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  *out = ktruss_last(p, "mgx_ktruss_truss_device").truss.data();
  MGX_CATCH
}
int mgx_ktruss_vertex_truss_device(mgx_ktruss_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  ktruss_last(p, "mgx_ktruss_vertex_truss_device");
  *out = p->st->vtruss.data();
  MGX_CATCH
}
int mgx_ktruss_step_kinds(mgx_ktruss_t p, int* host_kinds, int cap, int64_t* launches) {
  return chain_step_kinds(p, &mgx_ktruss_s::st, &mgx::ktruss_state_t::log_launches, "mgx_ktruss_step_kinds", host_kinds, cap, launches);
}
int mgx_ktruss_set_timing(mgx_ktruss_t p, int on) {
  MGX_TRY
  enter(p);
  ktruss_state(p).timing = on != 0;
  MGX_CATCH
}
int mgx_ktruss_phase_ms(mgx_ktruss_t p, double* out) {
  return chain_phase_ms(p, &mgx_ktruss_s::st, &mgx::ktruss_state_t::log_launches, &mgx::ktruss_state_t::phase_ms, "mgx_ktruss_phase_ms", out);
}

// ---- strongly connected components --------------------------------------------------
int mgx_scc_create(mgx_graph_t g, mgx_scc_t* out) { return create_handle(g, out); }
int mgx_scc_free(mgx_scc_t p) { return free_handle(p); }
int mgx_scc_run(mgx_scc_t p, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  MGX_REQUIRE(!g.csc_is_csr, "mgx_scc_run: needs the graph's genuine CSC (mgx_graph_build_csc)");
  if (!p->fused) p->fused.reset(new mgx::scc_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->labels = nullptr;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_offsets.data(),
                                                  g.d_row_indices.data(), ctx);
  p->labels = p->fused->label.data();
  put_stats(stats, 8, st);
  MGX_CATCH
}
int mgx_scc_enact(mgx_scc_t p, int64_t* stats) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  MGX_REQUIRE(!g.csc_is_csr, "mgx_scc_enact: needs the graph's genuine CSC (mgx_graph_build_csc)");
  p->labels = nullptr;
  const int n = g.num_nodes;
  if (n <= 0) { put_stats(stats, 8, {0, 0, 0, 0, 0, 0, 0, 0}); return MGX_OK; }
  if (!p->op_state) p->op_state.reset(new scc::scc_state_t(n, ctx));
  scc::scc_state_t& os = *p->op_state;
  // the views borrow the graph's arrays: new ones whenever those are not the ones they hold (the CSC may have been rebuilt)
  if (!p->fwd || p->bwd->gslice->d_row_offsets.data() != g.d_col_offsets.data() || p->bwd->gslice->d_col_indices.data() != g.d_row_indices.data()) {
    const scc::scc_problem_t::data_slice_t slice = {g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_offsets.data(), g.d_row_indices.data(),
                                                    os.d_state.data(), os.d_col.data(), os.d_claim.data(), os.d_label.data(), os.d_scalars.data()};
    p->fwd = std::make_shared<scc::scc_problem_t>(p->g->g, slice, ctx);
    p->bwd = std::make_shared<scc::scc_problem_t>(slice, n, g.num_edges, ctx);
  }
  if (!p->e) p->e.reset(new scc::scc_enactor_t(ctx, n, g.num_edges));
  if (!p->label_stats) p->label_stats.reset(new mgx::cc_label_stats_t(n, ctx));
  p->e->enact(p->fwd, p->bwd, os, ctx);
  const std::vector<long long> st = p->label_stats->run(os.d_label.data(), n, ctx);
  p->labels = os.d_label.data();
  put_stats(stats, 8, {st[0], st[1], st[2], p->e->trimmed, p->e->pivot_size, p->e->rounds, p->e->waits + 1, p->e->calls});
  MGX_CATCH
}
int mgx_scc_labels(mgx_scc_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->labels, "mgx_scc_labels");
  read_back(p, host, p->labels, p->n());
  MGX_CATCH
}
int mgx_scc_labels_device(mgx_scc_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->labels, "mgx_scc_labels_device");
  *out = p->labels;
  MGX_CATCH
}
int mgx_scc_step_kinds(mgx_scc_t p, int* host_kinds, int cap, int64_t* launches) {
  return chain_step_kinds(p, &mgx_scc_s::fused, &mgx::scc_fused_state_t::launches, "mgx_scc_step_kinds", host_kinds, cap, launches);
}
int mgx_scc_set_timing(mgx_scc_t p, int on) { return chain_set_timing(p, &mgx_scc_s::fused, on); }
int mgx_scc_phase_ms(mgx_scc_t p, double* out) {
  return chain_phase_ms(p, &mgx_scc_s::fused, &mgx::scc_fused_state_t::launches, &mgx::scc_fused_state_t::phase_ms, "mgx_scc_phase_ms", out);
}

// ---- label propagation and modularity ----------------------------------------------
static void lpa_check_args(const graph_device_t& g, int symmetric, int mode, int max_iter, const char* who) {
  MGX_REQUIRE(mode == MGX_LPA_SYNC || mode == MGX_LPA_LAZY, std::string(who) + ": mode must be MGX_LPA_SYNC or MGX_LPA_LAZY");
  MGX_REQUIRE(max_iter >= 0 && max_iter <= mgx::LPA_MAX_ITER_MAX, std::string(who) + ": max_iter must be in [0, 2^20]");
  MGX_REQUIRE(symmetric || !g.csc_is_csr, std::string(who) + ": symmetric = 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  if ((long long)g.num_edges > (1ll << 30)) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, std::string(who) + ": more than 2^30 entries");
}
int mgx_lpa_create(mgx_graph_t g, mgx_lpa_t* out) { return create_handle(g, out); }
int mgx_lpa_free(mgx_lpa_t p) { return free_handle(p); }
int mgx_lpa_run(mgx_lpa_t p, int symmetric, int mode, uint32_t seed, int max_iter, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->labels = nullptr;
  if (p->fused) p->fused->launches = -1;                     // (a run that is refused leaves nothing to the getters either)
  lpa_check_args(p->graph(), symmetric, mode, max_iter, "mgx_lpa_run");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::lpa_fused_state_t(g.num_nodes, g.num_edges, ctx));
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_offsets.data(),
                                                  g.d_row_indices.data(), symmetric, mode, seed, max_iter, ctx);
  p->labels = p->fused->vert.data();
  p->last_fused = true;
  put_stats(stats, 10, st);
  MGX_CATCH
}
int mgx_lpa_enact(mgx_lpa_t p, int symmetric, int mode, uint32_t seed, int max_iter, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->labels = nullptr;
  if (p->fused) p->fused->launches = -1;                     // (a run that is refused leaves nothing to the getters either)
  lpa_check_args(p->graph(), symmetric, mode, max_iter, "mgx_lpa_enact");
  // (the votes' segments are addressed by ints: both rows of every vertex are 2 m slots)
  if (!symmetric && (long long)p->graph().num_edges >= (1ll << 30))
    throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx_lpa_enact: symmetric = 0 takes fewer than 2^30 entries on the operator path");
  auto [ctx, g] = enter(p);
  const int n = g.num_nodes;
  if (!p->op_state) p->op_state.reset(new lpa::lpa_state_t(n, g.num_edges, ctx));
  lpa::lpa_state_t& os = *p->op_state;
  if (!p->e) p->e.reset(new lpa::lpa_enactor_t(ctx, n, g.num_edges));
  if (n <= 0) {
    p->e->trace.clear();
    p->labels = os.d_label.data();
    p->last_fused = false;
    put_stats(stats, 10, {0, 0, 0, 0, 1, 0, 0, 0, 0, 0});
    return MGX_OK;
  }
  // the views borrow the graph's arrays: new ones whenever those are not the ones they hold (the CSC may have been rebuilt)
  const lpa::lpa_problem_t::data_slice_t slice = {g.d_row_offsets.data(), g.d_col_offsets.data(), os.d_heads.data(), os.d_votes.data(),
                                                  os.d_label.data(), os.d_want.data(), os.d_scalars.data()};
  if (!p->fwd) p->fwd = std::make_shared<lpa::lpa_problem_t>(p->g->g, slice, ctx);
  if (!symmetric && (!p->bwd || p->bwd->gslice->d_row_offsets.data() != g.d_col_offsets.data() ||
                     p->bwd->gslice->d_col_indices.data() != g.d_row_indices.data())) {
    p->fwd = std::make_shared<lpa::lpa_problem_t>(p->g->g, slice, ctx);
    p->bwd = std::make_shared<lpa::lpa_problem_t>(slice, g.d_col_offsets.data(), g.d_row_indices.data(), n, g.num_edges, ctx);
  }
  if (!p->label_stats) p->label_stats.reset(new mgx::lpa_label_stats_t(n, ctx));
  p->e->enact(p->fwd, p->bwd, os, symmetric != 0, mode, seed, max_iter, ctx);
  const std::vector<long long> st = p->label_stats->run(os.d_label.data(), n, ctx);
  p->labels = os.d_label.data();
  p->last_fused = false;
  put_stats(stats, 10, {st[0], st[1], st[2], p->e->iterations, p->e->converged, p->e->unstable, (long long)n * (p->e->iterations + 1), 0,
                        p->e->waits + 1, p->e->calls});
  MGX_CATCH
}
int mgx_lpa_labels(mgx_lpa_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->labels, "mgx_lpa_labels");
  read_back(p, host, p->labels, p->n());
  MGX_CATCH
}
int mgx_lpa_labels_device(mgx_lpa_t p, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->labels, "mgx_lpa_labels_device");
  *out = p->labels;
  MGX_CATCH
}
int mgx_lpa_trace(mgx_lpa_t p, int64_t* host_triples, int cap, int64_t* iterations) {
  MGX_TRY
  MGX_REQUIRE(p && iterations && cap >= 0 && (host_triples || cap == 0), "bad argument");
  require_run(p->labels, "mgx_lpa_trace");
  if (p->last_fused) {
    const long long have = p->n() == 0 ? 0 : p->fused->iterations + 1;
    *iterations = have;
    const size_t take = (size_t)std::min<long long>(have, cap);
    std::vector<mgx::lpa_trace_t> h(take);
    read_back(p, h.data(), (const mgx::lpa_trace_t*)p->fused->trace.data(), take);
    for (size_t i = 0; i < take; ++i) {
      host_triples[3 * i] = h[i].unstable; host_triples[3 * i + 1] = h[i].changed; host_triples[3 * i + 2] = h[i].evaluated;
    }
  } else {
    const long long have = (long long)p->e->trace.size() / 3;
    *iterations = have;
    std::copy(p->e->trace.begin(), p->e->trace.begin() + 3 * std::min<long long>(have, cap), host_triples);
  }
  MGX_CATCH
}
int mgx_lpa_step_kinds(mgx_lpa_t p, int* host_kinds, int cap, int64_t* launches) {
  return chain_step_kinds(p, &mgx_lpa_s::fused, &mgx::lpa_fused_state_t::launches, "mgx_lpa_step_kinds", host_kinds, cap, launches);
}
int mgx_lpa_bins(mgx_lpa_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->fused && p->fused->launches >= 0, "mgx_lpa_bins");
  const mgx::lpa_fused_state_t& f = *p->fused;
  for (int i = 0; i < 4; ++i) out[i] = f.bins[i];
  out[4] = f.opts.cuts.short_max; out[5] = std::max(f.opts.cuts.wave_max, f.opts.cuts.short_max); out[6] = f.opts.table; out[7] = f.opts.list_div;
  out[8] = f.overflowed;
  MGX_CATCH
}
int mgx_lpa_set_timing(mgx_lpa_t p, int on) { return chain_set_timing(p, &mgx_lpa_s::fused, on); }
int mgx_lpa_phase_ms(mgx_lpa_t p, double* out) {
  return chain_phase_ms(p, &mgx_lpa_s::fused, &mgx::lpa_fused_state_t::launches, &mgx::lpa_fused_state_t::phase_ms, "mgx_lpa_phase_ms", out);
}
int mgx_modularity(mgx_graph_t g, const int* d_labels, int symmetric, uint64_t* out) {
  MGX_TRY
  MGX_REQUIRE(g && out && (d_labels || g->g->num_nodes == 0), "NULL argument");
  graph_device_t& G = *g->g;
  MGX_REQUIRE(symmetric || !G.csc_is_csr, "mgx_modularity: symmetric = 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  use_device(g->c);
  standard_context_t& ctx = *g->c->ctx;
  if (!g->mod) g->mod.reset(new mgx::modularity_state_t(G.num_nodes, ctx));      // (a second call on the graph, an LPA handle's included, allocates nothing)
  mgx::u64 r[3];
  g->mod->run(G.d_row_offsets.data(), G.d_col_indices.data(), G.d_col_offsets.data(), G.d_row_indices.data(), d_labels, symmetric, r, ctx);
  out[0] = r[0]; out[1] = r[1]; out[2] = r[2];
  MGX_CATCH
}

// ---- bit-parallel multi-source BFS and closeness -----------------------------------
// the sources as the run takes them (NULL: every vertex), checked before any device work
static long long msbfs_check_sources(mgx_msbfs_t p, const int* sources, int count, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(count >= 0, std::string(who) + ": count must not be negative");
  const int n = p->graph().num_nodes;
  if (!sources) return n;
  for (int i = 0; i < count; ++i) MGX_REQUIRE(sources[i] >= 0 && sources[i] < n, std::string(who) + ": source out of range");
  return count;
}
int mgx_msbfs_create(mgx_graph_t g, mgx_msbfs_t* out) { return create_handle(g, out); }
int mgx_msbfs_free(mgx_msbfs_t p) { return free_handle(p); }
int mgx_msbfs_run(mgx_msbfs_t p, const int* sources, int count, int symmetric, int want_depths, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->last = 0;
  if (p->fused) p->fused->launches = -1;                     // (a run that is refused leaves nothing to the getters either)
  const long long cnt = msbfs_check_sources(p, sources, count, "mgx_msbfs_run");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::msbfs_fused_state_t(g.num_nodes, g.num_edges, ctx));
  // the in-entries: the rows themselves on the caller's word, else the genuine CSC, else none (every level pushes)
  const bool csc = !symmetric && !g.csc_is_csr;
  const int* const io = symmetric ? g.d_row_offsets.data() : (csc ? g.d_col_offsets.data() : nullptr);
  const int* const ia = symmetric ? g.d_col_indices.data() : (csc ? g.d_row_indices.data() : nullptr);
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), io, ia, sources, cnt, csc, want_depths != 0, ctx);
  p->last = 1;
  p->count = cnt;
  put_stats(stats, 10, st);
  MGX_CATCH
}
int mgx_msbfs_enact(mgx_msbfs_t p, const int* sources, int count, int symmetric, int want_depths, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  (void)symmetric;                                           // (the operator path always pushes)
  p->last = 0;
  if (p->fused) p->fused->launches = -1;
  const long long cnt = msbfs_check_sources(p, sources, count, "mgx_msbfs_enact");
  auto [ctx, g] = enter(p);
  const int n = g.num_nodes;
  if (!p->op_state) p->op_state.reset(new msbfs::msbfs_state_t(n, ctx));
  msbfs::msbfs_state_t& os = *p->op_state;
  os.kept_depths = false;
  os.ensure(cnt, want_depths != 0, n, ctx);
  long long sum_reach = 0;
  if (n > 0 && cnt > 0) {
    if (!p->e) p->e.reset(new msbfs::msbfs_enactor_t(ctx, n, g.num_edges));
    if (sources) MGX_HIP(mgx::htod(os.d_sources.data(), sources, (size_t)cnt, ctx.stream()));
    if (want_depths) MGX_HIP(hipMemsetAsync(os.d_depth.data(), 0xff, (size_t)cnt * (size_t)n * sizeof(int), ctx.stream()));
    const msbfs::msbfs_problem_t::data_slice_t slice = os.slice(n, want_depths != 0, sources != nullptr);
    if (!p->p || memcmp(&slice, &p->p_slice, sizeof(slice)) != 0) {      // (the arrays grew, or the run wants other ones)
      p->p = std::make_shared<msbfs::msbfs_problem_t>(p->g->g, slice, ctx);
      memcpy(&p->p_slice, &slice, sizeof(slice));
    }
    p->e->enact(p->p, slice, sources, cnt, ctx);
    MGX_HIP(mgx::dtoh(os.h_per_src.data(), (const long long*)os.d_per_src.data(), 4 * (size_t)os.cap, ctx.stream()));
    for (long long s = 0; s < cnt; ++s) sum_reach += os.h_per_src[(size_t)s];
  }
  os.kept_depths = want_depths != 0;
  p->last = 2;
  p->count = cnt;
  const bool ran = n > 0 && cnt > 0;
  put_stats(stats, 10, {cnt, ran ? (cnt + 63) / 64 : 0, ran ? p->e->deepest : 0, sum_reach, ran ? p->e->levels : 0, 0, ran ? p->e->waits + 1 : 0,
                        ran ? p->e->calls : 0, 0, want_depths ? 1 : 0});
  MGX_CATCH
}
// one of the last run's per-source arrays (0 reach, 1 far, 2 ecc, 3 harm) to the caller's host array
static void msbfs_per_source(mgx_msbfs_t p, int which, void* host, const char* who) {
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->last != 0, who);
  const bool fused = p->last == 1;
  const std::vector<long long>& h = fused ? p->fused->h_per_src : p->op_state->h_per_src;
  const size_t cap = (size_t)(fused ? p->fused->src_cap : p->op_state->cap);
  if (p->count) memcpy(host, h.data() + (size_t)which * cap, (size_t)p->count * sizeof(long long));
}
int mgx_msbfs_reach(mgx_msbfs_t p, int64_t* host) {
  MGX_TRY
  msbfs_per_source(p, 0, host, "mgx_msbfs_reach");
  MGX_CATCH
}
int mgx_msbfs_far(mgx_msbfs_t p, int64_t* host) {
  MGX_TRY
  msbfs_per_source(p, 1, host, "mgx_msbfs_far");
  MGX_CATCH
}
int mgx_msbfs_ecc(mgx_msbfs_t p, int64_t* host) {
  MGX_TRY
  msbfs_per_source(p, 2, host, "mgx_msbfs_ecc");
  MGX_CATCH
}
int mgx_msbfs_harmonic(mgx_msbfs_t p, double* host) {
  MGX_TRY
  msbfs_per_source(p, 3, host, "mgx_msbfs_harmonic");
  MGX_CATCH
}
int mgx_msbfs_vertex_sums_device(mgx_msbfs_t p, const int64_t** d_reach_in, const int64_t** d_far_in) {
  MGX_TRY
  MGX_REQUIRE(p && d_reach_in && d_far_in, "NULL argument");
  require_run(p->last != 0, "mgx_msbfs_vertex_sums_device");
  if (p->last == 1) {
    *d_reach_in = (const int64_t*)p->fused->reach_in();
    *d_far_in = (const int64_t*)p->fused->far_in();
  } else {
    *d_reach_in = (const int64_t*)p->op_state->d_sums.data();
    *d_far_in = (const int64_t*)(p->op_state->d_sums.data() + p->op_state->N);
  }
  MGX_CATCH
}
int mgx_msbfs_vertex_sums(mgx_msbfs_t p, int64_t* reach_in, int64_t* far_in) {
  MGX_TRY
  MGX_REQUIRE(p && reach_in && far_in, "NULL argument");
  require_run(p->last != 0, "mgx_msbfs_vertex_sums");
  if (p->count == 0) {                                       // (a run without sources touches no device array)
    std::fill(reach_in, reach_in + p->n(), 0);
    std::fill(far_in, far_in + p->n(), 0);
    return MGX_OK;
  }
  const int64_t* r = nullptr;
  const int64_t* f = nullptr;
  if (p->last == 1) { r = (const int64_t*)p->fused->reach_in(); f = (const int64_t*)p->fused->far_in(); }
  else { r = (const int64_t*)p->op_state->d_sums.data(); f = r + p->op_state->N; }
  read_back(p, reach_in, r, p->n());
  read_back(p, far_in, f, p->n());
  MGX_CATCH
}
int mgx_msbfs_depths(mgx_msbfs_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  require_run(p->last != 0, "mgx_msbfs_depths");
  const bool kept = p->last == 1 ? p->fused->kept_depths : p->op_state->kept_depths;
  MGX_REQUIRE(kept, "mgx_msbfs_depths: the last run kept no depths (want_depths = 0)");
  const int* d = p->last == 1 ? p->fused->depth.data() : p->op_state->d_depth.data();
  read_back(p, host, d, (size_t)p->count * p->n());
  MGX_CATCH
}
int mgx_msbfs_level_kinds(mgx_msbfs_t p, int* host_kinds, int cap, int64_t* levels) {
  MGX_TRY
  MGX_REQUIRE(p && levels && cap >= 0 && (host_kinds || cap == 0), "bad argument");
  require_run(p->fused && p->fused->launches >= 0, "mgx_msbfs_level_kinds");
  *levels = p->fused->levels;
  const long long have = std::min<long long>(std::min<long long>(p->fused->levels, mgx::CHAIN_LOG_CAP), cap);
  read_back(p, host_kinds, (const int*)p->fused->ctl.data()->log, (size_t)have);
  MGX_CATCH
}
int mgx_msbfs_bins(mgx_msbfs_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->fused && p->fused->launches >= 0, "mgx_msbfs_bins");
  const mgx::msbfs_fused_state_t& f = *p->fused;
  for (int i = 0; i < mgx::MSBFS_BINS; ++i) out[i] = f.bins[i];
  out[10] = f.opts.cuts.short_max; out[11] = f.opts.cuts.wave_max; out[12] = f.opts.cuts.seg; out[13] = f.opts.pull_div;
  MGX_CATCH
}
int mgx_msbfs_set_timing(mgx_msbfs_t p, int on) { return chain_set_timing(p, &mgx_msbfs_s::fused, on); }
int mgx_msbfs_phase_ms(mgx_msbfs_t p, double* out) {
  return chain_phase_ms(p, &mgx_msbfs_s::fused, &mgx::msbfs_fused_state_t::launches, &mgx::msbfs_fused_state_t::phase_ms, "mgx_msbfs_phase_ms", out);
}

// ---- random walks and node2vec sampling --------------------------------------------
// a run's arguments, checked before any device work (the parameters first: their messages do not need a handle)
static mgx::rw_request_t rw_check(mgx_rw_t p, const int* starts, int count, int walks_per_start, int length, uint32_t seed, int weighted,
                                  float p_ret, float q_inout, float restart, int want_paths, int want_visits, const char* who) {
  const std::string w(who);
  MGX_REQUIRE(count >= 0 || !starts, w + ": count must not be negative");
  MGX_REQUIRE(length >= 0, w + ": length must not be negative");
  MGX_REQUIRE(walks_per_start >= 1, w + ": walks_per_start must be at least 1");
  MGX_REQUIRE(std::isfinite(p_ret) && p_ret > 0.f && std::isfinite(q_inout) && q_inout > 0.f, w + ": p and q must be finite and positive");
  MGX_REQUIRE(restart >= 0.f && restart < 1.f, w + ": restart must lie in [0, 1)");
  MGX_REQUIRE(p, "NULL argument");
  const int n = p->graph().num_nodes;
  mgx::rw_request_t r;
  r.h_starts = starts;
  r.starts = starts ? count : n;
  if (starts) for (int i = 0; i < count; ++i) MGX_REQUIRE(starts[i] >= 0 && starts[i] < n, w + ": start out of range");
  r.per_start = walks_per_start; r.length = length; r.seed = seed;
  if (r.walkers() >= (1ll << 31)) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, w + ": 2^31 walkers or more");
  r.weighted = weighted != 0;
  r.second = !(p_ret == 1.f && q_inout == 1.f);
  r.ip = 1.0f / p_ret; r.iq = 1.0f / q_inout; r.restart = restart;
  r.want_paths = want_paths != 0; r.want_visits = want_visits != 0;
  return r;
}
static void rw_finish(mgx_rw_t p, int path, const mgx::rw_request_t& r) {
  p->last = path;
  p->walkers = r.walkers(); p->length = r.length;
  p->kept_paths = r.want_paths; p->kept_visits = r.want_visits;
}
static const mgx::rw_results_t& rw_results(mgx_rw_t p, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, who);
  return p->last == 1 ? p->fused->res : p->op_state->res;
}
int mgx_rw_create(mgx_graph_t g, mgx_rw_t* out) { return create_handle(g, out); }
int mgx_rw_free(mgx_rw_t p) { return free_handle(p); }
int mgx_rw_run(mgx_rw_t p, const int* starts, int count, int walks_per_start, int length, uint32_t seed, int weighted, float p_ret,
               float q_inout, float restart, int want_paths, int want_visits, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;                                        // (a run that is refused leaves nothing to the getters)
  const mgx::rw_request_t r = rw_check(p, starts, count, walks_per_start, length, seed, weighted, p_ret, q_inout, restart, want_paths,
                                       want_visits, "mgx_rw_run");
  auto [ctx, g] = enter(p);
  if (!p->setup) p->setup.reset(new mgx::rw_setup_state_t(g.num_nodes, g.num_edges, ctx));
  if (!p->fused) p->fused.reset(new mgx::rw_fused_state_t(g.num_nodes, ctx));
  p->fused->timing = p->timing;
  const std::vector<long long> st = p->fused->run(*p->setup, g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_values.data(), r, ctx);
  rw_finish(p, 1, r);
  put_stats(stats, 10, st);
  MGX_CATCH
}
int mgx_rw_enact(mgx_rw_t p, const int* starts, int count, int walks_per_start, int length, uint32_t seed, int weighted, float p_ret,
                 float q_inout, float restart, int want_paths, int want_visits, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;
  const mgx::rw_request_t r = rw_check(p, starts, count, walks_per_start, length, seed, weighted, p_ret, q_inout, restart, want_paths,
                                       want_visits, "mgx_rw_enact");
  auto [ctx, g] = enter(p);
  const int n = g.num_nodes;
  const long long W = r.walkers();
  if (!p->setup) p->setup.reset(new mgx::rw_setup_state_t(n, g.num_edges, ctx));
  if (!p->op_state) p->op_state.reset(new rw::rw_state_t());
  std::vector<long long> st = {W, r.length, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n > 0 && W > 0) {
    const hipStream_t s = ctx.stream();
    mgx::rw_setup_state_t& su = *p->setup;
    rw::rw_state_t& os = *p->op_state;
    long long launches = 0, waits = 0;
    su.ensure(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_values.data(), r.weighted, r.second, ctx, launches, waits);
    os.ensure(r, n, ctx);
    if (starts) { MGX_HIP(mgx::htod(os.res.d_starts.data(), starts, (size_t)r.starts, s)); ++waits; }
    MGX_HIP(hipMemsetAsync(os.res.counters.data(), 0, mgx::RW_COUNTERS * sizeof(mgx::u64), s));
    if (r.want_visits) MGX_HIP(hipMemsetAsync(os.res.visits.data(), 0, (size_t)n * sizeof(mgx::u64), s));
    if (r.want_paths) MGX_HIP(hipMemsetAsync(os.res.paths.data(), 0xff, (size_t)W * ((size_t)r.length + 1) * sizeof(int), s));
    const rw::rw_problem_t::data_slice_t slice =
        os.slice(su.graph(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_values.data(), r.weighted, r.second), mgx::rw_params_of(r, su.opts), r);
    if (!p->p) p->p = std::make_shared<rw::rw_problem_t>(p->g->g, slice, ctx);
    else MGX_HIP(mgx::htod(p->p->d_data_slice.data(), &slice, 1, s));
    ++waits;
    if (!p->e) p->e.reset(new rw::rw_enactor_t());
    p->e->enact(p->p, slice, r, ctx);
    mgx::u64 c[mgx::RW_COUNTERS];
    MGX_HIP(mgx::dtoh(c, (const mgx::u64*)os.res.counters.data(), mgx::RW_COUNTERS, s));
    ++waits;
    st = {W, r.length, (long long)c[mgx::RW_C_STEPS], (long long)c[mgx::RW_C_DEAD], (long long)c[mgx::RW_C_RESTARTS], (long long)c[mgx::RW_C_TRIES],
          (long long)c[mgx::RW_C_FALLBACKS], su.unsorted && r.second ? 1 : 0, launches + p->e->calls, waits + p->e->waits};
  }
  rw_finish(p, 2, r);
  put_stats(stats, 10, st);
  MGX_CATCH
}
int mgx_rw_paths(mgx_rw_t p, int* host) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_paths");
  MGX_REQUIRE(host, "NULL argument");
  MGX_REQUIRE(p->kept_paths, "mgx_rw_paths: the last run kept no paths (want_paths = 0)");
  if (p->walkers && p->n()) read_back(p, host, (const int*)res.paths.data(), (size_t)p->walkers * ((size_t)p->length + 1));
  MGX_CATCH
}
int mgx_rw_paths_device(mgx_rw_t p, const int** d_paths) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_paths_device");
  MGX_REQUIRE(d_paths, "NULL argument");
  MGX_REQUIRE(p->kept_paths, "mgx_rw_paths_device: the last run kept no paths (want_paths = 0)");
  *d_paths = p->walkers && p->n() ? res.paths.data() : nullptr;
  MGX_CATCH
}
int mgx_rw_ends(mgx_rw_t p, int* host) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_ends");
  MGX_REQUIRE(host, "NULL argument");
  if (p->walkers && p->n()) read_back(p, host, (const int*)res.ends.data(), (size_t)p->walkers);
  MGX_CATCH
}
int mgx_rw_lengths(mgx_rw_t p, int* host) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_lengths");
  MGX_REQUIRE(host, "NULL argument");
  if (p->walkers && p->n()) read_back(p, host, (const int*)res.lengths.data(), (size_t)p->walkers);
  MGX_CATCH
}
int mgx_rw_visits(mgx_rw_t p, int64_t* host) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_visits");
  MGX_REQUIRE(host, "NULL argument");
  MGX_REQUIRE(p->kept_visits, "mgx_rw_visits: the last run kept no visits (want_visits = 0)");
  if (p->walkers == 0) std::fill(host, host + p->n(), 0);     // (a run without walkers touches no device array)
  else read_back(p, host, (const int64_t*)res.visits.data(), p->n());
  MGX_CATCH
}
int mgx_rw_visits_device(mgx_rw_t p, const int64_t** d_visits) {
  MGX_TRY
  const mgx::rw_results_t& res = rw_results(p, "mgx_rw_visits_device");
  MGX_REQUIRE(d_visits, "NULL argument");
  MGX_REQUIRE(p->kept_visits, "mgx_rw_visits_device: the last run kept no visits (want_visits = 0)");
  *d_visits = p->walkers && p->n() ? (const int64_t*)res.visits.data() : nullptr;
  MGX_CATCH
}
int mgx_rw_bins(mgx_rw_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last != 0 && p->setup, "mgx_rw_bins");
  const mgx::rw_setup_state_t& su = *p->setup;
  for (int i = 0; i < mgx::RW_BINS; ++i) out[i] = su.bins[i];
  out[5] = su.opts.cuts.short_max; out[6] = su.opts.cuts.wave_max; out[7] = su.opts.cuts.seg; out[8] = su.opts.tries; out[9] = su.opts.tile;
  MGX_CATCH
}
int mgx_rw_set_timing(mgx_rw_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->timing = on != 0;
  MGX_CATCH
}
int mgx_rw_phase_ms(mgx_rw_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_rw_phase_ms");
  out[0] = p->fused->phase_ms[0]; out[1] = p->fused->phase_ms[1];
  MGX_CATCH
}


// ---- neighbour sampling for GNN mini-batches ---------------------------------------
// a run's arguments, checked before any device work (the parameters first: their messages do not need a handle)
static mgx::ns_request_t nsample_check(mgx_nsample_t p, const int* seeds, int count, const int* fanouts, int hops, int replace, uint32_t seed,
                                       mgx::ns_bounds_t* bounds, const char* who) {
  const std::string w(who);
  MGX_REQUIRE(hops >= 0 && hops <= mgx::NS_MAX_HOPS, w + ": hops must be in [0, 16]");
  MGX_REQUIRE(fanouts || hops == 0, w + ": fanouts is NULL");
  for (int h = 0; h < hops; ++h)
    MGX_REQUIRE(fanouts[h] == -1 || (fanouts[h] >= 1 && fanouts[h] <= mgx::NS_MAX_FANOUT), w + ": every one of fanouts must be -1 or in 1 .. 64");
  MGX_REQUIRE(count >= 0 || !seeds, w + ": count must not be negative");
  MGX_REQUIRE(p, "NULL argument");
  const int n = p->graph().num_nodes;
  mgx::ns_request_t r;
  r.h_seeds = seeds;
  r.count = seeds ? count : n;
  if (seeds) for (int i = 0; i < count; ++i) MGX_REQUIRE(seeds[i] >= 0 && seeds[i] < n, w + ": seed out of range");
  r.hops = hops;
  for (int h = 0; h < hops; ++h) r.fanouts[h] = fanouts[h];
  r.replace = replace != 0; r.seed = seed;
  *bounds = mgx::ns_bounds(n, (long long)p->graph().num_edges, r, mgx::ns_opts_t::from_env().cuts);
  if (bounds->overflow()) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, w + ": a capacity bound of 2^31 or more (seeds x fanouts)");
  return r;
}
static const mgx::ns_results_t& nsample_results(mgx_nsample_t p, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, who);
  return p->last == 1 ? p->fused->res : p->op_state->res;
}
int mgx_nsample_create(mgx_graph_t g, mgx_nsample_t* out) { return create_handle(g, out); }
int mgx_nsample_free(mgx_nsample_t p) { return free_handle(p); }
int mgx_nsample_run(mgx_nsample_t p, const int* seeds, int count, const int* fanouts, int hops, int replace, uint32_t seed, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;                                        // (a run that is refused leaves nothing to the getters)
  mgx::ns_bounds_t b;
  const mgx::ns_request_t r = nsample_check(p, seeds, count, fanouts, hops, replace, seed, &b, "mgx_nsample_run");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::ns_fused_state_t(g.num_nodes, g.num_edges, ctx));
  p->fused->timing = p->timing;
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), r, b, ctx);
  p->last = 1;
  put_stats(stats, mgx::NS_STATS, st);
  MGX_CATCH
}
int mgx_nsample_enact(mgx_nsample_t p, const int* seeds, int count, const int* fanouts, int hops, int replace, uint32_t seed, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;
  mgx::ns_bounds_t b;
  const mgx::ns_request_t r = nsample_check(p, seeds, count, fanouts, hops, replace, seed, &b, "mgx_nsample_enact");
  auto [ctx, g] = enter(p);
  const int n = g.num_nodes;
  if (!p->op_state) p->op_state.reset(new nsample::nsample_state_t());
  nsample::nsample_state_t& os = *p->op_state;
  std::vector<long long> st = {r.count, 0, r.hops, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n > 0 && r.count > 0) {
    const hipStream_t s = ctx.stream();
    long long waits = 0;
    os.ensure(r, b, n, ctx);
    if (seeds) { MGX_HIP(mgx::htod(os.res.d_seeds.data(), seeds, (size_t)r.count, s)); ++waits; }
    const nsample::nsample_problem_t::data_slice_t slice = os.slice(g.d_row_offsets.data(), g.d_col_indices.data(), r);
    if (!p->p) p->p = std::make_shared<nsample::nsample_problem_t>(p->g->g, slice, ctx);
    else MGX_HIP(mgx::htod(p->p->d_data_slice.data(), &slice, 1, s));
    ++waits;
    if (!p->e) p->e.reset(new nsample::nsample_enactor_t(ctx, n));
    p->e->enact(p->p, os, slice, r, n, ctx);
    const unsigned long long* c = p->e->counters;
    st = {r.count, os.res.hop_offsets[1], r.hops, os.res.count_vertices(), os.res.count_rows(), os.res.edges, (long long)c[mgx::NS_C_EMPTY],
          (long long)c[mgx::NS_C_WHOLE], (long long)c[mgx::NS_C_SAMPLED], (long long)c[mgx::NS_C_DRAWS], (long long)c[mgx::NS_C_COLLISIONS],
          (long long)c[mgx::NS_C_REVISITS], p->e->calls, waits + p->e->waits};
  } else {
    os.res.nothing(r);
  }
  p->last = 2;
  put_stats(stats, mgx::NS_STATS, st);
  MGX_CATCH
}
// an array of the last run to the host; NULL skips it.  A run without device work has no array but row_offsets = {0}.
static int nsample_get(mgx_nsample_t p, int* host, const char* who, mem_t<int> mgx::ns_results_t::*arr, int which) {
  MGX_TRY
  const mgx::ns_results_t& res = nsample_results(p, who);
  if (!host) return MGX_OK;
  const size_t count = which == 0 ? (size_t)res.count_vertices() : which == 1 ? (size_t)res.count_rows() + 1 : which == 2 ? (size_t)res.edges : (size_t)res.seeds;
  if (!res.device) { if (which == 1) host[0] = 0; return MGX_OK; }
  read_back(p, host, (const int*)(res.*arr).data(), count);
  MGX_CATCH
}
static int nsample_get_device(mgx_nsample_t p, const int** out, const char* who, mem_t<int> mgx::ns_results_t::*arr) {
  MGX_TRY
  const mgx::ns_results_t& res = nsample_results(p, who);
  MGX_REQUIRE(out, "NULL argument");
  *out = res.device ? (res.*arr).data() : nullptr;
  MGX_CATCH
}
int mgx_nsample_vertices(mgx_nsample_t p, int* host) { return nsample_get(p, host, "mgx_nsample_vertices", &mgx::ns_results_t::vertices, 0); }
int mgx_nsample_row_offsets(mgx_nsample_t p, int* host) { return nsample_get(p, host, "mgx_nsample_row_offsets", &mgx::ns_results_t::row_offsets, 1); }
int mgx_nsample_cols(mgx_nsample_t p, int* host) { return nsample_get(p, host, "mgx_nsample_cols", &mgx::ns_results_t::cols, 2); }
int mgx_nsample_entry_pos(mgx_nsample_t p, int* host) { return nsample_get(p, host, "mgx_nsample_entry_pos", &mgx::ns_results_t::entry_pos, 2); }
int mgx_nsample_seed_local(mgx_nsample_t p, int* host) { return nsample_get(p, host, "mgx_nsample_seed_local", &mgx::ns_results_t::seed_local, 3); }
int mgx_nsample_hop_offsets(mgx_nsample_t p, int* host) {
  MGX_TRY
  const mgx::ns_results_t& res = nsample_results(p, "mgx_nsample_hop_offsets");
  if (host) std::copy(res.hop_offsets.begin(), res.hop_offsets.end(), host);
  MGX_CATCH
}
int mgx_nsample_vertices_device(mgx_nsample_t p, const int** out) { return nsample_get_device(p, out, "mgx_nsample_vertices_device", &mgx::ns_results_t::vertices); }
int mgx_nsample_row_offsets_device(mgx_nsample_t p, const int** out) { return nsample_get_device(p, out, "mgx_nsample_row_offsets_device", &mgx::ns_results_t::row_offsets); }
int mgx_nsample_cols_device(mgx_nsample_t p, const int** out) { return nsample_get_device(p, out, "mgx_nsample_cols_device", &mgx::ns_results_t::cols); }
int mgx_nsample_entry_pos_device(mgx_nsample_t p, const int** out) { return nsample_get_device(p, out, "mgx_nsample_entry_pos_device", &mgx::ns_results_t::entry_pos); }
int mgx_nsample_bins(mgx_nsample_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_nsample_bins");
  const mgx::ns_fused_state_t& f = *p->fused;
  for (int i = 0; i < mgx::NS_BINS; ++i) out[i] = f.bins[i];
  out[5] = f.opts.cuts.short_max; out[6] = f.opts.cuts.wave_max; out[7] = f.opts.cuts.seg;
  MGX_CATCH
}
int mgx_nsample_set_timing(mgx_nsample_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->timing = on != 0;
  MGX_CATCH
}
int mgx_nsample_phase_ms(mgx_nsample_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_nsample_phase_ms");
  out[0] = p->fused->phase_ms[0]; out[1] = p->fused->phase_ms[1];
  MGX_CATCH
}

// ---- neighbour feature aggregation for GNN layers ----------------------------------
// a call's arguments, checked before any device work (the parameters first: their messages do not need a handle)
static mgx::agg_request_t agg_check(mgx_agg_t p, int source, mgx_nsample_t block, int hop, const float* d_x, int64_t x_rows, int64_t ldx, int feats,
                                    int op, int weighted, float* d_y, int64_t ldy, const char* who) {
  const std::string w(who);
  MGX_REQUIRE(feats >= 1 && feats <= mgx::AGG_MAX_FEATS, w + ": feats must be in [1, 65536]");
  MGX_REQUIRE(ldx >= feats && ldy >= feats, w + ": ldx and ldy must be at least feats");
  MGX_REQUIRE(op >= 0 && op < mgx::AGG_OPS, w + ": op must be 0 (sum), 1 (mean), 2 (max) or 3 (min)");
  MGX_REQUIRE(source >= 0 && source < mgx::AGG_SOURCES, w + ": source must be 0 (out-rows), 1 (in-rows) or 2 (block)");
  MGX_REQUIRE(x_rows >= 0, w + ": x_rows must not be negative");
  MGX_REQUIRE(p, "NULL argument");
  const graph_device_t& g = p->graph();
  const size_t m = (size_t)g.num_edges;
  mgx::agg_request_t r;
  r.x = d_x; r.y = d_y; r.ldx = ldx; r.ldy = ldy; r.feats = feats; r.op = op; r.source = source;
  long long need_rows = g.num_nodes;
  if (source == mgx::AGG_SRC_OUT) {
    r.ro = g.d_row_offsets.data(); r.ci = g.d_col_indices.data();
    MGX_REQUIRE(!weighted || g.d_col_values.size() >= m, w + ": weighted, and the graph has no weights");
    if (weighted) r.w = g.d_col_values.data();
    r.R = g.num_nodes; r.entries = g.num_edges;
  } else if (source == mgx::AGG_SRC_IN) {
    MGX_REQUIRE(!g.csc_is_csr, w + ": the in-rows need the graph's genuine CSC (mgx_graph_build_csc)");
    r.ro = g.d_col_offsets.data(); r.ci = g.d_row_indices.data();
    MGX_REQUIRE(!weighted || g.d_row_values.size() >= m, w + ": weighted, and the CSC has no weights");
    if (weighted) r.w = g.d_row_values.data();
    r.R = g.num_nodes; r.entries = g.num_edges;
  } else {
    MGX_REQUIRE(block, w + ": source 2 needs a block (an mgx_nsample_t)");
    MGX_REQUIRE(block->g == p->g, w + ": the block was sampled from another graph");
    MGX_REQUIRE(block->last != 0, w + ": the block has no successful sampling run");
    const mgx::ns_results_t& res = block->last == 1 ? block->fused->res : block->op_state->res;
    const int hops = (int)res.hop_offsets.size() - 2;
    MGX_REQUIRE(hop >= -1 && hop < hops, w + ": hop must be -1 (all sampled rows) or in [0, the run's hops)");
    MGX_REQUIRE(!weighted || g.d_col_values.size() >= m, w + ": weighted, and the graph has no weights");
    need_rows = res.count_vertices();
    if (res.device) {
      const int h0 = hop < 0 ? 0 : hop, h1 = hop < 0 ? hops : hop + 1;
      r.ro = res.row_offsets.data() + res.hop_offsets[h0]; r.ci = res.cols.data();
      r.R = res.hop_offsets[h1] - res.hop_offsets[h0];
      r.entries = res.edge_offsets[h1] - res.edge_offsets[h0];
      if (weighted) { r.w = g.d_col_values.data(); r.entry_pos = res.entry_pos.data(); }
      r.needs_plan = res.any_whole;
    }
  }
  MGX_REQUIRE(x_rows >= need_rows, w + ": x_rows is below the number of vertices the columns name");
  MGX_REQUIRE(r.R == 0 || (d_x && d_y), w + ": d_x or d_y is NULL");
  if (r.R > 0 && x_rows > 0) {
    const char* const x0 = (const char*)d_x;
    const char* const x1 = x0 + ((size_t)(x_rows - 1) * (size_t)ldx + (size_t)feats) * sizeof(float);
    const char* const y0 = (const char*)d_y;
    const char* const y1 = y0 + ((size_t)(r.R - 1) * (size_t)ldy + (size_t)feats) * sizeof(float);
    MGX_REQUIRE(x1 <= y0 || y1 <= x0, w + ": the ranges of X and Y overlap");
  }
  return r;
}
// MGX_AGG_SEG is read once per handle: seg is part of the result's definition, and both paths of a handle use the same
static int agg_seg(mgx_agg_t p) {
  if (!p->seg) p->seg = mgx::agg_seg_from_env();
  return p->seg;
}
static void agg_ran(mgx_agg_t p, const mgx::agg_request_t& r, int which) {
  p->last_y = r.y; p->last_ldy = r.ldy; p->last_rows = r.R; p->last_feats = r.feats;
  p->last = which;
}
int mgx_agg_create(mgx_graph_t g, mgx_agg_t* out) { return create_handle(g, out); }
int mgx_agg_free(mgx_agg_t p) { return free_handle(p); }
int mgx_agg_run(mgx_agg_t p, int source, mgx_nsample_t block, int hop, const float* d_x, int64_t x_rows, int64_t ldx, int feats, int op, int weighted,
                float* d_y, int64_t ldy, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;                                        // (a run that is refused leaves nothing to the getters)
  const mgx::agg_request_t r = agg_check(p, source, block, hop, d_x, x_rows, ldx, feats, op, weighted, d_y, ldy, "mgx_agg_run");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::agg_fused_state_t(agg_seg(p)));
  p->fused->timing = p->timing;
  const std::vector<long long> st = p->fused->run(r, ctx);
  agg_ran(p, r, 1);
  put_stats(stats, mgx::AGG_STATS, st);
  MGX_CATCH
}
int mgx_agg_enact(mgx_agg_t p, int source, mgx_nsample_t block, int hop, const float* d_x, int64_t x_rows, int64_t ldx, int feats, int op, int weighted,
                  float* d_y, int64_t ldy, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;
  const mgx::agg_request_t r = agg_check(p, source, block, hop, d_x, x_rows, ldx, feats, op, weighted, d_y, ldy, "mgx_agg_enact");
  auto [ctx, g] = enter(p);
  const mgx::agg_shape_t sh = mgx::agg_shape(feats, mgx::agg_vector_ok(d_x, ldx, d_y, ldy, feats));
  const int seg = agg_seg(p);
  long long calls = 0, waits = 0;
  if (r.R > 0) {
    const agg::agg_problem_t::data_slice_t slice = {r.ro, r.ci, r.w ? r.entry_pos : nullptr, r.w, r.x, r.y, r.ldx, r.ldy, r.feats, r.op, seg};
    if (!p->p) p->p = std::make_shared<agg::agg_problem_t>(p->g->g, slice, ctx);
    else MGX_HIP(mgx::htod(p->p->d_data_slice.data(), &slice, 1, ctx.stream()));
    ++waits;
    if (!p->e) p->e.reset(new agg::agg_enactor_t());
    p->e->enact(p->p, r.R, ctx);
    calls = p->e->calls; waits += p->e->waits;
  }
  agg_ran(p, r, 2);
  put_stats(stats, mgx::AGG_STATS, {r.R, r.entries, r.feats, sh.G, sh.tiles, sh.vector, seg, calls, waits});
  MGX_CATCH
}
// a handle-owned array grown to `want` floats (growing only)
static float* agg_buffer(mgx_agg_t p, mem_t<float> mgx_agg_s::*buf, size_t mgx_agg_s::*cap, size_t want) {
  if (want > p->*cap) {
    p->ctx().synchronize();                                  // (a queued run may still read the old one)
    p->*buf = mem_t<float>();
    p->*cap = 0;
    p->*buf = mem_t<float>(want, p->ctx());
    p->*cap = want;
  }
  return (p->*buf).data();
}
int mgx_agg_upload(mgx_agg_t p, const float* host_x, int64_t rows, int feats, float** d_x) {
  MGX_TRY
  MGX_REQUIRE(p && d_x && rows >= 0 && feats >= 1 && (host_x || rows == 0), "mgx_agg_upload: NULL or negative argument");
  auto [ctx, g] = enter(p);
  const size_t count = (size_t)rows * (size_t)feats;
  *d_x = agg_buffer(p, &mgx_agg_s::xbuf, &mgx_agg_s::xcap, count);
  MGX_HIP(mgx::htod(*d_x, host_x, count, ctx.stream()));
  MGX_CATCH
}
int mgx_agg_output(mgx_agg_t p, int64_t rows, int64_t ld, float** d_y) {
  MGX_TRY
  MGX_REQUIRE(p && d_y && rows >= 0 && ld >= 1, "mgx_agg_output: NULL or negative argument");
  auto [ctx, g] = enter(p);
  *d_y = agg_buffer(p, &mgx_agg_s::ybuf, &mgx_agg_s::ycap, (size_t)rows * (size_t)ld);
  MGX_CATCH
}
int mgx_agg_result(mgx_agg_t p, float* host_y) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, "mgx_agg_result");
  auto [ctx, g] = enter(p);
  ctx.synchronize();
  if (host_y && p->last_rows > 0) {
    MGX_HIP(hipMemcpy2DAsync(host_y, (size_t)p->last_feats * sizeof(float), p->last_y, (size_t)p->last_ldy * sizeof(float),
                             (size_t)p->last_feats * sizeof(float), (size_t)p->last_rows, hipMemcpyDeviceToHost, ctx.stream()));
    ctx.synchronize();
  }
  MGX_CATCH
}
int mgx_agg_bins(mgx_agg_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_agg_bins");
  auto [ctx, g] = enter(p);
  long long b[mgx::AGG_BINS];
  p->fused->bins(b, ctx);
  for (int i = 0; i < mgx::AGG_BINS; ++i) out[i] = b[i];
  MGX_CATCH
}
int mgx_agg_set_timing(mgx_agg_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->timing = on != 0;
  MGX_CATCH
}
int mgx_agg_phase_ms(mgx_agg_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_agg_phase_ms");
  auto [ctx, g] = enter(p);
  p->fused->read_phases(out);
  MGX_CATCH
}

// ---- the backward of the neighbour feature aggregation -----------------------------
// a call's arguments, checked before any device work (the parameters first: their messages do not need a handle)
static mgx::aggb_request_t aggbwd_check(mgx_aggbwd_t p, int source, mgx_nsample_t block, int hop, const float* d_gy, int64_t ldgy, int feats, int op,
                                        int weighted, const float* d_x, int64_t ldx, int64_t x_rows, float* d_gx, int64_t ldgx, const char* who) {
  const std::string w(who);
  const bool minmax = op == mgx::AGG_MAX || op == mgx::AGG_MIN;
  MGX_REQUIRE(feats >= 1 && feats <= mgx::AGG_MAX_FEATS, w + ": feats must be in [1, 65536]");
  MGX_REQUIRE(ldgy >= feats && ldgx >= feats, w + ": ldgy and ldgx must be at least feats");
  MGX_REQUIRE(op >= 0 && op < mgx::AGG_OPS, w + ": op must be 0 (sum), 1 (mean), 2 (max) or 3 (min)");
  MGX_REQUIRE(!minmax || ldx >= feats, w + ": ldx must be at least feats (max and min read X)");
  MGX_REQUIRE(source >= 0 && source < mgx::AGG_SOURCES, w + ": source must be 0 (out-rows), 1 (in-rows) or 2 (block)");
  MGX_REQUIRE(x_rows >= 0 && x_rows <= INT_MAX, w + ": x_rows must be in [0, 2^31)");
  MGX_REQUIRE(p, "NULL argument");
  const graph_device_t& g = p->graph();
  const size_t m = (size_t)g.num_edges;
  mgx::aggb_request_t r;
  r.gy = d_gy; r.x = minmax ? d_x : nullptr; r.gx = d_gx; r.ldgy = ldgy; r.ldx = ldx; r.ldgx = ldgx; r.feats = feats; r.op = op; r.source = source;
  r.T = (int)x_rows;
  long long need_rows = g.num_nodes;
  if (source == mgx::AGG_SRC_OUT) {
    r.ro = g.d_row_offsets.data(); r.ci = g.d_col_indices.data();
    MGX_REQUIRE(!weighted || g.d_col_values.size() >= m, w + ": weighted, and the graph has no weights");
    if (weighted) r.w = g.d_col_values.data();
    r.R = g.num_nodes; r.entries = g.num_edges;
  } else if (source == mgx::AGG_SRC_IN) {
    MGX_REQUIRE(!g.csc_is_csr, w + ": the in-rows need the graph's genuine CSC (mgx_graph_build_csc)");
    r.ro = g.d_col_offsets.data(); r.ci = g.d_row_indices.data();
    MGX_REQUIRE(!weighted || g.d_row_values.size() >= m, w + ": weighted, and the CSC has no weights");
    if (weighted) r.w = g.d_row_values.data();
    r.R = g.num_nodes; r.entries = g.num_edges;
  } else {
    MGX_REQUIRE(block, w + ": source 2 needs a block (an mgx_nsample_t)");
    MGX_REQUIRE(block->g == p->g, w + ": the block was sampled from another graph");
    MGX_REQUIRE(block->last != 0, w + ": the block has no successful sampling run");
    const mgx::ns_results_t& res = block->last == 1 ? block->fused->res : block->op_state->res;
    const int hops = (int)res.hop_offsets.size() - 2;
    MGX_REQUIRE(hop >= -1 && hop < hops, w + ": hop must be -1 (all sampled rows) or in [0, the run's hops)");
    MGX_REQUIRE(!weighted || g.d_col_values.size() >= m, w + ": weighted, and the graph has no weights");
    need_rows = res.count_vertices();
    if (res.device) {
      const int h0 = hop < 0 ? 0 : hop, h1 = hop < 0 ? hops : hop + 1;
      r.ro = res.row_offsets.data() + res.hop_offsets[h0]; r.ci = res.cols.data();
      r.R = res.hop_offsets[h1] - res.hop_offsets[h0];
      r.e0 = res.edge_offsets[h0];
      r.entries = res.edge_offsets[h1] - res.edge_offsets[h0];
      if (weighted) { r.w = g.d_col_values.data(); r.entry_pos = res.entry_pos.data(); }
      r.needs_plan = res.any_whole;
    }
  }
  MGX_REQUIRE(x_rows >= need_rows, w + ": x_rows is below the number of vertices the columns name");
  MGX_REQUIRE(x_rows == 0 || d_gx, w + ": d_gx is NULL");
  MGX_REQUIRE(r.R == 0 || d_gy, w + ": d_gy is NULL");
  MGX_REQUIRE(!minmax || r.R == 0 || d_x, w + ": d_x is NULL, and max and min need the forward's X");
  // the three ranges, pairwise
  struct range_t { const char* b; const char* e; const char* name; };
  auto range = [](const float* p0, long long rows, long long ld, int f, const char* name) {
    const char* const b = (const char*)p0;
    return range_t{b, (p0 && rows > 0) ? b + ((size_t)(rows - 1) * (size_t)ld + (size_t)f) * sizeof(float) : b, name};
  };
  const range_t rg[3] = {range(d_gy, r.R, ldgy, feats, "GY"), range(r.x, r.R > 0 ? x_rows : 0, ldx, feats, "X"), range(d_gx, x_rows, ldgx, feats, "GX")};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      MGX_REQUIRE(rg[i].b == rg[i].e || rg[j].b == rg[j].e || rg[i].e <= rg[j].b || rg[j].e <= rg[i].b,
                  w + ": the ranges of " + rg[i].name + " and " + rg[j].name + " overlap");
  return r;
}
static mgx::aggb_state_t& aggbwd_state(mgx_aggbwd_t p) {
  if (!p->st) p->st.reset(new mgx::aggb_state_t(mgx::agg_seg_from_env()));      // (MGX_AGG_SEG is read once per handle, as the forward reads it)
  return *p->st;
}
static void aggbwd_ran(mgx_aggbwd_t p, const mgx::aggb_request_t& r, int which) {
  p->last_gx = r.gx; p->last_ldgx = r.ldgx; p->last_rows = r.T; p->last_feats = r.feats;
  p->last = which;
}
int mgx_aggbwd_create(mgx_graph_t g, mgx_aggbwd_t* out) { return create_handle(g, out); }
int mgx_aggbwd_free(mgx_aggbwd_t p) { return free_handle(p); }
int mgx_aggbwd_run(mgx_aggbwd_t p, int source, mgx_nsample_t block, int hop, const float* d_gy, int64_t ldgy, int feats, int op, int weighted,
                   const float* d_x, int64_t ldx, int64_t x_rows, float* d_gx, int64_t ldgx, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;                                        // (a run that is refused leaves nothing to the getters)
  const mgx::aggb_request_t r = aggbwd_check(p, source, block, hop, d_gy, ldgy, feats, op, weighted, d_x, ldx, x_rows, d_gx, ldgx, "mgx_aggbwd_run");
  auto [ctx, g] = enter(p);
  mgx::aggb_state_t& st = aggbwd_state(p);
  st.timing = p->timing;
  const std::vector<long long> s = st.run(r, ctx);
  aggbwd_ran(p, r, 1);
  put_stats(stats, mgx::AGGB_STATS, s);
  MGX_CATCH
}
int mgx_aggbwd_enact(mgx_aggbwd_t p, int source, mgx_nsample_t block, int hop, const float* d_gy, int64_t ldgy, int feats, int op, int weighted,
                     const float* d_x, int64_t ldx, int64_t x_rows, float* d_gx, int64_t ldgx, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;
  const mgx::aggb_request_t r = aggbwd_check(p, source, block, hop, d_gy, ldgy, feats, op, weighted, d_x, ldx, x_rows, d_gx, ldgx, "mgx_aggbwd_enact");
  auto [ctx, g] = enter(p);
  mgx::aggb_state_t& st = aggbwd_state(p);
  const mgx::agg_shape_t sh = mgx::agg_shape(feats, mgx::agg_vector_ok(d_gy, ldgy, d_gx, ldgx, feats));
  long long calls = 0, waits = 0, launches = 0;
  bool built = false;
  st.last_tr = nullptr;
  if (r.T > 0) {
    built = st.prepare(r, ctx, launches, waits);              // (the transpose's own launches are not operator calls: its waits are counted)
    const mgx::aggb_transpose_t& t = st.tr[r.source];
    const bool minmax = r.x != nullptr && r.R > 0;
    const long long ldw = ((long long)feats + 3) / 4 * 4;
    const aggbwd::aggbwd_problem_t::data_slice_t slice = {t.t_off.data(), t.t_row.data(), t.t_pos.data(), r.ro, r.ci, r.w ? r.entry_pos : nullptr, r.w,
                                                          r.gy, r.x, r.gx, minmax ? st.ensure_win(r.R, feats, ctx) : nullptr,
                                                          r.ldgy, r.ldx, r.ldgx, ldw, r.feats, r.op, st.seg};
    if (!p->p) p->p = std::make_shared<aggbwd::aggbwd_problem_t>(p->g->g, slice, ctx);
    else MGX_HIP(mgx::htod(p->p->d_data_slice.data(), &slice, 1, ctx.stream()));
    ++waits;
    if (!p->e) p->e.reset(new aggbwd::aggbwd_enactor_t());
    p->e->enact(p->p, r.R, r.T, minmax, ctx);
    calls = p->e->calls; waits += p->e->waits;
  }
  aggbwd_ran(p, r, 2);
  put_stats(stats, mgx::AGGB_STATS, {r.T, r.entries, r.feats, sh.G, sh.tiles, sh.vector, st.seg, calls, waits, built ? 1 : 0});
  MGX_CATCH
}
// a handle-owned array grown to `want` floats (growing only)
static float* aggbwd_buffer(mgx_aggbwd_t p, mem_t<float>& buf, size_t& cap, size_t want) {
  if (want > cap) {
    p->ctx().synchronize();                                  // (a queued run may still read the old one)
    buf = mem_t<float>();
    cap = 0;
    buf = mem_t<float>(want, p->ctx());
    cap = want;
  }
  return buf.data();
}
int mgx_aggbwd_upload(mgx_aggbwd_t p, int which, const float* host, int64_t rows, int feats, float** d_out) {
  MGX_TRY
  MGX_REQUIRE(p && d_out && rows >= 0 && feats >= 1 && (host || rows == 0), "mgx_aggbwd_upload: NULL or negative argument");
  MGX_REQUIRE(which == 0 || which == 1, "mgx_aggbwd_upload: which must be 0 (GY) or 1 (X)");
  auto [ctx, g] = enter(p);
  const size_t count = (size_t)rows * (size_t)feats;
  *d_out = aggbwd_buffer(p, p->inbuf[which], p->incap[which], count);
  MGX_HIP(mgx::htod(*d_out, host, count, ctx.stream()));
  MGX_CATCH
}
int mgx_aggbwd_output(mgx_aggbwd_t p, int64_t rows, int64_t ld, float** d_gx) {
  MGX_TRY
  MGX_REQUIRE(p && d_gx && rows >= 0 && ld >= 1, "mgx_aggbwd_output: NULL or negative argument");
  auto [ctx, g] = enter(p);
  *d_gx = aggbwd_buffer(p, p->outbuf, p->outcap, (size_t)rows * (size_t)ld);
  MGX_CATCH
}
int mgx_aggbwd_result(mgx_aggbwd_t p, float* host_gx) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, "mgx_aggbwd_result");
  auto [ctx, g] = enter(p);
  ctx.synchronize();
  if (host_gx && p->last_rows > 0) {
    MGX_HIP(hipMemcpy2DAsync(host_gx, (size_t)p->last_feats * sizeof(float), p->last_gx, (size_t)p->last_ldgx * sizeof(float),
                             (size_t)p->last_feats * sizeof(float), (size_t)p->last_rows, hipMemcpyDeviceToHost, ctx.stream()));
    ctx.synchronize();
  }
  MGX_CATCH
}
int mgx_aggbwd_transpose(mgx_aggbwd_t p, int* offsets, int* rows, int* pos) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, "mgx_aggbwd_transpose");
  const mgx::aggb_transpose_t* t = p->st->last_tr;
  if (t) {
    if (offsets) read_back(p, offsets, (const int*)t->t_off.data(), (size_t)t->T + 1);
    if (rows) read_back(p, rows, (const int*)t->t_row.data(), (size_t)t->E);
    if (pos) read_back(p, pos, (const int*)t->t_pos.data(), (size_t)t->E);
  }
  MGX_CATCH
}
int mgx_aggbwd_bins(mgx_aggbwd_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_aggbwd_bins");
  auto [ctx, g] = enter(p);
  long long b[mgx::AGGB_BINS];
  p->st->bins(b, ctx);
  for (int i = 0; i < mgx::AGGB_BINS; ++i) out[i] = b[i];
  MGX_CATCH
}
int mgx_aggbwd_set_timing(mgx_aggbwd_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->timing = on != 0;
  MGX_CATCH
}
int mgx_aggbwd_phase_ms(mgx_aggbwd_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_aggbwd_phase_ms");
  auto [ctx, g] = enter(p);
  p->st->read_phases(out);
  MGX_CATCH
}

// ---- vertex similarity for link prediction -----------------------------------------
static mgx::sim_state_t& sim_state(mgx_sim_t p) {
  if (!p->st) p->st.reset(new mgx::sim_state_t(p->graph().num_nodes, p->graph().num_edges, p->ctx()));
  return *p->st;
}
// a run's arguments, checked before any device work (the ids are checked on the device)
static void sim_check(mgx_sim_t p, const int* h_u, const int* h_v, int pairs, int measure, const double* h_x, const char* who) {
  const std::string w(who);
  MGX_REQUIRE(p, "NULL argument");
  MGX_REQUIRE(measure >= 0 && measure < mgx::SIM_MEASURES, w + ": measure must be one of MGX_SIM_*");
  MGX_REQUIRE((h_u == nullptr) == (h_v == nullptr), w + ": of the two pair arrays one is NULL");
  MGX_REQUIRE(!h_u || pairs >= 0, w + ": pairs must not be negative");
  MGX_REQUIRE(measure != mgx::SIM_WEIGHTED || h_x, w + ": MGX_SIM_WEIGHTED needs the weights h_x");
}
static const mgx::sim_results_t& sim_results(mgx_sim_t p, const char* who) {
  MGX_REQUIRE(p, "NULL argument");
  require_run(p->last != 0, who);
  return p->last == 1 ? p->st->res : p->op_res;
}
int mgx_sim_create(mgx_graph_t g, mgx_sim_t* out) { return create_handle(g, out); }
int mgx_sim_free(mgx_sim_t p) { return free_handle(p); }
int mgx_sim_prepare(mgx_sim_t p, int symmetric) {
  MGX_TRY
  auto [ctx, g] = enter(p);
  sim_state(p).prepare(symmetric != 0, g.d_row_offsets.data(), g.d_col_indices.data(), ctx);
  p->sym = symmetric != 0 ? 1 : 0;
  MGX_CATCH
}
int mgx_sim_run(mgx_sim_t p, int symmetric, const int* h_u, const int* h_v, int pairs, int measure, const double* h_x, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;                                          // (a run that is refused leaves nothing to the getters)
  sim_check(p, h_u, h_v, pairs, measure, h_x, "mgx_sim_run");
  auto [ctx, g] = enter(p);
  mgx::sim_state_t& st = sim_state(p);
  st.timing = p->timing;
  const std::vector<long long> out = st.run(g.d_row_offsets.data(), g.d_col_indices.data(), symmetric != 0, h_u, h_v, pairs, measure, h_x, ctx);
  p->sym = symmetric != 0 ? 1 : 0;
  p->last = 1;
  put_stats(stats, mgx::SIM_STATS, out);
  MGX_CATCH
}
int mgx_sim_enact(mgx_sim_t p, int symmetric, const int* h_u, const int* h_v, int pairs, int measure, const double* h_x, int64_t* stats) {
  MGX_TRY
  if (p) p->last = 0;
  sim_check(p, h_u, h_v, pairs, measure, h_x, "mgx_sim_enact");
  auto [ctx, g] = enter(p);
  mgx::sim_state_t& st = sim_state(p);
  const int sym = symmetric != 0 ? 1 : 0;
  const bool timing = st.timing;
  st.timing = false;                                           // (the phases describe fused runs)
  const bool built_now = st.begin(sym != 0, g.d_row_offsets.data(), g.d_col_indices.data(), ctx);
  st.timing = timing;
  p->op_res.pairs = 0;
  std::vector<long long> out = {0, 0, 0, 0, 0, 0, 0, 0};
  if (st.n > 0) {
    const hipStream_t s = ctx.stream();
    mgx::ktruss_graph_t& kg = st.kt.gr[sym];
    const long long P = h_u ? pairs : kg.m;
    const bool weighted = measure == mgx::SIM_WEIGHTED;
    mgx::sim_results_t& res = p->op_res;
    res.ensure((size_t)P, weighted, st.n, ctx);
    if (p->op_sums.size() == 0) p->op_sums = mem_t<unsigned long long>(2, ctx);
    res.upload(h_u, h_v, P, kg.src.data(), st.kt.tc.dag[sym].ci.data(), weighted ? h_x : nullptr, st.n, s);
    MGX_HIP(hipMemsetAsync(p->op_sums.data(), 0, 2 * sizeof(unsigned long long), s));
    const sim::sim_problem_t::data_slice_t slice = {kg.adj_ro.data(), kg.adj_ci.data(), res.u, res.v, weighted ? res.x.data() : nullptr,
                                                    res.common.data(), res.score.data(), p->op_sums.data(), st.n, measure};
    if (!p->p) p->p = std::make_shared<sim::sim_problem_t>(p->g->g, slice, ctx);
    else MGX_HIP(mgx::htod(p->p->d_data_slice.data(), &slice, 1, s));
    long long waits = 1, positive = 0, calls = 0;              // (the data slice goes up with a blocking copy)
    if (P > 0) {
      if (!p->e || (size_t)P > p->e->cap) {
        p->e.reset();
        p->e.reset(new sim::sim_enactor_t(ctx, (size_t)P));
      }
      positive = p->e->enact(p->p, P, ctx);
      waits += p->e->waits;
      calls = p->e->calls;
    }
    unsigned long long sums[2] = {0, 0};
    MGX_HIP(mgx::dtoh(sums, (const unsigned long long*)p->op_sums.data(), 2, s));
    ++waits;
    MGX_REQUIRE(!sums[1], "mgx_sim_enact: a pair names a vertex outside [0, n)");
    const long long longest = st.longest_row(sym, ctx);
    out = {P, (long long)sums[0], positive, 2ll * kg.m, longest, built_now ? 1 : 0, st.kt.tc.waits + waits, st.kt.tc.launches + 1 + 2 * calls};
  }
  p->sym = sym;
  p->last = 2;
  put_stats(stats, mgx::SIM_STATS, out);
  MGX_CATCH
}
int mgx_sim_common(mgx_sim_t p, int* host) {
  MGX_TRY
  const mgx::sim_results_t& res = sim_results(p, "mgx_sim_common");
  if (host) read_back(p, host, (const int*)res.common.data(), (size_t)res.pairs);
  MGX_CATCH
}
int mgx_sim_scores(mgx_sim_t p, double* host) {
  MGX_TRY
  const mgx::sim_results_t& res = sim_results(p, "mgx_sim_scores");
  if (host) read_back(p, host, (const double*)res.score.data(), (size_t)res.pairs);
  MGX_CATCH
}
int mgx_sim_common_device(mgx_sim_t p, const int** out) {
  MGX_TRY
  const mgx::sim_results_t& res = sim_results(p, "mgx_sim_common_device");
  MGX_REQUIRE(out, "NULL argument");
  *out = res.pairs ? res.common.data() : nullptr;
  MGX_CATCH
}
int mgx_sim_scores_device(mgx_sim_t p, const double** out) {
  MGX_TRY
  const mgx::sim_results_t& res = sim_results(p, "mgx_sim_scores_device");
  MGX_REQUIRE(out, "NULL argument");
  *out = res.pairs ? res.score.data() : nullptr;
  MGX_CATCH
}
int mgx_sim_pairs(mgx_sim_t p, int* h_u, int* h_v) {
  MGX_TRY
  const mgx::sim_results_t& res = sim_results(p, "mgx_sim_pairs");
  if (h_u) read_back(p, h_u, res.u, (size_t)res.pairs);
  if (h_v) read_back(p, h_v, res.v, (size_t)res.pairs);
  MGX_CATCH
}
int mgx_sim_degrees(mgx_sim_t p, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  MGX_REQUIRE(p->sym >= 0, "mgx_sim_degrees: no adjacency yet (mgx_sim_prepare)");
  const size_t n = p->n();
  if (n == 0) return MGX_OK;
  std::vector<int> ro(n + 1);
  read_back(p, ro.data(), (const int*)p->st->kt.gr[p->sym].adj_ro.data(), n + 1);
  for (size_t v = 0; v < n; ++v) host[v] = ro[v + 1] - ro[v];
  MGX_CATCH
}
int mgx_sim_bins(mgx_sim_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_sim_bins");
  const mgx::sim_state_t& st = *p->st;
  for (int i = 0; i < mgx::SIM_CLASSES; ++i) out[i] = st.bins[i];
  out[5] = st.opts.short_max; out[6] = st.opts.probe_ratio; out[7] = st.opts.wave_max; out[8] = st.opts.stage; out[9] = st.entries_read;
  MGX_CATCH
}
int mgx_sim_set_timing(mgx_sim_t p, int on) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->timing = on != 0;
  MGX_CATCH
}
int mgx_sim_phase_ms(mgx_sim_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_sim_phase_ms");
  for (int i = 0; i < 3; ++i) out[i] = p->st->phase_ms[i];
  MGX_CATCH
}

// ---- Louvain community detection ---------------------------------------------------
static void louvain_check_args(const graph_device_t& g, int symmetric, int max_iter, int max_levels, double tol, const char* who) {
  MGX_REQUIRE(max_iter >= 0 && max_iter <= mgx::LV_MAX_ITER_MAX, std::string(who) + ": max_iter must be in [0, 2^20]");
  MGX_REQUIRE(max_levels >= 0 && max_levels <= mgx::LV_MAX_LEVELS_MAX, std::string(who) + ": max_levels must be in [0, 64]");
  MGX_REQUIRE(tol >= 0.0 && tol <= 1.0, std::string(who) + ": tol must be in [0, 1]");      // (false for a NaN)
  MGX_REQUIRE(symmetric || !g.csc_is_csr, std::string(who) + ": symmetric = 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
  if ((long long)g.num_edges > (1ll << 30)) throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, std::string(who) + ": more than 2^30 entries");
  // (the contraction addresses the votes, W <= the entries or twice as many, by int32)
  if (!symmetric && (long long)g.num_edges >= (1ll << 30) - 1)
    throw mgx::mgx_error(MGX_E_FRONTIER_OVERFLOW, std::string(who) + ": symmetric = 0 takes fewer than 2^30 - 1 entries");
}
long long mgx_device_allocations(void) { return mgx::device_allocations().load(); }
int mgx_louvain_create(mgx_graph_t g, mgx_louvain_t* out) { return create_handle(g, out); }
int mgx_louvain_free(mgx_louvain_t p) { return free_handle(p); }
int mgx_louvain_run(mgx_louvain_t p, int symmetric, uint32_t seed, int max_iter, int max_levels, double tol, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->last = 0;                                               // (a run that is refused leaves nothing to the getters either)
  louvain_check_args(p->graph(), symmetric, max_iter, max_levels, tol, "mgx_louvain_run");
  auto [ctx, g] = enter(p);
  if (!p->fused) p->fused.reset(new mgx::louvain_fused_state_t(g.num_nodes, g.num_edges, ctx));
  const std::vector<long long> st = p->fused->run(g.d_row_offsets.data(), g.d_col_indices.data(), g.d_col_offsets.data(),
                                                  g.d_row_indices.data(), symmetric, seed, max_iter, max_levels, tol, ctx);
  p->last = 1;
  put_stats(stats, 10, st);
  MGX_CATCH
}
int mgx_louvain_enact(mgx_louvain_t p, int symmetric, uint32_t seed, int max_iter, int max_levels, double tol, int64_t* stats) {
  MGX_TRY
  MGX_REQUIRE(p, "NULL argument");
  p->last = 0;
  louvain_check_args(p->graph(), symmetric, max_iter, max_levels, tol, "mgx_louvain_enact");
  auto [ctx, g] = enter(p);
  const int n = g.num_nodes;
  if (!p->e) p->e.reset(new louvain::louvain_enactor_t(ctx, n, g.num_edges));
  if (n <= 0) {
    p->e->levels.clear(); p->e->trace.clear(); p->e->map_off.assign(1, 0);
    p->last = 2;
    put_stats(stats, 10, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
    return MGX_OK;
  }
  const long long entries = symmetric ? (long long)g.num_edges : 2ll * g.num_edges;
  if (!p->op_state || p->op_entries < entries) {
    ctx.synchronize();
    p->op_state.reset(new louvain::louvain_state_t(n, entries, ctx));
    p->op_agg.reset(new mgx::louvain_aggregate_t(n, entries, ctx));
    p->op_entries = entries;
  }
  if (!p->label_stats) p->label_stats.reset(new mgx::lpa_label_stats_t(n, ctx));
  louvain::louvain_enactor_t& e = *p->e;
  e.enact(p->g->g, *p->op_state, *p->op_agg, symmetric != 0, seed, max_iter, max_levels, tol, ctx);
  const std::vector<long long> st = p->label_stats->run(p->op_state->d_final.data(), n, ctx);
  p->last = 2;
  put_stats(stats, 10, {st[0], st[1], st[2], (long long)e.map_off.size() - 1, e.s_in, e.s_sq, e.w, e.waits + 1, e.calls, e.iterations});
  MGX_CATCH
}
// the labels of `level` of the last run: where they are and how many
static const int* louvain_level(mgx_louvain_t p, int level, size_t* count, const char* who) {
  require_run(p->last != 0, who);
  const std::vector<long long>& off = p->last == 1 ? p->fused->map_off : p->e->map_off;
  const int levels = (int)off.size() - 1;
  MGX_REQUIRE(level >= -1 && level < levels, std::string(who) + ": level must be -1 or below the levels aggregated");
  if (level < 0) { *count = p->n(); return p->last == 1 ? p->fused->final_lab.data() : p->op_state->d_final.data(); }
  *count = (size_t)(off[level + 1] - off[level]);
  return (p->last == 1 ? p->fused->maps.data() : p->op_state->d_maps.data()) + off[level];
}
int mgx_louvain_labels(mgx_louvain_t p, int level, int* host) {
  MGX_TRY
  MGX_REQUIRE(p && host, "NULL argument");
  size_t count = 0;
  const int* const src = louvain_level(p, level, &count, "mgx_louvain_labels");
  read_back(p, host, src, count);
  MGX_CATCH
}
int mgx_louvain_labels_device(mgx_louvain_t p, int level, const int** out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  size_t count = 0;
  *out = louvain_level(p, level, &count, "mgx_louvain_labels_device");
  MGX_CATCH
}
int mgx_louvain_levels(mgx_louvain_t p, int64_t* host_sextuples, int cap, int64_t* levels_run) {
  MGX_TRY
  MGX_REQUIRE(p && levels_run && cap >= 0 && (host_sextuples || cap == 0), "bad argument");
  require_run(p->last != 0, "mgx_louvain_levels");
  if (p->last == 2) {
    const std::vector<long long>& l = p->e->levels;
    *levels_run = (int64_t)l.size() / 6;
    std::copy(l.begin(), l.begin() + 6 * std::min<size_t>(l.size() / 6, (size_t)cap), host_sextuples);
    return MGX_OK;
  }
  const std::vector<mgx::lv_level_t>& l = p->fused->levels;
  *levels_run = (int64_t)l.size();
  for (size_t i = 0; i < std::min<size_t>(l.size(), (size_t)cap); ++i) {
    int64_t* const o = host_sextuples + 6 * i;
    o[0] = l[i].vertices; o[1] = l[i].entries; o[2] = l[i].iterations; o[3] = l[i].accepted; o[4] = l[i].communities; o[5] = l[i].q;
  }
  MGX_CATCH
}
int mgx_louvain_trace(mgx_louvain_t p, int64_t* host_triples, int cap, int64_t* iterations) {
  MGX_TRY
  MGX_REQUIRE(p && iterations && cap >= 0 && (host_triples || cap == 0), "bad argument");
  require_run(p->last != 0, "mgx_louvain_trace");
  const std::vector<long long>& t = p->last == 1 ? p->fused->h_trace : p->e->trace;
  const long long have = (long long)t.size() / 3;
  *iterations = have;
  std::copy(t.begin(), t.begin() + 3 * std::min<long long>(have, cap), host_triples);
  MGX_CATCH
}
int mgx_louvain_step_kinds(mgx_louvain_t p, int* host_kinds, int cap, int64_t* launches) {
  MGX_TRY
  MGX_REQUIRE(p && launches && cap >= 0 && (host_kinds || cap == 0), "bad argument");
  require_run(p->last == 1, "mgx_louvain_step_kinds");
  const std::vector<int>& k = p->fused->kinds;
  *launches = (int64_t)k.size();
  std::copy(k.begin(), k.begin() + std::min<size_t>(k.size(), (size_t)cap), host_kinds);
  MGX_CATCH
}
int mgx_louvain_bins(mgx_louvain_t p, int64_t* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_louvain_bins");
  const mgx::louvain_fused_state_t& f = *p->fused;
  for (int i = 0; i < 4; ++i) out[i] = f.bins[i];
  out[4] = f.opts.cuts.short_max; out[5] = f.opts.cuts.wave_max; out[6] = f.opts.cuts.seg; out[7] = f.long_items;
  MGX_CATCH
}
int mgx_louvain_set_timing(mgx_louvain_t p, int on) { return chain_set_timing(p, &mgx_louvain_s::fused, on); }
int mgx_louvain_phase_ms(mgx_louvain_t p, double* out) {
  MGX_TRY
  MGX_REQUIRE(p && out, "NULL argument");
  require_run(p->last == 1, "mgx_louvain_phase_ms");
  for (int i = 0; i < 6; ++i) out[i] = p->fused->phase_ms[i];
  MGX_CATCH
}

}  // extern "C"

// ---- R-MAT generator (spec: oracle/oracle.c orc_rmat_edges) -----------------------
namespace {
__global__ void k_rmat_edges(int scale, long long first_edge, long long count, unsigned long long seed, int do_scramble,
                             int* __restrict__ src, int* __restrict__ dst, float* __restrict__ weight) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < count; i += stride) {
    const unsigned long long e = (unsigned long long)(first_edge + i);
    unsigned s, d;
    mgx::rmat_pair(scale, seed, e, do_scramble, s, d);
    src[i] = (int)s;
    dst[i] = (int)d;
    if (weight) weight[i] = mgx::rmat_weight(seed, e);
  }
}
}  // namespace

extern "C" int mgx_rmat_edges(mgx_ctx_t c, int scale, int64_t first_edge, int64_t count, uint64_t seed, int scramble_ids,
                              int* d_src, int* d_dst, float* d_weight) {
  MGX_TRY
  MGX_REQUIRE(c && d_src && d_dst && scale >= 1 && scale <= 31 && count >= 0 && first_edge >= 0,
              "mgx_rmat_edges: bad argument");
  use_device(c);
  if (count > 0)
    hipLaunchKernelGGL(k_rmat_edges, dim3(mgx::grid_for(count, 256, 8192)), dim3(256), 0, c->ctx->stream(), scale,
                       (long long)first_edge, (long long)count, (unsigned long long)seed, scramble_ids, d_src, d_dst,
                       d_weight);
  MGX_CATCH
}
