// mgx/ktruss_fused.hpp -- k-truss decomposition (mgx_ktruss_run, mgx_ktruss_enact): the adjacency with edge ids and the supports
// both paths peel on, and the fused peel.
//
// The definition (the operator path include/gunrock/ktruss/ and tests/ktruss_model.py compute the same):
//   the graph is the underlying simple undirected graph of DESIGN 3.10; its edges are the entries of the oriented graph (DAG) the
//   triangle count builds: edge e = position e of dag_ci, joining row a (src[e]) to dag_ci[e]; m_dag of them.
//   sup0[e] = the triangles that contain e.  An edge is alive, in the front, or removed.
//   loop: no edge alive: stop.  k = 2 + min(sup over alive edges).  front = { alive e : sup[e] <= k - 2 }
//         while the front is not empty (one PASS):
//             every triangle {e, e1, e2} with e in the front and e1, e2 not removed:
//                 neither e1 nor e2 in the front: sup[e1] -= 1, sup[e2] -= 1
//                 exactly one of them in the front: the third loses 1, ONCE per triangle (here: charged by the lower edge id)
//                 both in the front: nothing
//             truss[front] = k, the front is removed
//             front = the alive edges whose sup this pass took from > k - 2 to <= k - 2
//   vtruss[v] = the largest trussness of an edge at v (0: none), hist[k] = edges of trussness k.
//   Every edge enters a front exactly once: order[m_dag], appended to throughout the run, holds every front as a range and is the
//   peel order.
//
// The build (once per `symmetric` value, kept on the handle beside the DAG of tc_state_t::ensure_dag):
//   adj_ro = scan of sdeg (the DAG's build leaves it); k_ktruss_adj_fill writes row a's DAG entries in order at the head of row a
//   and each entry's reverse behind the forward entries of the row it names, through a cursor; the rows are then sorted by
//   neighbour with the edge id as the value (segsort.hpp; the keys of a row are distinct, so the result does not depend on the
//   cursors' order).  The sort's host side waits twice: both waits are counted in the first run's host waits.
//
// The supports: the three count kernels of tc_fused.hpp with EDGES = true: the adds go to the three entries of a triangle.
//
// The peel: a chain of launches of k_ktruss_step (launch_chain.hpp: the ring, the log, the host's batches).  A launch derives its
// kind from the word the launch before left: its kind, its k, the range of `order` it worked on, what it appended and listed.
//   MIN     over all edges: the smallest sup of an alive edge (a level begins), or nobody is alive: DONE
//   LIST    over all edges: the alive ones at sup <= k - 2 are appended to `order`
//   SEAL    over the front just expanded (none behind a LIST): truss = k, state removed, atomicMax on vtruss of both ends; over what
//           the launch before appended to `order`: state front, and into the next EXPAND's work lists by the length of the shorter
//           adjacency row of its ends.  A step of its own because "after all of this pass's reads of the states and before any of
//           the next pass's" is a launch boundary.  An empty new front: the level is over, MIN follows.
//   EXPAND  the front's triangles: for edge {u, v} the entries of the shorter of rows u, v are searched in the longer; the two
//           other edges' ids come from adj_eid, their states are plain loads (states change in SEAL only), the rule above with
//           returning decrements; the one that returns k - 1 has crossed and appends its edge to `order` -- once per edge and run.
//           Shorter rows of at most short_max entries: a lane per edge, the wave walking its edges in step.  Longer: (edge, segment)
//           items of `seg` entries, a wave each, consecutive lanes taking consecutive entries.  The item list holds m_dag + 64
//           items; an edge whose segments do not fit goes to a third list and is walked whole by one wave (right, and slower).
//   DONE
// Atomics: sup changes by 32-bit device-scope atomicAdd only (supports: adds; peel: returning decrements, not clamped); list
// appends through wave-private LDS stages behind one returning add each (worklist.hpp); nothing is read back inside a launch.
// No cooperative launch, no grid-wide barrier; every device loop is bounded by a list size read once.
// Not built: kcore's MINI kind (one workgroup running a small front's passes on its own), MIN folded into the level before it,
// dropping removed entries from the adjacency at level boundaries.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "env.hpp"
#include "launch_chain.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "segsort.hpp"
#include "tc_fused.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (both defaults are unmeasured guesses until tools/ktruss_bench.py has run on the device)
constexpr int KTRUSS_SHORT_MAX_DEFAULT = 16;   // shorter rows of at most this many entries: a lane per edge
constexpr int KTRUSS_SEG_DEFAULT = 512;        // entries of the shorter row one wave takes
constexpr int KTRUSS_STAGE = 2 * WAVE;         // a wave's LDS stage of list appends

enum ktruss_kind_t : int { KTRUSS_INIT = 0, KTRUSS_MIN = 1, KTRUSS_LIST = 2, KTRUSS_EXPAND = 3, KTRUSS_SEAL = 4, KTRUSS_DONE = 5 };
enum : int { KTRUSS_ALIVE = 0, KTRUSS_FRONT = 1, KTRUSS_REMOVED = 2 };

struct ktruss_opts_t {
  int short_max = KTRUSS_SHORT_MAX_DEFAULT, seg = KTRUSS_SEG_DEFAULT;
  static ktruss_opts_t from_env() {
    ktruss_opts_t o;
    o.short_max = env_int("MGX_KTRUSS_SHORT_MAX", 0, INT_MAX, o.short_max);
    o.seg = env_int("MGX_KTRUSS_SEG", 1, INT_MAX, o.seg);
    return o;
  }
};

// what a launch leaves for the next one (cleared two launches ahead)
struct ktruss_word_t {
  unsigned long long n_items;   // SEAL: (edge, segment) items as reserved (the list holds item_cap; the rest went to `whole`)
  int kind;        // what the launch was
  int k;           // the level it worked at
  int lo, hi;      // order[lo, hi): the front an EXPAND expands / has expanded (LIST, MIN: empty, at base)
  int base;        // entries of `order` when the launch began (== hi)
  int app;         // entries the launch appended to `order`
  int min_enc;     // MIN: INT_MAX - (smallest sup of an alive edge); 0: nobody is alive
  int n_short;     // SEAL: the next EXPAND's other lists: edges a lane takes,
  int n_whole;     //       edges a wave walks whole
};

struct ktruss_totals_t {
  long long levels, passes, triangles;
  int largest, done;
};

using ktruss_control_t = chain_control_t<ktruss_word_t, ktruss_totals_t>;

struct ktruss_adj_args_t {
  const int* dag_ro;
  const int* dag_ci;
  int n;
  const int* adj_ro;
  int* adj_ci;
  int* adj_eid;
  int* src;
  int* cur;        // the reverse entries' cursors (cleared before)
};

// Row a's DAG entries (groups of 8 lanes a row): forward in order at the head of adjacency row a, each one's reverse behind the
// forward entries of row b at b's cursor; src[e] = a.  Slots: adj_ro is the scan of sdeg = d+ + entries that name the vertex.
__global__ __launch_bounds__(BLOCK) void k_ktruss_adj_fill(ktruss_adj_args_t a) {
  constexpr int G = 8;
  const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x, gthreads = (long long)gridDim.x * BLOCK;
  const int sub = (int)(gtid % G);
  for (long long v = gtid / G; v < a.n; v += gthreads / G) {
    const int beg = a.dag_ro[v], end = a.dag_ro[v + 1];
    const int head = a.adj_ro[v];
    for (int e = beg + sub; e < end; e += G) {
      const int b = a.dag_ci[e];
      a.src[e] = (int)v;
      a.adj_ci[head + (e - beg)] = b;
      a.adj_eid[head + (e - beg)] = e;
      const int slot = a.adj_ro[b] + (a.dag_ro[b + 1] - a.dag_ro[b]) + atomicAdd(a.cur + b, 1);
      a.adj_ci[slot] = (int)v;
      a.adj_eid[slot] = e;
    }
  }
}

// adj_ro[n] must be twice the DAG's entries: everything behind it is sized by that
__global__ void k_ktruss_adj_check(const int* adj_ro, int n, long long want, u64* stat) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && (long long)adj_ro[n] != want) stat[TC_S_ERR] = 1;
}

// stat[TC_S_TOTAL] += sum of sup (the operator path's triangles are this sum / 3); one add per workgroup
__global__ __launch_bounds__(BLOCK) void k_ktruss_sum(const int* sup, int m, u64* stat) {
  u64 mine = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (long long)gridDim.x * BLOCK) mine += (u64)sup[i];
  tc_flush_total(mine, stat + TC_S_TOTAL);
}

struct ktruss_step_args_t {
  const int* dag_ci;
  const int* src;
  const int* adj_ro;
  const int* adj_ci;
  const int* adj_eid;
  int* sup;
  int* state;
  int* truss;
  int* vtruss;
  int* hist;
  int* order;
  int* f_short;
  int2* f_items;
  int* f_whole;
  const u64* stat;               // the DAG's stat words (the supports' total)
  ktruss_control_t* ctl;
  int n, m;                      // vertices, edges (m_dag)
  int short_max, seg, item_cap;
};

// the two adjacency rows of edge e, the shorter one first: (start, length) each
__device__ __forceinline__ void ktruss_rows(const ktruss_step_args_t& a, int e, int& s, int& sl, int& l, int& ll) {
  const int u = a.src[e], v = a.dag_ci[e];
  s = a.adj_ro[u]; sl = a.adj_ro[u + 1] - s;
  l = a.adj_ro[v]; ll = a.adj_ro[v + 1] - l;
  if (sl > ll) {
    const int t = s; s = l; l = t;
    const int tl = sl; sl = ll; ll = tl;
  }
}

// One entry of the shorter row of front edge e (at position i; `on`: this lane has one) against the longer row [l, l + ll): the
// triangle's other two edges, the rule, and the crossing decrements' appends.  All lanes of the wave call it.
__device__ __forceinline__ void ktruss_entry(const ktruss_step_args_t& a, bool on, int e, int i, int l, int ll, int k, int* out, int* counter,
                                             int* stage, int& fill) {
  int x1 = -1, x2 = -1;                                      // the edges this lane decrements
  if (on) {
    const int e1 = a.adj_eid[i];
    const int s1 = a.state[e1];
    if (e1 != e && s1 != KTRUSS_REMOVED) {
      const int w = a.adj_ci[i];
      int lo = l, hi = l + ll;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.adj_ci[mid] < w) lo = mid + 1;
        else hi = mid;
      }
      if (lo < l + ll && a.adj_ci[lo] == w) {
        const int e2 = a.adj_eid[lo];
        const int s2 = a.state[e2];
        if (s2 != KTRUSS_REMOVED) {
          const bool f1 = s1 == KTRUSS_FRONT, f2 = s2 == KTRUSS_FRONT;
          if (!f1 && !f2) { x1 = e1; x2 = e2; }
          else if (f1 && !f2) { if (e < e1) x1 = e2; }
          else if (f2 && !f1) { if (e < e2) x1 = e1; }
        }
      }
    }
  }
  const bool c1 = x1 >= 0 && atomicAdd(a.sup + x1, -1) == k - 1;
  const bool c2 = x2 >= 0 && atomicAdd(a.sup + x2, -1) == k - 1;
  wave_stage_push<KTRUSS_STAGE>(c1, x1, stage, fill, out, counter);
  wave_stage_push<KTRUSS_STAGE>(c2, x2, stage, fill, out, counter);
}

// entries [j0, j1) of the shorter row of edge e by one wave, consecutive lanes consecutive entries
__device__ __forceinline__ void ktruss_wave_range(const ktruss_step_args_t& a, int e, int j0, int seg, int k, int* out, int* counter, int* stage,
                                                  int& fill) {
  int s, sl, l, ll;
  ktruss_rows(a, e, s, sl, l, ll);
  const int j1 = seg > 0 ? min(sl, j0 + seg) : sl;
  for (int j = j0; j < j1; j += WAVE) {
    const bool on = j + lane_id() < j1;
    ktruss_entry(a, on, e, s + j + lane_id(), l, ll, k, out, counter, stage, fill);
  }
}

// launch: the launch's number in the run
__global__ __launch_bounds__(BLOCK) void k_ktruss_step(ktruss_step_args_t a, unsigned launch) {
  const ktruss_word_t prev = a.ctl->left_by_prev(launch);
  ktruss_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left
  const int cur_n = prev.base + prev.app;                    // entries of `order` now
  int kind, k = prev.k, lo = cur_n, hi = cur_n;
  switch (prev.kind) {
    case KTRUSS_INIT: kind = KTRUSS_MIN; break;
    case KTRUSS_MIN:
      if (prev.min_enc == 0) kind = KTRUSS_DONE;
      else { kind = KTRUSS_LIST; k = 0x7fffffff - prev.min_enc + 2; }
      break;
    case KTRUSS_LIST: kind = KTRUSS_SEAL; lo = prev.hi; break;       // (nothing expanded: order[prev.hi, cur_n) is the new front)
    case KTRUSS_EXPAND: kind = KTRUSS_SEAL; lo = prev.hi; break;
    case KTRUSS_SEAL:
      if (prev.hi > prev.lo) { kind = KTRUSS_EXPAND; lo = prev.lo; hi = prev.hi; }
      else kind = KTRUSS_MIN;
      break;
    default: kind = KTRUSS_DONE; break;
  }
  if (first_thread) {
    next->kind = kind;
    next->k = k;
    next->lo = lo;
    next->hi = hi;
    next->base = cur_n;
    a.ctl->log_kind(launch, kind);
    if (kind == KTRUSS_LIST) a.ctl->totals.levels += 1;
    if (kind == KTRUSS_EXPAND) a.ctl->totals.passes += 1;
    if (kind == KTRUSS_DONE && prev.kind != KTRUSS_DONE) {
      a.ctl->totals.largest = prev.k;
      a.ctl->totals.triangles = (long long)a.stat[TC_S_TOTAL];
      a.ctl->totals.done = 1;
    }
  }
  if (kind == KTRUSS_DONE) return;

  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  __shared__ int stages[WAVES_PER_BLOCK][KTRUSS_STAGE];
  __shared__ int block_best[WAVES_PER_BLOCK];
  int* const stage = stages[threadIdx.x / WAVE];
  int fill = 0;
  int* const out = a.order + cur_n;                          // where this launch appends

  if (kind == KTRUSS_MIN) {
    int best = 0x7fffffff;
    for (unsigned e = gtid; e < (unsigned)a.m; e += gthreads)
      if (a.state[e] == KTRUSS_ALIVE) best = min(best, max(a.sup[e], 0));
    best = wave_min(best);
    if (lane == 0) block_best[threadIdx.x / WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {                                  // one add a workgroup, if it would change anything
#pragma unroll
      for (int w = 0; w < WAVES_PER_BLOCK; ++w) best = min(best, block_best[w]);
      const int enc = 0x7fffffff - best;
      if (enc > 0 && __hip_atomic_load(&next->min_enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < enc) atomicMax(&next->min_enc, enc);
    }
    return;
  }

  if (kind == KTRUSS_LIST) {
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)a.m; base += (unsigned)waves * WAVE) {
      const unsigned e = base + lane;
      const bool take = e < (unsigned)a.m && a.state[e] == KTRUSS_ALIVE && a.sup[e] <= k - 2;
      wave_stage_push<KTRUSS_STAGE>(take, (int)e, stage, fill, out, &next->app);
    }
    wave_stage_flush(stage, fill, out, &next->app);
    return;
  }

  if (kind == KTRUSS_SEAL) {
    // the front just expanded leaves
    for (unsigned i = (unsigned)prev.lo + gtid; i < (unsigned)prev.hi; i += gthreads) {
      const int e = a.order[i];
      a.truss[e] = k;
      a.state[e] = KTRUSS_REMOVED;
      const int u = a.src[e], v = a.dag_ci[e];
      if (a.vtruss[u] < k) atomicMax(a.vtruss + u, k);       // (vtruss changes in SEAL only and only upwards: a stale read adds an atomic)
      if (a.vtruss[v] < k) atomicMax(a.vtruss + v, k);
    }
    if (first_thread && prev.hi > prev.lo && k >= 0 && k <= a.n) a.hist[k] += prev.hi - prev.lo;
    // what was appended since becomes the front, binned by the shorter row of its ends
    const unsigned count = (unsigned)(cur_n - prev.hi);
    for (unsigned base = (unsigned)wave * WAVE; base < count; base += (unsigned)waves * WAVE) {
      const unsigned i = base + lane;
      const bool in = i < count;
      int e = 0, sl = 0;
      if (in) {
        int s, l, ll;
        e = a.order[prev.hi + i];
        a.state[e] = KTRUSS_FRONT;
        ktruss_rows(a, e, s, sl, l, ll);
      }
      const bool is_short = in && sl <= a.short_max;
      wave_stage_push<KTRUSS_STAGE>(is_short, e, stage, fill, a.f_short, &next->n_short);
      // the longer ones: (edge, segment) items behind one add per call, as worklist.hpp's wave_append_segments -- which has no
      // capacity: an edge whose items would end past item_cap marks its slots below it empty and goes to `whole`
      const bool is_long = in && !is_short;
      if (__ballot(is_long)) {
        const int segs = is_long ? (sl + a.seg - 1) / a.seg : 0;
        const int incl = wave_inclusive_sum(segs);
        long long at = 0;
        if (lane == WAVE - 1) at = (long long)atomicAdd(&next->n_items, (unsigned long long)incl);
        at = __shfl(at, WAVE - 1, WAVE) + incl - segs;
        const bool fits = at + segs <= a.item_cap;
        for (int sgm = 0; sgm < segs && at + sgm < a.item_cap; ++sgm) a.f_items[at + sgm] = fits ? make_int2(e, sgm) : make_int2(-1, 0);
        wave_append(is_long && !fits, e, a.f_whole, &next->n_whole);
      }
    }
    wave_stage_flush(stage, fill, a.f_short, &next->n_short);
    return;
  }

  // EXPAND: the items first (a wave each), then the whole rows, then the short ones (a lane each, the wave in step)
  const int n_items = (int)min(prev.n_items, (unsigned long long)a.item_cap), n_whole = prev.n_whole, n_short = prev.n_short;
  for (int it = wave; it < n_items; it += waves) {
    const int2 item = a.f_items[it];
    if (item.x >= 0) ktruss_wave_range(a, item.x, item.y * a.seg, a.seg, k, out, &next->app, stage, fill);
  }
  for (int it = wave; it < n_whole; it += waves) ktruss_wave_range(a, a.f_whole[it], 0, 0, k, out, &next->app, stage, fill);
  for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)n_short; base += (unsigned)waves * WAVE) {
    const unsigned i = base + lane;
    const bool in = i < (unsigned)n_short;
    int e = 0, s = 0, sl = 0, l = 0, ll = 0;
    if (in) {
      e = a.f_short[i];
      ktruss_rows(a, e, s, sl, l, ll);
    }
    int longest = sl;
    longest = wave_max(longest);
    for (int j = 0; j < longest; ++j) ktruss_entry(a, j < sl, e, s + j, l, ll, k, out, &next->app, stage, fill);
  }
  wave_stage_flush(stage, fill, out, &next->app);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// what is kept per `symmetric` value beside the DAG: the adjacency with edge ids, and the arrays of m_dag entries a run works on
struct ktruss_graph_t {
  bool built = false;
  int m = 0;                                   // m_dag
  mem_t<int> adj_ro, adj_ci, adj_eid, src;
  mem_t<int> sup0, sup, state, truss, order, f_short, f_whole;
  mem_t<int2> f_items;
  int item_cap = 0;
};

struct ktruss_state_t {
  int n = 0;
  ktruss_opts_t opts;
  tc_state_t tc;                               // the DAGs, their statistics and work lists
  ktruss_graph_t gr[2];                        // [symmetric]
  mem_t<int> vtruss, hist;                     // n, n + 1
  mem_t<ktruss_control_t> ctl;
  pinned_t<ktruss_totals_t> h_totals;
  int last = -1;                               // the graph of the last run (-1: no run yet)
  long long launches = 0, waits = 0, peel_launches = 0;
  long long log_launches = -1;                 // launches of the last FUSED run, whose kinds the log holds (-1: none yet)
  bool last_fused = false;                     // the last run left a peel order
  bool timing = false;                         // mgx_ktruss_set_timing: events round the fused run's support launches and its peel
  event_t ev[3];
  double phase_ms[2] = {0.0, 0.0};             // the last timed fused run: support, peel
  long long res[5] = {0, 0, 0, 0, 0};          // stats [0] - [4] of the last run

  ktruss_state_t(int n_, long long m_, standard_context_t& ctx) : n(n_), opts(ktruss_opts_t::from_env()), tc(n_, m_, ctx) {
    const size_t N = (size_t)std::max(n, 1);
    vtruss = mem_t<int>(N, ctx);
    hist = mem_t<int>(N + 1, ctx);
    ctl = mem_t<ktruss_control_t>(1, ctx);
    h_totals = pinned_t<ktruss_totals_t>(1);
  }

  // The DAG and the adjacency of `symmetric`, unless they are there; true: this call built them.  Waits for the device (the DAG's
  // stats, the sort's host side).
  bool ensure_graph(bool symmetric, const int* ro, const int* ci, standard_context_t& ctx) {
    const int sym = symmetric ? 1 : 0;
    ktruss_graph_t& g = gr[sym];
    tc_dag_t& d = tc.dag[sym];
    if (g.built && d.built) return false;
    g = ktruss_graph_t();
    const hipStream_t st = ctx.stream();
    {
      tc_build_tmp_t tmp;
      const bool built_now = tc.ensure_dag(symmetric, ro, ci, tmp, ctx);
      if (built_now) tc.read_stats(d, true, ctx);            // (m_dag sizes everything below; the build's scratch goes behind the wait)
    }
    const int m = (int)d.h[TC_S_MDAG];
    const size_t N = (size_t)std::max(n, 1), M = (size_t)std::max(m, 1);
    g.m = m;
    g.adj_ro = mem_t<int>(N + 1, ctx);
    g.adj_ci = mem_t<int>(2 * M, ctx);
    g.adj_eid = mem_t<int>(2 * M, ctx);
    g.src = mem_t<int>(M, ctx);
    g.sup0 = mem_t<int>(M, ctx);
    g.sup = mem_t<int>(M, ctx);
    g.state = mem_t<int>(M, ctx);
    g.truss = mem_t<int>(M, ctx);
    g.order = mem_t<int>(M, ctx);
    g.f_short = mem_t<int>(M, ctx);
    g.f_whole = mem_t<int>(M, ctx);
    g.item_cap = m + 64;
    g.f_items = mem_t<int2>((size_t)g.item_cap, ctx);
    const int nn = n;
    const int* sdeg = d.sdeg.data();
    tc.scan([=] __device__(long long i) { return i < nn ? sdeg[i] : 0; }, g.adj_ro.data(), ctx);
    hipLaunchKernelGGL(k_ktruss_adj_check, dim3(1), dim3(WAVE), 0, st, (const int*)g.adj_ro.data(), n, 2ll * m, d.stat.data());
    tc.launches += 1;
    if (m > 0) {
      mem_t<int> cur(N, ctx);
      MGX_HIP(hipMemsetAsync(cur.data(), 0, N * sizeof(int), st));
      // (the check above is read before the fill is enqueued: a scan that does not end at 2 m_dag would send the fill out of its arrays)
      tc.read_stats(d, false, ctx);
      ktruss_adj_args_t a;
      a.dag_ro = d.ro.data(); a.dag_ci = d.ci.data(); a.n = n; a.adj_ro = g.adj_ro.data(); a.adj_ci = g.adj_ci.data();
      a.adj_eid = g.adj_eid.data(); a.src = g.src.data(); a.cur = cur.data();
      hipLaunchKernelGGL(k_ktruss_adj_fill, dim3(grid_for((long long)n * 8, BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(BLOCK), 0, st, a);
      MGX_CHECK_LAUNCH("mgx ktruss adjacency");
      tc.launches += 2;
      auto up = [] __device__(int x, int y) { return x < y; };
      const int passes = segmented_sort_impl<int, int>(g.adj_ci.data(), g.adj_eid.data(), 2ll * m, (const int*)g.adj_ro.data() + 1, n - 1, up, ctx);
      tc.waits += 2;                                         // (segsort.hpp's host side: the list sizes, and its scratch's release)
      tc.launches += 5 + passes + (passes & 1);              // (its clear, the classification, and every band counted as run)
    }
    g.built = true;
    return true;
  }

  // sup0 of g from the DAG d: the count kernels of tc_fused.hpp with the adds sent to the entries
  void support(ktruss_graph_t& g, tc_dag_t& d, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    MGX_HIP(hipMemsetAsync(g.sup0.data(), 0, (size_t)std::max(g.m, 1) * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(d.stat.data() + TC_S_TOTAL, 0, sizeof(u64), st));
    tc_count_args_t a;
    a.ro = d.ro.data(); a.ci = d.ci.data(); a.s_list = d.s_list.data(); a.m_list = d.m_list.data(); a.l_list = d.l_list.data();
    a.cnt = d.words.data(); a.tri = nullptr; a.stat = d.stat.data(); a.stage = tc.opts.stage; a.sup = g.sup0.data();
    hipLaunchKernelGGL(k_tc_block<true>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_tc_wave<true>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_tc_short<true>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
    MGX_CHECK_LAUNCH("mgx ktruss support");
    tc.launches += 5;
  }

  // the run's arrays as a run finds them: sup = sup0, every edge alive, truss / vtruss / hist / the control words cleared
  void begin_peel(ktruss_graph_t& g, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const size_t M = (size_t)std::max(g.m, 1), N = (size_t)std::max(n, 1);
    MGX_HIP(dtod(g.sup.data(), (const int*)g.sup0.data(), M, st));
    MGX_HIP(hipMemsetAsync(g.state.data(), 0, M * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(g.truss.data(), 0, M * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(vtruss.data(), 0, N * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(hist.data(), 0, (N + 1) * sizeof(int), st));
    ktruss_control_t::reset(ctl.data(), st);
    tc.launches += 6;
  }

  void start_run() {
    tc.launches = tc.waits = 0;
    launches = waits = peel_launches = 0;
    last = -1;
    last_fused = false;
  }
  // {largest trussness, m_dag, triangles, levels, passes, built, host waits, launches}
  std::vector<long long> finish_run(int sym, bool built_now) {
    launches = tc.launches + peel_launches;
    waits = tc.waits;
    last = sym;
    return {res[0], res[1], res[2], res[3], res[4], built_now ? 1 : 0, waits, launches};
  }

  // The fused run (ro, ci: the CSR on the device).
  std::vector<long long> run(const int* ro, const int* ci, bool symmetric, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int sym = symmetric ? 1 : 0;
    start_run();
    if (n <= 0) return {0, 0, 0, 0, 0, 0, 0, 0};
    const bool built_now = ensure_graph(symmetric, ro, ci, ctx);
    ktruss_graph_t& g = gr[sym];
    tc_dag_t& d = tc.dag[sym];
    if (timing) MGX_HIP(hipEventRecord(ev[0], st));
    support(g, d, ctx);
    if (timing) MGX_HIP(hipEventRecord(ev[1], st));
    begin_peel(g, ctx);
    ktruss_step_args_t a;
    a.dag_ci = d.ci.data(); a.src = g.src.data(); a.adj_ro = g.adj_ro.data(); a.adj_ci = g.adj_ci.data(); a.adj_eid = g.adj_eid.data();
    a.sup = g.sup.data(); a.state = g.state.data(); a.truss = g.truss.data(); a.vtruss = vtruss.data(); a.hist = hist.data();
    a.order = g.order.data(); a.f_short = g.f_short.data(); a.f_items = g.f_items.data(); a.f_whole = g.f_whole.data();
    a.stat = d.stat.data(); a.ctl = ctl.data(); a.n = n; a.m = g.m;
    a.short_max = opts.short_max; a.seg = opts.seg; a.item_cap = g.item_cap;
    const int blocks = grid_for(std::max(g.m, 1), BLOCK, std::max(ctx.num_cus, 1) * 4);
    // every edge leaves in a pass of its own and a level of its own at worst: MIN, LIST, SEAL, EXPAND, SEAL each, and then the end
    const long long most = 5ll * std::max(g.m, 1) + 8;
    peel_launches = run_launch_chain(
        [&](long long i) { hipLaunchKernelGGL(k_ktruss_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
        [&]() {
          h_totals.fetch(&ctl.data()->totals, 1, st);
          return h_totals->done != 0;
        },
        most, "mgx ktruss step", &tc.waits);
    log_launches = peel_launches;
    last_fused = true;
    if (timing) {
      float ms = 0.f;
      MGX_HIP(hipEventRecord(ev[2], st));
      MGX_HIP(hipEventSynchronize(ev[2]));
      MGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      phase_ms[0] = ms;
      MGX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
      phase_ms[1] = ms;
    }
    res[0] = h_totals->largest; res[1] = g.m; res[2] = h_totals->triangles; res[3] = h_totals->levels; res[4] = h_totals->passes;
    return finish_run(sym, built_now);
  }
};

}  // namespace mgx
