// mgx/lpa_fused.hpp -- label propagation, fused (mgx_lpa_run): every vertex takes the most frequent label among its voters'; and
// the modularity of a labelling (mgx_modularity).  One launch per step, batches of steps per host wait (launch_chain.hpp).
//
// The definition (the operator path include/gunrock/lpa/ and tests/lpa_model.py compute the same).  Original ids.
//   votes      symmetric != 0 (the caller's word that every entry has its reverse): each CSR entry (v, u), u != v, gives v one vote
//              for lab[u].  symmetric == 0: each entry (v, u), u != v, gives v one vote for lab[u] and u one vote for lab[v] -- v's
//              voters are its out-row and its in-row (the genuine CSC); no merged copy of the graph is built.  Self-loops never
//              vote, duplicates vote once each; float weights are not used (their sums would depend on the order of additions).
//   iteration  lab_0[v] = v.  c_t(v, l) = votes of v for l under lab_t, M its maximum over l.  want_t[v] = lab_t[v] if v has no
//              votes or c_t(v, lab_t[v]) == M (the current label is kept on a tie), else the smallest l with c_t(v, l) == M.
//              unstable_t = #{want_t != lab_t}.  unstable_t == 0: the run is over, converged, iterations = t.  t == max_iter: over,
//              not converged.  Otherwise lab_{t+1}[v] = want_t[v] where moves(v, t), lab_t[v] elsewhere.  SYNC: moves is always
//              true (oscillates on anything bipartite).  LAZY: moves(v, t) = color_key(v, color_salt(seed, t)) & 1.
//   active set A_0 = the vertices with votes; A_{t+1} = the unstable vertices that did not move, and whoever receives a vote from a
//              vertex that moved.  Outside A_t want_t == lab_t, so evaluating A_t alone changes no result and no unstable_t.
//   kinds      iteration t runs over A_t (LIST) when list_div > 0 and |A_t| <= n / list_div (integer division), over all vertices
//              (DENSE) otherwise: a function of |A_t|, n and MGX_LPA_LIST_DIV alone (0: always DENSE; 1: always LIST).
//
// The run is a chain of launches of k_lpa_step (launch_chain.hpp: the ring, the log, the clock, the host's batches).
//   SETUP   over all vertices: lab = own id, stamp = 0; who has a vote is A_0 (listed); the rows per body are counted
//   EVAL    over all vertices or over A_t: want[v] from lab_t, by the number of entries of v's rows (self-loops included: an upper
//           bound of its votes) --
//             up to short_max entries (at most 16): a lane each, the gathered labels in registers, every pair compared;
//             up to wave_max entries (at most 512): a wave each, an open-addressed (label, count) table of twice as many slots
//               as the row has entries, wave-private in LDS, filled with LDS atomics; it cannot overflow;
//             longer: listed for LONG.
//   LONG    (only behind an EVAL that listed rows) a workgroup per listed row: the same table for `table` labels in 2 x table
//           slots.  A row with more distinct labels than that OVERFLOWS: the workgroup then passes over the row once per hash
//           class of the label (classes = a power of two, at first 2 x entries / table rounded up, doubled while a class still
//           overflows; fmix32 is a bijection, so 2^32 classes hold one label each and the doubling ends), each pass counting the
//           labels of its class only; the winner is the best over all passes.  LDS is bounded, nothing is allocated.
//           The winner of a table: largest count, then the current label, then the smallest label -- one 64-bit maximum.
//   APPLY   over the same vertices: an unstable vertex that moves writes lab (no label is read in this launch but the thread's
//           own: the launch boundary is the synchronous rule) and marks its voters for A_{t+1}; one that is held lists itself.
//           Marks are stamps taken with atomicExch (the iteration's number + 1), so a vertex is listed once and nothing is cleared.
//           A mover's rows of more than 32 entries go out as (vertex, segment) items of 256 entries (worklist.hpp).
//   MARK    (only behind an APPLY that left items) a wave per item: the segment's voters are marked and listed the same way
//   DONE
// What holds between the workgroups of one launch (per-XCD L2s are not coherent, a CU's L1 is not refreshed):
//   (a) EVAL and LONG read lab and write want; APPLY reads want[v], lab[v] of the thread's own vertex and writes lab[v]: nothing
//       written in a launch is read in it by another thread, but the stamps.
//   (b) stamps change by device-scope atomicExch only; the plain load in front of it may be old, then the exchange decides.
//   (c) the counters of a ring word change by device-scope atomicAdd only and are read by the launches after.
// No cooperative launch, no grid-wide barrier, no inline assembly; every device loop is bounded by a size read once.
// Not built: weighted votes, Louvain and aggregation, labels renamed to a member, more than one device.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "cc_fused.hpp"
#include "color_hash.hpp"
#include "env.hpp"
#include "launch_chain.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (all four defaults are unmeasured guesses until tools/lpa_bench.py has swept them on the device)
constexpr int LPA_SHORT_MAX_DEFAULT = 16;
constexpr int LPA_WAVE_MAX_DEFAULT = 256;
constexpr int LPA_TABLE_DEFAULT = 2048;
constexpr int LPA_LIST_DIV_DEFAULT = 8;
constexpr int LPA_SHORT_CAP = 16;             // labels a lane keeps in registers
constexpr int LPA_WAVE_CAP = 512;             // labels a wave's table holds (2 x as many slots)
constexpr int LPA_TABLE_CAP = 2048;           // labels a workgroup's table holds (2 x as many slots: 32 KiB of LDS)
constexpr int LPA_TABLE_MIN = 32;
constexpr int LPA_APPLY_LANE_MAX = 32;        // a mover's rows of at most this many entries are marked by its lane
constexpr int LPA_SEG = 256;                  // entries of a mover's longer rows one wave marks
constexpr int LPA_STAGE = 2 * WAVE;           // a wave's LDS stage of listed vertices
constexpr int LPA_MAX_ITER_MAX = 1 << 20;
constexpr int LPA_EMPTY = -1;                 // a free table slot (labels are >= 0)

enum lpa_kind_t : int {
  LPA_INIT = 0, LPA_SETUP = 1, LPA_EVAL_DENSE = 2, LPA_EVAL_LIST = 3, LPA_LONG = 4, LPA_APPLY_DENSE = 5, LPA_APPLY_LIST = 6, LPA_DONE = 7,
  LPA_MARK = 8
};
enum : int { LPA_SYNC = 0, LPA_LAZY = 1 };
enum : int { LPA_T_SETUP = 0, LPA_T_EVAL = 1, LPA_T_LONG = 2, LPA_T_APPLY = 3 };

struct lpa_opts_t {
  row_cuts_t cuts = {LPA_SHORT_MAX_DEFAULT, LPA_WAVE_MAX_DEFAULT, LPA_SEG};      // (wave_max as read: the kernel's is raised to short_max)
  int table = LPA_TABLE_DEFAULT, list_div = LPA_LIST_DIV_DEFAULT;
  static lpa_opts_t from_env() {
    lpa_opts_t o;
    o.cuts.short_max = env_int("MGX_LPA_SHORT_MAX", 0, LPA_SHORT_CAP, o.cuts.short_max);
    o.cuts.wave_max = env_int("MGX_LPA_WAVE_MAX", 0, LPA_WAVE_CAP, o.cuts.wave_max);
    if (const char* e = env("MGX_LPA_TABLE")) {
      int t = LPA_TABLE_MIN;
      while (t < LPA_TABLE_CAP && t < atoi(e)) t *= 2;      // a power of two in [32, 2048]
      o.table = t;
    }
    o.list_div = env_int("MGX_LPA_LIST_DIV", 0, INT_MAX, o.list_div);
    return o;
  }
};

// what a launch leaves for the next one (cleared two launches ahead)
struct lpa_word_t {
  int kind;         // what the launch was
  int t;            // its iteration
  int dense;        // the iteration runs over all vertices
  int n_act;        // |A_t|: the list the iteration runs over (in the lists' half t & 1)
  int n_items;      // APPLY: the (vertex, segment) items of the movers' long rows
  int n_long;       // EVAL: the rows listed for LONG
  int unstable;     // EVAL, LONG: vertices with want != lab
  int changed;      // APPLY: vertices that moved
  int overflowed;   // LONG: rows whose labels did not fit the table
  int pad;
};

struct lpa_totals_t {
  long long rows, overflowed;  // rows evaluated and rows that overflowed, over the run
  long long bins[4];           // vertices per body: no entries, short, wave, long
  chain_clock_t<4> timed;      // wall clock ticks per LPA_T_* (timed runs)
  int n_list[2];               // the vertices listed in the lists' halves: [t & 1] is |A_t| once APPLY and MARK of t - 1 are over
  int iterations, converged, unstable;
  int done;                    // bit 0: the run is over
};

using lpa_control_t = chain_control_t<lpa_word_t, lpa_totals_t>;

struct lpa_trace_t { long long unstable, changed, evaluated; };

struct lpa_step_args_t {
  const int* ro;    // CSR
  const int* ci;
  const int* co;    // the genuine CSC (symmetric == 0 only)
  const int* ri;
  int* vert;        // N = max(n, 1) labels | N wanted labels | N stamps | 2 x N: A_t by iteration parity | long_cap long rows
                    // (one pointer: the kernel's scalar registers are counted)
  int2* items;      // item_cap
  lpa_trace_t* trace;
  lpa_control_t* ctl;
  int n, symmetric, mode, max_iter, trace_cap, long_cap, item_cap;
  unsigned seed;
  row_cuts_t cuts;  // (seg: LPA_SEG; the kernel uses the constant)
  int table, list_div, timing;
  __device__ __forceinline__ int* part(int k) const { return vert + (size_t)k * (size_t)max(n, 1); }
  __device__ __forceinline__ int* lab() const { return vert; }
  __device__ __forceinline__ int* want() const { return part(1); }
  __device__ __forceinline__ int* stamp() const { return part(2); }
  __device__ __forceinline__ int* list_of(int t) const { return part(3 + (t & 1)); }
  __device__ __forceinline__ int* long_rows() const { return part(5); }
};

// a vertex's voters: its out-row, and behind it its in-row when the graph is not symmetric
using lpa_row_t = row_pair_t;
__device__ __forceinline__ lpa_row_t lpa_row(const lpa_step_args_t& a, bool valid, int v) { return row_pair_of(a.ro, a.co, !a.symmetric, valid, v); }
__device__ __forceinline__ int lpa_entry(const lpa_step_args_t& a, const lpa_row_t& r, int k) {
  return k < r.olen ? a.ci[r.ob + k] : a.ri[r.ib + (k - r.olen)];
}

// the order of the candidates: count, then being the current label, then the smaller label -- larger is better; 0: no votes
__device__ __forceinline__ u64 lpa_key(int count, int label, int cur) {
  return ((u64)(unsigned)count << 33) | ((u64)(label == cur ? 1u : 0u) << 32) | (u64)(0xffffffffu - (unsigned)label);
}
__device__ __forceinline__ int lpa_winner(u64 best, int cur) { return best == 0 ? cur : (int)(0xffffffffu - (unsigned)(best & 0xffffffffull)); }

// one vote for `label` into the table of `slots` slots (a power of two); false: every slot holds another label
__device__ __forceinline__ bool lpa_insert(int* keys, int* counts, int slots, int label, bool* fresh) {
  unsigned h = color_fmix32((unsigned)label ^ 0x9E3779B9u) & (unsigned)(slots - 1);
  *fresh = false;
  for (int probe = 0; probe < slots; ++probe) {
    int old = keys[h];
    if (old == LPA_EMPTY) {
      old = atomicCAS(keys + h, LPA_EMPTY, label);
      if (old == LPA_EMPTY) *fresh = true;
    }
    if (old == LPA_EMPTY || old == label) {
      atomicAdd(counts + h, 1);
      return true;
    }
    h = (h + 1) & (unsigned)(slots - 1);
  }
  return false;
}

// a lane's row of at most LPA_SHORT_CAP entries: the labels in registers, every pair compared
__device__ __forceinline__ int lpa_short_want(const lpa_step_args_t& a, const lpa_row_t& r, int v, int cur) {
  int l[LPA_SHORT_CAP];
  const int len = r.len();
#pragma unroll
  for (int k = 0; k < LPA_SHORT_CAP; ++k) {
    const bool has = k < len;
    const int u = has ? lpa_entry(a, r, k) : v;
    l[k] = u != v ? a.lab()[u] : LPA_EMPTY;
  }
  u64 best = 0;
#pragma unroll
  for (int i = 0; i < LPA_SHORT_CAP; ++i) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < LPA_SHORT_CAP; ++j) c += l[j] == l[i] ? 1 : 0;
    if (l[i] != LPA_EMPTY) best = max(best, lpa_key(c, l[i], cur));
  }
  return lpa_winner(best, cur);
}

// a wave's row of at most LPA_WAVE_CAP entries (all lanes call with the same row): its table has room for every entry
__device__ __forceinline__ int lpa_wave_want(const lpa_step_args_t& a, const lpa_row_t& r, int v, int cur, int* keys, int* counts) {
  const int lane = lane_id();
  const int len = r.len();
  int slots = 2 * WAVE;
  while (slots < 2 * len) slots *= 2;                        // (len <= LPA_WAVE_CAP: at most 2 x LPA_WAVE_CAP)
  for (int s = lane; s < slots; s += WAVE) { keys[s] = LPA_EMPTY; counts[s] = 0; }
  wave_lds_fence();
  for (int k = lane; k < len; k += WAVE) {
    const int u = lpa_entry(a, r, k);
    bool fresh;
    if (u != v) lpa_insert(keys, counts, slots, a.lab()[u], &fresh);
  }
  wave_lds_fence();
  u64 best = 0;
  for (int s = lane; s < slots; s += WAVE)
    if (keys[s] != LPA_EMPTY) best = max(best, lpa_key(counts[s], keys[s], cur));
  wave_lds_fence();                                          // (the table is cleared again by the next row)
  return lpa_winner(wave_max(best), cur);
}

// what the kernel keeps in LDS: the waves' tables or the workgroup's (never both in one launch), the waves' list stages
struct lpa_lds_t {
  int keys[2 * LPA_TABLE_CAP];                               // = WAVES_PER_BLOCK x 2 x LPA_WAVE_CAP
  int counts[2 * LPA_TABLE_CAP];
  int stage[WAVES_PER_BLOCK][LPA_STAGE];
  u64 best[WAVES_PER_BLOCK];
  int fresh, failed;
};
static_assert(WAVES_PER_BLOCK * 2 * LPA_WAVE_CAP == 2 * LPA_TABLE_CAP, "the waves' tables and the workgroup's share their LDS");

// a workgroup's row (all threads call with the same row): -> want; *over: the row's labels did not fit the table
__device__ __forceinline__ int lpa_block_want(const lpa_step_args_t& a, const lpa_row_t& r, int v, int cur, lpa_lds_t& s, bool* over) {
  const int len = r.len();
  const int slots = 2 * a.table;
  const int wave = threadIdx.x / WAVE;
  u64 classes = 1, best = 0;
  *over = false;
  for (int attempt = 0; attempt < 34; ++attempt) {           // (the classes at most double up to 2^32)
    best = 0;
    bool failed = false;
    for (u64 p = 0; p < classes && !failed; ++p) {
      for (int i = threadIdx.x; i < slots; i += BLOCK) { s.keys[i] = LPA_EMPTY; s.counts[i] = 0; }
      if (threadIdx.x == 0) { s.fresh = 0; s.failed = 0; }
      __syncthreads();
      for (int k = threadIdx.x; k < len; k += BLOCK) {
        const int u = lpa_entry(a, r, k);
        if (u == v) continue;
        const int label = a.lab()[u];
        if (((u64)color_fmix32((unsigned)label) & (classes - 1)) != p) continue;
        bool fresh;
        const bool ok = lpa_insert(s.keys, s.counts, slots, label, &fresh);
        if (!ok || (fresh && atomicAdd(&s.fresh, 1) >= a.table)) { s.failed = 1; break; }
      }
      __syncthreads();
      failed = s.failed != 0;                                // (the same for every thread: read behind the barrier)
      u64 mine = 0;
      if (!failed)
        for (int i = threadIdx.x; i < slots; i += BLOCK)
          if (s.keys[i] != LPA_EMPTY) mine = max(mine, lpa_key(s.counts[i], s.keys[i], cur));
      mine = wave_max(mine);
      if (lane_id() == 0) s.best[wave] = mine;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < WAVES_PER_BLOCK; ++w) best = max(best, s.best[w]);
      __syncthreads();                                       // (the table and the flags are written again by the next pass)
    }
    if (!failed) break;
    *over = true;
    if (attempt == 0) {
      classes = 2;
      while (classes * (u64)a.table < 2 * (u64)len) classes *= 2;
    } else {
      classes *= 2;
    }
  }
  return lpa_winner(best, cur);
}

// a wave's share of the list being made: vertices wait in its stage and go out behind one returning add (worklist.hpp)
struct lpa_list_t {
  int* stage;
  int* out;
  int* counter;
  int fill = 0;
  __device__ __forceinline__ void push(bool take, int v) { wave_stage_push<LPA_STAGE>(take, v, stage, fill, out, counter); }
  __device__ __forceinline__ void flush() { wave_stage_flush(stage, fill, out, counter); }
};

__device__ __forceinline__ bool lpa_is_dense(int n_act, int n, int list_div) { return !(list_div > 0 && n_act <= n / list_div); }
__device__ __forceinline__ int lpa_clock_of(int kind) {
  if (kind == LPA_SETUP) return LPA_T_SETUP;
  if (kind == LPA_EVAL_DENSE || kind == LPA_EVAL_LIST) return LPA_T_EVAL;
  return kind == LPA_LONG ? LPA_T_LONG : LPA_T_APPLY;          // (APPLY and MARK)
}

// launch: the launch's number in the run
__global__ __launch_bounds__(BLOCK) void k_lpa_step(lpa_step_args_t a, unsigned launch) {
  const lpa_word_t prev = a.ctl->left_by_prev(launch);
  lpa_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left
  const bool was_eval = prev.kind == LPA_EVAL_DENSE || prev.kind == LPA_EVAL_LIST;
  const bool was_apply = prev.kind == LPA_APPLY_DENSE || prev.kind == LPA_APPLY_LIST;
  const bool evaluated = (was_eval && prev.n_long == 0) || prev.kind == LPA_LONG;      // iteration prev.t knows its unstable
  int kind, t = prev.t, n_act = prev.n_act, dense = prev.dense;
  if (prev.kind == LPA_INIT) {
    kind = LPA_SETUP;
  } else if (was_apply && prev.n_items > 0) {
    kind = LPA_MARK;
  } else if (prev.kind == LPA_SETUP || was_apply || prev.kind == LPA_MARK) {
    t = prev.kind == LPA_SETUP ? 0 : prev.t + 1;
    n_act = min(a.ctl->totals.n_list[t & 1], a.n);            // (what SETUP, or APPLY and MARK of the iteration before, listed)
    dense = lpa_is_dense(n_act, a.n, a.list_div) ? 1 : 0;
    kind = dense ? LPA_EVAL_DENSE : LPA_EVAL_LIST;
  } else if (was_eval && prev.n_long > 0) {
    kind = LPA_LONG;
  } else if (evaluated) {
    kind = (prev.unstable == 0 || prev.t >= a.max_iter) ? LPA_DONE : (dense ? LPA_APPLY_DENSE : LPA_APPLY_LIST);
  } else {
    kind = LPA_DONE;
  }
  if (first_thread) {
    const lpa_word_t* const pw = a.ctl->left_by_prev_at(launch);   // (read again here: the scalar registers are counted)
    next->kind = kind;
    next->t = t;
    next->dense = dense;
    next->n_act = n_act;
    lpa_totals_t& tot = a.ctl->totals;
    a.ctl->log_kind(launch, kind);
    if (kind == LPA_LONG) atomicAdd(&next->unstable, pw->unstable);      // (the iteration's count goes on through LONG)
    if (kind == LPA_EVAL_DENSE || kind == LPA_EVAL_LIST) tot.n_list[(t + 1) & 1] = 0;      // (A_{t-1}'s half: APPLY and MARK of t fill it)
    if (pw->kind == LPA_LONG) tot.overflowed += pw->overflowed;
    if (evaluated) {
      const long long rows = pw->dense ? a.n : pw->n_act;
      tot.rows += rows;
      tot.iterations = pw->t;
      tot.unstable = pw->unstable;
      if (pw->t < a.trace_cap) {
        a.trace[pw->t].unstable = pw->unstable;
        a.trace[pw->t].changed = 0;
        a.trace[pw->t].evaluated = rows;
      }
      if (kind == LPA_DONE) { tot.converged = pw->unstable == 0 ? 1 : 0; tot.done |= 1; }
    }
    if (was_apply && pw->t < a.trace_cap) a.trace[pw->t].changed = pw->changed;
    tot.timed.tick(a.timing, pw->kind, LPA_DONE, lpa_clock_of(pw->kind));
  }
  if (kind == LPA_DONE) return;

  const int lane = lane_id();
  const int wave_in_block = threadIdx.x / WAVE;
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  __shared__ lpa_lds_t lds;

  if (kind == LPA_LONG) {                                    // a workgroup per listed row
    const int n_long = min(a.ctl->left_by_prev_at(launch)->n_long, a.long_cap);
    int unstable = 0, overflowed = 0;
    for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
      const int v = a.long_rows()[i];
      const lpa_row_t r = lpa_row(a, true, v);
      const int cur = a.lab()[v];
      bool over;
      const int w = lpa_block_want(a, r, v, cur, lds, &over);
      if (threadIdx.x == 0) a.want()[v] = w;
      unstable += w != cur ? 1 : 0;
      overflowed += over ? 1 : 0;
    }
    if (threadIdx.x == 0 && unstable) atomicAdd(&next->unstable, unstable);
    if (threadIdx.x == 0 && overflowed) atomicAdd(&next->overflowed, overflowed);
    return;
  }

  lpa_list_t list;
  list.stage = lds.stage[wave_in_block];

  if (kind == LPA_SETUP) {
    list.out = a.list_of(0);
    list.counter = &a.ctl->totals.n_list[0];
    row_bins_t bins;
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)a.n; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < (unsigned)a.n;
      const int v = (int)(base + lane);
      const lpa_row_t r = lpa_row(a, in, v);
      const int len = r.len();
      bool votes = false;
      for (int k = 0; k < len && !votes; ++k) votes = lpa_entry(a, r, k) != v;
      if (in) { a.lab()[v] = v; a.want()[v] = v; a.stamp()[v] = 0; }
      bins.count(in ? a.cuts.body_of(len) : -1);
      list.push(in && votes, v);
    }
    list.flush();
    bins.add_to(a.ctl->totals.bins);
    return;
  }

  if (kind == LPA_MARK) {                                    // a wave per (vertex, segment) item of the movers' long rows
    list.out = a.list_of(t + 1);
    list.counter = &a.ctl->totals.n_list[(t + 1) & 1];
    const int n_items = min(a.ctl->left_by_prev_at(launch)->n_items, a.item_cap);
    const int tag = t + 1;
    for (int it = wave; it < n_items; it += waves) {
      const int2 item = a.items[it];
      const int v = item.x;
      const lpa_row_t r = lpa_row(a, true, v);
      const int k0 = item.y * LPA_SEG;
      const int k1 = min(r.len(), k0 + LPA_SEG);
      for (int k = k0; k < k1; k += WAVE) {
        const int u = k + lane < k1 ? lpa_entry(a, r, k + lane) : v;
        bool take = u != v && a.stamp()[u] != tag;
        if (take) take = atomicExch(a.stamp() + u, tag) != tag;
        list.push(take, u);
      }
    }
    list.flush();
    return;
  }

  const unsigned count = dense ? (unsigned)a.n : (unsigned)min(n_act, a.n);
  const int* const act = a.list_of(t);

  if (kind == LPA_EVAL_DENSE || kind == LPA_EVAL_LIST) {
    list.out = a.long_rows();
    list.counter = &next->n_long;
    int* const keys = lds.keys + wave_in_block * 2 * LPA_WAVE_CAP;
    int* const counts = lds.counts + wave_in_block * 2 * LPA_WAVE_CAP;
    int unstable = 0;
    for (unsigned base = (unsigned)wave * WAVE; base < count; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < count;
      const int v = in ? (dense ? (int)(base + lane) : act[base + lane]) : 0;
      const lpa_row_t r = lpa_row(a, in, v);
      const int body = in ? a.cuts.body_of(r.len()) : ROW_NONE;
      const int cur = in ? a.lab()[v] : 0;
      int w = cur;
      if (body == ROW_LANE) w = lpa_short_want(a, r, v, cur);
      for_each_wave_row(body == ROW_WAVE, [&](int src) {
        const int ww = lpa_wave_want(a, r.of_lane(src), __shfl(v, src, WAVE), __shfl(cur, src, WAVE), keys, counts);
        if (lane == src) w = ww;
      });
      list.push(body == ROW_LONG, v);
      if (in && body != ROW_LONG) {
        a.want()[v] = w;
        unstable += w != cur ? 1 : 0;
      }
    }
    list.flush();
    unstable = wave_sum(unstable);
    if (lane == 0 && unstable) atomicAdd(&next->unstable, unstable);
    return;
  }

  {                                                          // APPLY
    list.out = a.list_of(t + 1);
    list.counter = &a.ctl->totals.n_list[(t + 1) & 1];
    const int tag = t + 1;
    const unsigned salt = color_salt(a.seed, t);
    int changed = 0;
    for (unsigned base = (unsigned)wave * WAVE; base < count; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < count;
      const int v = in ? (dense ? (int)(base + lane) : act[base + lane]) : 0;
      const int w = in ? a.want()[v] : 0;
      const bool unst = in && w != a.lab()[v];
      const bool moves = unst && (a.mode == LPA_SYNC || (color_key(v, salt) & 1u));
      if (moves) a.lab()[v] = w;
      changed += moves ? 1 : 0;
      bool held = unst && !moves;
      if (held) held = atomicExch(a.stamp() + v, tag) != tag;
      list.push(held, v);
      // the movers' voters: a lane walks its short rows, the wave in step; the longer ones go out as items
      const lpa_row_t r = lpa_row(a, moves, v);
      const int len = r.len();
      const int mine = len <= LPA_APPLY_LANE_MAX ? len : 0;
      const int longest = wave_max(mine);
      for (int k = 0; k < longest; ++k) {
        const int u = k < mine ? lpa_entry(a, r, k) : v;
        bool take = u != v && a.stamp()[u] != tag;
        if (take) take = atomicExch(a.stamp() + u, tag) != tag;
        list.push(take, u);
      }
      if (__ballot(len > LPA_APPLY_LANE_MAX)) wave_append_segments_outlined(len > LPA_APPLY_LANE_MAX, v, len, LPA_SEG, a.items, &next->n_items);      // (the longer ones: MARK's)
    }
    list.flush();
    changed = wave_sum(changed);
    if (lane == 0 && changed) atomicAdd(&next->changed, changed);
  }
}

// {communities, largest, its label} of labels in [0, n) that need not name a member of their community (cc_label_stats_t counts
// the vertices that carry their own id, which is right for labels that are the smallest id of their set only): the sizes by the
// connected components' kernel, then every label that has a size is a community
__global__ __launch_bounds__(BLOCK) void k_lpa_largest(const int* __restrict__ sizes, int n, u64* __restrict__ out) {
  u64 best = 0, some = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int c = (int)i;
    if (sizes[c] > 0) {
      ++some;
      best = max(best, ((u64)(u32)sizes[c] << 32) | (u32)~c);
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    best = max(best, (u64)__shfl_xor((long long)best, d, WAVE));
    some += (u64)__shfl_xor((long long)some, d, WAVE);
  }
  __shared__ u64 s_best[WAVES_PER_BLOCK], s_some[WAVES_PER_BLOCK];      // (one add and one max per workgroup, as k_cc_largest)
  if (lane_id() == 0) {
    s_best[threadIdx.x / WAVE] = best;
    s_some[threadIdx.x / WAVE] = some;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) {
      best = max(best, s_best[w]);
      some += s_some[w];
    }
    if (some) atomicAdd(out + 1, some);
    if (best) atomicMax(out, best);
  }
}
struct lpa_label_stats_t {
  mem_t<int> sizes, hot;
  mem_t<u64> out;
  pinned_t<u64> h_pinned;
  lpa_label_stats_t(int n, context_t& ctx) {
    sizes = mem_t<int>((size_t)std::max(n, 1), ctx);
    hot = mem_t<int>(1, ctx);
    out = mem_t<u64>(2, ctx);
    h_pinned = pinned_t<u64>(2);
  }
  // one host wait
  std::vector<long long> run(const int* label, int n, standard_context_t& ctx) {
    if (n <= 0) return {0, 0, 0};
    const hipStream_t st = ctx.stream();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    MGX_HIP(hipMemsetAsync(out.data(), 0, 2 * sizeof(u64), st));
    MGX_HIP(hipMemsetAsync(sizes.data(), 0, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL(k_cc_sample, dim3(1), dim3(BLOCK), 0, st, label, n, CC_SEED_DEFAULT, hot.data());
    hipLaunchKernelGGL(k_cc_sizes, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, label, n, (const int*)hot.data(), sizes.data());
    hipLaunchKernelGGL(k_lpa_largest, dim3(grid_for(n, BLOCK, std::max(max_blocks / 8, 1))), dim3(BLOCK), 0, st, (const int*)sizes.data(), n, out.data());
    MGX_CHECK_LAUNCH("mgx lpa label stats");
    h_pinned.fetch(out.data(), 2, st);
    long long s[3];
    cc_unpack_stats(h_pinned.data(), s);
    return {s[0], s[1], s[2]};
  }
};

// The device state of a graph's fused label propagation, and the run (host side).  Everything a run needs is allocated at the
// first run (the trace grows only when a later run asks for more iterations): a second run allocates nothing.
struct lpa_fused_state_t {
  int n = 0;
  long long m = 0;
  lpa_opts_t opts;
  mem_t<int> vert;                             // the labels first (lpa_step_args_t::vert)
  mem_t<int2> items;
  int long_cap = 0, item_cap = 0;
  mem_t<lpa_trace_t> trace;
  int trace_cap = 0;
  mem_t<lpa_control_t> ctl;
  pinned_t<lpa_totals_t> h_totals;
  lpa_label_stats_t label_stats;
  long long launches = -1;                     // of the last run, the idle ones behind its end included (-1: no run yet)
  long long iterations = 0;                    // of the last run
  long long bins[4] = {0, 0, 0, 0}, overflowed = 0;
  bool timing = false;
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the last timed run: setup, evaluate, long rows, apply

  lpa_fused_state_t(int n_, long long m_, context_t& ctx) : n(n_), m(m_), opts(lpa_opts_t::from_env()), label_stats(n_, ctx) {
    const size_t N = (size_t)std::max(n, 1);
    // rows of more than wave_max entries: out- and in-entries together are 2 m at most
    long_cap = (int)std::min<long long>((long long)N, 2 * m / (std::max(opts.cuts.wave_max, opts.cuts.short_max) + 1) + 1);
    vert = mem_t<int>(5 * N + (size_t)long_cap, ctx);
    // a mover's rows of more than LPA_APPLY_LANE_MAX entries, once an iteration: an item per LPA_SEG entries and one per row
    item_cap = (int)(std::min<long long>((long long)N, 2 * m / (LPA_APPLY_LANE_MAX + 1) + 1) + 2 * m / LPA_SEG + 1);
    items = mem_t<int2>((size_t)item_cap, ctx);
    ctl = mem_t<lpa_control_t>(1, ctx);
    h_totals = pinned_t<lpa_totals_t>(1);
  }

  // Propagate (ro, ci: the CSR on the device; co, ri: its genuine CSC, read when symmetric == 0 only).  Returns {communities,
  // largest, its label, iterations, converged, unstable of the last iteration, rows evaluated, overflowed rows, host waits,
  // launches}.
  std::vector<long long> run(const int* ro, const int* ci, const int* co, const int* ri, int symmetric, int mode, unsigned seed, int max_iter,
                             standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    launches = -1;                                           // (a run that throws leaves no launches to ask about)
    if (n <= 0) {
      launches = 0;
      iterations = 0;
      return {0, 0, 0, 0, 1, 0, 0, 0, 0, 0};
    }
    if (trace_cap < max_iter + 1) {
      trace = mem_t<lpa_trace_t>((size_t)max_iter + 1, ctx);
      trace_cap = max_iter + 1;
    }
    lpa_control_t::reset(ctl.data(), st);
    lpa_step_args_t a;
    a.ro = ro; a.ci = ci; a.co = co; a.ri = ri;
    a.vert = vert.data(); a.items = items.data();
    a.trace = trace.data(); a.ctl = ctl.data();
    a.n = n; a.symmetric = symmetric ? 1 : 0; a.mode = mode; a.max_iter = max_iter; a.trace_cap = trace_cap; a.long_cap = long_cap; a.item_cap = item_cap;
    a.seed = seed;
    a.cuts = opts.cuts;
    a.cuts.wave_max = std::max(opts.cuts.wave_max, opts.cuts.short_max);
    a.table = opts.table; a.list_div = opts.list_div;
    a.timing = timing ? 1 : 0;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 4);
    long long waits = 0;
    // SETUP, and at most an EVAL, a LONG, an APPLY and a MARK per iteration: a chain that is longer has not ended
    const long long most = 4ll * ((long long)max_iter + 2) + CHAIN_BATCH_MAX;
    const long long enqueued = run_launch_chain(
        [&](long long i) { hipLaunchKernelGGL(k_lpa_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
        [&]() {
          h_totals.fetch(&ctl.data()->totals, 1, st);
          return (h_totals->done & 1) != 0;
        },
        most, "mgx lpa step", &waits);
    if (timing)
      for (int i = 0; i < 4; ++i) phase_ms[i] = chain_ticks_ms(h_totals->timed.clock[i]);
    const lpa_totals_t tot = *h_totals.data();
    const std::vector<long long> ls = label_stats.run(vert.data(), n, ctx);
    ++waits;
    for (int b = 0; b < 4; ++b) bins[b] = tot.bins[b];
    overflowed = tot.overflowed;
    iterations = tot.iterations;
    launches = enqueued;
    return {ls[0], ls[1], ls[2], tot.iterations, tot.converged, tot.unstable, tot.rows, tot.overflowed, waits, launches};
  }
};

// ---- modularity of a labelling ----------------------------------------------------------------------------------------------
// S_in = votes whose two ends carry equal labels, tot_c = the votes of the vertices labelled c, S_sq = the sum of tot_c^2,
// W = all votes: exact in 64 bits (W <= 2 m < 2^32).  acc: [0] S_in, [1] S_sq, [2] W, [3] labels outside [0, n).
enum : int { MOD_S_IN = 0, MOD_S_SQ = 1, MOD_W = 2, MOD_BAD = 3 };

// over the vertices, a wave over 64 consecutive ones: a lane counts its rows of at most 32 entries, the wave the longer ones
__global__ __launch_bounds__(BLOCK) void k_mod_votes(const int* __restrict__ ro, const int* __restrict__ ci, const int* __restrict__ co,
                                                     const int* __restrict__ ri, const int* __restrict__ lab, int n, int symmetric,
                                                     u64* __restrict__ tot, u64* __restrict__ acc) {
  const int lane = lane_id();
  const unsigned wave = (blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE;
  const unsigned waves = gridDim.x * (unsigned)BLOCK / WAVE;
  u64 s_in = 0, w = 0, bad = 0;
  for (unsigned base = wave * WAVE; base < (unsigned)n; base += waves * WAVE) {
    const bool in = base + lane < (unsigned)n;
    const int v = (int)(base + lane);
    const int l = in ? lab[v] : 0;
    const bool ok = in && l >= 0 && l < n;
    bad += (in && !ok) ? 1 : 0;
    u64 equal = 0, votes = 0;
    for (int side = 0; side < (symmetric ? 1 : 2); ++side) {
      const int* const off = side == 0 ? ro : co;
      const int* const adj = side == 0 ? ci : ri;
      const int beg = in ? off[v] : 0;
      const int len = in ? off[v + 1] - beg : 0;
      if (len <= 32)
        for (int k = 0; k < len; ++k) {
          const int u = adj[beg + k];
          votes += u != v ? 1 : 0;
          equal += (side == 0 && u != v && lab[u] == l) ? 1 : 0;
        }
      for_each_wave_row(len > 32, [&](int src) {
        const int vv = __shfl(v, src, WAVE), b = __shfl(beg, src, WAVE), e = b + __shfl(len, src, WAVE), ll = __shfl(l, src, WAVE);
        u64 c = 0, q = 0;
        for (int k = b + lane; k < e; k += WAVE) {
          const int u = adj[k];
          c += u != vv ? 1 : 0;
          q += (side == 0 && u != vv && lab[u] == ll) ? 1 : 0;
        }
        c = wave_sum(c);
        q = wave_sum(q);
        if (lane == src) { votes += c; equal += q; }
      });
    }
    if (ok && votes) atomicAdd(tot + l, votes);
    w += votes;
    s_in += symmetric ? equal : 2 * equal;                   // (not symmetric: an entry is a vote at both of its ends)
  }
  s_in = wave_sum(s_in);
  w = wave_sum(w);
  bad = wave_sum(bad);
  if (lane == 0) {
    if (s_in) atomicAdd(acc + MOD_S_IN, s_in);
    if (w) atomicAdd(acc + MOD_W, w);
    if (bad) atomicAdd(acc + MOD_BAD, bad);
  }
}
__global__ __launch_bounds__(BLOCK) void k_mod_squares(const u64* __restrict__ tot, int n, u64* __restrict__ acc) {
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  u64 s = 0;
  for (unsigned c = gtid; c < (unsigned)n; c += gthreads) s += tot[c] * tot[c];
  s = wave_sum(s);
  if (lane_id() == 0 && s) atomicAdd(acc + MOD_S_SQ, s);
}

struct modularity_state_t {
  int n = 0;
  mem_t<u64> tot, acc;
  pinned_t<u64> h_acc;
  modularity_state_t(int n_, context_t& ctx) : n(n_) {
    tot = mem_t<u64>((size_t)std::max(n, 1), ctx);
    acc = mem_t<u64>(4, ctx);
    h_acc = pinned_t<u64>(4);
  }
  // out[3] = {S_in, S_sq, W}; one host wait.  A label outside [0, n): MGX_E_INVALID.
  void run(const int* ro, const int* ci, const int* co, const int* ri, const int* d_labels, int symmetric, u64* out, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    out[0] = out[1] = out[2] = 0;
    if (n <= 0) return;
    MGX_HIP(hipMemsetAsync(tot.data(), 0, (size_t)n * sizeof(u64), st));
    MGX_HIP(hipMemsetAsync(acc.data(), 0, 4 * sizeof(u64), st));
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8);
    hipLaunchKernelGGL(k_mod_votes, dim3(blocks), dim3(BLOCK), 0, st, ro, ci, co, ri, d_labels, n, symmetric ? 1 : 0, tot.data(), acc.data());
    hipLaunchKernelGGL(k_mod_squares, dim3(blocks), dim3(BLOCK), 0, st, (const u64*)tot.data(), n, acc.data());
    MGX_CHECK_LAUNCH("mgx modularity");
    h_acc.fetch(acc.data(), 4, st);
    if (h_acc.data()[MOD_BAD]) throw mgx_error(MGX_E_INVALID, "mgx_modularity: a label is outside [0, n)");
    out[0] = h_acc.data()[MOD_S_IN]; out[1] = h_acc.data()[MOD_S_SQ]; out[2] = h_acc.data()[MOD_W];
  }
};

}  // namespace mgx
