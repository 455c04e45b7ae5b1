// mgx/louvain_fused.hpp -- Louvain community detection, fused (mgx_louvain_run): levels of local moves that raise the modularity,
// each followed by a contraction of the communities into the next level's graph (louvain_aggregate.hpp).
//
// The definition (tests/louvain_model.py computes the same, bit for bit).  All arithmetic is integer.
//   level 0    symmetric != 0: every CSR entry (v, u), u != v, is weight 1 from v to u.  symmetric == 0: every entry gives weight 1 to
//              both ends (v's row is its out-row and its in-row, the genuine CSC).  Self-loops are dropped, duplicates add.
//              k_v = the sum of v's weights, W = the sum of all k_v.  At most 2^30 entries, so W <= 2^31.
//   iteration  lab_0[v] = v.  Sigma_c = the k of the vertices labelled c; k_{v,c} = the weight from v to vertices labelled c, v's
//              own self entry excluded.  s(c) = k_{v,c} W - (Sigma_c - [c == lab[v]] k_v) k_v over the candidates lab[v] and the
//              labels of v's neighbours; key(c) = color_key(c, seed).  best(v): the greatest score, on equal scores the current
//              label, else the smaller key.  v moves iff best(v) != lab[v] and key(best) < key(lab[v]) (t even) or > (t odd).
//   64 bits    k_{v,c}, Sigma_c, k_v <= W <= 2^31: k_{v,c} W <= 2^62 and Sigma_c k_v <= 2^62, a score lies in (-2^62, 2^62];
//              S_in <= W and S_sq <= W^2: Qnum = S_in W - S_sq lies in [-2^62, 2^62], and a difference of two in [-2^63, 2^63)
//              only when both ends are met, which needs S_in = W with S_sq = 0: impossible (S_sq >= S_in^2 / communities > 0).
//   accept     Qnum(lab) = S_in W - S_sq.  The moved labelling is accepted iff a vertex moved and Qnum(new) - Qnum(old) > thr,
//              thr = min((int64) ceil(tol * (double) W * (double) W), 2^62); else the labels stay.  A level ends after two
//              consecutive rejected iterations or at max_iter.
//   levels     a level that accepted nothing ends the run, as does level == max_levels; else the level is contracted.
//
// A level is a chain of launches of k_louvain_step (launch_chain.hpp: the ring, the log, the clock, the host's batches; the control
// is reset and the log read back per level).  A launch derives its kind -- every thread the same -- from the word the launch
// before left and from sums no thread of the launch changes.
//   SETUP      over all vertices: lab = own id, k_v, Sigma = k, W, the identity's S_in and S_sq; the rows per body; a long row gets
//              its table in device memory (a returning add on one cursor) and its (vertex, segment) items, once per level
//   EVAL       over all vertices, by the entries of the row: up to short_max (at most 16) a lane, labels and weights in registers,
//              every pair compared; up to wave_max (at most 512) a wave with an open-addressed (label, weight) table in LDS, filled
//              with LDS atomics, twice as many slots as entries; longer rows wait for LONG.  Sigma is copied to the other buffer.
//   LONG_FILL  (only when the level has long rows) a wave per (vertex, segment) item: seg entries of the row go into the ROW'S table
//              in device memory (2 x entries slots, a CAS on the label, an integer add on the weight): exact whatever the order
//   LONG_SCAN  a wave per item again: 2 x seg slots of the table are scored, the best goes to the item's slot, the slots are
//              emptied for the next iteration
//   APPLY      over all vertices: a long row's best is the best of its items' slots; movers write the OTHER label buffer and move
//              their k between the other buffer's Sigma by integer atomics
//   QNUM       S_in of the other labels by a row sweep (long rows by their items), S_sq from the other Sigma, reduced in LDS, one
//              atomic of each per workgroup.  The head of the next launch accepts or rejects: it picks the label buffer.
//   DONE
// Long rows: the (vertex, segment) items spread a hub's entries over the chip in both passes, every entry is read once per
// iteration, and a table has room for every entry, so there is no overflow and no retry: the items are a function of the rows'
// lengths alone (ceil(entries / seg) per long row and iteration).  LPA's one workgroup per row and hash class re-reads a hub once
// per class.  The price: 16 bytes of device memory per entry of a long row, and adds that meet on one word when a
// hub's neighbours share a label.
// What holds between the workgroups of a launch: labels and Sigma are read from one buffer and written to the other; the tables
// change by device-scope atomics only (the load in front of the CAS is an atomic load); counters change by device-scope atomicAdd.
// No cooperative launch, no grid-wide barrier, no inline assembly; every device loop is bounded by a size read once.
// Not built: float weights, a resolution parameter, Leiden refinement, more than one device, an active-vertex list.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "cc_fused.hpp"
#include "color_hash.hpp"
#include "env.hpp"
#include "launch_chain.hpp"
#include "louvain_aggregate.hpp"
#include "lpa_fused.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (swept at RMAT-20 only, DESIGN 3.18: WAVE_MAX 512 was 10 % faster there, SEG 256 the best of 64 / 256 / 1024; guesses elsewhere)
constexpr int LV_SHORT_MAX_DEFAULT = 16;
constexpr int LV_WAVE_MAX_DEFAULT = 256;
constexpr int LV_SEG_DEFAULT = 256;
constexpr int LV_SHORT_CAP = 16;              // entries a lane keeps in registers
constexpr int LV_WAVE_CAP = 512;              // entries a wave's table holds (2 x as many slots)
constexpr int LV_SEG_MIN = 64;
constexpr int LV_SEG_CAP = 1024;
constexpr int LV_QNUM_LANE_MAX = 32;          // QNUM and SETUP: rows of at most this many entries are summed by their lane
constexpr int LV_MAX_ITER_MAX = 1 << 20;
constexpr int LV_MAX_LEVELS_MAX = 64;
constexpr int LV_EMPTY = -1;                  // a free table slot (labels are >= 0)
constexpr long long LV_THR_MAX = 1ll << 62;

enum lv_kind_t : int { LV_INIT = 0, LV_SETUP = 1, LV_EVAL = 2, LV_LONG_FILL = 3, LV_LONG_SCAN = 4, LV_APPLY = 5, LV_QNUM = 6, LV_DONE = 7 };
enum : int { LV_T_SETUP = 0, LV_T_EVAL = 1, LV_T_LONG = 2, LV_T_APPLY = 3, LV_T_QNUM = 4, LV_T_AGG = 5 };

struct lv_opts_t {
  row_cuts_t cuts = {LV_SHORT_MAX_DEFAULT, LV_WAVE_MAX_DEFAULT, LV_SEG_DEFAULT};
  static lv_opts_t from_env() {
    lv_opts_t o;
    o.cuts.short_max = env_int("MGX_LOUVAIN_SHORT_MAX", 0, LV_SHORT_CAP, o.cuts.short_max);
    o.cuts.wave_max = env_int("MGX_LOUVAIN_WAVE_MAX", 0, LV_WAVE_CAP, o.cuts.wave_max);
    if (const char* e = env("MGX_LOUVAIN_SEG")) {
      int s = LV_SEG_MIN;
      while (s < LV_SEG_CAP && s < atoi(e)) s *= 2;          // a power of two in [64, 1024]
      o.cuts.seg = s;
    }
    o.cuts.wave_max = std::max(o.cuts.wave_max, o.cuts.short_max);
    return o;
  }
};

// what a launch leaves for the next one (cleared two launches ahead)
struct lv_word_t {
  int kind;         // what the launch was
  int t;            // its iteration
  int cur;          // the label buffer that holds the level's labels
  int rejects;      // consecutive rejected iterations
  int accepted;     // accepted iterations
  int moved;        // APPLY (carried through QNUM): vertices that moved
  long long q;      // Qnum of the labels in buffer cur
  u64 s_in, s_sq;   // SETUP: of the identity; QNUM: of the other buffer's labels
};

struct lv_totals_t {
  u64 w;                       // SETUP: the sum of all k
  long long q;                 // of the level's labels at its end
  u64 s_in, s_sq;
  long long bins[4];           // vertices per body: no entries, short, wave, long
  chain_clock_t<5> timed;      // wall clock ticks per LV_T_* (timed runs)
  unsigned long long cursor;   // SETUP: the table slots handed out
  int n_items;                 // SETUP: the long rows' (vertex, segment) items
  int cur, iterations, accepted;
  int done;                    // bit 0: the level is over
  int pad;
};

// (the log holds a level's first CHAIN_LOG_CAP launches: a longer level's list of kinds ends there, without its DONE)
using lv_control_t = chain_control_t<lv_word_t, lv_totals_t>;

struct lv_trace_t { long long moved, accepted, q; };

struct lv_args_t {
  lv_graph_t g;
  int* vert;                   // N-sized parts: 0, 1 the label buffers | 2, 3 Sigma of each (uint32) | 4 k (uint32) | 5 EVAL's best label
                               // of the short and the wave rows | 6, 7 a long row's first table slot (int64, a multiple of 2 x seg)
                               // (one pointer, and one for the tables: the kernel's scalar registers are counted)
  int* tab;                    // the long rows' tables: table_cap labels | table_cap weights (uint32) | item_cap best labels of the
                               // items | item_cap best scores (int64) | item_cap (vertex, segment) items
  lv_trace_t* trace;
  lv_control_t* ctl;
  size_t N;
  long long item_cap;          // table_cap = item_cap x 2 x seg
  double tol;
  int max_iter, trace_cap, timing;
  row_cuts_t cuts;
  unsigned seed;
  __device__ __forceinline__ int* lab_of(int b) const { return vert + (size_t)(b & 1) * N; }
  __device__ __forceinline__ unsigned* sigma_of(int b) const { return (unsigned*)vert + (size_t)(2 + (b & 1)) * N; }
  __device__ __forceinline__ unsigned* k() const { return (unsigned*)vert + 4 * N; }
  __device__ __forceinline__ int* best() const { return vert + 5 * N; }
  __device__ __forceinline__ long long* base() const { return (long long*)(vert + 6 * N); }
  __device__ __forceinline__ size_t table_cap() const { return (size_t)item_cap * 2 * (size_t)cuts.seg; }
  __device__ __forceinline__ int* tkeys() const { return tab; }
  __device__ __forceinline__ unsigned* tsum() const { return (unsigned*)tab + table_cap(); }
  __device__ __forceinline__ int* wlabel() const { return tab + 2 * table_cap(); }
  __device__ __forceinline__ long long* wscore() const { return (long long*)(tab + 2 * table_cap() + 2 * (size_t)((item_cap + 1) / 2)); }
  __device__ __forceinline__ int2* items() const { return (int2*)(wscore() + item_cap); }
};

// a candidate: its score and its label.  Wider than one 64-bit word, so the order is a function
struct lv_best_t { long long score; int label; };
__device__ __forceinline__ bool lv_better(const lv_best_t& x, const lv_best_t& y, int cur, unsigned seed) {
  if (x.score != y.score) return x.score > y.score;
  if (x.label == y.label) return false;
  if ((x.label == cur) != (y.label == cur)) return x.label == cur;
  return color_key(x.label, seed) < color_key(y.label, seed);
}
__device__ __forceinline__ long long lv_score(unsigned kvc, long long W, unsigned sigma_c, bool is_cur, unsigned kv) {
  return (long long)kvc * W - ((long long)sigma_c - (is_cur ? (long long)kv : 0ll)) * (long long)kv;
}
__device__ __forceinline__ lv_best_t lv_wave_best(lv_best_t b, int cur, unsigned seed) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    lv_best_t o;
    o.score = __shfl_xor(b.score, d, WAVE);
    o.label = __shfl_xor(b.label, d, WAVE);
    if (lv_better(o, b, cur, seed)) b = o;
  }
  return b;
}
__device__ __forceinline__ long long lv_threshold(double tol, u64 w) {
  const double x = tol * (double)w * (double)w;
  return x >= (double)LV_THR_MAX ? LV_THR_MAX : min((long long)ceil(x), LV_THR_MAX);
}

// a lane's row of at most LV_SHORT_CAP entries: labels and weights in registers, every pair compared
__device__ __forceinline__ int lv_short_best(const lv_args_t& a, const lv_row_t& r, int v, int cur, unsigned kv, long long W,
                                             const int* __restrict__ lab, const unsigned* __restrict__ sigma) {
  int l[LV_SHORT_CAP];
  unsigned x[LV_SHORT_CAP];
  const int len = r.len();
#pragma unroll
  for (int j = 0; j < LV_SHORT_CAP; ++j) {
    l[j] = LV_EMPTY;
    x[j] = 0;
    if (j < len) {
      unsigned xx;
      const int u = lv_entry(a.g, r, v, j, &xx);
      if (u != v && xx) { l[j] = lab[u]; x[j] = xx; }
    }
  }
  lv_best_t best = {lv_score(0, W, sigma[cur], true, kv), cur};
  // the candidate is slot 0 and the slots rotate, so that every index is a constant (the arrays stay in registers) and the body
  // is compiled once (unrolled, its sixteen copies' compare masks spilled a hundred scalar registers)
#pragma unroll 1
  for (int i = 0; i < len; ++i) {
    const int cand = l[0];
    const unsigned x0 = x[0];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < LV_SHORT_CAP; ++j) c += l[j] == cand ? x[j] : 0u;
    if (cand != LV_EMPTY) {
      const lv_best_t o = {lv_score(c, W, sigma[cand], cand == cur, kv), cand};
      if (lv_better(o, best, cur, a.seed)) best = o;
    }
#pragma unroll
    for (int j = 0; j + 1 < LV_SHORT_CAP; ++j) { l[j] = l[j + 1]; x[j] = x[j + 1]; }
    l[LV_SHORT_CAP - 1] = cand;
    x[LV_SHORT_CAP - 1] = x0;
  }
  return best.label;
}

// `weight` for `label` into an open-addressed LDS table of `slots` slots (a power of two, more than the row has entries)
__device__ __forceinline__ void lv_lds_insert(int* keys, unsigned* sums, int slots, int label, unsigned weight) {
  unsigned h = color_fmix32((unsigned)label ^ 0x9E3779B9u) & (unsigned)(slots - 1);
  for (int probe = 0; probe < slots; ++probe) {
    int old = keys[h];
    if (old == LV_EMPTY) old = atomicCAS(keys + h, LV_EMPTY, label);
    if (old == LV_EMPTY || old == label) {
      atomicAdd(sums + h, weight);
      return;
    }
    h = (h + 1) & (unsigned)(slots - 1);
  }
}

// a wave's row of at most LV_WAVE_CAP entries (all lanes call with the same row)
__device__ __forceinline__ int lv_wave_row_best(const lv_args_t& a, const lv_row_t& r, int v, int cur, unsigned kv, long long W,
                                                const int* __restrict__ lab, const unsigned* __restrict__ sigma, int* keys,
                                                unsigned* sums) {
  const int lane = lane_id();
  const int len = r.len();
  int slots = 2 * WAVE;
  while (slots < 2 * len) slots *= 2;                          // (len <= LV_WAVE_CAP: at most 2 x LV_WAVE_CAP)
  for (int s = lane; s < slots; s += WAVE) { keys[s] = LV_EMPTY; sums[s] = 0; }
  wave_lds_fence();
  for (int j = lane; j < len; j += WAVE) {
    unsigned xx;
    const int u = lv_entry(a.g, r, v, j, &xx);
    if (u != v && xx) lv_lds_insert(keys, sums, slots, lab[u], xx);
  }
  wave_lds_fence();
  lv_best_t best = {lv_score(0, W, sigma[cur], true, kv), cur};
  for (int s = lane; s < slots; s += WAVE) {
    const int c = keys[s];
    if (c != LV_EMPTY) {
      const lv_best_t o = {lv_score(sums[s], W, sigma[c], c == cur, kv), c};
      if (lv_better(o, best, cur, a.seed)) best = o;
    }
  }
  wave_lds_fence();                                            // (the table is cleared again by the next row)
  return lv_wave_best(best, cur, a.seed).label;
}

struct lv_lds_t {
  int keys[WAVES_PER_BLOCK][2 * LV_WAVE_CAP];
  unsigned sums[WAVES_PER_BLOCK][2 * LV_WAVE_CAP];
  u64 red[2][WAVES_PER_BLOCK];
};

__device__ __forceinline__ int lv_clock_of(int kind) {
  if (kind == LV_SETUP) return LV_T_SETUP;
  if (kind == LV_EVAL) return LV_T_EVAL;
  if (kind == LV_LONG_FILL || kind == LV_LONG_SCAN) return LV_T_LONG;
  return kind == LV_APPLY ? LV_T_APPLY : LV_T_QNUM;
}
// two sums of a workgroup, one atomic each (all threads call)
__device__ __forceinline__ void lv_block_add2(u64 x, u64 y, u64* px, u64* py, lv_lds_t& s) {
  x = wave_sum(x);
  y = wave_sum(y);
  if (lane_id() == 0) { s.red[0][threadIdx.x / WAVE] = x; s.red[1][threadIdx.x / WAVE] = y; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) { x += s.red[0][w]; y += s.red[1][w]; }
    if (x) atomicAdd(px, x);
    if (y) atomicAdd(py, y);
  }
}

// launch: the launch's number in the level's chain
__global__ __launch_bounds__(BLOCK) void k_louvain_step(lv_args_t a, unsigned launch) {
  const lv_word_t prev = a.ctl->left_by_prev(launch);
  lv_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left.  totals.w and totals.n_items are SETUP's: nothing changes them later
  const long long W = prev.kind == LV_INIT ? 0 : (long long)a.ctl->totals.w;
  const int n_items = prev.kind == LV_INIT ? 0 : a.ctl->totals.n_items;
  int kind, t = prev.t, cur = prev.cur, rejects = prev.rejects, accepted = prev.accepted;
  long long q = prev.q, qn = 0;
  bool ok = false;
  if (prev.kind == LV_INIT) {
    kind = LV_SETUP;
  } else if (prev.kind == LV_SETUP) {
    q = (long long)prev.s_in * W - (long long)prev.s_sq;
    kind = (W == 0 || a.max_iter == 0) ? LV_DONE : LV_EVAL;
  } else if (prev.kind == LV_EVAL) {
    kind = n_items > 0 ? LV_LONG_FILL : LV_APPLY;
  } else if (prev.kind == LV_LONG_FILL) {
    kind = LV_LONG_SCAN;
  } else if (prev.kind == LV_LONG_SCAN) {
    kind = LV_APPLY;
  } else if (prev.kind == LV_APPLY) {
    kind = LV_QNUM;
  } else if (prev.kind == LV_QNUM) {
    qn = (long long)prev.s_in * W - (long long)prev.s_sq;
    ok = prev.moved > 0 && qn - q > lv_threshold(a.tol, (u64)W);
    if (ok) { cur ^= 1; q = qn; rejects = 0; ++accepted; }
    else ++rejects;
    ++t;
    kind = (rejects >= 2 || t >= a.max_iter) ? LV_DONE : LV_EVAL;
  } else {
    kind = LV_DONE;
  }
  if (first_thread) {
    const lv_word_t* const pw = a.ctl->left_by_prev_at(launch);
    next->kind = kind; next->t = t; next->cur = cur; next->rejects = rejects; next->accepted = accepted; next->q = q;
    lv_totals_t& tot = a.ctl->totals;
    a.ctl->log_kind(launch, kind);
    if (kind == LV_QNUM) atomicAdd(&next->moved, pw->moved);      // (the iteration's movers go on through QNUM)
    if (pw->kind == LV_SETUP) { tot.s_in = pw->s_in; tot.s_sq = pw->s_sq; }
    if (pw->kind == LV_QNUM) {
      if (pw->t < a.trace_cap) { a.trace[pw->t].moved = pw->moved; a.trace[pw->t].accepted = ok ? 1 : 0; a.trace[pw->t].q = qn; }
      if (ok) { tot.s_in = pw->s_in; tot.s_sq = pw->s_sq; }
    }
    if (kind == LV_DONE && pw->kind != LV_DONE) {
      tot.q = q; tot.cur = cur; tot.iterations = t; tot.accepted = accepted;
      tot.done |= 1;
    }
    tot.timed.tick(a.timing, pw->kind, LV_DONE, lv_clock_of(pw->kind));
  }
  if (kind == LV_DONE) return;

  const int lane = lane_id();
  const int wave_in_block = threadIdx.x / WAVE;
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  const int n = a.g.n;
  __shared__ lv_lds_t lds;
  const int* const lab_c = a.lab_of(cur);
  int* const lab_o = a.lab_of(cur ^ 1);
  const unsigned* const sig_c = a.sigma_of(cur);
  unsigned* const sig_o = a.sigma_of(cur ^ 1);

  if (kind == LV_SETUP) {
    row_bins_t bins;
    u64 s_in = 0, s_sq = 0, wsum = 0;
    for (unsigned b0 = (unsigned)wave * WAVE; b0 < (unsigned)n; b0 += (unsigned)waves * WAVE) {
      const bool in = b0 + lane < (unsigned)n;
      const int v = (int)(b0 + lane);
      const lv_row_t r = lv_row(a.g, in, v);
      const int len = r.len();
      u64 kv = 0, self = 0;
      if (len <= LV_QNUM_LANE_MAX)
        for (int j = 0; j < len; ++j) {
          unsigned x;
          const int u = lv_entry(a.g, r, v, j, &x);
          kv += x;
          self += u == v ? x : 0u;
        }
      for_each_wave_row(len > LV_QNUM_LANE_MAX, [&](int src) {
        const lv_row_t rr = r.of_lane(src);
        const int vv = __shfl(v, src, WAVE);
        u64 c = 0, sf = 0;
        for (int j = lane; j < rr.len(); j += WAVE) {
          unsigned x;
          const int u = lv_entry(a.g, rr, vv, j, &x);
          c += x;
          sf += u == vv ? x : 0u;
        }
        c = wave_sum(c);
        sf = wave_sum(sf);
        if (lane == src) { kv = c; self = sf; }
      });
      const int body = in ? a.cuts.body_of(len) : -1;
      if (in) {
        a.lab_of(0)[v] = v;
        a.k()[v] = (unsigned)kv;
        a.sigma_of(0)[v] = (unsigned)kv;
      }
      if (body == ROW_LONG) {
        const unsigned long long room = (unsigned long long)a.cuts.segments_of(len) * (unsigned long long)(2 * a.cuts.seg);
        a.base()[v] = (long long)atomicAdd(&a.ctl->totals.cursor, room);
      }
      if (__ballot(body == ROW_LONG)) wave_append_segments(body == ROW_LONG, v, len, a.cuts.seg, a.items(), &a.ctl->totals.n_items);
      bins.count(body);
      s_in += self;
      s_sq += kv * kv;
      wsum += kv;
    }
    bins.add_to(a.ctl->totals.bins);
    wsum = wave_sum(wsum);
    if (lane == 0 && wsum) atomicAdd(&a.ctl->totals.w, wsum);
    lv_block_add2(s_in, s_sq, &next->s_in, &next->s_sq, lds);
    return;
  }

  if (kind == LV_LONG_FILL) {                                // a wave per item: seg entries into the row's table
    for (int it = wave; it < n_items; it += waves) {
      const int2 item = a.items()[it];
      const int v = item.x;
      const lv_row_t r = lv_row(a.g, true, v);
      const int len = r.len();
      const long long tb = a.base()[v];
      const unsigned slots = 2u * (unsigned)len;
      const int j1 = min(len, (item.y + 1) * a.cuts.seg);
      for (int j = item.y * a.cuts.seg + lane; j < j1; j += WAVE) {
        unsigned x;
        const int u = lv_entry(a.g, r, v, j, &x);
        if (u == v || !x) continue;
        const int label = lab_c[u];
        unsigned h = color_fmix32((unsigned)label ^ 0x9E3779B9u) % slots;
        for (unsigned probe = 0; probe < slots; ++probe) {
          int old = __hip_atomic_load(a.tkeys() + tb + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (old == LV_EMPTY) old = atomicCAS(a.tkeys() + tb + h, LV_EMPTY, label);
          if (old == LV_EMPTY || old == label) {
            atomicAdd(a.tsum() + tb + h, x);
            break;
          }
          h = h + 1 == slots ? 0 : h + 1;
        }
      }
    }
    return;
  }

  if (kind == LV_LONG_SCAN) {                                // a wave per item: 2 x seg slots scored and emptied
    for (int it = wave; it < n_items; it += waves) {
      const int2 item = a.items()[it];
      const int v = item.x;
      const lv_row_t r = lv_row(a.g, true, v);
      const long long tb = a.base()[v];
      const long long s1 = min(2ll * r.len(), 2ll * (item.y + 1) * a.cuts.seg);
      const int c0 = lab_c[v];
      const unsigned kv = a.k()[v];
      lv_best_t best = {lv_score(0, W, sig_c[c0], true, kv), c0};
      for (long long s = 2ll * item.y * a.cuts.seg + lane; s < s1; s += WAVE) {
        const int c = a.tkeys()[tb + s];
        if (c != LV_EMPTY) {
          const lv_best_t o = {lv_score(a.tsum()[tb + s], W, sig_c[c], c == c0, kv), c};
          if (lv_better(o, best, c0, a.seed)) best = o;
          a.tkeys()[tb + s] = LV_EMPTY;
          a.tsum()[tb + s] = 0;
        }
      }
      best = lv_wave_best(best, c0, a.seed);
      if (lane == 0) {
        const long long slot = tb / (2 * a.cuts.seg) + item.y;
        a.wscore()[slot] = best.score;
        a.wlabel()[slot] = best.label;
      }
    }
    return;
  }

  if (kind == LV_EVAL) {
    int* const keys = lds.keys[wave_in_block];
    unsigned* const sums = lds.sums[wave_in_block];
    for (unsigned b0 = (unsigned)wave * WAVE; b0 < (unsigned)n; b0 += (unsigned)waves * WAVE) {
      const bool in = b0 + lane < (unsigned)n;
      const int v = in ? (int)(b0 + lane) : 0;
      const lv_row_t r = lv_row(a.g, in, v);
      const int body = in ? a.cuts.body_of(r.len()) : ROW_NONE;
      const int c0 = in ? lab_c[v] : 0;
      const unsigned kv = in ? a.k()[v] : 0u;
      int w = c0;
      if (body == ROW_LANE) w = lv_short_best(a, r, v, c0, kv, W, lab_c, sig_c);
      for_each_wave_row(body == ROW_WAVE, [&](int src) {
        const int ww = lv_wave_row_best(a, r.of_lane(src), __shfl(v, src, WAVE), __shfl(c0, src, WAVE), (unsigned)__shfl((int)kv, src, WAVE), W, lab_c,
                                        sig_c, keys, sums);
        if (lane == src) w = ww;
      });
      if (in) {
        a.best()[v] = w;
        sig_o[v] = sig_c[v];
      }
    }
    return;
  }

  if (kind == LV_APPLY) {
    int moved = 0;
    for (unsigned b0 = (unsigned)wave * WAVE; b0 < (unsigned)n; b0 += (unsigned)waves * WAVE) {
      const bool in = b0 + lane < (unsigned)n;
      const int v = in ? (int)(b0 + lane) : 0;
      const lv_row_t r = lv_row(a.g, in, v);
      const int body = in ? a.cuts.body_of(r.len()) : ROW_NONE;
      const int c0 = in ? lab_c[v] : 0;
      const unsigned kv = in ? a.k()[v] : 0u;
      int w = in ? a.best()[v] : 0;
      for_each_wave_row(body == ROW_LONG, [&](int src) {      // a long row's best is the best of its items' slots
        const int vv = __shfl(v, src, WAVE);
        const int cc = __shfl(c0, src, WAVE);
        const unsigned kk = (unsigned)__shfl((int)kv, src, WAVE);
        const int segs = a.cuts.segments_of(__shfl(r.len(), src, WAVE));
        const long long slot0 = a.base()[vv] / (2 * a.cuts.seg);
        lv_best_t best = {lv_score(0, W, sig_c[cc], true, kk), cc};
        for (int s = lane; s < segs; s += WAVE) {
          const lv_best_t o = {a.wscore()[slot0 + s], a.wlabel()[slot0 + s]};
          if (lv_better(o, best, cc, a.seed)) best = o;
        }
        best = lv_wave_best(best, cc, a.seed);
        if (lane == src) w = best.label;
      });
      const unsigned kw = color_key(w, a.seed), kc = color_key(c0, a.seed);
      const bool moves = in && w != c0 && ((t & 1) ? kw > kc : kw < kc);
      if (in) lab_o[v] = moves ? w : c0;
      if (moves && kv) {
        atomicSub(sig_o + c0, kv);
        atomicAdd(sig_o + w, kv);
      }
      moved += moves ? 1 : 0;
    }
    moved = wave_sum(moved);
    if (lane == 0 && moved) atomicAdd(&next->moved, moved);
    return;
  }

  {                                                          // QNUM: of the other buffer's labels
    u64 s_in = 0, s_sq = 0;
    for (unsigned b0 = (unsigned)wave * WAVE; b0 < (unsigned)n; b0 += (unsigned)waves * WAVE) {
      const bool in = b0 + lane < (unsigned)n;
      const int v = in ? (int)(b0 + lane) : 0;
      const lv_row_t r = lv_row(a.g, in, v);
      const int len = r.len();
      const int body = in ? a.cuts.body_of(len) : ROW_NONE;
      const int l = in ? lab_o[v] : 0;
      if (body != ROW_LONG && len <= LV_QNUM_LANE_MAX)
        for (int j = 0; j < len; ++j) {
          unsigned x;
          const int u = lv_entry(a.g, r, v, j, &x);
          s_in += lab_o[u] == l ? x : 0u;
        }
      for_each_wave_row(body != ROW_LONG && len > LV_QNUM_LANE_MAX, [&](int src) {
        const lv_row_t rr = r.of_lane(src);
        const int vv = __shfl(v, src, WAVE), ll = __shfl(l, src, WAVE);
        for (int j = lane; j < rr.len(); j += WAVE) {
          unsigned x;
          const int u = lv_entry(a.g, rr, vv, j, &x);
          s_in += lab_o[u] == ll ? x : 0u;
        }
      });
      if (in) {
        const u64 s = sig_o[v];
        s_sq += s * s;
      }
    }
    for (int it = wave; it < n_items; it += waves) {           // the long rows, by their items
      const int2 item = a.items()[it];
      const int v = item.x;
      const lv_row_t r = lv_row(a.g, true, v);
      const int l = lab_o[v];
      const int j1 = min(r.len(), (item.y + 1) * a.cuts.seg);
      for (int j = item.y * a.cuts.seg + lane; j < j1; j += WAVE) {
        unsigned x;
        const int u = lv_entry(a.g, r, v, j, &x);
        s_in += lab_o[u] == l ? x : 0u;
      }
    }
    lv_block_add2(s_in, s_sq, &next->s_in, &next->s_sq, lds);
  }
}

// what mgx_louvain_levels reports of a level that ran
struct lv_level_t {
  long long vertices, entries, iterations, accepted, communities, q;
};

// The device state of a graph's fused Louvain run, and the run (host side).  Everything is allocated at the first run: a repeat run
// allocates nothing (later runs do only when one asks for more iterations than any before -- the trace --, is the first that is not
// symmetric -- twice the entries --, or when the levels together have more than 2 n vertices -- the maps).
struct louvain_fused_state_t {
  int n = 0;
  long long m = 0;
  lv_opts_t opts;
  size_t N = 1;
  long long E = 1;                              // level 0's entries at most, as allocated: m, or 2 m once a run was not symmetric
  mem_t<int> vert, tab, final_lab, maps;           // (lv_args_t::vert and ::tab)
  mem_t<int> cro[2], cci[2];
  mem_t<unsigned> cwt[2];
  long long item_cap = 0, table_cap = 0;
  mem_t<lv_trace_t> trace;
  int trace_cap = 0;
  mem_t<lv_control_t> ctl;
  pinned_t<lv_totals_t> h_totals;
  std::unique_ptr<louvain_aggregate_t> agg;
  std::unique_ptr<lpa_label_stats_t> label_stats;
  bool allocated = false, tables_clean = false;
  // the last run
  long long launches = -1;                      // -1: no run yet
  std::vector<int> kinds;                       // the launches' kinds, level by level, each up to its DONE
  std::vector<lv_level_t> levels;
  std::vector<long long> map_off;               // the aggregated levels' maps in `maps`: [l] .. [l + 1]
  std::vector<long long> h_trace;               // (moved, accepted, Qnum) per iteration, over the levels
  long long bins[4] = {0, 0, 0, 0}, long_items = 0, waits = 0;
  bool timing = false;
  double phase_ms[6] = {0, 0, 0, 0, 0, 0};

  louvain_fused_state_t(int n_, long long m_, context_t&) : n(n_), m(m_), opts(lv_opts_t::from_env()) {}

  // everything a run of at most `entries` level-0 entries needs (m when symmetric, 2 m else): once, and again only when a later
  // run on the handle needs more
  void allocate(long long entries, standard_context_t& ctx) {
    if (allocated && entries <= E) return;
    if (allocated) MGX_HIP(hipStreamSynchronize(ctx.stream()));
    allocated = false;
    tables_clean = false;
    N = (size_t)std::max(n, 1);
    E = std::max<long long>(entries, 1);
    vert = mem_t<int>(8 * N, ctx);
    final_lab = mem_t<int>(N, ctx);
    maps = mem_t<int>(2 * N, ctx);
    // rows of more than wave_max entries: an item per seg entries and one more per row; a table of 2 x seg slots per item
    const long long long_cap = std::min<long long>((long long)N, E / (opts.cuts.wave_max + 1) + 1);
    item_cap = E / opts.cuts.seg + long_cap + 1;
    table_cap = item_cap * 2 * opts.cuts.seg;
    tab = mem_t<int>(2 * (size_t)table_cap + 2 * (size_t)((item_cap + 1) / 2) + 4 * (size_t)item_cap, ctx);
    for (int i = 0; i < 2; ++i) {
      cro[i] = mem_t<int>(N + 1, ctx);
      cci[i] = mem_t<int>((size_t)E, ctx);
      cwt[i] = mem_t<unsigned>((size_t)E, ctx);
    }
    ctl = mem_t<lv_control_t>(1, ctx);
    h_totals = pinned_t<lv_totals_t>(1);
    agg.reset(new louvain_aggregate_t(n, E, ctx));
    label_stats.reset(new lpa_label_stats_t(n, ctx));
    allocated = true;
  }

  // (ro, ci: the CSR on the device; co, ri: its genuine CSC, read when symmetric == 0 only).  Returns {communities, largest, its
  // id, levels, S_in, S_sq, W, host waits, launches, iterations}.
  std::vector<long long> run(const int* ro, const int* ci, const int* co, const int* ri, int symmetric, unsigned seed, int max_iter,
                             int max_levels, double tol, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    launches = -1;
    kinds.clear(); levels.clear(); h_trace.clear();
    map_off.assign(1, 0);
    for (int b = 0; b < 4; ++b) bins[b] = 0;
    for (int i = 0; i < 6; ++i) phase_ms[i] = 0.0;
    long_items = 0; waits = 0;
    if (n <= 0) {
      launches = 0;
      return {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    allocate(symmetric ? m : 2 * m, ctx);
    agg->waits = 0;
    if (trace_cap < max_iter + 1) {
      trace = mem_t<lv_trace_t>((size_t)max_iter + 1, ctx);
      trace_cap = max_iter + 1;
    }
    // the tables are empty before the first iteration and LONG_SCAN leaves them so: they are cleared for the handle's first run
    // and behind a run that did not end
    if (!tables_clean) {
      MGX_HIP(hipMemsetAsync(tab.data(), 0xff, (size_t)table_cap * sizeof(int), st));
      MGX_HIP(hipMemsetAsync(tab.data() + table_cap, 0, (size_t)table_cap * sizeof(unsigned), st));
    }
    tables_clean = false;
    lv_args_t a;
    a.vert = vert.data(); a.tab = tab.data(); a.trace = trace.data(); a.ctl = ctl.data();
    a.N = N; a.item_cap = item_cap; a.tol = tol; a.max_iter = max_iter; a.trace_cap = trace_cap;
    a.cuts = opts.cuts; a.timing = timing ? 1 : 0; a.seed = seed;
    lv_graph_t g = {ro, ci, nullptr, symmetric ? nullptr : co, symmetric ? nullptr : ri, n};
    long long entries = symmetric ? m : 2 * m, total_launches = 0, iterations = 0;
    unsigned long long W = 0, s_in = 0, s_sq = 0;
    bool any = false;
    int level = 0;
    for (;; ++level) {
      const bool sums_only = level >= max_levels;             // (max_levels == 0: SETUP alone, for W and the identity's sums)
      lv_control_t::reset(ctl.data(), st);
      a.g = g;
      a.max_iter = sums_only ? 0 : max_iter;
      const int blocks = grid_for(g.n, BLOCK, std::max(ctx.num_cus, 1) * 4);
      // SETUP, and at most an EVAL, two LONG launches, an APPLY and a QNUM per iteration: a chain that is longer has not ended
      const long long most = 5ll * ((long long)max_iter + 2) + CHAIN_BATCH_MAX;
      const long long enqueued = run_launch_chain(
          [&](long long i) { hipLaunchKernelGGL(k_louvain_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
          [&]() {
            h_totals.fetch(&ctl.data()->totals, 1, st);
            return (h_totals->done & 1) != 0;
          },
          most, "mgx louvain step", &waits);
      total_launches += enqueued;
      const lv_totals_t tot = *h_totals.data();
      if (level == 0) { W = tot.w; s_in = tot.s_in; s_sq = tot.s_sq; }
      if (W == 0 || sums_only) break;                          // (no votes: identity labels, no level)
      {                                                      // the level's launches up to its DONE, and its trace
        const size_t have = (size_t)std::min<long long>(enqueued, CHAIN_LOG_CAP);
        std::vector<int> log(have);
        MGX_HIP(dtoh(log.data(), (const int*)ctl.data()->log, have, st));
        for (size_t i = 0; i < have; ++i) {
          kinds.push_back(log[i]);
          if (log[i] == LV_DONE) break;
        }
        std::vector<lv_trace_t> tr((size_t)tot.iterations);
        MGX_HIP(dtoh(tr.data(), (const lv_trace_t*)trace.data(), tr.size(), st));
        for (const lv_trace_t& x : tr) { h_trace.push_back(x.moved); h_trace.push_back(x.accepted); h_trace.push_back(x.q); }
      }
      if (timing)
        for (int i = 0; i < 5; ++i) phase_ms[i] += chain_ticks_ms(tot.timed.clock[i]);
      for (int b = 0; b < 4; ++b) bins[b] += tot.bins[b];
      long_items += (long long)tot.n_items * tot.iterations;
      iterations += tot.iterations;
      lv_level_t rec = {g.n, entries, tot.iterations, tot.accepted, g.n, tot.q};
      if (tot.accepted == 0) {
        levels.push_back(rec);
        break;
      }
      s_in = tot.s_in; s_sq = tot.s_sq;
      const auto t0 = std::chrono::steady_clock::now();
      // dense ids; the map joins the dendrogram; the coarse graph unless this was the last level
      const long long at = map_off.back();
      if ((size_t)(at + g.n) > maps.size()) {
        mem_t<int> bigger(2 * (size_t)(at + g.n), ctx);
        MGX_HIP(dtod(bigger.data(), (const int*)maps.data(), (size_t)at, st));
        MGX_HIP(hipStreamSynchronize(st));
        maps.swap(bigger);
      }
      const bool more = level + 1 < max_levels;
      const int* const labels = vert.data() + (size_t)(tot.cur & 1) * N;
      const unsigned* const kk = (const unsigned*)vert.data() + 4 * N;
      const int nc = agg->renumber(g, labels, kk, maps.data() + at, final_lab.data(), n, !any, more, ctx);
      any = true;
      map_off.push_back(at + g.n);
      rec.communities = nc;
      levels.push_back(rec);
      if (more) {
        const int o = level & 1;
        const long long total = g.wt ? entries : (long long)W;
        entries = agg->contract(g, maps.data() + at, kk, nc, total, cro[o].data(), cci[o].data(), cwt[o].data(), ctx);
        g = lv_graph_t{cro[o].data(), cci[o].data(), cwt[o].data(), nullptr, nullptr, nc};
      }
      if (!more) {
        if (timing) phase_ms[LV_T_AGG] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        break;
      }
      if (timing) {
        MGX_HIP(hipStreamSynchronize(st));
        phase_ms[LV_T_AGG] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
    }
    if (!any) hipLaunchKernelGGL(k_cc_init, dim3(grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(BLOCK), 0, st, final_lab.data(), n);
    const std::vector<long long> ls = label_stats->run(final_lab.data(), n, ctx);
    waits += agg->waits + 1;
    tables_clean = true;
    launches = total_launches;
    return {ls[0], ls[1], ls[2], (long long)map_off.size() - 1, (long long)s_in, (long long)s_sq, (long long)W, waits, launches, iterations};
  }
};

}  // namespace mgx
