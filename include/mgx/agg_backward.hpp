// mgx/agg_backward.hpp -- the backward of the neighbour feature aggregation (mgx_aggbwd_run; the forward is agg_fused.hpp): the
// gradient with respect to the features, GX[c, :] = (+)_{e : col_e == c} w_e g[row_e, :], in a fixed order of arithmetic, over the
// TRANSPOSED rows of the forward's CSR -- the graph's out-rows, its in-rows or the rows of a neighbour-sampling run.
//
// The definition (the operator path include/gunrock/aggbwd/ and tests/aggbwd_model.py compute the same float32 bits).
//   upstream g[r, f] = GY[r, f]; for mean agg_div(GY[r, f], float(d_r)), one correctly rounded division BEFORE the weight
//   L_c      the selected rows' entries e with col_e == c in ASCENDING e, the forward's stored order
//   term     u_e = g[row_e, f], or agg_term(w_e, g[row_e, f]) rounded once, never fused with the add; for max / min u_e is that when
//            e == win[row_e, f] and +0.0 otherwise (the kernel selects, it does not compact)
//   win      the entry whose term the forward's fold kept, recomputed from X: within a segment the first entry, then e exactly when
//            t_e > acc (max) / t_e < acc (min); the segments' winners combined in segment order by the same test on their values;
//            a row without entries has none (-1)
//   fold     GX[c, f] is the forward's fold of L_c's terms: segments of seg entries, acc = u_0 then acc = acc + u_j, the segments'
//            values added in segment order; an empty L_c gives +0.0.  Every element of GX[:x_rows, :F] is written on every run,
//            the padding columns never.
// The transposed CSR (t_off[x_rows + 1], t_row[E] the forward row and t_pos[E] the forward entry of every slot) is built on the
// device: a count by column (integer adds: the counts do not depend on their order), the library's exclusive scan, a cursor fill
// in whatever order the adds land, then segsort.hpp's segmented sort of every transposed row ascending by t_pos -- the keys are
// distinct, so the result is one array whatever the fill did -- and t_row by a binary search of t_pos in the forward's offsets.
// (A stable radix pass by column would sort E keys of log2(x_rows) bits in several passes over all of them; the segmented sort
// touches a row's slots only and is the library's own.)  For the out- and in-rows it is built by the first run and kept for the
// handle's life with the plan of its long rows; for a block it is rebuilt on every run.
// The launches of the backward proper mirror the forward's: a team of G lanes per transposed row, lane-columns of 4 floats where F,
// ldgy, ldgx are multiples of 4 and both bases 16-byte aligned, AGG_UNROLL slots' loads in flight per trip in rounds (t_row and
// t_pos; the weight's place; the weight; the pieces of g[row] and for max / min of win[row]), adds
// in L_c's order; transposed rows longer than seg as (row, segment) items and a fold (k_agg_plan_count / k_agg_plan_fill over t_off).
// The mean's division is a pass of its own that writes g into a handle-owned R x F buffer (k_aggb_scale, one launch more; done in
// the walk it would divide once per ENTRY and cost the rows' and the items' kernels 14 to 20 spilled scalar registers).  No atomics
// on GX, no LDS, no scratch.
//   k_aggb_rows / k_aggb_items / k_aggb_fold           the backward, as the forward's three
//   k_aggb_scale                                       mean only: g
//   k_aggb_win_rows / k_aggb_win_items / k_aggb_win_fold   max / min only: win[R, F] over the FORWARD rows, as the forward's three
//   k_aggb_tr_count / k_aggb_tr_fill / k_aggb_tr_rows  the transpose
// Not built: the gradient with respect to the edge weights; the graph's CSC as a shortcut for sum / mean (the winner test needs
// t_pos, and one mechanism is one definition); fp16 / bf16; several blocks per launch.
#pragma once
#include <algorithm>
#include <vector>

#include "agg_fused.hpp"
#include "scan.hpp"
#include "segsort.hpp"

namespace mgx {

enum : int { AGGB_K_SUM = 0, AGGB_K_WIN = 1 };      // what a backward kernel is compiled for (the mean runs the sum's on g)
enum : int { AGGB_STATS = 10, AGGB_BINS = 5, AGGB_PHASES = 5 };

template <typename V> struct aggb_ivec;
template <> struct aggb_ivec<float> {
  typedef int type;
  static __device__ __forceinline__ int splat(int e) { return e; }
};
template <> struct aggb_ivec<float4> {
  typedef int4 type;
  static __device__ __forceinline__ int4 splat(int e) { return make_int4(e, e, e, e); }
};

// ---- the arithmetic both paths share beyond agg_term / agg_comb / agg_div ----
// the term of an entry that did not win is +0.0: selected, never multiplied (a NaN gradient stays with the winner)
__device__ __forceinline__ float aggb_pick(int win, int e, float u) { return win == e ? u : 0.f; }
__device__ __forceinline__ float4 aggb_pick(int4 win, int e, float4 u) {
  return make_float4(aggb_pick(win.x, e, u.x), aggb_pick(win.y, e, u.y), aggb_pick(win.z, e, u.z), aggb_pick(win.w, e, u.w));
}
__device__ __forceinline__ float aggb_sel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ float4 aggb_sel(bool c, float4 a, float4 b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }
// the forward's max / min step with its winner: e takes over exactly when the comparison is true
template <int K>
__device__ __forceinline__ void aggb_take(float& acc, int& win, float t, int e) {
#pragma clang fp contract(off)
  const bool take = K == AGG_K_MAX ? t > acc : t < acc;
  if (take) { acc = t; win = e; }
}
template <int K>
__device__ __forceinline__ void aggb_take(float4& acc, int4& win, float4 t, int4 e) {
  aggb_take<K>(acc.x, win.x, t.x, e.x);
  aggb_take<K>(acc.y, win.y, t.y, e.y);
  aggb_take<K>(acc.z, win.z, t.z, e.z);
  aggb_take<K>(acc.w, win.w, t.w, e.w);
}
__device__ __forceinline__ void aggb_take_op(int op, float& acc, int& win, float t, int e) {
  if (op == AGG_MAX) aggb_take<AGG_K_MAX>(acc, win, t, e);
  else aggb_take<AGG_K_MIN>(acc, win, t, e);
}

struct aggb_args_t {
  const int* t_off;      // T + 1 offsets of the transposed rows (slots), from 0
  const int* t_row;      // E: the forward row of a slot
  const int* t_pos;      // E: the forward entry of a slot, an absolute place in ci
  const int* ro;         // the forward rows: R + 1 offsets, absolute places in ci
  const int* ci;
  const int* entry_pos;  // a block's: the place of entry e in the graph's weights (NULL: e itself)
  const float* w;        // NULL: unweighted
  const float* gy;
  const float* x;        // max / min only
  float* gx;
  float* g;              // R x ldp, mean only: the upstream value
  int* win;              // R x ldw, max / min only
  float* partials;       // n_items x ldp
  int* wparts;           // n_items x ldp: the winners of the forward's long rows' segments
  const int2* items;
  const int2* heads;
  agg_control_t* ctl;
  long long ldgy, ldx, ldgx, ldp;
  int ldw;               // (win's leading dimension: feats rounded up to 4, at most 65536)
  int R, T, C, G, tiles, op, seg, n_items, n_long;
};

// The sibling of agg_walk over the slots [beg, beg + len) of one transposed row (or one of its segments): the lane's piece of every
// g[t_row] at float offset `coff`, folded in L_c's order.  Every lane runs the same trips.
template <typename V, int K>
__device__ __forceinline__ V aggb_walk(const aggb_args_t& a, int beg, int len, long long coff, bool on, int maxlen) {
#pragma clang fp contract(off)
  typedef typename aggb_ivec<V>::type I;
  V acc = agg_vec<V>::zero();
  const int mine = on ? len : 0;
  for (int base = 0; base < maxlen; base += AGG_UNROLL) {
    V gs[AGG_UNROLL];
    I wn[AGG_UNROLL];
    float ws[AGG_UNROLL];
    int rows[AGG_UNROLL], pos[AGG_UNROLL], wpos[AGG_UNROLL];
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) {
      const int s = beg + base + u;
      rows[u] = base + u < mine ? a.t_row[s] : -1;
      pos[u] = base + u < mine ? a.t_pos[s] : 0;
    }
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u)
      wpos[u] = (rows[u] >= 0 && a.entry_pos) ? a.entry_pos[pos[u]] : pos[u];
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) ws[u] = (rows[u] >= 0 && a.w) ? a.w[wpos[u]] : 1.f;
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) {
      gs[u] = rows[u] >= 0 ? *(const V*)(a.gy + (long long)rows[u] * a.ldgy + coff) : agg_vec<V>::zero();
      if (K == AGGB_K_WIN) wn[u] = rows[u] >= 0 ? *(const I*)(a.win + (long long)rows[u] * a.ldw + coff) : aggb_ivec<V>::splat(-1);
    }
    // (selects, not branches: a slot past the lane's own computes on zeros and leaves acc as it is)
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) {
      V t = a.w ? agg_term(ws[u], gs[u]) : gs[u];
      if (K == AGGB_K_WIN) t = aggb_pick(wn[u], pos[u], t);
      const V s = base + u == 0 ? t : agg_comb<AGG_K_ADD>(acc, t);
      acc = aggb_sel(base + u < mine, s, acc);
    }
  }
  return acc;
}

// a team per transposed row; a wave takes 64 / G of them a pass
template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_aggb_rows(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.T + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  // the rows by class in a loop of their own: the counters, the cuts and the control words are then not live across the walk (with
  // them the winners' instances spilled two scalar registers)
  {
    const row_cuts_t cuts = {a.seg, a.seg, a.seg};
    row_bins_t bins;
    long long segs = 0;
    for (int q = wave; q < passes; q += waves) {
      const long long c0 = (long long)q * per_pass + team;
      const int d = c0 < a.T ? a.t_off[c0 + 1] - a.t_off[c0] : 0;
      const int body = c0 < a.T ? cuts.body_of(d) : -1;
      bins.count(j == 0 ? body : -1);
      if (j == 0 && body == ROW_LONG) segs += cuts.segments_of(d);
    }
    bins.add_to(a.ctl->bins);
    segs = wave_sum(segs);
    if (lane == 0 && segs) atomicAdd((u64*)&a.ctl->segments, (u64)segs);
  }
  for (int q = wave; q < passes; q += waves) {
    const long long c0 = (long long)q * per_pass + team;
    const bool valid = c0 < a.T;
    int beg = 0, d = 0;
    if (valid) {
      beg = a.t_off[c0];
      d = a.t_off[c0 + 1] - beg;
    }
    const bool mine = valid && d <= a.seg;                       // (a long row is the items' and the fold's)
    const int maxlen = wave_max(mine ? d : 0);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = mine && c < a.C;
      const V acc = aggb_walk<V, K>(a, beg, d, (long long)c * VW, on, maxlen);
      if (on) *(V*)(a.gx + c0 * a.ldgx + (long long)c * VW) = acc;
    }
  }
}

// a team per (transposed row, segment) item of the long ones
template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_aggb_items(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.n_items + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  for (int q = wave; q < passes; q += waves) {
    const long long it = (long long)q * per_pass + team;
    const bool valid = it < a.n_items;
    int beg = 0, len = 0;
    if (valid) {
      const int2 item = a.items[it];
      const int b0 = a.t_off[item.x];
      const int d = a.t_off[item.x + 1] - b0;
      beg = b0 + item.y * a.seg;
      len = min(a.seg, d - item.y * a.seg);
    }
    const int maxlen = wave_max(len);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = valid && c < a.C;
      const V acc = aggb_walk<V, K>(a, beg, len, (long long)c * VW, on, maxlen);
      if (on) *(V*)(a.partials + it * a.ldp + (long long)c * VW) = acc;
    }
  }
}

// a team per long transposed row adds the row's partials in segment order
template <typename V>
__global__ __launch_bounds__(BLOCK) void k_aggb_fold(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.n_long + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  for (int q = wave; q < passes; q += waves) {
    const long long k = (long long)q * per_pass + team;
    if (k >= a.n_long) continue;
    const int2 head = a.heads[k];
    const int d = a.t_off[head.x + 1] - a.t_off[head.x];
    const int segs = (d + a.seg - 1) / a.seg;
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      if (c >= a.C) continue;
      const float* const p = a.partials + (long long)head.y * a.ldp + (long long)c * VW;
      V acc = *(const V*)p;
      for (int s = 1; s < segs; ++s) acc = agg_comb<AGG_K_ADD>(acc, *(const V*)(p + (long long)s * a.ldp));
      *(V*)(a.gx + (long long)head.x * a.ldgx + (long long)c * VW) = acc;
    }
  }
}

// the mean's upstream value, one pass: g[r, :] = GY[r, :] / float(d_r) into the handle's R x ldp buffer (a row without entries is
// never read: zeros)
template <typename V>
__global__ __launch_bounds__(BLOCK) void k_aggb_scale(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  const long long total = (long long)a.R * a.C, gthreads = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += gthreads) {
    const long long r = i / a.C, c = i % a.C;
    const int d = a.ro[r + 1] - a.ro[r];
    V g = agg_vec<V>::zero();
    if (d > 0) g = agg_div(*(const V*)(a.gy + r * a.ldgy + c * VW), (float)d);
    *(V*)(a.g + r * a.ldp + c * VW) = g;
  }
}

// ---- the winners of max / min over the FORWARD rows: agg_walk's loads and order, the winner beside the value ----
template <typename V, int K>
__device__ __forceinline__ void aggb_win_walk(const aggb_args_t& a, int beg, int len, long long coff, bool on, int maxlen, V& acc,
                                              typename aggb_ivec<V>::type& win) {
#pragma clang fp contract(off)
  acc = agg_vec<V>::zero();
  win = aggb_ivec<V>::splat(-1);
  const int mine = on ? len : 0;
  for (int base = 0; base < maxlen; base += AGG_UNROLL) {
    V xs[AGG_UNROLL];
    float ws[AGG_UNROLL];
    int cols[AGG_UNROLL], wpos[AGG_UNROLL];
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) {
      const int e = beg + base + u;
      cols[u] = base + u < mine ? a.ci[e] : -1;
      wpos[u] = (base + u < mine && a.w && a.entry_pos) ? a.entry_pos[e] : e;
    }
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) ws[u] = (cols[u] >= 0 && a.w) ? a.w[wpos[u]] : 1.f;
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) xs[u] = cols[u] >= 0 ? *(const V*)(a.x + (long long)cols[u] * a.ldx + coff) : agg_vec<V>::zero();
#pragma unroll
    for (int u = 0; u < AGG_UNROLL; ++u) {
      if (base + u < mine) {
        const V t = a.w ? agg_term(ws[u], xs[u]) : xs[u];
        const int e = beg + base + u;
        if (base + u == 0) { acc = t; win = aggb_ivec<V>::splat(e); }
        else aggb_take<K>(acc, win, t, aggb_ivec<V>::splat(e));
      }
    }
  }
}

template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_aggb_win_rows(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  typedef typename aggb_ivec<V>::type I;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.R + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  for (int q = wave; q < passes; q += waves) {
    const long long r = (long long)q * per_pass + team;
    const bool valid = r < a.R;
    int beg = 0, d = 0;
    if (valid) {
      beg = a.ro[r];
      d = a.ro[r + 1] - beg;
    }
    const bool mine = valid && d <= a.seg;                       // (a long row is the items' and the fold's)
    const int maxlen = wave_max(mine ? d : 0);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = mine && c < a.C;
      V acc;
      I win;
      aggb_win_walk<V, K>(a, beg, d, (long long)c * VW, on, maxlen, acc, win);
      if (on) *(I*)(a.win + r * a.ldw + (long long)c * VW) = win;
    }
  }
}

template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_aggb_win_items(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  typedef typename aggb_ivec<V>::type I;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.n_items + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  for (int q = wave; q < passes; q += waves) {
    const long long it = (long long)q * per_pass + team;
    const bool valid = it < a.n_items;
    int beg = 0, len = 0;
    if (valid) {
      const int2 item = a.items[it];
      const int b0 = a.ro[item.x];
      const int d = a.ro[item.x + 1] - b0;
      beg = b0 + item.y * a.seg;
      len = min(a.seg, d - item.y * a.seg);
    }
    const int maxlen = wave_max(len);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = valid && c < a.C;
      V acc;
      I win;
      aggb_win_walk<V, K>(a, beg, len, (long long)c * VW, on, maxlen, acc, win);
      if (on) {
        *(V*)(a.partials + it * a.ldp + (long long)c * VW) = acc;
        *(I*)(a.wparts + it * a.ldp + (long long)c * VW) = win;
      }
    }
  }
}

template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_aggb_win_fold(aggb_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  typedef typename aggb_ivec<V>::type I;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.n_long + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  for (int q = wave; q < passes; q += waves) {
    const long long k = (long long)q * per_pass + team;
    if (k >= a.n_long) continue;
    const int2 head = a.heads[k];
    const int d = a.ro[head.x + 1] - a.ro[head.x];
    const int segs = (d + a.seg - 1) / a.seg;
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      if (c >= a.C) continue;
      const long long at = (long long)head.y * a.ldp + (long long)c * VW;
      V acc = *(const V*)(a.partials + at);
      I win = *(const I*)(a.wparts + at);
      for (int s = 1; s < segs; ++s)
        aggb_take<K>(acc, win, *(const V*)(a.partials + at + (long long)s * a.ldp), *(const I*)(a.wparts + at + (long long)s * a.ldp));
      *(I*)(a.win + (long long)head.x * a.ldw + (long long)c * VW) = win;
    }
  }
}

// ---- the transpose ----
// entries [e0, e0 + E) of ci, columns in [0, T) (anything else is skipped: the C-ABI has checked x_rows against what the columns name)
__global__ __launch_bounds__(BLOCK) void k_aggb_tr_count(const int* ci, long long e0, long long E, int T, int* cnt) {
  const long long gthreads = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < E; i += gthreads) {
    const int c = ci[e0 + i];
    if (c >= 0 && c < T) atomicAdd(&cnt[c], 1);
  }
}
// every entry takes a slot of its column, in the order the adds land: the sort behind it puts every row into ascending e
__global__ __launch_bounds__(BLOCK) void k_aggb_tr_fill(const int* ci, long long e0, long long E, int T, const int* t_off, int* cur, int* t_pos) {
  const long long gthreads = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < E; i += gthreads) {
    const int c = ci[e0 + i];
    if (c < 0 || c >= T) continue;
    const long long slot = (long long)t_off[c] + atomicAdd(&cur[c], 1);
    if (slot < E) t_pos[slot] = (int)(e0 + i);
  }
}
// the forward row of every slot: the last row that starts at or before the slot's entry
__global__ __launch_bounds__(BLOCK) void k_aggb_tr_rows(const int* ro, int R, const int* t_pos, long long E, int* t_row) {
  const long long gthreads = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < E; i += gthreads) {
    const int e = t_pos[i];
    int lo = 0, hi = R - 1;
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (ro[mid + 1] <= e) lo = mid + 1;
      else hi = mid;
    }
    t_row[i] = lo;
  }
}

struct aggb_less_t {
  __device__ __forceinline__ bool operator()(int x, int y) const { return x < y; }
};

struct aggb_transpose_t {
  bool built = false;
  const int* built_for = nullptr;    // the forward offsets it was built from
  int T = 0;                         // and the x_rows
  long long E = 0, e0 = 0;
  mem_t<int> t_off, t_row, t_pos;
  size_t off_cap = 0, ent_cap = 0;
  agg_plan_t plan;                   // its long rows
};

struct aggb_request_t {
  const int* ro = nullptr;
  const int* ci = nullptr;
  const int* entry_pos = nullptr;
  const float* w = nullptr;
  const float* gy = nullptr;
  const float* x = nullptr;
  float* gx = nullptr;
  long long ldgy = 0, ldx = 0, ldgx = 0, entries = 0, e0 = 0;
  int R = 0, T = 0, feats = 0, op = 0, source = 0;
  bool needs_plan = true;            // of the FORWARD rows (a block whose sampling run had no fan-out of -1 has no long row)
};

// The device state of a handle's backward aggregation, and the run (host side).
struct aggb_state_t {
  int seg;
  agg_fused_state_t planner;                   // build_plan, its control words and its pinned word, as they are
  aggb_transpose_t tr[AGG_SOURCES];
  agg_plan_t fplans[AGG_SOURCES];              // the forward rows' long ones, for the winners
  const aggb_transpose_t* last_tr = nullptr;   // what the last run of either path ran on
  mem_t<int> cnt;
  size_t cnt_cap = 0;
  segsort_workspace_t<int, segsort_no_value_t> ws;
  mem_t<agg_control_t> ctl;
  mem_t<float> partials, gbuf;
  mem_t<int> wparts, win;
  size_t partials_cap = 0, gbuf_cap = 0, wparts_cap = 0, win_cap = 0;
  bool timing = false;
  double phase_ms[AGGB_PHASES] = {0.0, 0.0, 0.0, 0.0, 0.0};      // the last timed run: transpose, winners (or the mean's g), rows, items, fold
  std::vector<event_t> ev;
  size_t stamps = 0;

  explicit aggb_state_t(int seg_) : seg(seg_), planner(seg_) {}

  static void grow(mem_t<int>& m, size_t& cap, size_t want, context_t& ctx) {
    if (want <= cap) return;
    m = mem_t<int>();
    cap = 0;
    m = mem_t<int>(want, ctx);
    cap = want;
  }

  // the transposed CSR of entries [e0, e0 + E) under the offsets ro[0 .. R], and the plan of its long rows
  void build_transpose(aggb_transpose_t& t, const aggb_request_t& r, standard_context_t& ctx, long long& launches, long long& waits) {
    const hipStream_t st = ctx.stream();
    const int cap = std::max(ctx.num_cus, 1) * 8;
    const int T = r.T;
    const long long E = r.entries;
    t.built = false;
    grow(t.t_off, t.off_cap, (size_t)T + 1, ctx);
    if ((size_t)E > t.ent_cap) {
      size_t c0 = t.ent_cap, c1 = t.ent_cap;
      grow(t.t_row, c0, (size_t)E, ctx);
      grow(t.t_pos, c1, (size_t)E, ctx);
      t.ent_cap = (size_t)E;
    }
    t.plan.n_items = t.plan.n_long = 0;
    if (E == 0) {
      MGX_HIP(hipMemsetAsync(t.t_off.data(), 0, ((size_t)T + 1) * sizeof(int), st));
    } else {
      grow(cnt, cnt_cap, (size_t)T + 1, ctx);
      ctx.reserve_scratch(scan_scratch_bytes((long long)T + 1));
      if (E >= 2 && (E > ws.count_cap || T > ws.segs_cap)) {
        const long long c = std::max(E, ws.count_cap);
        const int s = std::max(T, ws.segs_cap);
        ws = segsort_workspace_t<int, segsort_no_value_t>();
        ws = segsort_workspace_t<int, segsort_no_value_t>(c, s, ctx);
      }
      int* const c = cnt.data();
      MGX_HIP(hipMemsetAsync(c, 0, ((size_t)T + 1) * sizeof(int), st));
      hipLaunchKernelGGL(k_aggb_tr_count, dim3(grid_for(E, BLOCK, cap)), dim3(BLOCK), 0, st, r.ci, r.e0, E, T, c);
      transform_scan([=] __device__(long long i) { return i < T ? c[i] : 0; }, (long long)T + 1, t.t_off.data(), ctx, nullptr);
      MGX_HIP(hipMemsetAsync(c, 0, ((size_t)T + 1) * sizeof(int), st));
      hipLaunchKernelGGL(k_aggb_tr_fill, dim3(grid_for(E, BLOCK, cap)), dim3(BLOCK), 0, st, r.ci, r.e0, E, T, (const int*)t.t_off.data(), c, t.t_pos.data());
      MGX_CHECK_LAUNCH("mgx aggbwd transpose");
      launches += 3;
      if (E >= 2) {
        const int passes = segmented_sort_impl<int, segsort_no_value_t>(t.t_pos.data(), nullptr, E, (const int*)t.t_off.data() + 1, T - 1, aggb_less_t(), ctx, &ws);
        launches += 4 + passes + (passes & 1);         // (the classification and the three bands, each counted as run, and the merge passes)
        ++waits;
      }
      hipLaunchKernelGGL(k_aggb_tr_rows, dim3(grid_for(E, BLOCK, cap)), dim3(BLOCK), 0, st, r.ro, r.R, (const int*)t.t_pos.data(), E, t.t_row.data());
      MGX_CHECK_LAUNCH("mgx aggbwd transpose rows");
      ++launches;
      planner.build_plan(t.plan, t.t_off.data(), T, ctx, launches, waits);
    }
    t.built = true;
    t.built_for = r.ro;
    t.T = T; t.E = E; t.e0 = r.e0;
  }

  // the transpose a request runs on, built where it is not kept; true: this call built it
  bool prepare(const aggb_request_t& r, standard_context_t& ctx, long long& launches, long long& waits) {
    aggb_transpose_t& t = tr[r.source];
    last_tr = &t;
    if (t.built && t.built_for == r.ro && t.T == r.T && t.E == r.entries && r.source != AGG_SRC_BLOCK) return false;
    build_transpose(t, r, ctx, launches, waits);
    return true;
  }

  int* ensure_win(int R, int feats, context_t& ctx) {
    grow(win, win_cap, (size_t)std::max(R, 1) * (size_t)(((long long)feats + 3) / 4 * 4), ctx);
    return win.data();
  }
  void ensure_partials(size_t want, bool winners, context_t& ctx) {
    if (want > partials_cap) {
      partials = mem_t<float>();
      partials_cap = 0;
      partials = mem_t<float>(want, ctx);
      partials_cap = want;
    }
    if (winners) grow(wparts, wparts_cap, want, ctx);
  }

  template <typename V, int K>
  void launch_winners(const aggb_args_t& a, standard_context_t& ctx, long long& launches) {
    const hipStream_t st = ctx.stream();
    const int cap = std::max(ctx.num_cus, 1) * 8;
    const int per_pass = WAVE / a.G;
    hipLaunchKernelGGL((k_aggb_win_rows<V, K>), dim3(grid_for(((long long)a.R + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
    ++launches;
    if (a.n_items > 0) {
      hipLaunchKernelGGL((k_aggb_win_items<V, K>), dim3(grid_for(((long long)a.n_items + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL((k_aggb_win_fold<V, K>), dim3(grid_for(((long long)a.n_long + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      launches += 2;
    }
  }

  template <typename V, int K>
  void launch(const aggb_args_t& a, standard_context_t& ctx, long long& launches, size_t& stamp) {
    const hipStream_t st = ctx.stream();
    const int cap = std::max(ctx.num_cus, 1) * 8;
    const int per_pass = WAVE / a.G;
    auto mark_time = [&]() { if (timing) MGX_HIP(hipEventRecord(ev[stamp++], st)); };
    hipLaunchKernelGGL((k_aggb_rows<V, K>), dim3(grid_for(((long long)a.T + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
    ++launches;
    mark_time();
    if (a.n_items > 0) {
      hipLaunchKernelGGL((k_aggb_items<V, K>), dim3(grid_for(((long long)a.n_items + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      mark_time();
      hipLaunchKernelGGL((k_aggb_fold<V>), dim3(grid_for(((long long)a.n_long + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      mark_time();
      launches += 2;
    }
  }
  template <typename V>
  void launch_op(const aggb_args_t& a, standard_context_t& ctx, long long& launches, size_t& stamp) {
    if (a.op == AGG_MAX || a.op == AGG_MIN) launch<V, AGGB_K_WIN>(a, ctx, launches, stamp);
    else launch<V, AGGB_K_SUM>(a, ctx, launches, stamp);
  }

  // Only enqueues, but for the waits of a run that builds a transpose or a plan.  Returns the ten stats of mgx_aggbwd_run.
  std::vector<long long> run(const aggb_request_t& r, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    long long launches = 0, waits = 0;
    for (double& p : phase_ms) p = 0.0;
    stamps = 0;
    const bool minmax = r.op == AGG_MAX || r.op == AGG_MIN;
    const agg_shape_t sh = agg_shape(r.feats, agg_vector_ok(r.gy, r.ldgy, r.gx, r.ldgx, r.feats));
    if (ctl.size() == 0) ctl = mem_t<agg_control_t>(1, ctx);
    MGX_HIP(hipMemsetAsync(ctl.data(), 0, sizeof(agg_control_t), st));
    bool built = false;
    last_tr = nullptr;
    if (r.T > 0) {
      if (timing) while (ev.size() < AGGB_PHASES + 1) ev.emplace_back();
      size_t stamp = 0;
      auto mark_time = [&]() { if (timing) MGX_HIP(hipEventRecord(ev[stamp++], st)); };
      mark_time();
      built = prepare(r, ctx, launches, waits);
      const aggb_transpose_t& t = tr[r.source];
      mark_time();
      aggb_args_t a;
      a.t_off = t.t_off.data(); a.t_row = t.t_row.data(); a.t_pos = t.t_pos.data();
      a.ro = r.ro; a.ci = r.ci; a.entry_pos = r.w ? r.entry_pos : nullptr; a.w = r.w; a.gy = r.gy; a.x = r.x; a.gx = r.gx;
      a.win = nullptr; a.wparts = nullptr; a.g = nullptr; a.ctl = ctl.data();
      a.ldgy = r.ldgy; a.ldx = r.ldx; a.ldgx = r.ldgx; a.ldp = ((long long)r.feats + 3) / 4 * 4; a.ldw = (int)a.ldp;
      a.R = r.R; a.T = r.T; a.op = r.op; a.seg = seg;
      if (minmax && r.R > 0) {
        agg_plan_t& fp = fplans[r.source];
        if (!r.needs_plan) { fp.n_items = fp.n_long = 0; fp.built = false; }
        else if (!fp.built || fp.built_for != r.ro || r.source == AGG_SRC_BLOCK) planner.build_plan(fp, r.ro, r.R, ctx, launches, waits);
        a.win = ensure_win(r.R, r.feats, ctx);
        ensure_partials((size_t)std::max(fp.n_items, t.plan.n_items) * (size_t)a.ldp, true, ctx);
        a.partials = partials.data(); a.wparts = wparts.data();
        aggb_args_t f = a;
        const agg_shape_t fs = agg_shape(r.feats, agg_vector_ok(r.x, r.ldx, a.win, a.ldw, r.feats));
        f.C = fs.C; f.G = fs.G; f.tiles = fs.tiles;
        f.items = fp.items.data(); f.heads = fp.heads.data(); f.n_items = (int)fp.n_items; f.n_long = (int)fp.n_long;
        if (fs.vector) { if (r.op == AGG_MAX) launch_winners<float4, AGG_K_MAX>(f, ctx, launches); else launch_winners<float4, AGG_K_MIN>(f, ctx, launches); }
        else { if (r.op == AGG_MAX) launch_winners<float, AGG_K_MAX>(f, ctx, launches); else launch_winners<float, AGG_K_MIN>(f, ctx, launches); }
      } else {
        ensure_partials((size_t)t.plan.n_items * (size_t)a.ldp, false, ctx);
        a.partials = partials.data();
      }
      a.C = sh.C; a.G = sh.G; a.tiles = sh.tiles;
      if (r.op == AGG_MEAN && r.R > 0) {
        const size_t want = (size_t)r.R * (size_t)a.ldp;
        if (want > gbuf_cap) {
          gbuf = mem_t<float>();
          gbuf_cap = 0;
          gbuf = mem_t<float>(want, ctx);
          gbuf_cap = want;
        }
        a.g = gbuf.data();
        const int grid = grid_for((long long)r.R * a.C, BLOCK, std::max(ctx.num_cus, 1) * 8);
        if (sh.vector) hipLaunchKernelGGL((k_aggb_scale<float4>), dim3(grid), dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_aggb_scale<float>), dim3(grid), dim3(BLOCK), 0, st, a);
        ++launches;
        a.gy = a.g; a.ldgy = a.ldp;                            // (the walk reads g; the gate stays the caller's arrays')
      }
      mark_time();
      a.items = t.plan.items.data(); a.heads = t.plan.heads.data(); a.n_items = (int)t.plan.n_items; a.n_long = (int)t.plan.n_long;
      if (sh.vector) launch_op<float4>(a, ctx, launches, stamp);
      else launch_op<float>(a, ctx, launches, stamp);
      MGX_CHECK_LAUNCH("mgx aggbwd run");
      stamps = stamp;
    }
    return {r.T, r.entries, r.feats, sh.G, sh.tiles, sh.vector, seg, launches, waits, built ? 1 : 0};
  }

  // ms of the last timed run's transpose, winners, rows, items and fold (waits for the last of them)
  void read_phases(double* out) {
    if (stamps) {
      MGX_HIP(hipEventSynchronize(ev[stamps - 1]));
      for (size_t i = 0; i + 1 < stamps; ++i) {
        float ms = 0.f;
        MGX_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        phase_ms[i] = ms;
      }
      stamps = 0;
    }
    for (int i = 0; i < AGGB_PHASES; ++i) out[i] = phase_ms[i];
  }

  // the last run's transposed rows by class (waits): none, a team's, long, the long rows' segments, seg
  void bins(long long* out, standard_context_t& ctx) {
    planner.h_ctl.fetch(ctl.data(), 1, ctx.stream());
    const pinned_t<agg_control_t>& h = planner.h_ctl;
    out[0] = h->bins[ROW_NONE]; out[1] = h->bins[ROW_LANE]; out[2] = h->bins[ROW_LONG]; out[3] = h->segments; out[4] = seg;
  }
};

}  // namespace mgx
