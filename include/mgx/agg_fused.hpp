// mgx/agg_fused.hpp -- neighbour feature aggregation for GNN layers, fused (mgx_agg_run): for every row of a CSR the reduction of
// its neighbours' FEATURE ROWS, Y[r, :] = (+)_{e in row r} w_e X[col_e, :], in a fixed order of arithmetic -- the memory-bound step
// of a GraphSAGE / GCN layer, over the graph's out-rows, its in-rows (the CSC) or the blocks of a neighbour-sampling run.
//
// The definition (the operator path include/gunrock/agg/ and tests/agg_model.py compute the same float32 bits).
//   term     t_e = X[col_e, f], or w_e * X[col_e, f] rounded once to float32: the multiply and the add are never fused (every function
//            below that does arithmetic says `#pragma clang fp contract(off)`: without it the compiler emits v_fmac_f32)
//   order    a row's entries are cut into segments of `seg` entries in STORED order.  Within a segment acc = t_0, then acc = acc (+)
//            t_j for j = 1, 2, ..; the row's value is the segments' values combined the same way, in segment order.  (+) is float32
//            + for sum and mean, t > acc ? t : acc for max, t < acc ? t : acc for min -- written out so, which fixes +-0 and NaN
//   mean     the sum divided by float(d), one correctly rounded division.  A row without entries gives 0.0 for every op.  Every
//            element of Y[:R, :F] is written on every run, the padding columns F .. ldy - 1 never.
// Lane-columns: with F, ldx and ldy multiples of 4 and both bases 16-byte aligned a lane owns 4 consecutive columns (one 16-byte
// load per entry), C = F / 4 lane-columns; otherwise one column a lane, C = F.  A TEAM of G lanes of one wave, G the smallest power
// of two >= min(C, AGG_TILE), takes a row: a wave runs 64 / G rows at a time, and with C > AGG_TILE the team walks its row once per
// tile of AGG_TILE lane-columns.  The team's lanes load the same cols[e] (and w_e, through entry_pos[e] for a block), then their
// pieces of X[col_e]: one contiguous read of the feature row.  The loads of AGG_UNROLL entries are issued before the first add; the
// adds are in stored order.  All 64 lanes stay in the loop: teams whose row is shorter, empty or past the end ride along predicated.
// No LDS, no scratch, no atomics on Y.
// The launches:
//   k_agg_rows        a team per row: rows of at most seg entries, zeros for the rows without entries; counts the rows by class
//   k_agg_items       a team per (row, segment) item of the longer rows -> partials[item]
//   k_agg_fold        a team per long row (the plan lists every long row with its first item; a row's items are consecutive): the
//                     partials in segment order, the division for mean, Y[row]
//   the plan          k_agg_plan_count (the long rows and their segments), one host wait, k_agg_plan_fill (the items as
//                     worklist.hpp's wave_append_segments writes them, and the long rows' heads behind the same add).  It depends on the CSR and seg alone, not on F, op or weights: for the graph's out- and
//                     in-rows it is built by the first run that uses them and kept for the handle's life; for a block it is needed
//                     only when the sampling run had a fan-out of -1 (else every row has <= 64 <= seg entries: ONE launch, no wait),
//                     and is then rebuilt every run.
// Grids are sized by bounds and capped at 8 workgroups a compute unit.
// The backward (the gradient with respect to X, over the transposed rows) is agg_backward.hpp; it shares the arithmetic,
// the shape and the plan kernels below as they are.
// Not built: fp16 / bf16 features, several blocks per launch, features fused with the sampler's gather
// X[vertices], more than one device, MFMA (there is no dense weight matrix here).
#pragma once
#include <algorithm>
#include <vector>

#include "env.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (seg's default won its sweep on R-MAT-20; the unroll and the grids' cap are unmeasured guesses; tests/agg_model.py
// mirrors the constants)
constexpr int AGG_SEG_DEFAULT = 256;
constexpr int AGG_SEG_MIN = 64;
constexpr int AGG_SEG_MAX = 4096;
constexpr int AGG_UNROLL = 8;          // entries whose loads are in flight before the first add
constexpr int AGG_TILE = WAVE;         // lane-columns a team walks at a time
constexpr int AGG_MAX_FEATS = 65536;
enum : int { AGG_SUM = 0, AGG_MEAN = 1, AGG_MAX = 2, AGG_MIN = 3, AGG_OPS = 4 };
enum : int { AGG_SRC_OUT = 0, AGG_SRC_IN = 1, AGG_SRC_BLOCK = 2, AGG_SOURCES = 3 };
enum : int { AGG_K_ADD = 0, AGG_K_MAX = 1, AGG_K_MIN = 2 };          // the combine a kernel is compiled for (sum and mean share one)
enum : int { AGG_STATS = 9, AGG_BINS = 5 };

// MGX_AGG_SEG: the smallest power of two in 64 .. 4096 that is >= the value
inline int agg_seg_from_env() {
  const char* e = env("MGX_AGG_SEG");
  if (!e) return AGG_SEG_DEFAULT;
  const long long v = std::strtoll(e, nullptr, 10);
  int s = AGG_SEG_MIN;
  while (s < AGG_SEG_MAX && s < v) s *= 2;
  return s;
}

// lane-columns, team width and column tiles of a run
struct agg_shape_t {
  int vector, C, G, tiles;
};
inline agg_shape_t agg_shape(int feats, bool vector) {
  agg_shape_t s;
  s.vector = vector ? 1 : 0;
  s.C = vector ? feats / 4 : feats;
  s.G = 1;
  while (s.G < std::min(s.C, AGG_TILE)) s.G *= 2;
  s.tiles = (s.C + AGG_TILE - 1) / AGG_TILE;
  return s;
}
inline bool agg_vector_ok(const void* x, long long ldx, const void* y, long long ldy, int feats) {
  return feats % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
}

// ---- the arithmetic both paths share: never contracted ----
template <int K>
__device__ __forceinline__ float agg_comb(float acc, float t) {
#pragma clang fp contract(off)
  if (K == AGG_K_MAX) return t > acc ? t : acc;
  if (K == AGG_K_MIN) return t < acc ? t : acc;
  return acc + t;
}
template <int K>
__device__ __forceinline__ float4 agg_comb(float4 acc, float4 t) {
  return make_float4(agg_comb<K>(acc.x, t.x), agg_comb<K>(acc.y, t.y), agg_comb<K>(acc.z, t.z), agg_comb<K>(acc.w, t.w));
}
__device__ __forceinline__ float agg_term(float w, float x) {
#pragma clang fp contract(off)
  const float t = w * x;
  return t;
}
__device__ __forceinline__ float4 agg_term(float w, float4 x) { return make_float4(agg_term(w, x.x), agg_term(w, x.y), agg_term(w, x.z), agg_term(w, x.w)); }
__device__ __forceinline__ float agg_div(float s, float d) {
#pragma clang fp contract(off)
  const float q = s / d;
  return q;
}
__device__ __forceinline__ float4 agg_div(float4 s, float d) { return make_float4(agg_div(s.x, d), agg_div(s.y, d), agg_div(s.z, d), agg_div(s.w, d)); }
// the combine by its run-time name (the operator path, whose one functor serves every op)
__device__ __forceinline__ float agg_comb_op(int op, float acc, float t) {
  return op == AGG_MAX ? agg_comb<AGG_K_MAX>(acc, t) : (op == AGG_MIN ? agg_comb<AGG_K_MIN>(acc, t) : agg_comb<AGG_K_ADD>(acc, t));
}

template <typename V> struct agg_vec;
template <> struct agg_vec<float> {
  static constexpr int width = 1;
  static __device__ __forceinline__ float zero() { return 0.f; }
};
template <> struct agg_vec<float4> {
  static constexpr int width = 4;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};

// the plan's and a run's words in device memory
struct agg_control_t {
  int n_items;           // the long rows' segments (k_agg_plan_count)
  int n_long;
  int fill;              // k_agg_plan_fill's counters: the items written,
  int heads;             // the long rows listed
  long long bins[4];     // a run's rows by class: ROW_NONE, ROW_LANE (a team's), ROW_WAVE (none), ROW_LONG
  long long segments;
};

struct agg_args_t {
  const int* ro;         // R + 1 offsets, absolute places in ci (a block's hop starts where the hop before ends)
  const int* ci;
  const int* entry_pos;  // a block's: the place of entry e in the graph's weights (NULL: e itself)
  const float* w;        // NULL: unweighted
  const float* x;
  float* y;
  float* partials;       // n_items x ldp
  const int2* items;
  const int2* heads;     // n_long x (row, its first item)
  agg_control_t* ctl;
  long long ldx, ldy, ldp;
  int R, C, G, tiles, op, seg, n_items, n_long;
};

// One walk for both kinds of work: entries [beg, beg + len) of one row (a row of at most seg entries, or one segment), the
// lane's piece of every X[col_e] at float offset `coff`, folded in stored order.  maxlen is the longest len in the wave: every lane
// runs the same trips, its loads and adds predicated by `on` and its own len.
template <typename V, int K>
__device__ __forceinline__ V agg_walk(const agg_args_t& a, int beg, int len, long long coff, bool on, int maxlen) {
  V acc = agg_vec<V>::zero();
  const int mine = on ? len : 0;
  for (int base = 0; base < maxlen; base += AGG_UNROLL) {
    // three rounds of loads, none of which waits for one of its own round: the columns (and the weights' places), the weights,
    // the pieces of the feature rows
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
        acc = base + u == 0 ? t : agg_comb<K>(acc, t);
      }
    }
  }
  return acc;
}

// a team per row; a wave takes 64 / G rows a pass
template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_agg_rows(agg_args_t a) {
  constexpr int VW = agg_vec<V>::width;
  const int lane = lane_id();
  const int G = a.G, per_pass = WAVE / G;
  const int j = lane & (G - 1), team = lane / G;
  const int passes = (int)(((long long)a.R + per_pass - 1) / per_pass);
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  const row_cuts_t cuts = {a.seg, a.seg, a.seg};
  row_bins_t bins;
  long long segs = 0;
  for (int q = wave; q < passes; q += waves) {
    const long long r = (long long)q * per_pass + team;          // (64 bits: R may be close to 2^31)
    const bool valid = r < a.R;
    int beg = 0, d = 0;
    if (valid) {
      beg = a.ro[r];
      d = a.ro[r + 1] - beg;
    }
    const int body = valid ? cuts.body_of(d) : -1;
    bins.count(j == 0 ? body : -1);
    if (j == 0 && body == ROW_LONG) segs += cuts.segments_of(d);
    const bool mine = valid && body != ROW_LONG;                 // (a long row is the items' and the fold's)
    const int maxlen = wave_max(mine ? d : 0);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = mine && c < a.C;
      V acc = agg_walk<V, K>(a, beg, d, (long long)c * VW, on, maxlen);
      if (on) {
        if (a.op == AGG_MEAN && d > 0) acc = agg_div(acc, (float)d);
        *(V*)(a.y + r * a.ldy + (long long)c * VW) = acc;
      }
    }
  }
  bins.add_to(a.ctl->bins);
  segs = wave_sum(segs);
  if (lane == 0 && segs) atomicAdd((u64*)&a.ctl->segments, (u64)segs);
}

// a team per (row, segment) item of the long rows
template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_agg_items(agg_args_t a) {
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
      const int b0 = a.ro[item.x];
      const int d = a.ro[item.x + 1] - b0;
      beg = b0 + item.y * a.seg;
      len = min(a.seg, d - item.y * a.seg);
    }
    const int maxlen = wave_max(len);
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      const bool on = valid && c < a.C;
      const V acc = agg_walk<V, K>(a, beg, len, (long long)c * VW, on, maxlen);
      if (on) *(V*)(a.partials + it * a.ldp + (long long)c * VW) = acc;
    }
  }
}

// a team per long row (heads: the row and its first item; a row's items are consecutive) adds the row's partials in segment order
template <typename V, int K>
__global__ __launch_bounds__(BLOCK) void k_agg_fold(agg_args_t a) {
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
    const int d = a.ro[head.x + 1] - a.ro[head.x];
    const int segs = (d + a.seg - 1) / a.seg;
    for (int t = 0; t < a.tiles; ++t) {
      const int c = t * AGG_TILE + j;
      if (c >= a.C) continue;
      const float* const p = a.partials + (long long)head.y * a.ldp + (long long)c * VW;
      V acc = *(const V*)p;
      for (int s = 1; s < segs; ++s) acc = agg_comb<K>(acc, *(const V*)(p + (long long)s * a.ldp));
      if (a.op == AGG_MEAN) acc = agg_div(acc, (float)d);
      *(V*)(a.y + (long long)head.x * a.ldy + (long long)c * VW) = acc;
    }
  }
}

// the plan: the long rows' segments, then the items
__global__ __launch_bounds__(BLOCK) void k_agg_plan_count(const int* ro, int R, int seg, agg_control_t* ctl) {
  const row_cuts_t cuts = {seg, seg, seg};
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  int items = 0, rows = 0;
  for (unsigned r = blockIdx.x * (unsigned)BLOCK + threadIdx.x; r < (unsigned)R; r += gthreads) {
    const int d = ro[r + 1] - ro[r];
    if (cuts.body_of(d) == ROW_LONG) { items += cuts.segments_of(d); ++rows; }
  }
  items = wave_sum(items);
  rows = wave_sum(rows);
  if (lane_id() == 0 && rows) {
    atomicAdd(&ctl->n_items, items);
    atomicAdd(&ctl->n_long, rows);
  }
}
// wave_append_segments (worklist.hpp) with one thing more: the fold wants every long row's first item, which only the append knows,
// so the same add's base also goes to heads[k] = (row, first item), k from a second counter.  All 64 lanes call.
__global__ __launch_bounds__(BLOCK) void k_agg_plan_fill(const int* ro, int R, int seg, int2* items, int2* heads, agg_control_t* ctl) {
  const row_cuts_t cuts = {seg, seg, seg};
  const long long gthreads = (long long)gridDim.x * BLOCK;
  const int lane = lane_id();
  for (long long base = (long long)blockIdx.x * BLOCK + threadIdx.x - lane; base < R; base += gthreads) {
    const long long r = base + lane;
    const int d = r < R ? ro[r + 1] - ro[r] : 0;
    const bool keep = cuts.body_of(d) == ROW_LONG;
    const u64 m = __ballot(keep);
    if (!m) continue;
    const int segs = keep ? cuts.segments_of(d) : 0;
    const int incl = wave_inclusive_sum(segs);
    int first = 0, hbase = 0;
    if (lane == WAVE - 1) {
      first = atomicAdd(&ctl->fill, incl);
      hbase = atomicAdd(&ctl->heads, __popcll(m));
    }
    first = __shfl(first, WAVE - 1, WAVE) + incl - segs;
    hbase = __shfl(hbase, WAVE - 1, WAVE);
    if (keep) {
      for (int s = 0; s < segs; ++s) items[first + s] = make_int2((int)r, s);
      heads[hbase + rank_in_mask(m)] = make_int2((int)r, first);
    }
  }
}

// which rows of a CSR are long, as (row, segment) items
struct agg_plan_t {
  bool built = false;
  const int* built_for = nullptr;    // the offsets it was built from (a CSC built later has others)
  long long n_items = 0, n_long = 0;
  mem_t<int2> items, heads;
  size_t items_cap = 0, heads_cap = 0;
};

// The device state of a handle's fused aggregation, and the run (host side).
struct agg_request_t {
  const int* ro = nullptr;
  const int* ci = nullptr;
  const int* entry_pos = nullptr;
  const float* w = nullptr;
  const float* x = nullptr;
  float* y = nullptr;
  long long ldx = 0, ldy = 0, entries = 0;
  int R = 0, feats = 0, op = 0, source = 0;
  bool needs_plan = true;            // (a block whose sampling run had no fan-out of -1 has no long row)
};

struct agg_fused_state_t {
  int seg;
  agg_plan_t plans[AGG_SOURCES];
  mem_t<agg_control_t> ctl, pctl;
  pinned_t<agg_control_t> h_ctl;
  mem_t<float> partials;
  size_t partials_cap = 0;
  bool timing = false;
  double phase_ms[3] = {0.0, 0.0, 0.0};        // the last timed run: rows, items, fold
  std::vector<event_t> ev;
  size_t stamps = 0;                           // events the last timed run recorded and nobody has read yet

  explicit agg_fused_state_t(int seg_) : seg(seg_) { h_ctl = pinned_t<agg_control_t>(1); }

  void build_plan(agg_plan_t& p, const int* ro, int R, standard_context_t& ctx, long long& launches, long long& waits) {
    const hipStream_t st = ctx.stream();
    const int cap = std::max(ctx.num_cus, 1) * 8;
    if (pctl.size() == 0) pctl = mem_t<agg_control_t>(1, ctx);
    MGX_HIP(hipMemsetAsync(pctl.data(), 0, sizeof(agg_control_t), st));
    hipLaunchKernelGGL(k_agg_plan_count, dim3(grid_for(R, BLOCK, cap)), dim3(BLOCK), 0, st, ro, R, seg, pctl.data());
    MGX_CHECK_LAUNCH("mgx agg plan");
    h_ctl.fetch(pctl.data(), 1, st);
    p.n_items = h_ctl->n_items;
    p.n_long = h_ctl->n_long;
    if ((size_t)p.n_items > p.items_cap) {
      p.items = mem_t<int2>();
      p.items_cap = 0;
      p.items = mem_t<int2>((size_t)p.n_items, ctx);
      p.items_cap = (size_t)p.n_items;
    }
    if ((size_t)p.n_long > p.heads_cap) {
      p.heads = mem_t<int2>();
      p.heads_cap = 0;
      p.heads = mem_t<int2>((size_t)p.n_long, ctx);
      p.heads_cap = (size_t)p.n_long;
    }
    hipLaunchKernelGGL(k_agg_plan_fill, dim3(grid_for(R, BLOCK, cap)), dim3(BLOCK), 0, st, ro, R, seg, p.items.data(), p.heads.data(), pctl.data());
    p.built = true;
    p.built_for = ro;
    launches += 2;
    ++waits;
  }

  template <typename V, int K>
  void launch(const agg_args_t& a, bool items, standard_context_t& ctx, long long& launches, size_t& stamp) {
    const hipStream_t st = ctx.stream();
    const int cap = std::max(ctx.num_cus, 1) * 8;
    const int per_pass = WAVE / a.G;
    auto mark_time = [&]() { if (timing) MGX_HIP(hipEventRecord(ev[stamp++], st)); };
    mark_time();
    hipLaunchKernelGGL((k_agg_rows<V, K>), dim3(grid_for(((long long)a.R + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
    ++launches;
    mark_time();
    if (items) {
      const int grid = grid_for(((long long)a.n_items + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap);
      hipLaunchKernelGGL((k_agg_items<V, K>), dim3(grid), dim3(BLOCK), 0, st, a);
      mark_time();
      hipLaunchKernelGGL((k_agg_fold<V, K>), dim3(grid_for(((long long)a.n_long + per_pass - 1) / per_pass, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      mark_time();
      launches += 2;
    }
  }
  template <typename V>
  void launch_op(const agg_args_t& a, bool items, standard_context_t& ctx, long long& launches, size_t& stamp) {
    if (a.op == AGG_MAX) launch<V, AGG_K_MAX>(a, items, ctx, launches, stamp);
    else if (a.op == AGG_MIN) launch<V, AGG_K_MIN>(a, items, ctx, launches, stamp);
    else launch<V, AGG_K_ADD>(a, items, ctx, launches, stamp);
  }

  // Only enqueues (but for the wait of a run that builds a plan).  Returns the nine stats of mgx_agg_run.
  std::vector<long long> run(const agg_request_t& r, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    long long launches = 0, waits = 0;
    phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.0;
    stamps = 0;
    const agg_shape_t sh = agg_shape(r.feats, agg_vector_ok(r.x, r.ldx, r.y, r.ldy, r.feats));
    if (ctl.size() == 0) ctl = mem_t<agg_control_t>(1, ctx);
    MGX_HIP(hipMemsetAsync(ctl.data(), 0, sizeof(agg_control_t), st));
    if (r.R > 0) {
      agg_plan_t& plan = plans[r.source];
      if (!r.needs_plan) { plan.n_items = plan.n_long = 0; plan.built = false; }
      else if (!plan.built || plan.built_for != r.ro || r.source == AGG_SRC_BLOCK) build_plan(plan, r.ro, r.R, ctx, launches, waits);
      agg_args_t a;
      a.ro = r.ro; a.ci = r.ci; a.entry_pos = r.w ? r.entry_pos : nullptr; a.w = r.w; a.x = r.x; a.y = r.y;
      a.items = plan.items.data(); a.heads = plan.heads.data(); a.ctl = ctl.data();
      a.ldx = r.ldx; a.ldy = r.ldy; a.ldp = ((long long)r.feats + 3) / 4 * 4;
      a.R = r.R; a.C = sh.C; a.G = sh.G; a.tiles = sh.tiles; a.op = r.op; a.seg = seg; a.n_items = (int)plan.n_items; a.n_long = (int)plan.n_long;
      const size_t want = (size_t)plan.n_items * (size_t)a.ldp;
      if (want > partials_cap) {
        partials = mem_t<float>();
        partials_cap = 0;
        partials = mem_t<float>(want, ctx);
        partials_cap = want;
      }
      a.partials = partials.data();
      if (timing) while (ev.size() < 4) ev.emplace_back();
      size_t stamp = 0;
      if (sh.vector) launch_op<float4>(a, plan.n_items > 0, ctx, launches, stamp);
      else launch_op<float>(a, plan.n_items > 0, ctx, launches, stamp);
      MGX_CHECK_LAUNCH("mgx agg run");
      stamps = stamp;
    }
    return {r.R, r.entries, r.feats, sh.G, sh.tiles, sh.vector, seg, launches, waits};
  }

  // ms of the last timed run's rows, items and fold launches (waits for the last of them: the run itself only enqueues)
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
    out[0] = phase_ms[0]; out[1] = phase_ms[1]; out[2] = phase_ms[2];
  }

  // the last run's rows by class (waits): none, a team's, long, the long rows' segments, seg
  void bins(long long* out, standard_context_t& ctx) {
    h_ctl.fetch(ctl.data(), 1, ctx.stream());
    out[0] = h_ctl->bins[ROW_NONE]; out[1] = h_ctl->bins[ROW_LANE]; out[2] = h_ctl->bins[ROW_LONG]; out[3] = h_ctl->segments; out[4] = seg;
  }
};

}  // namespace mgx
