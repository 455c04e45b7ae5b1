// mgx/rw_fused.hpp -- random walks and node2vec sampling, fused (mgx_rw_run): one launch runs every walker of a run from its first
// step to its last, a lane per walker, the walk's state in registers.  The draws are counter-based, a pure function of (seed,
// walker, step, draw), so that a walker's path depends on nothing but the graph and its own number.
//
// The definition (the operator path include/gunrock/rw/ and tests/rw_model.py compute the same, bit for bit).
//   walkers    walker w of [0, S R) starts at starts[w / R] (starts == NULL: at vertex w / R); its path has L + 1 slots, slot 0 the
//              start, -1 behind the walk's end.
//   draw       draw(seed, w, t, k) = fmix32(fmix32(fmix32(seed + 0x9E3779B9 (w + 1)) ^ 0x85EBCA6B (t + 1)) ^ 0xC2B2AE35 (k + 1)),
//              fmix32 = color_fmix32; u(r) = float(r >> 8) 2^-24 in [0, 1), exact; a row position is umulhi(r, d) (a position's
//              probability is off 1 / d by at most 2^-32, a row's total bias at most d / 2^32).
//   step t     from cur, prev the vertex before it or none:
//              1. restart > 0 and u(draw(k = 0)) < restart: to the walker's start, prev = none; a step and a restart.
//              2. else d = cur's out-degree; the row is dead when d == 0, or when the run is weighted and wmax[cur] <= 0.  A dead
//                 row ends the walk (a dead end) when restart == 0 and jumps to the start as in 1 when restart > 0.
//              3. else tries i = 0 .. T - 1: j = umulhi(draw(k = 1 + 2 i), d), c = col[off + j] (the STORED order), a = u(draw(k
//                 = 2 + 2 i)); accepted iff a * (wmax[cur] * M) < w[off + j] * b, every product one float32 multiply.  Unweighted:
//                 w = wmax = 1.  First order (p == q == 1, or prev is none): b = M = 1.  Second order: b = ip when c == prev, 1
//                 when the entry prev -> c exists, iq otherwise; M = max(ip, 1, iq); ip = 1.0f / p and iq = 1.0f / q come from the
//                 host.  The unweighted first-order step takes try 0 and draws no a.
//              4. after T rejections the row's first maximum-weight entry, position amax[cur]: a fallback.  The sampled
//                 distribution is the intended one exactly where fallbacks == 0; the expected tries per step are
//                 wmax M / mean(w b).
//   setup      per handle, when the mode needs what is missing (k_rw_setup, then k_rw_setup_long for the segmented rows): wm[v] =
//              (the bits of wmax[v]) << 32 | (2^32 - 1 - amax[v]), one 64-bit maximum per row whatever the order of its parts: rows
//              of at most short_max entries a lane each, of at most wave_max a wave, longer ones as (vertex, segment) items; a
//              negative or NaN weight raises a flag (MGX_E_NEGATIVE_WEIGHT).  Second order: a flag when any row is not ascending;
//              then the membership search runs on a sorted copy of col_indices (segsort.hpp), the picks still index the stored
//              order.
//   results    paths int32[W][L + 1] on request, ends and lengths int32[W], visits int64[n] on request (the path slots >= 0 that
//              hold v, slot 0 included; 64-bit integer atomic adds: exact whatever the order), five exact counters.
// k_rw_walk<WEIGHTED, SECOND>: a grid-stride loop over workgroup-sized blocks of walkers.  What decides its speed:
//   the path store   a lane that stored slot t of its own walker would write 4 bytes at a stride of 4 (L + 1): 64 cache lines a
//              wave instruction.  Instead the workgroup keeps `tile` slots of its 256 walkers in LDS ([slot][walker], the row
//              padded by one word) and flushes the tile transposed: consecutive lanes write consecutive slots of one walker, 4
//              tile bytes at a time (64 at the default of 16).  The -1 padding goes the same way.  Without paths there is no tile
//              and no barrier: a wave whose walkers are all over goes on to the next block.
//   latency    a step is a chain of dependent gathers: both offsets of cur and wm[cur] are read back to back, then the candidate
//              (and its weight), then -- second order -- a branch-light binary search over prev's row.  Nothing overlaps inside
//              a walker; the lever is waves in flight, so the kernels keep out of scratch (DESIGN 3.17 has their registers).
// Not built: alias tables or an exact inverse-CDF fallback, more than one device, walkers re-sorted by vertex per
// step, metapaths.  (Sampling without replacement / k-hop fan-out: nsample_fused.hpp)
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "color_hash.hpp"
#include "env.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "segsort.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (the three cuts are unmeasured guesses; tools/rw_bench.py measures TILE)
constexpr int RW_TRIES_DEFAULT = 64;
constexpr int RW_TILE_DEFAULT = 16;
constexpr int RW_TILE_MAX = 64;
constexpr int RW_SHORT_MAX_DEFAULT = 32;
constexpr int RW_WAVE_MAX_DEFAULT = 1024;
constexpr int RW_SEG_DEFAULT = 1024;
constexpr int RW_CUT_MAX = 1 << 20;
constexpr int RW_TRIES_MAX = 1 << 20;
constexpr int RW_TILE_PITCH = BLOCK + 1;        // words of a tile's row: the flush's lanes read down a column
enum : int { RW_C_STEPS = 0, RW_C_DEAD = 1, RW_C_RESTARTS = 2, RW_C_TRIES = 3, RW_C_FALLBACKS = 4, RW_COUNTERS = 5 };
enum : int { RW_BINS = 5 };                     // rows without entries, a lane's, a wave's, segmented, their segments
enum : unsigned { RW_FLAG_NEGATIVE = 1u, RW_FLAG_UNSORTED = 2u };

struct rw_opts_t {
  int tries = RW_TRIES_DEFAULT, tile = RW_TILE_DEFAULT;
  row_cuts_t cuts = {RW_SHORT_MAX_DEFAULT, RW_WAVE_MAX_DEFAULT, RW_SEG_DEFAULT};
  static rw_opts_t from_env() {
    rw_opts_t o;
    o.tries = env_int("MGX_RW_TRIES", 1, RW_TRIES_MAX, o.tries);
    if (const char* e = env("MGX_RW_TILE")) {
      const int want = std::min(std::max(atoi(e), 1), RW_TILE_MAX);
      o.tile = 1;
      while (o.tile * 2 <= want) o.tile *= 2;                // (the power of two at or below)
    }
    o.cuts.short_max = env_int("MGX_RW_SHORT_MAX", 0, RW_CUT_MAX, o.cuts.short_max);
    o.cuts.wave_max = env_int("MGX_RW_WAVE_MAX", 0, RW_CUT_MAX, o.cuts.wave_max);
    o.cuts.seg = env_int("MGX_RW_SEG", 1, RW_CUT_MAX, o.cuts.seg);
    o.cuts.wave_max = std::max(o.cuts.wave_max, o.cuts.short_max);
    return o;
  }
};

// ---- the draw, the acceptance test and the step: shared with the operator path (include/gunrock/rw/rw_functor.hxx) ----
__host__ __device__ __forceinline__ unsigned rw_walker_key(unsigned seed, unsigned w) { return color_fmix32(seed + 0x9E3779B9u * (w + 1u)); }
__host__ __device__ __forceinline__ unsigned rw_step_key(unsigned walker_key, unsigned t) { return color_fmix32(walker_key ^ (0x85EBCA6Bu * (t + 1u))); }
__host__ __device__ __forceinline__ unsigned rw_draw(unsigned step_key, unsigned k) { return color_fmix32(step_key ^ (0xC2B2AE35u * (k + 1u))); }
__host__ __device__ __forceinline__ float rw_unit(unsigned r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }      // 2^-24
__device__ __forceinline__ int rw_index(unsigned r, int d) { return (int)__umulhi(r, (unsigned)d); }
// a * (wmax * M) < w * b: products only, nothing an FMA could be contracted from
__device__ __forceinline__ bool rw_accept(float a, float limit, float w, float b) { return a * limit < w * b; }
__host__ __device__ __forceinline__ float rw_wmax_of(u64 wm) {
  const unsigned bits = (unsigned)(wm >> 32);
  float f;
  memcpy(&f, &bits, sizeof(f));
  return f;
}
__host__ __device__ __forceinline__ int rw_amax_of(u64 wm) { return (int)(0xFFFFFFFFu - (unsigned)wm); }
constexpr u64 RW_WM_UNIT = ((u64)0x3F800000u << 32) | 0xFFFFFFFFull;      // wmax = 1.0f, amax = 0: every row of an unweighted run

// whether c is among the ascending s[lo, hi): the last entry <= c, found without a data-dependent branch in the loop
__device__ __forceinline__ bool rw_member(const int* __restrict__ s, int lo, int hi, int c) {
  int len = hi - lo;
  if (len <= 0) return false;
  while (len > 1) {
    const int half = len >> 1;
    lo = s[lo + half] <= c ? lo + half : lo;
    len -= half;
  }
  return s[lo] == c;
}

struct rw_graph_t {
  const int* ro;
  const int* ci;
  const float* w;        // the entries' weights (weighted runs)
  const u64* wm;         // (wmax, amax) per row (weighted runs)
  const int* sorted;     // col_indices with ascending rows: ci itself or the sorted copy (second-order runs)
};
struct rw_params_t {
  unsigned seed;
  int tries;
  float ip, iq, big;     // 1 / p, 1 / q, M = max(ip, 1, iq)
  float restart;
};
struct rw_tally_t {
  unsigned restarts = 0, dead = 0, fallbacks = 0;
  u64 tries = 0;
};

// One step of a walker standing on cur (prev: the vertex before it, -1 none).  Returns the next vertex, or -1 when the walk ends
// here; prev follows.
template <bool WEIGHTED, bool SECOND>
__device__ __forceinline__ int rw_step(const rw_graph_t& g, const rw_params_t& P, unsigned walker_key, int t, int start, int cur, int& prev,
                                       rw_tally_t& tally) {
  const unsigned key = rw_step_key(walker_key, (unsigned)t);
  bool jump = P.restart > 0.f && rw_unit(rw_draw(key, 0)) < P.restart;
  int beg = 0, d = 0;
  u64 wm = RW_WM_UNIT;
  if (!jump) {
    beg = g.ro[cur];
    const int end = g.ro[cur + 1];
    if (WEIGHTED) wm = g.wm[cur];
    d = end - beg;
    const bool dead = d == 0 || (WEIGHTED && !(rw_wmax_of(wm) > 0.f));
    if (dead) {
      if (!(P.restart > 0.f)) { ++tally.dead; return -1; }
      jump = true;
    }
  }
  if (jump) {
    ++tally.restarts;
    prev = -1;
    return start;
  }
  int pick;
  if (!WEIGHTED && !SECOND) {
    pick = g.ci[beg + rw_index(rw_draw(key, 1), d)];
    ++tally.tries;
  } else {
    const bool second = SECOND && prev >= 0;
    const float limit = rw_wmax_of(wm) * (second ? P.big : 1.f);
    int pb = 0, pe = 0;
    if (second) { pb = g.ro[prev]; pe = g.ro[prev + 1]; }
    pick = -1;
    int i = 0;
#pragma nounroll
    for (; i < P.tries; ++i) {
      const int j = rw_index(rw_draw(key, 1u + 2u * (unsigned)i), d);
      const int c = g.ci[beg + j];
      const float w = WEIGHTED ? g.w[beg + j] : 1.f;
      const float a = rw_unit(rw_draw(key, 2u + 2u * (unsigned)i));
      float b = 1.f;
      if (second) b = c == prev ? P.ip : (rw_member(g.sorted, pb, pe, c) ? 1.f : P.iq);
      if (rw_accept(a, limit, w, b)) { pick = c; ++i; break; }
    }
    tally.tries += (u64)i;
    if (pick < 0) {
      ++tally.fallbacks;
      pick = g.ci[beg + rw_amax_of(wm)];
    }
  }
  prev = cur;
  return pick;
}

// ---- setup: the rows' maxima and whether the rows ascend ----
struct rw_setup_args_t {
  const int* ro;
  const int* ci;
  const float* w;
  u64* wm;               // n (NULL: no maxima wanted)
  int check_order;       // the rows' order is wanted
  int2* items;           // item_cap (vertex, segment) items of the segmented rows
  int* n_items;
  unsigned* flags;       // RW_FLAG_*
  long long* bins;       // RW_BINS
  int n, item_cap;
  row_cuts_t cuts;
};

// entries [k0, k1) of a row of len entries at beg, k0 + first, k0 + first + stride ...: the maximum of (weight, first position)
// and the flags (an entry greater than the one behind it; a negative or NaN weight)
__device__ __forceinline__ u64 rw_scan_row(const rw_setup_args_t& a, int beg, int len, int k0, int k1, int first, int stride, unsigned& flags) {
  u64 best = 0;
  for (int k = k0 + first; k < k1; k += stride) {
    if (a.wm) {
      const float w = a.w[beg + k];
      if (!(w >= 0.f)) flags |= RW_FLAG_NEGATIVE;
      const unsigned bits = w > 0.f ? __float_as_uint(w) : 0u;       // (-0.0f counts as 0.0f)
      best = max(best, ((u64)bits << 32) | (u64)(0xFFFFFFFFu - (unsigned)k));
    }
    if (a.check_order && k + 1 < len && a.ci[beg + k] > a.ci[beg + k + 1]) flags |= RW_FLAG_UNSORTED;
  }
  return best;
}

__global__ __launch_bounds__(BLOCK) void k_rw_setup(rw_setup_args_t a) {
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const int lane = lane_id();
  const unsigned n = (unsigned)a.n;
  unsigned flags = 0;
  int b[4] = {0, 0, 0, 0};
  long long segs = 0;
  for (unsigned base = gtid - lane; base < n; base += gthreads) {
    const bool in = base + lane < n;
    const int v = (int)(base + lane);
    const int beg = in ? a.ro[v] : 0;
    const int len = in ? a.ro[v + 1] - beg : 0;
    const int body = in ? a.cuts.body_of(len) : -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] += body == c ? 1 : 0;
    if (body == ROW_LONG) segs += a.cuts.segments_of(len);
    if (body == ROW_LANE) {
      const u64 best = rw_scan_row(a, beg, len, 0, len, 0, 1, flags);
      if (a.wm) a.wm[v] = best;
    }
    if ((body == ROW_NONE || body == ROW_LONG) && a.wm) a.wm[v] = 0;          // (a segmented row's items meet here, in the launch behind)
    u64 todo = __ballot(body == ROW_WAVE);                       // (for_each_wave_row and row_bins_t, written out: either cost this
    while (todo) {                                               //  kernel two registers)
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int b0 = __shfl(beg, src, WAVE), l0 = __shfl(len, src, WAVE);
      const u64 best = wave_max(rw_scan_row(a, b0, l0, 0, l0, lane, WAVE, flags));
      if (lane == src && a.wm) a.wm[v] = best;
    }
    if (__ballot(body == ROW_LONG)) wave_append_segments(body == ROW_LONG, v, len, a.cuts.seg, a.items, a.n_items);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int s = wave_sum(b[c]);
    if (lane == 0 && s) atomicAdd((u64*)&a.bins[c], (u64)s);
  }
  segs = wave_sum(segs);
  if (lane == 0 && segs) atomicAdd((u64*)&a.bins[4], (u64)segs);
  if (flags) atomicOr(a.flags, flags);
}

// a wave per (vertex, segment) item of the rows of more than wave_max entries
__global__ __launch_bounds__(BLOCK) void k_rw_setup_long(rw_setup_args_t a) {
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (unsigned)BLOCK / WAVE);
  const int n_items = min(*a.n_items, a.item_cap);
  unsigned flags = 0;
  for (int it = wave; it < n_items; it += waves) {
    const int2 item = a.items[it];
    const int beg = a.ro[item.x];
    const int len = a.ro[item.x + 1] - beg;
    const long long k0 = (long long)item.y * a.cuts.seg;
    const int k1 = (int)min((long long)len, k0 + a.cuts.seg);
    const u64 best = wave_max(rw_scan_row(a, beg, len, (int)k0, k1, lane, WAVE, flags));
    if (lane == 0 && a.wm && best) atomicMax(a.wm + item.x, best);
  }
  if (flags) atomicOr(a.flags, flags);
}

// ---- the walk ----
struct rw_args_t {
  rw_graph_t g;
  rw_params_t P;
  const int* starts;     // S ids on the device (NULL: start s is vertex s)
  int* paths;            // W x (L + 1) (NULL: not kept)
  int* ends;             // W
  int* lengths;          // W
  u64* visits;           // n (NULL: not kept)
  u64* counters;         // RW_COUNTERS
  int walkers, per_start, length, tile;
};

// the tile's slots [first, first + count) of the workgroup's walkers [base, base + BLOCK) to their rows of the path matrix:
// consecutive lanes write consecutive slots of one walker
__device__ __forceinline__ void rw_flush_tile(const rw_args_t& a, const int* tile, long long base, int first, int count) {
  __syncthreads();
  const size_t pitch = (size_t)a.length + 1;
  for (int i = threadIdx.x; i < BLOCK * count; i += BLOCK) {
    const int x = i / count, k = i - x * count;
    if (base + x < a.walkers) a.paths[(size_t)(base + x) * pitch + (size_t)(first + k)] = tile[k * RW_TILE_PITCH + x];
  }
  __syncthreads();
}

template <bool WEIGHTED, bool SECOND>
__global__ __launch_bounds__(BLOCK) void k_rw_walk(rw_args_t a) {
  extern __shared__ int s_tile[];                                // tile x RW_TILE_PITCH words (none without paths)
  const int lane = lane_id();
  const int tmask = a.tile - 1;
  rw_tally_t tally;
  u64 steps = 0;
  for (long long base = (long long)blockIdx.x * BLOCK; base < a.walkers; base += (long long)gridDim.x * BLOCK) {
    const long long w = base + threadIdx.x;
    const bool in = w < a.walkers;
    int start = -1;
    if (in) {
      const int s = (int)(w / a.per_start);
      start = a.starts ? a.starts[s] : s;
    }
    const unsigned key = rw_walker_key(a.P.seed, (unsigned)w);
    int cur = start, prev = -1, len = 0;
    bool alive = in;
    if (a.visits && in) atomicAdd(a.visits + start, 1ull);
    if (a.paths) {
      s_tile[threadIdx.x] = start;
      if (tmask == 0 || a.length == 0) rw_flush_tile(a, s_tile, base, 0, 1);
    }
    for (int t = 0; t < a.length; ++t) {
      int nxt = -1;
      if (alive) {
        nxt = rw_step<WEIGHTED, SECOND>(a.g, a.P, key, t, start, cur, prev, tally);
        alive = nxt >= 0;
        if (alive) {
          cur = nxt;
          ++len;
          if (a.visits) atomicAdd(a.visits + nxt, 1ull);
        }
      }
      if (a.paths) {
        const int slot = t + 1, k = slot & tmask;
        s_tile[k * RW_TILE_PITCH + threadIdx.x] = nxt;
        if (k == tmask || slot == a.length) rw_flush_tile(a, s_tile, base, slot - k, k + 1);
      } else if (!__any(alive)) {
        break;
      }
    }
    if (in) {
      a.ends[w] = cur;
      a.lengths[w] = len;
    }
    steps += (u64)len;
  }
  const u64 c[RW_COUNTERS] = {steps, (u64)tally.dead, (u64)tally.restarts, tally.tries, (u64)tally.fallbacks};
#pragma unroll
  for (int k = 0; k < RW_COUNTERS; ++k) {
    const u64 s = wave_sum(c[k]);
    if (lane == 0 && s) atomicAdd(a.counters + k, s);
  }
}

// what a run of either path is asked for, checked by the C-ABI
struct rw_request_t {
  const int* h_starts;   // S ids on the host (NULL: every vertex)
  long long starts, per_start, length;
  unsigned seed;
  bool weighted, second, want_paths, want_visits;
  float ip, iq, restart;
  long long walkers() const { return starts * per_start; }
};

// The setup both paths share, per handle: redone when a run's mode needs what is missing.
struct rw_setup_state_t {
  int n = 0;
  long long m = 0;
  rw_opts_t opts;
  mem_t<u64> wm;
  mem_t<int> sorted;                 // the sorted copy of col_indices (only when some row is not ascending)
  mem_t<int2> items;
  mem_t<int> n_items;
  mem_t<unsigned> flags;
  mem_t<long long> d_bins;
  int item_cap = 0;
  bool have_weights = false, have_order = false, unsorted = false;
  long long bins[RW_BINS] = {0};

  rw_setup_state_t(int n_, long long m_, context_t& ctx) : n(n_), m(m_), opts(rw_opts_t::from_env()) {
    item_cap = (int)std::min<long long>(std::min<long long>(std::max(n, 1), m / (opts.cuts.wave_max + 1) + 1) + m / opts.cuts.seg + 1, 0x7fffffff);
    n_items = mem_t<int>(1, ctx);
    flags = mem_t<unsigned>(1, ctx);
    d_bins = mem_t<long long>(RW_BINS, ctx);
  }

  // What the run needs and the handle does not have yet.  Adds its launches and host waits: two launches and one wait when
  // anything was missing, a call of the segmented sort (counted as one launch, two waits) for the sorted copy.
  void ensure(const int* ro, const int* ci, const float* w, bool weighted, bool second, standard_context_t& ctx, long long& launches,
              long long& waits) {
    const bool need_w = weighted && !have_weights, need_o = second && !have_order;
    if ((!need_w && !need_o) || n <= 0) return;
    const hipStream_t st = ctx.stream();
    if (need_w && wm.size() == 0) wm = mem_t<u64>((size_t)n, ctx);
    if (items.size() == 0) items = mem_t<int2>((size_t)item_cap, ctx);
    MGX_HIP(hipMemsetAsync(n_items.data(), 0, sizeof(int), st));
    MGX_HIP(hipMemsetAsync(flags.data(), 0, sizeof(unsigned), st));
    MGX_HIP(hipMemsetAsync(d_bins.data(), 0, RW_BINS * sizeof(long long), st));
    rw_setup_args_t a;
    a.ro = ro; a.ci = ci; a.w = w;
    a.wm = need_w ? wm.data() : nullptr;
    a.check_order = need_o ? 1 : 0;
    a.items = items.data(); a.n_items = n_items.data(); a.flags = flags.data(); a.bins = d_bins.data();
    a.n = n; a.item_cap = item_cap; a.cuts = opts.cuts;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8);
    hipLaunchKernelGGL(k_rw_setup, dim3(blocks), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_rw_setup_long, dim3(blocks), dim3(BLOCK), 0, st, a);
    MGX_CHECK_LAUNCH("mgx rw setup");
    launches += 2;
    unsigned h_flags = 0;
    MGX_HIP(dtoh(bins, (const long long*)d_bins.data(), RW_BINS, st));
    MGX_HIP(dtoh(&h_flags, (const unsigned*)flags.data(), 1, st));
    ++waits;
    if (need_w) {
      if (h_flags & RW_FLAG_NEGATIVE) throw mgx_error(MGX_E_NEGATIVE_WEIGHT, "mgx rw: negative or NaN edge weight in a weighted run");
      have_weights = true;
    }
    if (need_o) {
      unsorted = (h_flags & RW_FLAG_UNSORTED) != 0;
      if (unsorted) {
        sorted = mem_t<int>((size_t)m, ctx);
        MGX_HIP(dtod(sorted.data(), ci, (size_t)m, st));
        auto up = [] __device__(int x, int y) { return x < y; };
        segmented_sort_impl<int, segsort_no_value_t>(sorted.data(), nullptr, m, ro + 1, n - 1, up, ctx);
        ++launches;
        waits += 2;
      }
      have_order = true;
    }
  }
  rw_graph_t graph(const int* ro, const int* ci, const float* w, bool weighted, bool second) const {
    rw_graph_t g;
    g.ro = ro; g.ci = ci;
    g.w = weighted ? w : nullptr;
    g.wm = weighted ? wm.data() : nullptr;
    g.sorted = second ? (unsorted ? sorted.data() : ci) : nullptr;
    return g;
  }
};

inline rw_params_t rw_params_of(const rw_request_t& r, const rw_opts_t& o) {
  rw_params_t P;
  P.seed = r.seed; P.tries = o.tries;
  P.ip = r.ip; P.iq = r.iq; P.big = std::max(std::max(r.ip, 1.0f), r.iq);
  P.restart = r.restart;
  return P;
}

// The results' arrays of one path (the fused one's or the operator path's): they grow with the largest run.
struct rw_results_t {
  mem_t<int> d_starts, paths, ends, lengths;
  mem_t<u64> visits, counters;
  size_t starts_cap = 0, walker_cap = 0, path_cap = 0;
  void ensure(const rw_request_t& r, int n, context_t& ctx) {
    const size_t W = (size_t)r.walkers();
    if (counters.size() == 0) counters = mem_t<u64>(RW_COUNTERS, ctx);
    if (r.h_starts && (size_t)r.starts > starts_cap) { d_starts = mem_t<int>((size_t)r.starts, ctx); starts_cap = (size_t)r.starts; }
    if (W > walker_cap) { ends = mem_t<int>(W, ctx); lengths = mem_t<int>(W, ctx); walker_cap = W; }
    const size_t slots = W * ((size_t)r.length + 1);
    if (r.want_paths && slots > path_cap) {
      paths = mem_t<int>();                                     // (the old one goes first: both need not fit)
      path_cap = 0;
      paths = mem_t<int>(slots, ctx);
      path_cap = slots;
    }
    if (r.want_visits && visits.size() == 0) visits = mem_t<u64>((size_t)std::max(n, 1), ctx);
  }
};

// The device state of a graph's fused walks, and the run (host side).
struct rw_fused_state_t {
  int n = 0;
  rw_results_t res;
  pinned_t<u64> h_counters;
  bool timing = false;
  double phase_ms[2] = {0.0, 0.0};               // the last timed run: setup, walk
  event_t ev[3];

  rw_fused_state_t(int n_, context_t&) : n(n_) { h_counters = pinned_t<u64>(RW_COUNTERS); }

  // Returns the ten stats of mgx_rw_run.  Host waits: one for the starts' upload (when given), the setup's, one for the counters.
  std::vector<long long> run(rw_setup_state_t& su, const int* ro, const int* ci, const float* w, const rw_request_t& r, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const long long W = r.walkers();
    long long launches = 0, waits = 0;
    phase_ms[0] = phase_ms[1] = 0.0;
    if (n <= 0 || W == 0) return {W, r.length, 0, 0, 0, 0, 0, 0, 0, 0};
    res.ensure(r, n, ctx);
    if (timing) MGX_HIP(hipEventRecord(ev[0], st));
    su.ensure(ro, ci, w, r.weighted, r.second, ctx, launches, waits);
    if (timing) MGX_HIP(hipEventRecord(ev[1], st));
    if (r.h_starts) { MGX_HIP(htod(res.d_starts.data(), r.h_starts, (size_t)r.starts, st)); ++waits; }
    MGX_HIP(hipMemsetAsync(res.counters.data(), 0, RW_COUNTERS * sizeof(u64), st));
    if (r.want_visits) MGX_HIP(hipMemsetAsync(res.visits.data(), 0, (size_t)n * sizeof(u64), st));
    rw_args_t a;
    a.g = su.graph(ro, ci, w, r.weighted, r.second);
    a.P = rw_params_of(r, su.opts);
    a.starts = r.h_starts ? res.d_starts.data() : nullptr;
    a.paths = r.want_paths ? res.paths.data() : nullptr;
    a.ends = res.ends.data(); a.lengths = res.lengths.data();
    a.visits = r.want_visits ? res.visits.data() : nullptr;
    a.counters = res.counters.data();
    a.walkers = (int)W; a.per_start = (int)r.per_start; a.length = (int)r.length; a.tile = su.opts.tile;
    const int blocks = grid_for(W, BLOCK, std::max(ctx.num_cus, 1) * 8);
    const size_t lds = r.want_paths ? (size_t)su.opts.tile * RW_TILE_PITCH * sizeof(int) : 0;
    if (r.weighted) {
      if (r.second) hipLaunchKernelGGL((k_rw_walk<true, true>), dim3(blocks), dim3(BLOCK), lds, st, a);
      else hipLaunchKernelGGL((k_rw_walk<true, false>), dim3(blocks), dim3(BLOCK), lds, st, a);
    } else {
      if (r.second) hipLaunchKernelGGL((k_rw_walk<false, true>), dim3(blocks), dim3(BLOCK), lds, st, a);
      else hipLaunchKernelGGL((k_rw_walk<false, false>), dim3(blocks), dim3(BLOCK), lds, st, a);
    }
    MGX_CHECK_LAUNCH("mgx rw walk");
    ++launches;
    if (timing) MGX_HIP(hipEventRecord(ev[2], st));
    h_counters.fetch(res.counters.data(), RW_COUNTERS, st);
    ++waits;
    if (timing) {
      float ms = 0.f;
      MGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); phase_ms[0] = ms;
      MGX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2])); phase_ms[1] = ms;
    }
    const u64* c = h_counters.data();
    return {W, r.length, (long long)c[RW_C_STEPS], (long long)c[RW_C_DEAD], (long long)c[RW_C_RESTARTS], (long long)c[RW_C_TRIES],
            (long long)c[RW_C_FALLBACKS], su.unsorted && r.second ? 1 : 0, launches, waits};
  }
};

}  // namespace mgx
