// mgx/nsample_fused.hpp -- fan-out neighbour sampling for GNN mini-batches, fused (mgx_nsample_run): from a batch of seeds up to
// k_h out-neighbours of every newly reached vertex at hop h, without replacement (or with), the result one renumbered subgraph.
// The whole run is 5 H + 4 launches enqueued back to back and one read-back: nothing is asked of the device between the hops.
//
// The definition (the operator path include/gunrock/nsample/ and tests/nsample_model.py compute the same, bit for bit).
//   frontiers  V_0 is the ascending set of distinct seeds; every v of V_h is sampled once, at hop h; V_{h + 1} is the ascending set
//              of the sampled destinations that are in none of V_0 .. V_h.  A vertex's local id is its place in V_0 | V_1 | .. | V_H.
//   a row      v at hop h, d its out-degree, k = fanouts[h], key = rw_step_key(rw_walker_key(seed, v), h) -- from the GLOBAL id: a
//              vertex's sample depends on the graph, the seed, h and v, never on who else is in the batch.
//              d == 0: nothing.  k == -1, or !replace and d <= k: positions 0 .. d - 1 in the STORED order (a whole row).
//              replace: positions umulhi(rw_draw(key, j), d), j = 0 .. k - 1.
//              else Floyd's algorithm, exactly k draws and no retries: j = 0 .. k - 1, i = d - k + j, t = umulhi(rw_draw(key, j),
//              i + 1), p_j = i when t is among p_0 .. p_{j - 1} (a collision), else t.  Slot j of the row holds p_j: insertion
//              order, no sort.  Self-loops and duplicate entries are entries like any other.
//   results    vertices int32[N] (local -> global), hop_offsets int32[H + 2], row_offsets int32[R + 1] over the R = hop_offsets[H]
//              local rows, cols int32[E] (local ids), entry_pos int32[E] (the index into the graph's col_indices / weights of
//              every sampled entry), seed_local int32[count], twelve exact counters.
// Capacities come from bounds (ns_bounds_t), so the run never asks the device how big a hop was: F_0 = min(n, count), E_h = F_h k_h
// (clamped to m unless replace; k = -1: m), F_{h + 1} = min(n, E_h).  Every array is allocated to them before the first launch, on
// the handle, growing only.  Every kernel reads its true counts from the control block in device memory and runs a grid sized by
// the bound and capped at 8 workgroups a compute unit.
// The launches:
//   k_ns_mark          the seeds set their bits in `fresh`
//   k_ns_rank_count    popcounts of fresh's 64-bit words per tile of NS_TILE words
//   k_ns_rank_apply    the words' ranks (the tile sums before it, a workgroup scan inside): a new vertex's ascending local id, its
//                      slot of `vertices`, its word of the local-id map; fresh is folded into `seen` and cleared
//   per hop: k_ns_rows   min(d, k) (k with replace, d with -1) per frontier row, scanned inside a tile of NS_TILE rows
//            k_ns_sample a group of G lanes of one wave per row, G the smallest power of two >= k: a wave runs 64 / G rows at a
//                        time in k steps; a pick's membership among the row's earlier picks is ONE __ballot masked to the group: no
//                        LDS, no scratch, no per-lane arrays, all 64 lanes active through the ballots.  A row's cost is k draws
//                        and k gathers whatever its degree.  k = -1: rows are copies, by length (row_bodies.hpp): a lane's, a
//                        wave's, or (vertex, segment) items.  Destinations not in `seen` (read-only within a launch) set their
//                        bit in `fresh` with a device-scope atomicOr
//            k_ns_long   a wave per (row, segment) item; its first wave closes the hop's entry total
//            k_ns_rank_count, k_ns_rank_apply: the next frontier
//   k_ns_finish        cols become local ids through the map, the seeds' local ids, and the words of `seen` the run's vertices touched
//                      are cleared: O(vertices), not O(n) -- a later run on the handle finds what a fresh handle finds
// Cost per hop: O(frontier x k + n / 64 words).  There is no sort.
// Not built: weighted (biased) sampling, more than one device, several batches per host wait, fan-outs above 64.
#pragma once
#include <algorithm>
#include <vector>

#include "env.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "rw_fused.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (the three cuts are unmeasured guesses)
constexpr int NS_MAX_HOPS = 16;
constexpr int NS_MAX_FANOUT = 64;
constexpr int NS_SHORT_MAX_DEFAULT = 32;
constexpr int NS_WAVE_MAX_DEFAULT = 1024;
constexpr int NS_SEG_DEFAULT = 1024;
constexpr int NS_CUT_MAX = 1 << 20;
constexpr int NS_PER_THREAD = 8;
constexpr int NS_TILE = BLOCK * NS_PER_THREAD;      // rows (k_ns_rows) or bitmap words (k_ns_rank_*) per tile sum
enum : int { NS_C_EMPTY = 0, NS_C_WHOLE = 1, NS_C_SAMPLED = 2, NS_C_DRAWS = 3, NS_C_COLLISIONS = 4, NS_C_REVISITS = 5, NS_COUNTERS = 6 };
enum : int { NS_BINS = 5 };                         // the copied rows (k = -1): without entries, a lane's, a wave's, segmented, their segments
enum : int { NS_STATS = 14 };
constexpr int NS_SLOTS = 64;                        // copies of the counters, a 64-byte line each: a wave adds to its workgroup's


struct ns_opts_t {
  row_cuts_t cuts = {NS_SHORT_MAX_DEFAULT, NS_WAVE_MAX_DEFAULT, NS_SEG_DEFAULT};
  static ns_opts_t from_env() {
    ns_opts_t o;
    o.cuts.short_max = env_int("MGX_NSAMPLE_SHORT_MAX", 0, NS_CUT_MAX, o.cuts.short_max);
    o.cuts.wave_max = env_int("MGX_NSAMPLE_WAVE_MAX", 0, NS_CUT_MAX, o.cuts.wave_max);
    o.cuts.seg = env_int("MGX_NSAMPLE_SEG", 1, NS_CUT_MAX, o.cuts.seg);
    o.cuts.wave_max = std::max(o.cuts.wave_max, o.cuts.short_max);
    return o;
  }
};

// ---- what both paths share: a row's key, its entry count, the bounds ----
__host__ __device__ __forceinline__ unsigned ns_row_key(unsigned seed, int v, int hop) { return rw_step_key(rw_walker_key(seed, (unsigned)v), (unsigned)hop); }
__host__ __device__ __forceinline__ bool ns_whole(int d, int k, int replace) { return k < 0 || (!replace && d <= k); }
__host__ __device__ __forceinline__ int ns_entries(int d, int k, int replace) { return d == 0 ? 0 : (ns_whole(d, k, replace) ? d : k); }
// the smallest power of two >= k (k in 1 .. 64); 1 for k = -1
inline int ns_group(int k) {
  int g = 1;
  while (g < k) g *= 2;
  return g;
}

// what a run is asked for, checked by the C-ABI
struct ns_request_t {
  const int* h_seeds = nullptr;      // `count` ids on the host (NULL: every vertex)
  long long count = 0;               // the seeds (n when h_seeds == NULL)
  int hops = 0;
  int fanouts[NS_MAX_HOPS] = {0};
  int replace = 0;
  unsigned seed = 0;
};

// the capacities: F[h] bounds |V_h|, E[h] hop h's entries
struct ns_bounds_t {
  long long F[NS_MAX_HOPS + 1] = {0}, E[NS_MAX_HOPS] = {0};
  long long vertices = 0, rows = 0, entries = 0, front = 0, items = 0;
  bool overflow() const { return vertices >= (1ll << 31) || rows >= (1ll << 31) || entries >= (1ll << 31) || items >= (1ll << 31); }
};
inline ns_bounds_t ns_bounds(long long n, long long m, const ns_request_t& r, const row_cuts_t& cuts) {
  ns_bounds_t b;
  b.F[0] = std::min(n, r.count);
  for (int h = 0; h < r.hops; ++h) {
    const int k = r.fanouts[h];
    b.E[h] = k < 0 ? m : (r.replace ? b.F[h] * k : std::min(m, b.F[h] * k));
    b.F[h + 1] = std::min(n, b.E[h]);
    b.entries += b.E[h];
    b.rows += b.F[h];
    if (k < 0) b.items = std::max(b.items, std::min(b.F[h], m / ((long long)cuts.wave_max + 1) + 1) + m / cuts.seg + 1);
  }
  b.rows = std::min(n, b.rows);
  b.vertices = std::min(n, b.rows + b.F[r.hops]);
  for (int h = 0; h <= r.hops; ++h) b.front = std::max(b.front, b.F[h]);
  return b;
}

// the run's words in device memory: every kernel reads its true counts here
struct ns_control_t {
  int hop_off[NS_MAX_HOPS + 2];      // V_h = vertices[hop_off[h], hop_off[h + 1])
  int edge_off[NS_MAX_HOPS + 1];     // the entries before hop h
  int n_items[NS_MAX_HOPS];          // hop h's (row, segment) items
  u64 counters[NS_SLOTS][8];         // (every wave of a hop adds here at its end: one line would serialise them)
  long long bins[NS_BINS];
};

struct ns_args_t {
  const int* ro;
  const int* ci;
  const int* seeds;      // count ids on the device (NULL: seed i is vertex i)
  ns_control_t* ctl;
  u64* seen;             // (n + 63) / 64 words: the vertices that have a local id; read-only within a launch
  u64* fresh;            // as many: the destinations found in this hop
  int* map;              // n: global -> local, defined where seen or fresh is set
  int* vertices;
  int* row_offsets;
  int* cols;
  int* entry_pos;
  int* seed_local;
  int* partials;         // the tile sums of the launch before
  int2* items;
  int n, count, hops, item_cap;
  int hop, k, group, replace;
  unsigned seed;
  row_cuts_t cuts;
};

// the sum of x over the workgroup, in every thread (two barriers)
__device__ __forceinline__ int ns_block_sum(int x, int* smem) {
  int total;
  (void)block_exclusive_sum(x, smem, &total);
  return total;
}
// the sum of p[0, count) in every thread
__device__ __forceinline__ int ns_block_sum_of(const int* p, int count, int* smem) {
  int s = 0;
  for (int i = threadIdx.x; i < count; i += BLOCK) s += p[i];
  return ns_block_sum(s, smem);
}

__global__ __launch_bounds__(BLOCK) void k_ns_mark(ns_args_t a) {
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  for (unsigned i = blockIdx.x * (unsigned)BLOCK + threadIdx.x; i < (unsigned)a.count; i += gthreads) {
    const int v = a.seeds ? a.seeds[i] : (int)i;
    atomicOr(a.fresh + (v >> 6), 1ull << (v & 63));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.row_offsets[0] = 0;
}

__global__ __launch_bounds__(BLOCK) void k_ns_rank_count(ns_args_t a) {
  __shared__ int sm[WAVES_PER_BLOCK + 1];
  const int words = (a.n + 63) / 64;
  const int tiles = (words + NS_TILE - 1) / NS_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int w0 = tile * NS_TILE + threadIdx.x * NS_PER_THREAD;
    int c = 0;
#pragma unroll
    for (int i = 0; i < NS_PER_THREAD; ++i) c += w0 + i < words ? __popcll(a.fresh[w0 + i]) : 0;
    const int total = ns_block_sum(c, sm);
    if (threadIdx.x == 0) a.partials[tile] = total;
  }
}

// slot: the new vertices are V_slot (0: the seeds)
__global__ __launch_bounds__(BLOCK) void k_ns_rank_apply(ns_args_t a, int slot) {
  __shared__ int sm[WAVES_PER_BLOCK + 1];
  const int words = (a.n + 63) / 64;
  const int tiles = (words + NS_TILE - 1) / NS_TILE;
  const int base = a.ctl->hop_off[slot];
  if (blockIdx.x == 0) {
    const int all = ns_block_sum_of(a.partials, tiles, sm);
    if (threadIdx.x == 0) a.ctl->hop_off[slot + 1] = base + all;
  }
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int before = ns_block_sum_of(a.partials, tile, sm);
    const int w0 = tile * NS_TILE + threadIdx.x * NS_PER_THREAD;
    int c = 0;
#pragma unroll
    for (int i = 0; i < NS_PER_THREAD; ++i) c += w0 + i < words ? __popcll(a.fresh[w0 + i]) : 0;
    int total;
    int id = base + before + block_exclusive_sum(c, sm, &total);
    if (c == 0) continue;                                        // (no barrier below)
    for (int i = 0; i < NS_PER_THREAD; ++i) {
      if (w0 + i >= words) break;
      u64 f = a.fresh[w0 + i];
      if (!f) continue;
      a.seen[w0 + i] |= f;
      a.fresh[w0 + i] = 0;
      while (f) {
        const int v = (w0 + i) * 64 + __ffsll((long long)f) - 1;
        f &= f - 1;
        a.vertices[id] = v;
        a.map[v] = id;
        ++id;
      }
    }
  }
}

// the entries of every frontier row, scanned inside its tile: row_offsets holds the tile-local prefix until k_ns_sample adds what lies before
__global__ __launch_bounds__(BLOCK) void k_ns_rows(ns_args_t a) {
  __shared__ int sm[WAVES_PER_BLOCK + 1];
  const int hb = a.ctl->hop_off[a.hop];
  const int F = a.ctl->hop_off[a.hop + 1] - hb;
  const int tiles = (F + NS_TILE - 1) / NS_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile * NS_TILE + threadIdx.x * NS_PER_THREAD;
    int c[NS_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < NS_PER_THREAD; ++i) {
      c[i] = 0;
      if (r0 + i < F) {
        const int v = a.vertices[hb + r0 + i];
        c[i] = ns_entries(a.ro[v + 1] - a.ro[v], a.k, a.replace);
      }
      mine += c[i];
    }
    int total;
    int run = block_exclusive_sum(mine, sm, &total);
#pragma unroll
    for (int i = 0; i < NS_PER_THREAD; ++i) {
      if (r0 + i < F) a.row_offsets[hb + r0 + i] = run;
      run += c[i];
    }
    if (threadIdx.x == 0) a.partials[tile] = total;
  }
}

// entry e of the sampled subgraph is position pos of the graph's entries; its destination is numbered later (k_ns_finish)
__device__ __forceinline__ void ns_emit(const ns_args_t& a, int e, int pos, unsigned& revisits) {
  const int dst = a.ci[pos];
  a.entry_pos[e] = pos;
  a.cols[e] = dst;
  const u64 bit = 1ull << (dst & 63);
  if (a.seen[dst >> 6] & bit) ++revisits;
  else atomicOr(a.fresh + (dst >> 6), bit);
}

// A wave takes a run of consecutive passes, 64 / group rows each, so that it adds up the tiles before its rows once.
__global__ __launch_bounds__(BLOCK) void k_ns_sample(ns_args_t a) {
  const int lane = lane_id();
  const int hb = a.ctl->hop_off[a.hop];
  const int F = a.ctl->hop_off[a.hop + 1] - hb;
  const int eb = a.ctl->edge_off[a.hop];
  const int G = a.group, per_pass = WAVE / G;
  const int passes = (F + per_pass - 1) / per_pass;
  const int waves = (int)(gridDim.x * (unsigned)WAVES_PER_BLOCK);
  const int wave = (int)(blockIdx.x * (unsigned)WAVES_PER_BLOCK + threadIdx.x / WAVE);
  const int chunk = (passes + waves - 1) / waves;
  const int q0 = (int)min((long long)wave * chunk, (long long)passes), q1 = (int)min((long long)q0 + chunk, (long long)passes);
  const int j = lane & (G - 1), first = lane - j;
  const u64 gmask = G == WAVE ? ~0ull : ((1ull << G) - 1ull) << first;
  unsigned c_empty = 0, c_whole = 0, c_sampled = 0, c_draws = 0, c_coll = 0, c_rev = 0;
  long long segs = 0;
  row_bins_t bins;
  int tile = -1, before = 0;
  for (int q = q0; q < q1; ++q) {
    const int r = q * per_pass + lane / G;
    const int t = (q * per_pass) / NS_TILE;                      // (per_pass divides NS_TILE: a pass lies in one tile)
    if (tile < 0) {
      int s = 0;
      for (int i = lane; i < t; i += WAVE) s += a.partials[i];
      before = wave_sum(s);
      tile = t;
    }
    for (; tile < t; ++tile) before += a.partials[tile];
    const bool valid = r < F;
    int v = 0, beg = 0, d = 0, off = 0;
    if (valid) {
      v = a.vertices[hb + r];
      beg = a.ro[v];
      d = a.ro[v + 1] - beg;
      off = eb + before + a.row_offsets[hb + r];
      if (j == 0) {
        a.row_offsets[hb + r] = off;
        if (d == 0) ++c_empty;
        else if (ns_whole(d, a.k, a.replace)) ++c_whole;
        else { ++c_sampled; c_draws += (unsigned)a.k; }
      }
    }
    if (a.k < 0) {                                               // copies, a lane per row (G == 1)
      const int body = valid ? a.cuts.body_of(d) : -1;
      bins.count(body);
      if (body == ROW_LANE) for (int e = 0; e < d; ++e) ns_emit(a, off + e, beg + e, c_rev);
      for_each_wave_row(body == ROW_WAVE, [&](int src) {
        const int b0 = __shfl(beg, src, WAVE), l0 = __shfl(d, src, WAVE), o0 = __shfl(off, src, WAVE);
        for (int e = lane; e < l0; e += WAVE) ns_emit(a, o0 + e, b0 + e, c_rev);
      });
      if (body == ROW_LONG) segs += a.cuts.segments_of(d);
      wave_append_segments(body == ROW_LONG, r, d, a.cuts.seg, a.items, a.ctl->n_items + a.hop);
      continue;
    }
    const unsigned key = ns_row_key(a.seed, v, a.hop);
    const bool floyd = valid && !a.replace && d > a.k;
    int p = -1;                                                  // this lane's position in its row (-1: none)
    if (valid && j < a.k) {
      if (a.replace) p = d > 0 ? rw_index(rw_draw(key, (unsigned)j), d) : -1;
      else if (!floyd) p = j < d ? j : -1;
    }
    if (__any(floyd)) {
      // lane j of a group holds draw j; step s hands it to the group, whose lanes say in one ballot whether they hold it already
      const int mine = floyd && j < a.k ? rw_index(rw_draw(key, (unsigned)j), d - a.k + j + 1) : -1;
      for (int s = 0; s < a.k; ++s) {
        const int cand = __shfl(mine, first + s, WAVE);
        const u64 hit = __ballot(floyd && p == cand) & gmask;
        if (floyd && j == s) {
          p = hit ? d - a.k + s : cand;
          c_coll += hit ? 1u : 0u;
        }
      }
    }
    if (p >= 0) ns_emit(a, off + j, beg + p, c_rev);
  }
  const unsigned c[NS_COUNTERS] = {c_empty, c_whole, c_sampled, c_draws, c_coll, c_rev};
#pragma unroll
  for (int i = 0; i < NS_COUNTERS; ++i) {
    const unsigned s = wave_sum(c[i]);
    if (lane == 0 && s) atomicAdd(&a.ctl->counters[blockIdx.x & (NS_SLOTS - 1)][i], (u64)s);
  }
  if (a.k < 0) {
    bins.add_to(a.ctl->bins);
    segs = wave_sum(segs);
    if (lane == 0 && segs) atomicAdd((u64*)&a.ctl->bins[4], (u64)segs);
  }
}

// a wave per (row, segment) item of the copied rows of more than wave_max entries; the first wave closes the hop's entries
__global__ __launch_bounds__(BLOCK) void k_ns_long(ns_args_t a) {
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (unsigned)BLOCK / WAVE);
  const int hb = a.ctl->hop_off[a.hop];
  const int F = a.ctl->hop_off[a.hop + 1] - hb;
  if (wave == 0) {
    const int tiles = (F + NS_TILE - 1) / NS_TILE;
    int s = 0;
    for (int i = lane; i < tiles; i += WAVE) s += a.partials[i];
    s = wave_sum(s) + a.ctl->edge_off[a.hop];
    if (lane == 0) {
      a.ctl->edge_off[a.hop + 1] = s;
      a.row_offsets[hb + F] = s;
    }
  }
  const int n_items = min(a.ctl->n_items[a.hop], a.item_cap);
  unsigned c_rev = 0;
  for (int it = wave; it < n_items; it += waves) {
    const int2 item = a.items[it];
    const int v = a.vertices[hb + item.x];
    const int beg = a.ro[v];
    const int len = a.ro[v + 1] - beg;
    const int off = a.row_offsets[hb + item.x];
    const long long k0 = (long long)item.y * a.cuts.seg;
    const int k1 = (int)min((long long)len, k0 + a.cuts.seg);
    for (int e = (int)k0 + lane; e < k1; e += WAVE) ns_emit(a, off + e, beg + e, c_rev);
  }
  c_rev = wave_sum(c_rev);
  if (lane == 0 && c_rev) atomicAdd(&a.ctl->counters[blockIdx.x & (NS_SLOTS - 1)][NS_C_REVISITS], (u64)c_rev);
}

__global__ __launch_bounds__(BLOCK) void k_ns_finish(ns_args_t a) {
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const unsigned E = (unsigned)a.ctl->edge_off[a.hops], N = (unsigned)a.ctl->hop_off[a.hops + 1];
  for (unsigned e = gtid; e < E; e += gthreads) a.cols[e] = a.map[a.cols[e]];
  for (unsigned i = gtid; i < (unsigned)a.count; i += gthreads) a.seed_local[i] = a.map[a.seeds ? a.seeds[i] : (int)i];
  for (unsigned i = gtid; i < N; i += gthreads) a.seen[a.vertices[i] >> 6] = 0;
}

// The results' arrays of one path (the fused one's or the operator path's), sized by the bounds, growing only, and what the
// host knows of the last run.
struct ns_results_t {
  mem_t<int> d_seeds, vertices, row_offsets, cols, entry_pos, seed_local;
  size_t seeds_cap = 0, vertices_cap = 0, rows_cap = 0, entries_cap = 0;
  std::vector<int> hop_offsets;      // H + 2
  std::vector<int> edge_offsets;     // H + 1: the entries before hop h (what a reader of one hop's rows needs without a wait)
  bool any_whole = false;            // a fan-out of the run was -1: rows may be longer than NS_MAX_FANOUT
  long long seeds = 0, edges = 0;
  bool device = false;               // the last run did device work (else every array is empty and row_offsets is {0})
  static void grow(mem_t<int>& m, size_t& cap, size_t want, context_t& ctx) {
    if (want <= cap) return;
    m = mem_t<int>();                                            // (the old one goes first: both need not fit)
    cap = 0;
    m = mem_t<int>(want, ctx);
    cap = want;
  }
  void ensure(const ns_request_t& r, const ns_bounds_t& b, context_t& ctx) {
    if ((size_t)r.count > seeds_cap) {
      size_t c0 = seeds_cap, c1 = seeds_cap;
      grow(d_seeds, c0, (size_t)r.count, ctx);
      grow(seed_local, c1, (size_t)r.count, ctx);
      seeds_cap = (size_t)r.count;
    }
    grow(vertices, vertices_cap, (size_t)b.vertices, ctx);
    grow(row_offsets, rows_cap, (size_t)b.rows + 1, ctx);
    if ((size_t)b.entries > entries_cap) {
      size_t c0 = entries_cap, c1 = entries_cap;
      grow(cols, c0, (size_t)b.entries, ctx);
      grow(entry_pos, c1, (size_t)b.entries, ctx);
      entries_cap = (size_t)b.entries;
    }
  }
  void nothing(const ns_request_t& r) {
    hop_offsets.assign((size_t)r.hops + 2, 0);
    edge_offsets.assign((size_t)r.hops + 1, 0);
    any_whole = false;
    seeds = r.count; edges = 0; device = false;
  }
  long long count_vertices() const { return hop_offsets.empty() ? 0 : hop_offsets.back(); }
  long long count_rows() const { return hop_offsets.size() < 2 ? 0 : hop_offsets[hop_offsets.size() - 2]; }
};

// (launches, host waits) of a fused run
inline void ns_fused_counts(long long n, const ns_request_t& r, long long& launches, long long& waits) {
  launches = waits = 0;
  if (n <= 0 || r.count == 0) return;
  launches = 5ll * r.hops + 4;
  waits = (r.h_seeds ? 1 : 0) + 1;
}

// The device state of a graph's fused sampling, and the run (host side).
struct ns_fused_state_t {
  int n = 0;
  long long m = 0;
  ns_opts_t opts;
  ns_results_t res;
  mem_t<u64> seen, fresh;
  mem_t<int> map, partials;
  mem_t<int2> items;
  mem_t<ns_control_t> ctl;
  pinned_t<ns_control_t> h_ctl;
  size_t partials_cap = 0, items_cap = 0;
  bool dirty = true;                 // seen / fresh may hold bits (before the first run; behind a run that failed)
  bool timing = false;
  double phase_ms[2] = {0.0, 0.0};   // the last timed run: sample, dedup
  std::vector<event_t> ev;
  long long bins[NS_BINS] = {0};

  ns_fused_state_t(int n_, long long m_, context_t&) : n(n_), m(m_), opts(ns_opts_t::from_env()) { h_ctl = pinned_t<ns_control_t>(1); }

  static int tiles_of(long long items) { return (int)((items + NS_TILE - 1) / NS_TILE); }

  // Returns the fourteen stats of mgx_nsample_run.
  std::vector<long long> run(const int* ro, const int* ci, const ns_request_t& r, const ns_bounds_t& b, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    long long launches = 0, waits = 0;
    phase_ms[0] = phase_ms[1] = 0.0;
    std::fill(bins, bins + NS_BINS, 0);
    if (n <= 0 || r.count == 0) {
      res.nothing(r);
      return {r.count, 0, r.hops, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    const size_t words = ((size_t)n + 63) / 64;
    res.ensure(r, b, ctx);
    if (seen.size() == 0) {
      seen = mem_t<u64>(words, ctx);
      fresh = mem_t<u64>(words, ctx);
      map = mem_t<int>((size_t)n, ctx);
      ctl = mem_t<ns_control_t>(1, ctx);
    }
    const size_t want_partials = (size_t)std::max(tiles_of((long long)words), tiles_of(b.front)) + 1;
    if (want_partials > partials_cap) { partials = mem_t<int>(); partials = mem_t<int>(want_partials, ctx); partials_cap = want_partials; }
    if ((size_t)b.items > items_cap) { items = mem_t<int2>(); items = mem_t<int2>((size_t)b.items, ctx); items_cap = (size_t)b.items; }
    if (timing) while (ev.size() < 2 * (size_t)r.hops + 3) ev.emplace_back();
    if (dirty) {
      MGX_HIP(hipMemsetAsync(seen.data(), 0, words * sizeof(u64), st));
      MGX_HIP(hipMemsetAsync(fresh.data(), 0, words * sizeof(u64), st));
    }
    dirty = true;
    MGX_HIP(hipMemsetAsync(ctl.data(), 0, sizeof(ns_control_t), st));
    if (r.h_seeds) { MGX_HIP(htod(res.d_seeds.data(), r.h_seeds, (size_t)r.count, st)); ++waits; }
    ns_args_t a;
    a.ro = ro; a.ci = ci;
    a.seeds = r.h_seeds ? res.d_seeds.data() : nullptr;
    a.ctl = ctl.data();
    a.seen = seen.data(); a.fresh = fresh.data(); a.map = map.data();
    a.vertices = res.vertices.data(); a.row_offsets = res.row_offsets.data(); a.cols = res.cols.data(); a.entry_pos = res.entry_pos.data();
    a.seed_local = res.seed_local.data();
    a.partials = partials.data();
    a.items = items.data();
    a.n = n; a.count = (int)r.count; a.hops = r.hops; a.item_cap = (int)items_cap;
    a.hop = 0; a.k = 0; a.group = 1; a.replace = r.replace; a.seed = r.seed;
    a.cuts = opts.cuts;
    const int cap = std::max(ctx.num_cus, 1) * 8;
    const int rank_blocks = std::min(std::max(tiles_of((long long)words), 1), cap);
    size_t stamp = 0;
    auto mark_time = [&]() { if (timing) MGX_HIP(hipEventRecord(ev[stamp++], st)); };
    auto rank = [&](int slot) {
      hipLaunchKernelGGL(k_ns_rank_count, dim3(rank_blocks), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_ns_rank_apply, dim3(rank_blocks), dim3(BLOCK), 0, st, a, slot);
      launches += 2;
    };
    mark_time();
    hipLaunchKernelGGL(k_ns_mark, dim3(grid_for(r.count, BLOCK, cap)), dim3(BLOCK), 0, st, a);
    ++launches;
    rank(0);
    for (int h = 0; h < r.hops; ++h) {
      mark_time();
      a.hop = h; a.k = r.fanouts[h]; a.group = ns_group(a.k);
      const long long passes = (b.F[h] * a.group + WAVE - 1) / WAVE;
      hipLaunchKernelGGL(k_ns_rows, dim3(std::min(std::max(tiles_of(b.F[h]), 1), cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_ns_sample, dim3(grid_for(passes, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_ns_long, dim3(a.k < 0 ? grid_for(b.items, WAVES_PER_BLOCK, cap) : 1), dim3(BLOCK), 0, st, a);
      launches += 3;
      mark_time();
      rank(h + 1);
    }
    mark_time();
    hipLaunchKernelGGL(k_ns_finish, dim3(grid_for(std::max(std::max(b.entries, b.vertices), r.count), BLOCK, cap)), dim3(BLOCK), 0, st, a);
    ++launches;
    mark_time();
    MGX_CHECK_LAUNCH("mgx nsample run");
    h_ctl.fetch(ctl.data(), 1, st);
    ++waits;
    dirty = false;
    const ns_control_t& c = *h_ctl.data();
    long long sum[NS_COUNTERS] = {0};
    for (int s = 0; s < NS_SLOTS; ++s)
      for (int i = 0; i < NS_COUNTERS; ++i) sum[i] += (long long)c.counters[s][i];
    res.hop_offsets.assign(c.hop_off, c.hop_off + r.hops + 2);
    res.edge_offsets.assign(c.edge_off, c.edge_off + r.hops + 1);
    res.any_whole = std::any_of(r.fanouts, r.fanouts + r.hops, [](int k) { return k < 0; });
    res.seeds = r.count; res.edges = c.edge_off[r.hops]; res.device = true;
    std::copy(c.bins, c.bins + NS_BINS, bins);
    if (timing) {
      for (size_t i = 0; i + 1 < stamp; ++i) {
        float ms = 0.f;
        MGX_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        phase_ms[(i % 2 == 1 && i + 2 < stamp) ? 0 : 1] += ms;     // (odd intervals are a hop's sampling, the last one is the finish)
      }
    }
    return {r.count, c.hop_off[1], r.hops, c.hop_off[r.hops + 1], c.hop_off[r.hops], c.edge_off[r.hops],
            sum[NS_C_EMPTY], sum[NS_C_WHOLE], sum[NS_C_SAMPLED], sum[NS_C_DRAWS], sum[NS_C_COLLISIONS], sum[NS_C_REVISITS], launches, waits};
  }
};

}  // namespace mgx
