// mgx/louvain_aggregate.hpp -- the contraction between two levels of the Louvain run: the communities of a level
// get dense ids in ascending order of their label, and the coarse graph gets one row per community, its columns ascending and
// unique, its weights the uint32 sums of the members' weights; the self entry (a, a) holds the internal weight, both directions.
//
//   renumber   flag[lab[v]] = 1, an exclusive scan of the flags is the dense id of every label; map[v] = dense[lab[v]]
//   count      cnt[a] += the entries v brings (level 0: its votes, self-loops dropped; coarse: its row), one atomic per vertex
//   fill       off = scan(cnt); a vertex takes its piece of its community's segment with one returning add and writes
//              (dense community of the neighbour, weight) there: the order inside a segment varies from run to run
//   order      segmented_sort over the segments, the weights riding along
//   reduce     a run of equal columns inside a segment is one coarse entry: head[p] = p starts a segment or its column differs
//              from the one before; an exclusive scan of the heads is every entry's place in the coarse row; the weights meet there
//              by integer atomicAdd, so the sums do not depend on the order the fill left
// Three host waits per contracted level: the communities, the sort's list sizes, the coarse entries.  Everything, the sort's lists
// and scratch copy included, is allocated once per handle, bounded by level 0's vertices and votes: a contraction allocates nothing.
#pragma once
#include <algorithm>
#include <climits>

#include "row_bodies.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "segsort.hpp"
#include "wave.hpp"

namespace mgx {

constexpr int LV_AGG_LANE_MAX = 32;           // rows of at most this many entries are written by their lane

struct lv_less_t {
  __device__ __forceinline__ bool operator()(int a, int b) const { return a < b; }
};

// the graph of a level: wt == nullptr is level 0 (every entry weighs 1, self-loops are dropped; co / ri: the genuine CSC, read
// when the caller's graph is not symmetric)
struct lv_graph_t {
  const int* ro;
  const int* ci;
  const unsigned* wt;
  const int* co;
  const int* ri;
  int n;
};

using lv_row_t = row_pair_t;
__device__ __forceinline__ lv_row_t lv_row(const lv_graph_t& g, bool valid, int v) { return row_pair_of(g.ro, g.co, g.co != nullptr, valid, v); }
// entry k of v's row: the neighbour, and its weight (0: a self-loop of level 0)
__device__ __forceinline__ int lv_entry(const lv_graph_t& g, const lv_row_t& r, int v, int k, unsigned* x) {
  const int u = k < r.olen ? g.ci[r.ob + k] : g.ri[r.ib + (k - r.olen)];
  *x = g.wt ? g.wt[r.ob + k] : (u != v ? 1u : 0u);
  return u;
}

__global__ __launch_bounds__(BLOCK) void k_lv_flag(const int* __restrict__ lab, int n, int* __restrict__ flag) {
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) flag[lab[v]] = 1;
}
// map[v] = the dense id of v's community; cnt[that] += the entries v brings (count != nullptr)
__global__ __launch_bounds__(BLOCK) void k_lv_map(lv_graph_t g, const int* __restrict__ lab, const int* __restrict__ dense,
                                                   const unsigned* __restrict__ k, int* __restrict__ map, int* __restrict__ cnt) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < g.n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const int a = dense[lab[v]];
    map[v] = a;
    const int c = g.wt ? g.ro[v + 1] - g.ro[v] : (int)k[v];
    if (cnt && c) atomicAdd(cnt + a, c);
  }
}
__global__ __launch_bounds__(BLOCK) void k_lv_compose(int* __restrict__ final_lab, const int* __restrict__ map, int n) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) final_lab[i] = map[final_lab[i]];
}

// a wave over 64 consecutive vertices: every vertex takes its piece of its community's segment and writes its entries there
__global__ __launch_bounds__(BLOCK) void k_lv_fill(lv_graph_t g, const int* __restrict__ map, const unsigned* __restrict__ k,
                                                    const int* __restrict__ off, int* __restrict__ cursor, int* __restrict__ keys,
                                                    unsigned* __restrict__ vals) {
  const int lane = lane_id();
  const unsigned wave = (blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE;
  const unsigned waves = gridDim.x * (unsigned)BLOCK / WAVE;
  for (unsigned base = wave * WAVE; base < (unsigned)g.n; base += waves * WAVE) {
    const bool in = base + lane < (unsigned)g.n;
    const int v = (int)(base + lane);
    const lv_row_t r = lv_row(g, in, v);
    const int len = r.len();
    const int c = !in ? 0 : (g.wt ? len : (int)k[v]);
    int pos = 0;
    if (c) {
      const int a = map[v];
      pos = off[a] + atomicAdd(cursor + a, c);
    }
    if (len <= LV_AGG_LANE_MAX)
      for (int j = 0; j < len; ++j) {
        unsigned x;
        const int u = lv_entry(g, r, v, j, &x);
        if (x) { keys[pos] = map[u]; vals[pos] = x; ++pos; }
      }
    for_each_wave_row(len > LV_AGG_LANE_MAX, [&](int src) {
      const lv_row_t rr = r.of_lane(src);
      const int vv = __shfl(v, src, WAVE);
      int p = __shfl(pos, src, WAVE);
      const int ll = rr.len();
      for (int j0 = 0; j0 < ll; j0 += WAVE) {
        unsigned x = 0;
        int u = vv;
        if (j0 + lane < ll) u = lv_entry(g, rr, vv, j0 + lane, &x);
        const u64 m = __ballot(x != 0);
        if (x) { keys[p + rank_in_mask(m)] = map[u]; vals[p + rank_in_mask(m)] = x; }
        p += __popcll(m);
      }
    });
  }
}

__global__ __launch_bounds__(BLOCK) void k_lv_starts(const int* __restrict__ off, int nc, int* __restrict__ isstart) {
  for (long long a = (long long)blockIdx.x * BLOCK + threadIdx.x; a < nc; a += (long long)gridDim.x * BLOCK)
    if (off[a] < off[a + 1]) isstart[off[a]] = 1;
}
__device__ __forceinline__ int lv_head(const int* keys, const int* isstart, long long p, long long total) {
  if (p >= total) return 0;
  return (isstart[p] || keys[p] != keys[p - 1]) ? 1 : 0;      // (p == 0 starts a segment: keys[-1] is not read)
}
__global__ __launch_bounds__(BLOCK) void k_lv_compact(const int* __restrict__ keys, const unsigned* __restrict__ vals,
                                                       const int* __restrict__ isstart, const int* __restrict__ idx, long long total,
                                                       int* __restrict__ ci, unsigned* __restrict__ wt) {
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * BLOCK) {
    const int h = lv_head(keys, isstart, p, total);
    const int out = idx[p] + h - 1;
    if (h) ci[out] = keys[p];
    atomicAdd(wt + out, vals[p]);
  }
}
__global__ __launch_bounds__(BLOCK) void k_lv_rows(const int* __restrict__ off, const int* __restrict__ idx, int nc, int* __restrict__ ro) {
  for (long long a = (long long)blockIdx.x * BLOCK + threadIdx.x; a <= nc; a += (long long)gridDim.x * BLOCK) ro[a] = idx[off[a]];
}

struct louvain_aggregate_t {
  int N = 0;                                  // level 0's vertices (at least 1)
  long long E = 0;                            // level 0's votes: no level has more entries
  mem_t<int> flag, dense, cnt, off, cursor, keys, isstart, idx;
  mem_t<unsigned> vals;
  segsort_workspace_t<int, unsigned> sort_ws;  // the sort's lists and scratch copy: a contraction allocates nothing
  long long waits = 0;

  louvain_aggregate_t(int n, long long votes, standard_context_t& ctx) : N(std::max(n, 1)), E(std::max<long long>(votes, 1)) {
    flag = mem_t<int>((size_t)N + 1, ctx);
    dense = mem_t<int>((size_t)N + 1, ctx);
    cnt = mem_t<int>((size_t)N + 1, ctx);
    off = mem_t<int>((size_t)N + 2, ctx);
    cursor = mem_t<int>((size_t)N, ctx);
    keys = mem_t<int>((size_t)E, ctx);
    vals = mem_t<unsigned>((size_t)E, ctx);
    isstart = mem_t<int>((size_t)E + 1, ctx);
    idx = mem_t<int>((size_t)E + 1, ctx);
    sort_ws = segsort_workspace_t<int, unsigned>(E, N, ctx);
    ctx.reserve_scratch(scan_scratch_bytes(std::max<long long>(N, E) + 2));
  }

  // dense ids for the labels of level `g` (lab: g.n labels in [0, g.n)) -> map (g.n ints), composed into final_lab (n0 ints)
  // unless first (then final_lab = map).  Returns the communities.  One host wait.
  int renumber(const lv_graph_t& g, const int* lab, const unsigned* k, int* map, int* final_lab, int n0, bool first, bool count,
               standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int n = g.n;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8);
    MGX_HIP(hipMemsetAsync(flag.data(), 0, ((size_t)n + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_lv_flag, dim3(blocks), dim3(BLOCK), 0, st, lab, n, flag.data());
    long long nc = 0;
    const int* const f = flag.data();
    transform_scan([=] __device__(long long i) { return i < n ? f[i] : 0; }, (long long)n + 1, dense.data(), ctx, &nc);
    ++waits;
    if (count) MGX_HIP(hipMemsetAsync(cnt.data(), 0, ((size_t)nc + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_lv_map, dim3(blocks), dim3(BLOCK), 0, st, g, lab, (const int*)dense.data(), k, map, count ? cnt.data() : (int*)nullptr);
    if (first) MGX_HIP(dtod(final_lab, (const int*)map, (size_t)n0, st));
    else hipLaunchKernelGGL(k_lv_compose, dim3(grid_for(n0, BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(BLOCK), 0, st, final_lab, (const int*)map, n0);
    MGX_CHECK_LAUNCH("mgx louvain renumber");
    return (int)nc;
  }

  // the coarse graph of `map` (renumber with count = true ran before): nc rows into ro (nc + 1), ci and wt (`total` at most).
  // total: the entries the level brings (level 0: W; coarse: its entries).  Returns the coarse entries.
  long long contract(const lv_graph_t& g, const int* map, const unsigned* k, int nc, long long total, int* ro, int* ci, unsigned* wt,
                     standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    if (total > INT_MAX - 1) throw mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx louvain: the contraction's positions are int32");      // (refused before the run: mgx_louvain_run)
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const int* const c = cnt.data();
    transform_scan([=] __device__(long long i) { return i < nc ? c[i] : 0; }, (long long)nc + 1, off.data(), ctx, nullptr);
    MGX_HIP(hipMemsetAsync(cursor.data(), 0, (size_t)nc * sizeof(int), st));
    hipLaunchKernelGGL(k_lv_fill, dim3(grid_for(g.n, WAVE, max_blocks)), dim3(BLOCK), 0, st, g, map, k, (const int*)off.data(), cursor.data(),
                       keys.data(), vals.data());
    MGX_CHECK_LAUNCH("mgx louvain fill");
    segmented_sort_impl<int, unsigned, lv_less_t>(keys.data(), vals.data(), total, off.data() + 1, nc - 1, lv_less_t(), ctx, &sort_ws);
    ++waits;
    MGX_HIP(hipMemsetAsync(isstart.data(), 0, ((size_t)total + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_lv_starts, dim3(grid_for(nc, BLOCK, max_blocks)), dim3(BLOCK), 0, st, (const int*)off.data(), nc, isstart.data());
    long long nnz = 0;
    const int* const kk = keys.data();
    const int* const ss = isstart.data();
    transform_scan([=] __device__(long long p) { return lv_head(kk, ss, p, total); }, total + 1, idx.data(), ctx, &nnz);
    ++waits;
    MGX_HIP(hipMemsetAsync(wt, 0, (size_t)nnz * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_lv_compact, dim3(grid_for(total, BLOCK, max_blocks)), dim3(BLOCK), 0, st, kk, (const unsigned*)vals.data(), ss,
                       (const int*)idx.data(), total, ci, wt);
    hipLaunchKernelGGL(k_lv_rows, dim3(grid_for((long long)nc + 1, BLOCK, max_blocks)), dim3(BLOCK), 0, st, (const int*)off.data(),
                       (const int*)idx.data(), nc, ro);
    MGX_CHECK_LAUNCH("mgx louvain contract");
    return nnz;
  }
};

}  // namespace mgx
