// mgx/pagerank_fused.hpp -- PageRank to convergence, fused (mgx_pagerank_run): the iterations run on the device, the host
// enqueues them in batches and looks once per batch.
//
// The definition (the operator path include/gunrock/pagerank/ and tests/pagerank_model.py compute the same):
//   CSR entry (u, v) is an edge u -> v, duplicates count once each, self-loops count; d(u) = length of row u, a = damping
//     r_0[v]     = 1 / n
//     D_t        = sum of r_t[u] over the u with d(u) = 0                       (dangling mass)
//     S_t[v]     = sum of r_t[u] / d(u) over the entries (u, v)                 (in-entries of v, with multiplicity)
//     r_{t+1}[v] = (1 - a) / n + a * (S_t[v] + D_t / n)
//     e_{t+1}    = sum over v of | r_{t+1}[v] - r_t[v] |                        (L1 residual)
//   stop after the first iteration t + 1 with e_{t+1} <= tol ("converged") or after max_iter iterations.
//   Ranks, contributions r / d and S are float; D and e are accumulated in double.
//
// An iteration is three or four launches:
//   reduce   S[v] from the contributions.  Two shapes:
//            layout  (symmetric graph that carries the hub-first layout with its sliced long rows): k_nrs_edges + k_nrs_fold of
//                    mgx/nreduce.hpp, driven directly.  Everything of the run -- ranks, contributions, S -- lives in LAYOUT order
//                    (the kernels are handed an identity map where they expect old_of_new), so the values pass and its gather
//                    through old_of_new (k_nr_values) are not paid: the update below writes the contributions where the reduce
//                    reads its vals[].  The ranks are brought back to original ids once, at the end of the run.
//            general (no layout, or the in-entries of a directed graph from its genuine CSC): k_pagerank_reduce over the plain
//                    offsets / indices -- rows of up to PGR_LANE_MAX entries a lane each, longer ones a wave each, rows of at
//                    least PGR_HUGE_MIN entries a workgroup each (k_pagerank_reduce_huge, from a list made at the start of the
//                    run).  Every row is folded in an order that depends on the row alone.
//   update   k_pagerank_update, per vertex: the new rank from S, D / n and the base; |new - old| and, for a vertex without
//            out-entries, the new rank into the workgroup's two double sums; the next contribution r / d.  The two sums leave
//            the workgroup as ONE double each (no float atomics, no same-address atomics: nreduce.hpp:138-139).
//   verdict  k_pagerank_verdict, one workgroup: adds the workgroups' partials in a fixed order -> e, the next D; stores e into
//            the trace; sets the control block's `done` word when e <= tol or the iteration count reaches max_iter.
// The grid of the update depends on n and the device alone, so two runs with the same arguments add the same numbers in the
// same order: ranks and residuals are bit-equal from run to run, on both reduce shapes.
//
// Termination: every kernel returns at once when it finds done != 0 (the sliced kernels through their dev_flag / epoch pair:
// dev_flag = &done, epoch = 1), so the iterations enqueued behind the last one cost a launch each and change nothing.
// Batches: the first is PGR_FIRST_BATCH iterations; after a look that found the run unfinished the host sizes the next one from
// the last two residuals, log(tol / e) / log(e / e_prev) + PGR_BATCH_SLACK, clamped to [PGR_MIN_BATCH, PGR_MAX_BATCH]
// (PGR_MAX_BATCH when tol = 0 or the residuals did not fall).  A run of max_iter iterations therefore makes at most
// 1 + ceil((max_iter - PGR_FIRST_BATCH) / PGR_MIN_BATCH) looks, and exactly one when max_iter <= PGR_FIRST_BATCH.  A look is
// a copy of the control block (80 bytes) to pinned memory and a stream wait.
// The residual trace e_1 .. e_T holds at most PGR_TRACE_CAP entries (later iterations run, their residuals are not kept).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "nreduce.hpp"
#include "runtime.hpp"
#include "wave.hpp"

namespace mgx {

constexpr int PGR_LANE_MAX = 16;          // general reduce: rows of at most this many entries are summed by one lane
constexpr int PGR_HUGE_MIN = 8192;        // ... of at least this many by a workgroup; the others by a wave
constexpr int PGR_HUGE_BLOCKS = 64;       // workgroups of the huge rows' launch (they stride over the list)
constexpr int PGR_FIRST_BATCH = 32;       // iterations enqueued before the first look
constexpr int PGR_MIN_BATCH = 8, PGR_MAX_BATCH = 256, PGR_BATCH_SLACK = 2;
constexpr int PGR_TRACE_CAP = 1 << 16;    // residuals kept per run
constexpr int PGR_MAX_PARTIALS = 4096;    // workgroups of the update at most (a partial pair each)

// the control block on the device (copied to the host at every look)
struct pagerank_ctrl_t {
  u32 done;                 // != 0: the run is over, every later launch returns at once
  u32 converged;
  int iterations;           // iterations run so far
  int max_iter;
  int trace_cap;
  int huge_rows;            // rows in the huge list (general reduce)
  long long dangling;       // vertices without out-entries
  double tol;
  double D;                 // dangling mass of the current ranks
  double e, e_prev;         // residuals of the last two iterations
  double alpha, base;       // damping, (1 - alpha) / n
};

// a workgroup's double sums -> one value in thread 0 (fixed order: lanes by xor-shuffle, then the waves ascending)
__device__ __forceinline__ double pgr_block_sum(double x, double* s_w) {
  x = wave_sum(x);
  if (lane_id() == 0) s_w[threadIdx.x / WAVE] = x;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    t = s_w[0];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) t += s_w[w];
  }
  __syncthreads();
  return t;
}

// r_0, its contributions and its dangling mass; off: the offsets whose differences are the OUT-degrees, in the order the run lives in
__global__ __launch_bounds__(BLOCK) void k_pagerank_init(const int* __restrict__ off, float* __restrict__ rank, float* __restrict__ contrib,
                                                         int n, double* __restrict__ part_d, long long* __restrict__ part_cnt) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  const float r0 = (float)(1.0 / (double)n);
  double dsum = 0.0, cnt = 0.0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int d = off[i + 1] - off[i];
    rank[i] = r0;
    contrib[i] = d > 0 ? r0 / (float)d : 0.0f;
    if (d <= 0) { dsum += (double)r0; cnt += 1.0; }
  }
  const double bd = pgr_block_sum(dsum, s_w);
  const double bc = pgr_block_sum(cnt, s_w);           // (exact: a count below 2^53)
  if (threadIdx.x == 0) { part_d[blockIdx.x] = bd; part_cnt[blockIdx.x] = (long long)bc; }
}

// one workgroup: the control block of a new run, with the partials of the init launch -> D_0 and the dangling count
__global__ __launch_bounds__(BLOCK) void k_pagerank_begin(pagerank_ctrl_t* c, pagerank_ctrl_t fresh, const double* __restrict__ part_d,
                                                          const long long* __restrict__ part_cnt, int parts) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  double d = 0.0, k = 0.0;
  for (int i = threadIdx.x; i < parts; i += BLOCK) { d += part_d[i]; k += (double)part_cnt[i]; }
  d = pgr_block_sum(d, s_w);
  k = pgr_block_sum(k, s_w);
  if (threadIdx.x == 0) {
    fresh.D = d;
    fresh.dangling = (long long)k;
    *c = fresh;
  }
}

// general reduce: S[v] = sum of vals[idx[e]] over e in [off[v], off[v + 1])
__global__ __launch_bounds__(BLOCK) void k_pagerank_reduce(const int* __restrict__ off, const int* __restrict__ idx, const float* __restrict__ vals,
                                                           float* __restrict__ S, int n, const pagerank_ctrl_t* c) {
  if (c->done) return;                                 // (grid-uniform)
  const int lane = lane_id();
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) / WAVE, waves = (long long)gridDim.x * WAVES_PER_BLOCK;
  for (long long base = wave * WAVE; base < n; base += waves * WAVE) {
    const long long v = base + lane;
    const bool in = v < n;
    const int beg = in ? off[v] : 0, end = in ? off[v + 1] : 0;
    const int len = end - beg;
    if (in && len <= PGR_LANE_MAX) {
      float a = 0.0f;
      for (int e = beg; e < end; ++e) a += vals[idx[e]];
      S[v] = a;
    }
    u64 m = __ballot(in && len > PGR_LANE_MAX && len < PGR_HUGE_MIN);
    while (m) {                                        // (wave-uniform)
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int b = __shfl(beg, l, WAVE), e1 = __shfl(end, l, WAVE);
      float a0 = 0.0f, a1 = 0.0f;
      int e = b + lane;
      for (; e + WAVE < e1; e += 2 * WAVE) {
        const float x0 = vals[idx[e]], x1 = vals[idx[e + WAVE]];
        a0 += x0; a1 += x1;
      }
      if (e < e1) a0 += vals[idx[e]];
      const float a = wave_sum(a0 + a1);
      if (lane == 0) S[base + l] = a;
    }
  }
}

// the rows of at least PGR_HUGE_MIN entries (their order in the list is arbitrary; a row's sum does not depend on it)
__global__ __launch_bounds__(BLOCK) void k_pagerank_huge_list(const int* __restrict__ off, int n, int* __restrict__ list, int cap, pagerank_ctrl_t* c) {
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) {
    if (off[v + 1] - off[v] >= PGR_HUGE_MIN) {
      const int at = atomicAdd(&c->huge_rows, 1);
      if (at < cap) list[at] = (int)v;
    }
  }
}
__global__ __launch_bounds__(BLOCK) void k_pagerank_reduce_huge(const int* __restrict__ off, const int* __restrict__ idx, const float* __restrict__ vals,
                                                                float* __restrict__ S, const int* __restrict__ list, int cap, const pagerank_ctrl_t* c) {
  __shared__ float s_w[WAVES_PER_BLOCK];
  if (c->done) return;
  const int rows = min(c->huge_rows, cap);
  for (int i = blockIdx.x; i < rows; i += gridDim.x) {       // (workgroup-uniform)
    const int v = list[i];
    const int b = off[v], e1 = off[v + 1];
    float a0 = 0.0f, a1 = 0.0f;
    int e = b + (int)threadIdx.x;
    for (; e + BLOCK < e1; e += 2 * BLOCK) {
      const float x0 = vals[idx[e]], x1 = vals[idx[e + BLOCK]];
      a0 += x0; a1 += x1;
    }
    if (e < e1) a0 += vals[idx[e]];
    const float a = wave_sum(a0 + a1);
    if (lane_id() == 0) s_w[threadIdx.x / WAVE] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = s_w[0];
#pragma unroll
      for (int w = 1; w < WAVES_PER_BLOCK; ++w) t += s_w[w];
      S[v] = t;
    }
    __syncthreads();
  }
}

// the update of one iteration (see the head of the file); off as for k_pagerank_init
__global__ __launch_bounds__(BLOCK) void k_pagerank_update(const int* __restrict__ off, const float* __restrict__ S, float* __restrict__ rank,
                                                           float* __restrict__ contrib, int n, const pagerank_ctrl_t* c,
                                                           double* __restrict__ part_e, double* __restrict__ part_d) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  if (c->done) return;
  const double alpha = c->alpha, base = c->base, share = c->D / (double)n;
  double esum = 0.0, dsum = 0.0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int d = off[i + 1] - off[i];
    const float old = rank[i];
    const float now = (float)(base + alpha * ((double)S[i] + share));
    rank[i] = now;
    contrib[i] = d > 0 ? now / (float)d : 0.0f;
    esum += fabs((double)now - (double)old);
    if (d <= 0) dsum += (double)now;
  }
  const double be = pgr_block_sum(esum, s_w);
  const double bd = pgr_block_sum(dsum, s_w);
  if (threadIdx.x == 0) { part_e[blockIdx.x] = be; part_d[blockIdx.x] = bd; }
}

// one workgroup: the update's partials in a fixed order -> e, D; the trace; the verdict
__global__ __launch_bounds__(BLOCK) void k_pagerank_verdict(pagerank_ctrl_t* c, const double* __restrict__ part_e, const double* __restrict__ part_d,
                                                            int parts, double* __restrict__ trace) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  if (c->done) return;
  double e = 0.0, d = 0.0;
  for (int i = threadIdx.x; i < parts; i += BLOCK) { e += part_e[i]; d += part_d[i]; }
  e = pgr_block_sum(e, s_w);
  d = pgr_block_sum(d, s_w);
  if (threadIdx.x == 0) {
    const int it = c->iterations + 1;
    c->iterations = it;
    c->e_prev = c->e;
    c->e = e;
    c->D = d;
    if (it <= c->trace_cap) trace[it - 1] = e;
    if (e <= c->tol) { c->converged = 1u; c->done = 1u; }
    else if (it >= c->max_iter) c->done = 1u;
  }
}

// layout order -> original ids, once per run
__global__ __launch_bounds__(BLOCK) void k_pagerank_unpermute(const float* __restrict__ rank, const int* __restrict__ old_of_new, float* __restrict__ out, int n) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) out[old_of_new[i]] = rank[i];
}
__global__ __launch_bounds__(BLOCK) void k_pagerank_iota(int* out, int n) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) out[i] = (int)i;
}

// What a run reads of the graph.  in_off / in_idx: the rows that hold the in-entries (the CSR's own when the graph is symmetric,
// else its genuine CSC); out_off: the CSR's offsets (out-degrees).  layout != nullptr: the layout reduce -- *layout filled as for
// nr_full_frontier with its sliced long rows (nrs_mu != nullptr), the graph symmetric, the context's arena at least
// nr_scratch_bytes(n, nrs units, 4); old_of_new then brings the ranks back.
struct pagerank_graph_t {
  const int* in_off = nullptr;
  const int* in_idx = nullptr;
  const int* out_off = nullptr;
  long long in_entries = 0;
  const nr_layout_t* layout = nullptr;
  const int* old_of_new = nullptr;
};

struct pagerank_stats_t {
  long long iterations = 0, converged = 0, dangling = 0, layout_path = 0, waits = 0, launches = 0;
  double residual = 0.0;
};

// The device state of a graph's PageRank runs.  Also serves the operator path (include/gunrock/pagerank/), which shares the
// update, the verdict and the control block and brings its own reduce.
struct pagerank_state_t {
  int n = 0;
  mem_t<float> rank, contrib, S;     // in the order the run lives in
  mem_t<float> rank_orig;            // layout runs: the ranks by original id (allocated at the first such run)
  mem_t<int> iota;                   // layout runs: what the sliced kernels get as old_of_new
  mem_t<int> huge;                   // general runs: the huge rows
  mem_t<double> part;                // 2 x PGR_MAX_PARTIALS
  mem_t<long long> part_cnt;
  mem_t<double> trace;
  mem_t<pagerank_ctrl_t> ctrl;
  pinned_t<pagerank_ctrl_t> h_ctrl;
  const float* result = nullptr;     // the last run's ranks by original id (nullptr: no run yet)
  int trace_cap = 0;
  int last_iterations = 0;
  int last_huge_rows = -1;           // the last fused run's huge list (0 after a layout run; -1: no fused run yet)

  pagerank_state_t(int n_, context_t& ctx) : n(n_) {
    const size_t N = (size_t)std::max(n, 1);
    rank = mem_t<float>(N, ctx);
    contrib = mem_t<float>(N + 64, ctx);      // (the sliced kernels' tables read whole slices: room behind the last value)
    S = mem_t<float>(N, ctx);
    part = mem_t<double>(2 * (size_t)PGR_MAX_PARTIALS, ctx);
    part_cnt = mem_t<long long>((size_t)PGR_MAX_PARTIALS, ctx);
    ctrl = mem_t<pagerank_ctrl_t>(1, ctx);
    h_ctrl = pinned_t<pagerank_ctrl_t>(1);
  }

  int update_grid(const standard_context_t& ctx) const { return grid_for(n, BLOCK, std::min(std::max(ctx.num_cus, 1) * 8, PGR_MAX_PARTIALS)); }

  // r_0, D_0, a cleared S and control block: the start of a run of either path (asynchronous).  off: out-degrees' offsets in the
  // run's order.  Returns the launches enqueued.
  int begin(const int* off, double alpha, double tol, int max_iter, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int want = std::min(max_iter, PGR_TRACE_CAP);
    if (want > trace_cap) {
      MGX_HIP(hipStreamSynchronize(st));
      trace = mem_t<double>((size_t)want, ctx);
      trace_cap = want;
    }
    result = nullptr;
    pagerank_ctrl_t c = {};
    c.max_iter = max_iter; c.trace_cap = trace_cap; c.tol = tol; c.alpha = alpha; c.base = (1.0 - alpha) / (double)n;
    MGX_HIP(hipMemsetAsync(S.data(), 0, (size_t)n * sizeof(float), st));
    const int grid = update_grid(ctx);
    hipLaunchKernelGGL(k_pagerank_init, dim3(grid), dim3(BLOCK), 0, st, off, rank.data(), contrib.data(), n, part.data(), part_cnt.data());
    hipLaunchKernelGGL(k_pagerank_begin, dim3(1), dim3(BLOCK), 0, st, ctrl.data(), c, (const double*)part.data(), (const long long*)part_cnt.data(), grid);
    return 2;
  }
  // update + verdict of one iteration (asynchronous); returns the launches enqueued
  int step(const int* off, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int grid = update_grid(ctx);
    hipLaunchKernelGGL(k_pagerank_update, dim3(grid), dim3(BLOCK), 0, st, off, (const float*)S.data(), rank.data(), contrib.data(), n,
                       (const pagerank_ctrl_t*)ctrl.data(), part.data(), part.data() + PGR_MAX_PARTIALS);
    hipLaunchKernelGGL(k_pagerank_verdict, dim3(1), dim3(BLOCK), 0, st, ctrl.data(), (const double*)part.data(),
                       (const double*)(part.data() + PGR_MAX_PARTIALS), grid, trace.data());
    return 2;
  }
  // the control block to the host: one wait
  const pagerank_ctrl_t& look(standard_context_t& ctx) {
    h_ctrl.fetch(ctrl.data(), 1, ctx.stream());
    return h_ctrl[0];
  }

  // iterations to enqueue after a look that found the run unfinished
  static int next_batch(const pagerank_ctrl_t& c) {
    int b = PGR_MAX_BATCH;
    if (c.tol > 0.0 && c.e > c.tol && c.e_prev > c.e && c.iterations >= 2) {
      const double need = std::log(c.tol / c.e) / std::log(c.e / c.e_prev);
      if (need < (double)PGR_MAX_BATCH) b = (int)std::ceil(need) + PGR_BATCH_SLACK;
    }
    return std::min(std::max(b, PGR_MIN_BATCH), PGR_MAX_BATCH);
  }

  pagerank_stats_t run(const pagerank_graph_t& g, double alpha, double tol, int max_iter, standard_context_t& ctx) {
    pagerank_stats_t out;
    if (n <= 0) { out.converged = 1; return out; }
    const hipStream_t st = ctx.stream();
    const bool layout = g.layout != nullptr;
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const int grid_n = grid_for(n, BLOCK, max_blocks);
    nr_layout_t L;
    u32 fold_grid = 0;
    float* partial = nullptr;
    const int* off = g.out_off;
    int huge_cap = 0;
    if (layout) {
      L = *g.layout;
      off = (const int*)L.row_offsets;
      if (iota.size() < (size_t)n) {
        iota = mem_t<int>((size_t)n, ctx);
        rank_orig = mem_t<float>((size_t)n, ctx);
        hipLaunchKernelGGL(k_pagerank_iota, dim3(grid_n), dim3(BLOCK), 0, st, iota.data(), n);
      }
      L.old_of_new = iota.data();
      L.pos = nullptr;
      L.parts = 3u;
      partial = (float*)((char*)ctx.scratch + (((size_t)L.n + 64) * sizeof(float) + 255) / 256 * 256);    // (where nr_full_frontier keeps them)
      ++ctx.scratch_epoch;
      static unsigned char seen[64] = {};
      if (device_once_t once{seen})
        MGX_HIP(hipFuncSetAttribute((const void*)(k_nrs_edges<float, plus_t<float>, 1024>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      fold_grid = L.nrs_tier[0] + (L.nrs_tier[1] - L.nrs_tier[0] + BLOCK / WAVE - 1) / (BLOCK / WAVE) +
                  (L.nrs_tier[2] - L.nrs_tier[1] + BLOCK / 8 - 1) / (BLOCK / 8) + (L.nrs_rows - L.nrs_tier[2] + BLOCK - 1) / BLOCK;
    } else {
      huge_cap = (int)std::min<long long>(g.in_entries / PGR_HUGE_MIN + 1, (long long)n);
      if (huge.size() < (size_t)huge_cap) {
        MGX_HIP(hipStreamSynchronize(st));
        huge = mem_t<int>((size_t)huge_cap, ctx);
      }
    }
    out.launches += begin(off, alpha, tol, max_iter, ctx);
    if (!layout) {
      hipLaunchKernelGGL(k_pagerank_huge_list, dim3(grid_n), dim3(BLOCK), 0, st, g.in_off, n, huge.data(), huge_cap, ctrl.data());
      ++out.launches;
    }
    const u32* const done = &ctrl.data()->done;
    int enqueued = 0, batch = std::min(max_iter, PGR_FIRST_BATCH);
    for (;;) {
      for (int i = 0; i < batch; ++i) {
        if (layout) {
          hipLaunchKernelGGL((k_nrs_edges<float, plus_t<float>, 1024>), dim3(ctx.num_cus), dim3(1024), nr_lds_bytes(), st, L, (const float*)contrib.data(),
                             partial, S.data(), 0.0f, plus_t<float>(), done, 1u);
          ++out.launches;
          if (fold_grid) {
            if (L.nrs_slices + 1u <= (u32)NRS_FOLD_CHUNK)
              hipLaunchKernelGGL((k_nrs_fold<float, plus_t<float>, false>), dim3(fold_grid), dim3(BLOCK), 0, st, L, (const float*)partial, S.data(), 0.0f,
                                 plus_t<float>(), done, 1u);
            else
              hipLaunchKernelGGL((k_nrs_fold<float, plus_t<float>, true>), dim3(fold_grid), dim3(BLOCK), 0, st, L, (const float*)partial, S.data(), 0.0f,
                                 plus_t<float>(), done, 1u);
            ++out.launches;
          }
        } else {
          hipLaunchKernelGGL(k_pagerank_reduce, dim3(grid_n), dim3(BLOCK), 0, st, g.in_off, g.in_idx, (const float*)contrib.data(), S.data(), n,
                             (const pagerank_ctrl_t*)ctrl.data());
          hipLaunchKernelGGL(k_pagerank_reduce_huge, dim3(PGR_HUGE_BLOCKS), dim3(BLOCK), 0, st, g.in_off, g.in_idx, (const float*)contrib.data(), S.data(),
                             (const int*)huge.data(), huge_cap, (const pagerank_ctrl_t*)ctrl.data());
          out.launches += 2;
        }
        out.launches += step(off, ctx);
      }
      enqueued += batch;
      MGX_CHECK_LAUNCH("mgx pagerank run");
      const pagerank_ctrl_t& c = look(ctx);
      ++out.waits;
      if (c.done || enqueued >= max_iter) break;
      batch = std::min(next_batch(c), max_iter - enqueued);
    }
    const pagerank_ctrl_t& c = h_ctrl[0];
    if (layout) {
      hipLaunchKernelGGL(k_pagerank_unpermute, dim3(grid_n), dim3(BLOCK), 0, st, (const float*)rank.data(), g.old_of_new, rank_orig.data(), n);
      ++out.launches;
      MGX_CHECK_LAUNCH("mgx pagerank run");
      result = rank_orig.data();
    } else {
      result = rank.data();
    }
    last_iterations = c.iterations;
    last_huge_rows = layout ? 0 : c.huge_rows;
    out.iterations = c.iterations; out.converged = c.converged; out.dangling = c.dangling; out.layout_path = layout ? 1 : 0;
    out.residual = c.e;
    return out;
  }

  // which class took the rows of the last fused run, and the constants that draw the classes (mgx_pagerank_bins); reports only
  std::vector<long long> bins() const { return {last_huge_rows, PGR_LANE_MAX, PGR_HUGE_MIN, PGR_HUGE_BLOCKS}; }
};

}  // namespace mgx
