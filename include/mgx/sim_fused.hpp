// mgx/sim_fused.hpp -- vertex similarity for link prediction, fused (mgx_sim_run): the common neighbours of arbitrary vertex pairs
// and the scores made of them (Jaccard, overlap, Sorensen, cosine, a weighted sum: Adamic-Adar, resource allocation).
//
// The definition (the operator path include/gunrock/sim/ and tests/sim_model.py compute the same):
//   the graph is the underlying simple undirected graph of DESIGN 3.10: N(v) = the distinct neighbours of v other than v, original
//   ids, d(v) = |N(v)| = sdeg[v].  A run takes P pairs (u[p], v[p]); without pairs it runs EDGES MODE: the pairs are the m_dag edges
//   in the order of mgx_ktruss_edges.  c = |N(u) & N(v)|; common[p] = c always; score[p] by the measure (sim_score below; WEIGHTED:
//   the sum of x[w] over the common w).  u == v is legal (c = d(u)), duplicates are legal, an id outside [0, n) is found by the
//   classifying launch and makes the run MGX_E_INVALID.
// The adjacency is k-truss's (ktruss_fused.hpp: ensure_graph), built once per `symmetric` value and kept on the handle: the builder
// is CALLED, so this handle carries adj_eid and the peel's arrays unused (DESIGN 3.22 says what that costs).
// The launches of a run, enqueued back to back behind the pairs' upload, and one read-back of the control words:
//   k_sim_classify  ids checked, la = the shorter row's length, lb = the longer's (equal: the smaller id's row plays the shorter
//                   one, so that (u, v) and (v, u) run the same code on the same rows); la == 0: c = 0 written here; else the pair
//                   index goes to one of four work lists (worklist.hpp: wave-private LDS stages)
//   k_sim_lane      la <= short_max: a lane per pair; every entry of the short row is binary-searched in the long one, each search
//                   starting where the last one ended: la log lb loads whatever lb is (a leaf against a hub)
//   k_sim_probe     longer short rows against rows of at least probe_ratio x la: a group of 16 lanes per pair, consecutive lanes
//                   consecutive entries of the short row, each searching the long row in global memory; hits by ballot and popcount
//   k_sim_wave      la <= wave_max: the short row goes to a wave's LDS stage once, the long row is streamed, consecutive lanes
//   k_sim_block     consecutive entries, each lane searching LDS; longer: the same body (sim_staged_pair) by a workgroup.  A short
//                   row longer than the stage is staged chunk by chunk: both rows ascend, so a chunk spanning [lo, hi] needs only
//                   the slice of the long row within [lo, hi], found by two binary searches: the long row is streamed ONCE in total
//   k_sim_score     the four ratios from c and the two degrees (one correctly rounded division each), and the run's sums
// The pair kernels run over chip-sized grids and read the lists' sizes on the device; every array is sized from P on the host.
// WEIGHTED: no float atomics, one owner writes each pair.  x[w] is gathered on a hit only and summed per lane in entry order (long
// row entry k is always lane k mod TEAM's), then over the team by a fixed tree (the xor butterfly; a workgroup: its four waves in
// order), then over the chunks in chunk order: two runs are bit-equal.
// No grid barrier, no cooperative launch, no inline assembly, no scratch.
// Not built: pairs sorted by u so that one staged row serves many partners, a two-hop all-pairs top-k, a pair split
// across workgroups, edges mode from the oriented supports, more than one device.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "env.hpp"
#include "ktruss_fused.hpp"
#include "runtime.hpp"
#include "tc_fused.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

enum : int { SIM_COMMON = 0, SIM_JACCARD = 1, SIM_OVERLAP = 2, SIM_SORENSEN = 3, SIM_COSINE = 4, SIM_WEIGHTED = 5, SIM_MEASURES = 6 };
enum : int { SIM_NONE = 0, SIM_LANE = 1, SIM_PROBE = 2, SIM_WAVE = 3, SIM_BLOCK = 4, SIM_CLASSES = 5 };
// (short_max and wave_max are unmeasured guesses; the ratio is where PROBE and WAVE crossed at la = 256 on an MI355X: PROBE took
//  1.08 of WAVE's time at lb = 4 la and 0.90 at 8 la -- DESIGN 3.22)
constexpr int SIM_SHORT_MAX_DEFAULT = 16;
constexpr int SIM_PROBE_RATIO_DEFAULT = 8;
constexpr int SIM_WAVE_MAX_DEFAULT = 512;
constexpr int SIM_WAVE_STAGE = 512;            // entries of a wave's LDS stage
constexpr int SIM_BLOCK_STAGE = 4096;          // of a workgroup's
constexpr int SIM_GROUP = 16;                  // lanes of a PROBE pair
constexpr int SIM_APPEND_STAGE = 2 * WAVE;     // a wave's LDS stage of list appends
constexpr int SIM_STATS = 8;

struct sim_opts_t {
  int short_max = SIM_SHORT_MAX_DEFAULT, probe_ratio = SIM_PROBE_RATIO_DEFAULT, wave_max = SIM_WAVE_MAX_DEFAULT, stage = SIM_BLOCK_STAGE;
  static sim_opts_t from_env() {
    sim_opts_t o;
    o.short_max = env_int("MGX_SIM_SHORT_MAX", 0, INT_MAX, o.short_max);
    o.probe_ratio = env_int("MGX_SIM_PROBE_RATIO", 1, INT_MAX, o.probe_ratio);
    o.wave_max = env_int("MGX_SIM_WAVE_MAX", 0, INT_MAX, o.wave_max);
    o.stage = env_int("MGX_SIM_STAGE", 1, SIM_BLOCK_STAGE, o.stage);
    return o;
  }
};

// ---- what both paths and the model share ----
// the class of a pair by its row lengths, la <= lb
__host__ __device__ __forceinline__ int sim_class(int la, int lb, const sim_opts_t& o) {
  if (la == 0) return SIM_NONE;
  if (la <= o.short_max) return SIM_LANE;
  if ((long long)lb >= (long long)o.probe_ratio * la) return SIM_PROBE;
  return la <= o.wave_max ? SIM_WAVE : SIM_BLOCK;
}
// the score of a pair with c common neighbours and degrees du, dv: every ratio is one round-to-nearest division of integers that
// a double holds exactly (c, du, dv < 2^31); the cosine's product is one rounded multiplication, its root HIP's sqrt
__host__ __device__ __forceinline__ double sim_score(int measure, long long c, long long du, long long dv) {
  switch (measure) {
    case SIM_JACCARD: {
      const long long d = du + dv - c;
      return d ? (double)c / (double)d : 0.0;
    }
    case SIM_OVERLAP: {
      const long long d = du < dv ? du : dv;
      return d ? (double)c / (double)d : 0.0;
    }
    case SIM_SORENSEN: {
      const long long d = du + dv;
      return d ? (double)(2 * c) / (double)d : 0.0;
    }
    case SIM_COSINE: return du && dv ? (double)c / sqrt((double)du * (double)dv) : 0.0;
    default: return (double)c;
  }
}

// the run's words in device memory
struct sim_control_t {
  int n_list[4];                 // pairs in the LANE, PROBE, WAVE and BLOCK lists
  int err;                       // an id outside [0, n)
  int maxrow;                    // the longest simple row (copied from the graph's word by k_sim_score)
  u64 bins[SIM_CLASSES];
  u64 entries_read, sum_c, positive;
};

struct sim_args_t {
  const int* ro;                 // the sorted simple adjacency
  const int* ci;
  const int* u;                  // the pairs
  const int* v;
  const double* x;               // WEIGHTED: n doubles; else NULL
  int* common;
  double* score;
  int* lists[4];
  const int* maxrow;             // one word: the longest row, left by the build
  sim_control_t* ctl;
  int n, pairs, measure;
  sim_opts_t o;
};

// the two rows of a pair, the shorter one first (equally long: the smaller id's): start and length each
struct sim_rows_t {
  int a, la, b, lb;
};
__device__ __forceinline__ sim_rows_t sim_rows(const int* ro, int u, int v) {
  const int su = ro[u], lu = ro[u + 1] - su, sv = ro[v], lv = ro[v + 1] - sv;
  if (lu > lv || (lu == lv && u > v)) return {sv, lv, su, lu};
  return {su, lu, sv, lv};
}

// the first position of s[lo, hi) whose entry is >= x (UPPER: > x), hi when there is none; `reads` counts the loads
template <bool UPPER>
__device__ __forceinline__ int sim_bound(const int* s, int lo, int hi, int x, u64& reads) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int val = s[mid];
    ++reads;
    if (UPPER ? val <= x : val < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// x searched in the ascending s[lo, end): lo becomes its lower bound; true when it is there.  No load beyond the search's own: the
// value at the last `hi` the search set is remembered, so a row of lb entries costs at most floor(log2 lb) + 1 loads
__device__ __forceinline__ bool sim_search(const int* s, int& lo, int end, int x, u64& reads) {
  int hi = end;
  bool hit = false;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int val = s[mid];
    ++reads;
    if (val < x) lo = mid + 1;
    else {
      hi = mid;
      hit = val == x;
    }
  }
  return hit;
}

// the adjacency entries a workgroup's lanes loaded: summed per wave, added once per workgroup.  Every thread of the workgroup calls.
__device__ __forceinline__ void sim_flush_reads(u64 reads, u64* total) {
  __shared__ u64 s_reads[WAVES_PER_BLOCK];
  reads = wave_sum(reads);
  if (lane_id() == 0) s_reads[threadIdx.x / WAVE] = reads;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += s_reads[w];
    if (t) atomicAdd(total, t);
  }
}

__global__ __launch_bounds__(BLOCK) void k_sim_classify(sim_args_t a) {
  __shared__ int stages[WAVES_PER_BLOCK][4][SIM_APPEND_STAGE];
  const int w = threadIdx.x / WAVE, lane = lane_id();
  const long long wave = (long long)blockIdx.x * WAVES_PER_BLOCK + w, waves = (long long)gridDim.x * WAVES_PER_BLOCK;
  int f0 = 0, f1 = 0, f2 = 0, f3 = 0;
  unsigned b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
  bool bad = false;
  for (long long base = wave * WAVE; base < a.pairs; base += waves * WAVE) {
    const long long p = base + lane;
    int cls = -1;
    if (p < a.pairs) {
      const int u = a.u[p], v = a.v[p];
      if ((unsigned)u >= (unsigned)a.n || (unsigned)v >= (unsigned)a.n) {
        bad = true;
      } else {
        const int lu = a.ro[u + 1] - a.ro[u], lv = a.ro[v + 1] - a.ro[v];
        cls = sim_class(min(lu, lv), max(lu, lv), a.o);
        if (cls == SIM_NONE) {
          a.common[p] = 0;
          if (a.x) a.score[p] = 0.0;
        }
      }
    }
    b0 += cls == SIM_NONE; b1 += cls == SIM_LANE; b2 += cls == SIM_PROBE; b3 += cls == SIM_WAVE; b4 += cls == SIM_BLOCK;
    wave_stage_push<SIM_APPEND_STAGE>(cls == SIM_LANE, (int)p, stages[w][0], f0, a.lists[0], &a.ctl->n_list[0]);
    wave_stage_push<SIM_APPEND_STAGE>(cls == SIM_PROBE, (int)p, stages[w][1], f1, a.lists[1], &a.ctl->n_list[1]);
    wave_stage_push<SIM_APPEND_STAGE>(cls == SIM_WAVE, (int)p, stages[w][2], f2, a.lists[2], &a.ctl->n_list[2]);
    wave_stage_push<SIM_APPEND_STAGE>(cls == SIM_BLOCK, (int)p, stages[w][3], f3, a.lists[3], &a.ctl->n_list[3]);
  }
  wave_stage_flush(stages[w][0], f0, a.lists[0], &a.ctl->n_list[0]);
  wave_stage_flush(stages[w][1], f1, a.lists[1], &a.ctl->n_list[1]);
  wave_stage_flush(stages[w][2], f2, a.lists[2], &a.ctl->n_list[2]);
  wave_stage_flush(stages[w][3], f3, a.lists[3], &a.ctl->n_list[3]);
  b0 = wave_sum(b0); b1 = wave_sum(b1); b2 = wave_sum(b2); b3 = wave_sum(b3); b4 = wave_sum(b4);
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    if (b0) atomicAdd(&a.ctl->bins[SIM_NONE], (u64)b0);
    if (b1) atomicAdd(&a.ctl->bins[SIM_LANE], (u64)b1);
    if (b2) atomicAdd(&a.ctl->bins[SIM_PROBE], (u64)b2);
    if (b3) atomicAdd(&a.ctl->bins[SIM_WAVE], (u64)b3);
    if (b4) atomicAdd(&a.ctl->bins[SIM_BLOCK], (u64)b4);
    if (any_bad) a.ctl->err = 1;
  }
}

// LANE: a lane per pair
__global__ __launch_bounds__(BLOCK) void k_sim_lane(sim_args_t a) {
  const int count = a.ctl->n_list[0];
  const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x, gthreads = (long long)gridDim.x * BLOCK;
  u64 reads = 0;
  for (long long i = gtid; i < count; i += gthreads) {
    const int p = a.lists[0][i];
    const sim_rows_t r = sim_rows(a.ro, a.u[p], a.v[p]);
    const int end = r.b + r.lb;
    int c = 0, lo = r.b;
    double s = 0.0;
    for (int j = 0; j < r.la && lo < end; ++j) {
      const int w = a.ci[r.a + j];
      ++reads;
      if (sim_search(a.ci, lo, end, w, reads)) {
        ++c;
        ++lo;
        if (a.x) s += a.x[w];
      }
    }
    a.common[p] = c;
    if (a.x) a.score[p] = s;
  }
  sim_flush_reads(reads, &a.ctl->entries_read);
}

// PROBE: a group of SIM_GROUP lanes per pair, four pairs a wave at a time
__global__ __launch_bounds__(BLOCK) void k_sim_probe(sim_args_t a) {
  constexpr int G = SIM_GROUP, NG = WAVE / G;
  const int count = a.ctl->n_list[1];
  const int lane = lane_id(), sub = lane % G, first = lane - sub;
  const u64 gmask = ((1ull << G) - 1ull) << first;
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) / WAVE, waves = (long long)gridDim.x * WAVES_PER_BLOCK;
  u64 reads = 0;
  for (long long i0 = wave * NG; i0 < count; i0 += waves * NG) {
    const long long i = i0 + lane / G;
    const bool on = i < count;
    int p = 0;
    sim_rows_t r = {0, 0, 0, 0};
    if (on) {
      p = a.lists[1][i];
      r = sim_rows(a.ro, a.u[p], a.v[p]);
    }
    const int end = r.b + r.lb;
    const int longest = wave_max(r.la);
    int c = 0, from = r.b;
    double s = 0.0;
    for (int j0 = 0; j0 < longest; j0 += G) {
      const int j = j0 + sub;
      bool hit = false;
      int lo = from, w = 0;
      if (j < r.la) {
        w = a.ci[r.a + j];
        ++reads;
        hit = sim_search(a.ci, lo, end, w, reads);
      }
      c += __popcll(__ballot(hit) & gmask);
      if (hit && a.x) s += a.x[w];
      from = __shfl(lo, first + G - 1, WAVE);                 // (the group's later entries are larger than its last lane's)
    }
    if (a.x) {
#pragma unroll
      for (int d = G / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, WAVE);
    }
    if (on && sub == 0) {
      a.common[p] = c;
      if (a.x) a.score[p] = s;
    }
  }
  sim_flush_reads(reads, &a.ctl->entries_read);
}

// what a workgroup's team shares beside the stage
struct sim_team_smem_t {
  int bounds[2];
  int cnt[WAVES_PER_BLOCK];
  double part[WAVES_PER_BLOCK];
};

template <int TEAM>
__device__ __forceinline__ void sim_team_sync() {
  if (TEAM == WAVE) wave_lds_fence();
  else __syncthreads();
}

// One pair by a team of TEAM threads (a wave or the workgroup), thread `tid` of it: per chunk of at most S entries of the short
// row in `stage`, the slice of the long row within the chunk's values is streamed, entry k by thread k mod TEAM.
template <int TEAM>
__device__ __forceinline__ void sim_staged_pair(const sim_args_t& a, int p, int* stage, int S, int tid, sim_team_smem_t* sm, u64& reads) {
  const sim_rows_t r = sim_rows(a.ro, a.u[p], a.v[p]);
  const int* const row_b = a.ci + r.b;
  const bool weighted = a.x != nullptr;
  const bool chunked = r.la > S;
  int c = 0, from = 0;                                        // (the long row's entries before `from` lie below the chunk)
  double total = 0.0;
  for (int c0 = 0; c0 < r.la; c0 += S) {
    const int cl = min(S, r.la - c0);
    for (int k = tid; k < cl; k += TEAM) {
      stage[k] = a.ci[r.a + c0 + k];
      ++reads;
    }
    sim_team_sync<TEAM>();
    int slo = 0, shi = r.lb;
    if (chunked) {
      // (one wave searches, its lanes in step on the same addresses; its first lane counts the loads)
      u64 probes = 0;
      if (tid < WAVE) {
        slo = sim_bound<false>(row_b, from, r.lb, stage[0], probes);
        shi = sim_bound<true>(row_b, slo, r.lb, stage[cl - 1], probes);
        if (tid == 0) reads += probes;
      }
      if (TEAM != WAVE) {
        if (tid == 0) {
          sm->bounds[0] = slo;
          sm->bounds[1] = shi;
        }
        __syncthreads();
        slo = sm->bounds[0];
        shi = sm->bounds[1];
      }
      from = shi;
    }
    double s = 0.0;
    for (int j = slo - slo % TEAM + tid; j < shi; j += TEAM) {
      if (j < slo) continue;
      const int w = row_b[j];
      ++reads;
      if (tc_find(stage, cl, w) >= 0) {
        ++c;
        if (weighted) s += a.x[w];
      }
    }
    if (weighted) {
      s = wave_sum(s);
      if (TEAM != WAVE) {
        if (lane_id() == 0) sm->part[tid / WAVE] = s;
        __syncthreads();
        s = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) s += sm->part[w];
      }
      total += s;
    }
    sim_team_sync<TEAM>();                                    // (the stage and the team's words are read before the next chunk fills them)
  }
  c = wave_sum(c);
  if (TEAM != WAVE) {
    if (lane_id() == 0) sm->cnt[tid / WAVE] = c;
    __syncthreads();
    c = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) c += sm->cnt[w];
    __syncthreads();
  }
  if (tid == 0) {
    a.common[p] = c;
    if (weighted) a.score[p] = total;
  }
}

// WAVE: a pair per wave
__global__ __launch_bounds__(BLOCK) void k_sim_wave(sim_args_t a) {
  __shared__ int s_stage[WAVES_PER_BLOCK][SIM_WAVE_STAGE];
  const int count = a.ctl->n_list[2];
  const int w = threadIdx.x / WAVE, lane = lane_id();
  const int S = min(a.o.stage, SIM_WAVE_STAGE);
  u64 reads = 0;
  for (long long it = (long long)blockIdx.x * WAVES_PER_BLOCK + w; it < count; it += (long long)gridDim.x * WAVES_PER_BLOCK)
    sim_staged_pair<WAVE>(a, a.lists[2][it], s_stage[w], S, lane, nullptr, reads);
  sim_flush_reads(reads, &a.ctl->entries_read);
}

// BLOCK: a pair per workgroup
__global__ __launch_bounds__(BLOCK) void k_sim_block(sim_args_t a) {
  __shared__ int s_stage[SIM_BLOCK_STAGE];
  __shared__ sim_team_smem_t sm;
  const int count = a.ctl->n_list[3];
  const int S = min(a.o.stage, SIM_BLOCK_STAGE);
  u64 reads = 0;
  for (long long it = blockIdx.x; it < count; it += gridDim.x) sim_staged_pair<BLOCK>(a, a.lists[3][it], s_stage, S, (int)threadIdx.x, &sm, reads);
  sim_flush_reads(reads, &a.ctl->entries_read);
}

// the scores that are a function of c and the degrees, and the run's sums (one add per workgroup each)
__global__ __launch_bounds__(BLOCK) void k_sim_score(sim_args_t a) {
  __shared__ u64 s_sum[WAVES_PER_BLOCK], s_pos[WAVES_PER_BLOCK];
  u64 sum = 0, pos = 0;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < a.pairs; p += (long long)gridDim.x * BLOCK) {
    const int u = a.u[p], v = a.v[p];
    if ((unsigned)u >= (unsigned)a.n || (unsigned)v >= (unsigned)a.n) continue;      // (the run fails: k_sim_classify has said so)
    const int c = a.common[p];
    if (!a.x) a.score[p] = sim_score(a.measure, c, a.ro[u + 1] - a.ro[u], a.ro[v + 1] - a.ro[v]);
    sum += (u64)c;
    pos += c > 0;
  }
  sum = wave_sum(sum);
  pos = wave_sum(pos);
  if (lane_id() == 0) {
    s_sum[threadIdx.x / WAVE] = sum;
    s_pos[threadIdx.x / WAVE] = pos;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = pos = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) {
      sum += s_sum[w];
      pos += s_pos[w];
    }
    if (sum) atomicAdd(&a.ctl->sum_c, sum);
    if (pos) atomicAdd(&a.ctl->positive, pos);
    if (blockIdx.x == 0) a.ctl->maxrow = *a.maxrow;
  }
}

// the longest row of the adjacency into one word (cleared before), at the build
__global__ __launch_bounds__(BLOCK) void k_sim_maxrow(const int* ro, int n, int* out) {
  int best = 0;
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) best = max(best, ro[v + 1] - ro[v]);
  best = wave_max(best);
  if (lane_id() == 0 && best) atomicMax(out, best);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// The pairs and results of one path (the fused one's or the operator path's), sized by the largest P seen, growing only.
struct sim_results_t {
  mem_t<int> d_u, d_v, common;
  mem_t<double> score, x;
  pinned_t<int> h_uv;                // the upload's pinned staging: u then v
  pinned_t<double> h_x;
  size_t cap = 0;
  const int* u = nullptr;            // the last run's pairs on the device: d_u / d_v, or in edges mode the graph's src / dag_ci
  const int* v = nullptr;
  long long pairs = 0;
  void ensure(size_t P, bool weighted, int n, context_t& ctx) {
    if (P > cap) {
      d_u = mem_t<int>(); d_v = mem_t<int>(); common = mem_t<int>(); score = mem_t<double>(); h_uv = pinned_t<int>();
      cap = 0;
      d_u = mem_t<int>(P, ctx); d_v = mem_t<int>(P, ctx); common = mem_t<int>(P, ctx); score = mem_t<double>(P, ctx);
      h_uv = pinned_t<int>(2 * P);
      cap = P;
    }
    if (weighted && x.size() == 0) {
      x = mem_t<double>((size_t)std::max(n, 1), ctx);
      h_x = pinned_t<double>((size_t)std::max(n, 1));
    }
  }
  // The pairs (NULL: edges mode, the graph's own arrays) and the weights to the device, without a wait: the staging is read by
  // the copies before the run's read-back returns, and written again only by a later run.
  void upload(const int* h_u, const int* h_v, long long P, const int* e_u, const int* e_v, const double* h_xs, int n, hipStream_t st) {
    pairs = P;
    if (h_u) {
      if (P > 0) {
        std::memcpy(h_uv.data(), h_u, (size_t)P * sizeof(int));
        std::memcpy(h_uv.data() + P, h_v, (size_t)P * sizeof(int));
        MGX_HIP(hipMemcpyAsync(d_u.data(), h_uv.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, st));
        MGX_HIP(hipMemcpyAsync(d_v.data(), h_uv.data() + P, (size_t)P * sizeof(int), hipMemcpyHostToDevice, st));
      }
      u = d_u.data(); v = d_v.data();
    } else {
      u = e_u; v = e_v;
    }
    if (h_xs && n > 0) {
      std::memcpy(h_x.data(), h_xs, (size_t)n * sizeof(double));
      MGX_HIP(hipMemcpyAsync(x.data(), h_x.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
  }
};

struct sim_state_t {
  int n = 0;
  sim_opts_t opts;
  ktruss_state_t kt;                 // the builder and owner of the DAGs and adjacencies (per `symmetric`)
  mem_t<int> maxrow;                 // [symmetric]: the longest simple row
  long long h_maxrow[2] = {-1, -1};  // as the host has read it (-1: not yet)
  sim_results_t res;
  mem_t<int> lists[4];
  size_t lists_cap = 0;
  mem_t<sim_control_t> ctl;
  pinned_t<sim_control_t> h_ctl;
  bool timing = false;
  event_t ev[5];                     // the build's ends, the classifying launch's end, the pair kernels' end, the upload's end
  double phase_ms[3] = {0.0, 0.0, 0.0};          // the last timed fused run: build, classify, pair kernels
  long long bins[SIM_CLASSES] = {0}, entries_read = 0;

  sim_state_t(int n_, long long m_, standard_context_t& ctx) : n(n_), opts(sim_opts_t::from_env()), kt(n_, m_, ctx) {
    maxrow = mem_t<int>(2, ctx);
    ctl = mem_t<sim_control_t>(1, ctx);
    h_ctl = pinned_t<sim_control_t>(1);
  }

  // The adjacency of `symmetric` unless it is there; true: this call built it.  Launches and waits go to kt.tc's counts.
  bool prepare(bool symmetric, const int* ro, const int* ci, standard_context_t& ctx) {
    if (n <= 0) return false;
    const bool built_now = kt.ensure_graph(symmetric, ro, ci, ctx);
    if (built_now) {
      const int sym = symmetric ? 1 : 0;
      const hipStream_t st = ctx.stream();
      MGX_HIP(hipMemsetAsync(maxrow.data() + sym, 0, sizeof(int), st));
      hipLaunchKernelGGL(k_sim_maxrow, dim3(grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8)), dim3(BLOCK), 0, st, (const int*)kt.gr[sym].adj_ro.data(), n,
                         maxrow.data() + sym);
      MGX_CHECK_LAUNCH("mgx sim build");
      kt.tc.launches += 2;
    }
    return built_now;
  }

  // what a run of either path starts with: the counts cleared, the adjacency there (timed as the build), the arrays sized
  bool begin(bool symmetric, const int* ro, const int* ci, standard_context_t& ctx) {
    kt.tc.launches = kt.tc.waits = 0;
    phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.0;
    if (timing) MGX_HIP(hipEventRecord(ev[0], ctx.stream()));
    const bool built_now = prepare(symmetric, ro, ci, ctx);
    if (timing) MGX_HIP(hipEventRecord(ev[1], ctx.stream()));
    return built_now;
  }

  // The fused run (ro, ci: the CSR on the device; h_u == NULL: edges mode).  Returns the eight stats; fails when an id is out of range.
  std::vector<long long> run(const int* ro, const int* ci, bool symmetric, const int* h_u, const int* h_v, long long P, int measure, const double* h_x,
                             standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int sym = symmetric ? 1 : 0;
    std::fill(bins, bins + SIM_CLASSES, 0);
    entries_read = 0;
    res.pairs = 0;
    const bool built_now = begin(symmetric, ro, ci, ctx);
    if (n <= 0) return {0, 0, 0, 0, 0, 0, 0, 0};
    ktruss_graph_t& g = kt.gr[sym];
    if (!h_u) P = g.m;
    const bool weighted = measure == SIM_WEIGHTED;
    res.ensure((size_t)P, weighted, n, ctx);
    if ((size_t)P > lists_cap) {
      for (auto& l : lists) l = mem_t<int>();
      lists_cap = 0;
      for (auto& l : lists) l = mem_t<int>((size_t)P, ctx);
      lists_cap = (size_t)P;
    }
    res.upload(h_u, h_v, P, g.src.data(), kt.tc.dag[sym].ci.data(), weighted ? h_x : nullptr, n, st);
    MGX_HIP(hipMemsetAsync(ctl.data(), 0, sizeof(sim_control_t), st));
    sim_args_t a;
    a.ro = g.adj_ro.data(); a.ci = g.adj_ci.data(); a.u = res.u; a.v = res.v; a.x = weighted ? res.x.data() : nullptr;
    a.common = res.common.data(); a.score = res.score.data();
    for (int k = 0; k < 4; ++k) a.lists[k] = lists[k].data();
    a.maxrow = maxrow.data() + sym; a.ctl = ctl.data(); a.n = n; a.pairs = (int)P; a.measure = measure; a.o = opts;
    const int cap = std::max(ctx.num_cus, 1) * 8;
    long long launches = 1;                                    // (the control words' clear)
    if (P > 0) {
      if (timing) MGX_HIP(hipEventRecord(ev[4], st));          // (behind the pairs' upload: the copy is in no phase)
      hipLaunchKernelGGL(k_sim_classify, dim3(grid_for(P, BLOCK, cap)), dim3(BLOCK), 0, st, a);
      if (timing) MGX_HIP(hipEventRecord(ev[2], st));
      hipLaunchKernelGGL(k_sim_block, dim3((unsigned)std::min<long long>(P, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_sim_wave, dim3(grid_for(P, WAVES_PER_BLOCK, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_sim_probe, dim3(grid_for(P * SIM_GROUP, BLOCK, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_sim_lane, dim3(grid_for(P, BLOCK, cap)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_sim_score, dim3(grid_for(P, BLOCK, cap)), dim3(BLOCK), 0, st, a);
      if (timing) MGX_HIP(hipEventRecord(ev[3], st));
      MGX_CHECK_LAUNCH("mgx sim run");
      launches += 6;
    }
    h_ctl.fetch(ctl.data(), 1, st);
    const sim_control_t& c = *h_ctl.data();
    if (timing) {
      float ms = 0.f;
      MGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      phase_ms[0] = ms;
      if (P > 0) {
        MGX_HIP(hipEventElapsedTime(&ms, ev[4], ev[2]));
        phase_ms[1] = ms;
        MGX_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
        phase_ms[2] = ms;
      }
    }
    if (c.err) throw mgx_error(MGX_E_INVALID, "mgx_sim_run: a pair names a vertex outside [0, n)");
    for (int k = 0; k < SIM_CLASSES; ++k) bins[k] = (long long)c.bins[k];
    entries_read = (long long)c.entries_read;
    if (P > 0) h_maxrow[sym] = c.maxrow;
    const long long longest = longest_row(sym, ctx);
    return {P, (long long)c.sum_c, (long long)c.positive, 2ll * g.m, longest, built_now ? 1 : 0, kt.tc.waits + 1, kt.tc.launches + launches};
  }

  // the longest row; where no launch of a run has carried it yet (P == 0, the operator path) a read of its own, once
  long long longest_row(int sym, standard_context_t& ctx) {
    if (h_maxrow[sym] < 0) {
      int v = 0;
      MGX_HIP(dtoh(&v, (const int*)maxrow.data() + sym, 1, ctx.stream()));
      kt.tc.waits += 1;
      h_maxrow[sym] = v;
    }
    return h_maxrow[sym];
  }
};

}  // namespace mgx
