// mgx/bc_fused.hpp -- betweenness centrality (Brandes), fused (mgx_bc_run): per source one fused BFS, then two PULL sweeps over
// the reached rows, level by level, without an atomic and without a label test per entry.
//
// The definition (the operator path include/gunrock/bc/ and tests/bc_model.py compute the same):
//   CSR entry (u, v) is an edge u -> v, every entry counts once (duplicates are parallel edges), self-loops lie on no shortest path.
//     label[v]  BFS depth from s, -1 unreached
//     sigma[v]  number of shortest s -> v entry-paths, sigma[s] = 1
//     delta[v]  = sum over the entries (v, w) with label[w] = label[v] + 1 of sigma[v] / sigma[w] * (1 + delta[w])
//     bc[v]     = sum over the given sources s != v of delta_s[v]
//   sigma, delta, bc are double.
//
// Two arrays P[0], P[1] and two arrays Q[0], Q[1] of n doubles, all cleared at the start of a source, P[0][s] = 1.
//   forward,  d = 1 .. D - 1, v on level d:   P[d & 1][v] = sum over ALL in-entries (u, v) of P[(d - 1) & 1][u]
//     An in-neighbour of a level-d vertex is unreached, on level d - 1, or deeper; only level d - 1 has written into the parity the
//     pass reads, so the sum is sigma[v].
//   backward, d = D - 2 .. 1, v on level d:   delta[v] = P[d & 1][v] * sum over ALL out-entries (v, w) of Q[(d + 1) & 1][w]
//                                             Q[d & 1][v] = (1 + delta[v]) / sigma[v],  bc[v] += delta[v]  (by the owner)
//     An out-neighbour is on level <= d + 1.  The levels d - 1, d - 3, .. share the parity the pass reads and ARE out-neighbours (the
//     parent of v, on a symmetric graph): they must still hold zero there.  So the forward pass seeds Q[d & 1][v] = 1 / sigma[v]
//     (the value for delta = 0) on the deepest level ONLY -- the one level no backward launch visits.  Deeper levels of the same
//     parity hold stale values; nothing on level d has an out-entry to them.
//   The host knows the depth only to one level (the traversal reports the levels that expanded an entry: D or D - 1): it plans for
//   D' = levels + 1, the forward pass seeds Q on the levels D' - 2 and D' - 1, the backward pass starts at D' - 2 and the device
//   leaves that level alone when the list of D' - 1 is empty (bc_deepest): it is the deepest then, delta = 0 and Q is seeded.
//   (Folding it all the same rewrites the same 1 / sigma for a finite sigma -- but an overflowed sigma gives inf * 0 = NaN, which
//   the next levels spread over the whole traversal: tests/bc_cases.py, sigma_limits at 2^1024.)
//
// Level lists: key[v] = (label + 1) * 4 + row class, (key, id) sorted with rocPRIM's radix sort over the bits D' needs, the
// list bounds found from the sorted keys -- one contiguous list per level and class, unreached vertices in front.  A directed
// graph sorts twice: by the in-rows' classes (forward), by the out-rows' (backward).
// Row classes (static per graph and direction, made once per handle): lane -- at most lane_max entries, one lane per row;
// wave -- one wave per row, lanes striding, the wave's sum by a fixed xor tree; huge -- at least huge_min entries, cut into
// segments of `seg` entries: one launch folds the segments of the level's huge rows into partials, a small one adds a row's
// partials in segment order.  Every row is folded in an order that depends on the row alone: results are bit-equal between runs.
// The three thresholds' defaults (16 / 8192 / 8192) and the chain's (1024) are UNMEASURED guesses.
//
// The chain: a run of at least two consecutive levels of at most `chain` vertices each (levels behind the end of the traversal's
// trace count as small) is ONE launch of ONE workgroup, k_bc_chain, which takes the levels one after the other.  Between two
// levels: __threadfence() + __syncthreads(), and the gathered values are read with relaxed agent-scope loads (other waves of the
// workgroup wrote them in this launch).  It folds every row exactly as the grid kernels do.
//
// No atomics, no grid barrier, no cooperative launch, no inline assembly.  A run waits for the host ONCE of its own, at the end.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <utility>
#include <vector>

#include "env.hpp"
#include "runtime.hpp"
#include "wave.hpp"

// (mgx_layout.hip: the one translation unit that includes rocPRIM)  tmp == nullptr: *tmp_bytes <- the scratch a sort of n pairs needs
extern "C" int mgx_bc_sort_device(const unsigned* keys_in, unsigned* keys_out, const int* ids_in, int* ids_out, int n, int end_bit,
                                  void* tmp, size_t* tmp_bytes, hipStream_t stream);

namespace mgx {

constexpr int BC_KEY_STRIDE = 4;              // keys per level: the three classes and one spare
constexpr int BC_LANE = 0, BC_WAVE = 1, BC_HUGE = 2;
constexpr int BC_INFO_WORDS = 16;
constexpr double BC_TWO53 = 9007199254740992.0;

struct bc_opts_t {
  // (all four defaults are unmeasured guesses)
  int lane_max = 16;      // MGX_BC_LANE_MAX: rows of at most this many entries are folded by one lane
  int huge_min = 8192;    // MGX_BC_HUGE_MIN: rows of at least this many by several workgroups; the others by a wave
  int seg = 8192;         // MGX_BC_SEG: entries of a huge row's segment
  int chain = 1024;       // MGX_BC_CHAIN: a level of at most this many vertices is small (0: no chain)
  static bc_opts_t from_env() {
    bc_opts_t o;
    o.lane_max = env_int("MGX_BC_LANE_MAX", 0, INT_MAX, o.lane_max);
    o.huge_min = env_int("MGX_BC_HUGE_MIN", 1, INT_MAX, o.huge_min);
    o.seg = env_int("MGX_BC_SEG", 1, INT_MAX, o.seg);
    o.chain = env_int("MGX_BC_CHAIN", 0, INT_MAX, o.chain);
    return o;
  }
  int row_class(int len) const { return len <= lane_max ? BC_LANE : (len >= huge_min ? BC_HUGE : BC_WAVE); }
};

// the rows of one direction as the kernels read them
struct bc_dir_t {
  const int* off;
  const int* idx;
  const int* seg_base;      // huge rows: the first slot of the row's partials
  const int* seg_row;       // the row of every segment of the graph's huge rows (segment s is slot s of the partials)
  int seg;
  int segments;
};
struct bc_arrays_t {
  double* P[2];
  double* Q[2];
  double* delta;
  double* bc;
  u32* flags;               // [0] inexact, [1] overflow
};
struct bc_ctrl_t {
  u32 inexact, overflow;
  int deepest;              // levels of the deepest traversal of the run
  int last_levels;          // levels of the last source
};

template <bool AGENT>
__device__ __forceinline__ double bc_ld(const double* p) {
  if constexpr (AGENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool AGENT>
__device__ __forceinline__ double bc_row_lane(const int* __restrict__ idx, int b, int e, const double* vals) {
  double a = 0.0;
  for (int k = b; k < e; ++k) a += bc_ld<AGENT>(vals + idx[k]);
  return a;
}
// all lanes of a wave, the same row; every lane gets the sum
template <bool AGENT>
__device__ __forceinline__ double bc_row_wave(const int* __restrict__ idx, int b, int e1, const double* vals, int lane) {
  double a0 = 0.0, a1 = 0.0;
  int e = b + lane;
  for (; e + WAVE < e1; e += 2 * WAVE) {
    const double x0 = bc_ld<AGENT>(vals + idx[e]), x1 = bc_ld<AGENT>(vals + idx[e + WAVE]);
    a0 += x0; a1 += x1;
  }
  if (e < e1) a0 += bc_ld<AGENT>(vals + idx[e]);
  return wave_sum(a0 + a1);
}
// all BLOCK threads of a workgroup, the same segment; every thread gets the sum (two barriers)
template <bool AGENT>
__device__ __forceinline__ double bc_seg_block(const int* __restrict__ idx, int b, int e1, const double* vals, double* s_w) {
  double a0 = 0.0, a1 = 0.0;
  int e = b + (int)threadIdx.x;
  for (; e + BLOCK < e1; e += 2 * BLOCK) {
    const double x0 = bc_ld<AGENT>(vals + idx[e]), x1 = bc_ld<AGENT>(vals + idx[e + BLOCK]);
    a0 += x0; a1 += x1;
  }
  if (e < e1) a0 += bc_ld<AGENT>(vals + idx[e]);
  const double a = wave_sum(a0 + a1);
  if (lane_id() == 0) s_w[threadIdx.x / WAVE] = a;
  __syncthreads();
  double t = s_w[0];
#pragma unroll
  for (int w = 1; w < WAVES_PER_BLOCK; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

// backward: is level d the deepest, i.e. is the list of level d + 1 empty?  Asked for the one level the host cannot tell.
__device__ __forceinline__ bool bc_deepest(const int* __restrict__ bound, int d) {
  const int k = (d + 2) * BC_KEY_STRIDE;
  return bound[k] == bound[k + BC_KEY_STRIDE];
}
// what the owner of v does with the row's sum S
template <bool BACK>
__device__ __forceinline__ void bc_finish(int v, double S, const bc_arrays_t& A, int d, int seed_q) {
  if constexpr (!BACK) {
    A.P[d & 1][v] = S;
    if (seed_q) A.Q[d & 1][v] = 1.0 / S;
    if (S >= BC_TWO53) A.flags[0] = 1u;
    if (!(S <= 1.7976931348623157e308)) A.flags[1] = 1u;
  } else {
    const double sigma = A.P[d & 1][v];
    const double dl = sigma * S;
    A.Q[d & 1][v] = (1.0 + dl) / sigma;
    A.delta[v] = dl;
    A.bc[v] += dl;
  }
}

// ---- the level lists ----------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_bc_keys(const int* __restrict__ labels, const unsigned char* __restrict__ cls_a,
                                                   const unsigned char* __restrict__ cls_b, u32* __restrict__ keys_a, u32* __restrict__ keys_b,
                                                   int* __restrict__ ids, int n) {
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) {
    const u32 base = (u32)(labels[v] + 1) * (u32)BC_KEY_STRIDE;
    keys_a[v] = base + cls_a[v];
    if (cls_b) keys_b[v] = base + cls_b[v];
    ids[v] = (int)v;
  }
}
// bound[k] = the first position of the sorted keys that holds a key >= k, for k = 0 .. K (bound[K] = n when every key is below K)
__global__ __launch_bounds__(BLOCK) void k_bc_bounds(const u32* __restrict__ keys, int n, int K, int* __restrict__ bound) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const long long lo = i == 0 ? 0 : (long long)keys[i - 1] + 1;
    const long long hi = std::min<long long>((long long)keys[i], (long long)K);
    for (long long k = lo; k <= hi; ++k) bound[k] = (int)i;
    if (i == n - 1)
      for (long long k = (long long)keys[i] + 1; k <= K; ++k) bound[k] = n;
  }
}
__global__ void k_bc_seed(double* P0, int src) {
  if (blockIdx.x == 0 && threadIdx.x == 0) P0[src] = 1.0;
}
// sigma of this source for inspection; the depth of its traversal into the control block (one thread, plain stores)
__global__ __launch_bounds__(BLOCK) void k_bc_finish(const int* __restrict__ labels, const double* __restrict__ P0, const double* __restrict__ P1,
                                                     double* __restrict__ sigma, int n, const u32* __restrict__ keys_sorted, bc_ctrl_t* c,
                                                     const u32* __restrict__ flags) {
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) {
    const int l = labels[v];
    sigma[v] = l < 0 ? 0.0 : ((l & 1) ? P1[v] : P0[v]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int lv = n > 0 ? (int)(keys_sorted[n - 1] / (u32)BC_KEY_STRIDE) : 0;
    c->last_levels = lv;
    if (lv > c->deepest) c->deepest = lv;
    if (flags[0]) c->inexact = 1u;
    if (flags[1]) c->overflow = 1u;
  }
}

// ---- one level, chip-sized grid: the lane rows and the wave rows ------------------------------------
// seed_q: forward, seed Q on this level; backward, this level may be the deepest (nothing to do then)
template <bool BACK>
__global__ __launch_bounds__(BLOCK) void k_bc_level(bc_dir_t G, const int* __restrict__ list, const int* __restrict__ bound, int d, int seed_q,
                                                    bc_arrays_t A) {
  if (BACK && seed_q && bc_deepest(bound, d)) return;
  const int k0 = (d + 1) * BC_KEY_STRIDE;
  const int l0 = bound[k0], l1 = bound[k0 + 1], l2 = bound[k0 + 2];
  const double* const vals = BACK ? A.Q[(d + 1) & 1] : A.P[(d - 1) & 1];
  const long long threads = (long long)gridDim.x * BLOCK, tid = (long long)blockIdx.x * BLOCK + threadIdx.x;
  for (long long i = l0 + tid; i < l1; i += threads) {
    const int v = list[i];
    bc_finish<BACK>(v, bc_row_lane<false>(G.idx, G.off[v], G.off[v + 1], vals), A, d, seed_q);
  }
  const int lane = lane_id();
  for (long long i = l1 + tid / WAVE; i < l2; i += threads / WAVE) {        // (wave-uniform)
    const int v = list[i];
    const double S = bc_row_wave<false>(G.idx, G.off[v], G.off[v + 1], vals, lane);
    if (lane == 0) bc_finish<BACK>(v, S, A, d, seed_q);
  }
}
// the segments of the level's huge rows -> partials.  The workgroups stride over ALL segments of the graph's huge rows (a static
// list: a few thousand at RMAT-22) and take those whose row is on level d -- one label read per segment, none per entry.  (First
// shape: every workgroup walked the level's huge rows and took "its" segment of each; most huge rows have one to three segments, so
// three workgroups folded nearly all of them one after the other: 28 ms a level at RMAT-22.)
template <bool BACK>
__global__ __launch_bounds__(BLOCK) void k_bc_huge_seg(bc_dir_t G, const int* __restrict__ labels, int d, bc_arrays_t A, double* __restrict__ partial) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  const double* const vals = BACK ? A.Q[(d + 1) & 1] : A.P[(d - 1) & 1];
  for (int s = blockIdx.x; s < G.segments; s += gridDim.x) {               // (workgroup-uniform)
    const int v = G.seg_row[s];
    if (labels[v] != d) continue;
    const int b = G.off[v], e = G.off[v + 1];
    const long long sb = (long long)b + (long long)(s - G.seg_base[v]) * G.seg;
    const int se = (int)std::min<long long>(sb + G.seg, (long long)e);
    const double t = bc_seg_block<false>(G.idx, (int)sb, se, vals, s_w);
    if (threadIdx.x == 0) partial[s] = t;
  }
}
// a huge row's partials in segment order, by one lane
template <bool BACK>
__global__ __launch_bounds__(BLOCK) void k_bc_huge_fold(bc_dir_t G, const int* __restrict__ list, const int* __restrict__ bound, int d, int seed_q,
                                                        bc_arrays_t A, const double* __restrict__ partial) {
  if (BACK && seed_q && bc_deepest(bound, d)) return;
  const int k0 = (d + 1) * BC_KEY_STRIDE;
  const int l2 = bound[k0 + 2], l3 = bound[k0 + 3];
  for (long long i = l2 + (long long)blockIdx.x * BLOCK + threadIdx.x; i < l3; i += (long long)gridDim.x * BLOCK) {
    const int v = list[i];
    const int base = G.seg_base[v];
    const int nseg = (int)(((long long)(G.off[v + 1] - G.off[v]) + G.seg - 1) / G.seg);
    double S = 0.0;
    for (int s = 0; s < nseg; ++s) S += partial[base + s];
    bc_finish<BACK>(v, S, A, d, seed_q);
  }
}

// ---- the chain: ONE workgroup, the levels [lo, hi] one after the other (backward: hi down to lo) -----
// seed_from: forward, the levels from here on seed Q; backward, the levels from here on may be the deepest
template <bool BACK>
__global__ __launch_bounds__(BLOCK) void k_bc_chain(bc_dir_t G, const int* __restrict__ list, const int* __restrict__ bound, int lo, int hi,
                                                    int seed_from, bc_arrays_t A) {
  __shared__ double s_w[WAVES_PER_BLOCK];
  const int lane = lane_id(), wave = (int)threadIdx.x / WAVE;
  for (int d = BACK ? hi : lo; BACK ? d >= lo : d <= hi; BACK ? --d : ++d) {   // (workgroup-uniform)
    if (BACK && d >= seed_from && bc_deepest(bound, d)) continue;               // (workgroup-uniform; nothing written, no fence)
    const int k0 = (d + 1) * BC_KEY_STRIDE;
    const int l0 = bound[k0], l1 = bound[k0 + 1], l2 = bound[k0 + 2], l3 = bound[k0 + 3];
    const double* const vals = BACK ? A.Q[(d + 1) & 1] : A.P[(d - 1) & 1];
    const int seed_q = d >= seed_from ? 1 : 0;
    for (int i = l0 + (int)threadIdx.x; i < l1; i += BLOCK) {
      const int v = list[i];
      bc_finish<BACK>(v, bc_row_lane<true>(G.idx, G.off[v], G.off[v + 1], vals), A, d, seed_q);
    }
    for (int i = l1 + wave; i < l2; i += WAVES_PER_BLOCK) {
      const int v = list[i];
      const double S = bc_row_wave<true>(G.idx, G.off[v], G.off[v + 1], vals, lane);
      if (lane == 0) bc_finish<BACK>(v, S, A, d, seed_q);
    }
    for (int r = l2; r < l3; ++r) {                  // a huge row: its segments in order, each folded as k_bc_huge_seg folds it
      const int v = list[r];
      const int b = G.off[v], e = G.off[v + 1];
      double S = 0.0;
      for (long long sb = b; sb < e; sb += G.seg)
        S += bc_seg_block<true>(G.idx, (int)sb, (int)std::min<long long>(sb + G.seg, (long long)e), vals, s_w);
      if (threadIdx.x == 0) bc_finish<BACK>(v, S, A, d, seed_q);
    }
    __threadfence();
    __syncthreads();
  }
}

// ---- host ---------------------------------------------------------------------------------------
// the rows of one direction: their classes and the huge rows' segments, made on the host once per handle
struct bc_rows_t {
  const int* off = nullptr;
  const int* idx = nullptr;
  mem_t<unsigned char> cls;
  mem_t<int> seg_base, seg_row;
  long long count[3] = {0, 0, 0};
  long long segments = 0;
  int longest = 0;

  void make(const int* d_off, const int* d_idx, int n, const bc_opts_t& o, standard_context_t& ctx) {
    off = d_off; idx = d_idx;
    std::vector<int> h((size_t)n + 1, 0);
    MGX_HIP(dtoh(h.data(), d_off, (size_t)n + 1, ctx.stream()));
    std::vector<unsigned char> c((size_t)std::max(n, 1), 0);
    std::vector<int> sb((size_t)std::max(n, 1), 0), sr;
    for (int v = 0; v < n; ++v) {
      const int len = h[(size_t)v + 1] - h[(size_t)v];
      const int k = o.row_class(len);
      c[(size_t)v] = (unsigned char)k;
      ++count[k];
      longest = std::max(longest, len);
      if (k == BC_HUGE) {
        if (segments + ((long long)len + o.seg - 1) / o.seg > 0x7fffffffLL) throw mgx_error(MGX_E_INVALID, "mgx bc: too many segments (MGX_BC_SEG too small)");
        sb[(size_t)v] = (int)segments;
        segments += ((long long)len + o.seg - 1) / o.seg;
        sr.resize((size_t)segments, v);
      }
    }
    cls = to_mem(c, ctx);
    seg_base = to_mem(sb, ctx);
    if (sr.empty()) sr.push_back(0);
    seg_row = to_mem(sr, ctx);
  }
  bc_dir_t view(const bc_opts_t& o) const { return bc_dir_t{off, idx, seg_base.data(), seg_row.data(), o.seg, (int)segments}; }
};

struct bc_state_t {
  int n = 0;
  bc_opts_t opts;
  bc_rows_t rows[2];                 // [0] the in-entries' rows, [1] the out-entries' (one and the same when symmetric: rows[1] unused)
  bool made[2] = {false, false};     // per `symmetric`: [1] rows_sym, [0] rows[0] / rows[1]
  bc_rows_t rows_sym;
  mem_t<double> work;                // P[0], P[1], Q[0], Q[1], delta: 5 n doubles, cleared per source
  mem_t<double> sigma, bc, partial;
  mem_t<u32> keys_in[2], keys_sorted[2];
  mem_t<int> ids, list[2], bound[2];
  mem_t<u32> flags;
  mem_t<bc_ctrl_t> ctrl;
  pinned_t<bc_ctrl_t> h_ctrl;
  mem_t<char> sort_tmp;
  size_t sort_bytes = 0;
  int bound_cap = 0;
  bool ran = false;
  // counters of the run in flight / the last run
  long long waits = 0, launches = 0, chain_launches = 0, last_chain_launches = 0, sources = 0, reached = 0;
  int used_csc = 0;
  // phase times (mgx_bc_set_timing; tools/bc_bench.py): HIP events around the traversal, the list build, the forward and the backward
  // launches of the first BC_TIMED sources of a run -- an event costs a few microseconds of stream gap, so only on request
  static constexpr int BC_TIMED = 64;
  bool timing = false;
  std::vector<event_t> ev;           // 5 per timed source
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};
  int timed = 0;

  bc_state_t(int n_, standard_context_t& ctx) : n(n_), opts(bc_opts_t::from_env()) {
    if (n > (1 << 29)) throw mgx_error(MGX_E_INVALID, "mgx bc: more than 2^29 vertices");
    const size_t N = (size_t)std::max(n, 1);
    work = mem_t<double>(5 * N, ctx);
    sigma = mem_t<double>(N, ctx);
    bc = mem_t<double>(N, ctx);
    for (int i = 0; i < 2; ++i) { keys_in[i] = mem_t<u32>(N, ctx); keys_sorted[i] = mem_t<u32>(N, ctx); list[i] = mem_t<int>(N, ctx); }
    ids = mem_t<int>(N, ctx);
    flags = mem_t<u32>(2, ctx);
    ctrl = mem_t<bc_ctrl_t>(1, ctx);
    h_ctrl = pinned_t<bc_ctrl_t>(1);
    const int rc = mgx_bc_sort_device(nullptr, nullptr, nullptr, nullptr, std::max(n, 1), 32, nullptr, &sort_bytes, ctx.stream());
    if (rc != 0) throw hip_error((hipError_t)rc, "mgx bc: sort scratch", __FILE__, __LINE__);
    sort_tmp = mem_t<char>(std::max<size_t>(sort_bytes, 16), ctx);
    grow_bounds(std::min(n, 1 << 16) + 2, ctx);
  }
  // event k (0: before the traversal, 1: behind it, 2: lists built, 3: forward done, 4: source done) of the source in flight
  void mark(int k, hipStream_t st) {
    if (!timing || sources >= BC_TIMED) return;
    while (ev.size() < (size_t)(sources + 1) * 5) ev.emplace_back();
    MGX_HIP(hipEventRecord(ev[(size_t)sources * 5 + (size_t)k], st));
  }
  // room for the list bounds of a traversal of `levels` levels
  void grow_bounds(int levels, standard_context_t& ctx) {
    const int want = (levels + 2) * BC_KEY_STRIDE + 1;
    if (want <= bound_cap) return;
    for (int i = 0; i < 2; ++i) bound[i] = mem_t<int>((size_t)want, ctx);
    bound_cap = want;
  }

  // the row tables of a run with this `symmetric`; in / out rows as the graph holds them
  void ensure_rows(bool symmetric, const int* ro, const int* ci, const int* co, const int* ri, standard_context_t& ctx) {
    if (made[symmetric ? 1 : 0]) return;
    if (symmetric) rows_sym.make(ro, ci, n, opts, ctx);
    else { rows[0].make(co, ri, n, opts, ctx); rows[1].make(ro, ci, n, opts, ctx); }
    const long long segs = symmetric ? rows_sym.segments : std::max(rows[0].segments, rows[1].segments);
    if ((long long)partial.size() < std::max<long long>(segs, 1)) {
      MGX_HIP(hipStreamSynchronize(ctx.stream()));
      partial = mem_t<double>((size_t)std::max<long long>(segs, 1), ctx);
    }
    made[symmetric ? 1 : 0] = true;
  }
  bc_arrays_t arrays() const {
    const size_t N = (size_t)std::max(n, 1);
    double* w = work.data();
    return bc_arrays_t{{w, w + N}, {w + 2 * N, w + 3 * N}, w + 4 * N, bc.data(), flags.data()};
  }
  const double* delta() const { return work.data() + 4 * (size_t)std::max(n, 1); }

  void begin_run(bool symmetric, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    waits = launches = chain_launches = last_chain_launches = sources = reached = 0;
    used_csc = symmetric ? 0 : 1;
    ran = false;
    MGX_HIP(hipMemsetAsync(bc.data(), 0, (size_t)std::max(n, 1) * sizeof(double), st));
    MGX_HIP(hipMemsetAsync(sigma.data(), 0, (size_t)std::max(n, 1) * sizeof(double), st));
    MGX_HIP(hipMemsetAsync(work.data(), 0, 5 * (size_t)std::max(n, 1) * sizeof(double), st));
    MGX_HIP(hipMemsetAsync(flags.data(), 0, 2 * sizeof(u32), st));
    MGX_HIP(hipMemsetAsync(ctrl.data(), 0, sizeof(bc_ctrl_t), st));
    launches += 5;
  }

  // Everything of one source behind its traversal, enqueued on the context's stream (no wait): labels[] holds the traversal's depths,
  // `levels` is the number of levels that expanded an entry (the depth D is levels or levels + 1), trace[d].first the vertices of
  // level d for the levels the traversal traced.
  void source(const int* labels, int src, int levels, const std::vector<std::pair<long long, long long>>& trace, bool symmetric,
              standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int D = levels + 1;                                   // levels 0 .. D - 1 may hold vertices
    if ((D + 2) * BC_KEY_STRIDE + 1 > bound_cap) {              // (a traversal deeper than any before: the bounds grow behind a wait)
      MGX_HIP(hipStreamSynchronize(st));
      ++waits;
      grow_bounds(D, ctx);
    }
    const bc_rows_t& rin = symmetric ? rows_sym : rows[0];
    const bc_rows_t& rout = symmetric ? rows_sym : rows[1];
    const int two = symmetric ? 1 : 2;                          // sorts
    const bc_arrays_t A = arrays();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const int grid_n = grid_for(n, BLOCK, max_blocks);
    const int K = (D + 1) * BC_KEY_STRIDE;                      // keys 0 .. K - 1
    int end_bit = 1;
    while (end_bit < 32 && (1ll << end_bit) < (long long)K) ++end_bit;

    mark(1, st);
    // 2. clears, keys, sort, bounds
    MGX_HIP(hipMemsetAsync(work.data(), 0, 5 * (size_t)n * sizeof(double), st));
    hipLaunchKernelGGL(k_bc_seed, dim3(1), dim3(64), 0, st, A.P[0], src);
    hipLaunchKernelGGL(k_bc_keys, dim3(grid_n), dim3(BLOCK), 0, st, labels, (const unsigned char*)rin.cls.data(),
                       symmetric ? (const unsigned char*)nullptr : (const unsigned char*)rout.cls.data(), keys_in[0].data(), keys_in[1].data(),
                       ids.data(), n);
    launches += 3;
    for (int i = 0; i < two; ++i) {
      size_t bytes = sort_bytes;
      const int rc = mgx_bc_sort_device(keys_in[i].data(), keys_sorted[i].data(), ids.data(), list[i].data(), n, end_bit, sort_tmp.data(), &bytes, st);
      if (rc != 0) throw hip_error((hipError_t)rc, "mgx bc: sort", __FILE__, __LINE__);
      // (cleared first: a key the traversal's level count did not promise could leave a bound unwritten -- an empty list then, never a stray index)
      MGX_HIP(hipMemsetAsync(bound[i].data(), 0, (size_t)(K + 1) * sizeof(int), st));
      hipLaunchKernelGGL(k_bc_bounds, dim3(grid_n), dim3(BLOCK), 0, st, (const u32*)keys_sorted[i].data(), n, K, bound[i].data());
      launches += 3;                                            // (the sort counts as one)
    }
    mark(2, st);
    const int* const list_f = list[0].data();
    const int* const bound_f = bound[0].data();
    const int* const list_b = list[symmetric ? 0 : 1].data();
    const int* const bound_b = bound[symmetric ? 0 : 1].data();
    const bc_dir_t Gin = rin.view(opts), Gout = rout.view(opts);

    // 3. the plan: runs of small levels go to the chain
    auto vertices = [&](int d) -> long long { return d < (int)trace.size() ? trace[(size_t)d].first : -1; };      // -1: not traced
    auto small = [&](int d) { const long long c = vertices(d); return opts.chain > 0 && (c < 0 || c <= (long long)opts.chain); };
    auto level_grid = [&](int d) {
      const long long c = vertices(d);
      return c < 0 ? 32 : (int)std::min<long long>((long long)max_blocks, std::max<long long>(1, (c + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK));
    };
    const int seed_from = D - 2;                                // the forward pass seeds Q on the levels that may be the deepest
    last_chain_launches = 0;
    // forward: d = 1 .. D - 1
    for (int d = 1; d <= D - 1;) {
      int e = d;
      while (e <= D - 1 && small(e)) ++e;
      if (e - d >= 2) {
        hipLaunchKernelGGL(k_bc_chain<false>, dim3(1), dim3(BLOCK), 0, st, Gin, list_f, bound_f, d, e - 1, seed_from, A);
        ++launches; ++chain_launches; ++last_chain_launches;
        d = e;
        continue;
      }
      const int seed_q = d >= seed_from ? 1 : 0;
      hipLaunchKernelGGL(k_bc_level<false>, dim3(level_grid(d)), dim3(BLOCK), 0, st, Gin, list_f, bound_f, d, seed_q, A);
      ++launches;
      if (rin.count[BC_HUGE] > 0) {
        hipLaunchKernelGGL(k_bc_huge_seg<false>, dim3((int)std::min<long long>(max_blocks, rin.segments)), dim3(BLOCK), 0, st, Gin, labels, d, A,
                           partial.data());
        hipLaunchKernelGGL(k_bc_huge_fold<false>, dim3(1), dim3(BLOCK), 0, st, Gin, list_f, bound_f, d, seed_q, A, (const double*)partial.data());
        launches += 2;
      }
      ++d;
    }
    mark(3, st);
    // backward: d = D - 2 .. 1; D - 2 is the deepest level when the traversal's last level expanded an entry: the device looks
    for (int d = D - 2; d >= 1;) {
      int e = d;
      while (e >= 1 && small(e)) --e;
      if (d - e >= 2) {
        hipLaunchKernelGGL(k_bc_chain<true>, dim3(1), dim3(BLOCK), 0, st, Gout, list_b, bound_b, e + 1, d, D - 2, A);
        ++launches; ++chain_launches; ++last_chain_launches;
        d = e;
        continue;
      }
      const int maybe_deepest = d == D - 2 ? 1 : 0;
      hipLaunchKernelGGL(k_bc_level<true>, dim3(level_grid(d)), dim3(BLOCK), 0, st, Gout, list_b, bound_b, d, maybe_deepest, A);
      ++launches;
      if (rout.count[BC_HUGE] > 0) {
        hipLaunchKernelGGL(k_bc_huge_seg<true>, dim3((int)std::min<long long>(max_blocks, rout.segments)), dim3(BLOCK), 0, st, Gout, labels, d, A,
                           partial.data());
        hipLaunchKernelGGL(k_bc_huge_fold<true>, dim3(1), dim3(BLOCK), 0, st, Gout, list_b, bound_b, d, maybe_deepest, A, (const double*)partial.data());
        launches += 2;
      }
      --d;
    }
    // 4. sigma of this source, the depth, the flags
    hipLaunchKernelGGL(k_bc_finish, dim3(grid_n), dim3(BLOCK), 0, st, labels, (const double*)A.P[0], (const double*)A.P[1], sigma.data(), n,
                       (const u32*)keys_sorted[0].data(), ctrl.data(), (const u32*)flags.data());
    ++launches;
    mark(4, st);
    MGX_CHECK_LAUNCH("mgx bc run");
    ++sources;
  }

  // the run's ONE wait of its own: the control block
  const bc_ctrl_t& end_run(standard_context_t& ctx) {
    h_ctrl.fetch(ctrl.data(), 1, ctx.stream());
    ++waits;
    ran = true;
    timed = 0;
    for (double& x : phase_ms) x = 0.0;
    for (long long i = 0; timing && i < sources && i < BC_TIMED && ev.size() >= (size_t)(i + 1) * 5; ++i, ++timed)
      for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        MGX_HIP(hipEventElapsedTime(&ms, ev[(size_t)i * 5 + (size_t)k], ev[(size_t)i * 5 + (size_t)k + 1]));
        phase_ms[k] += (double)ms;
      }
    return h_ctrl[0];
  }
};

}  // namespace mgx
