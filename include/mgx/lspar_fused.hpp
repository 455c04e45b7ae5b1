// mgx/lspar_fused.hpp -- local graph sparsification, fused (mgx_lspar_run): a minhash pass and a select pass on the plain CSR,
// in original ids, one host wait (the kept total, to size the outputs).
//
// The definition (the operator path include/gunrock/lspar/ and tests/lspar_model.py compute the same):
//   salt_j = fmix32(seed + 0x9E3779B9 * (j + 1)),  h_j(u) = fmix32(u ^ salt_j)             (colouring's keys, j = 0 .. k - 1)
//   mh_j(v) = unsigned min of h_j(u) over the entries u of row v (0xFFFFFFFF: empty row)
//   sim(p) = |{ j : mh_j(v) == mh_j(u) }| for entry p of row v, neighbour u                  (0 .. k)
//   t(v) = min(d, floor(pow(d, e) * (1 + 2^-40))), d = ro[v + 1] - ro[v], in double
//   row v keeps the first t(v) entries in the order (sim descending, position ascending), written in row order.
//
// What the passes do:
//   * minhash: each row is read once per 8 hash functions (once for k <= 8), the k hashes computed in ALU (no hash array);
//     rows of at most LSPAR_SHORT_MAX entries go to 8-lane groups, longer ones to a wave per LSPAR_SEG-entry segment, combined
//     by unsigned atomicMin.  The table is n x S, vertex-major, S = k padded to a multiple of 4 (k > 2) for 16-byte loads; the
//     padding columns are never written (all ones on both sides, so they compare equal and are subtracted).
//   * select, short rows: a 16-lane group per row, 4 entries a lane held in registers: the cut level c is found by group ballots
//     from the group's largest sim down, then the kept entries go out in row order.
//   * select, longer rows: a wave per segment; a count kernel writes every segment's sim histogram, a write kernel sums the
//     row's histograms (and those of the segments before its own), finds c and q and writes its kept entries, gathering the
//     neighbours' minhashes again (no staged sims).
//   * out_ro is the exclusive scan of t (scan.hpp); its total is the one host wait.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "color_hash.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int LSPAR_SHORT_MAX = 64;            // rows up to this many entries: the group kernels
constexpr int LSPAR_SEG = 4096;                // entries of a longer row one wave item covers
constexpr int LSPAR_MH_GROUP = 8;              // lanes per short row, minhash pass
constexpr int LSPAR_SEL_GROUP = 16;            // lanes per short row, select pass (x LSPAR_SEL_REGS entries a lane)
constexpr int LSPAR_SEL_REGS = LSPAR_SHORT_MAX / LSPAR_SEL_GROUP;
constexpr int LSPAR_K_MAX = 32;
constexpr unsigned LSPAR_SEED_DEFAULT = 15485863u;

// the keep count t(v) of a row of d entries (host and device: the same double arithmetic)
__host__ __device__ __forceinline__ int lspar_keep(int d, double e) {
  if (d <= 0) return 0;
  const double p = pow((double)d, e) * (1.0 + 1.0 / 1099511627776.0);    // (1 + 2^-40): exact powers stay exact
  if (!(p < (double)d)) return d;
  return (int)floor(p);
}
__host__ __device__ __forceinline__ int lspar_stride(int k) { return k <= 2 ? k : (k + 3) & ~3; }

struct lspar_args_t {
  const int* ro;
  const int* ci;
  int n, k, S;
  unsigned seed;
  double e;
  unsigned* mh;                 // n x S minhashes
  const int* oro;               // out_ro (the scan of t)
  int* oci;
  int* oeid;
  int* osim;
  int2* items;                  // (row, segment) of the rows longer than LSPAR_SHORT_MAX
  int* cnt;                     // [0] items, [1] rows cut (t < d)
  int* seg_hist;                // items x (k + 1): every segment's count per sim level
};

// sim of entry (v, u): equal minhash columns, padding columns subtracted
__device__ __forceinline__ int lspar_sim(const lspar_args_t& a, int v, int u) {
  int s = 0;
  if ((a.S & 3) == 0) {
    const uint4* const x = (const uint4*)(a.mh + (size_t)v * a.S);
    const uint4* const y = (const uint4*)(a.mh + (size_t)u * a.S);
    for (int j = 0; j < (a.S >> 2); ++j) {
      const uint4 p = x[j], q = y[j];
      s += (p.x == q.x) + (p.y == q.y) + (p.z == q.z) + (p.w == q.w);
    }
    return s - (a.S - a.k);
  }
  for (int j = 0; j < a.S; ++j) s += a.mh[(size_t)v * a.S + j] == a.mh[(size_t)u * a.S + j];
  return s;
}

// Rows longer than LSPAR_SHORT_MAX: their segments into the item list; rows cut counted.
__global__ __launch_bounds__(BLOCK) void k_lspar_classify(lspar_args_t a) {
  const int lane = lane_id();
  int cut = 0;
  for (long long base = (long long)blockIdx.x * BLOCK + threadIdx.x - lane; base < a.n; base += (long long)gridDim.x * BLOCK) {
    const int v = (int)base + lane;
    const int d = v < a.n ? a.ro[v + 1] - a.ro[v] : 0;
    cut += (d > 0 && lspar_keep(d, a.e) < d) ? 1 : 0;
    wave_append_segments(d > LSPAR_SHORT_MAX, v, d, LSPAR_SEG, a.items, a.cnt);
  }
  cut = wave_sum(cut);
  if (lane == 0 && cut) atomicAdd(a.cnt + 1, cut);
}

// k hashes of one neighbour into KC running minima (hash functions jc .. jc + KC - 1)
template <int KC>
__device__ __forceinline__ void lspar_mins(unsigned (&mn)[KC], const unsigned (&salt)[KC], int u) {
#pragma unroll
  for (int jj = 0; jj < KC; ++jj) mn[jj] = min(mn[jj], color_key(u, salt[jj]));
}

// minhash, short rows: an 8-lane group per row
template <int KC>
__global__ __launch_bounds__(BLOCK) void k_lspar_minhash_short(lspar_args_t a) {
  constexpr int G = LSPAR_MH_GROUP;
  const int gl = lane_id() & (G - 1);
  const long long groups = (long long)gridDim.x * (BLOCK / G);
  for (long long g = ((long long)blockIdx.x * BLOCK + threadIdx.x) / G; g < a.n; g += groups) {
    const int v = (int)g;
    const int b = a.ro[v], e = a.ro[v + 1];
    if (e - b > LSPAR_SHORT_MAX) continue;                  // (group-uniform) k_lspar_minhash_long
    for (int jc = 0; jc < a.k; jc += KC) {
      unsigned mn[KC], salt[KC];
#pragma unroll
      for (int jj = 0; jj < KC; ++jj) { mn[jj] = 0xFFFFFFFFu; salt[jj] = color_salt(a.seed, jc + jj); }
      for (int p = b + gl; p < e; p += G) lspar_mins<KC>(mn, salt, a.ci[p]);
#pragma unroll
      for (int jj = 0; jj < KC; ++jj)
#pragma unroll
        for (int d = G / 2; d > 0; d >>= 1) mn[jj] = min(mn[jj], (unsigned)__shfl_xor((int)mn[jj], d, WAVE));
#pragma unroll
      for (int jj = 0; jj < KC; ++jj)
        if (gl == jj && jc + jj < a.k) a.mh[(size_t)v * a.S + jc + jj] = mn[jj];
    }
  }
}

// minhash, longer rows: a wave per segment, unsigned atomicMin into the table (filled with ones before)
template <int KC>
__global__ __launch_bounds__(BLOCK) void k_lspar_minhash_long(lspar_args_t a) {
  const int lane = lane_id();
  const int nitems = a.cnt[0];
  const int waves = (int)(gridDim.x * WAVES_PER_BLOCK);
  for (int it = (int)(blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / WAVE); it < nitems; it += waves) {
    const int2 item = a.items[it];
    const int v = item.x;
    const int b = a.ro[v] + item.y * LSPAR_SEG, e = min(a.ro[v + 1], b + LSPAR_SEG);
    for (int jc = 0; jc < a.k; jc += KC) {
      unsigned mn[KC], salt[KC];
#pragma unroll
      for (int jj = 0; jj < KC; ++jj) { mn[jj] = 0xFFFFFFFFu; salt[jj] = color_salt(a.seed, jc + jj); }
      int p = b + lane;
      for (; p + 3 * WAVE < e; p += 4 * WAVE) {             // four loads in flight a lane
        int u[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] = a.ci[p + r * WAVE];
#pragma unroll
        for (int r = 0; r < 4; ++r) lspar_mins<KC>(mn, salt, u[r]);
      }
      for (; p < e; p += WAVE) lspar_mins<KC>(mn, salt, a.ci[p]);
#pragma unroll
      for (int jj = 0; jj < KC; ++jj)
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) mn[jj] = min(mn[jj], (unsigned)__shfl_xor((int)mn[jj], d, WAVE));
#pragma unroll
      for (int jj = 0; jj < KC; ++jj)
        if (lane == jj && jc + jj < a.k) atomicMin(a.mh + (size_t)v * a.S + jc + jj, mn[jj]);
    }
  }
}

__device__ __forceinline__ void lspar_emit(const lspar_args_t& a, int pos, int u, int p, int s) {
  a.oci[pos] = u;
  a.oeid[pos] = p;
  a.osim[pos] = s;
}

// select, short rows: a 16-lane group per row, LSPAR_SEL_REGS entries a lane (entry r * 16 + lane of the row)
__global__ __launch_bounds__(BLOCK) void k_lspar_select_short(lspar_args_t a) {
  constexpr int G = LSPAR_SEL_GROUP, R = LSPAR_SEL_REGS;
  const int lane = lane_id(), gl = lane & (G - 1);
  const u64 gmask = (((u64)1 << G) - 1) << (lane - gl);
  const u64 below = gmask & (((u64)1 << lane) - 1);
  const long long groups = (long long)gridDim.x * (BLOCK / G);
  for (long long g = ((long long)blockIdx.x * BLOCK + threadIdx.x) / G; g < a.n; g += groups) {
    const int v = (int)g;
    const int b = a.ro[v], d = a.ro[v + 1] - b;
    if (d == 0 || d > LSPAR_SHORT_MAX) continue;           // (group-uniform)
    const int ob = a.oro[v], t = a.oro[v + 1] - ob;
    int u[R], s[R];
    int top = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = r * G + gl;
      u[r] = p < d ? a.ci[b + p] : 0;
      s[r] = p < d ? lspar_sim(a, v, u[r]) : -1;
      top = max(top, s[r]);
    }
    if (t == d) {                                          // everything stays
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (s[r] >= 0) lspar_emit(a, ob + r * G + gl, u[r], b + r * G + gl, s[r]);
      continue;
    }
#pragma unroll
    for (int d2 = G / 2; d2 > 0; d2 >>= 1) top = max(top, __shfl_xor(top, d2, WAVE));
    // the cut level c: the largest with #(sim >= c) >= t; `above` = #(sim > c)
    int c = top, above = 0;
    for (;;) {
      int ge = above;
#pragma unroll
      for (int r = 0; r < R; ++r) ge += __popcll(__ballot(s[r] == c) & gmask);
      if (ge >= t || c == 0) break;
      above = ge;
      --c;
    }
    const int q = t - above;
    int kept = 0, at_c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u64 mc = __ballot(s[r] == c) & gmask;
      const bool keep = s[r] > c || (s[r] == c && at_c + __popcll(mc & below) < q);
      const u64 mk = __ballot(keep) & gmask;
      if (keep) lspar_emit(a, ob + kept + __popcll(mk & below), u[r], b + r * G + gl, s[r]);
      at_c += __popcll(mc);
      kept += __popcll(mk);
    }
  }
}

// select, longer rows, step 1: every segment's count per sim level
__global__ __launch_bounds__(BLOCK) void k_lspar_select_count(lspar_args_t a) {
  const int lane = lane_id();
  const int nitems = a.cnt[0];
  const int waves = (int)(gridDim.x * WAVES_PER_BLOCK);
  for (int it = (int)(blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / WAVE); it < nitems; it += waves) {
    const int2 item = a.items[it];
    const int v = item.x;
    const int b = a.ro[v] + item.y * LSPAR_SEG, e = min(a.ro[v + 1], b + LSPAR_SEG);
    int mine = 0;                                          // lane c: entries at level c
    for (int p0 = b; p0 < e; p0 += 4 * WAVE) {
      int s[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + r * WAVE + lane;
        s[r] = p < e ? a.ci[p] : -1;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = s[r] >= 0 ? lspar_sim(a, v, s[r]) : -1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        u64 pend = __ballot(s[r] >= 0);
        while (pend) {                                     // one ballot per level present
          const int l = __shfl(s[r], __ffsll((long long)pend) - 1, WAVE);
          const u64 m = __ballot(s[r] == l);
          if (lane == l) mine += __popcll(m);
          pend &= ~m;
        }
      }
    }
    if (lane <= a.k) a.seg_hist[(size_t)it * (a.k + 1) + lane] = mine;
  }
}

// suffix sum over lanes: lane c gets x(c) + x(c + 1) + ... + x(63)
__device__ __forceinline__ int lspar_suffix_sum(int x) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int y = __shfl_down(x, d, WAVE);
    if (lane + d < WAVE) x += y;
  }
  return x;
}

// select, longer rows, step 2: the row's cut level from the segments' counts, then this segment's kept entries
__global__ __launch_bounds__(BLOCK) void k_lspar_select_write(lspar_args_t a) {
  const int lane = lane_id();
  const int nitems = a.cnt[0];
  const int waves = (int)(gridDim.x * WAVES_PER_BLOCK);
  for (int it = (int)(blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / WAVE); it < nitems; it += waves) {
    const int2 item = a.items[it];
    const int v = item.x;
    const int rb = a.ro[v], d = a.ro[v + 1] - rb;
    const int segs = (d + LSPAR_SEG - 1) / LSPAR_SEG;
    const int first = it - item.y;
    const int ob = a.oro[v], t = a.oro[v + 1] - ob;
    // lane c: the row's count at level c (H) and that of the segments before this one (P)
    int H = 0, P = 0;
    if (lane <= a.k) {
      for (int i = 0; i < segs; ++i) {
        const int x = a.seg_hist[(size_t)(first + i) * (a.k + 1) + lane];
        H += x;
        if (i < item.y) P += x;
      }
    }
    const int ge = lspar_suffix_sum(H), pge = lspar_suffix_sum(P);
    const u64 fits = __ballot(lane <= a.k && ge >= t);      // (bit 0 always: ge(0) = d >= t)
    const int c = 63 - __clzll((long long)fits);
    const int above = __shfl(ge, c, WAVE) - __shfl(H, c, WAVE);
    const int q = t - above;
    const int pc = __shfl(P, c, WAVE);
    int kept = __shfl(pge, c, WAVE) - pc + min(pc, q);        // kept entries of the row before this segment
    int at_c = pc;
    const int b = rb + item.y * LSPAR_SEG, e = min(rb + d, b + LSPAR_SEG);
    const u64 below = ((u64)1 << lane) - 1;
    for (int p0 = b; p0 < e; p0 += 4 * WAVE) {
      int u[4], s[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + r * WAVE + lane;
        u[r] = p < e ? a.ci[p] : -1;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = u[r] >= 0 ? lspar_sim(a, v, u[r]) : -1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u64 mc = __ballot(s[r] == c);
        const bool keep = s[r] > c || (s[r] == c && at_c + __popcll(mc & below) < q);
        const u64 mk = __ballot(keep);
        if (keep) lspar_emit(a, ob + kept + __popcll(mk & below), u[r], p0 + r * WAVE + lane, s[r]);
        at_c += __popcll(mc);
        kept += __popcll(mk);
      }
    }
  }
}

__global__ void k_lspar_total(int* oro, int n, const long long* total) { oro[n] = (int)*total; }

// The device state of a graph's fused sparsification, and the run (host side)
struct lspar_fused_state_t {
  int n = 0;
  long long m = 0;
  mem_t<unsigned> mh;
  int S = 0;
  mem_t<int> oro, oci, oeid, osim;
  mem_t<int2> items;
  mem_t<int> cnt, seg_hist;
  pinned_t<int> h_pinned;           // the item count and rows cut
  long long last_items = -1;        // the last run's item count (mgx_lspar_info; -1: no run yet)

  lspar_fused_state_t(int n_, long long m_, standard_context_t& ctx) : n(n_), m(m_) {
    oro = mem_t<int>((size_t)n + 1, ctx);
    items = mem_t<int2>((size_t)(m / LSPAR_SHORT_MAX + m / LSPAR_SEG + 2), ctx);
    cnt = mem_t<int>(2, ctx);
    ctx.reserve_scratch(scan_scratch_bytes(std::max(n, 1)));
    h_pinned = pinned_t<int>(2);
  }

  // returns {kept entries, rows cut, host waits}; the outputs are complete when the stream is
  std::vector<long long> run(const int* ro, const int* ci, unsigned seed, int k, double e, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    last_items = -1;
    S = lspar_stride(k);
    const size_t cells = (size_t)std::max(n, 1) * S;
    if (mh.size() < cells) mh = mem_t<unsigned>(cells, ctx);
    MGX_HIP(hipMemsetAsync(mh.data(), 0xFF, cells * sizeof(unsigned), st));
    MGX_HIP(hipMemsetAsync(cnt.data(), 0, 2 * sizeof(int), st));
    lspar_args_t a;
    a.ro = ro; a.ci = ci; a.n = n; a.k = k; a.S = S; a.seed = seed; a.e = e;
    a.mh = mh.data(); a.oro = oro.data(); a.oci = a.oeid = a.osim = nullptr;
    a.items = items.data(); a.cnt = cnt.data(); a.seg_hist = nullptr;
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    if (n > 0) {
      hipLaunchKernelGGL(k_lspar_classify, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, a);
      MGX_HIP(hipMemcpyAsync(h_pinned.data(), cnt.data(), 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      const int mh_blocks = grid_for(n, BLOCK / LSPAR_MH_GROUP, max_blocks);
      if (k == 1) {
        hipLaunchKernelGGL(k_lspar_minhash_short<1>, dim3(mh_blocks), dim3(BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_lspar_minhash_long<1>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
      } else {
        hipLaunchKernelGGL(k_lspar_minhash_short<8>, dim3(mh_blocks), dim3(BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_lspar_minhash_long<8>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
      }
      MGX_CHECK_LAUNCH("mgx lspar minhash");
    } else {
      h_pinned[0] = h_pinned[1] = 0;
    }
    long long total = 0;
    const int* const ro_c = ro;
    const long long* d_total = transform_scan([=] __device__(long long v) { return lspar_keep(ro_c[v + 1] - ro_c[v], e); }, (long long)n,
                                              oro.data(), ctx, &total);            // the one host wait
    hipLaunchKernelGGL(k_lspar_total, dim3(1), dim3(1), 0, st, oro.data(), n, d_total);
    const size_t cap = (size_t)std::max<long long>(total, 1);
    if (oci.size() < cap) {
      oci = mem_t<int>(cap, ctx);
      oeid = mem_t<int>(cap, ctx);
      osim = mem_t<int>(cap, ctx);
    }
    a.oci = oci.data(); a.oeid = oeid.data(); a.osim = osim.data();
    const long long nitems = h_pinned[0], cut = h_pinned[1];
    if (n > 0) {
      hipLaunchKernelGGL(k_lspar_select_short, dim3(grid_for(n, BLOCK / LSPAR_SEL_GROUP, max_blocks)), dim3(BLOCK), 0, st, a);
      if (nitems > 0) {
        const size_t hcells = (size_t)nitems * (k + 1);
        if (seg_hist.size() < hcells) seg_hist = mem_t<int>(hcells, ctx);
        a.seg_hist = seg_hist.data();
        const int blocks = (int)std::min<long long>((nitems + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, max_blocks);
        hipLaunchKernelGGL(k_lspar_select_count, dim3(blocks), dim3(BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_lspar_select_write, dim3(blocks), dim3(BLOCK), 0, st, a);
      }
      MGX_CHECK_LAUNCH("mgx lspar select");
    }
    last_items = nitems;
    return {total, cut, 1};
  }
};

}  // namespace mgx
