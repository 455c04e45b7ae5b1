// mgx/cc_fused.hpp -- connected components, fused (mgx_cc_run): Afforest-style union-find on the plain CSR in original ids,
// every phase a launch of its own on the context's stream, one host wait per run (the stats).
//
// The definition (the operator path include/gunrock/cc/ and tests/cc_model.py compute the same):
//   weakly connected components, every CSR entry (v, u) read as the undirected pair {v, u}; self-loops and duplicates change
//   nothing, a vertex without entries is a component of its own.  label[v] = the smallest vertex id of v's component.
//
// The phases:
//   init                comp[v] = v
//   neighbour round r   (r = 0, 1) every v of degree > r links with ci[ro[v] + r]; a compress launch follows each round
//   sample              1024 vertices (color_salt(seed, j) % n); one workgroup finds the most frequent root among them (ties:
//                       the smaller), c, and stores it in a device word
//   work list           from the snapshot the last compress left: the rows still to link of every vertex with comp[v] != c
//                       (skip modes) or of every vertex (no skip) -- short rows an item each, long rows one item per CC_SEG
//                       entries, compacted through a wave-private LDS stage; the counts stay on the device
//   final link          skip mode (symmetric): out-entries from r = 2 on; skip mode with a genuine CSC: those and every
//                       in-entry; no skip (directed, no CSC): out-entries from r = 2 on of every vertex.  An entry whose near
//                       end is in c is seen from its far end, through symmetry or through the CSC, so the skip is sound.
//   final compress, then the shared label reduction (cc_label_stats) and one read-back.
//
// Why it is correct on gfx950, where per-XCD L2s are not coherent within a launch and a CU's L1 is never refreshed by other CUs'
// stores (a plain load of comp[x] in a link launch may be stale for the whole launch):
//   (a) in link launches comp is written only by device-scope atomicCAS;
//   (b) every retry after a CAS uses the value the CAS returned; nothing spins on a load;
//   (c) comp[x] <= x always and values only decrease, so any value a load returns, however stale, is an ancestor in x's set:
//       a walk on such loads moves to ancestors, and every step of cc_link strictly lowers the larger of its two roots, so the
//       loop ends within n steps;
//   (d) compress launches link nothing: they shorten paths with plain stores while no root changes.
// A root only ever links to a smaller root, so a set's root is its smallest member: after the final compress comp is the
// label array, and the partition after the two neighbour rounds (hence c and stats[3]) does not depend on the races.
#pragma once
#include <algorithm>
#include <vector>

#include "color_hash.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int CC_SEG = 2048;              // entries of a long row one wave links
constexpr int CC_LONG_MIN = 32;           // rows of at least this many entries left to link are long
constexpr int CC_SAMPLES = 1024;          // vertices the sample looks at
constexpr int CC_SAMPLE_SLOTS = 2048;     // its LDS hash table (a power of two above CC_SAMPLES)
constexpr int CC_NEIGHBOR_ROUNDS = 2;
constexpr unsigned CC_SEED_DEFAULT = 15485863u;
constexpr int CC_STAGE = 2 * WAVE;        // a wave's LDS stage of short-row items

enum cc_mode_t { CC_SKIP = 0, CC_SKIP_CSC = 1, CC_NO_SKIP = 2 };

__device__ __forceinline__ int cc_load(const int* comp, int x) {
  return __hip_atomic_load(comp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Union the sets of u and v (rules (a) - (c) above).  high strictly decreases from one pass of the loop to the next.
__device__ __forceinline__ void cc_link(int* comp, int u, int v) {
  int p1 = cc_load(comp, u), p2 = cc_load(comp, v);
  while (p1 != p2) {
    const int high = max(p1, p2), low = min(p1, p2);
    const int ph = cc_load(comp, high);
    if (ph == low) return;                                   // linked already (values only decrease: it stays so)
    if (ph == high) {
      const int old = atomicCAS(comp + high, high, low);
      if (old == high) return;                               // high was a root and now hangs under low
      p1 = old;                                              // high is no root: go on from what the CAS saw, < high
    } else {
      p1 = cc_load(comp, ph);                                // ph < high
    }
    p2 = cc_load(comp, low);                                 // <= low < high
  }
}

__global__ __launch_bounds__(BLOCK) void k_cc_init(int* comp, int n) {
  for (long long v = (long long)blockIdx.x * BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * BLOCK) comp[v] = (int)v;
}

// neighbour round r: every v of degree > r links with its r-th entry
__global__ __launch_bounds__(BLOCK) void k_cc_neighbor(const int* ro, const int* ci, int* comp, int n, int r) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const int beg = ro[v];
    if (ro[v + 1] - beg > r) cc_link(comp, v, ci[beg + r]);
  }
}

// every comp[v] becomes its root (no link runs meanwhile: roots stand still, paths only get shorter)
__global__ __launch_bounds__(BLOCK) void k_cc_compress(int* comp, int n) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const int p = comp[v];
    int x = p, y;
    while ((y = comp[x]) != x) x = y;
    if (x != p) comp[v] = x;
  }
}

// One workgroup: the most frequent value of comp over the samples color_salt(seed, j) % n, j < CC_SAMPLES (ties: the smaller)
// -> *out.  comp holds roots (a compress ran last).
__global__ __launch_bounds__(BLOCK) void k_cc_sample(const int* comp, int n, unsigned seed, int* out) {
  __shared__ int keys[CC_SAMPLE_SLOTS];
  __shared__ int counts[CC_SAMPLE_SLOTS];
  __shared__ u64 best_of_wave[WAVES_PER_BLOCK];
  for (int i = threadIdx.x; i < CC_SAMPLE_SLOTS; i += BLOCK) {
    keys[i] = -1;
    counts[i] = 0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < CC_SAMPLES; j += BLOCK) {
    const int r = comp[color_salt(seed, j) % (unsigned)n];
    unsigned h = color_fmix32((unsigned)r) & (CC_SAMPLE_SLOTS - 1);
    for (int probe = 0; probe < CC_SAMPLE_SLOTS; ++probe) {  // (at most CC_SAMPLES keys: a free slot or r is always found)
      const int k = atomicCAS(keys + h, -1, r);
      if (k == -1 || k == r) {
        atomicAdd(counts + h, 1);
        break;
      }
      h = (h + 1) & (CC_SAMPLE_SLOTS - 1);
    }
  }
  __syncthreads();
  u64 best = 0;                                              // (count << 32) | ~root: the largest count, then the smallest root
  for (int i = threadIdx.x; i < CC_SAMPLE_SLOTS; i += BLOCK)
    if (counts[i]) best = max(best, ((u64)counts[i] << 32) | (u32)~keys[i]);
  best = wave_max(best);
  if (lane_id() == 0) best_of_wave[threadIdx.x / WAVE] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) best = max(best, best_of_wave[w]);
    *out = (int)~(u32)best;
  }
}

struct cc_list_args_t {
  const int* ro;
  const int* ci;
  const int* co;                 // the genuine CSC (CC_SKIP_CSC only)
  const int* ri;
  const int* comp;
  const int* c_word;             // the sampled root (skip modes)
  int n;
  int mode;
  int* s_list;                   // short rows: v (out-entries from r = 2 on) or ~v (in-entries)
  int2* l_list;                  // long rows: (v or ~v, segment)
  int* cnt;                      // [0] short rows, [1] long items
  u64* skipped;
};

// short rows through the wave's LDS stage, long rows' segments behind one add per wave and pass (worklist.hpp)
__global__ __launch_bounds__(BLOCK) void k_cc_worklist(cc_list_args_t a) {
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (BLOCK / WAVE));
  __shared__ int s_stage[WAVES_PER_BLOCK][CC_STAGE];
  int* const stage = s_stage[threadIdx.x / WAVE];
  int fill = 0, skipped = 0;
  const int c = a.mode == CC_NO_SKIP ? -1 : *a.c_word;
  for (long long base = (long long)wave * WAVE; base < a.n; base += (long long)waves * WAVE) {
    const int v = (int)base + lane;
    const bool in = v < a.n;
    const int out_len = in ? max(a.ro[v + 1] - a.ro[v] - CC_NEIGHBOR_ROUNDS, 0) : 0;
    const int in_len = in && a.mode == CC_SKIP_CSC ? a.co[v + 1] - a.co[v] : 0;
    const bool has = out_len + in_len > 0;
    const bool skip = has && a.mode != CC_NO_SKIP && a.comp[v] == c;
    skipped += __popcll(__ballot(skip));
    const bool out_go = has && !skip && out_len > 0, in_go = has && !skip && in_len > 0;
    wave_stage_push<CC_STAGE>(out_go && out_len < CC_LONG_MIN, v, stage, fill, a.s_list, a.cnt);
    wave_stage_push<CC_STAGE>(in_go && in_len < CC_LONG_MIN, ~v, stage, fill, a.s_list, a.cnt);
    wave_append_segments(out_go && out_len >= CC_LONG_MIN, v, out_len, CC_SEG, a.l_list, a.cnt + 1);
    wave_append_segments(in_go && in_len >= CC_LONG_MIN, ~v, in_len, CC_SEG, a.l_list, a.cnt + 1);
  }
  wave_stage_flush(stage, fill, a.s_list, a.cnt);
  if (lane == 0 && skipped) atomicAdd(a.skipped, (u64)skipped);
}

struct cc_link_args_t {
  const int* ro;
  const int* ci;
  const int* co;
  const int* ri;
  int* comp;
  const int* s_list;
  const int2* l_list;
  const int* cnt;
};

// the entries [beg, end) an item stands for: v's out-entries from r = 2 on (item >= 0) or all of v's in-entries (item = ~v)
__device__ __forceinline__ const int* cc_item_row(const cc_link_args_t& a, int item, int& v, int& beg, int& end) {
  if (item >= 0) {
    v = item;
    beg = a.ro[v] + CC_NEIGHBOR_ROUNDS;
    end = a.ro[v + 1];
    return a.ci;
  }
  v = ~item;
  beg = a.co[v];
  end = a.co[v + 1];
  return a.ri;
}

// the final link: long items a wave each, then short rows a thread each; the grid is sized to the chip, the counts come from
// the device
__global__ __launch_bounds__(BLOCK) void k_cc_link(cc_link_args_t a) {
  const int ns = a.cnt[0], nl = a.cnt[1];
  const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const long long gthreads = (long long)gridDim.x * BLOCK;
  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE), waves = (int)(gthreads / WAVE);
  for (int it = wave; it < nl; it += waves) {
    const int2 item = a.l_list[it];
    int v, beg, end;
    const int* const nbr = cc_item_row(a, item.x, v, beg, end);
    const int s1 = min(end, beg + (item.y + 1) * CC_SEG);
    for (int e = beg + item.y * CC_SEG + lane; e < s1; e += WAVE) cc_link(a.comp, v, nbr[e]);
  }
  for (long long i = gtid; i < ns; i += gthreads) {
    int v, beg, end;
    const int* const nbr = cc_item_row(a, a.s_list[i], v, beg, end);
    for (int e = beg; e < end; ++e) cc_link(a.comp, v, nbr[e]);
  }
}

// ---- the shared label reduction (both paths; not part of either algorithm) ----
// sizes[label] over every vertex: the hot label (*hot, the sampled root) through one add per workgroup, every other label
// through one add per wave and label for the lanes that share the wave's first, one add per lane for the rest
__global__ __launch_bounds__(BLOCK) void k_cc_sizes(const int* label, int n, const int* hot, int* sizes) {
  __shared__ int hot_count;
  if (threadIdx.x == 0) hot_count = 0;
  __syncthreads();
  const int h = *hot;
  const int lane = lane_id();
  int mine = 0;
  for (long long base = (long long)blockIdx.x * BLOCK + (threadIdx.x - lane); base < n; base += (long long)gridDim.x * BLOCK) {
    const int v = (int)base + lane;
    const int l = v < n ? label[v] : -1;
    mine += __popcll(__ballot(l == h && l >= 0));
    const bool rest = l >= 0 && l != h;
    const u64 m = __ballot(rest);
    if (!m) continue;
    const int first = __ffsll((long long)m) - 1;
    const int lf = __shfl(l, first, WAVE);
    const u64 same = __ballot(rest && l == lf);
    if (lane == first) atomicAdd(sizes + lf, __popcll(same));
    else if (rest && l != lf) atomicAdd(sizes + l, 1);
  }
  if (lane == 0 && mine) atomicAdd(&hot_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && hot_count) atomicAdd(sizes + h, hot_count);
}

// out[0] = max over roots of (size << 32) | ~root (largest, then the smallest label), out[1] = number of roots; one add and one max
// per workgroup (the two words are single: one pair per wave over a chip-sized grid cost RMAT-22 0.2 ms)
__global__ __launch_bounds__(BLOCK) void k_cc_largest(const int* label, int n, const int* sizes, u64* out) {
  __shared__ u64 s_best[WAVES_PER_BLOCK], s_roots[WAVES_PER_BLOCK];
  u64 best = 0, roots = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    if (label[v] == v) {
      ++roots;
      best = max(best, ((u64)(u32)sizes[v] << 32) | (u32)~v);
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    best = max(best, (u64)__shfl_xor(best, d, WAVE));
    roots += (u64)__shfl_xor(roots, d, WAVE);
  }
  if (lane_id() == 0) {
    s_best[threadIdx.x / WAVE] = best;
    s_roots[threadIdx.x / WAVE] = roots;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) {
      best = max(best, s_best[w]);
      roots += s_roots[w];
    }
    if (roots) atomicAdd(out + 1, roots);
    if (best) atomicMax(out, best);
  }
}

// The device side of both paths' stats: sizes (n ints) and out (2 words) are cleared here, *hot is read on the device.
inline void cc_label_stats(const int* label, int n, const int* hot, int* sizes, u64* out, int max_blocks, hipStream_t st) {
  MGX_HIP(hipMemsetAsync(out, 0, 2 * sizeof(u64), st));
  if (n <= 0) return;
  MGX_HIP(hipMemsetAsync(sizes, 0, (size_t)n * sizeof(int), st));
  hipLaunchKernelGGL(k_cc_sizes, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, label, n, hot, sizes);
  hipLaunchKernelGGL(k_cc_largest, dim3(grid_for(n, BLOCK, std::max(max_blocks / 8, 1))), dim3(BLOCK), 0, st, label, n,
                     (const int*)sizes, out);
  MGX_CHECK_LAUNCH("mgx cc label stats");
}

// host view of the words cc_label_stats left: {components, largest, its label}
inline void cc_unpack_stats(const u64* w, long long* out) {
  out[0] = (long long)w[1];
  out[1] = (long long)(w[0] >> 32);
  out[2] = w[0] ? (long long)(int)~(u32)w[0] : 0;
}

// The reduction on its own, for labels that come with no sampled root (the operator path): the sample kernel picks the hot label
// from the labels first.  One host wait.
struct cc_label_stats_t {
  mem_t<int> sizes;
  mem_t<int> hot;
  mem_t<u64> out;
  pinned_t<u64> h_pinned;

  cc_label_stats_t(int n, context_t& ctx) {
    sizes = mem_t<int>((size_t)std::max(n, 1), ctx);
    hot = mem_t<int>(1, ctx);
    out = mem_t<u64>(2, ctx);
    h_pinned = pinned_t<u64>(2);
  }

  // {components, largest, its label} of a label array of n entries on the device
  std::vector<long long> run(const int* label, int n, standard_context_t& ctx) {
    if (n <= 0) return {0, 0, 0};
    const hipStream_t st = ctx.stream();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    hipLaunchKernelGGL(k_cc_sample, dim3(1), dim3(BLOCK), 0, st, label, n, CC_SEED_DEFAULT, hot.data());
    cc_label_stats(label, n, hot.data(), sizes.data(), out.data(), max_blocks, st);
    h_pinned.fetch(out.data(), 2, st);
    long long s[3];
    cc_unpack_stats(h_pinned.data(), s);
    return {s[0], s[1], s[2]};
  }
};

// The device state of a graph's fused CC, and the run (host side)
struct cc_fused_state_t {
  int n = 0;
  mem_t<int> comp;                  // the labels after a run
  mem_t<int> sizes;
  mem_t<int> s_list;                // 2n: an out item and an in item per vertex at most
  mem_t<int2> l_list;
  mem_t<int> words;                 // [0] short count, [1] long items, [2] c
  mem_t<u64> stat;                  // [0] packed largest, [1] components, [2] skipped
  pinned_t<u64> h_pinned;           // the one read-back
  long long l_cap = 0;

  cc_fused_state_t(int n_, long long m, context_t& ctx) : n(n_) {
    const size_t N = (size_t)std::max(n, 1);
    comp = mem_t<int>(N, ctx);
    sizes = mem_t<int>(N, ctx);
    s_list = mem_t<int>(2 * N, ctx);
    // long items, per side: at most min(n, m / CC_LONG_MIN) rows, plus one item per CC_SEG entries beyond their first segment
    l_cap = 2 * (std::min<long long>((long long)N, m / CC_LONG_MIN + 1) + m / CC_SEG + 1);
    l_list = mem_t<int2>((size_t)l_cap, ctx);
    words = mem_t<int>(4, ctx);
    stat = mem_t<u64>(4, ctx);
    h_pinned = pinned_t<u64>(4);
  }

  // Label the graph (ro, ci: CSR on the device; co, ri: its genuine CSC or nullptr).  symmetric: the caller's word that every
  // entry has its reverse.  Returns {components, largest, its label, skipped, host waits}.
  std::vector<long long> run(const int* ro, const int* ci, const int* co, const int* ri, bool symmetric, unsigned seed,
                             standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    if (n <= 0) return {0, 0, 0, 0, 0};
    const int mode = symmetric ? CC_SKIP : (co ? CC_SKIP_CSC : CC_NO_SKIP);
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const int grid_n = grid_for(n, BLOCK, max_blocks);
    MGX_HIP(hipMemsetAsync(words.data(), 0, 4 * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(stat.data() + 2, 0, sizeof(u64), st));
    hipLaunchKernelGGL(k_cc_init, dim3(grid_n), dim3(BLOCK), 0, st, comp.data(), n);
    for (int r = 0; r < CC_NEIGHBOR_ROUNDS; ++r) {
      hipLaunchKernelGGL(k_cc_neighbor, dim3(grid_n), dim3(BLOCK), 0, st, ro, ci, comp.data(), n, r);
      hipLaunchKernelGGL(k_cc_compress, dim3(grid_n), dim3(BLOCK), 0, st, comp.data(), n);
    }
    int* const c_word = words.data() + 2;
    hipLaunchKernelGGL(k_cc_sample, dim3(1), dim3(BLOCK), 0, st, (const int*)comp.data(), n, seed, c_word);
    cc_list_args_t la;
    la.ro = ro; la.ci = ci; la.co = co; la.ri = ri; la.comp = comp.data(); la.c_word = c_word; la.n = n; la.mode = mode;
    la.s_list = s_list.data(); la.l_list = l_list.data(); la.cnt = words.data(); la.skipped = stat.data() + 2;
    hipLaunchKernelGGL(k_cc_worklist, dim3(grid_n), dim3(BLOCK), 0, st, la);
    cc_link_args_t ka;
    ka.ro = ro; ka.ci = ci; ka.co = co; ka.ri = ri; ka.comp = comp.data();
    ka.s_list = s_list.data(); ka.l_list = l_list.data(); ka.cnt = words.data();
    hipLaunchKernelGGL(k_cc_link, dim3(max_blocks), dim3(BLOCK), 0, st, ka);
    hipLaunchKernelGGL(k_cc_compress, dim3(grid_n), dim3(BLOCK), 0, st, comp.data(), n);
    MGX_CHECK_LAUNCH("mgx cc run");
    cc_label_stats(comp.data(), n, c_word, sizes.data(), stat.data(), max_blocks, st);
    h_pinned.fetch(stat.data(), 3, st);
    long long s[3];
    cc_unpack_stats(h_pinned.data(), s);
    return {s[0], s[1], s[2], (long long)h_pinned[2], 1};
  }
};

}  // namespace mgx
