// mgx/color_fused.hpp -- graph colouring, fused (mgx_color_run): one launch per round, batches of rounds per host wait.
//
// The definition (the operator path include/gunrock/coloring/ and tests/coloring_model.py compute the same):
//   salt_i = fmix32(seed + 0x9E3779B9 * (i + 1)),  key_i(v) = fmix32(v ^ salt_i)   -- a bijection: no two vertices tie
//   round i, every v uncoloured at the START of the round: key_i(v) below every other uncoloured neighbour -> 2i + 1,
//   else above every other uncoloured neighbour -> 2i + 2.  Comparisons unsigned; a self-loop changes nothing.
//
// What a round does here:
//   * "uncoloured" is a bitmap (n / 32 words, L2-resident), three of them rotated: round i reads B[i % 3], ORs its survivors
//     into B[(i + 1) % 3] and clears B[(i + 2) % 3] (read by round i - 1, written by round i + 1) -- rounds are separate
//     launches, so round i decides on the state at its start without a grid barrier;
//   * keys come from the vertex id in ALU (no hash array); a row stops at its first uncoloured neighbour below and above;
//   * only the active vertices are visited: short rows (< long_min entries) a thread each, from a list of vertex ids; long
//     rows a wave per SEGMENT of COLOR_SEG entries, from a list of (vertex, segment) items.  A row of several segments is
//     decided by the wave that arrives last at its 64-bit tally (arrivals | segments that saw a key below | above);
//   * survivors are compacted into the next round's lists through a wave-private LDS stage: one returning add per 64 - 128
//     of them;
//   * the counts (per round: short rows, long items, long rows) live on the device; a round whose count is 0 returns at
//     once, so the host enqueues rounds in batches and waits once per batch.
// Round 0 needs no bitmap (every vertex is uncoloured): k_color_first walks 0 .. n - 1, decides the short rows and lists the
// long rows' segments, which the round kernel then decides.
#pragma once
#include <algorithm>
#include <vector>

#include "color_hash.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int COLOR_SEG = 2048;          // entries of a long row one wave scans
constexpr int COLOR_LONG_MIN = 32;       // rows of at least this many entries are long
constexpr int COLOR_BATCH_MAX = 128;     // rounds per host wait, at most
constexpr unsigned COLOR_SEED_DEFAULT = 15485863u;

// the segment tally of a split row: arrivals, segments that saw a key below, above -- 21 bits each
constexpr int COLOR_TALLY_SHIFT = 21;
constexpr unsigned long long COLOR_TALLY_MASK = (1ull << COLOR_TALLY_SHIFT) - 1;

struct color_round_args_t {
  const int* ro;
  const int* ci;
  int* colour;
  const unsigned* bm_cur;          // uncoloured at the start of the round (not read by round 0)
  unsigned* bm_next;               // the round's survivors
  uint4* bm_zero;                  // the third bitmap, cleared here
  unsigned zero4;                  // its size in uint4 (0: nothing to clear)
  const int* s_in;                 // short rows of the round
  int* s_out;
  const int2* l_in;                // (vertex, segment) items of the round's long rows
  int2* l_out;
  const int* cnt_in;               // [0] short rows, [1] long items, [2] long rows of this round
  int* cnt_out;                    // ... of the next, counted here
  unsigned long long* tally;       // per vertex: the segment tally of a split row (0 between rounds)
  int* max_colour;
  unsigned salt;
  int c_lo;                        // 2i + 1
  int long_min;
};

__device__ __forceinline__ bool color_uncoloured(const unsigned* bm, int u) { return (bm[u >> 5] >> (u & 31)) & 1u; }

// one wave: after a round's decisions, the largest colour any of its lanes gave (one atomic per wave, if any)
__device__ __forceinline__ void color_note_max(int* max_colour, int mine) {
  mine = wave_max(mine);
  if (lane_id() == 0 && mine > 0 && __hip_atomic_load(max_colour, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine)
    atomicMax(max_colour, mine);
}

// a short row, one thread: 2i + 1, 2i + 2, or 0 (survives)
template <bool ALL>
__device__ __forceinline__ int color_short_row(const color_round_args_t& a, int v) {
  const unsigned kv = color_key(v, a.salt);
  const int end = a.ro[v + 1];
  bool below = false, above = false;
  for (int e = a.ro[v]; e < end; ++e) {
    const int u = a.ci[e];
    if (!ALL && !color_uncoloured(a.bm_cur, u)) continue;
    const unsigned k = color_key(u, a.salt);
    below |= k < kv;
    above |= k > kv;
    if (below && above) break;
  }
  return !below ? a.c_lo : (!above ? a.c_lo + 1 : 0);
}

// a wave's LDS stage of survivors (worklist.hpp): one for the short rows -- they go into the stage (then the next round's list) and
// into the next round's bitmap -- and one for the long rows' items
constexpr int COLOR_STAGE = 2 * WAVE;

// Round 0, before the round kernel: vertices 0 .. n - 1 -- short rows decided (every neighbour is uncoloured), long rows'
// segments listed into l_out / cnt_out[1], [2] (the round kernel of round 0 reads them with cnt_out[0] == 0).
__global__ __launch_bounds__(BLOCK) void k_color_first(color_round_args_t a, int n, int2* l0, int* cnt0) {
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (BLOCK / WAVE));
  __shared__ int s_stage[WAVES_PER_BLOCK][COLOR_STAGE];
  int* const stage = s_stage[threadIdx.x / WAVE];
  int fill = 0, long_rows = 0;
  int top = 0;
  for (long long base = (long long)wave * WAVE; base < n; base += (long long)waves * WAVE) {
    const int v = (int)base + lane;
    const bool in = v < n;
    const int deg = in ? a.ro[v + 1] - a.ro[v] : 0;
    const bool is_long = in && deg >= a.long_min;
    int c = 0;
    if (in && !is_long) c = color_short_row<true>(a, v);
    if (c) a.colour[v] = c;
    top = max(top, c);
    const bool keep = in && !is_long && c == 0;
    wave_stage_push<COLOR_STAGE>(keep, v, stage, fill, a.s_out, a.cnt_out);
    if (keep) atomicOr(a.bm_next + (v >> 5), 1u << (v & 31));
    // long rows: their segments into round 0's item list (one add per wave and pass)
    wave_append_segments(is_long, v, deg, COLOR_SEG, l0, cnt0 + 1);
    long_rows += __popcll(__ballot(is_long));
  }
  wave_stage_flush(stage, fill, a.s_out, a.cnt_out);
  if (lane == 0 && long_rows) atomicAdd(cnt0 + 2, long_rows);
  color_note_max(a.max_colour, top);
}

// One round (round 0 with ALL: no bitmap read).  Long items first (a wave each), then short rows (a thread each).
template <bool ALL>
__global__ __launch_bounds__(BLOCK) void k_color_round(color_round_args_t a) {
  const int ns = a.cnt_in[0], nl = a.cnt_in[1];
  if (ns + nl == 0) return;                                // the rounds of a batch behind the last one
  const int lane = lane_id();
  const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const long long gthreads = (long long)gridDim.x * BLOCK;
  for (long long w = gtid; w < (long long)a.zero4; w += gthreads) a.bm_zero[w] = make_uint4(0u, 0u, 0u, 0u);
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  __shared__ int2 l_stages[WAVES_PER_BLOCK][COLOR_STAGE];
  __shared__ int s_stages[WAVES_PER_BLOCK][COLOR_STAGE];
  int2* const l_stage = l_stages[threadIdx.x / WAVE];
  int* const s_stage = s_stages[threadIdx.x / WAVE];
  int l_fill = 0, s_fill = 0, long_rows = 0;
  int top = 0;

  for (int it = wave; it < nl; it += waves) {
    const int2 item = a.l_in[it];
    const int v = item.x;
    const int beg = a.ro[v], end = a.ro[v + 1];
    const int segs = (end - beg + COLOR_SEG - 1) / COLOR_SEG;
    const int s0 = beg + item.y * COLOR_SEG, s1 = min(end, s0 + COLOR_SEG);
    const unsigned kv = color_key(v, a.salt);
    bool below = false, above = false;                     // wave-uniform: from ballots
    bool seen_both = false;
    if (segs > 1) {
      // another segment of this row has seen both already: nothing left to find here
      unsigned long long t = 0;
      if (lane == 0) t = __hip_atomic_load(a.tally + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      t = __shfl(t, 0, WAVE);
      seen_both = ((t >> COLOR_TALLY_SHIFT) & COLOR_TALLY_MASK) && (t >> (2 * COLOR_TALLY_SHIFT));
    }
    for (int base = s0; base < s1 && !seen_both; base += 4 * WAVE) {
      int u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = base + j * WAVE + lane;
        u[j] = e < s1 ? a.ci[e] : -1;
      }
      bool b = false, ab = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (u[j] >= 0 && (ALL || color_uncoloured(a.bm_cur, u[j]))) {
          const unsigned k = color_key(u[j], a.salt);
          b |= k < kv;
          ab |= k > kv;
        }
      }
      below |= __ballot(b) != 0;
      above |= __ballot(ab) != 0;
      if (below && above) break;
    }
    if (segs > 1) {
      const unsigned long long add = 1ull | ((unsigned long long)below << COLOR_TALLY_SHIFT) | ((unsigned long long)above << (2 * COLOR_TALLY_SHIFT));
      unsigned long long t = 0;
      if (lane == 0) t = atomicAdd(a.tally + v, add) + add;
      t = __shfl(t, 0, WAVE);
      if ((int)(t & COLOR_TALLY_MASK) != segs) continue;   // not the last segment to arrive
      if (lane == 0) a.tally[v] = 0;                       // ready for the next round (a later launch)
      below = (t >> COLOR_TALLY_SHIFT) & COLOR_TALLY_MASK;
      above = (t >> (2 * COLOR_TALLY_SHIFT)) != 0;
    }
    const int c = !below ? a.c_lo : (!above ? a.c_lo + 1 : 0);
    if (c) {
      if (lane == 0) a.colour[v] = c;
      top = max(top, c);
    } else {
      if (lane == 0) atomicOr(a.bm_next + (v >> 5), 1u << (v & 31));
      ++long_rows;
      if (segs > COLOR_STAGE - l_fill) wave_stage_flush(l_stage, l_fill, a.l_out, a.cnt_out + 1);
      if (segs > COLOR_STAGE) {                            // (a row of more than COLOR_STAGE segments goes out on its own)
        int base_i = 0;
        if (lane == 0) base_i = atomicAdd(a.cnt_out + 1, segs);
        base_i = __shfl(base_i, 0, WAVE);
        for (int s = lane; s < segs; s += WAVE) a.l_out[base_i + s] = make_int2(v, s);
      } else {
        for (int s = lane; s < segs; s += WAVE) l_stage[l_fill + s] = make_int2(v, s);
        l_fill += segs;
      }
    }
  }
  wave_stage_flush(l_stage, l_fill, a.l_out, a.cnt_out + 1);
  if (lane == 0 && long_rows) atomicAdd(a.cnt_out + 2, long_rows);

  for (long long base = (long long)wave * WAVE; base < ns; base += (long long)waves * WAVE) {
    const long long i = base + lane;
    const bool in = i < ns;
    const int v = in ? a.s_in[i] : 0;
    const int c = in ? color_short_row<ALL>(a, v) : 0;
    if (c) a.colour[v] = c;
    top = max(top, c);
    const bool keep = in && c == 0;
    wave_stage_push<COLOR_STAGE>(keep, v, s_stage, s_fill, a.s_out, a.cnt_out);
    if (keep) atomicOr(a.bm_next + (v >> 5), 1u << (v & 31));
  }
  wave_stage_flush(s_stage, s_fill, a.s_out, a.cnt_out);
  color_note_max(a.max_colour, top);
}

// The device state of a graph's fused colouring, and the run (host side)
struct color_fused_state_t {
  int n = 0;
  mem_t<int> colour;
  mem_t<uint4> bm;                  // three bitmaps, words4 uint4 each
  unsigned words4 = 0;
  mem_t<int> s_list[2];
  mem_t<int2> l_list[2];
  mem_t<unsigned long long> tally;
  mem_t<int> cnt;                   // 3 per round (+ 3 for the round behind the last)
  mem_t<int> max_colour;
  pinned_t<int> h_pinned;           // one batch's counts + the largest colour
  long long l_cap = 0;
  // the last run, per round run: short rows, long items, long rows at the start of the round (mgx_color_info); round 0's short
  // rows are the vertices of fewer than long_min entries.  has_run: a run has finished.
  std::vector<long long> round_rows;
  bool has_run = false;

  color_fused_state_t(int n_, long long m, context_t& ctx) : n(n_) {
    const size_t N = (size_t)std::max(n, 1);
    colour = mem_t<int>(N, ctx);
    words4 = (unsigned)((N + 127) / 128);
    bm = mem_t<uint4>((size_t)words4 * 3, ctx);
    // long items: at most min(n, m / long_min) rows, plus one item per COLOR_SEG entries beyond their first segment
    l_cap = std::min<long long>((long long)N, m / COLOR_LONG_MIN + 1) + m / COLOR_SEG + 1;
    for (int k = 0; k < 2; ++k) {
      s_list[k] = mem_t<int>(N, ctx);
      l_list[k] = mem_t<int2>((size_t)l_cap, ctx);
    }
    tally = mem_t<unsigned long long>(N, ctx);
    MGX_HIP(hipMemsetAsync(tally.data(), 0, N * sizeof(unsigned long long), ctx.stream()));
    max_colour = mem_t<int>(1, ctx);
    h_pinned = pinned_t<int>(3 * (COLOR_BATCH_MAX + 2) + 1);
  }

  // Colour the graph (ro, ci: CSR on the device) from all-uncoloured.  trace gets the active vertices at the start of every round
  // run; returns {rounds, left uncoloured, largest colour, host waits}.
  std::vector<long long> run(const int* ro, const int* ci, unsigned seed, int max_iter, standard_context_t& ctx,
                             std::vector<long long>& trace) {
    const hipStream_t st = ctx.stream();
    trace.clear();
    round_rows.clear();
    has_run = false;
    const long long half = ((long long)n + 1) / 2;
    const long long cap = max_iter > 0 ? std::min<long long>(max_iter, half) : half;
    if (cnt.size() < (size_t)(3 * (cap + 2))) {
      MGX_HIP(hipStreamSynchronize(st));
      cnt = mem_t<int>((size_t)(3 * (cap + 2)), ctx);
    }
    MGX_HIP(hipMemsetAsync(colour.data(), 0, (size_t)std::max(n, 1) * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(bm.data(), 0, (size_t)words4 * 3 * sizeof(uint4), st));
    MGX_HIP(hipMemsetAsync(max_colour.data(), 0, sizeof(int), st));
    long long waits = 0, rounds = 0, left = n;
    if (cap == 0) { has_run = true; return {0, (long long)n, 0, 0}; }

    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    auto blocks_for = [&](long long s, long long items) {
      long long b = (s + BLOCK - 1) / BLOCK + (items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      b = std::max<long long>(b, ((long long)words4 + 1023) / 1024);
      return (int)std::min<long long>(std::max<long long>(b, 1), max_blocks);
    };
    auto args_for = [&](long long i) {
      color_round_args_t a;
      a.ro = ro; a.ci = ci; a.colour = colour.data();
      a.bm_cur = (const unsigned*)(bm.data() + (size_t)(i % 3) * words4);
      a.bm_next = (unsigned*)(bm.data() + (size_t)((i + 1) % 3) * words4);
      a.bm_zero = bm.data() + (size_t)((i + 2) % 3) * words4;
      a.zero4 = i == 0 ? 0u : words4;          // (round 0: the third bitmap is still clear)
      a.s_in = s_list[i & 1].data(); a.s_out = s_list[(i + 1) & 1].data();
      a.l_in = l_list[i & 1].data(); a.l_out = l_list[(i + 1) & 1].data();
      a.cnt_in = cnt.data() + 3 * i; a.cnt_out = cnt.data() + 3 * (i + 1);
      a.tally = tally.data(); a.max_colour = max_colour.data();
      a.salt = color_salt(seed, (int)i); a.c_lo = (int)(2 * i + 1); a.long_min = COLOR_LONG_MIN;
      return a;
    };

    long long known_s = n, known_items = n;      // what the next batch's first round has (an upper bound before the first wait)
    long long i = 0;
    std::vector<long long> cnt_host;
    while (i < cap) {
      const long long b = std::min<long long>(cap - i, std::min<long long>(std::max<long long>(i, 8), COLOR_BATCH_MAX));
      // the batch's out-counters (and round 0's own) start at 0
      MGX_HIP(hipMemsetAsync(cnt.data() + 3 * (i == 0 ? 0 : i + 1), 0, (size_t)(3 * (i == 0 ? b + 1 : b)) * sizeof(int), st));
      const int blocks = blocks_for(known_s, known_items);
      for (long long r = i; r < i + b; ++r) {
        color_round_args_t a = args_for(r);
        if (r == 0) {
          hipLaunchKernelGGL(k_color_first, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, a, n, l_list[0].data(), cnt.data());
          hipLaunchKernelGGL(k_color_round<true>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
        } else {
          hipLaunchKernelGGL(k_color_round<false>, dim3(blocks), dim3(BLOCK), 0, st, a);
        }
      }
      MGX_CHECK_LAUNCH("mgx color round");
      MGX_HIP(hipMemcpyAsync(h_pinned.data(), cnt.data() + 3 * i, (size_t)(3 * (b + 1)) * sizeof(int), hipMemcpyDeviceToHost, st));
      MGX_HIP(hipMemcpyAsync(h_pinned.data() + 3 * (COLOR_BATCH_MAX + 2), max_colour.data(), sizeof(int), hipMemcpyDeviceToHost, st));
      MGX_HIP(hipStreamSynchronize(st));
      ++waits;
      for (long long r = 0; r <= b; ++r) {
        const long long active = (i + r == 0) ? (long long)n : (long long)h_pinned[3 * r] + h_pinned[3 * r + 2];
        left = active;
        if (r == b || active == 0) break;
        trace.push_back(active);
        round_rows.push_back(i + r == 0 ? (long long)n - h_pinned[2] : (long long)h_pinned[3 * r]);
        round_rows.push_back(h_pinned[3 * r + 1]);
        round_rows.push_back(h_pinned[3 * r + 2]);
        ++rounds;
      }
      i += b;
      known_s = h_pinned[3 * b];
      known_items = h_pinned[3 * b + 1];
      if (left == 0) break;
    }
    has_run = true;
    return {rounds, left, (long long)h_pinned[3 * (COLOR_BATCH_MAX + 2)], waits};
  }
};

}  // namespace mgx
