// mgx/mst_fused.hpp -- minimum spanning forest, fused (mgx_mst_run): Boruvka rounds over per-vertex incident arrays sorted once,
// every phase a launch of its own on the context's stream, one host wait per run (the stats).
//
// The definition (the operator path include/gunrock/mst/ and tests/mst_model.py compute the same):
//   every CSR entry (v, u, w) is the undirected edge {v, u} of weight w; self-loops are ignored, parallel entries are parallel
//   edges, a vertex without entries is a tree of its own.  key(w): the IEEE bits b of w (-0.0 read as +0.0) mapped monotonically
//   to u32, b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000).  Edges are ordered by (key(w), min(v, u), max(v, u)); entries with the same
//   triple are the same edge, so the minimum spanning forest is unique.  A NaN weight (on an entry that is no self-loop) makes the
//   run MGX_E_INVALID.  label[v] = the smallest vertex id of v's component, as the connected components' (cc_fused.hpp).
//
// Setup, once per handle and `symmetric`, kept on the handle:
//   count / scan / fill   the incident array of v: 8-byte keys (key(w) << 32) | neighbour of v's out-entries and -- symmetric == 0
//                         -- its in-entries from the genuine CSC, self-loops dropped; NaNs are counted in the fill
//   sort                  every row ascending (segsort.hpp's kernels; the list sizes stay on the device, no host wait).  Ascending
//                         (key, u) within the row of v is ascending in the edge order, so the first entry of v that leaves v's
//                         component is v's lightest outgoing edge, and entries before it stay internal for good: a cursor per
//                         vertex only ever moves forward.
// A round (each step a launch; rt is the snapshot of the roots the last compress left, read-only all round):
//   work list   live vertices (cursor not at the end): rows with at least MST_LONG_MIN entries left are long, an item per MST_SEG
//               entries from the cursor on; the others short, compacted through a wave-private LDS stage (worklist.hpp)
//   scan        a short row a lane: walk from the cursor to the first entry with rt[nbr] != rt[v].  A long item a wave: 64 entries a
//               step, a __ballot finds the first that leaves; the windows of one row meet in an atomicMin on the row's position
//               word (a window behind a position already found gives up: an optimisation, never needed for the result)
//   weight      cursor <- the position found (or the end); atomicMin of its key(w) on the component's 32-bit word
//   pair        vertices whose best has that weight: atomicMin of (min << 32 | max) on the component's 64-bit word.  Now every
//               component holds its lightest outgoing edge under the edge order
//   hook        the vertex that holds its component r's edge, leading to component o, takes it -- marks its position in the bit
//               array -- unless o's edge is the same triple and o < r (the mutual pair: taken once, by the smaller root); it then
//               unions with cc_link
//   compress    comp[v] and rt[v] <- the root; one thread closes the round: nothing chosen -> the done word
// ceil(log2 n) + 1 rounds are enqueued; their kernels read the done word and return at once behind the last round that chose
// something.  Finish: the marked positions compacted in ascending position (scan.hpp's kernels on the bit array) to (a, b, w),
// the weights summed in double over fixed tiles, the shared label reduction (cc_label_stats), one read-back.  The list's order is
// a function of the graph alone: a component's lightest edge and who takes it do not depend on the races.
//
// Why a false `symmetric` word can give a wrong forest but never a hang or a fault (gfx950: per-XCD L2s are not coherent within a
// launch, a CU's L1 is never refreshed by other CUs' stores):
//   (a) comp is written by device-scope atomicCAS in the hook launch (cc_link, rules (a) - (c) of cc_fused.hpp) and by plain
//       stores in the compress launch, where nothing links; every decision of a round reads rt, cw, cp, cur and the position
//       words, which no launch both writes plainly and reads: cross-CU visibility comes from launch boundaries and atomics only;
//   (b) nothing spins on a load.  cc_link's loop strictly lowers the larger of its two roots; a cursor walk ends at the row's end;
//       a window is at most MST_SEG entries; the number of rounds is fixed by the host before the first launch;
//   (c) every index is bounded by the arrays' own sizes whatever the graph says: positions lie in [off[v], off[v + 1]), the
//       compaction writes at most n list entries (a guard: with a false word two components may take different edges towards
//       each other -- both are marked, the union happens once, the list is too long for a forest but not for its arrays).
// With a true word the components that still have an outgoing edge at least halve per round (each joins another such one), so
// the enqueued rounds suffice; with a false one the run ends after them wherever it stands.
// The cursor bound: stats[6] counts an entry a short row's lane looks at and a 64-entry step a wave takes.  A step either passes
// at least one entry for good (the cursor moves beyond it: at most stats[7] such steps in a run, the round that chooses nothing
// included -- there every step does), or it finds the row's leaving entry at its own first position: once a vertex and round that
// chose something.  So stats[6] <= stats[7] + stats[4] * n holds unconditionally while no row has more than MST_SEG entries left:
// every row is one item then.  A row beyond that has windows behind its first; what they look at behind the row's first leaving
// entry is passed by nobody and looked at again next round: at most (entries left in such rows) / 64 + their windows steps a
// round, and how many of them a window takes before it sees the position word is a race (stats[6] is not reproducible there).
// With such rows the bound is a condition on the input, not a theorem: it holds when these steps fit into what the two terms leave
// -- a wave passes 64 entries a step where stats[7] allows one each, and n counts every vertex where only live ones look.  DESIGN
// 3.12 and tests/test_gpu_mst.py name the inputs of the suite that have such rows.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cc_fused.hpp"
#include "env.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "segsort.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int MST_LONG_MIN_DEFAULT = 64;   // rows with at least this many entries left go to the wave path (unmeasured guess)
constexpr int MST_SEG_DEFAULT = 2048;      // entries of a long row's window (unmeasured guess; CC_SEG's value)
constexpr u32 MST_NONE = 0x7FFFFFFFu;      // no position
constexpr int MST_LIST_STAGE = 2 * WAVE;   // a wave's LDS stage of short-row items
constexpr int MST_SUM_TILE = 2048;         // list entries one workgroup sums

// stat words of a run, as read back
enum { MST_S_LARGEST = 0, MST_S_COMPONENTS, MST_S_STEPS, MST_S_LONG, MST_S_SHORT, MST_S_NAN, MST_S_ENTRIES, MST_S_EDGES,
       MST_S_TOTAL, MST_S_ROUNDS, MST_S_WORDS };
// control words of the rounds
enum { MST_W_SHORT = 0, MST_W_LONG, MST_W_CHOSEN, MST_W_DONE, MST_W_ROUNDS, MST_W_WORDS = 8 };

__host__ __device__ __forceinline__ u32 mst_key_of_bits(u32 b) {
  if (b == 0x80000000u) b = 0u;                                  // -0.0 is +0.0
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ u32 mst_bits_of_key(u32 k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
__device__ __forceinline__ u32 mst_key(float w) { return mst_key_of_bits(__float_as_uint(w)); }
__device__ __forceinline__ bool mst_is_nan(float w) { return (__float_as_uint(w) & 0x7FFFFFFFu) > 0x7F800000u; }
__device__ __forceinline__ u64 mst_pair(int v, int u) { return ((u64)(u32)min(v, u) << 32) | (u32)max(v, u); }

struct mst_opts_t {
  int long_min = MST_LONG_MIN_DEFAULT;
  int seg = MST_SEG_DEFAULT;
  // read per run: MGX_MST_LONG_MIN >= 1, MGX_MST_SEG rounded up to a multiple of 64
  static mst_opts_t from_env() {
    mst_opts_t o;
    if (const char* e = env("MGX_MST_LONG_MIN")) { const long long v = atoll(e); if (v >= 1) o.long_min = (int)std::min<long long>(v, 0x7FFFFFFF); }
    if (const char* e = env("MGX_MST_SEG")) { const long long v = atoll(e); if (v >= 1) o.seg = (int)std::min<long long>((v + WAVE - 1) / WAVE * WAVE, 1 << 30); }
    return o;
  }
};

// ---- setup: the incident arrays ---------------------------------------------------------------------------------------------
struct mst_inc_args_t {
  const int* ro;
  const int* ci;
  const float* w;
  const int* co;                 // the genuine CSC (symmetric == 0) or nullptr
  const int* ri;
  const float* rw;
  int n;
  int* cnt;                      // !FILL: incident entries of v
  const int* off;                // FILL: their exclusive scan
  u64* keys;
  u64* nanw;
};

// one row of v's (out- or in-) entries by a lane
template <bool FILL>
__device__ __forceinline__ void mst_inc_lane(const mst_inc_args_t& a, const int* nbr, const float* wt, int b, int e, int v, int& pos,
                                             u32& nans) {
  for (int q = b; q < e; ++q) {
    const int u = nbr[q];
    if (u == v) continue;
    if (FILL) {
      const float w = wt[q];
      nans += mst_is_nan(w) ? 1u : 0u;
      a.keys[pos] = ((u64)mst_key(w) << 32) | (u32)u;
    }
    ++pos;
  }
}
// ... by a wave
template <bool FILL>
__device__ __forceinline__ void mst_inc_wave(const mst_inc_args_t& a, const int* nbr, const float* wt, int b, int e, int v, int& pos,
                                             u32& nans) {
  const int lane = lane_id();
  for (int p = b; p < e; p += WAVE) {
    const int q = p + lane;
    const int u = q < e ? nbr[q] : v;
    const bool ok = u != v;
    const u64 m = __ballot(ok);
    if (FILL && ok) {
      const float w = wt[q];
      nans += mst_is_nan(w) ? 1u : 0u;
      a.keys[pos + rank_in_mask(m)] = ((u64)mst_key(w) << 32) | (u32)u;
    }
    pos += __popcll(m);
  }
}

// FILL = false: cnt[v] = v's incident entries that are no self-loops; FILL = true: their keys from off[v] on, the NaNs counted.
// 64 vertices a wave: rows of fewer than 64 entries a lane each, the others by the whole wave one after the other.
template <bool FILL>
__global__ __launch_bounds__(BLOCK) void k_mst_incident(mst_inc_args_t a) {
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (BLOCK / WAVE));
  u32 nans = 0;
  for (long long base = (long long)wave * WAVE; base < a.n; base += (long long)waves * WAVE) {
    const int v = (int)base + lane;
    const bool in = v < a.n;
    const int ob = in ? a.ro[v] : 0, oe = in ? a.ro[v + 1] : 0;
    const int ib = in && a.co ? a.co[v] : 0, ie = in && a.co ? a.co[v + 1] : 0;
    const bool big = (oe - ob) + (ie - ib) >= WAVE;
    if (in && !big) {
      int pos = FILL ? a.off[v] : 0;
      mst_inc_lane<FILL>(a, a.ci, a.w, ob, oe, v, pos, nans);
      mst_inc_lane<FILL>(a, a.ri, a.rw, ib, ie, v, pos, nans);
      if (!FILL) a.cnt[v] = pos;
    }
    u64 bm = __ballot(big);
    while (bm) {
      const int l = __ffsll((long long)bm) - 1;
      bm &= bm - 1;
      const int vv = __shfl(v, l, WAVE);
      const int b0 = __shfl(ob, l, WAVE), e0 = __shfl(oe, l, WAVE), b1 = __shfl(ib, l, WAVE), e1 = __shfl(ie, l, WAVE);
      int pos = FILL ? a.off[vv] : 0;
      mst_inc_wave<FILL>(a, a.ci, a.w, b0, e0, vv, pos, nans);
      mst_inc_wave<FILL>(a, a.ri, a.rw, b1, e1, vv, pos, nans);
      if (!FILL && lane == 0) a.cnt[vv] = pos;
    }
  }
  if (FILL) {
    nans = wave_sum(nans);
    if (lane == 0 && nans) atomicAdd(a.nanw, (u64)nans);
  }
}

// the rows of the incident array into the segmented sort's lists by length (segment v = row v; as k_segsort_classify, the sizes
// stay on the device)
__global__ __launch_bounds__(BLOCK) void k_mst_sort_classify(segsort_args_t<u64, segsort_no_value_t> s, const int* off, int n) {
  for (long long base = (long long)blockIdx.x * BLOCK; base < n; base += (long long)gridDim.x * BLOCK) {
    const int v = (int)base + (int)threadIdx.x;
    const int len = v < n ? off[v + 1] - off[v] : 0;
    segsort_classify_one(s, v, len);
  }
}

// ---- the rounds -------------------------------------------------------------------------------------------------------------
struct mst_round_args_t {
  const int* off;
  const u64* keys;
  int* cur;                      // the cursors: positions in keys
  int* rt;                       // the roots as the last compress left them
  int* comp;
  u32* lbpos;                    // position of v's lightest outgoing entry this round (MST_NONE: none)
  u32* cw;                       // per root: key(w) of the component's lightest outgoing edge
  u64* cp;                       // per root: its (min << 32 | max)
  int n;
  int long_min;
  int seg;
  int* s_list;
  int2* l_list;
  int* words;                    // MST_W_*
  u64* stat;                     // MST_S_*
  u64* bits;                     // the marked positions, a bit each
};

__global__ __launch_bounds__(BLOCK) void k_mst_init(int* comp, int* rt, int* cur, const int* off, int n) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    comp[i] = (int)i;
    rt[i] = (int)i;
    cur[i] = off[i];
  }
}

__global__ __launch_bounds__(BLOCK) void k_mst_worklist(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (BLOCK / WAVE));
  __shared__ int s_stage[WAVES_PER_BLOCK][MST_LIST_STAGE];
  int* const stage = s_stage[threadIdx.x / WAVE];
  int fill = 0;
  for (long long base = (long long)wave * WAVE; base < a.n; base += (long long)waves * WAVE) {
    const int v = (int)base + lane;
    const bool in = v < a.n;
    const int rem = in ? a.off[v + 1] - a.cur[v] : 0;
    if (in) {
      a.lbpos[v] = MST_NONE;
      a.cw[v] = 0xFFFFFFFFu;
      a.cp[v] = ~0ull;
    }
    // short rows through the wave's LDS stage, long rows' windows behind one add per wave and pass (worklist.hpp)
    wave_stage_push<MST_LIST_STAGE>(rem > 0 && rem < a.long_min, v, stage, fill, a.s_list, a.words + MST_W_SHORT);
    wave_append_segments(rem >= a.long_min && rem > 0, v, rem, a.seg, a.l_list, a.words + MST_W_LONG);
  }
  wave_stage_flush(stage, fill, a.s_list, a.words + MST_W_SHORT);
}

// long items a wave each, then short rows a lane each; the grid is sized to the chip, the counts come from the device
__global__ __launch_bounds__(BLOCK) void k_mst_scan(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  const int ns = a.words[MST_W_SHORT], nl = a.words[MST_W_LONG];
  const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const long long gthreads = (long long)gridDim.x * BLOCK;
  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE), waves = (int)(gthreads / WAVE);
  u32 steps = 0;
  for (int it = wave; it < nl; it += waves) {
    const int2 item = a.l_list[it];
    const int v = item.x;
    const int end = a.off[v + 1], lv = a.rt[v];
    const int b = a.cur[v] + item.y * a.seg;
    const int e1 = min(end, b + a.seg);
    for (int p = b; p < e1; p += WAVE) {
      if (item.y > 0) {                                      // an earlier window has found the row's entry already
        u32 seen = 0;
        if (lane == 0) seen = __hip_atomic_load(a.lbpos + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__shfl(seen, 0, WAVE) < (u32)p) break;
      }
      const int q = p + lane;
      const bool leaves = q < e1 && a.rt[(int)(u32)a.keys[q]] != lv;
      const u64 m = __ballot(leaves);
      if (lane == 0) ++steps;
      if (m) {
        if (lane == 0) atomicMin(a.lbpos + v, (u32)(p + __ffsll((long long)m) - 1));
        break;
      }
    }
  }
  for (long long i = gtid; i < ns; i += gthreads) {
    const int v = a.s_list[i];
    const int end = a.off[v + 1], lv = a.rt[v];
    int p = a.cur[v];
    while (p < end && a.rt[(int)(u32)a.keys[p]] == lv) { ++p; ++steps; }
    if (p < end) {
      ++steps;
      a.lbpos[v] = (u32)p;
    }
  }
  steps = wave_sum(steps);
  if (lane == 0 && steps) atomicAdd(a.stat + MST_S_STEPS, (u64)steps);
  if (gtid == 0) {
    if (nl) atomicAdd(a.stat + MST_S_LONG, (u64)nl);
    if (ns) atomicAdd(a.stat + MST_S_SHORT, (u64)ns);
  }
}

// the cursor moves to the position found (or to the end); the component's lightest weight
__global__ __launch_bounds__(BLOCK) void k_mst_weight(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const int end = a.off[v + 1];
    if (a.cur[v] >= end) continue;
    const u32 lp = a.lbpos[v];
    if (lp == MST_NONE) {
      a.cur[v] = end;
    } else {
      a.cur[v] = (int)lp;
      atomicMin(a.cw + a.rt[v], (u32)(a.keys[lp] >> 32));
    }
  }
}

// among the entries of that weight, the component's smallest pair
__global__ __launch_bounds__(BLOCK) void k_mst_pair(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const u32 lp = a.lbpos[v];
    if (lp == MST_NONE) continue;
    const u64 k = a.keys[lp];
    const int r = a.rt[v];
    if ((u32)(k >> 32) == a.cw[r]) atomicMin(a.cp + r, mst_pair(v, (int)(u32)k));
  }
}

// the holder of its component's edge marks it (unless the other side holds the same edge and has the smaller root) and unions
__global__ __launch_bounds__(BLOCK) void k_mst_hook(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  const int lane = lane_id();
  for (long long base = (long long)blockIdx.x * BLOCK + (threadIdx.x - lane); base < a.n; base += (long long)gridDim.x * BLOCK) {
    const int v = (int)base + lane;
    bool take = false;
    if (v < a.n) {
      const u32 lp = a.lbpos[v];
      if (lp != MST_NONE) {
        const u64 k = a.keys[lp];
        const int u = (int)(u32)k;
        const int r = a.rt[v];
        const u32 wk = (u32)(k >> 32);
        const u64 pk = mst_pair(v, u);
        if (wk == a.cw[r] && pk == a.cp[r]) {
          const int o = a.rt[u];
          const bool other_takes = o < r && a.cw[o] == wk && a.cp[o] == pk;
          if (!other_takes) {
            take = true;
            atomicOr(a.bits + (lp >> 6), 1ull << (lp & 63u));
            cc_link(a.comp, v, u);
          }
        }
      }
    }
    const u64 m = __ballot(take);
    if (m && lane == __ffsll((long long)m) - 1) atomicAdd(a.words + MST_W_CHOSEN, __popcll(m));
  }
}

// every comp[v] and rt[v] becomes its root (no link runs meanwhile); one thread closes the round
__global__ __launch_bounds__(BLOCK) void k_mst_compress(mst_round_args_t a) {
  if (a.words[MST_W_DONE]) return;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
    const int v = (int)i;
    const int p = a.comp[v];
    int x = p, y;
    while ((y = a.comp[x]) != x) x = y;
    if (x != p) a.comp[v] = x;
    a.rt[v] = x;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // (a workgroup that starts late and sees the done word skips a compress that has nothing to do: nothing was chosen)
    if (a.words[MST_W_CHOSEN] == 0) a.words[MST_W_DONE] = 1;
    else a.words[MST_W_ROUNDS] += 1;
    a.words[MST_W_SHORT] = 0;
    a.words[MST_W_LONG] = 0;
    a.words[MST_W_CHOSEN] = 0;
  }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
// tile_sum[t] = the weights of list entries [t * MST_SUM_TILE, ..) in double, summed in an order fixed by the count alone
__device__ __forceinline__ double mst_block_sum(double x, double* sm) {
  x = wave_sum(x);
  if (lane_id() == 0) sm[threadIdx.x / WAVE] = x;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += sm[w];
  __syncthreads();
  return t;
}
__global__ __launch_bounds__(BLOCK) void k_mst_sum_tiles(const float* w, const long long* count, long long cap, double* tile_sum) {
  __shared__ double sm[WAVES_PER_BLOCK];
  const long long cnt = min(*count, cap);
  const long long base = (long long)blockIdx.x * MST_SUM_TILE;
  double x = 0.0;
  for (int k = 0; k < MST_SUM_TILE / BLOCK; ++k) {
    const long long i = base + (long long)k * BLOCK + threadIdx.x;
    if (i < cnt) x += (double)w[i];
  }
  const double t = mst_block_sum(x, sm);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = t;
}
// one workgroup: the tiles' sums, and the run's words gathered for the read-back
__global__ __launch_bounds__(BLOCK) void k_mst_finish(const double* tile_sum, const long long* count, long long cap, const int* words,
                                                      const u64* nanw, const int* off, int n, u64* stat) {
  __shared__ double sm[WAVES_PER_BLOCK];
  const long long cnt = min(*count, cap);
  const long long tiles = (cnt + MST_SUM_TILE - 1) / MST_SUM_TILE;
  double x = 0.0;
  for (long long t = threadIdx.x; t < tiles; t += BLOCK) x += tile_sum[t];
  const double total = mst_block_sum(x, sm);
  if (threadIdx.x == 0) {
    stat[MST_S_EDGES] = (u64)cnt;
    stat[MST_S_TOTAL] = (u64)__double_as_longlong(total);
    stat[MST_S_ROUNDS] = words ? (u64)words[MST_W_ROUNDS] : 0ull;
    stat[MST_S_NAN] = nanw ? *nanw : 0ull;
    stat[MST_S_ENTRIES] = off ? (u64)off[n] : 0ull;
  }
}

// Both paths' list total: sums w[0, *count) (at most cap) into stat[MST_S_EDGES] / stat[MST_S_TOTAL]; tile_sum holds cap /
// MST_SUM_TILE + 1 doubles.
inline void mst_sum_list(const float* w, const long long* count, long long cap, double* tile_sum, const int* words, const u64* nanw,
                         const int* off, int n, u64* stat, hipStream_t st) {
  const int tiles = (int)((cap + MST_SUM_TILE - 1) / MST_SUM_TILE);
  if (tiles > 0) hipLaunchKernelGGL(k_mst_sum_tiles, dim3(tiles), dim3(BLOCK), 0, st, w, count, cap, tile_sum);
  hipLaunchKernelGGL(k_mst_finish, dim3(1), dim3(BLOCK), 0, st, (const double*)tile_sum, count, cap, words, nanw, off, n, stat);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct mst_setup_t {
  bool built = false;
  long long cap = 0;             // entries the incident array has room for: m, or 2 m with the in-entries
  mem_t<int> off;                // n + 1
  mem_t<u64> keys;
  mem_t<u64> bits;               // a bit per position
  mem_t<u64> nanw;
  long long entries = 0;         // off[n] as the host last read it
  int passes = 0;                // merge passes of the sort
};

// what a setup needs until its launches have run (freed behind the run's host wait)
struct mst_setup_tmp_t {
  mem_t<int> cnt, short_list, mid_list, sort_cnt;
  mem_t<int2> tile_list;
  mem_t<u64> keys_tmp;
};

struct mst_fused_state_t {
  int n = 0;
  long long m = 0;
  mst_setup_t setup[2];          // [symmetric]
  mem_t<int> comp, rt, cur, sizes, s_list, words, hot;
  mem_t<int2> l_list;
  mem_t<u32> lbpos, cw;
  mem_t<u64> cp, stat;
  mem_t<int> out_a, out_b;       // the list: n entries of room
  mem_t<float> out_w;
  mem_t<double> tile_sum;
  pinned_t<u64> h_pinned;
  mst_opts_t opts;               // of the last run
  long long h[MST_S_WORDS] = {0};
  int last = -1;                 // the setup of the last run (-1: none, or it failed)
  long long waits = 0;           // host waits of the run in progress: counted where the host waits, not stated
  bool reused = false;

  mst_fused_state_t(int n_, long long m_, standard_context_t& ctx) : n(n_), m(m_) {
    // (the sort's merge passes keep run widths w with 2 w an int; positions are ints)
    if (m > (1LL << 29)) throw mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx mst: more than 2^29 CSR entries");
    const size_t N = (size_t)std::max(n, 1);
    comp = mem_t<int>(N, ctx); rt = mem_t<int>(N, ctx); cur = mem_t<int>(N, ctx); sizes = mem_t<int>(N, ctx);
    s_list = mem_t<int>(N, ctx);
    // long items: at most min(n, cap / long_min) rows, plus one per seg entries beyond their first window; cap <= 2 m, long_min
    // >= 1, seg >= 64.  Sized once for any switches, so that no run has to free a list (a hipFree waits for the device).
    l_list = mem_t<int2>((size_t)((long long)N + 2 * m / WAVE + 2), ctx);
    words = mem_t<int>(MST_W_WORDS, ctx);
    hot = mem_t<int>(1, ctx);
    lbpos = mem_t<u32>(N, ctx); cw = mem_t<u32>(N, ctx);
    cp = mem_t<u64>(N, ctx);
    stat = mem_t<u64>(MST_S_WORDS, ctx);
    out_a = mem_t<int>(N, ctx); out_b = mem_t<int>(N, ctx);
    out_w = mem_t<float>(N, ctx);
    tile_sum = mem_t<double>(N / MST_SUM_TILE + 2, ctx);
    h_pinned = pinned_t<u64>(MST_S_WORDS);
    ctx.reserve_scratch(scan_scratch_bytes(std::max<long long>((long long)n + 1, 2 * m)));
  }

  // enqueue the build of setup[symmetric]; `t` must outlive the launches
  void build(mst_setup_t& s, mst_setup_tmp_t& t, const int* ro, const int* ci, const float* w, const int* co, const int* ri,
             const float* rw, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const size_t N = (size_t)std::max(n, 1);
    s.cap = co ? 2 * m : m;
    const size_t M = (size_t)std::max<long long>(s.cap, 1);
    s.off = mem_t<int>(N + 1, ctx);
    s.keys = mem_t<u64>(M, ctx);
    s.bits = mem_t<u64>(M / 64 + 2, ctx);
    s.nanw = mem_t<u64>(1, ctx);
    t.cnt = mem_t<int>(N + 1, ctx);
    MGX_HIP(hipMemsetAsync(s.nanw.data(), 0, sizeof(u64), st));
    MGX_HIP(hipMemsetAsync(t.cnt.data(), 0, (N + 1) * sizeof(int), st));
    mst_inc_args_t a;
    a.ro = ro; a.ci = ci; a.w = w; a.co = co; a.ri = ri; a.rw = rw; a.n = n; a.cnt = t.cnt.data(); a.off = s.off.data();
    a.keys = s.keys.data(); a.nanw = s.nanw.data();
    const int grid = grid_for(n, WAVE, max_blocks);          // (a lane a vertex, 64 vertices a wave: BLOCK / WAVE chunks a workgroup)
    hipLaunchKernelGGL(k_mst_incident<false>, dim3(grid), dim3(BLOCK), 0, st, a);
    const int nn = n;
    const int* cnt = t.cnt.data();
    transform_scan([=] __device__(long long i) { return i < nn ? cnt[i] : 0; }, (long long)n + 1, s.off.data(), ctx, nullptr);
    hipLaunchKernelGGL(k_mst_incident<true>, dim3(grid), dim3(BLOCK), 0, st, a);
    s.passes = 0;
    if (s.cap >= 2) {
      t.short_list = mem_t<int>(N, ctx);
      t.mid_list = mem_t<int>(N, ctx);
      t.sort_cnt = mem_t<int>(4, ctx);
      t.tile_list = mem_t<int2>((size_t)(2 * (s.cap / SEGSORT_TILE) + 2), ctx);
      MGX_HIP(hipMemsetAsync(t.sort_cnt.data(), 0, 4 * sizeof(int), st));
      segsort_args_t<u64, segsort_no_value_t> g;
      g.keys = s.keys.data(); g.vals = nullptr; g.keys_tmp = nullptr; g.vals_tmp = nullptr;
      g.count = 0; g.heads = s.off.data() + 1; g.num_segments = n;           // (segment v < n = row v; count is unused)
      g.short_list = t.short_list.data(); g.mid_list = t.mid_list.data(); g.tile_list = t.tile_list.data(); g.cnt = t.sort_cnt.data();
      auto up = [] __device__(u64 x, u64 y) { return x < y; };
      typedef decltype(up) C;
      typedef segsort_no_value_t V;
      hipLaunchKernelGGL(k_mst_sort_classify, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, g, (const int*)s.off.data(), n);
      hipLaunchKernelGGL((k_segsort_wave<u64, V, C>), dim3(max_blocks), dim3(BLOCK), 0, st, g, up);
      hipLaunchKernelGGL((k_segsort_block<u64, V, C, false>), dim3(max_blocks), dim3(BLOCK), 0, st, g, up);
      if (s.cap > SEGSORT_TILE) {
        t.keys_tmp = mem_t<u64>(M, ctx);
        g.keys_tmp = t.keys_tmp.data();
        hipLaunchKernelGGL((k_segsort_block<u64, V, C, true>), dim3(max_blocks), dim3(BLOCK), 0, st, g, up);
        u64* src = g.keys;
        u64* dst = g.keys_tmp;
        for (long long wd = SEGSORT_TILE; wd < s.cap; wd *= 2) {
          hipLaunchKernelGGL((k_segsort_merge<u64, V, C>), dim3(max_blocks), dim3(BLOCK), 0, st, g, (const u64*)src, (const V*)nullptr,
                             dst, (V*)nullptr, (int)wd, up);
          std::swap(src, dst);
          ++s.passes;
        }
        if (s.passes & 1) hipLaunchKernelGGL((k_segsort_copy_back<u64, V>), dim3(max_blocks), dim3(BLOCK), 0, st, g);
      }
    }
    MGX_CHECK_LAUNCH("mgx mst setup");
  }

  // The fused run (ro, ci, w: the CSR on the device; co, ri, rw: its genuine CSC -- required when !symmetric).  Returns the eight
  // stats of mgx_mst_run.  Throws MGX_E_INVALID for a NaN weight (no result is kept then).
  std::vector<long long> run(const int* ro, const int* ci, const float* w, const int* co, const int* ri, const float* rw,
                             bool symmetric, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    last = -1;
    opts = mst_opts_t::from_env();
    for (long long& x : h) x = 0;
    if (!symmetric && !co) throw mgx_error(MGX_E_INVALID, "mgx_mst_run: symmetric == 0 needs the graph's genuine CSC (mgx_graph_build_csc)");
    if (n <= 0) { last = symmetric ? 1 : 0; reused = false; return {0, 0, 0, 0, 0, 0, 0, 0}; }
    mst_setup_t& s = setup[symmetric ? 1 : 0];
    mst_setup_tmp_t tmp;
    reused = s.built;
    waits = 0;
    if (!s.built) {
      s = mst_setup_t();
      if (symmetric) build(s, tmp, ro, ci, w, nullptr, nullptr, nullptr, ctx);
      else build(s, tmp, ro, ci, w, co, ri, rw, ctx);
    }
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const int grid_n = grid_for(n, BLOCK, max_blocks);
    MGX_HIP(hipMemsetAsync(words.data(), 0, MST_W_WORDS * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(stat.data(), 0, MST_S_WORDS * sizeof(u64), st));
    MGX_HIP(hipMemsetAsync(s.bits.data(), 0, s.bits.size() * sizeof(u64), st));
    hipLaunchKernelGGL(k_mst_init, dim3(grid_n), dim3(BLOCK), 0, st, comp.data(), rt.data(), cur.data(), (const int*)s.off.data(), n);
    mst_round_args_t a;
    a.off = s.off.data(); a.keys = s.keys.data(); a.cur = cur.data(); a.rt = rt.data(); a.comp = comp.data(); a.lbpos = lbpos.data();
    a.cw = cw.data(); a.cp = cp.data(); a.n = n; a.long_min = opts.long_min; a.seg = opts.seg; a.s_list = s_list.data();
    a.l_list = l_list.data(); a.words = words.data(); a.stat = stat.data(); a.bits = s.bits.data();
    int rounds = 1;
    while ((1LL << (rounds - 1)) < n) ++rounds;              // ceil(log2 n) + 1
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(k_mst_worklist, dim3(grid_for(n, WAVE, max_blocks)), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_mst_scan, dim3(max_blocks), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_mst_weight, dim3(grid_n), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_mst_pair, dim3(grid_n), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_mst_hook, dim3(grid_n), dim3(BLOCK), 0, st, a);
      hipLaunchKernelGGL(k_mst_compress, dim3(grid_n), dim3(BLOCK), 0, st, a);
    }
    MGX_CHECK_LAUNCH("mgx mst rounds");
    // the marked positions in ascending position -> (a, b, w): scan.hpp's compaction kernels on the bit array, no host wait
    long long* const partials = (long long*)ctx.scratch;
    const long long* d_count = nullptr;
    if (s.cap > 0) {
      const long long ntiles = scan_num_tiles(s.cap);
      if ((size_t)ntiles > ctx.lookback_tiles || (size_t)(ntiles + 2) * sizeof(long long) > ctx.scratch_bytes)
        throw mgx_error(MGX_E_INVALID, "mgx mst: scratch arena too small");
      ++ctx.scratch_epoch;
      const bool single = ntiles <= SCAN_LOOKBACK_MAX_TILES;
      const unsigned epoch = single ? ctx.next_lookback_epoch() : 0u;
      typedef compact_t::no_pred_t P;
      hipLaunchKernelGGL((k_compact_upsweep<P, true>), dim3((unsigned)ntiles), dim3(BLOCK), 0, st, P(), s.cap, s.bits.data(), partials,
                         single ? ctx.lookback_status.data() : (unsigned long long*)nullptr, ctx.lookback_ticket.data(), ctx.lookback_ticket_base,
                         epoch, (long long*)nullptr, 0LL);
      if (single) ctx.lookback_ticket_base += (unsigned)ntiles;
      else hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(BLOCK), 0, st, partials, ntiles, (long long*)nullptr, 0LL);
      const int* off = s.off.data();
      const u64* keys = s.keys.data();
      int* oa = out_a.data();
      int* ob = out_b.data();
      float* ow = out_w.data();
      const int nn = n;
      auto emit = [=] __device__(long long to, long long from) {
        if (to >= nn) return;                                // (a false `symmetric` word: see the header)
        int lo = 0, hi = nn;                                 // the row of position `from`: the last v with off[v] <= from
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (off[mid] <= from) lo = mid; else hi = mid - 1;
        }
        const u64 k = keys[from];
        const int u = (int)(u32)k;
        oa[to] = min(lo, u);
        ob[to] = max(lo, u);
        ow[to] = __uint_as_float(mst_bits_of_key((u32)(k >> 32)));
      };
      hipLaunchKernelGGL(k_compact_downsweep<decltype(emit)>, dim3((unsigned)ntiles), dim3(BLOCK), 0, st, emit, s.cap,
                         (const u64*)s.bits.data(), (const long long*)partials);
      d_count = partials + ntiles;
    } else {
      MGX_HIP(hipMemsetAsync(partials, 0, sizeof(long long), st));
      d_count = partials;
    }
    hipLaunchKernelGGL(k_cc_sample, dim3(1), dim3(BLOCK), 0, st, (const int*)comp.data(), n, CC_SEED_DEFAULT, hot.data());
    cc_label_stats(comp.data(), n, hot.data(), sizes.data(), stat.data(), max_blocks, st);
    mst_sum_list(out_w.data(), d_count, (long long)n, tile_sum.data(), words.data(), s.nanw.data(), s.off.data(), n, stat.data(), st);
    MGX_CHECK_LAUNCH("mgx mst finish");
    h_pinned.fetch(stat.data(), MST_S_WORDS, st);
    ++waits;
    for (int i = 0; i < MST_S_WORDS; ++i) h[i] = (long long)h_pinned[i];
    if (h[MST_S_NAN]) {
      s = mst_setup_t();                                     // (nothing of it is worth keeping)
      throw mgx_error(MGX_E_INVALID, "mgx_mst_run: a NaN edge weight");
    }
    s.built = true;
    s.entries = h[MST_S_ENTRIES];
    last = symmetric ? 1 : 0;
    long long cs[3];
    cc_unpack_stats(h_pinned.data(), cs);
    return {h[MST_S_EDGES], cs[0], cs[1], cs[2], h[MST_S_ROUNDS], waits, h[MST_S_STEPS], h[MST_S_ENTRIES]};
  }

  double total() const {
    double d;
    const long long b = h[MST_S_TOTAL];
    std::memcpy(&d, &b, sizeof(d));
    return d;
  }

  // {long items, short items, MST_LONG_MIN, MST_SEG, merge passes of the setup sort, setup reused}
  std::vector<long long> info() const {
    if (last < 0) throw mgx_error(MGX_E_INVALID, "mgx_mst_info: no fused run yet");
    return {h[MST_S_LONG], h[MST_S_SHORT], opts.long_min, opts.seg, setup[last].passes, reused ? 1 : 0, 0, 0};
  }
};

}  // namespace mgx
