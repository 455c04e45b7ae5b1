// mgx/tc_fused.hpp -- triangle counting (mgx_tc_run, mgx_tc_enact): the oriented graph both paths count on, and the fused count.
//
// The definition (the operator path include/gunrock/tc/ and tests/tc_model.py compute the same):
//   triangles of the underlying simple undirected graph: a CSR entry (v, u), v != u, is the pair {v, u}; self-loops and duplicate
//   entries change nothing; original ids.  tri[v] = triangles that contain v (64 bits), total = sum tri / 3, sdeg[v] = distinct
//   neighbours of v other than v.
//   symmetric != 0 (every entry has its reverse): rank(v) = (row length, v); the entries with rank(v) < rank(u) are kept.
//   symmetric == 0 (any graph): deg(v) = row length + entries that name v; every entry goes to the row of its lower-ranked end.
//   Either way the oriented graph (DAG) is dag_ro[n + 1], dag_ci[m_dag]: row a = the distinct neighbours of a of higher rank,
//   ascending by id.  A triangle of ranks a < b < c is counted once, at entry (a, b), as a common element of rows a and b.
//
// The build (device only; the host enqueues the same launches whatever the data are and looks at nothing before the stats):
//   row info     symmetric: one flag, whether every CSR row is ascending; else the degree histogram
//   select       kept entries per row -> scan (scan.hpp) -> fill.  Ascending rows of a symmetric graph: the fill drops adjacent
//                duplicates itself and writes the DAG ("direct": the launches behind it find nothing to do)
//   sort         else the oriented rows are sorted by the segmented sort's kernels (segsort.hpp), classified here on the device:
//                chip-sized grids read the list sizes from device words, the merge passes run for the longest row the entry
//                count admits (a pass over a row that is sorted already copies it)
//   dedup        count -> scan -> fill once more, dropping adjacent duplicates
//   dag stats    sdeg[v] = d+(v) + DAG entries that name v; m_dag, the longest row, the wedges
//   work list    vertices with d+ >= 2 by d+ into three lists, compacted through wave-private LDS stages (worklist.hpp)
// Sizes: the arrays hold m entries (m_dag <= m < 2^31 by construction; a CSR of more than 2^30 entries is refused at the first
// run), every scan's total is checked on the device against them before anything is written behind it; a failed check and a
// failed allocation are statuses (MGX_E_FRONTIER_OVERFLOW, MGX_E_HIP).
// The DAG, its statistics and its work lists stay on the handle per `symmetric` value: a repeat run only counts.
//
// The count (three launches over chip-sized grids, the list sizes read on the device, one host wait for the stats):
//   k_tc_short   rows of at most short_max entries: a wave takes 64 rows, spreads their entries (a, b) over its lanes; a lane
//                searches the shorter of rows a, b in the longer, from where the last probe ended
//   k_tc_wave    rows of at most wave_max entries, a wave each; k_tc_block the longer ones, a workgroup each: row a goes to LDS
//                once, groups of TC_GROUP lanes stream the rows b of its entries (consecutive lanes, consecutive entries), every
//                lane searches its entry in the LDS copy; hits are counted by __ballot + popcount.  A row longer than the stage
//                is staged chunk by chunk, every row b streamed again per chunk.
// Atomics (the rules of DESIGN 3.8 apply: nothing is read back inside a launch, integer adds commute, so two runs are bit-equal):
//   tri[a]: one 64-bit add per row (k_tc_short: from the wave's LDS counters); tri[b]: one per entry and chunk;
//   tri[w]: the staged kernels count the hits on w in an LDS counter beside w's slot of the stage and add them once per chunk,
//   k_tc_short adds one per hit; the total: one add per workgroup.
// The intersection bodies and the three count kernels take a template parameter EDGES (false: all of the above, unchanged).  true
// is the k-truss's support of every entry (mgx/ktruss_fused.hpp): the same triangles, the adds sent to their three ENTRIES.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "env.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "segsort.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int TC_SHORT_MAX_DEFAULT = 16;     // rows of at most this many oriented entries: k_tc_short
constexpr int TC_WAVE_MAX_DEFAULT = 256;     // ... : k_tc_wave; longer: k_tc_block
constexpr int TC_LIST_STAGE = 2 * WAVE;      // a wave's LDS stage of work-list items, per list
constexpr int TC_WAVE_STAGE = 512;           // entries of a wave's LDS stage
constexpr int TC_BLOCK_STAGE = 4096;         // entries of a workgroup's
constexpr int TC_GROUP = 16;                 // lanes that stream one row b

// stat words of a DAG (64 bits each): what the one read-back carries
enum { TC_S_TOTAL = 0, TC_S_MDAG = 1, TC_S_MAXROW = 2, TC_S_WEDGES = 3, TC_S_DIRECT = 4, TC_S_ERR = 5, TC_S_WORDS = 8 };

struct tc_opts_t {
  int short_max = TC_SHORT_MAX_DEFAULT, wave_max = TC_WAVE_MAX_DEFAULT, stage = TC_BLOCK_STAGE;
  static tc_opts_t from_env() {
    tc_opts_t o;
    o.short_max = env_int("MGX_TC_SHORT_MAX", 0, INT_MAX, o.short_max);
    o.wave_max = env_int("MGX_TC_WAVE_MAX", 0, INT_MAX, o.wave_max);
    o.stage = env_int("MGX_TC_STAGE", 1, TC_BLOCK_STAGE, o.stage);
    return o;
  }
};

__device__ __forceinline__ void tc_add(u64* p, u64 x) { atomicAdd(p, x); }

// rank(v) < rank(u): (degree, id); deg == nullptr: the row length is the degree (symmetric)
__device__ __forceinline__ bool tc_rank_less(const int* ro, const int* deg, int v, int u) {
  const int dv = deg ? deg[v] : ro[v + 1] - ro[v];
  const int du = deg ? deg[u] : ro[u + 1] - ro[u];
  return dv < du || (dv == du && v < u);
}

struct tc_build_args_t {
  const int* ro;          // the CSR
  const int* ci;
  int n;
  int symmetric;
  int* deg;               // symmetric == 0: row length + entries that name v
  int* cnt;               // n + 1 counts (the scans' input)
  int* cur;               // symmetric == 0: the fill's cursors
  int* tmp_ro;            // the oriented rows before the dedup
  int* tmp_ci;
  int* dag_ro;
  int* dag_ci;
  int* sdeg;
  u64* stat;
  long long cap;          // entries tmp_ci and dag_ci hold
};

// Rows over groups of G lanes (G = 64: a wave each), wave-uniform trip counts: every lane of a wave runs the same number of row
// steps, so the bodies may use __ballot and shuffles.  v = the group's row (valid: v < n).
#define TC_ROW_LOOP(G, n_rows)                                                                                  \
  const int lane = lane_id(), sub = lane % (G);                                                                 \
  const int gshift = lane - sub;                                                                                \
  const u64 gmask = (G) == 64 ? ~0ull : ((1ull << ((G) & 63)) - 1ull);                                          \
  const long long wave0 = (((long long)blockIdx.x * BLOCK + threadIdx.x) / WAVE) * (WAVE / (G));                \
  const long long wstep = (long long)gridDim.x * (BLOCK / WAVE) * (WAVE / (G));                                 \
  for (long long vb = wave0; vb < (n_rows); vb += wstep)

__global__ __launch_bounds__(BLOCK) void k_tc_init(u64* stat, int symmetric) {
  if (threadIdx.x < TC_S_WORDS) stat[threadIdx.x] = threadIdx.x == TC_S_DIRECT ? (u64)(symmetric != 0) : 0ull;
}

// symmetric: is every row ascending (stat[TC_S_DIRECT] stays 1)?  else: deg[v] = row length + entries that name v (deg cleared)
template <int G>
__global__ __launch_bounds__(BLOCK) void k_tc_rowinfo(tc_build_args_t a) {
  TC_ROW_LOOP(G, a.n) {
    const long long v = vb + gshift / G;
    if (v >= a.n) continue;
    const int beg = a.ro[v], end = a.ro[v + 1];
    bool bad = false;
    for (int e = beg + sub; e < end; e += G) {
      const int u = a.ci[e];
      if (a.symmetric) bad |= e > beg && a.ci[e - 1] > u;
      else atomicAdd(a.deg + u, 1);
    }
    if (bad) atomicExch(a.stat + TC_S_DIRECT, 0ull);
    if (!a.symmetric && sub == 0 && end > beg) atomicAdd(a.deg + (int)v, end - beg);
  }
  (void)gmask;
}

// MODE 0: the kept entries of the CSR's rows (symmetric): u != v, rank(v) < rank(u), and in direct mode not equal to the entry
//         before it; counted (FILL = false: cnt[v]) or written in order behind tmp_ro[v] (direct mode: into the DAG).
// MODE 1: the oriented rows without adjacent duplicates: counted, or written behind dag_ro[v]; direct mode: the counts are the
//         row lengths again and nothing is written (the DAG is there).
template <int G, int MODE, bool FILL>
__global__ __launch_bounds__(BLOCK) void k_tc_select(tc_build_args_t a) {
  const bool direct = a.stat[TC_S_DIRECT] != 0;
  if (a.stat[TC_S_ERR]) return;
  if (MODE == 1 && FILL && direct) return;
  const int* const sro = MODE == 0 ? a.ro : a.tmp_ro;
  const int* const sci = MODE == 0 ? a.ci : a.tmp_ci;
  const int* const dro = MODE == 0 ? a.tmp_ro : a.dag_ro;
  int* const dci = MODE == 0 ? (direct ? a.dag_ci : a.tmp_ci) : a.dag_ci;
  TC_ROW_LOOP(G, a.n) {
    const long long v = vb + gshift / G;
    const bool valid = v < a.n;
    const int beg = valid ? sro[v] : 0, end = valid ? sro[v + 1] : 0;
    if (MODE == 1 && direct) {
      if (valid && sub == 0) a.cnt[v] = end - beg;
      continue;
    }
    int at = valid && FILL ? dro[v] : 0, mine = 0;
    for (int e0 = beg;; e0 += G) {
      const int e = e0 + sub;
      const bool act = e < end;
      if (!__ballot(act)) break;
      bool keep = false;
      int u = 0;
      if (act) {
        u = sci[e];
        if (MODE == 0) keep = u != (int)v && tc_rank_less(a.ro, nullptr, (int)v, u) && !(direct && e > beg && sci[e - 1] == u);
        else keep = e == beg || sci[e - 1] != u;
      }
      const u64 km = (__ballot(keep) >> gshift) & gmask;
      if (FILL) {
        if (keep) dci[at + __popcll(km & ((1ull << sub) - 1ull))] = u;
        at += __popcll(km);
      } else {
        mine += __popcll(km);
      }
    }
    if (!FILL && valid && sub == 0) a.cnt[v] = mine;
  }
}

// symmetric == 0: every entry (v, u), v != u, belongs to the row of its lower-ranked end: counted (cnt cleared before), or
// written behind tmp_ro[row] at the row's cursor (cur cleared before)
template <int G, bool FILL>
__global__ __launch_bounds__(BLOCK) void k_tc_orient(tc_build_args_t a) {
  if (a.stat[TC_S_ERR]) return;
  TC_ROW_LOOP(G, a.n) {
    const long long v = vb + gshift / G;
    if (v >= a.n) continue;
    const int beg = a.ro[v], end = a.ro[v + 1];
    for (int e = beg + sub; e < end; e += G) {
      const int u = a.ci[e];
      if (u == (int)v) continue;
      const bool fwd = tc_rank_less(a.ro, a.deg, (int)v, u);
      const int lo = fwd ? (int)v : u, hi = fwd ? u : (int)v;
      if (FILL) a.tmp_ci[a.tmp_ro[lo] + atomicAdd(a.cur + lo, 1)] = hi;
      else atomicAdd(a.cnt + lo, 1);
    }
  }
  (void)gmask;
}

// after a scan over n + 1 counts (the last one 0) ro[n] is the total: it must fit the arrays behind it
__global__ void k_tc_check(const int* ro, int n, long long cap, u64* stat) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && (ro[n] < 0 || (long long)ro[n] > cap)) stat[TC_S_ERR] = 1;
}

// The segmented sort's classification (segsort.hpp: k_segsort_classify) over the oriented rows, on the device: segment s = row s
// with heads = tmp_ro + 1.  Nothing to sort in direct mode.
__global__ __launch_bounds__(BLOCK) void k_tc_sort_classify(segsort_args_t<int, segsort_no_value_t> s, const int* ro, int n,
                                                            const u64* stat) {
  if (stat[TC_S_DIRECT] != 0 || stat[TC_S_ERR] != 0) return;
  for (long long base = (long long)blockIdx.x * BLOCK; base < n; base += (long long)gridDim.x * BLOCK) {
    const int v = (int)base + (int)threadIdx.x;
    const int len = v < n ? ro[v + 1] - ro[v] : 0;
    segsort_classify_one(s, v, len);
  }
}

// sdeg[v] = d+(v) + DAG entries that name v (sdeg cleared before); m_dag, the longest row, the wedges
template <int G>
__global__ __launch_bounds__(BLOCK) void k_tc_dagstats(tc_build_args_t a) {
  if (a.stat[TC_S_ERR]) return;
  u64 wedges = 0;
  int longest = 0;
  TC_ROW_LOOP(G, a.n) {
    const long long v = vb + gshift / G;
    if (v >= a.n) continue;
    const int beg = a.dag_ro[v], end = a.dag_ro[v + 1];
    for (int e = beg + sub; e < end; e += G) atomicAdd(a.sdeg + a.dag_ci[e], 1);
    if (sub == 0 && end > beg) {
      const u64 d = (u64)(end - beg);
      atomicAdd(a.sdeg + (int)v, end - beg);
      wedges += d * (d - 1) / 2;
      longest = max(longest, end - beg);
    }
  }
  (void)gmask;
  wedges = wave_sum(wedges);
  longest = wave_max(longest);
  if (lane_id() == 0) {
    if (wedges) tc_add(a.stat + TC_S_WEDGES, wedges);
    if (longest) atomicMax(a.stat + TC_S_MAXROW, (u64)longest);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.stat[TC_S_MDAG] = (u64)a.dag_ro[a.n];
}

struct tc_list_args_t {
  const int* ro;          // the DAG
  int n;
  int short_max, wave_max;
  int* s_list;
  int* m_list;
  int* l_list;
  int* cnt;               // [0] short, [1] wave-staged, [2] workgroup-staged rows
  const u64* stat;
};

// vertices with d+ >= 2 (a row of one entry closes no triangle) by d+ into the three lists
__global__ __launch_bounds__(BLOCK) void k_tc_worklist(tc_list_args_t a) {
  if (a.stat[TC_S_ERR]) return;
  const int lane = lane_id();
  const int wave = (int)((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / WAVE);
  const int waves = (int)(gridDim.x * (BLOCK / WAVE));
  __shared__ int s_stage[WAVES_PER_BLOCK][3][TC_LIST_STAGE];
  int* const st0 = s_stage[threadIdx.x / WAVE][0];
  int* const st1 = s_stage[threadIdx.x / WAVE][1];
  int* const st2 = s_stage[threadIdx.x / WAVE][2];
  int f0 = 0, f1 = 0, f2 = 0;
  for (long long base = (long long)wave * WAVE; base < a.n; base += (long long)waves * WAVE) {
    const int v = (int)base + lane;
    const int d = v < a.n ? a.ro[v + 1] - a.ro[v] : 0;
    wave_stage_push<TC_LIST_STAGE>(d >= 2 && d <= a.short_max, v, st0, f0, a.s_list, a.cnt + 0);
    wave_stage_push<TC_LIST_STAGE>(d >= 2 && d > a.short_max && d <= a.wave_max, v, st1, f1, a.m_list, a.cnt + 1);
    wave_stage_push<TC_LIST_STAGE>(d >= 2 && d > a.short_max && d > a.wave_max, v, st2, f2, a.l_list, a.cnt + 2);
  }
  wave_stage_flush(st0, f0, a.s_list, a.cnt + 0);
  wave_stage_flush(st1, f1, a.m_list, a.cnt + 1);
  wave_stage_flush(st2, f2, a.l_list, a.cnt + 2);
}

struct tc_count_args_t {
  const int* ro;          // the DAG
  const int* ci;
  const int* s_list;
  const int* m_list;
  const int* l_list;
  const int* cnt;
  u64* tri;
  u64* stat;
  int stage;              // entries of a stage the staged kernels use (at most their LDS arrays)
  int* sup = nullptr;     // EDGES (mgx/ktruss_fused.hpp): the per-entry supports the adds go to instead of tri
};

// Common elements of the sorted rows ci[p, p + pl) and ci[q, q + ql): the shorter one's entries are searched in the longer,
// each search from where the last one ended.  tri[w] gets one add per common element w.
// EDGES (the k-truss's supports, mgx/ktruss_fused.hpp): `sink` is the per-entry array, and the two positions of w -- in the row
// searched from and in the row searched in, both entries of the triangle -- get the add instead of w (32-bit, one per hit each).
template <bool EDGES = false, typename T>
__device__ __forceinline__ int tc_intersect(const int* __restrict__ ci, int p, int pl, int q, int ql, T* sink) {
  if (pl > ql) {
    const int t = p; p = q; q = t;
    const int tl = pl; pl = ql; ql = tl;
  }
  const int qe = q + ql;
  int lo = q, c = 0;
  for (int i = 0; i < pl && lo < qe; ++i) {
    const int x = ci[p + i];
    int hi = qe;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ci[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    if (lo < qe && ci[lo] == x) {
      ++c;
      if constexpr (EDGES) {
        atomicAdd(sink + p + i, 1);
        atomicAdd(sink + lo, 1);
      } else {
        tc_add(sink + x, 1ull);
      }
      ++lo;
    }
  }
  return c;
}

// a workgroup's partial of the total -> one add
__device__ __forceinline__ void tc_flush_total(u64 mine, u64* total) {
  __shared__ u64 s_tot[WAVES_PER_BLOCK];
  mine = wave_sum(mine);
  if (lane_id() == 0) s_tot[threadIdx.x / WAVE] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += s_tot[w];
    if (t) tc_add(total, t);
  }
}

// short rows: a wave takes 64 of them and spreads their entries over its lanes.  EDGES: the entry's own count goes to the entry
template <bool EDGES = false>
__global__ __launch_bounds__(BLOCK) void k_tc_short(tc_count_args_t a) {
  __shared__ int s_scan[WAVES_PER_BLOCK][WAVE];
  __shared__ unsigned s_acc[WAVES_PER_BLOCK][WAVE];
  int* const sc = s_scan[threadIdx.x / WAVE];
  unsigned* const acc = s_acc[threadIdx.x / WAVE];
  const int lane = lane_id();
  const int ns = a.cnt[0];
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) / WAVE, waves = (long long)gridDim.x * WAVES_PER_BLOCK;
  u64 total = 0;
  for (long long base = wave * WAVE; base < ns; base += waves * WAVE) {
    const long long i = base + lane;
    const int v = i < ns ? a.s_list[i] : -1;
    const int rv = v >= 0 ? a.ro[v] : 0;
    const int dv = v >= 0 ? a.ro[v + 1] - rv : 0;
    const int incl = wave_inclusive_sum(dv);
    const int T = __shfl(incl, WAVE - 1, WAVE);
    sc[lane] = incl;
    acc[lane] = 0u;
    wave_lds_fence();
    for (int t0 = 0; t0 < T; t0 += WAVE) {
      const int t = t0 + lane;
      const bool act = t < T;
      int r = 0;                                             // the first row whose inclusive sum is above t
      if (act) {
        int hi = WAVE - 1;
        while (r < hi) {
          const int mid = (r + hi) >> 1;
          if (sc[mid] <= t) r = mid + 1;
          else hi = mid;
        }
      }
      const int ra = __shfl(rv, r, WAVE), da = __shfl(dv, r, WAVE);
      if (act) {
        const int j = t - (sc[r] - da);
        const int b = a.ci[ra + j];
        const int rb = a.ro[b];
        int c;
        if constexpr (EDGES) c = tc_intersect<true>(a.ci, ra, da, rb, a.ro[b + 1] - rb, a.sup);
        else c = tc_intersect(a.ci, ra, da, rb, a.ro[b + 1] - rb, a.tri);
        if (c) {
          if constexpr (EDGES) atomicAdd(a.sup + ra + j, c);
          else tc_add(a.tri + b, (u64)c);
          atomicAdd(acc + r, (unsigned)c);
        }
      }
    }
    wave_lds_fence();
    const unsigned mine = acc[lane];
    if constexpr (!EDGES)
      if (mine) tc_add(a.tri + v, (u64)mine);
    total += mine;
    wave_lds_fence();                                        // (read before the next rows fill the arrays)
  }
  tc_flush_total(total, a.stat + TC_S_TOTAL);
}

// position of x in the sorted LDS copy s[0, n), or -1
__device__ __forceinline__ int tc_find(const int* s, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && s[lo] == x ? lo : -1;
}

// One staged row a by a team of TEAM threads (a wave or the workgroup), thread `tid` of it: per chunk of at most S entries of
// row a in `stage`, groups of TC_GROUP lanes stream the rows b of all of row a's entries; hits[k] counts the hits on stage[k].
// Returns this thread's share of tri[a]'s count (group leaders only).
// EDGES: a triangle found at entry (a, b) with common element c adds to its three entries: the entry itself (once per entry and
// chunk), c's slot of the stage = its position in row a (through the hit counters, once per chunk), and the streamed position of c
// in row b (one add per hit: nothing aggregates it).
template <int TEAM, bool EDGES = false>
__device__ __forceinline__ u64 tc_staged_row(const tc_count_args_t& a, int va, int* stage, unsigned* hits, int S, int tid) {
  constexpr int G = TC_GROUP, NG = TEAM / G;
  const int lane = lane_id(), sub = lane % G, gshift = lane - sub, g = tid / G;
  const u64 gmask = (1ull << G) - 1ull;
  const int ra = a.ro[va], da = a.ro[va + 1] - ra;
  u64 ca = 0;
  for (int c0 = 0; c0 < da; c0 += S) {
    const int cl = min(S, da - c0);
    for (int k = tid; k < cl; k += TEAM) {
      stage[k] = a.ci[ra + c0 + k];
      hits[k] = 0u;
    }
    if (TEAM == WAVE) wave_lds_fence();
    else __syncthreads();
    for (int j0 = 0; j0 < da; j0 += NG) {
      const int j = j0 + g;
      int b = -1, rb = 0, db = 0;
      if (j < da) {
        b = a.ci[ra + j];
        rb = a.ro[b];
        db = a.ro[b + 1] - rb;
      }
      int cb = 0;
      for (int k = sub;; k += G) {
        const bool act = k < db;
        if (!__ballot(act)) break;
        int pos = -1;
        if (act) pos = tc_find(stage, cl, a.ci[rb + k]);
        const u64 hm = __ballot(pos >= 0);
        if (pos >= 0) {
          atomicAdd(hits + pos, 1u);
          if constexpr (EDGES) atomicAdd(a.sup + rb + k, 1);
        }
        cb += __popcll((hm >> gshift) & gmask);
      }
      if (sub == 0 && cb) {
        if constexpr (EDGES) atomicAdd(a.sup + ra + j, cb);
        else tc_add(a.tri + b, (u64)cb);
        ca += (u64)cb;
      }
    }
    if (TEAM == WAVE) wave_lds_fence();
    else __syncthreads();
    for (int k = tid; k < cl; k += TEAM) {
      const unsigned h = hits[k];
      if constexpr (EDGES) {
        if (h) atomicAdd(a.sup + ra + c0 + k, (int)h);
      } else {
        if (h) tc_add(a.tri + stage[k], (u64)h);
      }
    }
    if (TEAM == WAVE) wave_lds_fence();                       // (read before the next chunk fills the stage)
    else __syncthreads();
  }
  return ca;
}

// rows a wave stages
template <bool EDGES = false>
__global__ __launch_bounds__(BLOCK) void k_tc_wave(tc_count_args_t a) {
  __shared__ int s_stage[WAVES_PER_BLOCK][TC_WAVE_STAGE];
  __shared__ unsigned s_hits[WAVES_PER_BLOCK][TC_WAVE_STAGE];
  const int w = threadIdx.x / WAVE, lane = lane_id();
  const int nm = a.cnt[1];
  const int S = min(a.stage, TC_WAVE_STAGE);
  u64 total = 0;
  for (long long it = (long long)blockIdx.x * WAVES_PER_BLOCK + w; it < nm; it += (long long)gridDim.x * WAVES_PER_BLOCK) {
    const int va = a.m_list[it];
    const u64 ca = wave_sum(tc_staged_row<WAVE, EDGES>(a, va, s_stage[w], s_hits[w], S, lane));
    if (lane == 0) {
      if (!EDGES && ca) tc_add(a.tri + va, ca);
      total += ca;
    }
  }
  tc_flush_total(total, a.stat + TC_S_TOTAL);
}

// rows a workgroup stages
template <bool EDGES = false>
__global__ __launch_bounds__(BLOCK) void k_tc_block(tc_count_args_t a) {
  __shared__ int s_stage[TC_BLOCK_STAGE];
  __shared__ unsigned s_hits[TC_BLOCK_STAGE];
  __shared__ u64 s_ca[WAVES_PER_BLOCK];
  const int nl = a.cnt[2];
  const int S = min(a.stage, TC_BLOCK_STAGE);
  u64 total = 0;
  for (long long it = blockIdx.x; it < nl; it += gridDim.x) {
    const int va = a.l_list[it];
    const u64 ca = wave_sum(tc_staged_row<BLOCK, EDGES>(a, va, s_stage, s_hits, S, (int)threadIdx.x));
    if (lane_id() == 0) s_ca[threadIdx.x / WAVE] = ca;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 t = 0;
      for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += s_ca[w];
      if (!EDGES && t) tc_add(a.tri + va, t);
      total += t;
    }
    __syncthreads();
  }
  tc_flush_total(total, a.stat + TC_S_TOTAL);
}

// stat[TC_S_TOTAL] += sum of tri (the operator path's total is this sum / 3); one add per workgroup
__global__ __launch_bounds__(BLOCK) void k_tc_sum(const u64* tri, int n, u64* stat) {
  u64 mine = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) mine += tri[i];
  tc_flush_total(mine, stat + TC_S_TOTAL);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct tc_dag_t {
  bool built = false;
  mem_t<int> ro, ci, sdeg;
  mem_t<int> s_list, m_list, l_list;
  mem_t<int> words;                 // [0] short, [1] wave-staged, [2] workgroup-staged rows
  mem_t<u64> stat;                  // TC_S_*
  long long h[TC_S_WORDS] = {0};    // the stat words as the host last read them
};

// what a build needs until its launches have run (freed behind the run's host wait)
struct tc_build_tmp_t {
  mem_t<int> deg, cnt, cur, tmp_ro, tmp_ci, short_list, mid_list, sort_cnt;
  mem_t<int2> tile_list;
};

struct tc_state_t {
  int n = 0;
  long long m = 0;
  tc_opts_t opts;
  tc_dag_t dag[2];                  // [symmetric]
  mem_t<u64> tri;
  pinned_t<u64> h_pinned;
  int last = -1;                    // the DAG of the last run (-1: no run yet)
  long long launches = 0;
  long long waits = 0;              // host waits of the run in progress: counted where the host waits, not stated

  tc_state_t(int n_, long long m_, standard_context_t& ctx) : n(n_), m(m_), opts(tc_opts_t::from_env()) {
    // (the merge passes of the sort run for rows of up to m entries at run widths w with 2 w an int)
    if (m > (1LL << 30)) throw mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx tc: more than 2^30 CSR entries");
    tri = mem_t<u64>((size_t)std::max(n, 1), ctx);
    h_pinned = pinned_t<u64>(TC_S_WORDS);
    ctx.reserve_scratch(scan_scratch_bytes((long long)n + 1));
  }

  template <typename F>
  void scan(F f, int* out, standard_context_t& ctx) {
    const long long tiles = scan_num_tiles((long long)n + 1);
    transform_scan(f, (long long)n + 1, out, ctx, nullptr);
    launches += tiles <= SCAN_LOOKBACK_MAX_TILES ? 1 : 3;
  }

  template <int G>
  void build_g(tc_dag_t& d, tc_build_tmp_t& t, const int* ro, const int* ci, bool symmetric, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    const size_t N = (size_t)std::max(n, 1), M = (size_t)std::max<long long>(m, 1);
    d.ro = mem_t<int>(N + 1, ctx);
    d.ci = mem_t<int>(M, ctx);
    d.sdeg = mem_t<int>(N, ctx);
    d.s_list = mem_t<int>(N, ctx);
    d.m_list = mem_t<int>(N, ctx);
    d.l_list = mem_t<int>(N, ctx);
    d.words = mem_t<int>(4, ctx);
    d.stat = mem_t<u64>(TC_S_WORDS, ctx);
    t.cnt = mem_t<int>(N + 1, ctx);
    t.tmp_ro = mem_t<int>(N + 1, ctx);
    t.tmp_ci = mem_t<int>(M, ctx);
    t.short_list = mem_t<int>(N, ctx);
    t.mid_list = mem_t<int>(N, ctx);
    t.sort_cnt = mem_t<int>(4, ctx);
    t.tile_list = mem_t<int2>((size_t)(2 * (m / SEGSORT_TILE) + 2), ctx);
    if (!symmetric) {
      t.deg = mem_t<int>(N, ctx);
      t.cur = mem_t<int>(N, ctx);
    }
    tc_build_args_t a;
    a.ro = ro; a.ci = ci; a.n = n; a.symmetric = symmetric ? 1 : 0; a.deg = t.deg.data(); a.cnt = t.cnt.data(); a.cur = t.cur.data();
    a.tmp_ro = t.tmp_ro.data(); a.tmp_ci = t.tmp_ci.data(); a.dag_ro = d.ro.data(); a.dag_ci = d.ci.data(); a.sdeg = d.sdeg.data();
    a.stat = d.stat.data(); a.cap = m;
    // groups of G lanes per row: G rows of work a lane at most
    const int grid = grid_for((long long)n * G, BLOCK, max_blocks);
    hipLaunchKernelGGL(k_tc_init, dim3(1), dim3(BLOCK), 0, st, a.stat, a.symmetric);
    MGX_HIP(hipMemsetAsync(d.sdeg.data(), 0, N * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(d.words.data(), 0, 4 * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(t.sort_cnt.data(), 0, 4 * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(t.cnt.data(), 0, (N + 1) * sizeof(int), st));
    if (!symmetric) {
      MGX_HIP(hipMemsetAsync(t.deg.data(), 0, N * sizeof(int), st));
      MGX_HIP(hipMemsetAsync(t.cur.data(), 0, N * sizeof(int), st));
    }
    hipLaunchKernelGGL(k_tc_rowinfo<G>, dim3(grid), dim3(BLOCK), 0, st, a);
    if (symmetric) hipLaunchKernelGGL((k_tc_select<G, 0, false>), dim3(grid), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_tc_orient<G, false>), dim3(grid), dim3(BLOCK), 0, st, a);
    const int nn = n;
    const int* cnt = t.cnt.data();
    auto counts = [=] __device__(long long i) { return i < nn ? cnt[i] : 0; };
    scan(counts, a.tmp_ro, ctx);
    hipLaunchKernelGGL(k_tc_check, dim3(1), dim3(WAVE), 0, st, (const int*)a.tmp_ro, n, a.cap, a.stat);
    if (symmetric) hipLaunchKernelGGL((k_tc_select<G, 0, true>), dim3(grid), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_tc_orient<G, true>), dim3(grid), dim3(BLOCK), 0, st, a);
    launches += 5 + (symmetric ? 5 : 7);                      // (the kernels above, k_tc_init and the clears)
    // the oriented rows sorted (segsort.hpp's kernels; its host side waits for the list sizes, this one does not)
    {
      segsort_args_t<int, segsort_no_value_t> s;
      s.keys = a.tmp_ci; s.vals = nullptr; s.keys_tmp = a.dag_ci; s.vals_tmp = nullptr;      // (the DAG's array is free until the dedup)
      s.count = 0; s.heads = a.tmp_ro + 1; s.num_segments = n;                                // (segment s < n = row s; count is unused)
      s.short_list = t.short_list.data(); s.mid_list = t.mid_list.data(); s.tile_list = t.tile_list.data(); s.cnt = t.sort_cnt.data();
      auto up = [] __device__(int x, int y) { return x < y; };
      typedef decltype(up) C;
      typedef segsort_no_value_t V;
      hipLaunchKernelGGL(k_tc_sort_classify, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, s, (const int*)a.tmp_ro, n,
                         (const u64*)a.stat);
      hipLaunchKernelGGL((k_segsort_wave<int, V, C>), dim3(max_blocks), dim3(BLOCK), 0, st, s, up);
      hipLaunchKernelGGL((k_segsort_block<int, V, C, false>), dim3(max_blocks), dim3(BLOCK), 0, st, s, up);
      launches += 3;
      if (m > SEGSORT_TILE) {
        hipLaunchKernelGGL((k_segsort_block<int, V, C, true>), dim3(max_blocks), dim3(BLOCK), 0, st, s, up);
        ++launches;
        int passes = 0;
        int* src = s.keys;
        int* dst = s.keys_tmp;
        for (long long w = SEGSORT_TILE; w < m; w *= 2) {
          hipLaunchKernelGGL((k_segsort_merge<int, V, C>), dim3(max_blocks), dim3(BLOCK), 0, st, s, (const int*)src, (const V*)nullptr,
                             dst, (V*)nullptr, (int)w, up);
          std::swap(src, dst);
          ++passes;
        }
        if (passes & 1) hipLaunchKernelGGL((k_segsort_copy_back<int, V>), dim3(max_blocks), dim3(BLOCK), 0, st, s);
        launches += passes + (passes & 1);
      }
    }
    hipLaunchKernelGGL((k_tc_select<G, 1, false>), dim3(grid), dim3(BLOCK), 0, st, a);
    scan(counts, a.dag_ro, ctx);
    hipLaunchKernelGGL(k_tc_check, dim3(1), dim3(WAVE), 0, st, (const int*)a.dag_ro, n, a.cap, a.stat);
    hipLaunchKernelGGL((k_tc_select<G, 1, true>), dim3(grid), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_tc_dagstats<G>, dim3(grid), dim3(BLOCK), 0, st, a);
    tc_list_args_t la;
    la.ro = a.dag_ro; la.n = n; la.short_max = opts.short_max; la.wave_max = opts.wave_max;
    la.s_list = d.s_list.data(); la.m_list = d.m_list.data(); la.l_list = d.l_list.data(); la.cnt = d.words.data(); la.stat = a.stat;
    hipLaunchKernelGGL(k_tc_worklist, dim3(grid_for(n, BLOCK, max_blocks)), dim3(BLOCK), 0, st, la);
    launches += 5;
    MGX_CHECK_LAUNCH("mgx tc build");
  }

  // Enqueue the build of dag[symmetric] unless it is there; true: this call built it.  `t` must outlive the launches.
  bool ensure_dag(bool symmetric, const int* ro, const int* ci, tc_build_tmp_t& t, standard_context_t& ctx) {
    tc_dag_t& d = dag[symmetric ? 1 : 0];
    if (d.built) return false;
    d = tc_dag_t();
    if (m < 8LL * std::max(n, 1)) build_g<8>(d, t, ro, ci, symmetric, ctx);
    else build_g<64>(d, t, ro, ci, symmetric, ctx);
    return true;
  }

  // the stat words of d to the host: THE host wait.  Throws when the build's size check failed.
  void read_stats(tc_dag_t& d, bool built_now, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    h_pinned.fetch(d.stat.data(), TC_S_WORDS, st);
    ++waits;
    for (int i = 0; i < TC_S_WORDS; ++i) d.h[i] = (long long)h_pinned[i];
    if (d.h[TC_S_ERR]) {
      d = tc_dag_t();
      throw mgx_error(MGX_E_FRONTIER_OVERFLOW, "mgx tc: the oriented graph does not fit 2^31 - 1 entries");
    }
    // (d.ci keeps its m entries although m_dag <= m / 2 on symmetric input: fitting it needs a copy the host either waits for
    //  or frees around, and a run makes one host wait)
    if (built_now) d.built = true;
  }

  // which kernel the rows of the last run's DAG went to, and the switches in effect: {short rows, wave-staged rows,
  // workgroup-staged rows, entries of a workgroup's stage, entries of a wave's stage, short_max, wave_max}
  std::vector<long long> bins(standard_context_t& ctx) {
    if (last < 0) throw mgx_error(MGX_E_INVALID, "mgx_tc_bins: no run yet");
    int w[4] = {0, 0, 0, 0};
    if (n > 0) MGX_HIP(dtoh(w, (const int*)dag[last].words.data(), 4, ctx.stream()));
    return {w[0], w[1], w[2], std::min(opts.stage, TC_BLOCK_STAGE), std::min(opts.stage, TC_WAVE_STAGE), opts.short_max, opts.wave_max};
  }

  // {triangles, m_dag, longest row, wedges, rows used as they are, built, host waits, launches}
  std::vector<long long> result(const tc_dag_t& d, long long triangles, bool built_now) const {
    return {triangles, d.h[TC_S_MDAG], d.h[TC_S_MAXROW], d.h[TC_S_WEDGES], d.h[TC_S_DIRECT], built_now ? 1 : 0, waits, launches};
  }

  // The fused run (ro, ci: the CSR on the device).
  std::vector<long long> run(const int* ro, const int* ci, bool symmetric, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    launches = waits = 0;
    last = -1;
    if (n <= 0) return {0, 0, 0, 0, symmetric ? 1 : 0, 0, 0, 0};
    tc_build_tmp_t tmp;
    const bool built_now = ensure_dag(symmetric, ro, ci, tmp, ctx);
    tc_dag_t& d = dag[symmetric ? 1 : 0];
    const int max_blocks = std::max(ctx.num_cus, 1) * 8;
    MGX_HIP(hipMemsetAsync(tri.data(), 0, (size_t)n * sizeof(u64), st));
    MGX_HIP(hipMemsetAsync(d.stat.data() + TC_S_TOTAL, 0, sizeof(u64), st));
    tc_count_args_t a;
    a.ro = d.ro.data(); a.ci = d.ci.data(); a.s_list = d.s_list.data(); a.m_list = d.m_list.data(); a.l_list = d.l_list.data();
    a.cnt = d.words.data(); a.tri = tri.data(); a.stat = d.stat.data(); a.stage = opts.stage;
    hipLaunchKernelGGL(k_tc_block<false>, dim3(max_blocks), dim3(BLOCK), 0, st, a);      // the heaviest rows first
    hipLaunchKernelGGL(k_tc_wave<false>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_tc_short<false>, dim3(max_blocks), dim3(BLOCK), 0, st, a);
    launches += 5;                                             // (two clears, three kernels)
    MGX_CHECK_LAUNCH("mgx tc run");
    read_stats(d, built_now, ctx);
    last = symmetric ? 1 : 0;
    return result(d, d.h[TC_S_TOTAL], built_now);
  }
};

}  // namespace mgx
