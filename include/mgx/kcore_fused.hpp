// mgx/kcore_fused.hpp -- k-core decomposition, fused (mgx_kcore_run): worklist peeling, one launch per step, batches of steps
// per host wait.
//
// The definition (the operator path include/gunrock/kcore/ and tests/kcore_model.py compute the same, on any CSR):
//   deg = row lengths, core = 0, largest = -1
//   loop: no deg > 0: stop.  k = 1 + min(deg > 0); k > n: stop.  front = { deg == k - 1 }
//         while front: core[front] = k - 1, deg[front] = 0; every entry (v, u) of the front takes 1 from deg[u];
//                      cand = the u whose degree this pass took from >= k to < k; front = { u in cand: deg[u] > 0 }
//                      (a candidate at <= 0 is STRANDED: it never leaves and keeps core 0)
//         no deg > 0 left: largest = k - 1, stop   (all who are left have deg >= k or <= 0)
//
// What a step does here.  The run is a chain of steps, each a launch of k_kcore_step:
//   MIN     over all vertices: the smallest positive degree (a level begins) -- and after level k, whoever is at degree k
//           leaves at once: nobody positive is below k then, so they are the first front of level k + 1
//   LIST    over all vertices: those at k - 1 leave and become the front  (or the run ends: nobody left, or k > n); only
//           where MIN found the next level to be further than k + 1
//   EXPAND  the front's entries: one returning decrement each; the decrement that returns k has crossed: its target
//           becomes a candidate -- exactly once per vertex and k
//   FILTER  the candidates: degree > 0 leaves and joins the next front, the others are stranded.  It is a step of its own
//           because "after ALL of the pass's decrements and before any of the next pass's" is a launch boundary.
//   MINI    a front of at most KCORE_MINI_MAX entries: ONE workgroup runs expand / filter / expand ... with its own barrier
//           between them and the lists in LDS (entries spread over the threads by a search in the rows' running sum), until
//           the front is empty or has outgrown it -- most passes are this small, and a launch costs more than they do.
// Which kind a launch performs is decided on the device, from the word the launch before left (what it was, its k, what it
// counted): the ring, the log and the host's batches are launch_chain.hpp's.  No launch is idle until the run is over.
// The front is two lists: short rows (a thread each, the wave walking its rows in step) and (vertex, segment) items of
// KCORE_SEG entries for the long ones (a wave each) -- late passes are a few hubs with rows of 10^4 - 10^5 entries.
// List appends go through wave-private LDS stages (128 short rows, 64 long ones) behind one returning add each, and that
// add carries the entries of what it appends in its upper half (MINI or EXPAND: decided by their sum).  Adds to ONE word by
// every wave of the device are what a step costs (6 - 9 ns each, measured: three more a wave for the totals made a LIST step
// 100 us, one per long row and wave made a MIN step 145 us), so the scans run on a quarter of the workgroups, and "vertices
// removed" and "entries expanded" are counted once, by the launch that finds the run over: who left has a core number above 0.
#pragma once
#include <algorithm>
#include <vector>

#include "launch_chain.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int KCORE_UNROLL = 4;          // decrements a lane has in flight: their latency is what a small pass costs
constexpr int KCORE_SEG = KCORE_UNROLL * WAVE;      // entries of a long row one wave expands
constexpr int KCORE_LONG_MIN = 32;       // rows of at least this many entries are long
constexpr int KCORE_STAGE = 2 * WAVE;
constexpr int KCORE_MINI_MAX = 2048;     // entries of a front one workgroup peels on its own

enum kcore_kind_t : int { KCORE_INIT = 0, KCORE_MIN = 1, KCORE_LIST = 2, KCORE_EXPAND = 3, KCORE_FILTER = 4, KCORE_DONE = 5, KCORE_MINI = 6 };

// what a launch leaves for the next one (cleared two launches ahead)
struct kcore_word_t {
  int kind;                      // what the launch was (MINI leaves FILTER: it ends where a FILTER ends)
  int k;                         // the level it worked at
  int n_cand;                    // EXPAND: candidates
  int min_enc;                   // MIN: INT_MAX - (smallest positive degree); 0: nobody has one
  unsigned long long shorts;     // LIST, FILTER: short rows of the front | their entries << 32
  unsigned long long items;      //               (vertex, segment) items of its long rows | their entries << 32
};
__host__ __device__ __forceinline__ int kcore_lo(unsigned long long w) { return (int)(unsigned)w; }
__host__ __device__ __forceinline__ int kcore_hi(unsigned long long w) { return (int)(w >> 32); }

// what the run counts ([0] - [4] are mgx_kcore_run's stats), and how it ended
struct kcore_totals_t {
  long long levels, passes, expanded, removed, stranded;
  int largest, done;
};

// the run's words in device memory, behind one pointer (the kernel's scalar registers are counted)
using kcore_control_t = chain_control_t<kcore_word_t, kcore_totals_t>;

struct kcore_step_args_t {
  const int* ro;
  const int* ci;
  int* deg;
  int* core;
  int* cand;                     // the candidates, and behind them (at max(n, 1)) the front's short rows
  int2* f_items;
  kcore_control_t* ctl;
  int n;
  __device__ __forceinline__ int* f_short() const { return cand + max(n, 1); }
};

// A wave's share of the front being made: short rows wait in `rows`, long rows in `hubs`, each going out behind ONE returning add
// that also carries their entries (upper half of the word); a long row goes out as its segments' items.
struct kcore_front_stage_t {
  int* rows;
  int* hubs;
  int n_rows = 0, n_hubs = 0;
  int entries = 0;               // the lane's share of the staged short rows' entries
};
__device__ __forceinline__ void kcore_flush_rows(const kcore_step_args_t& a, kcore_word_t* next, kcore_front_stage_t& f) {
  if (f.n_rows == 0) return;
  wave_lds_fence();
  const int work = wave_sum(f.entries);
  int base = 0;
  if (lane_id() == 0) base = kcore_lo(atomicAdd(&next->shorts, ((unsigned long long)work << 32) | (unsigned)f.n_rows));
  base = __shfl(base, 0, WAVE);
  for (int j = lane_id(); j < f.n_rows; j += WAVE) a.f_short()[base + j] = f.rows[j];
  wave_lds_fence();
  f.n_rows = 0;
  f.entries = 0;
}
__device__ __forceinline__ void kcore_flush_hubs(const kcore_step_args_t& a, kcore_word_t* next, kcore_front_stage_t& f) {
  if (f.n_hubs == 0) return;
  wave_lds_fence();
  const bool has = lane_id() < f.n_hubs;
  const int v = has ? f.hubs[lane_id()] : 0;
  const int len = has ? a.ro[v + 1] - a.ro[v] : 0;
  const int segs = (len + KCORE_SEG - 1) / KCORE_SEG;
  const int incl = wave_inclusive_sum(segs);
  const int work = wave_sum(len);
  int base = 0;
  if (lane_id() == WAVE - 1) base = kcore_lo(atomicAdd(&next->items, ((unsigned long long)work << 32) | (unsigned)incl));
  base = __shfl(base, WAVE - 1, WAVE);
  for (int s = 0; s < segs; ++s) a.f_items[base + incl - segs + s] = make_int2(v, s);
  wave_lds_fence();
  f.n_hubs = 0;
}
// a wave's vertices that have left (at most one a lane, `len` entries; all lanes call) into the front
__device__ __forceinline__ void kcore_enlist(const kcore_step_args_t& a, kcore_word_t* next, bool leaves, int v, int len,
                                             kcore_front_stage_t& f) {
  const bool is_long = leaves && len >= KCORE_LONG_MIN;
  const bool is_short = leaves && !is_long;
  const u64 sm = __ballot(is_short);
  if (sm) {
    const int c = __popcll(sm);
    if (f.n_rows + c > KCORE_STAGE) kcore_flush_rows(a, next, f);
    if (is_short) {
      f.rows[f.n_rows + rank_in_mask(sm)] = v;
      f.entries += len;
    }
    f.n_rows += c;
  }
  const u64 lm = __ballot(is_long);
  if (lm) {
    const int c = __popcll(lm);
    if (f.n_hubs + c > WAVE) kcore_flush_hubs(a, next, f);
    if (is_long) f.hubs[f.n_hubs + rank_in_mask(lm)] = v;
    f.n_hubs += c;
  }
}
__device__ __forceinline__ void kcore_flush_front(const kcore_step_args_t& a, kcore_word_t* next, kcore_front_stage_t& f) {
  kcore_flush_rows(a, next, f);
  kcore_flush_hubs(a, next, f);
}

// EXPAND: KCORE_UNROLL entries a lane, e0 + j * stride for j with e0 + j * stride < e1 (all lanes call): the decrements first,
// all in flight together, then the candidates
__device__ __forceinline__ void kcore_take(const kcore_step_args_t& a, kcore_word_t* next, int e0, int stride, int e1, int k, int* stage,
                                           int& fill) {
  int u[KCORE_UNROLL], old[KCORE_UNROLL];
#pragma unroll
  for (int j = 0; j < KCORE_UNROLL; ++j) u[j] = e0 + j * stride < e1 ? a.ci[e0 + j * stride] : -1;
#pragma unroll
  for (int j = 0; j < KCORE_UNROLL; ++j) old[j] = u[j] >= 0 ? atomicAdd(a.deg + u[j], -1) : 0;
#pragma unroll
  for (int j = 0; j < KCORE_UNROLL; ++j) wave_stage_push<KCORE_STAGE>(u[j] >= 0 && old[j] == k, u[j], stage, fill, a.cand, &next->n_cand);
}

// What MINI keeps in LDS: the front (vertex, running sum of the row lengths before it), the candidates, and two counters --
// `pack` is front size << 32 | entries, so that one add gives a vertex its slot and its place in the running sum together.
struct kcore_mini_lds_t {
  int front[KCORE_MINI_MAX];
  int off[KCORE_MINI_MAX];
  int cand[KCORE_MINI_MAX];
  unsigned long long pack;
  int n_cand;
};

// MINI (workgroup 0 alone): the front the launch before left has at most KCORE_MINI_MAX entries.  Passes until the front is empty
// or larger than that; then it is handed on as a FILTER hands it on.  The degrees are read and zeroed with agent-scope atomics:
// the decrements are done in L2, a plain load could be served from this CU's own cache.
__device__ __forceinline__ void kcore_mini(const kcore_step_args_t& a, const kcore_word_t& prev, kcore_word_t* next, int k,
                                           kcore_mini_lds_t& s, kcore_front_stage_t& f) {
  const int tid = (int)threadIdx.x;
  auto join = [&](int v, int len) {
    const unsigned long long p = atomicAdd(&s.pack, (1ull << 32) | (unsigned)len);
    s.front[kcore_hi(p)] = v;
    s.off[kcore_hi(p)] = kcore_lo(p);
  };
  if (tid == 0) { s.pack = 0; s.n_cand = 0; }
  __syncthreads();
  for (int i = tid; i < kcore_lo(prev.shorts); i += BLOCK) {
    const int v = a.f_short()[i];
    join(v, a.ro[v + 1] - a.ro[v]);
  }
  for (int i = tid; i < kcore_lo(prev.items); i += BLOCK) {
    const int2 item = a.f_items[i];
    if (item.y == 0) join(item.x, a.ro[item.x + 1] - a.ro[item.x]);
  }
  __syncthreads();
  int passes = 0, stranded = 0;
  int nf, total;
  for (;;) {
    nf = kcore_hi(s.pack);
    total = kcore_lo(s.pack);
    ++passes;
    for (int e = tid; e < total; e += BLOCK) {
      int lo = 0, hi = nf;                                   // the last front vertex whose running sum is <= e
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.off[mid] <= e) lo = mid; else hi = mid;
      }
      const int u = a.ci[a.ro[s.front[lo]] + (e - s.off[lo])];
      if (atomicAdd(a.deg + u, -1) == k) s.cand[atomicAdd(&s.n_cand, 1)] = u;
    }
    __threadfence();
    __syncthreads();
    const int nc = s.n_cand;
    __syncthreads();                                         // (everybody has read the counters)
    if (tid == 0) { s.pack = 0; s.n_cand = 0; }
    __syncthreads();
    for (int i = tid; i < nc; i += BLOCK) {
      const int u = s.cand[i];
      if (__hip_atomic_load(a.deg + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) {
        a.core[u] = k - 1;
        __hip_atomic_store(a.deg + u, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        join(u, a.ro[u + 1] - a.ro[u]);
      } else {
        ++stranded;
      }
    }
    __threadfence();
    __syncthreads();
    nf = kcore_hi(s.pack);
    total = kcore_lo(s.pack);
    if (nf == 0 || total > KCORE_MINI_MAX) break;
  }
  // a front that has outgrown the workgroup: into the lists, for an EXPAND of the whole device
  if (nf > 0) {
    for (int base = 0; base < nf; base += BLOCK) {
      const int i = base + tid;
      const bool in = i < nf;
      const int v = in ? s.front[i] : 0;
      kcore_enlist(a, next, in, v, in ? a.ro[v + 1] - a.ro[v] : 0, f);
    }
    kcore_flush_front(a, next, f);
  }
  stranded = wave_sum(stranded);
  if (lane_id() == 0 && stranded) atomicAdd((unsigned long long*)&a.ctl->totals.stranded, (unsigned long long)stranded);
  if (tid == 0) atomicAdd((unsigned long long*)&a.ctl->totals.passes, (unsigned long long)passes);
}

// launch: the launch's number in the run
__global__ __launch_bounds__(BLOCK) void k_kcore_step(kcore_step_args_t a, unsigned launch) {
  const kcore_word_t prev = a.ctl->left_by_prev(launch);
  kcore_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;      // (the host launches at most 4 workgroups a CU)
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left
  const int front_work = kcore_hi(prev.shorts) + kcore_hi(prev.items);
  const bool front = kcore_lo(prev.shorts) + kcore_lo(prev.items) > 0;
  const int expand = front_work <= KCORE_MINI_MAX ? KCORE_MINI : KCORE_EXPAND;
  int kind, k = prev.k;
  bool new_level = false;
  switch (prev.kind) {
    case KCORE_INIT: kind = KCORE_MIN; break;
    case KCORE_MIN: {
      kind = KCORE_LIST;
      new_level = true;
      if (front) {                                           // the level behind the last was the next: MIN has listed it
        k = prev.k + 1;
        kind = expand;
      } else if (prev.min_enc == 0) {                               // nobody has a positive degree: the level before was the last
        kind = KCORE_DONE;
        if (first_thread && k > 0) a.ctl->totals.largest = k - 1;
      } else {
        k = 0x7fffffff - prev.min_enc + 1;
        if (k > a.n) kind = KCORE_DONE;                      // the reference's k runs to n: largest stays -1
      }
      break;
    }
    case KCORE_LIST: kind = expand; break;
    case KCORE_EXPAND: kind = prev.n_cand > 0 ? KCORE_FILTER : KCORE_MIN; break;
    case KCORE_FILTER: kind = front ? expand : KCORE_MIN; break;
    default: kind = KCORE_DONE; break;
  }
  if (first_thread) {
    next->kind = kind == KCORE_MINI ? KCORE_FILTER : kind;
    next->k = k;
    a.ctl->log_kind(launch, kind);
    if (new_level && kind != KCORE_DONE) a.ctl->totals.levels += 1;
    if (kind == KCORE_EXPAND) a.ctl->totals.passes += 1;         // (MINI adds its own)
    if (kind == KCORE_DONE) a.ctl->totals.done = 1;
  }
  if (kind == KCORE_DONE) {
    if (prev.kind == KCORE_DONE) return;
    // the launch that finds the run over counts what it did: who has left has a core number above 0, and all its entries were expanded
    long long rows = 0, entries = 0;
    for (unsigned v = gtid; v < (unsigned)a.n; v += gthreads)
      if (a.core[v] > 0) {
        ++rows;
        entries += a.ro[v + 1] - a.ro[v];
      }
    rows = wave_sum(rows);
    entries = wave_sum(entries);
    if (lane_id() == 0 && rows) {
      atomicAdd((unsigned long long*)&a.ctl->totals.removed, (unsigned long long)rows);
      atomicAdd((unsigned long long*)&a.ctl->totals.expanded, (unsigned long long)entries);
    }
    return;
  }

  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  __shared__ int stages[WAVES_PER_BLOCK][KCORE_STAGE];
  __shared__ int hub_stages[WAVES_PER_BLOCK][WAVE];
  __shared__ kcore_mini_lds_t mini;
  __shared__ int block_best[WAVES_PER_BLOCK];
  int* const stage = stages[threadIdx.x / WAVE];
  int fill = 0;                                              // (of the candidates' stage: EXPAND)
  kcore_front_stage_t f;
  f.rows = stage;
  f.hubs = hub_stages[threadIdx.x / WAVE];

  if (kind == KCORE_MINI) {
    if (blockIdx.x == 0) kcore_mini(a, prev, next, k, mini, f);
    return;
  }

  if (kind != KCORE_EXPAND) {
    // MIN, LIST: over all vertices, those at degree `at` leave.  LIST: at = k - 1.  MIN: after level k nobody positive is below k,
    // so whoever is AT k is the first front of level k + 1, the next one -- if there is such a vertex; if not, the smallest
    // degree found here tells a LIST step which level is.  FILTER: over the candidates, those above 0 leave.
    const bool scanning = kind != KCORE_FILTER;
    // (a scan's cost is its adds to the state word, one or two a wave: a quarter of the workgroups, four vertices a lane in flight)
    const int scan_blocks = max((int)gridDim.x / 4, 1);
    if (scanning && (int)blockIdx.x >= scan_blocks) return;
    const int my_waves = scanning ? scan_blocks * WAVES_PER_BLOCK : waves;
    const int at = kind == KCORE_LIST ? k - 1 : (kind == KCORE_MIN && k >= 1 && k < a.n ? k : 0);
    const int core_number = kind == KCORE_MIN ? k : k - 1;
    const unsigned count = (unsigned)(scanning ? a.n : prev.n_cand);       // (< 2^31, and a step below is < 2^20: no wrap)
    int stranded = 0, best = 0x7fffffff;
    for (unsigned base = (unsigned)wave * KCORE_SEG; base < count; base += (unsigned)my_waves * KCORE_SEG) {
      // (the four loads first, then the four decisions one after the other: not unrolled, the kernel's scalar registers are counted)
      int v[KCORE_UNROLL], d[KCORE_UNROLL];
#pragma unroll
      for (int j = 0; j < KCORE_UNROLL; ++j) {
        const unsigned i = base + j * WAVE + lane;
        v[j] = i < count ? (scanning ? (int)i : a.cand[i]) : -1;
      }
#pragma unroll
      for (int j = 0; j < KCORE_UNROLL; ++j) d[j] = v[j] >= 0 ? a.deg[v[j]] : 0;
      static_assert(KCORE_UNROLL == 4, "the selects below");
#pragma unroll 1
      for (int j = 0; j < KCORE_UNROLL; ++j) {
        const int vj = j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3];
        const int dj = j == 0 ? d[0] : j == 1 ? d[1] : j == 2 ? d[2] : d[3];
        if (dj > 0) best = min(best, dj);
        const bool leaves = vj >= 0 && (scanning ? (at > 0 && dj == at) : dj > 0);
        stranded += (vj >= 0 && !scanning && !leaves) ? 1 : 0;
        int len = 0;
        if (leaves) {
          a.core[vj] = core_number;
          a.deg[vj] = 0;
          len = a.ro[vj + 1] - a.ro[vj];
        }
        kcore_enlist(a, next, leaves, vj, len, f);
      }
    }
    kcore_flush_front(a, next, f);
    if (kind == KCORE_FILTER) {
      stranded = wave_sum(stranded);
      if (lane == 0 && stranded) atomicAdd((unsigned long long*)&a.ctl->totals.stranded, (unsigned long long)stranded);
    }
    if (kind == KCORE_MIN) {                                 // one add a workgroup, if it would change anything
      best = wave_min(best);
      if (lane == 0) block_best[threadIdx.x / WAVE] = best;
      __syncthreads();
      if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) best = min(best, block_best[w]);
        const int enc = 0x7fffffff - best;
        if (enc > 0 && __hip_atomic_load(&next->min_enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < enc) atomicMax(&next->min_enc, enc);
      }
    }
    return;
  }

  // EXPAND: long rows' items first (a wave each), then the short rows (a thread each, the wave in step)
  const int n_items = kcore_lo(prev.items), n_short = kcore_lo(prev.shorts);
  for (int it = wave; it < n_items; it += waves) {
    const int2 item = a.f_items[it];
    const int s0 = a.ro[item.x] + item.y * KCORE_SEG;
    kcore_take(a, next, s0 + lane, WAVE, min(a.ro[item.x + 1], s0 + KCORE_SEG), k, stage, fill);
  }
  for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)n_short; base += (unsigned)waves * WAVE) {
    const unsigned i = base + lane;
    const bool in = i < (unsigned)n_short;
    const int v = in ? a.f_short()[i] : 0;
    const int beg = in ? a.ro[v] : 0;
    const int len = in ? a.ro[v + 1] - beg : 0;
    int longest = len;
    longest = wave_max(longest);
    for (int j = 0; j < longest; j += KCORE_UNROLL) kcore_take(a, next, beg + j, 1, beg + len, k, stage, fill);
  }
  wave_stage_flush(stage, fill, a.cand, &next->n_cand);
}

// The scratch of a graph's fused k-core (the core numbers and degrees are the problem's), and the run (host side)
struct kcore_fused_state_t {
  int n = 0;
  mem_t<int> lists;                        // candidates | short rows of the front
  mem_t<int2> f_items;
  mem_t<kcore_control_t> ctl;
  pinned_t<kcore_totals_t> h_totals;
  long long launches = 0;                  // of the last run, the idle ones behind its end included

  kcore_fused_state_t(int n_, long long m, context_t& ctx) : n(n_) {
    const size_t N = (size_t)std::max(n, 1);
    lists = mem_t<int>(2 * N, ctx);        // a vertex crosses a k once, and leaves once
    // long rows: at most min(n, m / long_min) of them, plus one item per KCORE_SEG entries beyond their first segment
    const long long items = std::min<long long>((long long)N, m / KCORE_LONG_MIN + 1) + m / KCORE_SEG + 1;
    f_items = mem_t<int2>((size_t)items, ctx);
    ctl = mem_t<kcore_control_t>(1, ctx);
    h_totals = pinned_t<kcore_totals_t>(1);
  }

  // Peel the graph (ro, ci: CSR on the device).  deg holds the row lengths and core zeros when the stream gets here; they end
  // as the operator path leaves them.  Returns {levels, removing passes, entries expanded, vertices removed, stranded, host
  // waits} and the largest k-core.
  std::vector<long long> run(const int* ro, const int* ci, int* deg, int* core, standard_context_t& ctx, int& largest) {
    const hipStream_t st = ctx.stream();
    kcore_totals_t zero{};
    zero.largest = -1;
    h_totals[0] = zero;
    kcore_control_t::reset(ctl.data(), h_totals.data(), st);
    kcore_step_args_t a;
    a.ro = ro; a.ci = ci; a.deg = deg; a.core = core;
    a.cand = lists.data(); a.f_items = f_items.data();
    a.ctl = ctl.data(); a.n = n;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 4);
    long long waits = 0;
    launches = 0;
    // every vertex leaves in a pass of its own at worst: 2 n + 2 launches per level kind, and then the end
    const long long most = 4ll * std::max(n, 1) + 8;
    launches = run_launch_chain(
        [&](long long i) { hipLaunchKernelGGL(k_kcore_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
        [&]() {
          h_totals.fetch(&ctl.data()->totals, 1, st);
          return h_totals->done != 0;
        },
        most, "mgx kcore step", &waits);
    largest = h_totals->largest;
    return {h_totals->levels, h_totals->passes, h_totals->expanded, h_totals->removed, h_totals->stranded, waits};
  }
};

}  // namespace mgx
