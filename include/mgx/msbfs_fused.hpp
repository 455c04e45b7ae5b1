// mgx/msbfs_fused.hpp -- bit-parallel multi-source BFS, fused (mgx_msbfs_run): 64 traversals share one 64-bit word per vertex, an
// edge read serves all of them, a level is a pass of ORs (Then et al., "The More the Merrier", VLDB 2014).  From the per-level
// counts come reach, farness, eccentricity and the harmonic sum of every source, and per vertex how many sources reach it and
// the sum of their depths.  One launch per step, batches of steps per host wait (launch_chain.hpp).
//
// The definition (the operator path include/gunrock/msbfs/ and tests/msbfs_model.py compute the same).  Original ids;
// an attached hub-first layout is ignored.
//   batches    sources[count] in batches of 64 in the given order: source 64 B + b is bit b of batch B; the last batch may be
//              partial, its unused bits are never set anywhere.  full = the batch's valid bits.
//   a batch    u64 seen[n], front[n], next[n].  Level 0: front[s_b] |= 1 << b, seen = front.  Level t -> t + 1: next[u] = OR of
//              front[w] over the entries (w, u); new = next & ~seen; seen |= new; front = new.  The batch ends when front is zero:
//              a batch whose deepest vertex is at depth D runs D + 1 levels (the last one finds nothing).
//   kinds      e_t = the out-entries of A_t = {v : front[v] != 0}.  Level t is PULL iff in-entries are available and pull_div > 0
//              and (u64)e_t * pull_div >= m, else PUSH: a function of e_t, m, MGX_MSBFS_PULL_DIV and the in-entries alone
//              (0: never; 2^30: whenever the front has an out-entry).
//              In-entries: row u itself when symmetric != 0 (the caller's word), else the genuine CSC; neither: every level PUSH.
//   results    per source: reach = vertices at depth >= 1, far = the sum of their depths, ecc = the deepest level, all exact;
//              harm = the sum over d = 1, 2 ... of cnt_d / d in double, added in ascending d by one thread per source.
//              per vertex: reach_in[v] = the sources (with their multiplicity) that have v at depth >= 1, far_in[v] = the sum of
//              those depths.  On request the depths, int32[count][n], -1 where unreached.
//
// The run is a chain of launches of k_msbfs_step (launch_chain.hpp: the ring, the clock, the host's batches; the log is kept by
// level here, not by launch).
//   RESET     over all vertices: the batch's seen, front and next are zeroed (the first batch: the per-vertex sums too, and the
//             rows per body are counted); the batch's per-source results and the level counts are zeroed
//   SEED      64 threads: the sources' bits (atomicOr: duplicates share a word), A_0 = the distinct sources, e_0, depth 0
//   PUSH      over the list A_t: every out-entry (v, u) with front[v] & ~seen[u] != 0 ORs those bits into next[u] (atomicOr)
//   PULL      over every u with ~seen[u] & full != 0: next[u] = the OR of front[w] over u's in-entries, a plain store; a lane's row
//             stops once seen[u] | acc covers full
//   LONG      (only behind a PUSH or PULL that listed rows) a wave per (vertex, segment) item of a row of more than wave_max
//             entries: PUSH as above; PULL: the segment's OR, reduced across the wave, meets the others' in an atomicOr on next[u]
//   FINALIZE  over all vertices: new = next & ~seen, seen |= new, front = new, next = 0; reach_in += popc(new), far_in += d popc(new);
//             the depth stores; A_{t+1} through the waves' LDS stages (worklist.hpp; what is left in them at the end leaves the
//             workgroup behind one add), e_{t+1} (one add per workgroup); the per-source counts: a wave holding
//             64 vertices' new words loops over the bits of their OR, m = ballot((new >> b) & 1), lane b adds popc(m); a workgroup's
//             sums meet in LDS, then one 64-bit atomic per (bit, workgroup), into one of 32 copies of the counts (adders on one
//             row serialise); 64 threads fold the level before's counts into reach,
//             far, ecc and harm.  It runs over all vertices, not over a list of the touched ones: PUSH and LONG would have to build
//             that list behind their atomics, and a pass over 16 bytes a vertex is small beside the EXPAND it follows.
//   rows by length (out-rows in PUSH, in-rows in PULL): a lane each up to short_max entries, a wave each up to wave_max (PULL:
//             OR-reduced across the wave), longer ones as items of seg entries via wave_append_segments.
//   depths    a row per source, int32[count][n], as it is delivered: inside the loop over the bits of a wave's OR the lanes that
//             have bit b hold consecutive vertices, so a bit's stores fall next to each other in one row; no transposing pass and
//             no second buffer.  (A vertex-major block per batch would need both.)
// What holds between the workgroups of one launch (per-XCD L2s are not coherent, a CU's L1 is not refreshed):
//   (a) no word a launch reads with plain loads is written in that launch by another thread: PUSH, PULL and LONG read front and
//       seen and write next; FINALIZE reads and writes seen[v], front[v], next[v] of the thread's own vertex only.
//   (b) next takes device-scope atomicOr (PUSH, LONG) or the plain store of the one lane that owns the vertex (PULL's short and wave
//       rows; a vertex gets one or the other in a launch, by its row's length); it is read in the launch after.
//   (c) the counters of a ring word and the level counts change by device-scope atomicAdd only and are read by the launches after.
// No cooperative launch, no grid-wide barrier, no inline assembly; every device loop is bounded by a size read once.
// Not built: more than one device, weighted distances, a batch width other than 64, use of the hub-first layout, an
// early stop inside a wave's or a segment's PULL row.
#pragma once
#include <algorithm>
#include <vector>

#include "env.hpp"
#include "launch_chain.hpp"
#include "row_bodies.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (all four defaults are unmeasured guesses until tools/msbfs_bench.py has swept them on the device)
constexpr int MSBFS_SHORT_MAX_DEFAULT = 32;
constexpr int MSBFS_WAVE_MAX_DEFAULT = 1024;
constexpr int MSBFS_SEG_DEFAULT = 1024;
constexpr int MSBFS_PULL_DIV_DEFAULT = 8;
constexpr int MSBFS_CUT_MAX = 1 << 20;          // largest short_max, wave_max and seg
constexpr int MSBFS_PULL_DIV_MAX = 1 << 30;     // always pull
constexpr int MSBFS_STAGE = 8 * WAVE;           // a wave's LDS stage of listed vertices: a dense level lists every vertex, one returning add per stage
constexpr int MSBFS_CNT_COPIES = 32;            // copies of the level counts, a workgroup adds to copy blockIdx % 32: adders on one row serialise

enum msbfs_kind_t : int {
  MSBFS_INIT = 0, MSBFS_RESET = 1, MSBFS_SEED = 2, MSBFS_PUSH = 3, MSBFS_PULL = 4, MSBFS_LONG = 5, MSBFS_FINALIZE = 6, MSBFS_DONE = 7
};
enum : int { MSBFS_T_PUSH = 0, MSBFS_T_PULL = 1, MSBFS_T_LONG = 2, MSBFS_T_FINALIZE = 3 };
// bins: rows without entries, a lane's, a wave's, segmented rows, their segments -- of the out-rows, then of the in-rows
enum : int { MSBFS_BINS = 10 };

struct msbfs_opts_t {
  row_cuts_t cuts = {MSBFS_SHORT_MAX_DEFAULT, MSBFS_WAVE_MAX_DEFAULT, MSBFS_SEG_DEFAULT};
  int pull_div = MSBFS_PULL_DIV_DEFAULT;
  static msbfs_opts_t from_env() {
    msbfs_opts_t o;
    o.cuts.short_max = env_int("MGX_MSBFS_SHORT_MAX", 0, MSBFS_CUT_MAX, o.cuts.short_max);
    o.cuts.wave_max = env_int("MGX_MSBFS_WAVE_MAX", 0, MSBFS_CUT_MAX, o.cuts.wave_max);
    o.cuts.seg = env_int("MGX_MSBFS_SEG", 1, MSBFS_CUT_MAX, o.cuts.seg);
    o.pull_div = env_int("MGX_MSBFS_PULL_DIV", 0, MSBFS_PULL_DIV_MAX, o.pull_div);
    o.cuts.wave_max = std::max(o.cuts.wave_max, o.cuts.short_max);
    return o;
  }
};

// what a launch leaves for the next one (cleared two launches ahead)
struct msbfs_word_t {
  int kind;         // what the launch was           -- these four are written by the launch's first thread
  int batch;        // its batch
  int t;            // its level
  int pull;         // the level is a PULL
  int n_act;        // SEED, FINALIZE: |A| of the level to come -- these three take atomicAdd
  int n_items;      // PUSH, PULL: the (vertex, segment) items of the long rows
  u64 e;            // SEED, FINALIZE: the out-entries of A
};

struct msbfs_totals_t {
  long long bins[MSBFS_BINS];
  chain_clock_t<4> timed;      // wall clock ticks per MSBFS_T_* (timed runs)
  long long push_levels, pull_levels;
  int deepest;                 // levels of the deepest batch
  int done;                    // bit 0: the run is over
};

// (the log: PULL per (batch, level), the first CHAIN_LOG_CAP levels of a run)
struct msbfs_control_t : chain_control_t<msbfs_word_t, msbfs_totals_t> {
  u64 cnt[3][MSBFS_CNT_COPIES][WAVE];      // the vertices found per bit at depth d, in the copies of cnt[d % 3]
};

struct msbfs_args_t {
  const int* ro;     // CSR
  const int* ci;
  const int* io;     // the in-entries' offsets and ids (NULL: none, every level pushes)
  const int* ia;
  u64* words;        // N = max(n, 1) seen | N front | N next | N reach_in | N far_in
  int* list;         // N: A of the level to come
  int2* items;       // item_cap
  const int* sources;  // count ids (NULL: source i is vertex i)
  long long* per_src;  // src_cap reach | src_cap far | src_cap ecc | src_cap harm (double)
  int* depth;        // count x n (NULL: not kept)
  msbfs_control_t* ctl;
  long long m;
  int n, count, batches, src_cap, item_cap;
  row_cuts_t cuts;
  int pull_div, timing;
  __device__ __forceinline__ u64* part(int k) const { return words + (size_t)k * (size_t)max(n, 1); }
  __device__ __forceinline__ u64* seen() const { return words; }
  __device__ __forceinline__ u64* front() const { return part(1); }
  __device__ __forceinline__ u64* next() const { return part(2); }
  __device__ __forceinline__ u64* reach_in() const { return part(3); }
  __device__ __forceinline__ u64* far_in() const { return part(4); }
  __device__ __forceinline__ int source(long long i) const { return sources ? sources[i] : (int)i; }
};

__device__ __forceinline__ u64 msbfs_uniform(u64 x) {      // a value all lanes hold, into scalar registers
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(x >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)x);
}
__device__ __forceinline__ u64 msbfs_full(int count, int batch) {
  const long long valid = min((long long)count - (long long)batch * WAVE, (long long)WAVE);
  return valid >= WAVE ? ~0ull : ((1ull << valid) - 1ull);
}
__device__ __forceinline__ int msbfs_clock_of(int kind) {
  if (kind == MSBFS_PUSH) return MSBFS_T_PUSH;
  if (kind == MSBFS_PULL) return MSBFS_T_PULL;
  return kind == MSBFS_LONG ? MSBFS_T_LONG : MSBFS_T_FINALIZE;      // (RESET and SEED count as FINALIZE's)
}

// launch: the launch's number in the run
__global__ __launch_bounds__(BLOCK) void k_msbfs_step(msbfs_args_t a, unsigned launch) {
  const msbfs_word_t prev = a.ctl->left_by_prev(launch);
  msbfs_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left
  int kind, batch = prev.batch, t = prev.t, pull = prev.pull;
  if (prev.kind == MSBFS_INIT) {
    kind = MSBFS_RESET; batch = 0; t = 0; pull = 0;
  } else if (prev.kind == MSBFS_RESET) {
    kind = MSBFS_SEED;
  } else if (prev.kind == MSBFS_SEED || prev.kind == MSBFS_FINALIZE) {
    if (prev.kind == MSBFS_FINALIZE) t = prev.t + 1;
    if (prev.n_act == 0) {                                       // the batch is over (a SEED always lists somebody)
      pull = 0; t = 0;
      if (batch + 1 < a.batches) { kind = MSBFS_RESET; ++batch; } else { kind = MSBFS_DONE; }
    } else {
      pull = (a.io != nullptr && a.pull_div > 0 && prev.e * (u64)a.pull_div >= (u64)a.m) ? 1 : 0;
      kind = pull ? MSBFS_PULL : MSBFS_PUSH;
    }
  } else if (prev.kind == MSBFS_PUSH || prev.kind == MSBFS_PULL) {
    kind = prev.n_items > 0 ? MSBFS_LONG : MSBFS_FINALIZE;
  } else if (prev.kind == MSBFS_LONG) {
    kind = MSBFS_FINALIZE;
  } else {
    kind = MSBFS_DONE;
  }
  if (first_thread) {
    next->kind = kind; next->batch = batch; next->t = t; next->pull = pull;
    msbfs_totals_t& tot = a.ctl->totals;
    if (kind == MSBFS_PUSH || kind == MSBFS_PULL) {
      const long long level = tot.push_levels + tot.pull_levels;
      if (level < CHAIN_LOG_CAP) a.ctl->log[level] = pull;
      if (pull) ++tot.pull_levels; else ++tot.push_levels;
      tot.deepest = max(tot.deepest, t + 1);
    }
    if (kind == MSBFS_DONE) tot.done |= 1;
    tot.timed.tick(a.timing, prev.kind, MSBFS_DONE, msbfs_clock_of(prev.kind));
  }
  if (kind == MSBFS_DONE) return;

  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  const unsigned n = (unsigned)a.n;
  u64* const seen = a.seen();
  u64* const front = a.front();
  u64* const nxt = a.next();

  if (kind == MSBFS_RESET) {
    const bool first_batch = batch == 0;
    row_bins_t b_out, b_in;
    long long seg_out = 0, seg_in = 0;
    for (unsigned v = gtid; v < n; v += gthreads) {
      seen[v] = 0; front[v] = 0; nxt[v] = 0;
      if (first_batch) {
        a.reach_in()[v] = 0; a.far_in()[v] = 0;
        const int lo = a.ro[v + 1] - a.ro[v];
        const int co = a.cuts.body_of(lo);
        b_out.count(co);
        if (co == ROW_LONG) seg_out += a.cuts.segments_of(lo);
        if (a.io) {
          const int li = a.io[v + 1] - a.io[v];
          const int cin = a.cuts.body_of(li);
          b_in.count(cin);
          if (cin == ROW_LONG) seg_in += a.cuts.segments_of(li);
        }
      }
    }
    if (first_batch) {
      long long* const bins = a.ctl->totals.bins;
      b_out.add_to(bins);
      b_in.add_to(bins + 5);
      seg_out = wave_sum(seg_out); seg_in = wave_sum(seg_in);
      if (lane == 0 && seg_out) atomicAdd((u64*)&bins[4], (u64)seg_out);
      if (lane == 0 && seg_in) atomicAdd((u64*)&bins[9], (u64)seg_in);
    }
    if (blockIdx.x == 0 && threadIdx.x < WAVE) {
      u64* const all_cnt = &a.ctl->cnt[0][0][0];
      for (int k = 0; k < 3 * MSBFS_CNT_COPIES; ++k) all_cnt[k * WAVE + threadIdx.x] = 0;
      const long long s = (long long)batch * WAVE + threadIdx.x;
      if (s < a.count) {
        a.per_src[s] = 0; a.per_src[(size_t)a.src_cap + s] = 0; a.per_src[2 * (size_t)a.src_cap + s] = 0;
        ((double*)a.per_src)[3 * (size_t)a.src_cap + s] = 0.0;
      }
    }
    return;
  }

  if (kind == MSBFS_SEED) {
    if (blockIdx.x == 0 && threadIdx.x < WAVE) {
      const int b = threadIdx.x;                                 // (wave 0 of the workgroup: b is the lane)
      const long long first = (long long)batch * WAVE;
      const bool valid = first + b < a.count;
      const int s = valid ? a.source(first + b) : -1;
      bool fresh = true;                                         // no earlier bit of the batch names the same vertex
#pragma nounroll
      for (int j = 0; j < WAVE; ++j) {
        const int sj = __shfl(s, j, WAVE);
        fresh = fresh && (j >= b || sj != s);
      }
      if (valid) {
        atomicOr(front + s, 1ull << b);
        atomicOr(seen + s, 1ull << b);
        if (fresh) {
          a.list[atomicAdd(&next->n_act, 1)] = s;
          atomicAdd(&next->e, (u64)(a.ro[s + 1] - a.ro[s]));
        }
        if (a.depth) a.depth[(size_t)(first + b) * (size_t)n + (size_t)s] = 0;
      }
    }
    return;
  }

  if (kind == MSBFS_PUSH) {
    const unsigned n_act = (unsigned)min(prev.n_act, a.n);
    for (unsigned base = (unsigned)wave * WAVE; base < n_act; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < n_act;
      const int v = in ? a.list[base + lane] : 0;
      const int beg = in ? a.ro[v] : 0;
      const int len = in ? a.ro[v + 1] - beg : 0;
      const u64 fv = in ? front[v] : 0;
      const int body = a.cuts.body_of(len);
      if (body == ROW_LANE)
        for (int k = 0; k < len; ++k) {
          const int u = a.ci[beg + k];
          const u64 bits = fv & ~seen[u];
          if (bits) atomicOr(nxt + u, bits);
        }
      for_each_wave_row(body == ROW_WAVE, [&](int src) {
        const int b0 = __shfl(beg, src, WAVE), l0 = __shfl(len, src, WAVE);
        const u64 f0 = (u64)__shfl((long long)fv, src, WAVE);
        for (int k = lane; k < l0; k += WAVE) {
          const int u = a.ci[b0 + k];
          const u64 bits = f0 & ~seen[u];
          if (bits) atomicOr(nxt + u, bits);
        }
      });
      if (__ballot(body == ROW_LONG)) wave_append_segments_outlined(body == ROW_LONG, v, len, a.cuts.seg, a.items, &next->n_items);
    }
    return;
  }

  if (kind == MSBFS_PULL) {
    const u64 full = msbfs_full(a.count, batch);
    for (unsigned base = (unsigned)wave * WAVE; base < n; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < n;
      const int u = (int)(base + lane);
      const u64 sn = in ? seen[u] : full;
      const bool need = (~sn & full) != 0;
      const int beg = need ? a.io[u] : 0;
      const int len = need ? a.io[u + 1] - beg : 0;
      const int body = a.cuts.body_of(len);
      if (body == ROW_LANE) {
        u64 acc = 0;
        for (int k = 0; k < len; ++k) {
          acc |= front[a.ia[beg + k]];
          if (((sn | acc) & full) == full) break;
        }
        if (acc & ~sn) nxt[u] = acc;
      }
      for_each_wave_row(body == ROW_WAVE, [&](int src) {
        const int b0 = __shfl(beg, src, WAVE), l0 = __shfl(len, src, WAVE);
        u64 acc = 0;
        for (int k = lane; k < l0; k += WAVE) acc |= front[a.ia[b0 + k]];
        acc = wave_or(acc);
        if (lane == src && (acc & ~sn)) nxt[u] = acc;
      });
      if (__ballot(body == ROW_LONG)) wave_append_segments_outlined(body == ROW_LONG, u, len, a.cuts.seg, a.items, &next->n_items);
    }
    return;
  }

  if (kind == MSBFS_LONG) {                                      // a wave per (vertex, segment) item
    const int n_items = min(prev.n_items, a.item_cap);
    const int* const off = pull ? a.io : a.ro;
    const int* const adj = pull ? a.ia : a.ci;
    for (int it = wave; it < n_items; it += waves) {
      const int2 item = a.items[it];
      const int x = item.x;
      const int beg = off[x];
      const int len = off[x + 1] - beg;
      const long long k0 = (long long)item.y * a.cuts.seg;
      const int k1 = (int)min((long long)len, k0 + a.cuts.seg);
      if (!pull) {
        const u64 fv = front[x];
        for (int k = (int)k0 + lane; k < k1; k += WAVE) {
          const int u = adj[beg + k];
          const u64 bits = fv & ~seen[u];
          if (bits) atomicOr(nxt + u, bits);
        }
      } else {
        u64 acc = 0;
        for (int k = (int)k0 + lane; k < k1; k += WAVE) acc |= front[adj[beg + k]];
        acc = wave_or(acc);
        if (lane == 0 && (acc & ~seen[x])) atomicOr(nxt + x, acc);
      }
    }
    return;
  }

  {                                                              // FINALIZE: the vertices at depth d = t + 1
    __shared__ u64 s_cnt[WAVE];
    __shared__ int s_stage[WAVES_PER_BLOCK][MSBFS_STAGE];
    __shared__ u64 s_entries;
    __shared__ int s_tail, s_base;
    if (threadIdx.x < WAVE) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_entries = 0; s_tail = 0; s_base = 0; }
    __syncthreads();
    const int d = t + 1;
    int* const stage = s_stage[threadIdx.x / WAVE];
    int fill = 0;
    u64 mine = 0;                                                // the vertices found for bit `lane`
    long long entries = 0;
    for (unsigned base = (unsigned)wave * WAVE; base < n; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < n;
      const int v = (int)(base + lane);
      const u64 nx = in ? nxt[v] : 0;
      const u64 fr = in ? front[v] : 0;
      u64 nw = 0;
      if (nx) {
        const u64 sn = seen[v];
        nw = nx & ~sn;
        nxt[v] = 0;
        if (nw) seen[v] = sn | nw;
      }
      if (fr != nw) front[v] = nw;
      if (!__ballot(nw != 0)) continue;
      if (nw) {
        const u64 pc = (u64)__popcll(nw);
        a.reach_in()[v] += pc;
        a.far_in()[v] += pc * (u64)d;
        entries += a.ro[v + 1] - a.ro[v];
      }
      u64 bits = msbfs_uniform(wave_or(nw));
      while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const bool has = (nw >> b) & 1ull;
        const u64 m = __ballot(has);
        if (lane == b) mine += (u64)__popcll(m);
        if (a.depth && has) a.depth[((size_t)batch * WAVE + (size_t)b) * (size_t)n + (size_t)v] = d;
      }
      wave_stage_push<MSBFS_STAGE>(nw != 0, v, stage, fill, a.list, &next->n_act);
    }
    // what is left in the waves' stages and the waves' entries leave the workgroup behind one add each: adds to one word from
    // every wave of the device cost a level more than its pass over the words
    wave_lds_fence();
    entries = wave_sum(entries);
    int tail_at = 0;
    if (lane == 0) {
      if (fill) tail_at = atomicAdd(&s_tail, fill);
      if (entries) atomicAdd(&s_entries, (u64)entries);
    }
    tail_at = __shfl(tail_at, 0, WAVE);
    if (mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_tail) s_base = atomicAdd(&next->n_act, s_tail);
      if (s_entries) atomicAdd(&next->e, s_entries);
    }
    __syncthreads();
    for (int k = lane; k < fill; k += WAVE) a.list[s_base + tail_at + k] = stage[k];
    if (threadIdx.x < WAVE && s_cnt[threadIdx.x]) atomicAdd(&a.ctl->cnt[d % 3][blockIdx.x % MSBFS_CNT_COPIES][threadIdx.x], s_cnt[threadIdx.x]);
    // the level before is complete: one thread per source folds its counts, in ascending depth
    if (blockIdx.x == 0 && threadIdx.x < WAVE) {
      u64 c = 0;
      for (int k = 0; k < MSBFS_CNT_COPIES; ++k) {
        c += a.ctl->cnt[t % 3][k][threadIdx.x];
        a.ctl->cnt[(d + 1) % 3][k][threadIdx.x] = 0;             // (depth d - 2's, folded by the FINALIZE before)
      }
      const long long s = (long long)batch * WAVE + threadIdx.x;
      if (c && s < a.count) {
        a.per_src[s] += (long long)c;
        a.per_src[(size_t)a.src_cap + s] += (long long)c * t;
        a.per_src[2 * (size_t)a.src_cap + s] = t;
        ((double*)a.per_src)[3 * (size_t)a.src_cap + s] += (double)c / (double)t;
      }
    }
  }
}

// The device state of a graph's fused multi-source BFS, and the run (host side).  The per-vertex state is allocated with the
// handle's first run; the sources' arrays and the depths grow when a run asks for more than any run before: a repeat run
// allocates nothing.
struct msbfs_fused_state_t {
  int n = 0;
  long long m = 0;
  msbfs_opts_t opts;
  mem_t<u64> words;
  mem_t<int> list, d_sources, depth;
  mem_t<int2> items;
  mem_t<long long> per_src;
  int item_cap = 0, src_cap = 0;
  size_t depth_cap = 0;
  mem_t<msbfs_control_t> ctl;
  pinned_t<msbfs_totals_t> h_totals;
  std::vector<long long> h_per_src;            // the last run's reach | far | ecc | harm (double), src_cap each
  long long launches = -1;                     // of the last run, the idle ones behind its end included (-1: no run yet)
  long long count = 0, levels = 0;             // of the last run
  bool kept_depths = false, csc_served = false;
  long long bins[MSBFS_BINS] = {0};
  bool timing = false;
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the last timed run: push, pull, long rows, finalize

  msbfs_fused_state_t(int n_, long long m_, context_t& ctx) : n(n_), m(m_), opts(msbfs_opts_t::from_env()) {
    const size_t N = (size_t)std::max(n, 1);
    words = mem_t<u64>(5 * N, ctx);
    list = mem_t<int>(N, ctx);
    // rows of more than wave_max entries: an item per seg entries and one per row
    item_cap = (int)std::min<long long>(std::min<long long>((long long)N, m / (opts.cuts.wave_max + 1) + 1) + m / opts.cuts.seg + 1, 0x7fffffff);
    items = mem_t<int2>((size_t)item_cap, ctx);
    ctl = mem_t<msbfs_control_t>(1, ctx);
    h_totals = pinned_t<msbfs_totals_t>(1);
  }

  const long long* reach() const { return h_per_src.data(); }
  const long long* far() const { return h_per_src.data() + src_cap; }
  const long long* ecc() const { return h_per_src.data() + 2 * (size_t)src_cap; }
  const double* harm() const { return (const double*)(h_per_src.data() + 3 * (size_t)src_cap); }
  const u64* reach_in() const { return words.data() + 3 * (size_t)std::max(n, 1); }
  const u64* far_in() const { return words.data() + 4 * (size_t)std::max(n, 1); }

  // Traverse from h_sources[cnt] (NULL: every vertex; the ids are checked by the caller).  ro, ci: the CSR on the device; io, ia:
  // the in-entries (NULL: none).  Returns the ten stats of mgx_msbfs_run.  Host waits: one per batch of launches of the chain
  // (launch_chain.hpp) and one for the read-back of the per-source results.
  std::vector<long long> run(const int* ro, const int* ci, const int* io, const int* ia, const int* h_sources, long long cnt, bool csc,
                             bool want_depths, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    launches = -1;                                           // (a run that throws leaves nothing to ask about)
    kept_depths = false;
    const long long batches = (cnt + WAVE - 1) / WAVE;
    if (cnt > src_cap) {
      per_src = mem_t<long long>(4 * (size_t)cnt, ctx);
      d_sources = mem_t<int>((size_t)cnt, ctx);
      src_cap = (int)cnt;
      h_per_src.assign(4 * (size_t)cnt, 0);
    }
    if (want_depths && (size_t)cnt * (size_t)n > depth_cap) {
      depth = mem_t<int>();                                  // (the old one goes first: both need not fit)
      depth_cap = 0;
      depth = mem_t<int>((size_t)cnt * (size_t)n, ctx);      // (no room: hip_error, MGX_E_HIP at the C-ABI)
      depth_cap = (size_t)cnt * (size_t)n;
    }
    count = cnt;
    csc_served = csc;
    levels = 0;
    for (double& p : phase_ms) p = 0.0;
    if (n <= 0 || cnt == 0) {
      launches = 0;
      for (long long& b : bins) b = 0;
      kept_depths = want_depths;
      return {cnt, 0, 0, 0, 0, 0, 0, 0, csc ? 1 : 0, want_depths ? 1 : 0};
    }
    if (h_sources) MGX_HIP(htod(d_sources.data(), h_sources, (size_t)cnt, st));
    if (want_depths) MGX_HIP(hipMemsetAsync(depth.data(), 0xff, (size_t)cnt * (size_t)n * sizeof(int), st));
    msbfs_control_t::reset(ctl.data(), st);
    msbfs_args_t a;
    a.ro = ro; a.ci = ci; a.io = io; a.ia = ia;
    a.words = words.data(); a.list = list.data(); a.items = items.data();
    a.sources = h_sources ? d_sources.data() : nullptr;
    a.per_src = per_src.data();
    a.depth = want_depths ? depth.data() : nullptr;
    a.ctl = ctl.data();
    a.m = m; a.n = n; a.count = (int)cnt; a.batches = (int)batches; a.src_cap = src_cap; a.item_cap = item_cap;
    a.cuts = opts.cuts; a.pull_div = opts.pull_div;
    a.timing = timing ? 1 : 0;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 8);
    long long waits = 0;
    // per batch a RESET, a SEED and at most n levels of an EXPAND, a LONG and a FINALIZE: a chain that is longer has not ended
    const long long most = batches * (3ll * ((long long)n + 1) + 2) + CHAIN_BATCH_MAX;
    const long long enqueued = run_launch_chain(
        [&](long long i) { hipLaunchKernelGGL(k_msbfs_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
        [&]() {
          h_totals.fetch(&ctl.data()->totals, 1, st);
          return (h_totals->done & 1) != 0;
        },
        most, "mgx msbfs step", &waits);
    const msbfs_totals_t tot = *h_totals.data();
    MGX_HIP(dtoh(h_per_src.data(), (const long long*)per_src.data(), 4 * (size_t)src_cap, st));
    ++waits;
    if (timing)
      for (int i = 0; i < 4; ++i) phase_ms[i] = chain_ticks_ms(tot.timed.clock[i]);
    for (int b = 0; b < MSBFS_BINS; ++b) bins[b] = tot.bins[b];
    long long sum_reach = 0;
    for (long long s = 0; s < cnt; ++s) sum_reach += reach()[s];
    levels = tot.push_levels + tot.pull_levels;
    kept_depths = want_depths;
    launches = enqueued;
    return {cnt, batches, tot.deepest, sum_reach, tot.push_levels, tot.pull_levels, waits, launches, csc ? 1 : 0, want_depths ? 1 : 0};
  }
};

}  // namespace mgx
