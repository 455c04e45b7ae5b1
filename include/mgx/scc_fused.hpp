// mgx/scc_fused.hpp -- strongly connected components, fused (mgx_scc_run): trim, one pivot reach, colouring rounds; one launch
// per step, batches of steps per host wait.
//
// The definition (the operator path include/gunrock/scc/ and tests/scc_model.py compute the same).  The graph is the
// directed graph of the CSR entries (v -> u) in original ids, its in-entries the genuine CSC.  label[v] = the smallest id of v's
// strongly connected component.  outdeg[v] / indeg[v] count v's entries to / from ALIVE vertices other than v (duplicates count,
// self-loops never).
//   alive = all.  TRIM.
//   somebody alive (the PIVOT phase): p = the alive vertex of the largest outdeg * indeg (64-bit; ties: the smaller id);
//       S = (alive reachable from p) and (alive reaching p), through alive vertices; label[S] = min(S); S leaves.  TRIM.
//   while somebody is alive (a ROUND): col[v] = v; to the fixpoint col[u] = min(col[u], col[v]) over alive arcs v -> u;
//       roots = { col[v] == v }; C = roots, then to the fixpoint every alive v with an arc v -> u, u in C, col[v] == col[u];
//       label[C] = col[C]; C leaves.  TRIM.
//   TRIM: to the fixpoint, every alive v with outdeg[v] == 0 or indeg[v] == 0: label[v] = v, v leaves.
// A root is the smallest id that reaches it, and its whole component reaches it: col is already the canonical label; only the
// pivot's component needs a minimum of its own.
//
// The run is a chain of launches of k_scc_step (launch_chain.hpp: the ring, the log, the clock, the host's batches).  A launch
// derives its kind from the word the launch before left: its kind, the phase, who is alive, the sizes of the front it made.
//   DEGINIT  over all vertices: both degrees (row lengths minus self entries; a long row is counted by its wave), everybody alive
//   LIST     over all vertices: whoever has a degree of 0 leaves (label = own id) and is the first trim front
//   EXPAND   over a front of vertices that have left -- a trim front, the pivot's component, a round's components: one returning
//            decrement of indeg for every out-entry's target and of outdeg for every in-entry's source.  The decrement that returns
//            1 has emptied a counter: its thread claims the vertex (one CAS on the state: both counters may empty in one launch),
//            labels it and appends it to the next trim front.  An empty front: the phase's TRIM is over.
//   PMAX     over all vertices: the largest outdeg * indeg of an alive vertex (one atomicMax a wave)
//   PPICK    over all vertices: the smallest id that has it
//   RINIT    over all vertices: col = own id and everybody alive is the first sweep front (a round); or col = "none", the pivot
//            its own id and alone in the front (the pivot phase): from here on the pivot phase IS a round
//   FWD      over a front: col[u] = min(col[u], col[v]) over its out-entries to alive vertices; a target that was lowered joins the
//            next front.  An empty front: the fixpoint.
//   ROOTS    over all vertices: alive with col[v] == v: claimed, and the first backward front
//   BWD      over a front of claimed vertices u: every alive source v of an in-entry with col[v] == col[u] is claimed and joins the
//            next front.  An empty front: the fixpoint.
//   SEAL     over all vertices: the claimed ones get their label (col; the pivot phase: the minimum BWD kept), leave, and are the
//            front the next EXPAND takes the degrees down for
//   DONE
// A front is two lists: every vertex of it once in `rows` (a lane each walks whichever of its rows has fewer than `long_min`
// entries), and each row of at least long_min entries as (vertex, segment) items of `seg` entries, a wave each -- an out-row names
// its vertex as v, an in-row as ~v.  Appends go through wave-private LDS stages behind one returning add each (worklist.hpp).  A
// vertex is in a front at most once, so the lists have capacities that can be allocated: n, and the segments of m.
// The kernel's scalar registers are counted: what the run keeps per vertex sits in one record behind one pointer, the fronts'
// vertices behind the labels, and a launch reads the ring's words where it uses them.
//
// What holds between the workgroups of one launch (per-XCD L2s are not coherent, a CU's L1 is not refreshed; DESIGN 3.8 met the
// same):
//   (a) inside a FWD launch col changes by device-scope atomicMin only and only decreases; inside an EXPAND launch the degrees
//       change by returning atomicAdd only.
//   (b) nothing spins on a load.  A load of col may be as old as the launch's start: it is then larger than the truth, the
//       atomicMin it feeds lowers less than it could, and (c) brings the rest.
//   (c) no lowering is lost: the thread whose atomicMin returned more than it wrote puts the target into the NEXT launch's front,
//       exactly once -- stamp[u] holds the number of the last launch that listed u, taken with atomicExch, so nothing is cleared.  A
//       vertex lowered while it is itself being expanded is listed by whoever lowered it and runs again in the next launch.  BWD
//       claims with the same exchange on the same array; its stamp is the ROOTS launch's number, which no FWD launch of any round
//       shares.
//   (d) a vertex whose two counters both reach zero in one EXPAND is removed once: atomicCAS(state, ALIVE, REMOVED) has one winner.
//   (e) states change in LIST, EXPAND and SEAL only.  LIST and SEAL touch the state of the thread's own vertex; EXPAND reads no
//       state at all (its CAS is its only access).  FWD and BWD read states and write none: "after all of this pass's reads and
//       before the next pass's" is a launch boundary.
// No cooperative launch, no grid-wide barrier, no inline assembly; every device loop is bounded by a size read once.
// Not built: kcore's MINI kind (a ring of L vertices costs about L launches a phase without it), the pivot's two
// reaches through the fused BFS engine, trim-2, more than one device.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "cc_fused.hpp"
#include "env.hpp"
#include "launch_chain.hpp"
#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

// (both defaults are unmeasured guesses until tools/scc_bench.py has swept them on the device)
constexpr int SCC_LONG_MIN_DEFAULT = 32;    // rows of at least this many entries are long
constexpr int SCC_SEG_DEFAULT = 256;        // entries of a long row one wave takes
constexpr int SCC_STAGE = 2 * WAVE;         // a wave's LDS stage of front vertices
constexpr int SCC_NONE = 0x7fffffff;        // col of a vertex the pivot has not reached

enum scc_kind_t : int {
  SCC_INIT = 0, SCC_DEGINIT = 1, SCC_LIST = 2, SCC_EXPAND = 3, SCC_PMAX = 4, SCC_PPICK = 5, SCC_RINIT = 6, SCC_FWD = 7, SCC_ROOTS = 8,
  SCC_BWD = 9, SCC_SEAL = 10, SCC_DONE = 11
};
enum : int { SCC_ALIVE = 0, SCC_REMOVED = 1 };
enum : int { SCC_PH_TRIM0 = 0, SCC_PH_PIVOT = 1, SCC_PH_ROUNDS = 2 };     // the first TRIM, the pivot phase, the rounds
enum : int { SCC_OUT = 1, SCC_IN = 2 };                                   // the rows of a front vertex its consumer walks
enum : int { SCC_T_INIT = 0, SCC_T_TRIM = 1, SCC_T_PIVOT = 2, SCC_T_ROUNDS = 3 };

struct scc_opts_t {
  int long_min = SCC_LONG_MIN_DEFAULT, seg = SCC_SEG_DEFAULT;
  static scc_opts_t from_env() {
    scc_opts_t o;
    o.long_min = env_int("MGX_SCC_LONG_MIN", 1, INT_MAX, o.long_min);
    o.seg = env_int("MGX_SCC_SEG", 1, INT_MAX, o.seg);
    return o;
  }
};

// what a launch leaves for the next one (cleared two launches ahead)
struct scc_word_t {
  u64 best;        // PMAX: the largest outdeg * indeg of an alive vertex (alive vertices have both above 0 when it runs)
  int kind;        // what the launch was
  int phase;       // SCC_PH_*
  int alive;       // alive vertices when the launch began
  int tag;         // the stamp of the claimed (ROOTS sets it: its launch number + 1)
  int pivot_enc;   // PPICK: INT_MAX - (the smallest id at `best`)
  int n_rows;      // the front the launch made: its vertices,
  int n_items;     //   and the (vertex, segment) items of its long rows
  int streak;      // launches of this kind in a row, this one included
};

struct scc_totals_t {
  long long trimmed, pivot_size, rounds;
  chain_clock_t<4> timed;      // wall clock ticks per SCC_T_* (timed runs)
  int pivot_min;               // the smallest id BWD has claimed in the pivot phase
  int done;                    // bit 0: the run is over; bit 1: a fixpoint did not end and the host ends the run (a bug: `streak` in k_scc_step)
};

using scc_control_t = chain_control_t<scc_word_t, scc_totals_t>;

// what the run keeps per vertex, in one place: a sweep that meets u looks at its state, colour and stamp together
struct alignas(32) scc_vertex_t {
  int outdeg, indeg;   // entries to / from alive vertices other than itself
  int state;           // SCC_ALIVE, SCC_REMOVED
  int col;
  int stamp;           // the number + 1 of the last launch that listed it (FWD), or the tag of the claimed (ROOTS, BWD)
  int pad[3];
};

struct scc_step_args_t {
  const int* ro;   // CSR
  const int* ci;
  const int* co;   // the genuine CSC
  const int* ri;
  scc_vertex_t* vert;
  int* label;      // max(n, 1) labels, and behind them 2 x max(n, 1): the fronts' vertices, by launch parity
  int2* items;     // 2 x item_cap: the fronts' long rows, by launch parity
  scc_control_t* ctl;
  int n, item_cap, long_min, seg, timing;
  // the lists' halves, by launch parity
  __device__ __forceinline__ int* out_rows(unsigned half) const { return label + (half ? 2 * (size_t)max(n, 1) : (size_t)max(n, 1)); }
  __device__ __forceinline__ int2* out_items(unsigned half) const { return items + (half ? (size_t)item_cap : (size_t)0); }
};

// A wave's share of the front being made: its vertices wait in `stage`, those with a long row behind them -- an out-row as v, an
// in-row as ~v, which is also how the items name their vertex; each stage goes out behind one returning add, a long row as its
// segments' items.
struct scc_front_t {
  int* stage;          // SCC_STAGE vertices, behind them WAVE long rows
  scc_word_t* next;
  unsigned to;         // where they go: the lists' half of the next launch's parity
  int n_rows = 0, n_hubs = 0;
  __device__ __forceinline__ int* hubs() const { return stage + SCC_STAGE; }
};
__device__ __forceinline__ void scc_flush_hubs(const scc_step_args_t& a, scc_front_t& f) {
  if (f.n_hubs == 0) return;
  wave_lds_fence();
  const bool has = lane_id() < f.n_hubs;
  const int x = has ? f.hubs()[lane_id()] : 0;
  const int v = x >= 0 ? x : ~x;
  const int* const off = x >= 0 ? a.ro : a.co;
  const int len = has ? off[v + 1] - off[v] : 0;
  wave_append_segments(has, x, len, a.seg, a.out_items(f.to), &f.next->n_items);
  wave_lds_fence();
  f.n_hubs = 0;
}
__device__ __forceinline__ void scc_push_hubs(const scc_step_args_t& a, scc_front_t& f, bool take, int x) {
  const u64 m = __ballot(take);
  if (!m) return;
  const int c = __popcll(m);
  if (f.n_hubs + c > WAVE) scc_flush_hubs(a, f);
  if (take) f.hubs()[f.n_hubs + rank_in_mask(m)] = x;
  f.n_hubs += c;
}
// a wave's vertices for the next front (at most one a lane; all lanes call), whose consumer walks the rows of `sides`
__device__ __forceinline__ void scc_enlist(const scc_step_args_t& a, scc_front_t& f, bool take, int v, int sides) {
  if (!__ballot(take)) return;
  wave_stage_push<SCC_STAGE>(take, v, f.stage, f.n_rows, a.out_rows(f.to), &f.next->n_rows);
  if (sides & SCC_OUT) scc_push_hubs(a, f, take && a.ro[v + 1] - a.ro[v] >= a.long_min, v);
  if (sides & SCC_IN) scc_push_hubs(a, f, take && a.co[v + 1] - a.co[v] >= a.long_min, ~v);
}
__device__ __forceinline__ void scc_flush_front(const scc_step_args_t& a, scc_front_t& f) {
  wave_stage_flush(f.stage, f.n_rows, a.out_rows(f.to), &f.next->n_rows);
  scc_flush_hubs(a, f);
}

// what a sweep launch does with one entry; all lanes call, `has`: the lane holds an entry, of front vertex v (whose colour is c)
// naming u.  out_side: the entry is v -> u, else u -> v.
struct scc_visit_t {
  int stamp, pivot_phase;
};
template <int KIND>
__device__ __forceinline__ void scc_visit(const scc_step_args_t& a, scc_front_t& f, const scc_visit_t& w, bool out_side, bool has, int v, int c, int u) {
  bool take = has && u != v;
  if (KIND == SCC_EXPAND) {
    if (take) take = atomicAdd(out_side ? &a.vert[u].indeg : &a.vert[u].outdeg, -1) == 1;
    if (take) take = atomicCAS(&a.vert[u].state, (int)SCC_ALIVE, (int)SCC_REMOVED) == SCC_ALIVE;
    if (take) a.label[u] = u;
    scc_enlist(a, f, take, u, SCC_OUT | SCC_IN);
  } else if (KIND == SCC_FWD) {
    take = take && a.vert[u].state == SCC_ALIVE && a.vert[u].col > c;
    if (take) take = atomicMin(&a.vert[u].col, c) > c;
    if (take) take = atomicExch(&a.vert[u].stamp, w.stamp) != w.stamp;
    scc_enlist(a, f, take, u, SCC_OUT);
  } else {                                                   // BWD
    take = take && a.vert[u].state == SCC_ALIVE && a.vert[u].col == c && a.vert[u].stamp != w.stamp;
    if (take) take = atomicExch(&a.vert[u].stamp, w.stamp) != w.stamp;
    if (w.pivot_phase && __ballot(take)) {
      int lowest = take ? u : SCC_NONE;
      lowest = wave_min(lowest);
      if (lane_id() == 0) atomicMin(&a.ctl->totals.pivot_min, lowest);
    }
    scc_enlist(a, f, take, u, SCC_IN);
  }
}

// a sweep over a front: the long rows' items (a wave each), then the front's vertices (a lane each, the wave walking in step
// whichever of their rows are short): EXPAND walks both rows of a vertex, FWD its out-row, BWD its in-row
template <int KIND>
__device__ __forceinline__ void scc_sweep(const scc_step_args_t& a, scc_front_t& f, const scc_visit_t& w, int n_rows, int n_items, int wave, int waves) {
  const int lane = lane_id();
  const int2* const front_items = a.out_items(f.to ^ 1);
  for (int it = wave; it < n_items; it += waves) {
    const int2 item = front_items[it];
    const bool out_side = item.x >= 0;
    const int v = out_side ? item.x : ~item.x;
    const int* const off = out_side ? a.ro : a.co;
    const int* const adj = out_side ? a.ci : a.ri;
    const int c = KIND == SCC_EXPAND ? 0 : a.vert[v].col;
    const long long s0 = (long long)off[v] + (long long)item.y * a.seg;
    const int s1 = (int)min((long long)off[v + 1], s0 + a.seg);
    for (int base = (int)s0; base < s1; base += WAVE) {
      const bool has = base + lane < s1;
      scc_visit<KIND>(a, f, w, out_side, has, v, c, has ? adj[base + lane] : 0);
    }
  }
  const int* const front_rows = a.out_rows(f.to ^ 1);
  for (int side = (KIND == SCC_BWD ? 1 : 0); side <= (KIND == SCC_FWD ? 0 : 1); ++side) {
    const bool out_side = side == 0;
    const int* const off = out_side ? a.ro : a.co;
    const int* const adj = out_side ? a.ci : a.ri;
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)n_rows; base += (unsigned)waves * WAVE) {
      const unsigned i = base + lane;
      const bool in = i < (unsigned)n_rows;
      const int v = in ? front_rows[i] : 0;
      const int beg = in ? off[v] : 0;
      int len = in ? off[v + 1] - beg : 0;
      if (len >= a.long_min) len = 0;                        // (its items are walked above)
      const int c = (in && KIND != SCC_EXPAND) ? a.vert[v].col : 0;
      int longest = len;
      longest = wave_max(longest);
      for (int j = 0; j < longest; ++j) {
        const bool has = j < len;
        scc_visit<KIND>(a, f, w, out_side, has, v, c, has ? adj[beg + j] : 0);
      }
    }
  }
}

// entries of rows [beg, end) of `adj` that name v, for the lanes of a wave at once (all lanes call; `valid`: the lane has a row):
// a short row is counted by its lane, a long one by the whole wave
__device__ __forceinline__ int scc_self_entries(const int* adj, bool valid, int v, int beg, int end, int long_min) {
  const int lane = lane_id();
  const bool is_long = valid && end - beg >= long_min;
  int self = 0;
  if (valid && !is_long)
    for (int e = beg; e < end; ++e) self += adj[e] == v ? 1 : 0;
  u64 lm = __ballot(is_long);
  while (lm) {
    const int src = __ffsll((long long)lm) - 1;
    lm &= lm - 1;
    const int vv = __shfl(v, src, WAVE), b = __shfl(beg, src, WAVE), e = __shfl(end, src, WAVE);
    int cnt = 0;
    for (int j = b + lane; j < e; j += WAVE) cnt += adj[j] == vv ? 1 : 0;
    cnt = wave_sum(cnt);
    if (lane == src) self = cnt;
  }
  return self;
}

__device__ __forceinline__ int scc_clock_of(int kind, int phase) {
  if (kind == SCC_DEGINIT) return SCC_T_INIT;
  if (kind == SCC_LIST || kind == SCC_EXPAND) return SCC_T_TRIM;
  return (kind == SCC_PMAX || kind == SCC_PPICK || phase == SCC_PH_PIVOT) ? SCC_T_PIVOT : SCC_T_ROUNDS;
}

// launch: the launch's number in the run
__global__ __launch_bounds__(BLOCK) void k_scc_step(scc_step_args_t a, unsigned launch) {
  const scc_word_t prev = a.ctl->left_by_prev(launch);
  scc_word_t* const next = a.ctl->for_next(launch);
  const unsigned gtid = blockIdx.x * (unsigned)BLOCK + threadIdx.x;
  const unsigned gthreads = gridDim.x * (unsigned)BLOCK;
  const bool first_thread = gtid == 0;
  if (first_thread) a.ctl->clear_ahead(launch);

  // what this launch is, from what the one before it left
  const bool removing = prev.kind == SCC_LIST || prev.kind == SCC_EXPAND || prev.kind == SCC_SEAL;     // (its front is who left)
  const int alive = prev.kind == SCC_INIT ? a.n : (removing ? prev.alive - prev.n_rows : prev.alive);
  const bool front = prev.n_rows > 0;
  int kind, phase = prev.phase;
  switch (prev.kind) {
    case SCC_INIT: kind = SCC_DEGINIT; break;
    case SCC_DEGINIT: kind = SCC_LIST; break;
    case SCC_LIST:
    case SCC_EXPAND:
      if (front) kind = SCC_EXPAND;
      else if (alive == 0) kind = SCC_DONE;
      else if (phase == SCC_PH_TRIM0) { kind = SCC_PMAX; phase = SCC_PH_PIVOT; }
      else { kind = SCC_RINIT; phase = SCC_PH_ROUNDS; }
      break;
    case SCC_PMAX: kind = SCC_PPICK; break;
    case SCC_PPICK: kind = SCC_RINIT; break;
    case SCC_RINIT: kind = SCC_FWD; break;
    case SCC_FWD: kind = front ? SCC_FWD : SCC_ROOTS; break;
    case SCC_ROOTS: kind = SCC_BWD; break;
    case SCC_BWD: kind = front ? SCC_BWD : SCC_SEAL; break;
    case SCC_SEAL: kind = SCC_EXPAND; break;
    default: kind = SCC_DONE; break;
  }
  const int tag = kind == SCC_ROOTS ? (int)(launch + 1) : prev.tag;
  const bool pivot_phase = phase == SCC_PH_PIVOT;
  if (first_thread) {
    next->kind = kind;
    next->phase = phase;
    next->alive = alive;
    next->tag = tag;
    // A fixpoint ends within n + 1 launches: a trim front or a backward front that is not empty holds a vertex no earlier front
    // held, and a forward sweep's launch k has every colour that travels over at most k arcs where it belongs (a load is at least
    // as new as the launch's start), so launch n lowers nobody.  A chain of one kind longer than that is a bug in this file: bit 1
    // of done tells the host, which ends the run at its next wait -- no count of ALL launches could tell, a ring takes as many as it
    // has vertices.
    const int streak = kind == prev.kind ? prev.streak + 1 : 1;
    next->streak = streak;
    scc_totals_t& t = a.ctl->totals;
    if (kind != SCC_DONE && streak > a.n + 2) t.done |= 2;
    a.ctl->log_kind(launch, kind);
    if (prev.kind == SCC_LIST || prev.kind == SCC_EXPAND) t.trimmed += prev.n_rows;
    if (prev.kind == SCC_SEAL && prev.phase == SCC_PH_PIVOT) t.pivot_size = prev.n_rows;
    if (kind == SCC_RINIT && !pivot_phase) t.rounds += 1;
    if (kind == SCC_RINIT && pivot_phase) t.pivot_min = 0x7fffffff - prev.pivot_enc;      // (PPICK left the pivot)
    t.timed.tick(a.timing, prev.kind, SCC_DONE, scc_clock_of(prev.kind, prev.phase));
    if (kind == SCC_DONE) t.done |= 1;
  }
  if (kind == SCC_DONE) return;

  const int lane = lane_id();
  const int wave = (int)(gtid / WAVE);
  const int waves = (int)(gthreads / WAVE);
  __shared__ int stages[WAVES_PER_BLOCK][SCC_STAGE + WAVE];
  const unsigned from = launch & 1;                           // the lists' halves: the launch before filled `from`, this one fills the other
  scc_front_t f;
  f.stage = stages[threadIdx.x / WAVE];
  f.next = next;
  f.to = from ^ 1;

  // the kinds that run over all vertices, a wave over 64 consecutive ones at a time
  if (kind == SCC_DEGINIT) {
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)a.n; base += (unsigned)waves * WAVE) {
      const bool in = base + lane < (unsigned)a.n;
      const int v = (int)(base + lane);
      const int ob = in ? a.ro[v] : 0, oe = in ? a.ro[v + 1] : 0;
      const int ib = in ? a.co[v] : 0, ie = in ? a.co[v + 1] : 0;
      const int so = scc_self_entries(a.ci, in, v, ob, oe, a.long_min);
      const int si = scc_self_entries(a.ri, in, v, ib, ie, a.long_min);
      if (in) {
        a.vert[v].outdeg = oe - ob - so;
        a.vert[v].indeg = ie - ib - si;
        a.vert[v].state = SCC_ALIVE;
        a.vert[v].stamp = 0;
      }
    }
    return;
  }
  if (kind == SCC_PMAX || kind == SCC_PPICK) {
    // PMAX: the largest product; PPICK: INT_MAX - (the smallest id that has it), so that a cleared word says "nobody"
    const u64 at_best = a.ctl->left_by_prev_at(launch)->best;         // (read here, not kept from the launch's start: the scalar registers are counted)
    u64 best = 0;
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)a.n; base += (unsigned)waves * WAVE) {
      const int v = (int)(base + lane);
      if (base + lane >= (unsigned)a.n || a.vert[v].state != SCC_ALIVE) continue;
      const u64 prod = (u64)(unsigned)a.vert[v].outdeg * (u64)(unsigned)a.vert[v].indeg;
      if (kind == SCC_PMAX) best = max(best, prod);
      else if (prod == at_best) best = max(best, (u64)(0x7fffffff - v));
    }
    best = wave_max(best);
    if (lane == 0 && best > 0) {
      if (kind == SCC_PMAX) {
        if (__hip_atomic_load(&next->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < best) atomicMax(&next->best, best);
      } else if (__hip_atomic_load(&next->pivot_enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (int)best) {
        atomicMax(&next->pivot_enc, (int)best);
      }
    }
    return;
  }
  if (kind == SCC_LIST || kind == SCC_RINIT || kind == SCC_ROOTS || kind == SCC_SEAL) {
    // who joins the front, and which of its rows the front's consumer walks
    const int sides = kind == SCC_RINIT ? SCC_OUT : (kind == SCC_ROOTS ? SCC_IN : (SCC_OUT | SCC_IN));
    const int pivot_label = (kind == SCC_SEAL && pivot_phase) ? a.ctl->totals.pivot_min : -1;
    const int pivot = 0x7fffffff - a.ctl->left_by_prev_at(launch)->pivot_enc;     // (RINIT of the pivot phase: PPICK left it; read here, as at_best is)
    for (unsigned base = (unsigned)wave * WAVE; base < (unsigned)a.n; base += (unsigned)waves * WAVE) {
      const int v = (int)(base + lane);
      const bool is_alive = base + lane < (unsigned)a.n && a.vert[v].state == SCC_ALIVE;
      bool take = false;
      if (is_alive) {
        scc_vertex_t& x = a.vert[v];
        if (kind == SCC_LIST) {
          take = x.outdeg == 0 || x.indeg == 0;
          if (take) { x.state = SCC_REMOVED; a.label[v] = v; }
        } else if (kind == SCC_RINIT) {
          take = !pivot_phase || v == pivot;
          x.col = take ? v : SCC_NONE;
        } else if (kind == SCC_ROOTS) {
          take = x.col == v;
          if (take) x.stamp = tag;
        } else {                                               // SEAL
          take = x.stamp == tag;
          if (take) { x.state = SCC_REMOVED; a.label[v] = pivot_label >= 0 ? pivot_label : x.col; }
        }
      }
      scc_enlist(a, f, take, v, sides);
    }
    scc_flush_front(a, f);
    return;
  }
  {                                                          // EXPAND, FWD, BWD: over the front the launch before made
    const scc_word_t* const made = a.ctl->left_by_prev_at(launch);  // (the front's sizes are read here: the scalar registers are counted)
    const int n_rows = made->n_rows, n_items = made->n_items;
    scc_visit_t w;
    w.stamp = kind == SCC_BWD ? tag : (int)(launch + 1);
    w.pivot_phase = pivot_phase ? 1 : 0;
    if (kind == SCC_EXPAND) scc_sweep<SCC_EXPAND>(a, f, w, n_rows, n_items, wave, waves);
    else if (kind == SCC_FWD) scc_sweep<SCC_FWD>(a, f, w, n_rows, n_items, wave, waves);
    else scc_sweep<SCC_BWD>(a, f, w, n_rows, n_items, wave, waves);
    scc_flush_front(a, f);
  }
}

// The device state of a graph's fused SCC, and the run (host side).  Everything a run needs is allocated here: a second run
// allocates nothing.
struct scc_fused_state_t {
  int n = 0;
  scc_opts_t opts;
  mem_t<scc_vertex_t> vert;
  mem_t<int> label;                            // the labels | both halves of the fronts' vertices
  mem_t<int2> items;
  int item_cap = 0;
  mem_t<scc_control_t> ctl;
  pinned_t<scc_totals_t> h_totals;
  cc_label_stats_t label_stats;
  long long launches = -1;                     // of the last run, the idle ones behind its end included (-1: no run yet)
  bool timing = false;                         // mgx_scc_set_timing: the launches keep the device's wall clock per phase
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the last timed run: init, trim, pivot, rounds

  scc_fused_state_t(int n_, long long m, context_t& ctx) : n(n_), opts(scc_opts_t::from_env()), label_stats(n_, ctx) {
    const size_t N = (size_t)std::max(n, 1);
    vert = mem_t<scc_vertex_t>(N, ctx);
    label = mem_t<int>(3 * N, ctx);
    // long rows, per side: at most min(n, m / long_min) of them, and one item per `seg` entries beyond their first segment
    const long long cap = 2 * (std::min<long long>((long long)N, m / opts.long_min + 1) + m / opts.seg + 1);
    if (cap > 0x3fffffff) throw mgx_error(MGX_E_INVALID, "mgx scc: MGX_SCC_SEG is too small for this graph");
    item_cap = (int)cap;
    items = mem_t<int2>(2 * (size_t)item_cap, ctx);
    ctl = mem_t<scc_control_t>(1, ctx);
    h_totals = pinned_t<scc_totals_t>(1);
  }

  // Label the graph (ro, ci: the CSR on the device; co, ri: its genuine CSC).  Returns {components, largest, its label, trimmed,
  // the pivot's component, rounds, host waits, launches}.
  std::vector<long long> run(const int* ro, const int* ci, const int* co, const int* ri, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    launches = -1;                                           // (a run that throws leaves no launches to ask about)
    if (n <= 0) {
      launches = 0;
      return {0, 0, 0, 0, 0, 0, 0, 0};
    }
    scc_control_t::reset(ctl.data(), st);
    scc_step_args_t a;
    a.ro = ro; a.ci = ci; a.co = co; a.ri = ri;
    a.vert = vert.data(); a.label = label.data(); a.items = items.data();
    a.ctl = ctl.data(); a.n = n; a.item_cap = item_cap; a.long_min = opts.long_min; a.seg = opts.seg; a.timing = timing ? 1 : 0;
    const int blocks = grid_for(n, BLOCK, std::max(ctx.num_cus, 1) * 4);
    long long waits = 0;
    // The device reports a fixpoint that does not end (bit 1 of done, after n + 2 launches of one kind).  The count below only keeps
    // the stamps, launch numbers + 1, inside an int: it is hours of launches away and catches nothing early.
    const long long most = 0x7fff0000ll;
    const long long enqueued = run_launch_chain(
        [&](long long i) { hipLaunchKernelGGL(k_scc_step, dim3(blocks), dim3(BLOCK), 0, st, a, (unsigned)i); },
        [&]() {
          h_totals.fetch(&ctl.data()->totals, 1, st);
          if (h_totals->done & 2) throw mgx_error(MGX_E_HIP, "mgx scc: a fixpoint did not end within n + 2 launches");
          return h_totals->done != 0;
        },
        most, "mgx scc step", &waits);
    if (timing)
      for (int i = 0; i < 4; ++i) phase_ms[i] = chain_ticks_ms(h_totals->timed.clock[i]);
    const std::vector<long long> ls = label_stats.run(label.data(), n, ctx);      // (the stats CC reports, by CC's kernels)
    ++waits;
    launches = enqueued;
    return {ls[0], ls[1], ls[2], h_totals->trimmed, h_totals->pivot_size, h_totals->rounds, waits, launches};
  }
};

}  // namespace mgx
