// mgx/row_bodies.hpp -- rows by length: how a fused path sorts the rows of a wave's 64 vertices into those a lane
// takes, those the wave takes one after the other, and those that go out as (vertex, segment) items (worklist.hpp:
// wave_append_segments).  Label propagation, Louvain, multi-source BFS and the random walks' setup share it; each keeps its own
// defaults, caps and switches.
#pragma once
#include "wave.hpp"

namespace mgx {

// the classes, and the places of their counts in every `bins` array (tests/row_bodies.py counts the same)
enum : int { ROW_NONE = 0, ROW_LANE = 1, ROW_WAVE = 2, ROW_LONG = 3 };

// the cuts: a row of at most short_max entries is a lane's, of at most wave_max a wave's, a longer one is cut into segments of
// seg entries.  wave_max < short_max leaves the wave nothing.
struct row_cuts_t {
  int short_max, wave_max, seg;
  __host__ __device__ __forceinline__ int body_of(int len) const {
    return len == 0 ? ROW_NONE : (len <= short_max ? ROW_LANE : (len <= wave_max ? ROW_WAVE : ROW_LONG));
  }
  __host__ __device__ __forceinline__ int segments_of(int len) const { return (len + seg - 1) / seg; }
};

// The rows of the lanes with `mine`, one after the other in ascending lane order: f(src) runs with all 64 lanes active and reads
// lane src's values with __shfl(x, src, WAVE).  All lanes call.
template <typename F>
__device__ __forceinline__ void for_each_wave_row(bool mine, F&& f) {
  u64 todo = __ballot(mine);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    f(src);
  }
}

// a vertex's out-row and behind it its in-row (both == false: the out-row alone, as of a symmetric graph)
struct row_pair_t {
  int ob, olen, ib, ilen;
  __device__ __forceinline__ int len() const { return olen + ilen; }
  __device__ __forceinline__ row_pair_t of_lane(int src) const {
    row_pair_t r;
    r.ob = __shfl(ob, src, WAVE); r.olen = __shfl(olen, src, WAVE);
    r.ib = __shfl(ib, src, WAVE); r.ilen = __shfl(ilen, src, WAVE);
    return r;
  }
};
__device__ __forceinline__ row_pair_t row_pair_of(const int* ro, const int* co, bool both, bool valid, int v) {
  row_pair_t r = {0, 0, 0, 0};
  if (valid) {
    r.ob = ro[v];
    r.olen = ro[v + 1] - r.ob;
    if (both) {
      r.ib = co[v];
      r.ilen = co[v + 1] - r.ib;
    }
  }
  return r;
}

// the rows a lane has seen per class.  count: any lane may call, a lane without a row passes a value outside 0 .. 3; add_to:
// all lanes call once, one add per wave and class that has rows
struct row_bins_t {
  int n[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void count(int body) {
#pragma unroll
    for (int b = 0; b < 4; ++b) n[b] += body == b ? 1 : 0;
  }
  __device__ __forceinline__ void add_to(long long* bins) const {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int s = wave_sum(n[b]);
      if (lane_id() == 0 && s) atomicAdd((u64*)&bins[b], (u64)s);
    }
  }
};

}  // namespace mgx
