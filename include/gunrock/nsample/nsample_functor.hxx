// gunrock/nsample/nsample_functor.hxx -- the device functors of the neighbour sampling's operator path.
//   sample_functor_t   iteration = the hop, the filter over the frontier, a lane per row: the row's entries by the fused path's own
//                      keys and draws (mgx::ns_row_key, rw_draw, rw_index); Floyd's membership test reads the row's earlier picks
//                      back from entry_pos, k (k - 1) / 2 reads a row; every destination without a local id is marked.  Nothing
//                      is kept: the filter's count is the hop's host wait
//   fresh_functor_t    the filter over all vertices: kept are the marked ones without a local id, ascending -- the next frontier
#pragma once
#include "../intrinsics.hxx"
#include "nsample_problem.hxx"

namespace gunrock {
namespace nsample {

typedef nsample_problem_t::data_slice_t nsample_slice_t;

struct sample_functor_t {
  static __device__ __forceinline__ void emit(nsample_slice_t* d, int e, int pos) {
    const int dst = d->ci[pos];
    d->d_entry_pos[e] = pos;
    d->d_cols[e] = dst;
    if (d->d_local[dst] >= 0) atomicAdd(d->d_counters + mgx::NS_C_REVISITS, 1ull);
    else d->d_mark[dst] = 1;
  }
  static __device__ __forceinline__ bool cond_filter(int v, nsample_slice_t* d, int hop) {
    if (v < 0) return false;
    const int r = d->d_local[v];
    const int k = d->fanouts[hop];
    const int beg = d->ro[v];
    const int deg = d->ro[v + 1] - beg;
    const int off = d->d_edge_off[hop] + d->d_row_offsets[r];
    d->d_row_offsets[r] = off;
    if (deg == 0) {
      atomicAdd(d->d_counters + mgx::NS_C_EMPTY, 1ull);
      return false;
    }
    if (mgx::ns_whole(deg, k, d->replace)) {
      atomicAdd(d->d_counters + mgx::NS_C_WHOLE, 1ull);
      for (int e = 0; e < deg; ++e) emit(d, off + e, beg + e);
      return false;
    }
    atomicAdd(d->d_counters + mgx::NS_C_SAMPLED, 1ull);
    atomicAdd(d->d_counters + mgx::NS_C_DRAWS, (unsigned long long)k);
    const unsigned key = mgx::ns_row_key(d->seed, v, hop);
    unsigned collisions = 0;
    for (int j = 0; j < k; ++j) {
      int p;
      if (d->replace) {
        p = mgx::rw_index(mgx::rw_draw(key, (unsigned)j), deg);
      } else {
        const int i = deg - k + j;
        p = mgx::rw_index(mgx::rw_draw(key, (unsigned)j), i + 1);
        bool hit = false;
        for (int jj = 0; jj < j; ++jj) hit |= d->d_entry_pos[off + jj] == beg + p;
        if (hit) { p = i; ++collisions; }
      }
      emit(d, off + j, beg + p);
    }
    if (collisions) atomicAdd(d->d_counters + mgx::NS_C_COLLISIONS, (unsigned long long)collisions);
    return false;
  }
};

struct fresh_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, nsample_slice_t* d, int) { return v >= 0 && d->d_mark[v] != 0 && d->d_local[v] < 0; }
};

}  // namespace nsample
}  // namespace gunrock
