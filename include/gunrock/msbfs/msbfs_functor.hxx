// gunrock/msbfs/msbfs_functor.hxx -- the device functors of the multi-source BFS's operator path.  What the
// operators' `iteration` argument carries is said per functor.
//   expand_functor_t      iteration = t, the advance over every out-entry (v, u) of the front's vertices: the bits of front_t[v]
//                         that u has not seen are ORed into next[u]; the entry passes u on when it changed bits there
//   finalize_functor_t    iteration = d = t + 1, the filter behind it: the first slot that names u takes next[u] (one exchange: the
//                         dedup), new = next & ~seen, seen |= new, front_d[u] = new, the per-vertex sums, the depth stores and one
//                         add per new bit to the level's counts; kept: the vertices of the new front, once each
//   clear_functor_t       iteration = t, over the old front: front_t[v] = 0 (its half is written again at level t + 2)
#pragma once
#include "../intrinsics.hxx"
#include "msbfs_problem.hxx"

namespace gunrock {
namespace msbfs {

typedef msbfs_problem_t::data_slice_t msbfs_slice_t;

struct expand_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, msbfs_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int, int, int, msbfs_slice_t* d, int t) {
    const unsigned long long bits = d->d_front[(size_t)(t & 1) * (size_t)d->n + v] & ~d->d_seen[u];
    if (!bits) return false;
    return (atomicOr(d->d_next + u, bits) & bits) != bits;
  }
};

struct finalize_functor_t {
  static __device__ __forceinline__ bool cond_filter(int u, msbfs_slice_t* d, int depth) {
    if (u < 0) return false;
    const unsigned long long nx = atomicExch(d->d_next + u, 0ull);
    if (!nx) return false;                                     // (another slot of the frontier has taken it)
    const unsigned long long sn = d->d_seen[u];
    unsigned long long nw = nx & ~sn;
    if (!nw) return false;
    d->d_seen[u] = sn | nw;
    d->d_front[(size_t)(depth & 1) * (size_t)d->n + u] = nw;
    const long long pc = __popcll(nw);
    d->d_reach_in[u] += pc;
    d->d_far_in[u] += pc * depth;
    const size_t first = (size_t)d->d_scalars->batch * 64;
    while (nw) {
      const int b = __ffsll((long long)nw) - 1;
      nw &= nw - 1;
      atomicAdd(d->d_cnt + b, 1ull);
      if (d->d_depth) d->d_depth[(first + (size_t)b) * (size_t)d->n + (size_t)u] = depth;
    }
    return true;
  }
};

struct clear_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, msbfs_slice_t* d, int t) {
    d->d_front[(size_t)(t & 1) * (size_t)d->n + v] = 0;
    return false;
  }
};

}  // namespace msbfs
}  // namespace gunrock
