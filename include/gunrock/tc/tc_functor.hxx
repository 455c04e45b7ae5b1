// gunrock/tc/tc_functor.hxx -- the device functor of the triangle count's operator path.
//   cond_advance(a, b)   the advance over every DAG entry (a, b): one thread intersects the sorted rows a and b (the fused path's
//                        own per-thread intersection, mgx::tc_intersect: the shorter row's entries searched in the longer) and
//                        does the fused path's adds: tri[w] += 1 per common element w, tri[a] += c, tri[b] += c.  It says
//                        whether the entry closed a triangle; the advance writes no output.
// Integer adds commute: the counts do not depend on the order the entries run in.
#pragma once
#include "../../mgx/tc_fused.hpp"
#include "../intrinsics.hxx"
#include "tc_problem.hxx"

namespace gunrock {
namespace tc {

typedef tc_problem_t::data_slice_t tc_slice_t;

struct tc_functor_t {
  static __device__ __forceinline__ bool cond_advance(int a, int b, int, int, int, tc_slice_t* d, int) {
    const int* const ro = d->d_row_offsets;
    const int ra = ro[a], rb = ro[b];
    const int c = mgx::tc_intersect(d->d_col_indices, ra, ro[a + 1] - ra, rb, ro[b + 1] - rb, d->d_tri);
    if (c) {
      mgx::tc_add(d->d_tri + a, (mgx::u64)c);
      mgx::tc_add(d->d_tri + b, (mgx::u64)c);
    }
    return c > 0;
  }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, tc_slice_t*, int) { return true; }
};

}  // namespace tc
}  // namespace gunrock
