// gunrock/sim/sim_functor.hxx -- the device functor of the vertex similarity's operator path.
//   merge_functor_t   the filter over the pair indices, a thread per pair: a two-pointer merge of the two sorted rows counts the
//                     common neighbours, WEIGHTED adds x[w] in merge order; the score by the fused path's own sim_score.  Kept are
//                     the pairs with a common neighbour.
#pragma once
#include "../intrinsics.hxx"
#include "sim_problem.hxx"

namespace gunrock {
namespace sim {

typedef sim_problem_t::data_slice_t sim_slice_t;

struct merge_functor_t {
  static __device__ __forceinline__ bool cond_filter(int p, sim_slice_t* d, int) {
    if (p < 0) return false;
    const int u = d->u[p], v = d->v[p];
    if ((unsigned)u >= (unsigned)d->n || (unsigned)v >= (unsigned)d->n) {
      d->d_sums[1] = 1ull;
      return false;
    }
    int i = d->ro[u], j = d->ro[v];
    const int ie = d->ro[u + 1], je = d->ro[v + 1];
    const long long du = ie - i, dv = je - j;
    int c = 0;
    double s = 0.0;
    while (i < ie && j < je) {
      const int a = d->ci[i], b = d->ci[j];
      if (a == b) {
        ++c;
        if (d->x) s += d->x[a];
      }
      i += a <= b;
      j += b <= a;
    }
    d->d_common[p] = c;
    d->d_score[p] = d->x ? s : mgx::sim_score(d->measure, c, du, dv);
    if (c) atomicAdd(d->d_sums, (unsigned long long)c);
    return c > 0;
  }
};

}  // namespace sim
}  // namespace gunrock
