// gunrock/pagerank/pagerank_functor.hxx -- the device functor of PageRank's operator path: what a neighbour adds to a vertex's
// sum is its contribution r / d, a pure read (mgx_pure_gather: the operator may take it once per vertex, neighborhood.hxx).
#pragma once
#include "../intrinsics.hxx"
#include "pagerank_problem.hxx"

namespace gunrock {
namespace pagerank {

struct pagerank_functor_t {
  using slice_t = pagerank_problem_t::data_slice_t;
  static constexpr bool mgx_pure_gather = true;

  static __device__ __forceinline__ float get_value_to_reduce(int v, slice_t* d, int) { return d->d_contrib[v]; }
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, slice_t*, int) { return true; }
};

}  // namespace pagerank
}  // namespace gunrock
