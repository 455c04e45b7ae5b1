// gunrock/coloring/coloring_functor.hxx -- the device functors of the colouring's operator path (the reference's
// gunrock/src/coloring/coloring_functor.hxx, same names).
//   reduce_max_t / reduce_min_t   the neighbourhood reduce's value: an uncoloured vertex's key, a coloured one the identity;
//                                 pure gathers (mgx_pure_gather), so a full frontier on a graph with the layout takes the
//                                 library's one-pass reduce
//   coloring_functor_t            the filter over the active vertices: key <= min of the uncoloured neighbours -> 2i + 1,
//                                 else key >= max -> 2i + 2, else the vertex stays active.  `<=` / `>=`, not the reference's
//                                 strict tests: keys are distinct, so they mean "below / above every OTHER uncoloured
//                                 neighbour" and a self-loop changes nothing (the reference never colours such a vertex)
#pragma once
#include <climits>

#include "../intrinsics.hxx"
#include "coloring_problem.hxx"

namespace gunrock {
namespace coloring {

typedef coloring_problem_t::data_slice_t coloring_slice_t;

struct coloring_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, coloring_slice_t* d, int iteration) {
    const int hash = d->d_hashs[v];
    int color = 0;
    if (hash <= d->d_reduced_min[v]) color = 2 * iteration + 1;
    else if (hash >= d->d_reduced_max[v]) color = 2 * iteration + 2;
    if (color) d->d_colors[v] = color;
    return color == 0;
  }
};

struct reduce_max_t {
  static constexpr bool mgx_pure_gather = true;
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, coloring_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, coloring_slice_t*, int) { return true; }
  static __device__ __forceinline__ int get_value_to_reduce(int v, coloring_slice_t* d, int) {
    return d->d_colors[v] == 0 ? d->d_hashs[v] : INT_MIN;
  }
};

struct reduce_min_t {
  static constexpr bool mgx_pure_gather = true;
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, coloring_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, coloring_slice_t*, int) { return true; }
  static __device__ __forceinline__ int get_value_to_reduce(int v, coloring_slice_t* d, int) {
    return d->d_colors[v] == 0 ? d->d_hashs[v] : INT_MAX;
  }
};

}  // namespace coloring
}  // namespace gunrock
