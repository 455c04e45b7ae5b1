// gunrock/lspar/lspar_functor.hxx -- the device functors of the sparsification's operator path (the reference's
// gunrock/src/lspar/lspar_functor.hxx, same names).
//   minhash_functor_t   the neighbourhood reduce's value: the vertex's hash (bit 31 flipped); a pure gather (mgx_pure_gather),
//                       so the iota frontier on a graph with the layout takes the library's one-pass reduce
//   sim_functor_t       per entry: {eid, sim} with sim = the number of equal minhash columns of the two ends
//   select_functor_t    per entry of the sorted records: rank in the row < t(src)
#pragma once
#include "../intrinsics.hxx"
#include "lspar_problem.hxx"

namespace gunrock {
namespace lspar {

typedef lspar_problem_t::data_slice_t lspar_slice_t;

struct minhash_functor_t {
  static constexpr bool mgx_pure_gather = true;
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, lspar_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, lspar_slice_t*, int) { return true; }
  static __device__ __forceinline__ int get_value_to_reduce(int v, lspar_slice_t* d, int) { return d->d_hashs[v]; }
};

struct sim_functor_t {
  static __device__ __forceinline__ bool cond_advance(int src, int dst, int edge_id, int, int output_idx, lspar_slice_t* d, int) {
    const int k = d->num_hashs;
    const unsigned* const a = d->d_minwise_hashs + (size_t)src * k;
    const unsigned* const b = d->d_minwise_hashs + (size_t)dst * k;
    int sim = 0;
    for (int j = 0; j < k; ++j) sim += a[j] == b[j];
    d->d_sims[output_idx].sim = (float)sim;
    d->d_sims[output_idx].eid = edge_id;
    return sim > 0;
  }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, lspar_slice_t*, int) { return true; }
};

struct select_functor_t {
  static __device__ __forceinline__ bool cond_advance(int src, int, int, int rank, int, lspar_slice_t* d, int) {
    return rank < d->d_thresholds[src];
  }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, lspar_slice_t*, int) { return true; }
};

}  // namespace lspar
}  // namespace gunrock
