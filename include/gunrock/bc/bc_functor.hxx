// gunrock/bc/bc_functor.hxx -- the device functors of the betweenness centrality's operator path: Brandes in its textbook GPU form.
//   bc_forward_functor_t    advance over the level-`iteration` frontier: an entry (src, dst) claims label[dst] with a CAS (-1 ->
//                           iteration + 1) and, whenever dst ends up one level deeper -- claimed by this entry or by another of this
//                           level --, adds sigma[src] to sigma[dst]: a double atomicAdd, exact while the sums stay below 2^53.  The
//                           claiming entry alone keeps its output slot; the filter drops the others.
//   bc_backward_functor_t   advance over the stored level-`iteration` frontier, no output: an entry (src, dst) with dst one level
//                           deeper adds sigma[src] / sigma[dst] * (1 + delta[dst]) to delta[src].
// The order of the float adds is the hardware's: delta differs in its last bits from run to run (the fused path's does not).
#pragma once
#include "bc_problem.hxx"

namespace gunrock {
namespace bc {

typedef bc_problem_t::data_slice_t bc_slice_t;

struct bc_forward_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int dst, int, int, int, bc_slice_t* d, int iteration) {
    const int l = d->d_labels[dst];
    return l == -1 || l == iteration + 1;
  }
  // (called for EVERY entry, whatever cond_advance said: advance.hxx)
  static __device__ __forceinline__ bool apply_advance(int src, int dst, int, int, int, bc_slice_t* d, int iteration) {
    int* const label = d->d_labels + dst;
    int l = *label;
    bool claimed = false;
    if (l == -1) {
      l = atomicCAS(label, -1, iteration + 1);
      claimed = l == -1;
    }
    if (claimed || l == iteration + 1) atomicAdd(d->d_sigma + dst, d->d_sigma[src]);
    return claimed;
  }
  static __device__ __forceinline__ bool cond_filter(int slot_value, bc_slice_t*, int) { return slot_value != -1; }
  static constexpr bool cond_filter_of_slot_value_only = true;
};

struct bc_backward_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int dst, int, int, int, bc_slice_t* d, int iteration) {
    return d->d_labels[dst] == iteration + 1;
  }
  static __device__ __forceinline__ bool apply_advance(int src, int dst, int, int, int, bc_slice_t* d, int iteration) {
    if (d->d_labels[dst] == iteration + 1) atomicAdd(d->d_delta + src, d->d_sigma[src] / d->d_sigma[dst] * (1.0 + d->d_delta[dst]));
    return false;
  }
};

}  // namespace bc
}  // namespace gunrock
