// gunrock/cc/cc_functor.hxx -- the device functors of the connected components' operator path (Shiloach-Vishkin).
//   hook_functor_t   the advance over every entry (v, u): labels that differ hook the larger under the smaller,
//                    atomicMin(&comp[max], min); apply_advance says whether they differed, so the filter behind the advance
//                    counts the entries that hooked (its test looks at the slot's value alone).  Symmetric in v and u: the
//                    path is correct on any graph, directed or not.
//   jump_functor_t   the filter over every vertex: comp[v] = comp[comp[v]]; it keeps the vertices it moved, so a pass that
//                    keeps nobody means every vertex hangs directly under a root.
// The loads are plain: within a launch one may see an old label, but labels only decrease and always name a vertex of the same
// component, so an old one is still an ancestor; a hook it misses is seen again by the next iteration's advance.
#pragma once
#include "../intrinsics.hxx"
#include "cc_problem.hxx"

namespace gunrock {
namespace cc {

typedef cc_problem_t::data_slice_t cc_slice_t;

struct hook_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, cc_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int src, int dst, int, int, int, cc_slice_t* d, int) {
    const int a = d->d_comp[src], b = d->d_comp[dst];
    if (a == b) return false;
    atomicMin(d->d_comp + max(a, b), min(a, b));
    return true;
  }
  static __device__ __forceinline__ bool cond_filter(int slot_value, cc_slice_t*, int) { return slot_value != -1; }
  static constexpr bool cond_filter_of_slot_value_only = true;
};

struct jump_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, cc_slice_t* d, int) {
    int* const comp = d->d_comp;
    const int p = comp[v], pp = comp[p];
    if (pp == p) return false;
    comp[v] = pp;
    return true;
  }
};

}  // namespace cc
}  // namespace gunrock
