// gunrock/scc/scc_functor.hxx -- the device functors of the strongly connected components' operator path.  What the
// operators' `iteration` argument carries is said per functor.
//   trim_collect_functor_t::cond_filter(v)  alive v recounts its entries to and from alive vertices other than itself; no entry on
//                                           either side: it is DOOMED and kept.  The count takes a doomed vertex for alive: who
//                                           leaves in this pass was alive when the pass began, as the fused path's fronts are.
//   trim_seal_functor_t::cond_filter(v)     over the doomed: label = own id, removed
//   pivot_max_functor_t / pivot_pick_functor_t   over all vertices: atomicMax of outdeg * indeg (recounted), then atomicMin of the
//                                           ids that have it
//   init_functor_t::cond_filter(v)          iteration = 1, the pivot phase: col = "none", the pivot's its own id; 0, a round:
//                                           col = own id
//   forward_functor_t                       the advance over every arc v -> u between alive vertices: atomicMin(col[u], col[v]);
//                                           apply_advance says whether it lowered, so the filter behind the advance counts the
//                                           lowerings (cc's hook loop)
//   root_functor_t::cond_filter(v)          iteration = the round's tag: alive with col[v] == v: claimed
//   backward_functor_t                      the advance over the backward view, every in-entry (u <- v) as (u, v): u claimed, v
//                                           alive, not claimed and of u's colour: v is claimed (one exchange: once)
//   pivot_min_functor_t::cond_filter(v)     the pivot phase: atomicMin of the claimed ids
//   seal_functor_t::cond_filter(v)          iteration = tag, or -tag in the pivot phase: the claimed get their label and leave
// Loads are plain: within a launch one may see an old colour or claim, but both only move one way, and the pass after sees the rest.
#pragma once
#include "../intrinsics.hxx"
#include "scc_problem.hxx"

namespace gunrock {
namespace scc {

typedef scc_problem_t::data_slice_t scc_slice_t;

// v's entries in [offsets[v], offsets[v + 1]) of adj that name a vertex other than v that has not been removed
__device__ __forceinline__ int scc_count_alive(const int* offsets, const int* adj, const int* state, int v) {
  int c = 0;
  for (int e = offsets[v]; e < offsets[v + 1]; ++e) {
    const int u = adj[e];
    c += (u != v && state[u] != SCC_OP_REMOVED) ? 1 : 0;
  }
  return c;
}

struct trim_collect_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int) {
    if (d->d_state[v] != SCC_OP_ALIVE) return false;
    const bool leaves = scc_count_alive(d->d_row_offsets, d->d_col_indices, d->d_state, v) == 0 ||
                        scc_count_alive(d->d_col_offsets, d->d_row_indices, d->d_state, v) == 0;
    if (leaves) d->d_state[v] = SCC_OP_DOOMED;
    return leaves;
  }
};

struct trim_seal_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int) {
    d->d_state[v] = SCC_OP_REMOVED;
    d->d_label[v] = v;
    return false;
  }
};

__device__ __forceinline__ unsigned long long scc_product(scc_slice_t* d, int v) {
  return (unsigned long long)scc_count_alive(d->d_row_offsets, d->d_col_indices, d->d_state, v) *
         (unsigned long long)scc_count_alive(d->d_col_offsets, d->d_row_indices, d->d_state, v);
}
struct pivot_max_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int) {
    if (d->d_state[v] != SCC_OP_ALIVE) return false;
    atomicMax(&d->d_scalars->best, scc_product(d, v));
    return false;
  }
};
struct pivot_pick_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int) {
    if (d->d_state[v] != SCC_OP_ALIVE || scc_product(d, v) != d->d_scalars->best) return false;
    atomicMin(&d->d_scalars->pivot, v);
    return false;
  }
};

struct init_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int pivot_phase) {
    if (d->d_state[v] != SCC_OP_ALIVE) return false;
    d->d_col[v] = (!pivot_phase || v == d->d_scalars->pivot) ? v : SCC_OP_NONE;
    return false;
  }
};

struct forward_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, scc_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int, int, int, scc_slice_t* d, int) {
    if (v == u || d->d_state[v] != SCC_OP_ALIVE || d->d_state[u] != SCC_OP_ALIVE) return false;
    const int c = d->d_col[v];
    if (d->d_col[u] <= c) return false;
    return atomicMin(d->d_col + u, c) > c;
  }
  static __device__ __forceinline__ bool cond_filter(int slot_value, scc_slice_t*, int) { return slot_value != -1; }
  static constexpr bool cond_filter_of_slot_value_only = true;
};

struct root_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int tag) {
    const bool root = d->d_state[v] == SCC_OP_ALIVE && d->d_col[v] == v;
    if (root) d->d_claim[v] = tag;
    return root;
  }
};

struct backward_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, scc_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int u, int v, int, int, int, scc_slice_t* d, int tag) {
    if (d->d_claim[u] != tag || d->d_state[u] != SCC_OP_ALIVE || d->d_state[v] != SCC_OP_ALIVE) return false;
    if (d->d_claim[v] == tag || d->d_col[v] != d->d_col[u]) return false;
    return atomicExch(d->d_claim + v, tag) != tag;
  }
  static __device__ __forceinline__ bool cond_filter(int slot_value, scc_slice_t*, int) { return slot_value != -1; }
  static constexpr bool cond_filter_of_slot_value_only = true;
};

struct pivot_min_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int tag) {
    if (d->d_state[v] == SCC_OP_ALIVE && d->d_claim[v] == tag) atomicMin(&d->d_scalars->pivot_min, v);
    return false;
  }
};

struct seal_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, scc_slice_t* d, int signed_tag) {
    const int tag = signed_tag < 0 ? -signed_tag : signed_tag;
    if (d->d_state[v] != SCC_OP_ALIVE || d->d_claim[v] != tag) return false;
    d->d_state[v] = SCC_OP_REMOVED;
    d->d_label[v] = signed_tag < 0 ? d->d_scalars->pivot_min : d->d_col[v];
    return true;
  }
};

}  // namespace scc
}  // namespace gunrock
