// gunrock/lpa/lpa_functor.hxx -- the device functors of the label propagation's operator path.  What the operators'
// `iteration` argument carries is said per functor.
//   gather_out_functor_t     the advance over every entry (v, u) of the iota frontier: the slot of v's segment that belongs to the
//                            entry's rank gets lab[u], or "none" for a self-loop
//   gather_in_functor_t      the same over the backward view, every in-entry (v <- u) as (v, u), behind v's out-entries
//   want_functor_t           over all vertices, behind the segmented sort: a run-length scan of v's sorted segment -- the longest
//                            run wins, the run of the current label wins a tie, then the first (the smallest label); kept: the
//                            unstable vertices, so the filter's count is unstable_t
//   apply_functor_t          iteration = t, over the unstable: those that move take their label; kept: the movers
#pragma once
#include "../../mgx/color_hash.hpp"
#include "../intrinsics.hxx"
#include "lpa_problem.hxx"

namespace gunrock {
namespace lpa {

typedef lpa_problem_t::data_slice_t lpa_slice_t;

struct gather_out_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, lpa_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int, int rank, int, lpa_slice_t* d, int) {
    d->d_votes[d->d_heads[v] + rank] = u != v ? d->d_label[u] : LPA_OP_NONE;
    return false;
  }
};
struct gather_in_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, lpa_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int, int rank, int, lpa_slice_t* d, int) {
    const int out_entries = d->d_row_offsets[v + 1] - d->d_row_offsets[v];
    d->d_votes[d->d_heads[v] + out_entries + rank] = u != v ? d->d_label[u] : LPA_OP_NONE;
    return false;
  }
};

struct want_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, lpa_slice_t* d, int) {
    const int cur = d->d_label[v];
    int best = cur, best_count = 0;
    bool best_is_cur = false;
    const int end = d->d_heads[v + 1];
    for (int i = d->d_heads[v]; i < end;) {
      const int label = d->d_votes[i];
      if (label == LPA_OP_NONE) break;                         // (sorted: only self-loops follow)
      int j = i + 1;
      while (j < end && d->d_votes[j] == label) ++j;
      const int count = j - i;
      if (count > best_count || (count == best_count && label == cur && !best_is_cur)) {
        best = label; best_count = count; best_is_cur = label == cur;
      }
      i = j;
    }
    d->d_want[v] = best;
    return best != cur;
  }
};

struct apply_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, lpa_slice_t* d, int t) {
    const bool moves = d->d_scalars->mode == 0 || (mgx::color_key(v, mgx::color_salt(d->d_scalars->seed, t)) & 1u);
    if (moves) d->d_label[v] = d->d_want[v];
    return moves;
  }
};

}  // namespace lpa
}  // namespace gunrock
