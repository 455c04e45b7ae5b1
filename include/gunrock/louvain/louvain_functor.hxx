// gunrock/louvain/louvain_functor.hxx -- the device functors of the Louvain run's operator path.
//   gather_out_functor_t     the advance over every entry (v, u) of the iota frontier: the slot of v's segment that belongs to the
//                            entry's rank gets (lab[u], weight), or "none" for a self entry
//   gather_in_functor_t      level 0, symmetric == 0: the same over the backward view, behind v's out-entries
//   best_functor_t           iteration = t, over all vertices, behind the segmented sort: a scan of the runs of v's sorted segment
//                            sums k_{v,c}, scores every candidate and keeps best(v); kept: the vertices that move in iteration t
//   apply_functor_t          over the movers: they take their label, their k moves between the Sigmas by integer atomics
#pragma once
#include "../../mgx/color_hash.hpp"
#include "../intrinsics.hxx"
#include "louvain_problem.hxx"

namespace gunrock {
namespace louvain {

typedef louvain_problem_t::data_slice_t louvain_slice_t;

struct gather_out_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, louvain_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int edge, int rank, int, louvain_slice_t* d, int) {
    const int slot = d->d_heads[v] + rank;
    d->d_votes[slot] = u != v ? d->d_label[u] : LV_OP_NONE;
    d->d_vote_w[slot] = u != v ? (d->d_weights ? d->d_weights[edge] : 1u) : 0u;
    return false;
  }
};
struct gather_in_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, louvain_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int v, int u, int, int rank, int, louvain_slice_t* d, int) {
    const int slot = d->d_heads[v] + (d->d_row_offsets[v + 1] - d->d_row_offsets[v]) + rank;
    d->d_votes[slot] = u != v ? d->d_label[u] : LV_OP_NONE;
    d->d_vote_w[slot] = u != v ? 1u : 0u;
    return false;
  }
};

__device__ __forceinline__ long long lv_op_score(unsigned kvc, long long w, unsigned sigma_c, bool is_cur, unsigned kv) {
  return (long long)kvc * w - ((long long)sigma_c - (is_cur ? (long long)kv : 0ll)) * (long long)kv;
}

struct best_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, louvain_slice_t* d, int t) {
    const int cur = d->d_label[v];
    const unsigned kv = d->d_k[v], seed = d->d_scalars->seed;
    const long long w = d->d_scalars->w;
    int best = cur;
    long long best_score = lv_op_score(0, w, d->d_sigma[cur], true, kv);
    const int end = d->d_heads[v + 1];
    for (int i = d->d_heads[v]; i < end;) {
      const int label = d->d_votes[i];
      if (label == LV_OP_NONE) break;                          // (sorted: only self entries follow)
      unsigned kvc = 0;
      int j = i;
      while (j < end && d->d_votes[j] == label) kvc += d->d_vote_w[j++];
      const long long s = lv_op_score(kvc, w, d->d_sigma[label], label == cur, kv);
      const bool better = s != best_score ? s > best_score
                                          : (label != best && (label == cur || (best != cur && mgx::color_key(label, seed) < mgx::color_key(best, seed))));
      if (better) { best = label; best_score = s; }
      i = j;
    }
    d->d_best[v] = best;
    const unsigned kb = mgx::color_key(best, seed), kc = mgx::color_key(cur, seed);
    return best != cur && ((t & 1) ? kb > kc : kb < kc);
  }
};

struct apply_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, louvain_slice_t* d, int) {
    const int cur = d->d_label[v], best = d->d_best[v];
    const unsigned kv = d->d_k[v];
    d->d_label[v] = best;
    if (kv) {
      atomicSub(d->d_sigma + cur, kv);
      atomicAdd(d->d_sigma + best, kv);
    }
    return true;
  }
};

}  // namespace louvain
}  // namespace gunrock
