// gunrock/ktruss/ktruss_functor.hxx -- the device functors of the k-truss decomposition's operator path.  `k` arrives
// in the operators' `iteration` argument.
//   support_functor_t::cond_advance(a, b)  the advance over every DAG entry (a, b) at position `edge`: one thread intersects the
//                                          sorted rows a and b (mgx::tc_intersect with the adds sent to the entries: one to each of
//                                          the two positions of a common element) and adds the count to the entry itself
//   collect_functor_t::cond_filter(e)      an alive edge at sup <= k - 2 joins the front and is marked so (the thread that tests an
//                                          edge is the only one that looks at its state in that launch)
//   expand_functor_t::cond_filter(e)       front edge e = {u, v}: the entries of the shorter of adjacency rows u, v searched in the
//                                          longer, the two other edges of every triangle from adj_eid; neither in the front: both
//                                          lose 1; exactly one in the front: the third loses 1, charged by the lower edge id of the
//                                          two front edges; both in the front or one removed: nothing.  States are not written here.
//   seal_functor_t::cond_filter(e)         truss = k, removed, atomicMax on vtruss of both ends, hist[k] += 1
// Integer adds commute: the results do not depend on the order the edges run in.
#pragma once
#include "../../mgx/ktruss_fused.hpp"
#include "../intrinsics.hxx"
#include "ktruss_problem.hxx"

namespace gunrock {
namespace ktruss {

typedef ktruss_problem_t::data_slice_t ktruss_slice_t;

struct support_functor_t {
  static __device__ __forceinline__ bool cond_advance(int a, int b, int edge, int, int, ktruss_slice_t* d, int) {
    const int* const ro = d->d_row_offsets;
    const int ra = ro[a], rb = ro[b];
    const int c = mgx::tc_intersect<true>(d->d_col_indices, ra, ro[a + 1] - ra, rb, ro[b + 1] - rb, d->d_sup0);
    if (c) atomicAdd(d->d_sup0 + edge, c);
    return c > 0;
  }
  static __device__ __forceinline__ bool apply_advance(int, int, int, int, int, ktruss_slice_t*, int) { return true; }
};

struct collect_functor_t {
  static __device__ __forceinline__ bool cond_filter(int e, ktruss_slice_t* d, int k) {
    const bool joins = d->d_state[e] == mgx::KTRUSS_ALIVE && d->d_sup[e] <= k - 2;
    if (joins) d->d_state[e] = mgx::KTRUSS_FRONT;
    return joins;
  }
};

struct expand_functor_t {
  static __device__ __forceinline__ bool cond_filter(int e, ktruss_slice_t* d, int) {
    const int u = d->d_src[e], v = d->d_col_indices[e];
    int s = d->d_adj_ro[u], sl = d->d_adj_ro[u + 1] - s;
    int l = d->d_adj_ro[v], ll = d->d_adj_ro[v + 1] - l;
    if (sl > ll) {
      const int t = s; s = l; l = t;
      const int tl = sl; sl = ll; ll = tl;
    }
    const int le = l + ll;
    int lo = l;
    for (int i = s; i < s + sl && lo < le; ++i) {
      const int w = d->d_adj_ci[i];
      int hi = le;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d->d_adj_ci[mid] < w) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= le || d->d_adj_ci[lo] != w) continue;
      const int e1 = d->d_adj_eid[i], e2 = d->d_adj_eid[lo];
      const int s1 = d->d_state[e1], s2 = d->d_state[e2];
      if (s1 == mgx::KTRUSS_REMOVED || s2 == mgx::KTRUSS_REMOVED) continue;
      const bool f1 = s1 == mgx::KTRUSS_FRONT, f2 = s2 == mgx::KTRUSS_FRONT;
      if (!f1 && !f2) {
        atomicAdd(d->d_sup + e1, -1);
        atomicAdd(d->d_sup + e2, -1);
      } else if (f1 && !f2) {
        if (e < e1) atomicAdd(d->d_sup + e2, -1);
      } else if (f2 && !f1) {
        if (e < e2) atomicAdd(d->d_sup + e1, -1);
      }
    }
    return false;
  }
};

struct seal_functor_t {
  static __device__ __forceinline__ bool cond_filter(int e, ktruss_slice_t* d, int k) {
    d->d_truss[e] = k;
    d->d_state[e] = mgx::KTRUSS_REMOVED;
    atomicMax(d->d_vtruss + d->d_src[e], k);
    atomicMax(d->d_vtruss + d->d_col_indices[e], k);
    atomicAdd(d->d_hist + k, 1);
    return false;
  }
};

}  // namespace ktruss
}  // namespace gunrock
