// gunrock/mst/mst_functor.hxx -- the device functors of the minimum spanning forest's operator path (plain Boruvka).
//   weight_functor_t   advance over every entry (v, u, w) that joins two components: atomicMin of key(w) on the word of v's
//                      component -- and of u's when symmetric == 0: the entry is u's in-entry, the one the fused path reads from
//                      the CSC.  In round 0 it also counts the incident entries and the NaN weights.
//   pair_functor_t     the same entries again: those of their component's lightest weight atomicMin (min << 32 | max) on its pair word
//   hook_functor_t     filter over every vertex: a root r with an outgoing edge, leading to component o, appends the edge to the
//                      list and hangs itself under o.  The mutual pair (o's edge is the same triple) is appended once, by the
//                      smaller root, and the larger hangs under the smaller: the hooks of a round form no cycle.  It keeps the
//                      roots that chose or hooked: a round that keeps nobody ends the run.
//   jump_functor_t     filter over every vertex: comp[v] = comp[comp[v]], keeps the vertices it moved
// A round's decisions read d_root, the snapshot of the roots; only the hook and jump filters write d_comp.
#pragma once
#include "../intrinsics.hxx"
#include "mst_problem.hxx"

namespace gunrock {
namespace mst {

typedef mst_problem_t::data_slice_t mst_slice_t;

struct weight_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, mst_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int src, int dst, int edge, int, int, mst_slice_t* d, int iteration) {
    if (src == dst) return false;
    const float w = d->d_w[edge];
    if (iteration == 0) {
      const mgx::u64 m = __ballot(true);                     // (the lanes that hold an entry that is no self-loop)
      if (mgx::lane_id() == __ffsll((long long)m) - 1) atomicAdd(d->d_counters + 1, (unsigned long long)__popcll(m) * (d->symmetric ? 1 : 2));
      if (mgx::mst_is_nan(w)) atomicAdd(d->d_counters + 2, 1ull);
    }
    const int rs = d->d_root[src], rd = d->d_root[dst];
    if (rs == rd) return false;
    const unsigned key = mgx::mst_key(w);
    atomicMin(d->d_cw + rs, key);
    if (!d->symmetric) atomicMin(d->d_cw + rd, key);
    return true;
  }
};

struct pair_functor_t {
  static __device__ __forceinline__ bool cond_advance(int, int, int, int, int, mst_slice_t*, int) { return true; }
  static __device__ __forceinline__ bool apply_advance(int src, int dst, int edge, int, int, mst_slice_t* d, int) {
    if (src == dst) return false;
    const int rs = d->d_root[src], rd = d->d_root[dst];
    if (rs == rd) return false;
    const unsigned key = mgx::mst_key(d->d_w[edge]);
    const unsigned long long pk = mgx::mst_pair(src, dst);
    if (key == d->d_cw[rs]) atomicMin(d->d_cp + rs, pk);
    if (!d->symmetric && key == d->d_cw[rd]) atomicMin(d->d_cp + rd, pk);
    return true;
  }
};

struct hook_functor_t {
  static __device__ __forceinline__ bool cond_filter(int r, mst_slice_t* d, int) {
    if (d->d_root[r] != r) return false;
    const unsigned long long pk = d->d_cp[r];
    if (pk == ~0ull) return false;                           // no outgoing edge
    const unsigned wk = d->d_cw[r];
    const int a = (int)(pk >> 32), b = (int)(unsigned)pk;
    const int o = d->d_root[d->d_root[a] == r ? b : a];
    const bool mutual = d->d_cw[o] == wk && d->d_cp[o] == pk;
    if (!(mutual && o < r)) {
      const unsigned long long at = atomicAdd(d->d_counters, 1ull);
      if (at < (unsigned long long)d->cap) {
        d->d_a[at] = a;
        d->d_b[at] = b;
        d->d_w_out[at] = __uint_as_float(mgx::mst_bits_of_key(wk));
      }
    }
    if (!mutual || o < r) d->d_comp[r] = o;
    return true;
  }
};

struct jump_functor_t {
  static __device__ __forceinline__ bool cond_filter(int v, mst_slice_t* d, int) {
    int* const comp = d->d_comp;
    const int p = comp[v], pp = comp[p];
    if (pp == p) return false;
    comp[v] = pp;
    return true;
  }
};

}  // namespace mst
}  // namespace gunrock
