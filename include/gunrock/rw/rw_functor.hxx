// gunrock/rw/rw_functor.hxx -- the device functor of the random walks' operator path.
//   step_functor_t<WEIGHTED, SECOND>   iteration = t, the filter over the live walkers: walker w takes step t (mgx::rw_step, the
//                                      fused path's own draw and acceptance test), writes slot t + 1 of its path, adds its visit
//                                      and the step's counts; kept: the walkers whose walk goes on
#pragma once
#include "../intrinsics.hxx"
#include "rw_problem.hxx"

namespace gunrock {
namespace rw {

typedef rw_problem_t::data_slice_t rw_slice_t;

template <bool WEIGHTED, bool SECOND>
struct step_functor_t {
  static __device__ __forceinline__ bool cond_filter(int w, rw_slice_t* d, int t) {
    if (w < 0) return false;
    const int s = w / d->per_start;
    const int start = d->d_starts ? d->d_starts[s] : s;
    int prev = d->d_prev[w];
    mgx::rw_tally_t tally;
    const int nxt = mgx::rw_step<WEIGHTED, SECOND>(d->g, d->P, mgx::rw_walker_key(d->P.seed, (unsigned)w), t, start, d->d_cur[w], prev, tally);
    if (tally.dead) atomicAdd(d->d_counters + mgx::RW_C_DEAD, 1ull);
    if (tally.restarts) atomicAdd(d->d_counters + mgx::RW_C_RESTARTS, 1ull);
    if (tally.tries) atomicAdd(d->d_counters + mgx::RW_C_TRIES, tally.tries);
    if (tally.fallbacks) atomicAdd(d->d_counters + mgx::RW_C_FALLBACKS, 1ull);
    if (nxt < 0) return false;
    atomicAdd(d->d_counters + mgx::RW_C_STEPS, 1ull);
    d->d_cur[w] = nxt;
    d->d_prev[w] = prev;
    d->d_len[w] = t + 1;
    if (d->d_paths) d->d_paths[(size_t)w * ((size_t)d->length + 1) + (size_t)t + 1] = nxt;
    if (d->d_visits) atomicAdd(d->d_visits + nxt, 1ull);
    return true;
  }
};

}  // namespace rw
}  // namespace gunrock
