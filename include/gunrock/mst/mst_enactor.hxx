// gunrock/mst/mst_enactor.hxx -- minimum spanning forest on the advance and filter operators (mgx_mst_enact): plain Boruvka over
// the unsorted CSR, the fused path's cross-check and baseline.  Per round:
//   advance<weight_functor_t, idempotence = false, has_output = false>   over the iota frontier: the components' lightest weights
//   advance<pair_functor_t,   idempotence = false, has_output = false>   over the iota frontier: their smallest pairs
//   filter<hook_functor_t>    over the iota frontier: the roots append their edges and hook; nobody kept: stop
//   filter<jump_functor_t>    over the iota frontier until a pass moves nobody, then the roots' snapshot is renewed
// It rescans every entry every round: that is its point.  Every operator call reads its count back once: `waits` counts the calls
// (as the other operator paths' enactors do), not the operators' own synchronisations.
// The host loops are bounded (rounds and jump passes by ceil(log2 n) + 2 each): with a true `symmetric` word they end earlier by
// themselves; with a false one two roots may hook under each other, which no pointer jumping resolves -- the forest is wrong then,
// and the run still ends.
#pragma once
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "mst_functor.hxx"
#include "mst_problem.hxx"

namespace gunrock {
namespace mst {

struct mst_enactor_t : enactor_t {
  // what the last enact() did: rounds that chose something, jump passes, host waits
  long long rounds = 0, jumps = 0, waits = 0;

  mst_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {}
  mst_enactor_t(const mst_enactor_t&) = delete;
  mst_enactor_t& operator=(const mst_enactor_t&) = delete;

  void enact(std::shared_ptr<mst_problem_t> problem, bool symmetric, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    namespace fl = gunrock::oprtr::filter;
    const int n = problem->gslice->num_nodes;
    problem->reset(symmetric, ctx);
    frontier_ptr& everyone = indices;             // 0 .. n - 1, never written
    frontier_ptr& kept = filtered_indices;        // the filters' survivors (only their number is used)
    everyone->resize((size_t)n);
    rounds = jumps = waits = 0;
    int bound = 2;
    while ((1LL << (bound - 2)) < n) ++bound;     // ceil(log2 n) + 2
    int* const comp = problem->d_comp.data();
    int* const root = problem->d_root.data();
    int* const smallest = problem->d_min.data();
    unsigned* const cw = problem->d_cw.data();
    unsigned long long* const cp = problem->d_cp.data();
    for (int round = 0; round < bound; ++round) {
      transform([=] __device__(int v) { cw[v] = 0xFFFFFFFFu; cp[v] = ~0ull; }, n, ctx);
      adv::advance_forward_kernel<mst_problem_t, weight_functor_t, /*idempotence=*/false, /*has_output=*/false>(
          problem, everyone, buffers[0], round, ctx);
      adv::advance_forward_kernel<mst_problem_t, pair_functor_t, false, false>(problem, everyone, buffers[0], round, ctx);
      const int chose = fl::filter_kernel<mst_problem_t, hook_functor_t>(problem, everyone, kept, round, ctx);
      waits += 3;
      if (chose == 0) break;
      ++rounds;
      for (int pass = 0; pass < bound; ++pass) {
        ++jumps;
        const int moved = fl::filter_kernel<mst_problem_t, jump_functor_t>(problem, everyone, kept, round, ctx);
        ++waits;
        if (moved == 0) break;
      }
      transform([=] __device__(int v) { root[v] = comp[v]; }, n, ctx);
    }
    // the labels: the smallest id of every root's set, into d_root
    transform([=] __device__(int v) { smallest[v] = v; }, n, ctx);
    transform([=] __device__(int v) { atomicMin(smallest + comp[v], v); }, n, ctx);
    transform([=] __device__(int v) { root[v] = smallest[comp[v]]; }, n, ctx);
  }
};

}  // namespace mst
}  // namespace gunrock
