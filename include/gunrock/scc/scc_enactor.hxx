// gunrock/scc/scc_enactor.hxx -- strongly connected components on the advance and filter operators (mgx_scc_enact): the plain
// path, the fused path's cross-check and baseline.  One operator per call, one host wait per operator.
//   TRIM      passes of filter<trim_collect> over the iota frontier (every alive vertex recounts its alive neighbours, as the
//             operator k-core rescans) and filter<trim_seal> over what it kept, until a pass keeps nobody
//   pivot     filter<pivot_max>, filter<pivot_pick> over the iota frontier
//   a phase   filter<init>; advance<forward> over the iota frontier + the filter that counts its lowerings, until none (the hook loop
//             of cc_enactor_t); filter<root>; advance<backward> over the backward view + its filter, until nobody is claimed;
//             the pivot phase: filter<pivot_min>; filter<seal>; TRIM
// The pivot phase is a phase whose init seeds one colour; the rounds follow while somebody is alive.
#pragma once
#include <climits>

#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "scc_functor.hxx"
#include "scc_problem.hxx"

namespace gunrock {
namespace scc {

struct scc_enactor_t : enactor_t {
  // what the last enact() did
  long long trimmed = 0, pivot_size = 0, rounds = 0, waits = 0, calls = 0;

  // (the advances write one slot per entry: edge buffers of exactly num_edges, as cc_enactor_t's)
  scc_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {
    for (frontier_ptr& b : buffers) b = std::make_shared<frontier_t<int>>(ctx, (size_t)num_edges);
  }
  scc_enactor_t(const scc_enactor_t&) = delete;
  scc_enactor_t& operator=(const scc_enactor_t&) = delete;

  template <typename F>
  int filter(std::shared_ptr<scc_problem_t>& p, frontier_ptr& in, frontier_ptr& out, int iteration, standard_context_t& ctx) {
    ++waits; ++calls;
    return gunrock::oprtr::filter::filter_kernel<scc_problem_t, F>(p, in, out, iteration, ctx);
  }
  // advances of F over the iota frontier of `p`, each with the filter that counts what it applied, until one applies nothing
  template <typename F>
  void to_fixpoint(std::shared_ptr<scc_problem_t>& p, int iteration, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    for (;;) {
      adv::advance_forward_kernel<scc_problem_t, F, /*idempotence=*/false, /*has_output=*/true>(p, indices, buffers[0], iteration, ctx);
      ++waits; ++calls;                           // the advance (it reads its scan's total back); filter<> counts itself
      const int applied = filter<F>(p, buffers[0], buffers[1], iteration, ctx);
      if (applied == 0) break;
    }
  }
  long long trim(std::shared_ptr<scc_problem_t>& p, standard_context_t& ctx) {
    long long left = 0;
    for (;;) {
      const int doomed = filter<trim_collect_functor_t>(p, indices, filtered_indices, 0, ctx);
      if (doomed == 0) break;
      filter<trim_seal_functor_t>(p, filtered_indices, buffers[1], 0, ctx);
      left += doomed;
    }
    trimmed += left;
    return left;
  }

  void enact(std::shared_ptr<scc_problem_t> fwd, std::shared_ptr<scc_problem_t> bwd, scc_state_t& state, standard_context_t& ctx) {
    const int n = fwd->gslice->num_nodes;
    trimmed = pivot_size = rounds = waits = calls = 0;
    state.reset(n, ctx);
    indices->resize((size_t)n);                   // 0 .. n - 1, never written
    frontier_ptr& nobody = buffers[1];
    long long alive = n;
    alive -= trim(fwd, ctx);
    scc_scalars_t* const scalars = state.d_scalars.data();
    for (int tag = 1; alive > 0; ++tag) {
      const bool pivot_phase = tag == 1;
      if (pivot_phase) {
        transform([=] __device__(int) { scalars->best = 0; scalars->pivot = INT_MAX; scalars->pivot_min = INT_MAX; }, 1, ctx);
        filter<pivot_max_functor_t>(fwd, indices, nobody, 0, ctx);
        filter<pivot_pick_functor_t>(fwd, indices, nobody, 0, ctx);
      } else {
        ++rounds;
      }
      filter<init_functor_t>(fwd, indices, nobody, pivot_phase ? 1 : 0, ctx);
      to_fixpoint<forward_functor_t>(fwd, tag, ctx);
      filter<root_functor_t>(fwd, indices, filtered_indices, tag, ctx);
      to_fixpoint<backward_functor_t>(bwd, tag, ctx);
      if (pivot_phase) filter<pivot_min_functor_t>(fwd, indices, nobody, tag, ctx);
      const int sealed = filter<seal_functor_t>(fwd, indices, filtered_indices, pivot_phase ? -tag : tag, ctx);
      if (pivot_phase) pivot_size = sealed;
      alive -= sealed;
      alive -= trim(fwd, ctx);
    }
  }
};

}  // namespace scc
}  // namespace gunrock
