// gunrock/cc/cc_enactor.hxx -- connected components on the advance and filter operators (mgx_cc_enact): the slow, plain path,
// and the fused path's cross-check and baseline.  Shiloach-Vishkin, per iteration:
//   advance<hook_functor_t, idempotence = false, has_output = true>   over the iota frontier: every entry hooks
//   filter<hook_functor_t>     over the advance's slots: how many entries hooked (the operator's return value)
//   no entry hooked: stop.  Else filter<jump_functor_t> over the iota frontier, again until a pass moves nobody.
// Every operator reads its count back once: `waits` counts them.
#pragma once
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "cc_functor.hxx"
#include "cc_problem.hxx"

namespace gunrock {
namespace cc {

struct cc_enactor_t : enactor_t {
  // what the last enact() did: iterations (hook advances), jump passes, entries that hooked, host waits
  long long iterations = 0, jumps = 0, hooks = 0, waits = 0;

  // The hook advance writes one slot per entry.  enactor_t sizes its edge buffers (int)(num_edges * queue_sizing) in float, which
  // rounds some m above 2^24 down (m = 20 000 001 -> 20 000 000): here they are allocated at exactly num_edges (the base gets 0).
  cc_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {
    for (frontier_ptr& b : buffers) b = std::make_shared<frontier_t<int>>(ctx, (size_t)num_edges);
  }
  cc_enactor_t(const cc_enactor_t&) = delete;
  cc_enactor_t& operator=(const cc_enactor_t&) = delete;

  void enact(std::shared_ptr<cc_problem_t> problem, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    namespace fl = gunrock::oprtr::filter;
    const int n = problem->gslice->num_nodes;
    problem->reset(ctx);
    frontier_ptr& everyone = indices;             // 0 .. n - 1, never written
    frontier_ptr& moved = filtered_indices;       // the jump passes' survivors (only their number is used)
    everyone->resize((size_t)n);
    iterations = jumps = hooks = waits = 0;
    for (int iteration = 0;; ++iteration) {
      ++iterations;
      adv::advance_forward_kernel<cc_problem_t, hook_functor_t, /*idempotence=*/false, /*has_output=*/true>(
          problem, everyone, buffers[0], iteration, ctx);
      const int hooked = fl::filter_kernel<cc_problem_t, hook_functor_t>(problem, buffers[0], buffers[1], iteration, ctx);
      waits += 2;
      hooks += hooked;
      if (hooked == 0) break;
      for (;;) {
        ++jumps;
        const int changed = fl::filter_kernel<cc_problem_t, jump_functor_t>(problem, everyone, moved, iteration, ctx);
        ++waits;
        if (changed == 0) break;
      }
    }
  }
};

}  // namespace cc
}  // namespace gunrock
