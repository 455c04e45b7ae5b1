// gunrock/tc/tc_enactor.hxx -- triangle counting on the advance operator (mgx_tc_enact): the plain path, the fused path's
// cross-check and baseline.  One step:
//   advance<tc_functor_t, idempotence = false, has_output = false>   over the iota frontier of the oriented graph: every entry
//   (a, b) intersects rows a and b in one thread (tc_functor.hxx).
// The operator reads its work-item count back once: `waits` counts it (and the wait behind which its scan buffer grows, once).  Right on any input: the oriented graph is.
#pragma once
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "tc_functor.hxx"
#include "tc_problem.hxx"

namespace gunrock {
namespace tc {

struct tc_enactor_t : enactor_t {
  long long waits = 0;

  // no edge-capacity buffers: the advance writes no output
  tc_enactor_t(standard_context_t& ctx, int num_nodes) : enactor_t(ctx, num_nodes, 0, 0.0f) {}
  tc_enactor_t(const tc_enactor_t&) = delete;
  tc_enactor_t& operator=(const tc_enactor_t&) = delete;

  // tri (cleared by the caller) += the counts of the problem's oriented graph
  void enact(std::shared_ptr<tc_problem_t> problem, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    frontier_ptr& everyone = indices;             // 0 .. n - 1, never written
    everyone->resize((size_t)problem->gslice->num_nodes);
    waits = 0;
    if (problem->gslice->d_scanned_row_offsets.size() < everyone->capacity() + 1) ++waits;   // (the advance grows it behind a wait, once)
    adv::advance_forward_kernel<tc_problem_t, tc_functor_t, /*idempotence=*/false, /*has_output=*/false>(
        problem, everyone, buffers[0], 0, ctx);
    ++waits;
  }
};

}  // namespace tc
}  // namespace gunrock
