// gunrock/sim/sim_enactor.hxx -- vertex similarity on the filter operator (mgx_sim_enact): the plain path, the fused path's
// cross-check and yardstick.
//   filter<merge>   over the pair indices 0 .. P - 1: a thread per pair merges the two rows; kept are the pairs with c > 0, so the
//                   output frontier's length is stats [2]
// One operator call and its host wait (the filter's count).  (No enactor_t underneath: its frontiers hold a traversal's state.)
#pragma once
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "sim_functor.hxx"
#include "sim_problem.hxx"

namespace gunrock {
namespace sim {

struct sim_enactor_t {
  typedef std::shared_ptr<frontier_t<int>> frontier_ptr;
  frontier_ptr all, kept;                         // the pair indices; the pairs with a common neighbour
  size_t cap = 0;
  long long waits = 0, calls = 0;                 // what the last enact() did

  sim_enactor_t(standard_context_t& ctx, size_t pairs) : cap(pairs) {
    all = std::make_shared<frontier_t<int>>(ctx, pairs);
    kept = std::make_shared<frontier_t<int>>(ctx, pairs);
    int* const ids = all->data()->data();
    transform([=] __device__(int p) { ids[p] = p; }, (int)pairs, ctx);
  }
  sim_enactor_t(const sim_enactor_t&) = delete;
  sim_enactor_t& operator=(const sim_enactor_t&) = delete;

  // returns the pairs with a common neighbour
  long long enact(std::shared_ptr<sim_problem_t> p, long long pairs, standard_context_t& ctx) {
    waits = calls = 0;
    all->resize((size_t)pairs);
    mgx::frontier_touched();
    const int positive = gunrock::oprtr::filter::filter_kernel<sim_problem_t, merge_functor_t>(p, all, kept, 0, ctx);
    ++waits; ++calls;
    return positive;
  }
};

}  // namespace sim
}  // namespace gunrock
