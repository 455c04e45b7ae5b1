// gunrock/agg/agg_enactor.hxx -- neighbour feature aggregation on the filter operator (mgx_agg_enact): the plain path, the fused
// path's cross-check and yardstick.
//   filter<row>   one pass over the rows 0 .. R - 1, a lane per row (agg_functor.hxx); nothing is kept
// One operator call and its host wait, whatever the rows' lengths.  (No enactor_t underneath: its frontiers hold a traversal's
// state, this is one pass over an iota.)
#pragma once
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "agg_functor.hxx"
#include "agg_problem.hxx"

namespace gunrock {
namespace agg {

struct agg_enactor_t {
  typedef std::shared_ptr<frontier_t<int>> frontier_ptr;
  long long waits = 0, calls = 0;     // what the last enact() did
  frontier_ptr all, none;             // the rows; what the pass keeps (nothing)
  size_t room = 0;

  agg_enactor_t() {}
  agg_enactor_t(const agg_enactor_t&) = delete;
  agg_enactor_t& operator=(const agg_enactor_t&) = delete;

  // the iota over as many rows as the largest call so far
  void ensure(int R, standard_context_t& ctx) {
    if ((size_t)R <= room) return;
    all = std::make_shared<frontier_t<int>>(ctx, (size_t)R);
    none = std::make_shared<frontier_t<int>>(ctx, (size_t)R);
    int* const ids = all->data()->data();
    transform([=] __device__(int v) { ids[v] = v; }, R, ctx);
    room = (size_t)R;
    mgx::frontier_touched();
  }

  void enact(std::shared_ptr<agg_problem_t> p, int R, standard_context_t& ctx) {
    waits = calls = 0;
    if (R <= 0) return;
    ensure(R, ctx);
    all->resize((size_t)R);
    gunrock::oprtr::filter::filter_kernel<agg_problem_t, row_functor_t>(p, all, none, 0, ctx);
    ++calls; ++waits;
  }
};

}  // namespace agg
}  // namespace gunrock
