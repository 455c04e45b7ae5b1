// gunrock/rw/rw_enactor.hxx -- random walks on the filter operator (mgx_rw_enact): the plain path, the fused path's cross-check
// and yardstick.  The frontier is the list of the live walkers; a step is one filter and one host wait.
//   transform            every walker at its start: slot 0, its visit, the frontier 0 .. W - 1
//   filter<step>  x L    walker w takes step t and writes slot t + 1; kept: the walkers that go on.  The loop ends early when
//                        nobody is left
// The paths are stored directly (a walker's slot t + 1 at a stride of 4 (L + 1) bytes), the visits and the counts by atomics.
// (No enactor_t underneath: its frontiers are sized by the graph, these by the walkers.)
#pragma once
#include <vector>

#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "rw_functor.hxx"
#include "rw_problem.hxx"

namespace gunrock {
namespace rw {

struct rw_enactor_t {
  typedef std::shared_ptr<frontier_t<int>> frontier_ptr;
  // what the last enact() did
  long long steps_run = 0, waits = 0, calls = 0;
  frontier_ptr fronts[2];                         // walker capacity: the live walkers of step t in fronts[t & 1]
  size_t cap = 0;

  rw_enactor_t() {}
  rw_enactor_t(const rw_enactor_t&) = delete;
  rw_enactor_t& operator=(const rw_enactor_t&) = delete;

  template <bool WEIGHTED, bool SECOND>
  int step(std::shared_ptr<rw_problem_t>& p, int t, standard_context_t& ctx) {
    ++waits; ++calls;
    return gunrock::oprtr::filter::filter_kernel<rw_problem_t, step_functor_t<WEIGHTED, SECOND>>(p, fronts[t & 1], fronts[(t + 1) & 1], t, ctx);
  }

  void enact(std::shared_ptr<rw_problem_t> p, const rw_problem_t::data_slice_t& s, const mgx::rw_request_t& r, standard_context_t& ctx) {
    const long long W = r.walkers();
    steps_run = waits = calls = 0;
    if ((size_t)W > cap) {
      for (frontier_ptr& f : fronts) f = std::make_shared<frontier_t<int>>(ctx, (size_t)W);
      cap = (size_t)W;
    }
    int* const live = fronts[0]->data()->data();
    const rw_problem_t::data_slice_t d = s;
    transform([=] __device__(int w) {
      const int src = w / d.per_start;
      const int start = d.d_starts ? d.d_starts[src] : src;
      live[w] = w;
      d.d_cur[w] = start; d.d_prev[w] = -1; d.d_len[w] = 0;
      if (d.d_paths) d.d_paths[(size_t)w * ((size_t)d.length + 1)] = start;
      if (d.d_visits) atomicAdd(d.d_visits + start, 1ull);
    }, W, ctx);
    ++calls;
    fronts[0]->resize((size_t)W);
    mgx::frontier_touched();
    for (int t = 0; t < (int)r.length; ++t) {
      int kept;
      if (r.weighted) kept = r.second ? step<true, true>(p, t, ctx) : step<true, false>(p, t, ctx);
      else kept = r.second ? step<false, true>(p, t, ctx) : step<false, false>(p, t, ctx);
      ++steps_run;
      if (kept == 0) break;
    }
  }
};

}  // namespace rw
}  // namespace gunrock
