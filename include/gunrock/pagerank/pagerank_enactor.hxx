// gunrock/pagerank/pagerank_enactor.hxx -- PageRank on the neighbourhood-reduce operator (mgx_pagerank_enact): the plain path,
// and the fused path's cross-check and baseline.  Per iteration:
//   neighborhood_kernel<pagerank_functor_t, float, plus_t<float>, has_output = false, push = false>  over the iota frontier:
//       S[v] = the sum of the contributions of v's in-neighbours (the CSC slots: the CSR's own rows on a graph whose slots
//       mirror it, which is right when the graph is symmetric)
//   the update and the verdict (mgx/pagerank_fused.hpp), then the control block to the host: e, D, done.
// Two host waits per iteration (the operator's, the look): `waits` counts them.
#pragma once
#include "../enactor.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "../neighborhood.hxx"
#include "pagerank_functor.hxx"
#include "pagerank_problem.hxx"

namespace gunrock {
namespace pagerank {

struct pagerank_enactor_t : enactor_t {
  long long waits = 0, launches = 0;

  // (no edge-capacity frontiers: the loop has no output frontier)
  pagerank_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges)
      : enactor_t(ctx, num_nodes, num_edges, 0.0f), unused_output(std::make_shared<frontier_t<int>>(ctx, (size_t)1)) {}
  pagerank_enactor_t(const pagerank_enactor_t&) = delete;
  pagerank_enactor_t& operator=(const pagerank_enactor_t&) = delete;

  mgx::pagerank_stats_t enact(std::shared_ptr<pagerank_problem_t> problem, double alpha, double tol, int max_iter, standard_context_t& ctx) {
    namespace nb = gunrock::oprtr::neighborhood;
    mgx::pagerank_state_t& s = problem->state;
    mgx::pagerank_stats_t out;
    const int n = problem->gslice->num_nodes;
    waits = launches = 0;
    if (n <= 0) { out.converged = 1; return out; }
    const int* const off = problem->gslice->d_row_offsets.data();
    frontier_ptr& everyone = indices;              // 0 .. n - 1, never written
    everyone->resize((size_t)n);
    launches += s.begin(off, alpha, tol, max_iter, ctx);
    for (int it = 0;; ++it) {
      nb::neighborhood_kernel<pagerank_problem_t, pagerank_functor_t, float, mgx::plus_t<float>, false, false>(
          problem, everyone, unused_output, s.S.data(), 0.0f, it, ctx);
      launches += s.step(off, ctx);
      const mgx::pagerank_ctrl_t& c = s.look(ctx);
      waits += 2;
      if (c.done) {
        out.iterations = c.iterations; out.converged = c.converged; out.dangling = c.dangling; out.residual = c.e;
        break;
      }
    }
    s.last_iterations = (int)out.iterations;
    s.result = s.rank.data();
    out.waits = waits; out.launches = launches;
    return out;
  }

 private:
  std::shared_ptr<frontier_t<int>> unused_output;   // the operator's signature wants an output frontier
};

}  // namespace pagerank
}  // namespace gunrock
