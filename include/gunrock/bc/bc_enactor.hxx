// gunrock/bc/bc_enactor.hxx -- betweenness centrality on the operators (mgx_bc_enact): the plain path, the fused path's cross-check
// and baseline.  Per source:
//   forward    advance<bc_forward_functor_t> + filter per level; the frontiers are kept one after the other in ONE n-sized buffer
//              with their offsets (every reached vertex is in exactly one of them)
//   backward   one advance<bc_backward_functor_t, has_output = false> per level over the stored frontier, deepest - 1 down to 1
//              (the source's own level is left out: delta[s] is not part of the centrality)
// It needs no CSC.  Every operator call reads its count back: `waits` counts them.
#pragma once
#include <vector>
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "bc_functor.hxx"
#include "bc_problem.hxx"

namespace gunrock {
namespace bc {

struct bc_enactor_t : enactor_t {
  long long waits = 0;
  mem_t<int> levels_buf;                 // the frontiers of the levels 0, 1, .. back to back
  std::vector<size_t> level_off;         // level d is [level_off[d], level_off[d + 1])
  frontier_ptr level;                    // the stored frontier the backward advance reads

  bc_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges > 0 ? num_edges : 1) {
    levels_buf = mem_t<int>((size_t)(num_nodes > 0 ? num_nodes : 1), ctx);
    level = std::make_shared<frontier_t<int>>(ctx, (size_t)(num_nodes > 0 ? num_nodes : 1));
  }
  bc_enactor_t(const bc_enactor_t&) = delete;
  bc_enactor_t& operator=(const bc_enactor_t&) = delete;

  // labels, sigma and delta of one source (the arrays are reset here); returns the number of levels
  int enact(std::shared_ptr<bc_problem_t> problem, int src, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    namespace flt = gunrock::oprtr::filter;
    const size_t n = (size_t)problem->gslice->num_nodes;
    const hipStream_t st = ctx.stream();
    int* const labels = problem->labels;
    double* const sigma = problem->sigma;
    MGX_HIP(hipMemsetAsync(labels, 0xFF, n * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(sigma, 0, n * sizeof(double), st));
    MGX_HIP(hipMemsetAsync(problem->delta, 0, n * sizeof(double), st));
    mgx::transform([=] __device__(int) { labels[src] = 0; sigma[src] = 1.0; }, 1, ctx);
    (void)buffers[0]->load(std::vector<int>(1, src));
    MGX_HIP(mgx::dtod(levels_buf.data(), buffers[0]->data()->data(), 1, st));
    level_off.assign({0, 1});
    int selector = 0;
    for (int iteration = 0;; ++iteration) {
      int len = adv::advance_forward_kernel<bc_problem_t, bc_forward_functor_t, false, true>(problem, buffers[selector], buffers[selector ^ 1],
                                                                                            iteration, ctx);
      ++waits;
      selector ^= 1;
      if (!len) break;
      len = flt::filter_kernel<bc_problem_t, bc_forward_functor_t>(problem, buffers[selector], buffers[selector ^ 1], iteration, ctx);
      ++waits;
      if (!len) break;
      selector ^= 1;
      MGX_HIP(mgx::dtod(levels_buf.data() + level_off.back(), buffers[selector]->data()->data(), (size_t)len, st));
      level_off.push_back(level_off.back() + (size_t)len);
    }
    const int levels = (int)level_off.size() - 1;
    for (int d = levels - 2; d >= 1; --d) {
      const size_t len = level_off[(size_t)d + 1] - level_off[(size_t)d];
      level->resize(len);
      mgx::frontier_touched();
      MGX_HIP(mgx::dtod(level->data()->data(), levels_buf.data() + level_off[(size_t)d], len, st));
      adv::advance_forward_kernel<bc_problem_t, bc_backward_functor_t, false, false>(problem, level, buffers[0], d, ctx);
      ++waits;
    }
    return levels;
  }
};

}  // namespace bc
}  // namespace gunrock
