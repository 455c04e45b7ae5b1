// gunrock/lpa/lpa_enactor.hxx -- label propagation on the advance and filter operators and the library's segmented sort
// (mgx_lpa_enact): the plain path, the fused path's cross-check and yardstick.  Every vertex every iteration:
//   advance<gather_out>             over the iota frontier: every vote's label into its vertex's segment of the votes
//   advance<gather_in>              over the backward view, when the graph is not symmetric
//   segmented_sort(votes, heads)    every vertex's votes ascending
//   filter<want>                    run-length scan per vertex; keeps the unstable: its count is unstable_t
//   filter<apply>  (iteration = t)  over the unstable: the movers take their label; its count is what changed
#pragma once
#include <vector>

#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "../moderngpu/kernel_segsort.hxx"
#include "lpa_functor.hxx"
#include "lpa_problem.hxx"

namespace gunrock {
namespace lpa {

struct lpa_enactor_t : enactor_t {
  // what the last enact() did
  long long iterations = 0, converged = 0, unstable = 0, waits = 0, calls = 0;
  std::vector<long long> trace;                   // (unstable, changed, evaluated) per iteration

  // (the advances write no frontier; the second buffer takes the movers)
  lpa_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {
    buffers[1] = std::make_shared<frontier_t<int>>(ctx, (size_t)std::max(num_nodes, 1));
  }
  lpa_enactor_t(const lpa_enactor_t&) = delete;
  lpa_enactor_t& operator=(const lpa_enactor_t&) = delete;

  template <typename F>
  int filter(std::shared_ptr<lpa_problem_t>& p, frontier_ptr& in, frontier_ptr& out, int iteration, standard_context_t& ctx) {
    ++waits; ++calls;
    return gunrock::oprtr::filter::filter_kernel<lpa_problem_t, F>(p, in, out, iteration, ctx);
  }

  void enact(std::shared_ptr<lpa_problem_t> fwd, std::shared_ptr<lpa_problem_t> bwd, lpa_state_t& state, bool symmetric, int mode,
             unsigned seed, int max_iter, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    const int n = fwd->gslice->num_nodes;
    const long long m = fwd->gslice->num_edges;
    const long long votes = symmetric ? m : 2 * m;
    iterations = converged = unstable = waits = calls = 0;
    trace.clear();
    indices->resize((size_t)n);                   // 0 .. n - 1, never written
    lpa_scalars_t* const scalars = state.d_scalars.data();
    int* const label = state.d_label.data();
    int* const heads = state.d_heads.data();
    const int* const ro = fwd->gslice->d_row_offsets.data();
    const int* const co = symmetric ? nullptr : bwd->gslice->d_row_offsets.data();
    transform([=] __device__(int) { scalars->seed = seed; scalars->mode = mode; scalars->symmetric = symmetric ? 1 : 0; }, 1, ctx);
    transform([=] __device__(int v) {
      if (v < n) label[v] = v;
      heads[v] = ro[v] + (co ? co[v] : 0);
    }, (long long)n + 1, ctx);
    frontier_ptr nobody = buffers[0];
    for (int t = 0;; ++t) {
      adv::advance_forward_kernel<lpa_problem_t, gather_out_functor_t, /*idempotence=*/false, /*has_output=*/false>(fwd, indices, nobody, t, ctx);
      ++waits; ++calls;
      if (!symmetric) {
        adv::advance_forward_kernel<lpa_problem_t, gather_in_functor_t, false, false>(bwd, indices, nobody, t, ctx);
        ++waits; ++calls;
      }
      if (votes >= 2) {
        auto ascending = [] MGPU_DEVICE(int left, int right) { return left < right; };
        mgpu::segmented_sort(state.d_votes.data(), votes, (const int*)heads, n, ascending, ctx);
        waits += 2; ++calls;
      }
      const int unst = filter<want_functor_t>(fwd, indices, filtered_indices, t, ctx);
      iterations = t;
      unstable = unst;
      trace.push_back(unst); trace.push_back(0); trace.push_back(n);
      if (unst == 0 || t >= max_iter) break;
      const int changed = filter<apply_functor_t>(fwd, filtered_indices, buffers[1], t, ctx);
      trace[trace.size() - 2] = changed;
    }
    converged = unstable == 0 ? 1 : 0;
  }
};

}  // namespace lpa
}  // namespace gunrock
