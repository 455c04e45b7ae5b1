// gunrock/coloring/coloring_enactor.hxx -- graph colouring on the neighbourhood-reduce and filter operators
// (mgx_color_enact): the slow, faithful path, and the fused path's cross-check and baseline.  What the reference's
// coloring_enactor_t::enact does (gunrock/src/coloring/coloring_enactor.hxx), per round while vertices are left and
// iteration < max_iter:
//   neighborhood<reduce_max_t, maximum_t<int>, has_output = false, push = true>   over the iota frontier
//   neighborhood<reduce_min_t, minimum_t<int>, false, true>                       over the iota frontier
//   filter<coloring_functor_t>   over the active vertices: colours them or keeps them for the next round
//   reset_hashs                  the next round's keys
// Upstream passes five template arguments to the six-argument neighborhood_kernel and does not compile; here all six are
// given.  max_iter <= 0 runs until no vertex is left (upstream: no round at all).
#pragma once
#include <climits>

#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "../neighborhood.hxx"
#include "coloring_functor.hxx"
#include "coloring_problem.hxx"

namespace gunrock {
namespace coloring {

struct coloring_enactor_t : enactor_t {
  // what the last enact() did: rounds, vertices left uncoloured, largest colour, host waits; active vertices per round
  long long rounds = 0, left = 0, largest = 0, waits = 0;
  std::vector<long long> trace;
  frontier_ptr active_next;                       // the second active buffer (node capacity: upstream's buffers are m)

  coloring_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges) {
    active_next = std::make_shared<frontier_t<int>>(ctx, (size_t)num_nodes);
  }
  coloring_enactor_t(const coloring_enactor_t&) = delete;
  coloring_enactor_t& operator=(const coloring_enactor_t&) = delete;

  void enact(std::shared_ptr<coloring_problem_t> problem, standard_context_t& ctx) {
    namespace nb = gunrock::oprtr::neighborhood;
    namespace fl = gunrock::oprtr::filter;
    const int n = problem->gslice->num_nodes;
    problem->reset(ctx);
    frontier_ptr& everyone = indices;             // 0 .. n - 1, never written
    (void)filtered_indices->load(*everyone->data());
    frontier_ptr active[2] = {filtered_indices, active_next};
    active[0]->resize((size_t)n);
    rounds = waits = largest = 0;
    trace.clear();
    long long length = n;
    const long long limit = problem->max_iter > 0 ? problem->max_iter : LLONG_MAX;
    int* const reduced_max = problem->d_reduced_max.data();
    int* const reduced_min = problem->d_reduced_min.data();
    int selector = 0;
    for (int iteration = 0; length > 0 && iteration < limit; ++iteration) {
      trace.push_back(length);
      if (iteration > 0) problem->reset_hashs(iteration, ctx);
      const int edges = nb::neighborhood_kernel<coloring_problem_t, reduce_max_t, int, mgpu::maximum_t<int>, false, true>(
          problem, everyone, everyone, reduced_max, INT_MIN, iteration, ctx);
      nb::neighborhood_kernel<coloring_problem_t, reduce_min_t, int, mgpu::minimum_t<int>, false, true>(
          problem, everyone, everyone, reduced_min, INT_MAX, iteration, ctx);
      if (edges == 0)                             // (no entries at all: the operator leaves the results unwritten)
        transform([=] __device__(int v) { reduced_max[v] = INT_MIN; reduced_min[v] = INT_MAX; }, n, ctx);
      length = fl::filter_kernel<coloring_problem_t, coloring_functor_t>(problem, active[selector], active[selector ^ 1], iteration, ctx);
      waits += 3;                                 // each operator reads its count back
      selector ^= 1;
      ++rounds;
    }
    left = length;
    // every round colours its smallest and largest key: the last round's colours are the largest; one count says which
    if (rounds > 0) {
      const int top = (int)(2 * rounds);
      const int* const colors = problem->d_colors.data();
      auto counter = mgx::transform_compact((long long)n, ctx);
      const long long at_top = counter.upsweep([=] __device__(long long v) { return colors[v] == top; });
      ++waits;
      largest = at_top ? top : top - 1;
    }
  }
};

}  // namespace coloring
}  // namespace gunrock
