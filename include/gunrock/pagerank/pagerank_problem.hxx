// gunrock/pagerank/pagerank_problem.hxx -- state of the PageRank the operator path runs (mgx_pagerank_enact).
// The arrays -- ranks, contributions r / d, the reduced sums S, all float and by vertex id -- and the control block (dangling mass,
// residuals, iteration count) are those of mgx::pagerank_state_t (mgx/pagerank_fused.hpp): the two paths share the update and
// the verdict and differ in the reduce and in who drives the loop.  The functor sees the contributions through a one-element
// data_slice_t in device memory, as the other problems' do.
#pragma once
#include "../../mgx/pagerank_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace pagerank {

struct pagerank_problem_t : problem_t {
  struct data_slice_t {        // what the functor dereferences on the device
    const float* d_contrib;
  };

  mgx::pagerank_state_t state;
  mem_t<data_slice_t> d_data_slice;

  pagerank_problem_t(std::shared_ptr<graph_device_t> graph, standard_context_t& ctx) : problem_t(graph), state(graph->num_nodes, ctx) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{state.contrib.data()}), ctx);
  }
  pagerank_problem_t(const pagerank_problem_t&) = delete;
  pagerank_problem_t& operator=(const pagerank_problem_t&) = delete;
};

}  // namespace pagerank
}  // namespace gunrock
