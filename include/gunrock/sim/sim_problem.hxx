// gunrock/sim/sim_problem.hxx -- state of the vertex similarity the operator path runs (mgx_sim_enact): a view of the
// sorted simple adjacency the fused path's handle keeps, the pairs, and the results' arrays (mgx/sim_fused.hpp: sim_results_t).
#pragma once
#include "../../mgx/sim_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace sim {

struct sim_problem_t : problem_t {
  struct data_slice_t {        // what the functor dereferences on the device
    const int* ro;             // the adjacency
    const int* ci;
    const int* u;              // the pairs
    const int* v;
    const double* x;           // WEIGHTED: n doubles; else NULL
    int* d_common;
    double* d_score;
    unsigned long long* d_sums;  // [0] the sum of c, [1] 1 once an id was outside [0, n)
    int n, measure;
  };

  mem_t<data_slice_t> d_data_slice;

  sim_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  sim_problem_t(const sim_problem_t&) = delete;
  sim_problem_t& operator=(const sim_problem_t&) = delete;
};

}  // namespace sim
}  // namespace gunrock
