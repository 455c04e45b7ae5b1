// gunrock/bc/bc_problem.hxx -- state of the betweenness centrality the operator path runs (mgx_bc_enact).
// The arrays are the handle's own (mgx/bc_fused.hpp keeps them, the result calls read them whichever path ran): labels (BFS depth,
// -1 unreached), sigma (shortest entry-paths from the source), delta (the source's dependencies), all by original id.  The functors
// see them through a one-element data_slice_t in device memory, as the other problems' do.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace bc {

struct bc_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    int* d_labels;
    double* d_sigma;
    double* d_delta;
  };

  int* labels;
  double* sigma;
  double* delta;
  mem_t<data_slice_t> d_data_slice;

  bc_problem_t(std::shared_ptr<graph_device_t> graph, int* labels_, double* sigma_, double* delta_, standard_context_t& ctx)
      : problem_t(graph), labels(labels_), sigma(sigma_), delta(delta_) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{labels_, sigma_, delta_}), ctx);
  }
  bc_problem_t(const bc_problem_t&) = delete;
  bc_problem_t& operator=(const bc_problem_t&) = delete;
};

}  // namespace bc
}  // namespace gunrock
