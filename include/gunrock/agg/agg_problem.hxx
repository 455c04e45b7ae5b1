// gunrock/agg/agg_problem.hxx -- what the neighbour feature aggregation's operator path runs on (mgx_agg_enact): the
// CSR, the features and the result of one call.  Nothing here is state: the slice is uploaded anew for every call.
#pragma once
#include "../../mgx/agg_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace agg {

struct agg_problem_t : problem_t {
  struct data_slice_t {        // what the functor dereferences on the device
    const int* ro;             // R + 1 offsets, absolute places in ci
    const int* ci;
    const int* entry_pos;      // a block's: the place of entry e in the graph's weights (NULL: e itself)
    const float* w;            // NULL: unweighted
    const float* x;
    float* y;
    long long ldx, ldy;
    int feats, op, seg;
  };

  mem_t<data_slice_t> d_data_slice;

  agg_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  agg_problem_t(const agg_problem_t&) = delete;
  agg_problem_t& operator=(const agg_problem_t&) = delete;
};

}  // namespace agg
}  // namespace gunrock
