// gunrock/aggbwd/aggbwd_problem.hxx -- what the backward aggregation's operator path runs on (mgx_aggbwd_enact): the
// forward CSR, the transposed arrays the fused path runs on as well, the gradients and the winners of one call.  Nothing here is
// state: the slice is uploaded anew for every call.
#pragma once
#include "../../mgx/agg_backward.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace aggbwd {

struct aggbwd_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* t_off;          // x_rows + 1 offsets of the transposed rows
    const int* t_row;          // the forward row of a slot
    const int* t_pos;          // the forward entry of a slot
    const int* ro;             // the forward rows: R + 1 offsets, absolute places in ci
    const int* ci;
    const int* entry_pos;      // a block's: the place of entry e in the graph's weights (NULL: e itself)
    const float* w;            // NULL: unweighted
    const float* gy;
    const float* x;            // max / min only
    float* gx;
    int* win;                  // R x ldw, max / min only
    long long ldgy, ldx, ldgx, ldw;
    int feats, op, seg;
  };

  mem_t<data_slice_t> d_data_slice;

  aggbwd_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  aggbwd_problem_t(const aggbwd_problem_t&) = delete;
  aggbwd_problem_t& operator=(const aggbwd_problem_t&) = delete;
};

}  // namespace aggbwd
}  // namespace gunrock
