// gunrock/cc/cc_problem.hxx -- state of the connected components the operator path runs (mgx_cc_enact).
// One array: comp[v], the label v hangs under.  It starts as the identity, only ever decreases and always names a vertex of v's
// component; when the enactor stops it is the definition's label: the smallest id of v's component.  The functors
// see it through a one-element data_slice_t in device memory, as the other problems' do.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace cc {

struct cc_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    int* d_comp;
  };

  mem_t<int> d_comp;
  mem_t<data_slice_t> d_data_slice;

  cc_problem_t(std::shared_ptr<graph_device_t> graph, standard_context_t& ctx) : problem_t(graph) {
    d_comp = mem_t<int>((size_t)std::max(graph->num_nodes, 1), ctx);
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{d_comp.data()}), ctx);
    reset(ctx);
  }
  cc_problem_t(const cc_problem_t&) = delete;
  cc_problem_t& operator=(const cc_problem_t&) = delete;

  // every vertex its own label (asynchronous on the context's stream)
  void reset(standard_context_t& ctx) {
    int* const comp = d_comp.data();
    transform([=] __device__(int v) { comp[v] = v; }, gslice->num_nodes, ctx);
  }
};

}  // namespace cc
}  // namespace gunrock
