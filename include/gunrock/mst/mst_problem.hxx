// gunrock/mst/mst_problem.hxx -- state of the minimum spanning forest the operator path builds (mgx_mst_enact).
//   d_comp    the pointer every vertex hangs under: hooks and pointer jumping write it
//   d_root    the roots as the last round left them, read-only while a round decides; at the end: the labels (the smallest id of
//             every vertex's component)
//   d_cw      per root: key(w) of the component's lightest outgoing edge of this round (mgx/mst_fused.hpp: mst_key)
//   d_cp      per root: its (min << 32 | max)
//   d_min     the smallest id per final root (the relabelling)
//   d_a / d_b / d_w_out   the chosen edges in the order the hook filter's roots appended them (n entries of room)
//   d_counters  [0] edges appended, [1] incident entries (no self-loops; both ends' when symmetric == 0), [2] NaN weights
// The functors see them through a one-element data_slice_t in device memory, as the other problems' do.
#pragma once
#include "../../mgx/mst_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace mst {

struct mst_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    int* d_comp;
    int* d_root;
    unsigned* d_cw;
    unsigned long long* d_cp;
    const float* d_w;          // the CSR's weights, by entry
    int* d_a;
    int* d_b;
    float* d_w_out;
    unsigned long long* d_counters;
    int symmetric;
    int cap;
  };

  mem_t<int> d_comp, d_root, d_min, d_a, d_b;
  mem_t<unsigned> d_cw;
  mem_t<unsigned long long> d_cp, d_counters;
  mem_t<float> d_w_out;
  mem_t<data_slice_t> d_data_slice;

  mst_problem_t(std::shared_ptr<graph_device_t> graph, standard_context_t& ctx) : problem_t(graph) {
    const size_t N = (size_t)std::max(gslice->num_nodes, 1);
    d_comp = mem_t<int>(N, ctx); d_root = mem_t<int>(N, ctx); d_min = mem_t<int>(N, ctx);
    d_a = mem_t<int>(N, ctx); d_b = mem_t<int>(N, ctx);
    d_cw = mem_t<unsigned>(N, ctx);
    d_cp = mem_t<unsigned long long>(N, ctx);
    d_counters = mem_t<unsigned long long>(4, ctx);
    d_w_out = mem_t<float>(N, ctx);
    d_data_slice = mem_t<data_slice_t>(1, ctx);
  }
  mst_problem_t(const mst_problem_t&) = delete;
  mst_problem_t& operator=(const mst_problem_t&) = delete;

  // every vertex its own tree, no edge chosen (the slice is uploaded: the copy returns when it has arrived)
  void reset(bool symmetric, standard_context_t& ctx) {
    const data_slice_t s{d_comp.data(), d_root.data(), d_cw.data(), d_cp.data(), gslice->d_col_values.data(), d_a.data(), d_b.data(),
                         d_w_out.data(), d_counters.data(), symmetric ? 1 : 0, gslice->num_nodes};
    MGX_HIP(htod(d_data_slice.data(), &s, 1, ctx.stream()));
    MGX_HIP(hipMemsetAsync(d_counters.data(), 0, 4 * sizeof(unsigned long long), ctx.stream()));
    int* const comp = d_comp.data();
    int* const root = d_root.data();
    transform([=] __device__(int v) { comp[v] = v; root[v] = v; }, gslice->num_nodes, ctx);
  }
};

}  // namespace mst
}  // namespace gunrock
