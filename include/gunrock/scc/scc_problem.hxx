// gunrock/scc/scc_problem.hxx -- state of the strongly connected components the operator path runs (mgx_scc_enact).
// Two views of one state: the forward problem reads the graph itself (arcs v -> u are its CSR entries), the backward problem a
// graph_device_t that borrows the genuine CSC's arrays in the CSR's places, as tc_problem_t and ktruss_problem_t borrow the
// oriented graph -- an advance over it walks the in-entries.  Both hand their functors the same arrays through a one-element
// data_slice_t in device memory.  Nothing here is shared with the fused path (mgx/scc_fused.hpp).
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace scc {

enum : int { SCC_OP_ALIVE = 0, SCC_OP_DOOMED = 1, SCC_OP_REMOVED = 2 };
constexpr int SCC_OP_NONE = 0x7fffffff;        // col of a vertex the pivot has not reached

struct scc_scalars_t {
  unsigned long long best;     // the pivot filters: the largest outdeg * indeg of an alive vertex
  int pivot;                   //                    the smallest id that has it
  int pivot_min;               // the smallest id of the pivot's component
};

struct scc_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* d_row_offsets;  // the CSR
    const int* d_col_indices;
    const int* d_col_offsets;  // the genuine CSC
    const int* d_row_indices;
    int* d_state;
    int* d_col;
    int* d_claim;              // the tag of the round that claimed the vertex
    int* d_label;
    scc_scalars_t* d_scalars;
  };

  mem_t<data_slice_t> d_data_slice;

  // the forward view: the graph as it is
  scc_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  // the backward view: the CSC's arrays as a graph's CSR
  scc_problem_t(const data_slice_t& slice, int num_nodes, int num_edges, standard_context_t& ctx) : problem_t() {
    graph_device_t& g = *gslice;
    g.num_nodes = num_nodes;
    g.num_edges = num_edges;
    g.d_row_offsets = mem_t<int>::borrow(const_cast<int*>(slice.d_col_offsets), (size_t)num_nodes + 1);
    g.d_col_indices = mem_t<int>::borrow(const_cast<int*>(slice.d_row_indices), (size_t)num_edges);
    g.d_col_offsets = mem_t<int>::borrow(const_cast<int*>(slice.d_col_offsets), (size_t)num_nodes + 1);
    g.d_row_indices = mem_t<int>::borrow(const_cast<int*>(slice.d_row_indices), (size_t)num_edges);
    g.csc_is_csr = true;
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  scc_problem_t(const scc_problem_t&) = delete;
  scc_problem_t& operator=(const scc_problem_t&) = delete;
};

// the arrays both views point at
struct scc_state_t {
  mem_t<int> d_state, d_col, d_claim, d_label;
  mem_t<scc_scalars_t> d_scalars;
  scc_state_t(int num_nodes, standard_context_t& ctx) {
    const size_t N = (size_t)std::max(num_nodes, 1);
    d_state = mem_t<int>(N, ctx);
    d_col = mem_t<int>(N, ctx);
    d_claim = mem_t<int>(N, ctx);
    d_label = mem_t<int>(N, ctx);
    d_scalars = mem_t<scc_scalars_t>(1, ctx);
  }
  // everybody alive, nobody claimed (asynchronous on the context's stream)
  void reset(int num_nodes, standard_context_t& ctx) {
    int* const state = d_state.data();
    int* const claim = d_claim.data();
    transform([=] __device__(int v) { state[v] = SCC_OP_ALIVE; claim[v] = 0; }, num_nodes, ctx);
  }
};

}  // namespace scc
}  // namespace gunrock
