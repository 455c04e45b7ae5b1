// gunrock/ktruss/ktruss_problem.hxx -- state of the k-truss decomposition the operator path runs (mgx_ktruss_enact).
// The graph the problem reads is the oriented graph (DAG) of the triangle count, borrowed as a graph_device_t as tc_problem_t
// borrows it: the advance over it computes the supports.  The peel's frontiers hold EDGE ids (positions of the DAG's entries); its
// functors reach the adjacency with edge ids, the supports, the states and the results of mgx/ktruss_fused.hpp through a
// one-element data_slice_t in device memory.  Both builds are the fused path's; none of its peel kernels is used.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace ktruss {

struct ktruss_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* d_row_offsets;  // the DAG
    const int* d_col_indices;
    const int* d_src;          // row of every DAG entry
    const int* d_adj_ro;       // the simple adjacency, rows ascending by neighbour, with the DAG position of every entry's edge
    const int* d_adj_ci;
    const int* d_adj_eid;
    int* d_sup0;
    int* d_sup;
    int* d_state;
    int* d_truss;
    int* d_vtruss;
    int* d_hist;
  };

  mem_t<data_slice_t> d_data_slice;

  ktruss_problem_t(const data_slice_t& slice, int num_nodes, int num_dag_edges, standard_context_t& ctx) : problem_t() {
    graph_device_t& g = *gslice;
    g.num_nodes = num_nodes;
    g.num_edges = num_dag_edges;
    g.d_row_offsets = mem_t<int>::borrow(const_cast<int*>(slice.d_row_offsets), (size_t)num_nodes + 1);
    g.d_col_indices = mem_t<int>::borrow(const_cast<int*>(slice.d_col_indices), (size_t)num_dag_edges);
    g.d_col_offsets = mem_t<int>::borrow(const_cast<int*>(slice.d_row_offsets), (size_t)num_nodes + 1);
    g.d_row_indices = mem_t<int>::borrow(const_cast<int*>(slice.d_col_indices), (size_t)num_dag_edges);
    g.csc_is_csr = true;
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  ktruss_problem_t(const ktruss_problem_t&) = delete;
  ktruss_problem_t& operator=(const ktruss_problem_t&) = delete;
};

}  // namespace ktruss
}  // namespace gunrock
