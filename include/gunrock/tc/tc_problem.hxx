// gunrock/tc/tc_problem.hxx -- state of the triangle count the operator path runs (mgx_tc_enact).
// The graph the problem reads is not the caller's: it is the oriented graph (DAG) mgx/tc_fused.hpp built from it, wrapped as a
// graph_device_t that borrows the DAG's arrays (as the graph of lspar's result does): row a = the distinct neighbours of a of
// higher rank, ascending.  tri[v] (64 bits) is the per-vertex count both paths add into.  The functor sees them through a
// one-element data_slice_t in device memory, as the other problems' do.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace tc {

struct tc_problem_t : problem_t {
  struct data_slice_t {        // what the functor dereferences on the device
    const int* d_row_offsets;
    const int* d_col_indices;
    unsigned long long* d_tri;
  };

  mem_t<data_slice_t> d_data_slice;

  tc_problem_t(const int* dag_ro, const int* dag_ci, int num_nodes, int num_dag_edges, unsigned long long* tri,
               standard_context_t& ctx) : problem_t() {
    graph_device_t& g = *gslice;
    g.num_nodes = num_nodes;
    g.num_edges = num_dag_edges;
    g.d_row_offsets = mem_t<int>::borrow(const_cast<int*>(dag_ro), (size_t)num_nodes + 1);
    g.d_col_indices = mem_t<int>::borrow(const_cast<int*>(dag_ci), (size_t)num_dag_edges);
    g.d_col_offsets = mem_t<int>::borrow(const_cast<int*>(dag_ro), (size_t)num_nodes + 1);
    g.d_row_indices = mem_t<int>::borrow(const_cast<int*>(dag_ci), (size_t)num_dag_edges);
    g.csc_is_csr = true;
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{dag_ro, dag_ci, tri}), ctx);
  }
  tc_problem_t(const tc_problem_t&) = delete;
  tc_problem_t& operator=(const tc_problem_t&) = delete;
};

}  // namespace tc
}  // namespace gunrock
