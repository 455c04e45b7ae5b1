// gunrock/lpa/lpa_problem.hxx -- state of the label propagation the operator path runs (mgx_lpa_enact).  Two views
// of one state, as scc_problem_t has them: the forward problem reads the graph itself, the backward problem a graph_device_t that
// borrows the genuine CSC's arrays in the CSR's places, so that an advance over it walks the in-entries (symmetric == 0 only).
// Nothing here is shared with the fused path (mgx/lpa_fused.hpp).
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace lpa {

constexpr int LPA_OP_NONE = 0x7fffffff;       // a gathered slot that carries no vote (a self-loop): sorts behind every label

struct lpa_scalars_t {
  unsigned seed;
  int mode;                    // 0: every unstable vertex moves; 1: those whose key of the iteration is odd
  int symmetric;
};

struct lpa_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* d_row_offsets;  // the CSR
    const int* d_col_offsets;  // the genuine CSC (read when symmetric == 0 only)
    int* d_heads;              // n + 1: where every vertex's votes begin in d_votes
    int* d_votes;              // the label every vote carries, a segment per vertex: its out-entries, then its in-entries
    int* d_label;
    int* d_want;
    lpa_scalars_t* d_scalars;
  };

  mem_t<data_slice_t> d_data_slice;

  // the forward view: the graph as it is
  lpa_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  // the backward view: the CSC's arrays as a graph's CSR
  lpa_problem_t(const data_slice_t& slice, const int* col_offsets, const int* row_indices, int num_nodes, int num_edges,
                standard_context_t& ctx)
      : problem_t() {
    graph_device_t& g = *gslice;
    g.num_nodes = num_nodes;
    g.num_edges = num_edges;
    g.d_row_offsets = mem_t<int>::borrow(const_cast<int*>(col_offsets), (size_t)num_nodes + 1);
    g.d_col_indices = mem_t<int>::borrow(const_cast<int*>(row_indices), (size_t)num_edges);
    g.d_col_offsets = mem_t<int>::borrow(const_cast<int*>(col_offsets), (size_t)num_nodes + 1);
    g.d_row_indices = mem_t<int>::borrow(const_cast<int*>(row_indices), (size_t)num_edges);
    g.csc_is_csr = true;
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  lpa_problem_t(const lpa_problem_t&) = delete;
  lpa_problem_t& operator=(const lpa_problem_t&) = delete;
};

// the arrays both views point at
struct lpa_state_t {
  mem_t<int> d_heads, d_votes, d_label, d_want;
  mem_t<lpa_scalars_t> d_scalars;
  lpa_state_t(int num_nodes, long long num_edges, standard_context_t& ctx) {
    const size_t N = (size_t)std::max(num_nodes, 1);
    d_heads = mem_t<int>(N + 1, ctx);
    d_votes = mem_t<int>((size_t)std::max<long long>(2 * num_edges, 1), ctx);
    d_label = mem_t<int>(N, ctx);
    d_want = mem_t<int>(N, ctx);
    d_scalars = mem_t<lpa_scalars_t>(1, ctx);
  }
};

}  // namespace lpa
}  // namespace gunrock
