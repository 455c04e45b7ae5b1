// gunrock/louvain/louvain_problem.hxx -- state of the Louvain run the operator path makes (mgx_louvain_enact).  One
// state, seen through a view per level graph: the forward view reads the level's graph (level 0: the caller's; coarse: the
// contraction's weighted CSR, borrowed), the backward view of level 0 the genuine CSC's arrays borrowed as a graph's CSR
// (symmetric == 0 only), as lpa_problem_t has them.  Only the contraction (mgx/louvain_aggregate.hpp) is shared with the fused path.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace louvain {

constexpr int LV_OP_NONE = 0x7fffffff;        // a gathered slot that carries no vote (a self entry): sorts behind every label

struct louvain_scalars_t {
  unsigned seed;
  int pad;
  long long w;                                 // the sum of all k
  unsigned long long s_in, s_sq;               // of the labels the last Qnum sweep read
};

struct louvain_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* d_row_offsets;  // the level's CSR
    const int* d_col_offsets;  // level 0's genuine CSC (symmetric == 0 only, else null)
    const unsigned* d_weights; // the level's weights (null: level 0, every entry weighs 1)
    int* d_heads;              // n + 1: where every vertex's votes begin
    int* d_votes;              // the label every vote carries, a segment per vertex: its out-entries, then its in-entries
    unsigned* d_vote_w;        // ... and its weight
    int* d_label;
    int* d_best;
    unsigned* d_sigma;
    unsigned* d_k;
    louvain_scalars_t* d_scalars;
  };

  mem_t<data_slice_t> d_data_slice;

  // a view of the caller's graph
  louvain_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  // a view of borrowed CSR arrays: the genuine CSC of level 0, or a coarse level's graph
  louvain_problem_t(const data_slice_t& slice, const int* offsets, const int* indices, int num_nodes, int num_edges,
                    standard_context_t& ctx)
      : problem_t() {
    graph_device_t& g = *gslice;
    g.num_nodes = num_nodes;
    g.num_edges = num_edges;
    g.d_row_offsets = mem_t<int>::borrow(const_cast<int*>(offsets), (size_t)num_nodes + 1);
    g.d_col_indices = mem_t<int>::borrow(const_cast<int*>(indices), (size_t)num_edges);
    g.d_col_offsets = mem_t<int>::borrow(const_cast<int*>(offsets), (size_t)num_nodes + 1);
    g.d_row_indices = mem_t<int>::borrow(const_cast<int*>(indices), (size_t)num_edges);
    g.csc_is_csr = true;
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  louvain_problem_t(const louvain_problem_t&) = delete;
  louvain_problem_t& operator=(const louvain_problem_t&) = delete;
};

// the arrays every view points at, sized for level 0
struct louvain_state_t {
  mem_t<int> d_heads, d_votes, d_label, d_best, d_old, d_final, d_maps;
  mem_t<unsigned> d_vote_w, d_sigma, d_sigma_old, d_k;
  mem_t<int> cro[2], cci[2];
  mem_t<unsigned> cwt[2];
  mem_t<louvain_scalars_t> d_scalars;
  louvain_state_t(int num_nodes, long long entries, standard_context_t& ctx) {
    const size_t N = (size_t)std::max(num_nodes, 1), E = (size_t)std::max<long long>(entries, 1);
    d_heads = mem_t<int>(N + 1, ctx);
    d_votes = mem_t<int>(E, ctx);
    d_vote_w = mem_t<unsigned>(E, ctx);
    d_label = mem_t<int>(N, ctx);
    d_best = mem_t<int>(N, ctx);
    d_old = mem_t<int>(N, ctx);
    d_final = mem_t<int>(N, ctx);
    d_maps = mem_t<int>(2 * N, ctx);
    d_sigma = mem_t<unsigned>(N, ctx);
    d_sigma_old = mem_t<unsigned>(N, ctx);
    d_k = mem_t<unsigned>(N, ctx);
    for (int i = 0; i < 2; ++i) {
      cro[i] = mem_t<int>(N + 1, ctx);
      cci[i] = mem_t<int>(E, ctx);
      cwt[i] = mem_t<unsigned>(E, ctx);
    }
    d_scalars = mem_t<louvain_scalars_t>(1, ctx);
  }
};

}  // namespace louvain
}  // namespace gunrock
