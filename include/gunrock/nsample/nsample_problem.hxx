// gunrock/nsample/nsample_problem.hxx -- state of the neighbour sampling the operator path runs (mgx_nsample_enact):
// a local id and a mark per vertex, cleared per run, and the results' arrays (mgx/nsample_fused.hpp: ns_results_t), sized by the
// same bounds as the fused path's.
#pragma once
#include "../../mgx/nsample_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace nsample {

struct nsample_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    const int* ro;
    const int* ci;
    int* d_local;              // n: a vertex's local id, -1 before it has one
    int* d_mark;               // n: 1 once a sampled entry points at the vertex
    int* d_row_offsets;        // a hop's rows hold their prefix inside the hop until the sample adds the entries before it
    int* d_cols;               // global ids until the run's last transform
    int* d_entry_pos;
    int* d_edge_off;           // NS_MAX_HOPS + 1: the entries before hop h
    unsigned long long* d_counters;  // mgx::NS_COUNTERS
    int fanouts[mgx::NS_MAX_HOPS];
    int replace;
    unsigned seed;
  };

  mem_t<data_slice_t> d_data_slice;

  nsample_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  nsample_problem_t(const nsample_problem_t&) = delete;
  nsample_problem_t& operator=(const nsample_problem_t&) = delete;
};

// the arrays the problem points at; the results grow with the largest run
struct nsample_state_t {
  mgx::ns_results_t res;
  mem_t<int> d_local, d_mark, d_edge_off;
  mem_t<unsigned long long> d_counters;
  void ensure(const mgx::ns_request_t& r, const mgx::ns_bounds_t& b, int n, standard_context_t& ctx) {
    res.ensure(r, b, ctx);
    if (d_local.size() == 0) {
      d_local = mem_t<int>((size_t)n, ctx);
      d_mark = mem_t<int>((size_t)n, ctx);
      d_edge_off = mem_t<int>(mgx::NS_MAX_HOPS + 1, ctx);
      d_counters = mem_t<unsigned long long>(mgx::NS_COUNTERS, ctx);
    }
  }
  nsample_problem_t::data_slice_t slice(const int* ro, const int* ci, const mgx::ns_request_t& r) const {
    nsample_problem_t::data_slice_t s;
    s.ro = ro; s.ci = ci;
    s.d_local = d_local.data(); s.d_mark = d_mark.data();
    s.d_row_offsets = res.row_offsets.data(); s.d_cols = res.cols.data(); s.d_entry_pos = res.entry_pos.data();
    s.d_edge_off = d_edge_off.data(); s.d_counters = d_counters.data();
    for (int h = 0; h < mgx::NS_MAX_HOPS; ++h) s.fanouts[h] = h < r.hops ? r.fanouts[h] : 0;
    s.replace = r.replace; s.seed = r.seed;
    return s;
  }
};

}  // namespace nsample
}  // namespace gunrock
