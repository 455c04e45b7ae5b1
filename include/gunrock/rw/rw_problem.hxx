// gunrock/rw/rw_problem.hxx -- state of the random walks the operator path runs (mgx_rw_enact): every walker's
// position in arrays of its own, the setup arrays (the rows' maxima, the sorted copy) shared with the fused path
// (mgx/rw_fused.hpp: rw_setup_state_t).
#pragma once
#include "../../mgx/rw_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace rw {

struct rw_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    mgx::rw_graph_t g;
    mgx::rw_params_t P;
    const int* d_starts;       // S ids (NULL: start s is vertex s)
    int* d_cur;                // W: where every walker stands; the ends when the run is over
    int* d_prev;               // W: the vertex before it, -1 none
    int* d_len;                // W: the steps it has taken
    int* d_paths;              // W x (L + 1), -1 everywhere before the run (NULL: not kept)
    unsigned long long* d_visits;    // n (NULL: not kept)
    unsigned long long* d_counters;  // mgx::RW_COUNTERS
    int per_start, length;
  };

  mem_t<data_slice_t> d_data_slice;

  rw_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  rw_problem_t(const rw_problem_t&) = delete;
  rw_problem_t& operator=(const rw_problem_t&) = delete;
};

// the arrays the problem points at; they grow with the largest run
struct rw_state_t {
  mgx::rw_results_t res;       // (its ends are d_cur, its lengths d_len)
  mem_t<int> d_prev;
  size_t prev_cap = 0;
  void ensure(const mgx::rw_request_t& r, int n, standard_context_t& ctx) {
    res.ensure(r, n, ctx);
    if ((size_t)r.walkers() > prev_cap) { d_prev = mem_t<int>((size_t)r.walkers(), ctx); prev_cap = (size_t)r.walkers(); }
  }
  rw_problem_t::data_slice_t slice(const mgx::rw_graph_t& g, const mgx::rw_params_t& P, const mgx::rw_request_t& r) const {
    rw_problem_t::data_slice_t s;
    s.g = g; s.P = P;
    s.d_starts = r.h_starts ? res.d_starts.data() : nullptr;
    s.d_cur = res.ends.data(); s.d_prev = d_prev.data(); s.d_len = res.lengths.data();
    s.d_paths = r.want_paths ? res.paths.data() : nullptr;
    s.d_visits = r.want_visits ? res.visits.data() : nullptr;
    s.d_counters = res.counters.data();
    s.per_start = (int)r.per_start; s.length = (int)r.length;
    return s;
  }
};

}  // namespace rw
}  // namespace gunrock
