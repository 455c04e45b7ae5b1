// gunrock/lspar/lspar_enactor.hxx -- local sparsification on the neighbourhood-reduce, advance and segmented-sort operators
// (mgx_lspar_enact): the slow, faithful path, and the fused path's cross-check and baseline.  What the reference's
// lspar_enactor_t::enact does (gunrock/src/lspar/lspar_enactor.hxx), for k hash functions instead of one:
//   neighborhood<minhash_functor_t, minimum_t<int>, has_output = false, push = true>   over the iota frontier, once per j
//   advance<sim_functor_t, false, false>                                                {eid, sim} per entry
//   segmented_sort(sims, m, row_offsets, n, sim >)                                      stable: position breaks ties
//   advance<select_functor_t, false, true>                                              rank < t(src), -1 otherwise
//   transform_compact                                                                   the kept records
// and then what the reference leaves out (its result copy reads an array nothing writes): one more segmented_sort of the
// kept records by eid, which puts every row back in row order, and the four result arrays.  Upstream passes five template
// arguments to the six-argument neighborhood_kernel and does not compile; here all six are given.
#pragma once
#include <climits>

#include "../advance.hxx"
#include "../enactor.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "../moderngpu/kernel_segsort.hxx"
#include "../neighborhood.hxx"
#include "lspar_functor.hxx"
#include "lspar_problem.hxx"

namespace gunrock {
namespace lspar {

struct lspar_enactor_t : enactor_t {
  typedef lspar_problem_t::sim_edge_t sim_edge_t;
  // what the last enact() did: kept entries, rows cut, host waits; its result (out_ro has n + 1 entries)
  long long kept = 0, cut = 0, waits = 0;
  mem_t<sim_edge_t> d_kept;
  mem_t<int> d_out_ro, d_out_ci, d_out_eid, d_out_sim;

  lspar_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges) {
    d_out_ro = mem_t<int>((size_t)num_nodes + 1, ctx);
  }
  lspar_enactor_t(const lspar_enactor_t&) = delete;
  lspar_enactor_t& operator=(const lspar_enactor_t&) = delete;

  void enact(std::shared_ptr<lspar_problem_t> problem, standard_context_t& ctx) {
    namespace nb = gunrock::oprtr::neighborhood;
    namespace ad = gunrock::oprtr::advance;
    graph_device_t& g = *problem->gslice;
    const int n = g.num_nodes, m = g.num_edges, k = problem->k;
    frontier_ptr& everyone = indices;             // 0 .. n - 1, never written
    waits = 0;

    // minhashes, one neighbourhood reduce per hash function
    int* const reduced = problem->d_reduced.data();
    unsigned* const mwh = problem->d_minwise_hashs.data();
    for (int j = 0; j < k; ++j) {
      problem->reset_hashs(j, ctx);
      const int edges = nb::neighborhood_kernel<lspar_problem_t, minhash_functor_t, int, mgpu::minimum_t<int>, false, true>(
          problem, everyone, everyone, reduced, INT_MAX, 0, ctx);
      ++waits;
      const bool none = edges == 0;               // (no entries at all: the operator leaves the results unwritten)
      transform([=] __device__(int v) { mwh[(size_t)v * k + j] = none ? 0xFFFFFFFFu : (unsigned)reduced[v] ^ 0x80000000u; }, n, ctx);
    }

    // {eid, sim} per entry, sorted by sim within each row
    sim_edge_t* const sims = problem->d_sims.data();
    const int* const ro = g.d_row_offsets.data();
    if (m > 0) {
      (void)ad::advance_forward_kernel<lspar_problem_t, sim_functor_t, false, false>(problem, everyone, buffers[0], 0, ctx);
      ++waits;
      auto by_sim = [] MGPU_DEVICE(sim_edge_t left, sim_edge_t right) { return left.sim > right.sim; };
      mgpu::segmented_sort(sims, (long long)m, ro, n, by_sim, ctx);
      waits += 2;
    }

    // the first t(src) of every row, compacted
    if (d_kept.size() < (size_t)std::max(m, 1)) d_kept = mem_t<sim_edge_t>((size_t)std::max(m, 1), ctx);
    sim_edge_t* const kept_recs = d_kept.data();
    kept = 0;
    if (m > 0) {
      (void)ad::advance_forward_kernel<lspar_problem_t, select_functor_t, false, true>(problem, everyone, buffers[1], 0, ctx);
      ++waits;
      const int* const tagged = buffers[1]->data()->data();
      auto compact = mgx::transform_compact((long long)m, ctx);
      kept = compact.upsweep([=] __device__(long long i) { return tagged[i] != -1; });
      compact.downsweep([=] __device__(long long dest, long long src) { kept_recs[dest] = sims[src]; });
      ++waits;
    }

    // back to row order: the kept records of each row sorted by eid under the rows' new offsets
    const int* const t = problem->d_thresholds.data();
    long long total = 0;
    const long long* d_total = mgx::transform_scan([=] __device__(long long v) { return t[v]; }, (long long)n, d_out_ro.data(), ctx, &total);
    ++waits;
    int* const out_ro = d_out_ro.data();
    transform([=] __device__(int) { out_ro[n] = (int)*d_total; }, 1, ctx);
    if (total != kept) throw mgx::mgx_error(MGX_E_INVALID, "lspar enact: kept entries do not match the keep counts");
    if (kept > 0) {
      auto by_eid = [] MGPU_DEVICE(sim_edge_t left, sim_edge_t right) { return left.eid < right.eid; };
      mgpu::segmented_sort(kept_recs, kept, out_ro, n, by_eid, ctx);
      waits += 2;
    }

    const size_t cap = (size_t)std::max<long long>(kept, 1);
    if (d_out_ci.size() < cap) {
      d_out_ci = mem_t<int>(cap, ctx);
      d_out_eid = mem_t<int>(cap, ctx);
      d_out_sim = mem_t<int>(cap, ctx);
    }
    int* const oci = d_out_ci.data();
    int* const oeid = d_out_eid.data();
    int* const osim = d_out_sim.data();
    const int* const ci = g.d_col_indices.data();
    transform([=] __device__(int i) {
      const sim_edge_t r = kept_recs[i];
      oci[i] = ci[r.eid];
      oeid[i] = r.eid;
      osim[i] = (int)r.sim;
    }, kept, ctx);

    // rows cut (t < d)
    cut = 0;
    if (n > 0) {
      auto counter = mgx::transform_compact((long long)n, ctx);
      cut = counter.upsweep([=] __device__(long long v) { return t[v] < ro[v + 1] - ro[v]; });
      ++waits;
    }
  }
};

}  // namespace lspar
}  // namespace gunrock
