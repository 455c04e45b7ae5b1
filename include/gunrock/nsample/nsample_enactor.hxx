// gunrock/nsample/nsample_enactor.hxx -- neighbour sampling on the filter operator (mgx_nsample_enact): the plain path, the fused
// path's cross-check and yardstick.
//   transform              the seeds mark themselves
//   filter<fresh>          over all vertices: the marked ones without a local id, ascending -- V_0; a transform numbers them
//   per hop: scan          the rows' entry counts over the frontier
//            filter<sample> a lane per frontier row samples it and marks its destinations (nothing kept)
//            filter<fresh>, transform: V_{h + 1}, as above
//   transform x 2          cols to local ids, the seeds' local ids
// Two host waits per hop (the two filters' counts) and O(n) work per hop in the filter over all vertices: what the fused path's
// bitmap ranks and its bounds are there to avoid.  (No enactor_t underneath: its frontiers hold a traversal's state, not a batch's.)
#pragma once
#include <vector>

#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "nsample_functor.hxx"
#include "nsample_problem.hxx"

namespace gunrock {
namespace nsample {

struct nsample_enactor_t {
  typedef std::shared_ptr<frontier_t<int>> frontier_ptr;
  // what the last enact() did
  long long waits = 0, calls = 0;
  unsigned long long counters[mgx::NS_COUNTERS] = {0};
  frontier_ptr all, front, none;                  // every vertex; V_h; what the sample keeps (nothing)

  nsample_enactor_t(standard_context_t& ctx, int n) {
    all = std::make_shared<frontier_t<int>>(ctx, (size_t)n);
    front = std::make_shared<frontier_t<int>>(ctx, (size_t)n);
    none = std::make_shared<frontier_t<int>>(ctx, (size_t)n);
    int* const ids = all->data()->data();
    transform([=] __device__(int v) { ids[v] = v; }, n, ctx);
    all->resize((size_t)n);
  }
  nsample_enactor_t(const nsample_enactor_t&) = delete;
  nsample_enactor_t& operator=(const nsample_enactor_t&) = delete;

  // the marked vertices without a local id become V_slot, numbered from `base` on; returns how many there are
  int next_frontier(std::shared_ptr<nsample_problem_t>& p, nsample_state_t& s, int slot, int base, standard_context_t& ctx) {
    const int kept = gunrock::oprtr::filter::filter_kernel<nsample_problem_t, fresh_functor_t>(p, all, front, slot, ctx);
    ++waits; ++calls;
    const int* const ids = front->data()->data();
    int* const local = s.d_local.data();
    int* const vertices = s.res.vertices.data();
    transform([=] __device__(int i) { local[ids[i]] = base + i; vertices[base + i] = ids[i]; }, kept, ctx);
    ++calls;
    return kept;
  }

  void enact(std::shared_ptr<nsample_problem_t> p, nsample_state_t& s, const nsample_problem_t::data_slice_t& d, const mgx::ns_request_t& r,
             int n, standard_context_t& ctx) {
    const hipStream_t st = ctx.stream();
    waits = calls = 0;
    MGX_HIP(hipMemsetAsync(s.d_local.data(), 0xff, (size_t)n * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(s.d_mark.data(), 0, (size_t)n * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(s.d_edge_off.data(), 0, (mgx::NS_MAX_HOPS + 1) * sizeof(int), st));
    MGX_HIP(hipMemsetAsync(s.d_counters.data(), 0, mgx::NS_COUNTERS * sizeof(unsigned long long), st));
    MGX_HIP(hipMemsetAsync(s.res.row_offsets.data(), 0, sizeof(int), st));
    const int* const seeds = r.h_seeds ? s.res.d_seeds.data() : nullptr;
    transform([=] __device__(int i) { d.d_mark[seeds ? seeds[i] : i] = 1; }, r.count, ctx);
    ++calls;
    mgx::frontier_touched();
    std::vector<int>& off = s.res.hop_offsets;
    off.assign(1, 0);
    off.push_back(next_frontier(p, s, 0, 0, ctx));
    for (int h = 0; h < r.hops; ++h) {
      const int hb = off[h], F = off[h + 1] - off[h], k = r.fanouts[h], replace = r.replace;
      const int* const ids = front->data()->data();
      const long long* const total = mgx::transform_scan(
          [=] __device__(long long i) { return mgx::ns_entries(d.ro[ids[i] + 1] - d.ro[ids[i]], k, replace); }, F, d.d_row_offsets + hb, ctx, nullptr);
      transform([=] __device__(int) {
        d.d_edge_off[h + 1] = d.d_edge_off[h] + (int)*total;
        d.d_row_offsets[hb + F] = d.d_edge_off[h + 1];
      }, 1, ctx);
      calls += 2;
      gunrock::oprtr::filter::filter_kernel<nsample_problem_t, sample_functor_t>(p, front, none, h, ctx);
      ++calls;
      if (F > 0) ++waits;
      off.push_back(off[h + 1] + next_frontier(p, s, h + 1, off[h + 1], ctx));
    }
    int edge_off[mgx::NS_MAX_HOPS + 1];
    MGX_HIP(mgx::dtoh(edge_off, (const int*)s.d_edge_off.data(), mgx::NS_MAX_HOPS + 1, st));
    MGX_HIP(mgx::dtoh(counters, (const unsigned long long*)s.d_counters.data(), mgx::NS_COUNTERS, st));
    ++waits;
    s.res.seeds = r.count; s.res.edges = edge_off[r.hops]; s.res.device = true;
    s.res.edge_offsets.assign(edge_off, edge_off + r.hops + 1);
    s.res.any_whole = std::any_of(r.fanouts, r.fanouts + r.hops, [](int k) { return k < 0; });
    int* const seed_local = s.res.seed_local.data();
    transform([=] __device__(int e) { d.d_cols[e] = d.d_local[d.d_cols[e]]; }, s.res.edges, ctx);
    transform([=] __device__(int i) { seed_local[i] = d.d_local[seeds ? seeds[i] : i]; }, r.count, ctx);
    calls += 2;
  }
};

}  // namespace nsample
}  // namespace gunrock
