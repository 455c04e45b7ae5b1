// gunrock/louvain/louvain_enactor.hxx -- the Louvain run on the advance and filter operators and the library's segmented sort
// (mgx_louvain_enact): the plain path, the fused path's cross-check and yardstick.  Per level a setup (k, Sigma, W,
// the identity's Qnum), then every vertex every iteration:
//   advance<gather_out>                  over the iota frontier: every vote's (label, weight) into its vertex's segment
//   advance<gather_in>                   over the backward view (level 0, symmetric == 0)
//   segmented_sort(votes, weights)       every vertex's votes ascending by label, the weights riding along
//   filter<best>  (iteration = t)        scans the runs for best(v); keeps the vertices that move: its count is `moved`
//   filter<apply>                        over the movers, after the labels and Sigma were set aside
//   a Qnum sweep                         one thread per vertex; the host accepts, or puts the labels and Sigma back
// and the contraction of mgx/louvain_aggregate.hpp between the levels.  It waits on the host as often as it needs.
#pragma once
#include <cmath>
#include <vector>

#include "../../mgx/louvain_aggregate.hpp"
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "../moderngpu/kernel_segsort.hxx"
#include "louvain_functor.hxx"
#include "louvain_problem.hxx"

namespace gunrock {
namespace louvain {

struct louvain_enactor_t : enactor_t {
  // what the last enact() did
  std::vector<long long> levels;                  // (vertices, entries, iterations, accepted, communities, Qnum) per level
  std::vector<long long> trace;                   // (moved, accepted, Qnum) per iteration, the levels one behind the other
  std::vector<long long> map_off;                 // the aggregated levels' maps in the state's d_maps
  long long w = 0, s_in = 0, s_sq = 0, waits = 0, calls = 0, iterations = 0;

  louvain_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {
    buffers[1] = std::make_shared<frontier_t<int>>(ctx, (size_t)std::max(num_nodes, 1));
  }
  louvain_enactor_t(const louvain_enactor_t&) = delete;
  louvain_enactor_t& operator=(const louvain_enactor_t&) = delete;

  // S_in and S_sq of the state's labels on the level's graph -> Qnum (one host wait)
  long long qnum(const mgx::lv_graph_t& g, louvain_state_t& st, standard_context_t& ctx, long long* in, long long* sq) {
    louvain_scalars_t* const sc = st.d_scalars.data();
    const int* const lab = st.d_label.data();
    const unsigned* const sigma = st.d_sigma.data();
    transform([=] __device__(int) { sc->s_in = 0; sc->s_sq = 0; }, 1, ctx);
    transform([=] __device__(int v) {
      unsigned long long a = 0;
      for (int side = 0; side < (g.co ? 2 : 1); ++side) {
        const int* const off = side ? g.co : g.ro;
        const int* const adj = side ? g.ri : g.ci;
        for (int e = off[v]; e < off[v + 1]; ++e) {
          const int u = adj[e];
          const unsigned x = g.wt ? g.wt[e] : (u != v ? 1u : 0u);
          a += lab[u] == lab[v] ? x : 0u;
        }
      }
      if (a) atomicAdd(&sc->s_in, a);
      const unsigned long long s = sigma[v];
      if (s) atomicAdd(&sc->s_sq, s * s);
    }, g.n, ctx);
    louvain_scalars_t h;
    MGX_HIP(mgx::dtoh(&h, (const louvain_scalars_t*)sc, 1));
    ++waits;
    *in = (long long)h.s_in;
    *sq = (long long)h.s_sq;
    return (long long)h.s_in * w - (long long)h.s_sq;
  }

  void enact(std::shared_ptr<graph_device_t> graph, louvain_state_t& st, mgx::louvain_aggregate_t& agg, bool symmetric, unsigned seed,
             int max_iter, int max_levels, double tol, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    typedef std::shared_ptr<louvain_problem_t> problem_ptr;
    const int n0 = graph->num_nodes;
    levels.clear(); trace.clear();
    map_off.assign(1, 0);
    w = s_in = s_sq = waits = calls = iterations = 0;
    agg.waits = 0;
    louvain_scalars_t* const sc = st.d_scalars.data();
    int* const label = st.d_label.data();
    int* const heads = st.d_heads.data();
    unsigned* const kk = st.d_k.data();
    unsigned* const sigma = st.d_sigma.data();
    int* const final_lab = st.d_final.data();
    transform([=] __device__(int v) { final_lab[v] = v; }, n0, ctx);
    mgx::lv_graph_t g = {graph->d_row_offsets.data(), graph->d_col_indices.data(), nullptr,
                         symmetric ? nullptr : graph->d_col_offsets.data(), symmetric ? nullptr : graph->d_row_indices.data(), n0};
    long long entries = symmetric ? graph->num_edges : 2ll * graph->num_edges;
    bool any = false;
    for (int level = 0;; ++level) {
      const int n = g.n;
      // the level's setup: the segments' heads, labels, k, Sigma and W
      transform([=] __device__(int) { sc->seed = seed; sc->w = 0; sc->s_in = 0; sc->s_sq = 0; }, 1, ctx);
      transform([=] __device__(int v) {
        heads[v] = g.ro[v] + (g.co ? g.co[v] : 0);
        if (v >= n) return;
        unsigned long long k = 0;
        for (int side = 0; side < (g.co ? 2 : 1); ++side) {
          const int* const off = side ? g.co : g.ro;
          const int* const adj = side ? g.ri : g.ci;
          for (int e = off[v]; e < off[v + 1]; ++e) k += g.wt ? g.wt[e] : (adj[e] != v ? 1u : 0u);
        }
        label[v] = v;
        kk[v] = (unsigned)k;
        sigma[v] = (unsigned)k;
        if (k) atomicAdd((unsigned long long*)&sc->w, k);
      }, (long long)n + 1, ctx);
      louvain_scalars_t h;
      MGX_HIP(mgx::dtoh(&h, (const louvain_scalars_t*)sc, 1));
      ++waits;
      w = h.w;
      long long in = 0, sq = 0;
      long long q = qnum(g, st, ctx, &in, &sq);
      if (level == 0) { s_in = in; s_sq = sq; }
      if (w == 0 || level >= max_levels) break;
      const double x = tol * (double)w * (double)w;
      const long long cap = 1ll << 62;
      const long long thr = x >= (double)cap ? cap : std::min((long long)std::ceil(x), cap);
      // the level's views
      const louvain_problem_t::data_slice_t slice = {g.ro, g.co, g.wt, heads, st.d_votes.data(), st.d_vote_w.data(), label,
                                                     st.d_best.data(), sigma, kk, sc};
      problem_ptr fwd = level == 0 ? std::make_shared<louvain_problem_t>(graph, slice, ctx)
                                   : std::make_shared<louvain_problem_t>(slice, g.ro, g.ci, n, (int)entries, ctx);
      problem_ptr bwd;
      if (g.co) bwd = std::make_shared<louvain_problem_t>(slice, g.co, g.ri, n, graph->num_edges, ctx);
      indices->resize((size_t)n);                 // 0 .. n - 1, never written
      frontier_ptr nobody = buffers[0];
      int t = 0, rejects = 0, accepted = 0;
      while (t < max_iter && rejects < 2) {
        adv::advance_forward_kernel<louvain_problem_t, gather_out_functor_t, /*idempotence=*/false, /*has_output=*/false>(fwd, indices, nobody, t, ctx);
        ++waits; ++calls;
        if (bwd) {
          adv::advance_forward_kernel<louvain_problem_t, gather_in_functor_t, false, false>(bwd, indices, nobody, t, ctx);
          ++waits; ++calls;
        }
        if (entries >= 2) {
          auto ascending = [] MGPU_DEVICE(int left, int right) { return left < right; };
          mgpu::segmented_sort(st.d_votes.data(), st.d_vote_w.data(), entries, (const int*)heads, n, ascending, ctx);
          waits += 2; ++calls;
        }
        const int moved = gunrock::oprtr::filter::filter_kernel<louvain_problem_t, best_functor_t>(fwd, indices, filtered_indices, t, ctx);
        ++waits; ++calls;
        long long qn = q, in_n = in, sq_n = sq;
        if (moved > 0) {
          MGX_HIP(mgx::dtod(st.d_old.data(), (const int*)label, (size_t)n));
          MGX_HIP(mgx::dtod(st.d_sigma_old.data(), (const unsigned*)sigma, (size_t)n));
          gunrock::oprtr::filter::filter_kernel<louvain_problem_t, apply_functor_t>(fwd, filtered_indices, buffers[1], t, ctx);
          ++waits; ++calls;
          qn = qnum(g, st, ctx, &in_n, &sq_n);
        }
        const bool ok = moved > 0 && qn - q > thr;
        trace.push_back(moved); trace.push_back(ok ? 1 : 0); trace.push_back(qn);
        if (ok) {
          q = qn; in = in_n; sq = sq_n; rejects = 0; ++accepted;
        } else {
          ++rejects;
          if (moved > 0) {
            MGX_HIP(mgx::dtod(label, (const int*)st.d_old.data(), (size_t)n));
            MGX_HIP(mgx::dtod(sigma, (const unsigned*)st.d_sigma_old.data(), (size_t)n));
          }
        }
        ++t;
      }
      iterations += t;
      const size_t rec = levels.size();
      for (long long x6 : {(long long)n, entries, (long long)t, (long long)accepted, (long long)n, q}) levels.push_back(x6);
      if (accepted == 0) break;
      s_in = in; s_sq = sq;
      const long long at = map_off.back();
      if ((size_t)(at + n) > st.d_maps.size()) {
        mem_t<int> bigger(2 * (size_t)(at + n), ctx);
        MGX_HIP(mgx::dtod(bigger.data(), (const int*)st.d_maps.data(), (size_t)at));
        ctx.synchronize();
        st.d_maps.swap(bigger);
      }
      const bool more = level + 1 < max_levels;
      const int nc = agg.renumber(g, label, kk, st.d_maps.data() + at, final_lab, n0, !any, more, ctx);
      any = true;
      map_off.push_back(at + n);
      levels[rec + 4] = nc;
      if (!more) break;
      const int o = level & 1;
      entries = agg.contract(g, st.d_maps.data() + at, kk, nc, g.wt ? entries : w, st.cro[o].data(), st.cci[o].data(), st.cwt[o].data(), ctx);
      g = mgx::lv_graph_t{st.cro[o].data(), st.cci[o].data(), st.cwt[o].data(), nullptr, nullptr, nc};
    }
    waits += agg.waits;
  }
};

}  // namespace louvain
}  // namespace gunrock
