// gunrock/msbfs/msbfs_enactor.hxx -- bit-parallel multi-source BFS on the advance and filter operators (mgx_msbfs_enact): the
// plain path, the fused path's cross-check and yardstick.  It always pushes and visits every level with a host wait.
// Per batch of 64 sources the words are zeroed and the sources' bits set; then per level
//   advance<expand>    over the front's vertices: the atomicOr into next, the destination passed on when it changed bits
//   filter<finalize>   dedups and finalizes; what it keeps is the next front
//   filter<clear>      over the old front
//   64 threads         fold the level's counts into reach, far, ecc and harm (ascending depth, as the fused path adds them)
#pragma once
#include <vector>

#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "msbfs_functor.hxx"
#include "msbfs_problem.hxx"

namespace gunrock {
namespace msbfs {

struct msbfs_enactor_t : enactor_t {
  // what the last enact() did
  long long levels = 0, deepest = 0, waits = 0, calls = 0;
  frontier_ptr fronts[2];                         // node capacity: the front of level t in fronts[t & 1]

  // (the advance writes one slot per entry: edge buffers of exactly num_edges)
  msbfs_enactor_t(standard_context_t& ctx, int num_nodes, int num_edges) : enactor_t(ctx, num_nodes, num_edges, 0.0f) {
    buffers[0] = std::make_shared<frontier_t<int>>(ctx, (size_t)std::max(num_edges, 1));
    buffers[1] = std::make_shared<frontier_t<int>>(ctx, (size_t)std::max(num_nodes, 1));      // (what filter<clear> keeps: nobody)
    for (frontier_ptr& f : fronts) f = std::make_shared<frontier_t<int>>(ctx, (size_t)std::max(num_nodes, 1));
  }
  msbfs_enactor_t(const msbfs_enactor_t&) = delete;
  msbfs_enactor_t& operator=(const msbfs_enactor_t&) = delete;

  template <typename F>
  int filter(std::shared_ptr<msbfs_problem_t>& p, frontier_ptr& in, frontier_ptr& out, int iteration, standard_context_t& ctx) {
    ++waits; ++calls;
    return gunrock::oprtr::filter::filter_kernel<msbfs_problem_t, F>(p, in, out, iteration, ctx);
  }

  // h_sources: count ids, or NULL for every vertex
  void enact(std::shared_ptr<msbfs_problem_t> p, const msbfs_problem_t::data_slice_t& s, const int* h_sources, long long count,
             standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    const int n = s.n;
    const size_t N = (size_t)n;
    levels = deepest = waits = calls = 0;
    const long long batches = (count + 63) / 64;
    const int cap = s.cap;
    for (long long B = 0; B < batches; ++B) {
      const int valid = (int)std::min<long long>(64, count - 64 * B);
      const bool first_batch = B == 0;
      msbfs_scalars_t* const sc = s.d_scalars;
      unsigned long long* const seen = s.d_seen;
      unsigned long long* const front = s.d_front;
      unsigned long long* const next = s.d_next;
      unsigned long long* const cnt = s.d_cnt;
      long long* const rin = s.d_reach_in;
      long long* const fin = s.d_far_in;
      long long* const per = s.d_per_src;
      int* const depth = s.d_depth;
      const int* const sources = s.d_sources;
      const int batch = (int)B;
      transform([=] __device__(int v) {
        seen[v] = 0; front[v] = 0; front[N + v] = 0; next[v] = 0;
        if (first_batch) { rin[v] = 0; fin[v] = 0; }
      }, n, ctx);
      transform([=] __device__(int b) {
        if (b == 0) { sc->batch = batch; sc->valid = valid; }
        cnt[b] = 0;
        if (b < valid) {
          const size_t i = (size_t)batch * 64 + b;
          const int src = sources ? sources[i] : (int)i;
          per[i] = 0; per[(size_t)cap + i] = 0; per[2 * (size_t)cap + i] = 0; ((double*)per)[3 * (size_t)cap + i] = 0.0;
          atomicOr(front + src, 1ull << b);
          atomicOr(seen + src, 1ull << b);
          if (depth) depth[i * N + (size_t)src] = 0;
        }
      }, 64, ctx);
      calls += 2;
      std::vector<int> first;                     // the distinct sources, in their order
      for (int b = 0; b < valid; ++b) {
        const int src = h_sources ? h_sources[64 * B + b] : (int)(64 * B + b);
        bool fresh = true;
        for (int x : first) fresh = fresh && x != src;
        if (fresh) first.push_back(src);
      }
      MGX_HIP(fronts[0]->load(first));
      ++waits;
      for (int t = 0;; ++t) {
        frontier_ptr& in = fronts[t & 1];
        frontier_ptr& out = fronts[(t + 1) & 1];
        adv::advance_forward_kernel<msbfs_problem_t, expand_functor_t, /*idempotence=*/false, /*has_output=*/true>(p, in, buffers[0], t, ctx);
        ++waits; ++calls;
        const int found = filter<finalize_functor_t>(p, buffers[0], out, t + 1, ctx);
        filter<clear_functor_t>(p, in, buffers[1], t, ctx);
        const int d = t + 1;
        transform([=] __device__(int b) {
          const unsigned long long c = cnt[b];
          cnt[b] = 0;
          if (c && b < valid) {
            const size_t i = (size_t)batch * 64 + b;
            per[i] += (long long)c; per[(size_t)cap + i] += (long long)c * d; per[2 * (size_t)cap + i] = d;
            ((double*)per)[3 * (size_t)cap + i] += (double)c / (double)d;
          }
        }, 64, ctx);
        ++calls;
        ++levels;
        deepest = std::max<long long>(deepest, t + 1);
        if (found == 0) break;
      }
    }
  }
};

}  // namespace msbfs
}  // namespace gunrock
