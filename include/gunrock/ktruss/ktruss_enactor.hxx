// gunrock/ktruss/ktruss_enactor.hxx -- k-truss decomposition on the advance and filter operators (mgx_ktruss_enact): the plain
// path, the fused path's cross-check and baseline.
//   supports:  advance<support_functor_t, idempotence = false, has_output = false> over the iota frontier of the DAG's vertices
//   peel:      frontiers of EDGE ids.  For k = 2, 3, ... while edges are alive, passes until one finds no front:
//                  filter<collect_functor_t>  over all edges: the front, marked
//                  filter<expand_functor_t>   over the front: the triangles' decrements (no output)
//                  filter<seal_functor_t>     over the front: trussness, state, vtruss, hist (no output)
//              The next pass rescans all edges, as the operator k-core rescans all vertices.  A level is a k that had a front.
// Every operator call reads a count back: `waits` counts one per call.
#pragma once
#include "../advance.hxx"
#include "../enactor.hxx"
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "ktruss_functor.hxx"
#include "ktruss_problem.hxx"

namespace gunrock {
namespace ktruss {

struct ktruss_enactor_t : enactor_t {
  long long waits = 0, calls = 0, levels = 0, passes = 0;
  int largest = 0;

  // node-capacity frontiers of max(vertices, edges) ids: the iota serves the advance (vertices) and the filters (edge ids); no
  // edge-capacity buffers: no operator here writes an expansion
  ktruss_enactor_t(standard_context_t& ctx, int capacity) : enactor_t(ctx, capacity, 0, 0.0f) {}
  ktruss_enactor_t(const ktruss_enactor_t&) = delete;
  ktruss_enactor_t& operator=(const ktruss_enactor_t&) = delete;

  // sup0 (cleared by the caller) += the supports of the problem's DAG
  void supports(std::shared_ptr<ktruss_problem_t> problem, standard_context_t& ctx) {
    namespace adv = gunrock::oprtr::advance;
    frontier_ptr& everyone = indices;             // 0 .. capacity - 1, never written
    everyone->resize((size_t)problem->gslice->num_nodes);
    if (problem->gslice->d_scanned_row_offsets.size() < everyone->capacity() + 1) ++waits;   // (the advance grows it behind a wait, once)
    adv::advance_forward_kernel<ktruss_problem_t, support_functor_t, /*idempotence=*/false, /*has_output=*/false>(
        problem, everyone, buffers[0], 0, ctx);
    ++waits;
    ++calls;
  }

  // the peel of the problem's edges (sup = sup0, every state alive, the results cleared by the caller)
  void peel(std::shared_ptr<ktruss_problem_t> problem, standard_context_t& ctx) {
    namespace fl = gunrock::oprtr::filter;
    const long long m = problem->gslice->num_edges;
    frontier_ptr& everyone = indices;
    frontier_ptr& front = filtered_indices;
    frontier_ptr& nothing = buffers[0];
    everyone->resize((size_t)m);
    levels = passes = 0;
    largest = 0;
    long long alive = m;
    // (a support is at most vertices - 2: by k = vertices every edge has left; hist holds vertices + 1 counts)
    for (int k = 2; alive > 0 && k <= problem->gslice->num_nodes; ++k) {
      bool any = false;
      for (;;) {
        const int joined = fl::filter_kernel<ktruss_problem_t, collect_functor_t>(problem, everyone, front, k, ctx);
        ++waits; ++calls;
        if (joined == 0) break;
        any = true;
        ++passes;
        fl::filter_kernel<ktruss_problem_t, expand_functor_t>(problem, front, nothing, k, ctx);
        fl::filter_kernel<ktruss_problem_t, seal_functor_t>(problem, front, nothing, k, ctx);
        waits += 2; calls += 2;
        alive -= joined;
      }
      if (any) {
        ++levels;
        largest = k;
      }
    }
  }
};

}  // namespace ktruss
}  // namespace gunrock
