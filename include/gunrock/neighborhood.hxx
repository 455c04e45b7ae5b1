// gunrock/neighborhood.hxx -- segmented neighbourhood reduce.
// Drop-in for the reference's gunrock/src/neighborhood.hxx:12-70: same six template
// parameters (push is not deducible, callers must pass it -- SURVEY F11), same call contract:
// per edge cond_advance, apply_advance, optional output write, get_value_to_reduce(neighbor);
// reduced[] is indexed by FRONTIER POSITION (:58), identity for empty segments; returns the
// number of edges visited.
#pragma once

#include <type_traits>

#include "../mgx/lbs.hpp"
#include "../mgx/env.hpp"
#include "../mgx/nreduce.hpp"
#include "../mgx/scan.hpp"
#include "frontier.hxx"
#include "intrinsics.hxx"

namespace gunrock {
namespace oprtr {
namespace neighborhood {

// A functor may declare `static constexpr bool mgx_pure_gather = true`: its cond_advance / apply_advance are trivially
// true and get_value_to_reduce(v) is a pure read.  Only then may the operator skip the two calls and take a vertex's value
// once instead of once per edge (the full-frontier path below); the reference's own functors declare nothing and always
// get the per-edge contract of neighborhood.hxx:39-57.
template <typename F, typename = void>
struct is_pure_gather : std::false_type {};
template <typename F>
struct is_pure_gather<F, typename std::enable_if<F::mgx_pure_gather>::type> : std::true_type {};

// MGX_NR_SUBSET=0: frontiers that are not 0 .. n - 1 take the general kernel, as before round 6
inline bool nr_subset_enabled() {
  static const bool on = [] { const char* e = mgx::env("MGX_NR_SUBSET"); return !e || std::atoi(e) != 0; }();
  return on;
}

template <typename Problem, typename Functor, typename Value, typename reduce_op, bool has_output, bool push>
int neighborhood_kernel(std::shared_ptr<Problem> problem, std::shared_ptr<frontier_t<int>>& input,
                        std::shared_ptr<frontier_t<int>>& output, Value* reduced, Value identity, int iteration,
                        standard_context_t& context) {
  graph_device_t& graph = *problem->gslice;
  // out-edges (CSR) when pushing, in-edges (the CSC slots) when pulling
  const int* const offsets = push ? graph.d_row_offsets.data() : graph.d_col_offsets.data();
  const int* const neighbours = push ? graph.d_col_indices.data() : graph.d_row_indices.data();
  const int* const frontier = input->data()->data();
  const long long frontier_size = (long long)input->size();

  // Full frontier (0, 1, ..., n - 1: PR's first iteration) on a graph that carries the hub-first layout with unit blocks and
  // degree classes: mgx/nreduce.hpp.  Whether the frontier IS the iota is checked on the device (one pass over it);
  // it then holds every edge of the graph: no degree scan, no search.
  typename Problem::data_slice_t* const data = problem->d_data_slice.data();
  // (round 6) ... or a large SUBSET of the vertices in ascending order -- what PR's filter leaves for every iteration but the first
  // (pr_enactor.hxx:53-66): the same kernels compute every row and keep the frontier's, results by frontier position.  A frontier of
  // fewer than n / 8 vertices takes the general kernel, whose cost follows the frontier's edges (the fast path costs what a full
  // frontier costs).
  const bool full = frontier_size == (long long)graph.num_nodes;
  const bool subset = !full && frontier_size < (long long)graph.num_nodes && frontier_size * 8 >= (long long)graph.num_nodes && nr_subset_enabled();
  // what this call did, for mgx_graph_nr_last_call (host-side bookkeeping: nothing of it reaches a kernel)
  auto& last = context.nr_last_call;
  last.valid = true; last.body = 0; last.frontier = full ? 1 : subset ? 2 : 0; last.rejected = 0; last.edges = 0;
  // (the kernel keeps 40 000 4-byte values in the 160 KB of LDS: wider values take the general path; so does an operator whose neutral
  //  element is not known -- mgx::op_neutral -- since the layout's kernels fold padding entries and idle lanes)
  if constexpr (sizeof(Value) == 4 && mgx::op_neutral<reduce_op, Value>::known)
  if (!has_output && is_pure_gather<Functor>::value && (full || subset) && frontier_size > 0 &&
      (push || graph.csc_is_csr) && mgx::nr_units_valid(graph) &&
      context.scratch_bytes >= mgx::nr_scratch_bytes(graph.num_nodes, graph.rows.ub.units_pad, sizeof(Value))) {
    // the check (inside the first kernel) and the work go out back to back: the kernels behind it look at its verdict themselves (a device
    // word that holds the epoch of the last call whose frontier was NOT the iota); one host wait, behind everything
    context.mailbox[8] = 1;
    context.mailbox[9] = (long long)context.nr_edges_base;
    const unsigned epoch = context.next_nr_epoch();
    if (graph.num_edges > 0) {
      // the long rows by slice of their destinations when the graph carries them (MGX_NR_SLICED=0: the unit blocks, as before round 5)
      static const bool sliced = [] { const char* e = mgx::env("MGX_NR_SLICED"); return !e || std::atoi(e) != 0; }();
      static const unsigned parts = [] { const char* e = mgx::env("MGX_NR_PARTS"); return e ? (unsigned)std::atoi(e) & 3u : 3u; }();
      mgx::nr_layout_t L = mgx::nr_layout_of(graph, context, sizeof(Value), sliced);
      L.parts = parts ? parts : 3u;
      if (subset && graph.d_nr_pos.size() < (size_t)graph.num_nodes) {       // (first subset call on this graph: the one allocation of this path)
        context.synchronize();
        graph.d_nr_pos = mem_t<unsigned long long>((size_t)graph.num_nodes, context);
        MGX_HIP(hipMemsetAsync(graph.d_nr_pos.data(), 0, (size_t)graph.num_nodes * sizeof(unsigned long long), context.stream()));
      }
      const long long seq = mgx::nr_full_frontier<Value>(L, [=] __device__(int v) -> Value { return Functor::get_value_to_reduce(v, data, iteration); }, reduced,
                                   identity, reduce_op(), context, frontier, context.mailbox.data() + 8, context.nr_flag(), epoch,
                                   full ? -1 : frontier_size, offsets, subset ? (mgx::u64*)graph.d_nr_pos.data() : nullptr);
      if (seq) context.mailbox_wait(seq); else context.synchronize();
      // (a subset call added its frontier's degrees to the context's counter whatever its verdict: the base follows)
      const unsigned long long before = context.nr_edges_base;
      if (subset) context.nr_edges_base = (unsigned long long)context.mailbox[9];
      if (context.mailbox[8] == 1) {
        last.body = L.nrs_mu ? 2 : 1;
        last.edges = full ? (long long)graph.num_edges : (long long)(context.nr_edges_base - before);
        return (int)last.edges;
      }
      last.rejected = 1;
    }
  }

  // segment i = the neighbour list of frontier[i]: exclusive scan of the degrees into the graph's scratch scan
  graph.ensure_scanned(input->capacity(), context);
  int* const segment_start = graph.d_scanned_row_offsets.data();
  long long edges = 0;
  mgx::transform_scan([=] __device__(long long i) { return offsets[frontier[i] + 1] - offsets[frontier[i]]; },
                      frontier_size, segment_start, context, &edges);
  last.edges = edges;
  if (edges == 0) return 0;
  int* out = nullptr;
  if (has_output) {
    output->resize((size_t)edges);
    out = output->data()->data();
  }

  // per edge: the functor's contract (cond, then apply, both always), the optional output slot, and the value that
  // goes into the segment's reduction; reduced[i] belongs to frontier POSITION i (neighborhood.hxx:58)
  auto visit = [=] __device__(int slot, int segment, int rank) -> Value {
    const int v = frontier[segment];
    const int edge = offsets[v] + rank;
    const int u = neighbours[edge];
    const bool cond = Functor::cond_advance(v, u, edge, rank, slot, data, iteration);
    const bool applied = Functor::apply_advance(v, u, edge, rank, slot, data, iteration);
    if (has_output) out[slot] = (cond && applied) ? u : -1;
    return Functor::get_value_to_reduce(u, data, iteration);
  };
  mgx::lbs_segreduce<Value>(visit, edges, segment_start, frontier_size, reduced, reduce_op(), identity, context);
  return (int)edges;
}

}  // namespace neighborhood
}  // namespace oprtr
}  // namespace gunrock
