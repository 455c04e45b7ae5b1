// gunrock/coloring/coloring_problem.hxx -- state of the graph colouring the operator path runs (mgx_color_enact).
// The reference's coloring_problem_t (gunrock/src/coloring/coloring_problem.hxx): the same data-slice fields and constructor
// (graph, seed, max_iter, context).  What differs: the per-round keys are not moderngpu's fill_random over a
// host generator but key_i(v) = fmix32(v ^ salt_i) (mgx/color_hash.hpp), stored with bit 31 flipped so that the i32
// min / max of the neighbourhood reduce order them as unsigned -- one definition the fused path and the tests' model share.
#pragma once
#include "../../mgx/color_hash.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace coloring {

struct coloring_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device, all indexed by vertex id
    int* d_reduced_max;        // max of the uncoloured neighbours' keys (INT_MIN: none)
    int* d_reduced_min;        // min of the uncoloured neighbours' keys (INT_MAX: none)
    int* d_hashs;              // key_i(v) ^ 0x80000000 for the round being run
    int* d_colors;             // 0: uncoloured; round i gives 2i + 1 or 2i + 2
  };

  unsigned seed;
  int max_iter;                // <= 0: until no vertex is left
  mem_t<int> d_reduced_max, d_reduced_min, d_hashs, d_colors;
  mem_t<data_slice_t> d_data_slice;

  coloring_problem_t(std::shared_ptr<graph_device_t> graph, unsigned seed_, int max_iter_, standard_context_t& ctx)
      : problem_t(graph), seed(seed_), max_iter(max_iter_) {
    const size_t n = (size_t)std::max(graph->num_nodes, 1);
    d_reduced_max = mem_t<int>(n, ctx);
    d_reduced_min = mem_t<int>(n, ctx);
    d_hashs = mem_t<int>(n, ctx);
    d_colors = mem_t<int>(n, ctx);
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{d_reduced_max.data(), d_reduced_min.data(), d_hashs.data(),
                                                                    d_colors.data()}), ctx);
    reset(ctx);
  }
  coloring_problem_t(const coloring_problem_t&) = delete;
  coloring_problem_t& operator=(const coloring_problem_t&) = delete;

  // all uncoloured, the keys of round 0 (asynchronous on the context's stream)
  void reset(standard_context_t& ctx) {
    MGX_HIP(hipMemsetAsync(d_colors.data(), 0, (size_t)std::max(gslice->num_nodes, 1) * sizeof(int), ctx.stream()));
    reset_hashs(0, ctx);
  }

  // the reference redraws its random hashes per round; here they are the keys of round `iteration`, computed from the id
  void reset_hashs(int iteration, standard_context_t& ctx) {
    int* const h = d_hashs.data();
    const unsigned salt = mgx::color_salt(seed, iteration);
    transform([=] __device__(int v) { h[v] = (int)(mgx::color_key(v, salt) ^ 0x80000000u); }, gslice->num_nodes, ctx);
  }
};

}  // namespace coloring
}  // namespace gunrock
