// gunrock/lspar/lspar_problem.hxx -- state of the local sparsification the operator path runs (mgx_lspar_enact).
// The reference's lspar_problem_t (gunrock/src/lspar/lspar_problem.hxx): the data-slice fields d_hashs, d_minwise_hashs,
// d_thresholds, d_sims and the {eid, sim} record sim_edge_t.  What differs: the hashes are not std::rand()
// but colouring's h_j(v) = fmix32(v ^ salt_j) (mgx/color_hash.hpp), stored with bit 31 flipped so that the i32 minimum of
// the neighbourhood reduce orders them as unsigned; k hash functions (1 .. 32) instead of "only k = 1"; the keep count is
// mgx::lspar_keep (the guarded double pow), not floor(__powf); and the result is written, not left uninitialised.
#pragma once
#include "../../mgx/color_hash.hpp"
#include "../../mgx/lspar_fused.hpp"
#include "../problem.hxx"

namespace gunrock {
namespace lspar {

struct lspar_problem_t : problem_t {
  struct sim_edge_t {          // one entry of a row: its index into col_indices and its similarity (an integer 0 .. k)
    int eid;
    float sim;
  };
  struct data_slice_t {        // what the functors dereference on the device
    int* d_hashs;              // h_j(v) ^ 0x80000000 for the hash function being reduced, by vertex
    unsigned* d_minwise_hashs; // n x k, vertex-major: mh_j(v)
    int* d_thresholds;         // t(v)
    sim_edge_t* d_sims;        // per entry (by edge id)
    int num_hashs;             // k
  };

  unsigned seed;
  int k;
  double e;
  mem_t<int> d_hashs, d_reduced, d_thresholds;
  mem_t<unsigned> d_minwise_hashs;
  mem_t<sim_edge_t> d_sims;
  mem_t<data_slice_t> d_data_slice;

  lspar_problem_t(std::shared_ptr<graph_device_t> graph, unsigned seed_, int k_, double e_, standard_context_t& ctx)
      : problem_t(graph) {
    const size_t n = (size_t)std::max(graph->num_nodes, 1);
    d_hashs = mem_t<int>(n, ctx);
    d_reduced = mem_t<int>(n, ctx);
    d_thresholds = mem_t<int>(n, ctx);
    d_sims = mem_t<sim_edge_t>((size_t)std::max(graph->num_edges, 1), ctx);
    reset(seed_, k_, e_, ctx);
  }
  lspar_problem_t(const lspar_problem_t&) = delete;
  lspar_problem_t& operator=(const lspar_problem_t&) = delete;

  // the parameters of the next run: the minhash table sized for k, the keep counts t(v) (asynchronous on the context's stream)
  void reset(unsigned seed_, int k_, double e_, standard_context_t& ctx) {
    seed = seed_; k = k_; e = e_;
    const size_t cells = (size_t)std::max(gslice->num_nodes, 1) * k;
    if (d_minwise_hashs.size() < cells) {
      ctx.synchronize();
      d_minwise_hashs = mem_t<unsigned>(cells, ctx);
    }
    d_data_slice = to_mem(std::vector<data_slice_t>(1, data_slice_t{d_hashs.data(), d_minwise_hashs.data(), d_thresholds.data(),
                                                                    d_sims.data(), k}), ctx);
    const int* const ro = gslice->d_row_offsets.data();
    int* const t = d_thresholds.data();
    const double ee = e;
    transform([=] __device__(int v) { t[v] = mgx::lspar_keep(ro[v + 1] - ro[v], ee); }, gslice->num_nodes, ctx);
  }

  // the hashes of function j, computed from the id (the reference fills them from std::rand() once)
  void reset_hashs(int j, standard_context_t& ctx) {
    int* const h = d_hashs.data();
    const unsigned salt = mgx::color_salt(seed, j);
    transform([=] __device__(int v) { h[v] = (int)(mgx::color_key(v, salt) ^ 0x80000000u); }, gslice->num_nodes, ctx);
  }
};

}  // namespace lspar
}  // namespace gunrock
