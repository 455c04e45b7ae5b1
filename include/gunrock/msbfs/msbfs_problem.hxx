// gunrock/msbfs/msbfs_problem.hxx -- state of the bit-parallel multi-source BFS the operator path runs (mgx_msbfs_enact, DESIGN
// 3.16): the same 64-bit words per vertex as the fused path (mgx/msbfs_fused.hpp), in arrays of its own.
#pragma once
#include "../problem.hxx"

namespace gunrock {
namespace msbfs {

struct msbfs_scalars_t {
  int batch;                   // the batch the operators are working on
  int valid;                   // its sources
};

struct msbfs_problem_t : problem_t {
  struct data_slice_t {        // what the functors dereference on the device
    unsigned long long* d_seen;      // n
    unsigned long long* d_front;     // 2 n: the front of level t in half t & 1
    unsigned long long* d_next;      // n
    long long* d_reach_in;           // n
    long long* d_far_in;             // n
    unsigned long long* d_cnt;       // 64: the vertices found per bit at the level being finalized
    long long* d_per_src;            // cap reach | cap far | cap ecc | cap harm (double)
    int* d_depth;                    // count x n (NULL: not kept)
    const int* d_sources;            // count ids (NULL: source i is vertex i)
    msbfs_scalars_t* d_scalars;
    int n, cap;
  };

  mem_t<data_slice_t> d_data_slice;

  msbfs_problem_t(std::shared_ptr<graph_device_t> graph, const data_slice_t& slice, standard_context_t& ctx) : problem_t(graph) {
    d_data_slice = to_mem(std::vector<data_slice_t>(1, slice), ctx);
  }
  msbfs_problem_t(const msbfs_problem_t&) = delete;
  msbfs_problem_t& operator=(const msbfs_problem_t&) = delete;
};

// the arrays the problem points at; the per-source ones and the depths grow with the largest run
struct msbfs_state_t {
  mem_t<unsigned long long> d_words;           // N seen | 2 N front | N next | 64 counts
  mem_t<long long> d_sums;                     // N reach_in | N far_in
  mem_t<long long> d_per_src;
  mem_t<int> d_depth, d_sources;
  mem_t<msbfs_scalars_t> d_scalars;
  std::vector<long long> h_per_src;
  size_t N = 1, depth_cap = 0;
  int cap = 0;
  bool kept_depths = false;
  msbfs_state_t(int num_nodes, standard_context_t& ctx) {
    N = (size_t)std::max(num_nodes, 1);
    d_words = mem_t<unsigned long long>(4 * N + 64, ctx);
    d_sums = mem_t<long long>(2 * N, ctx);
    d_scalars = mem_t<msbfs_scalars_t>(1, ctx);
  }
  void ensure(long long count, bool want_depths, int n, standard_context_t& ctx) {
    if (count > cap) {
      d_per_src = mem_t<long long>(4 * (size_t)count, ctx);
      d_sources = mem_t<int>((size_t)count, ctx);
      h_per_src.assign(4 * (size_t)count, 0);
      cap = (int)count;
    }
    if (want_depths && (size_t)count * (size_t)n > depth_cap) {
      d_depth = mem_t<int>();
      depth_cap = 0;
      d_depth = mem_t<int>((size_t)count * (size_t)n, ctx);
      depth_cap = (size_t)count * (size_t)n;
    }
  }
  msbfs_problem_t::data_slice_t slice(int n, bool want_depths, bool have_sources) const {
    msbfs_problem_t::data_slice_t s;
    s.d_seen = d_words.data(); s.d_front = d_words.data() + N; s.d_next = d_words.data() + 3 * N; s.d_cnt = d_words.data() + 4 * N;
    s.d_reach_in = d_sums.data(); s.d_far_in = d_sums.data() + N;
    s.d_per_src = d_per_src.data();
    s.d_depth = want_depths ? d_depth.data() : nullptr;
    s.d_sources = have_sources ? d_sources.data() : nullptr;
    s.d_scalars = d_scalars.data();
    s.n = n; s.cap = cap;
    return s;
  }
};

}  // namespace msbfs
}  // namespace gunrock
