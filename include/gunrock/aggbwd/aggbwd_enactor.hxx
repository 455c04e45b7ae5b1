// gunrock/aggbwd/aggbwd_enactor.hxx -- the backward aggregation on the filter operator (mgx_aggbwd_enact): the plain path, the
// fused path's cross-check and yardstick.
//   filter<win>   max / min only: one pass over the forward rows 0 .. R - 1, a lane per row -> win
//   filter<col>   one pass over the iota of GX's rows 0 .. x_rows - 1, a lane per transposed row; nothing is kept
// One operator call and its host wait (two for max / min), whatever the rows' lengths, on the transposed arrays the fused path
// builds and keeps (mgx::aggb_state_t::prepare).
#pragma once
#include "../filter.hxx"
#include "../frontier.hxx"
#include "../graph.hxx"
#include "aggbwd_functor.hxx"
#include "aggbwd_problem.hxx"

namespace gunrock {
namespace aggbwd {

struct aggbwd_enactor_t {
  typedef std::shared_ptr<frontier_t<int>> frontier_ptr;
  long long waits = 0, calls = 0;     // what the last enact() did
  frontier_ptr all, none;             // the rows; what a pass keeps (nothing)
  size_t room = 0;

  aggbwd_enactor_t() {}
  aggbwd_enactor_t(const aggbwd_enactor_t&) = delete;
  aggbwd_enactor_t& operator=(const aggbwd_enactor_t&) = delete;

  // the iota over as many rows as the largest call so far
  void ensure(int rows, standard_context_t& ctx) {
    if ((size_t)rows <= room) return;
    all = std::make_shared<frontier_t<int>>(ctx, (size_t)rows);
    none = std::make_shared<frontier_t<int>>(ctx, (size_t)rows);
    int* const ids = all->data()->data();
    transform([=] __device__(int v) { ids[v] = v; }, rows, ctx);
    room = (size_t)rows;
    mgx::frontier_touched();
  }

  void enact(std::shared_ptr<aggbwd_problem_t> p, int R, int x_rows, bool winners, standard_context_t& ctx) {
    waits = calls = 0;
    if (x_rows <= 0) return;
    ensure(std::max(R, x_rows), ctx);
    if (winners && R > 0) {
      all->resize((size_t)R);
      gunrock::oprtr::filter::filter_kernel<aggbwd_problem_t, win_functor_t>(p, all, none, 0, ctx);
      ++calls; ++waits;
    }
    all->resize((size_t)x_rows);
    gunrock::oprtr::filter::filter_kernel<aggbwd_problem_t, col_functor_t>(p, all, none, 0, ctx);
    ++calls; ++waits;
  }
};

}  // namespace aggbwd
}  // namespace gunrock
