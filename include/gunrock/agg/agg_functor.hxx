// gunrock/agg/agg_functor.hxx -- the device functor of the neighbour feature aggregation's operator path.
//   row_functor_t   the filter over the rows gives a row to ONE lane, which walks it column by column, segment by segment, with the
//                   fused path's own term, combine and division (mgx::agg_term, agg_comb_op, agg_div) in the definition's order:
//                   the same float32 bits by construction.  Neighbouring lanes read different feature rows: uncoalesced on
//                   purpose, this is the yardstick.  Nothing is kept: the filter's count is the call's host wait.
#pragma once
#include "../intrinsics.hxx"
#include "agg_problem.hxx"

namespace gunrock {
namespace agg {

typedef agg_problem_t::data_slice_t agg_slice_t;

struct row_functor_t {
  static __device__ __forceinline__ bool cond_filter(int r, agg_slice_t* d, int) {
    if (r < 0) return false;
    const int beg = d->ro[r];
    const int len = d->ro[r + 1] - beg;
    float* const out = d->y + (long long)r * d->ldy;
    for (int f = 0; f < d->feats; ++f) {
      float row = 0.f;
      for (int s0 = 0; s0 < len; s0 += d->seg) {
        const int s1 = min(len, s0 + d->seg);
        float acc = 0.f;
        for (int k = s0; k < s1; ++k) {
          const int e = beg + k;
          const float xv = d->x[(long long)d->ci[e] * d->ldx + f];
          const float t = d->w ? mgx::agg_term(d->w[d->entry_pos ? d->entry_pos[e] : e], xv) : xv;
          acc = k == s0 ? t : mgx::agg_comb_op(d->op, acc, t);
        }
        row = s0 == 0 ? acc : mgx::agg_comb_op(d->op, row, acc);
      }
      if (d->op == mgx::AGG_MEAN && len > 0) row = mgx::agg_div(row, (float)len);
      out[f] = row;
    }
    return false;
  }
};

}  // namespace agg
}  // namespace gunrock
