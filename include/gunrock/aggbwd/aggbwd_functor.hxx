// gunrock/aggbwd/aggbwd_functor.hxx -- the device functors of the backward aggregation's operator path.
//   win_functor_t   max / min only: the filter over the FORWARD rows gives a row to one lane, which walks it column by column,
//                   segment by segment, as the forward's row_functor_t does, and keeps the entry whose term the fold kept
//                   (mgx::aggb_take_op: the forward's comparison, the winner beside the value)
//   col_functor_t   the filter over the iota of GX's rows gives a TRANSPOSED row to one lane, which folds its slots' terms column
//                   by column, segment by segment, with mgx::agg_div (mean, before the weight), agg_term, aggb_pick and agg_comb_op
//                   in the definition's order: the same float32 bits by construction
// Neighbouring lanes read different rows: uncoalesced on purpose, this is the yardstick.  Nothing is kept.
#pragma once
#include "../intrinsics.hxx"
#include "aggbwd_problem.hxx"

namespace gunrock {
namespace aggbwd {

typedef aggbwd_problem_t::data_slice_t aggbwd_slice_t;

struct win_functor_t {
  static __device__ __forceinline__ bool cond_filter(int r, aggbwd_slice_t* d, int) {
    if (r < 0) return false;
    const int beg = d->ro[r];
    const int len = d->ro[r + 1] - beg;
    int* const out = d->win + (long long)r * d->ldw;
    for (int f = 0; f < d->feats; ++f) {
      float row = 0.f;
      int row_win = -1;
      for (int s0 = 0; s0 < len; s0 += d->seg) {
        const int s1 = min(len, s0 + d->seg);
        float acc = 0.f;
        int win = -1;
        for (int k = s0; k < s1; ++k) {
          const int e = beg + k;
          const float xv = d->x[(long long)d->ci[e] * d->ldx + f];
          const float t = d->w ? mgx::agg_term(d->w[d->entry_pos ? d->entry_pos[e] : e], xv) : xv;
          if (k == s0) { acc = t; win = e; }
          else mgx::aggb_take_op(d->op, acc, win, t, e);
        }
        if (s0 == 0) { row = acc; row_win = win; }
        else mgx::aggb_take_op(d->op, row, row_win, acc, win);
      }
      out[f] = row_win;
    }
    return false;
  }
};

struct col_functor_t {
  static __device__ __forceinline__ bool cond_filter(int c, aggbwd_slice_t* d, int) {
    if (c < 0) return false;
    const int beg = d->t_off[c];
    const int len = d->t_off[c + 1] - beg;
    const bool minmax = d->op == mgx::AGG_MAX || d->op == mgx::AGG_MIN;
    float* const out = d->gx + (long long)c * d->ldgx;
    for (int f = 0; f < d->feats; ++f) {
      float col = 0.f;
      for (int s0 = 0; s0 < len; s0 += d->seg) {
        const int s1 = min(len, s0 + d->seg);
        float acc = 0.f;
        for (int k = s0; k < s1; ++k) {
          const int r = d->t_row[beg + k], e = d->t_pos[beg + k];
          float g = d->gy[(long long)r * d->ldgy + f];
          if (d->op == mgx::AGG_MEAN) g = mgx::agg_div(g, (float)(d->ro[r + 1] - d->ro[r]));
          float u = d->w ? mgx::agg_term(d->w[d->entry_pos ? d->entry_pos[e] : e], g) : g;
          if (minmax) u = mgx::aggb_pick(d->win[(long long)r * d->ldw + f], e, u);
          acc = k == s0 ? u : mgx::agg_comb_op(mgx::AGG_SUM, acc, u);
        }
        col = s0 == 0 ? acc : mgx::agg_comb_op(mgx::AGG_SUM, col, acc);
      }
      out[f] = col;
    }
    return false;
  }
};

}  // namespace aggbwd
}  // namespace gunrock
