// Forwarding header: code written against mini-gunrock includes <moderngpu/kernel_segsort.hxx> for mgpu::segmented_sort
// (the reference's lspar_enactor.hxx:85).  Here it is mgx's own stable segmented sort (mgx/segsort.hpp), new HIP
// for gfx950; nothing of moderngpu is used.  The same two shapes: keys only and keys + values, segments given by their
// heads, sorted in place on the context's stream.
#pragma once
#include "../../mgx/segsort.hpp"

#ifndef MGPU_DEVICE
#define MGPU_DEVICE __device__
#endif

namespace mgx {

template <typename key_t, typename comp_t>
void segmented_sort(key_t* keys, long long count, const int* segments, int num_segments, comp_t comp, standard_context_t& context) {
  segmented_sort_impl<key_t, segsort_no_value_t>(keys, nullptr, count, segments, num_segments, comp, context);
}

template <typename key_t, typename val_t, typename comp_t>
void segmented_sort(key_t* keys, val_t* vals, long long count, const int* segments, int num_segments, comp_t comp,
                    standard_context_t& context) {
  segmented_sort_impl<key_t, val_t>(keys, vals, count, segments, num_segments, comp, context);
}

}  // namespace mgx

namespace mgpu = mgx;
