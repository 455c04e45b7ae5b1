// mgx/worklist.hpp -- wave-level appends to device lists that many waves fill at once (the fused algorithms' work lists, the
// segmented sort's classification).  Every function is called by all 64 lanes of a wave together; lanes that have nothing
// to add pass false.
#pragma once
#include "wave.hpp"

namespace mgx {

// A wave's items wait in a wave-private LDS stage and go out a stage at a time behind one returning add: a list's counter is a
// single word every wave of the device adds to, and adds to one word are serialised (one add per surviving long row cost a
// uniform RMAT-22 colouring round ~19 ms).
// The stage is written by some lanes and read by others without a workgroup barrier, and the compiler reasons per thread
// (wave.hpp: wave_lds_fence): the first fence orders the lanes' stage writes before the copy out, the second the copy's reads
// before the stage is filled again.
template <typename T>
__device__ __forceinline__ void wave_stage_flush(T* stage, int& fill, T* out, int* counter) {
  if (fill == 0) return;
  wave_lds_fence();
  int base = 0;
  if (lane_id() == 0) base = atomicAdd(counter, fill);
  base = __shfl(base, 0, WAVE);
  for (int k = lane_id(); k < fill; k += WAVE) out[base + k] = stage[k];
  wave_lds_fence();
  fill = 0;
}

// lanes with `take` put `item` into the stage of CAP slots (CAP >= WAVE), which goes out first when they do not fit
template <int CAP, typename T>
__device__ __forceinline__ void wave_stage_push(bool take, T item, T* stage, int& fill, T* out, int* counter) {
  const u64 m = __ballot(take);
  if (!m) return;
  const int k = __popcll(m);
  if (fill + k > CAP) wave_stage_flush(stage, fill, out, counter);
  if (take) stage[fill + rank_in_mask(m)] = item;
  fill += k;
}

// unstaged: lanes with `take` append `item` behind one add per call (lists few waves add to)
__device__ __forceinline__ void wave_append(bool take, int item, int* list, int* counter) {
  const u64 m = __ballot(take);
  if (!m) return;
  int base = 0;
  if (lane_id() == 0) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, 0, WAVE);
  if (take) list[base + rank_in_mask(m)] = item;
}

// a long row's pieces: lanes with `keep` append (item, 0) .. (item, segs - 1), segs = len entries in segments of seg, behind one
// add per call for all the lanes' rows
__device__ __forceinline__ void wave_append_segments(bool keep, int item, int len, int seg, int2* out, int* counter) {
  if (!__ballot(keep)) return;
  const int segs = keep ? (len + seg - 1) / seg : 0;
  const int incl = wave_inclusive_sum(segs);
  int base = 0;
  if (lane_id() == WAVE - 1) base = atomicAdd(counter, incl);
  base = __shfl(base, WAVE - 1, WAVE);
  for (int s = 0; s < segs; ++s) out[base + incl - segs + s] = make_int2(item, s);
}
// the same for loops that count their scalar registers: rare there, and not inlined, since the scan inside it would cost the
// caller's loop scalar registers it does not have
__device__ __noinline__ void wave_append_segments_outlined(bool keep, int item, int len, int seg, int2* out, int* counter) {
  wave_append_segments(keep, item, len, seg, out, counter);
}

}  // namespace mgx
