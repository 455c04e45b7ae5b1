// mgx/color_hash.hpp -- the hash the colouring's keys are made of, host and device; the connected components' sample and
// the sparsification's minhashes use the same functions (tests/coloring_model.py, cc_model.py and lspar_model.py model them).
#pragma once
#include <hip/hip_runtime.h>

namespace mgx {

__host__ __device__ __forceinline__ unsigned color_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ unsigned color_salt(unsigned seed, int round) {
  return color_fmix32(seed + 0x9E3779B9u * (unsigned)(round + 1));
}
__host__ __device__ __forceinline__ unsigned color_key(int v, unsigned salt) { return color_fmix32((unsigned)v ^ salt); }

}  // namespace mgx
