// mgx/pack20.hpp -- unit-block entries at 20 bits: what the packer (mgx_layout.hip: k_pack20) writes and the unit-block body
// (bfs_fused_dense.hpp) reads.  For the blocks WITHOUT the cold-edge lists' entries only: every id in them lies inside the LDS
// prefix (< 32 * BFS_DENSE_HOTW = 652 288 < 2^20 - 1); "no entry" (-1: padding, the lanes of inactive units) is all ones, 0xFFFFF.
// The ids use bit 19 (524 288 .. 652 287), so the fields are UNSIGNED: a sign-extending unpack (what the 24-bit copy does, whose
// ids leave bit 23 free) would turn a fifth of the prefix into negative numbers.  unpack20 hands 0xFFFFF back as it is, and
// pack20_id turns it into -1 for whoever needs the id; the unit-block body does not: 0xFFFFF lies behind the prefix, where its
// probe reads the word "behind", all ones on every slot that reads these blocks (they run the cold-edge pass) -- visited, as -1 is.
//
// Arrangement: a CHUNK is 512 consecutive entries (8 units) in 320 words -- a plane of 64 x 4 words, then a plane of 64 x 1
// word.  Lane l of a wave holds the chunk's entries 8 l .. 8 l + 7 (all of unit l >> 3 of the chunk) as 160 bits, little endian
// (entry k in bits [20 k, 20 k + 20)): words 0..3 at plane A [4 l .. 4 l + 3], word 4 at plane B [l].  A wave reads a chunk with
// one 16-byte and one 4-byte load per lane, both aligned, unconditional and coalesced (1 KB + 256 B).
//
// Host and device: the arithmetic below is plain C++ but for the two builtins of the device side (tools/host_pack20 runs it
// under the sanitizers against a bit-by-bit reference).
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGX_PACK20_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MGX_PACK20_HD inline
#endif

namespace mgx {

constexpr unsigned PACK20_CHUNK_ENTRIES = 512;      // 8 units
constexpr unsigned PACK20_CHUNK_WORDS = 320;        // 512 * 20 / 32
constexpr unsigned PACK20_PLANE_B = 256;            // word offset of the 64 x 1-word plane inside a chunk
constexpr unsigned PACK20_SLACK_WORDS = 8;          // all ones behind the last chunk: what the lanes of inactive units read

// words of `entries` entries (a multiple of 512) and the slack behind them
constexpr size_t pack20_words(size_t entries) { return entries / PACK20_CHUNK_ENTRIES * PACK20_CHUNK_WORDS + PACK20_SLACK_WORDS; }
// where lane l of chunk c finds its words 0..3 / its word 4
constexpr size_t pack20_word_a(size_t chunk, unsigned lane) { return chunk * PACK20_CHUNK_WORDS + 4u * lane; }
constexpr size_t pack20_word_b(size_t chunk, unsigned lane) { return chunk * PACK20_CHUNK_WORDS + PACK20_PLANE_B + lane; }

// (hi : lo) >> s, low word -- v_alignbit_b32; s in 1..31
MGX_PACK20_HD unsigned pack20_alignbit(unsigned hi, unsigned lo, unsigned s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, s);
#else
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> s);
#endif
}
// bits [off, off + 20) of w -- v_bfe_u32; off in 0..12
MGX_PACK20_HD unsigned pack20_bfe20(unsigned w, unsigned off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ubfe(w, off, 20);
#else
  return (w >> off) & 0xFFFFFu;
#endif
}
constexpr unsigned PACK20_NONE = 0xFFFFFu;          // "no entry"
// a field as the id it stands for
MGX_PACK20_HD int pack20_id(unsigned f) { return f == PACK20_NONE ? -1 : (int)f; }

// eight entries (ids below 2^20 - 1, or -1 -> all ones) -> five words
MGX_PACK20_HD void pack20(const int e[8], unsigned w[5]) {
  unsigned f[8];
  for (int k = 0; k < 8; ++k) f[k] = (unsigned)e[k] & 0xFFFFFu;
  w[0] = f[0] | (f[1] << 20);
  w[1] = (f[1] >> 12) | (f[2] << 8) | (f[3] << 28);
  w[2] = (f[3] >> 4) | (f[4] << 16);
  w[3] = (f[4] >> 16) | (f[5] << 4) | (f[6] << 24);
  w[4] = (f[6] >> 8) | (f[7] << 12);
}

// ... and back (the fields, zero-extended): 12 vector instructions per eight entries -- a field inside a word is one v_bfe_u32,
// one that straddles two words v_alignbit_b32 + v_bfe_u32, the last one a shift
MGX_PACK20_HD void unpack20(unsigned w0, unsigned w1, unsigned w2, unsigned w3, unsigned w4, unsigned d[8]) {
  d[0] = pack20_bfe20(w0, 0);
  d[1] = pack20_bfe20(pack20_alignbit(w1, w0, 20), 0);
  d[2] = pack20_bfe20(w1, 8);
  d[3] = pack20_bfe20(pack20_alignbit(w2, w1, 28), 0);
  d[4] = pack20_bfe20(pack20_alignbit(w3, w2, 16), 0);
  d[5] = pack20_bfe20(w3, 4);
  d[6] = pack20_bfe20(pack20_alignbit(w4, w3, 24), 0);
  d[7] = w4 >> 12;
}

}  // namespace mgx
