// Sanitizer harness for the 20-bit unit-block entries (include/mgx/pack20.hpp): the packer's per-chunk arithmetic and the
// unpack of the unit-block body, compiled for the HOST (the two device builtins have plain-C++ stand-ins there) under
// AddressSanitizer + UndefinedBehaviorSanitizer by tools/host_pack20/run.sh.  No HIP call is made, no GPU is needed.
//   * every slot position of a lane's five words x {0, 1, 0x7FFFF, 0x80000, 0xFFFFE, all ones -> -1}, the seven other slots
//     holding the complement: a field that bleeds into its neighbour shows
//   * a few thousand random chunks (512 entries in 320 words, the arrangement the kernels read), -1 sprinkled in
//   * against a reference that moves the 160 bits one by one
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "mgx/pack20.hpp"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { if (failures < 20) std::printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } } while (0)

// the reference: entry k is bits [20 k, 20 k + 20) of the lane's 160 bits, little endian, written and read bit by bit
static void ref_pack(const int e[8], unsigned w[5]) {
  for (int i = 0; i < 5; ++i) w[i] = 0u;
  for (int k = 0; k < 8; ++k)
    for (int b = 0; b < 20; ++b)
      if (((unsigned)e[k] >> b) & 1u) { const int pos = 20 * k + b; w[pos / 32] |= 1u << (pos % 32); }
}
static void ref_unpack(const unsigned w[5], int d[8]) {
  for (int k = 0; k < 8; ++k) {
    unsigned f = 0u;
    for (int b = 0; b < 20; ++b) { const int pos = 20 * k + b; f |= ((w[pos / 32] >> (pos % 32)) & 1u) << b; }
    d[k] = f == 0xFFFFFu ? -1 : (int)f;
  }
}

static void round_trip(const int e[8], const char* what) {
  unsigned w[5], wr[5], f[8];
  int dr[8];
  mgx::pack20(e, w);
  ref_pack(e, wr);
  for (int i = 0; i < 5; ++i) EXPECT(w[i] == wr[i], what);
  mgx::unpack20(w[0], w[1], w[2], w[3], w[4], f);
  ref_unpack(w, dr);
  for (int k = 0; k < 8; ++k) {
    EXPECT(f[k] <= 0xFFFFFu, what);                      // nothing above the field
    EXPECT(mgx::pack20_id(f[k]) == e[k], what);
    EXPECT(dr[k] == e[k], what);
    EXPECT((f[k] == mgx::PACK20_NONE) == (e[k] == -1), what);
  }
}

int main() {
  const int values[] = {0, 1, 0x7FFFF, 0x80000, 0xFFFFE, -1};
  for (int slot = 0; slot < 8; ++slot)
    for (int v : values)
      for (int other = 0; other < 3; ++other) {          // the neighbours: the complement, all zeros, no entry
        int e[8];
        const int comp = (int)(~(unsigned)v & 0xFFFFFu);
        for (int k = 0; k < 8; ++k) e[k] = other == 0 ? (comp == 0xFFFFF ? -1 : comp) : other == 1 ? 0 : -1;
        e[slot] = v;
        round_trip(e, "slot x value");
      }
  // random chunks in the kernels' arrangement: lane l of chunk c holds entries 8 l .. 8 l + 7 in plane A [4 l ..] and plane B [l]
  std::mt19937 rng(20);
  const size_t chunks = 4096;
  const size_t entries = chunks * mgx::PACK20_CHUNK_ENTRIES;
  std::vector<int> col(entries);
  for (auto& x : col) { const unsigned r = rng(); x = (r >> 28) == 0 ? -1 : (int)((r & 0xFFFFFu) % 0xFFFFFu); }
  std::vector<unsigned> out(mgx::pack20_words(entries), 0u);
  EXPECT(out.size() == chunks * 320 + mgx::PACK20_SLACK_WORDS, "array size");
  for (size_t c = 0; c < chunks; ++c)
    for (unsigned l = 0; l < 64; ++l) {
      unsigned w[5];
      mgx::pack20(&col[c * 512 + 8 * l], w);
      const size_t a = mgx::pack20_word_a(c, l), b = mgx::pack20_word_b(c, l);
      for (int i = 0; i < 4; ++i) out[a + i] = w[i];
      out[b] = w[4];
    }
  for (unsigned i = 0; i < mgx::PACK20_SLACK_WORDS; ++i) out[chunks * 320 + i] = 0xFFFFFFFFu;
  for (size_t c = 0; c < chunks; ++c)
    for (unsigned l = 0; l < 64; ++l) {
      const size_t a = mgx::pack20_word_a(c, l), b = mgx::pack20_word_b(c, l);
      EXPECT(a % 4 == 0 && a + 3 < b && b < (c + 1) * 320, "planes inside the chunk, 16-byte aligned");
      unsigned f[8];
      mgx::unpack20(out[a], out[a + 1], out[a + 2], out[a + 3], out[b], f);
      const unsigned w[5] = {out[a], out[a + 1], out[a + 2], out[a + 3], out[b]};
      int dr[8];
      ref_unpack(w, dr);
      for (int k = 0; k < 8; ++k) {
        EXPECT(mgx::pack20_id(f[k]) == col[c * 512 + 8 * l + k], "random chunk");
        EXPECT(dr[k] == col[c * 512 + 8 * l + k], "random chunk, reference");
      }
    }
  {  // what the lanes of inactive units read: the slack behind the last chunk, as a 16-byte and a 4-byte load
    const size_t s = chunks * 320;
    unsigned f[8];
    mgx::unpack20(out[s], out[s + 1], out[s + 2], out[s + 3], out[s + 4], f);
    for (int k = 0; k < 8; ++k) EXPECT(mgx::pack20_id(f[k]) == -1, "slack");
  }
  std::printf("host_pack20: %d failures\n", failures);
  return failures ? 1 : 0;
}
