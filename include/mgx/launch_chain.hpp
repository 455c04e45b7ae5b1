// mgx/launch_chain.hpp -- a chain of launches whose kinds are decided on the device (the fused k-core, k-truss, SCC, label
// propagation, multi-source BFS and Louvain): the protocol, device and host side, in its one place.
//
// The run's words live in device memory behind one pointer, a chain_control_t: a ring of four words, the run's totals, the log.
//   launch i   reads ring[i & 3], what launch i - 1 left: its kind, its level or iteration, what it counted.  A cleared word has
//              kind 0, which every algorithm calls INIT: the reset below is what makes launch 0 the first.
//              derives its own kind from it and leaves ring[(i + 1) & 3] for the next launch: the fields its first thread writes,
//              and the counters all its threads add to;
//              clears ring[(i + 2) & 3]: launch i - 2 read it last, launch i + 1 adds to it next;
//              logs its kind, the first CHAIN_LOG_CAP launches of a run;
//              returns at once when the launch before was the end already (kind DONE follows DONE).
//   the host   enqueues CHAIN_BATCH_MIN, 2 x, 4 x ... up to CHAIN_BATCH_MAX launches and waits once per batch, for the totals: a
//              `done` word among them ends the run; a run with more than `most` launches out has not ended, which is an error.
// Nothing is read back inside a launch, no launch is cooperative, and the launches behind the end are what a wait costs less.
// A timed run keeps the device's wall clock per phase (chain_clock_t): the first thread of launch i charges the time since launch
// i - 1 began to that launch's phase.
//
// Not chains of this kind, and not folded into it: PageRank's residual-driven batches, the colouring's round batches, the BFS chain
// (bfs_fused_chain.hpp) and BC's small-level chain batch or end differently.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "runtime.hpp"

namespace mgx {

constexpr int CHAIN_BATCH_MIN = 64;           // launches per host wait: 64, 128, 256, 256 ... (those behind the end are 2.3 us each)
constexpr int CHAIN_BATCH_MAX = 256;
constexpr int CHAIN_LOG_CAP = 1 << 16;        // launches whose kind a run keeps for its *_step_kinds

// The wall clock ticks of a timed run per phase, K phases: a member of the algorithm's totals.
template <int K>
struct chain_clock_t {
  long long clock[K];
  long long last_tick;
  // The first thread of every launch: the time since the launch before began is that launch's, `slot` its phase (INIT has none,
  // and behind DONE nothing is charged).
  __device__ __forceinline__ void tick(int timing, int prev_kind, int done_kind, int slot) {
    if (timing && prev_kind != done_kind) {
      const long long now = (long long)wall_clock64();
      if (prev_kind != 0) clock[slot] += now - last_tick;
      last_tick = now;
    }
  }
};

// Word: what a launch leaves for the next one; Totals: what the run counts and how it ended (the host reads them once per wait);
// CAP: the launches whose kind the log keeps.  The reset relies on this order of the members, and on nothing else.
template <typename Word, typename Totals, int CAP = CHAIN_LOG_CAP>
struct chain_control_t {
  Word ring[4];
  Totals totals;
  int log[CAP];

  // what the launch before left: by value for the top of the kernel, by pointer where a kernel reads a field again later rather
  // than keep the word in scalar registers
  __device__ __forceinline__ Word left_by_prev(unsigned launch) const { return ring[launch & 3]; }
  __device__ __forceinline__ const Word* left_by_prev_at(unsigned launch) const { return ring + (launch & 3); }
  __device__ __forceinline__ Word* for_next(unsigned launch) { return ring + ((launch + 1) & 3); }
  // (the first thread) read by launch i - 2 last, written by launch i + 1 next
  __device__ __forceinline__ void clear_ahead(unsigned launch) { *(ring + ((launch + 2) & 3)) = Word{}; }
  __device__ __forceinline__ void log_kind(unsigned launch, int kind) {
    if (launch < (unsigned)CAP) log[launch] = kind;
  }

  // Host side, on the device's copy: a run begins with the ring and the totals cleared (or the totals as `init`, pinned, holds
  // them); the log keeps the run before until the launches overwrite it.
  static void reset(chain_control_t* dev, hipStream_t st) { MGX_HIP(hipMemsetAsync(dev, 0, offsetof(chain_control_t, log), st)); }
  static void reset(chain_control_t* dev, const Totals* init, hipStream_t st) {
    MGX_HIP(hipMemcpyAsync(&dev->totals, init, sizeof(Totals), hipMemcpyHostToDevice, st));
    MGX_HIP(hipMemsetAsync(dev->ring, 0, sizeof(dev->ring), st));
  }
};

// enqueue(i): launch number i on the stream; fetch_done(): one host wait, true when the device has ended the run (it throws
// on what the device reports as a fault).  `most`: a run that has enqueued more launches than this has not ended: MGX_E_HIP.
// Returns the launches enqueued; *waits counts the host waits.
template <typename Enqueue, typename FetchDone>
inline long long run_launch_chain(Enqueue enqueue, FetchDone fetch_done, long long most, const char* what, long long* waits) {
  long long enqueued = 0;
  int batch = CHAIN_BATCH_MIN;
  for (;;) {
    for (int j = 0; j < batch; ++j, ++enqueued) enqueue(enqueued);
    MGX_CHECK_LAUNCH(what);
    const bool done = fetch_done();
    ++*waits;
    if (done) break;
    if (enqueued > most) throw mgx_error(MGX_E_HIP, std::string(what) + ": the run did not end");
    batch = std::min(batch * 2, CHAIN_BATCH_MAX);
  }
  return enqueued;
}

// the rate of wall_clock64() on the current device, asked once per process (0: the device does not say)
inline int wall_clock_khz() {
  static const int khz = [] {
    int dev = 0, rate = 0;
    MGX_HIP(hipGetDevice(&dev));
    MGX_HIP(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, dev));
    return rate;
  }();
  return khz;
}
// a chain_clock_t's ticks as milliseconds
inline double chain_ticks_ms(long long ticks) {
  const int khz = wall_clock_khz();
  return khz > 0 ? (double)ticks / (double)khz : 0.0;
}

}  // namespace mgx
