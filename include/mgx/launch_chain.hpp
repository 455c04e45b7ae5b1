// mgx/launch_chain.hpp -- the host side of a chain of launches that ends on the device (the fused SCC and the label propagation):
// launch i reads what launch i - 1 left in a ring word and derives its own kind; launches behind the end return at once.  The
// host enqueues batches of CHAIN_BATCH_MIN, 2 x, 4 x ... up to CHAIN_BATCH_MAX launches and waits once per batch.
#pragma once
#include <algorithm>

#include "runtime.hpp"

namespace mgx {

constexpr int CHAIN_BATCH_MIN = 64;           // launches per host wait: 64, 128, 256, 256 ...
constexpr int CHAIN_BATCH_MAX = 256;

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

}  // namespace mgx
