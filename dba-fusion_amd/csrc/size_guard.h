// The size guard of the calls whose outputs are sized on the host from a remembered plan block (update_inputs.hip:
// dba_update_inputs_payload; vio_window.hip: dba_vio_window_payload).  The payload launch compares the N words its
// outputs were sized for with the words this call's plan launch left; on a mismatch it writes zeros and ONE lane reports
// through pinned, host-coherent words, which the next call polls without touching the device:
//   [0] raised, sticky until polled   [1..N] the plan's words   [N+1..2N] the words the outputs were sized for
// Each .hip file keeps a SizeGuard of its own: the reports of two calls never mix.
#pragma once
#include <string.h>

#include <mutex>

#include "common.h"

namespace dba {

constexpr int GUARD_WORDS = 16;  // 1 + 2 N of them are used, N <= 7

// The caller decides which lane runs it (one lane, once per launch) and what makes the launch not ok.  The words are
// fenced system-wide before the flag: a host that sees [0] raised sees them.
template <int N>
__device__ __forceinline__ void guard_report(int *status, const int (&got)[N], const int (&exp)[N]) {
  static_assert(1 + 2 * N <= GUARD_WORDS, "the report does not fit the pinned words");
#pragma unroll
  for (int k = 0; k < N; k++) status[1 + k] = got[k];
#pragma unroll
  for (int k = 0; k < N; k++) status[1 + N + k] = exp[k];
  __threadfence_system();
  status[0] = 1;
}

struct SizeGuard {
  std::mutex mu;
  int *pinned = nullptr;

  // the pinned words for a launch, allocated zeroed at first use (Portable: every device's kernels may write them)
  int words(int **out) {
    std::lock_guard<std::mutex> lock(mu);
    if (!pinned) {
      void *p = nullptr;
      DBA_HIP_CHECK(hipHostMalloc(&p, sizeof(int) * GUARD_WORDS,
                                  hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
      memset(p, 0, sizeof(int) * GUARD_WORDS);
      pinned = static_cast<int *>(p);
    }
    *out = pinned;
    return DBA_OK;
  }

  // 1 and words [1..n] in out (may be null) if a report is pending, which it clears; else 0.  No device call.
  int poll(int *out, int n) {
    std::lock_guard<std::mutex> lock(mu);
    if (!pinned) return 0;
    volatile int *w = pinned;
    if (!w[0]) return 0;
    if (out)
      for (int k = 0; k < n; k++) out[k] = w[1 + k];
    w[0] = 0;
    return 1;
  }
};

}  // namespace dba
