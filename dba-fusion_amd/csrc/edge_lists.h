// Device helpers of the one-workgroup kernels that edit edge lists: select_edges_kernel (factors.hip),
// add_factors_plan_kernel (add_factors.hip), update_inputs_edge_kernel (update_inputs.hip), vio_window_plan_kernel
// (vio_window.hip) and filter_repeated_edges_kernel (proximity.hip).  Integer index work, no atomics: every result is in
// the input's order.
// segment_reduce_kernel (upsample.hip) keeps a ballot compaction of its own: it is a many-workgroup throughput kernel
// with another barrier placement.
#pragma once
#include "common.h"

namespace dba {

// The order-preserving compaction of a workgroup of THREADS lanes.  All lanes call it; it returns the lane's slot among
// the raised flags in lane order and writes their number to *total.  Each wave ballots its flags, the wave counts go
// through wcount [THREADS / WAVE] in LDS, and a lane's slot is the count of the waves before it plus the popcount of the
// ballot below the lane.  Two barriers: the caller may reuse wcount at once.
template <int THREADS>
__device__ __forceinline__ int flag_slot(bool f, int *wcount, int *total) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint64_t m = __ballot(f);
  if (lane == 0) wcount[wv] = __popcll(m);
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < THREADS / WAVE; w++) {
    const int s = wcount[w];
    if (w < wv) before += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// The repeated-edge filter (covisible_graph.py:61-72) against one standing list: clears fresh[t] of every proposal
// (a[t], b[t]), t < tiles, that occurs in (ei, ej)[0, n).  A lane holds PER proposals in registers; the list passes
// through sx in LDS in tiles of THREADS entries.  All lanes call it, with one `tiles`.
template <int THREADS, int PER>
__device__ __forceinline__ void strike_listed(const int64_t *__restrict__ ei, const int64_t *__restrict__ ej, int n,
                                              const int64_t (&a)[PER], const int64_t (&b)[PER], bool (&fresh)[PER],
                                              int tiles, int64_t (&sx)[2][THREADS]) {
  const int tid = threadIdx.x;
  for (int e0 = 0; e0 < n; e0 += THREADS) {
    const int ne = min(n - e0, THREADS);
    __syncthreads();
    if (tid < ne) { sx[0][tid] = ei[e0 + tid]; sx[1][tid] = ej[e0 + tid]; }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PER; t++) {
      if (t >= tiles) break;
      if (fresh[t])
        for (int e = 0; e < ne; e++)
          if (sx[0][e] == a[t] && sx[1][e] == b[t]) { fresh[t] = false; break; }
    }
  }
}

}  // namespace dba
