// The window rollup's buffer rotation, in place (include/dba_hip.h "window rollup"):
//
//   dba_roll_rows   <- the twelve torch.roll(x, -roll, 0) statements of DBAFusionFrontend.__rollup over the video buffers
//                      (dbaf/dbaf_frontend.py:94-105) and the `-= roll` of video.cur_ii / cur_jj (:121-122)
//
// ONE launch, no scratch buffer, every byte read once and written once.  new[r] = old[(r + roll) mod R] decomposes the
// rows of a buffer into gcd(R, roll) disjoint cycles r, r + roll, r + 2 roll, ... (mod R) of R / gcd rows each; in live
// mode (only rows [0, live) hold frames, new[r] = old[r + roll] for r < live - roll) into min(roll, live - roll) open
// chains.  A work item is one such walk x one column element of the buffer's vector width (row_jobs.h: the widest of
// 16 / 8 / 4 / 2 / 1 bytes dividing the base address and the row size), and a workgroup is 256 neighbouring columns of one
// walk.  The lane that owns an item is the only thread of the grid that ever reads or writes those bytes, so there is
// nothing to synchronise: no LDS, no atomics, plain vector loads and stores.  A lane loads up to ROLL_GROUP rows of its
// walk before it stores the first (the reference's R = 80, roll = 30 has cycles of exactly 8 rows: one group); longer
// walks go on in such groups, and a cycle's first row waits in registers to close it.  The grid ends with the workgroups
// that subtract roll from the int64 lists.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "row_jobs.h"

namespace dba {

constexpr int ROLL_THREADS = MOVE_THREADS;
constexpr int ROLL_GROUP = 8;  // rows in flight per lane, a cycle's carried first row included

struct RollJobDev {
  char *base;
  long long row_elems;        // row bytes / width
  int rows, roll, live;       // roll reduced to (0, rows); live < 0: cycles, else chains below row `live`
  int width, walks;           // walks: gcd(rows, roll) cycles, or min(roll, live - roll) chains
  unsigned wg_start, chunks;  // first workgroup of the buffer; workgroups per walk
};

struct RollTable {
  RollJobDev j[DBA_MAX_SHIFT_BUFS];
  int n;
  int n_lists;
  long long *list[DBA_MAX_ROLL_LISTS];
  long long list_len[DBA_MAX_ROLL_LISTS];
  unsigned list_wg_start[DBA_MAX_ROLL_LISTS];
  unsigned lists_wg0;  // first workgroup of the lists
  long long sub;       // what the lists lose: the caller's roll, not reduced
};

// N steps of a walk from row `cur`: the N rows that follow it are loaded, then stored one place back.  Returns the row
// the walk stands on afterwards (its old content is in flight no more: it was the last one loaded).
template <typename T, int N>
__device__ __forceinline__ int roll_steps(T *col, long long row_elems, int rows, int roll, int cur) {
  T v[N];
  int q = cur;
#pragma unroll
  for (int u = 0; u < N; u++) {
    q += roll;
    if (q >= rows) q -= rows;
    v[u] = col[(long long)q * row_elems];
  }
  q = cur;
#pragma unroll
  for (int u = 0; u < N; u++) {
    col[(long long)q * row_elems] = v[u];
    q += roll;
    if (q >= rows) q -= rows;
  }
  return q;
}

// One walk of one column: `steps` moves new[p_k] = old[p_k+1] from row p0 on; closed: the last row takes old[p0].  The
// tail is dispatched on its length so that every group is straight-line code (a per-load test on a run-time count would
// make the compiler wait for each load in turn).
template <typename T>
__device__ __forceinline__ void roll_walk(T *col, long long row_elems, int rows, int roll, int p0, int steps, bool closed) {
  T first = T();
  if (closed) first = col[(long long)p0 * row_elems];
  int cur = p0;
  constexpr int G = ROLL_GROUP - 1;  // with `first`: ROLL_GROUP loads in flight
  switch (steps % G) {
    case 1: cur = roll_steps<T, 1>(col, row_elems, rows, roll, cur); break;
    case 2: cur = roll_steps<T, 2>(col, row_elems, rows, roll, cur); break;
    case 3: cur = roll_steps<T, 3>(col, row_elems, rows, roll, cur); break;
    case 4: cur = roll_steps<T, 4>(col, row_elems, rows, roll, cur); break;
    case 5: cur = roll_steps<T, 5>(col, row_elems, rows, roll, cur); break;
    case 6: cur = roll_steps<T, 6>(col, row_elems, rows, roll, cur); break;
    default: break;
  }
  for (int k = steps / G; k > 0; k--) cur = roll_steps<T, G>(col, row_elems, rows, roll, cur);
  if (closed) col[(long long)cur * row_elems] = first;
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_rows_kernel(RollTable t) {
  const unsigned bid = blockIdx.x;
  if (bid >= t.lists_wg0) {  // the int64 lists; constant indices and selects, as for the buffers below
    long long *p = t.list[0];
    long long len = t.list_len[0];
    unsigned start = t.list_wg_start[0];
#pragma unroll
    for (int q = 1; q < DBA_MAX_ROLL_LISTS; q++)
      if (q < t.n_lists && bid >= t.list_wg_start[q]) {
        p = t.list[q];
        len = t.list_len[q];
        start = t.list_wg_start[q];
      }
    const long long i = (long long)(bid - start) * ROLL_THREADS + threadIdx.x;
    if (i < len) p[i] -= t.sub;
    return;
  }
  // the workgroup's (buffer, walk, chunk): the table stays in scalar registers (row_jobs.h run_row_jobs)
  RollJobDev J = t.j[0];
#pragma unroll
  for (int q = 1; q < DBA_MAX_SHIFT_BUFS; q++)
    if (q < t.n && bid >= t.j[q].wg_start) J = t.j[q];
  const unsigned local = bid - J.wg_start;
  const int walk = (int)(local / J.chunks);
  const unsigned c = local - (unsigned)walk * J.chunks;
  const long long e = (long long)c * ROLL_THREADS + threadIdx.x;
  if (e >= J.row_elems) return;
  const bool closed = J.live < 0;
  // cycles: the rows congruent to `walk` mod gcd, rows / gcd of them; chains: walk, walk + roll, ... below `live`
  const int steps = closed ? J.rows / J.walks - 1 : (J.live - walk - 1) / J.roll;
  char *col = J.base + e * J.width;
  switch (J.width) {
    case 16: roll_walk((u32x4 *)col, J.row_elems, J.rows, J.roll, walk, steps, closed); break;
    case 8: roll_walk((uint64_t *)col, J.row_elems, J.rows, J.roll, walk, steps, closed); break;
    case 4: roll_walk((uint32_t *)col, J.row_elems, J.rows, J.roll, walk, steps, closed); break;
    case 2: roll_walk((uint16_t *)col, J.row_elems, J.rows, J.roll, walk, steps, closed); break;
    default: roll_walk((uint8_t *)col, J.row_elems, J.rows, J.roll, walk, steps, closed); break;
  }
}

}  // namespace dba

using namespace dba;

static int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t r = a % b;
    a = b;
    b = r;
  }
  return a;
}

extern "C" {

int dba_roll_rows(void *const *bases, const int64_t *row_bytes, const int64_t *rows, int n_bufs, int64_t roll, int64_t live,
                  int64_t *const *lists, const int64_t *list_lens, int n_lists, dba_stream_t stream) {
  if (n_bufs < 0 || n_bufs > DBA_MAX_SHIFT_BUFS || (n_bufs > 0 && (!bases || !row_bytes || !rows))) return DBA_ERR_ARG;
  if (n_lists < 0 || n_lists > DBA_MAX_ROLL_LISTS || (n_lists > 0 && (!lists || !list_lens))) return DBA_ERR_ARG;
  RollTable t{};
  uint64_t wgs = 0;
  for (int k = 0; k < n_bufs; k++) {
    const int64_t R = rows[k], rb = row_bytes[k];
    if (R < 0 || rb < 0 || R > INT32_MAX) return DBA_ERR_ARG;
    if (live >= 0 && !(0 <= roll && roll <= live && live <= R)) return DBA_ERR_ARG;
    if (R > 0 && rb > 0 && !bases[k]) return DBA_ERR_ARG;
    if (R == 0 || rb == 0) continue;
    const int64_t r = live >= 0 ? roll : ((roll % R) + R) % R;  // as torch.roll reduces its shift
    const int64_t walks = live >= 0 ? (r < live - r ? r : live - r) : (r ? gcd64(R, r) : 0);
    if (walks == 0) continue;  // nothing moves: the buffer is left out of the grid
    RollJobDev &J = t.j[t.n++];
    J.base = (char *)bases[k];
    J.width = vector_width(bases[k], bases[k], rb);
    J.row_elems = rb / J.width;
    J.rows = (int)R;
    J.roll = (int)r;
    J.live = live >= 0 ? (int)live : -1;
    J.walks = (int)walks;
    const uint64_t chunks = (uint64_t)((J.row_elems + ROLL_THREADS - 1) / ROLL_THREADS);
    if (chunks > (uint64_t)INT32_MAX) return DBA_ERR_ARG;
    J.chunks = (unsigned)chunks;
    J.wg_start = (unsigned)wgs;
    wgs += chunks * (uint64_t)walks;
    if (wgs > (uint64_t)INT32_MAX) return DBA_ERR_ARG;
  }
  t.lists_wg0 = (unsigned)wgs;
  t.sub = roll;
  for (int k = 0; k < n_lists; k++) {
    if (list_lens[k] < 0 || (list_lens[k] > 0 && !lists[k])) return DBA_ERR_ARG;
    if (list_lens[k] == 0 || roll == 0) continue;
    const int q = t.n_lists++;
    t.list[q] = (long long *)lists[k];
    t.list_len[q] = list_lens[k];
    t.list_wg_start[q] = (unsigned)wgs;
    wgs += (uint64_t)((list_lens[k] + ROLL_THREADS - 1) / ROLL_THREADS);
    if (wgs > (uint64_t)INT32_MAX) return DBA_ERR_ARG;
  }
  if (wgs == 0) return DBA_OK;
  hipLaunchKernelGGL(roll_rows_kernel, dim3((unsigned)wgs), dim3(ROLL_THREADS), 0, (hipStream_t)stream, t);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
