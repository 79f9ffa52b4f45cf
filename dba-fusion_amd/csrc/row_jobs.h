// The row mover's job table and copy body, shared by the launches that move payload rows (factors.hip: dba_move_rows,
// dba_shift_rows; add_factors.hip: dba_add_factors_payload; vio_window.hip: dba_vio_window_payload).  A job copies
// `count` rows of row_elems * width bytes,
// dst[dst_row0 + r] = src[pos ? pos[r] : r]; the grid is the concatenation of every job's (row, chunk) pairs, a chunk
// being 1024 elements of the job's vector width (16 KB at 16 bytes), four loads in flight per lane before the first
// store.  Pure streaming: no LDS, plain vector stores.  A position outside [0, src_rows) copies nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/dba_hip.h"

namespace dba {

constexpr int MOVE_THREADS = 256;
constexpr int MOVE_UNROLL = 4;
constexpr int MOVE_CHUNK = MOVE_THREADS * MOVE_UNROLL;  // elements of the job's width per workgroup

struct RowJobDev {
  const char *src;  // nullptr (tables run with FILL only): the rows are zeroed
  char *dst;
  const int *pos;
  long long row_elems;  // row bytes / width
  int count, dst_row0, src_rows, width;
  unsigned wg_start, chunks;  // first workgroup of the job; workgroups per row
};

template <int N>
struct RowTable {
  RowJobDev j[N];
  int n;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void copy_chunk(const char *s, char *d, long long n, unsigned chunk) {
  const T *sp = (const T *)s;
  T *dp = (T *)d;
  const long long e0 = (long long)chunk * MOVE_CHUNK + threadIdx.x;
  T v[MOVE_UNROLL];
  if ((long long)(chunk + 1) * MOVE_CHUNK <= n) {
#pragma unroll
    for (int u = 0; u < MOVE_UNROLL; u++) v[u] = sp[e0 + u * MOVE_THREADS];
#pragma unroll
    for (int u = 0; u < MOVE_UNROLL; u++) dp[e0 + u * MOVE_THREADS] = v[u];
  } else {
#pragma unroll
    for (int u = 0; u < MOVE_UNROLL; u++)
      if (e0 + u * MOVE_THREADS < n) v[u] = sp[e0 + u * MOVE_THREADS];
#pragma unroll
    for (int u = 0; u < MOVE_UNROLL; u++)
      if (e0 + u * MOVE_THREADS < n) dp[e0 + u * MOVE_THREADS] = v[u];
  }
}

template <typename T>
__device__ __forceinline__ void zero_chunk(char *d, long long n, unsigned chunk) {
  T *dp = (T *)d;
  const long long e0 = (long long)chunk * MOVE_CHUNK + threadIdx.x;
#pragma unroll
  for (int u = 0; u < MOVE_UNROLL; u++)
    if (e0 + u * MOVE_THREADS < n) dp[e0 + u * MOVE_THREADS] = T(0);
}

// the workgroup's (job, row, chunk) and its copy.  The table is read with constant indices and the job picked by
// selects, so it stays in scalar registers (a dynamic index could send it through private memory).
template <int N, bool FILL = false>
__device__ __forceinline__ void run_row_jobs(const RowTable<N> &t) {
  const unsigned bid = blockIdx.x;
  RowJobDev J = t.j[0];
#pragma unroll
  for (int q = 1; q < N; q++)
    if (q < t.n && bid >= t.j[q].wg_start) J = t.j[q];
  const unsigned local = bid - J.wg_start;
  const unsigned r = local / J.chunks, c = local - r * J.chunks;
  if ((int)r >= J.count) return;
  const long long row_bytes = J.row_elems * J.width;
  char *d = J.dst + (long long)(J.dst_row0 + (int)r) * row_bytes;
  if (FILL && !J.src) {
    switch (J.width) {
      case 16: zero_chunk<u32x4>(d, J.row_elems, c); break;
      case 8: zero_chunk<uint64_t>(d, J.row_elems, c); break;
      case 4: zero_chunk<uint32_t>(d, J.row_elems, c); break;
      case 2: zero_chunk<uint16_t>(d, J.row_elems, c); break;
      default: zero_chunk<uint8_t>(d, J.row_elems, c); break;
    }
    return;
  }
  const int srow = J.pos ? J.pos[r] : (int)r;
  if (srow < 0 || srow >= J.src_rows) return;
  const char *s = J.src + srow * row_bytes;
  switch (J.width) {
    case 16: copy_chunk<u32x4>(s, d, J.row_elems, c); break;
    case 8: copy_chunk<uint64_t>(s, d, J.row_elems, c); break;
    case 4: copy_chunk<uint32_t>(s, d, J.row_elems, c); break;
    case 2: copy_chunk<uint16_t>(s, d, J.row_elems, c); break;
    default: copy_chunk<uint8_t>(s, d, J.row_elems, c); break;
  }
}

// ---- host side: filling a table ------------------------------------------------------------------------------------

// the checks every kind of job passes: no negative size, and the rows written fit dst
inline bool row_range_ok(const dba_row_job &j) {
  if (j.count < 0 || j.row_bytes < 0 || j.dst_row0 < 0 || j.src_rows < 0 || j.dst_rows < 0) return false;
  return (int64_t)j.dst_row0 + j.count <= j.dst_rows;
}

enum PosRule { POS_FORBIDDEN, POS_OPTIONAL, POS_REQUIRED };

// The one validation of a dba_row_job: DBA_ERR_ARG, 0 for a job that moves nothing (it is left out of the table) or 1
// for a job to push.  reads: the rows come from j.src, and `pos` says whether the job may, must or must not name them
// through j.pos; a job that reads nothing (its rows are zeroed) is asked for neither src nor pos.
inline int check_row_job(const dba_row_job &j, bool reads, PosRule pos) {
  if (!row_range_ok(j)) return DBA_ERR_ARG;
  if (reads) {
    if (pos == POS_FORBIDDEN && j.pos) return DBA_ERR_ARG;
    if (pos == POS_REQUIRED && j.count > 0 && !j.pos) return DBA_ERR_ARG;
    if (!j.pos && j.count > j.src_rows) return DBA_ERR_ARG;
  }
  if (j.count == 0 || j.row_bytes == 0) return 0;
  if (!j.dst || (reads && !j.src)) return DBA_ERR_ARG;
  if (reads) {
    const char *s0 = (const char *)j.src, *s1 = s0 + (int64_t)j.src_rows * j.row_bytes;
    const char *d0 = (const char *)j.dst + (int64_t)j.dst_row0 * j.row_bytes, *d1 = d0 + (int64_t)j.count * j.row_bytes;
    if (s0 < d1 && d0 < s1) return DBA_ERR_ARG;  // the rows read and the rows written overlap
  }
  return 1;
}

// the widest of 16 / 8 / 4 / 2 / 1 bytes that divides the row size and both base addresses
inline int vector_width(const void *s, const void *d, int64_t row_bytes) {
  const uint64_t x = (uint64_t)(uintptr_t)s | (uint64_t)(uintptr_t)d | (uint64_t)row_bytes;
  for (int w = 16; w > 1; w >>= 1)
    if (x % w == 0) return w;
  return 1;
}

// appends the job to the table; false if the grid would pass 2^31 - 1 workgroups
template <int N>
inline bool push_job(RowTable<N> &t, uint64_t &wgs, const char *src, char *dst, const int *pos, int64_t row_bytes,
                     int count, int dst_row0, int src_rows) {
  RowJobDev &J = t.j[t.n];
  J.src = src;
  J.dst = dst;
  J.pos = pos;
  J.width = vector_width(src, dst, row_bytes);
  J.row_elems = row_bytes / J.width;
  J.count = count;
  J.dst_row0 = dst_row0;
  J.src_rows = src_rows;
  J.chunks = (unsigned)((J.row_elems + MOVE_CHUNK - 1) / MOVE_CHUNK);
  J.wg_start = (unsigned)wgs;
  wgs += (uint64_t)J.chunks * (uint64_t)count;
  t.n++;
  return wgs <= (uint64_t)INT32_MAX;
}

}  // namespace dba
