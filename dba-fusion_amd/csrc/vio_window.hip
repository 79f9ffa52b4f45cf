// The window split of DepthVideo.ba's IMU branch (dbaf/depth_video.py:360-367, :388-390, :470-475), gfx950, two launches:
//   plan     one workgroup of 1024 lanes, no atomics.  Two selections, each compacted in list order (flag_slot,
//            edge_lists.h), tiled over lists longer than the workgroup:
//              marginalised  over the OLD window's lists (cur_ii, cur_jj):  last_t0 <= ii < lo  &&  ii < last_t1 - 2  &&
//                            jj < last_t1 - 2                                                         (:360-364)
//              active        over the call's lists (ii, jj):                ii >= t0 && jj >= t0      (:470)
//            It writes the compacted ii / jj of both (:366-367, :471-472), the selected positions as int32 row lists
//            for the payload launch, and one result block: n_marg, max(marg_jj) (:372), n_active, min(ii) (:475).
//            The entries of an output list behind its count are the input's own entries at those positions, so that
//            a list cut at a remembered count never holds anything the caller did not pass in.
//   payload  the row mover's grid (row_jobs.h) over up to four gathers: marg_target, marg_weight (:388-389),
//            cur_target, cur_weight (:473-474).  It compares the result block of THIS call's plan with the four words
//            the outputs were sized for; on a mismatch every job's rows are zeroed (the table runs with FILL and no
//            source) -- zero weights leave BACore's system empty -- and a pinned host word is raised.
// Integers and bytes only: every result is exact.  No atomics, no inter-workgroup communication, nothing synchronises
// the host.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "edge_lists.h"
#include "row_jobs.h"
#include "size_guard.h"

namespace dba {

constexpr int VW_THREADS = 1024;
constexpr int VW_WAVES = VW_THREADS / WAVE;
constexpr int VW_INDEX_CLAMP = 1 << 30;

__device__ __forceinline__ int vw_clamp_index(int64_t v) {
  return (int)(v > VW_INDEX_CLAMP ? VW_INDEX_CLAMP : (v < -VW_INDEX_CLAMP ? -VW_INDEX_CLAMP : v));
}

template <bool IS_MIN>
__device__ __forceinline__ int vw_block_minmax(int x, int *sh) {
  x = wave_minmax<IS_MIN>(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  int r = sh[0];
#pragma unroll
  for (int w = 1; w < VW_WAVES; w++) r = IS_MIN ? min(r, sh[w]) : max(r, sh[w]);
  __syncthreads();
  return r;
}

// One selection: the entries p of (a, b)[0, n) with keep(a[p], b[p]), compacted in list order into out_a / out_b / pos
// (capacity n each).  Returns the count; *hi_b is the lane's running max of the selected b, *lo_a the lane's running min
// of every a.  All lanes call it.
template <typename Keep>
__device__ __forceinline__ int vw_select(const int64_t *__restrict__ a, const int64_t *__restrict__ b, int n, Keep keep,
                                         int64_t *__restrict__ out_a, int64_t *__restrict__ out_b, int *__restrict__ pos,
                                         int *wcount, int *hi_b, int *lo_a) {
  const int tid = threadIdx.x;
  int kept = 0;  // in the tiles before this one
  for (int start = 0; start < n; start += VW_THREADS) {
    const int p = start + tid;
    int64_t i = 0, j = 0;
    bool k = false;
    if (p < n) {
      i = a[p];
      j = b[p];
      k = keep(i, j);
      *lo_a = min(*lo_a, vw_clamp_index(i));
    }
    int total;
    const int q = kept + flag_slot<VW_THREADS>(k, wcount, &total);
    if (k) {
      out_a[q] = i;
      out_b[q] = j;
      pos[q] = p;
      *hi_b = max(*hi_b, vw_clamp_index(j));
    }
    kept += total;
  }
  // behind the count: the input's own entries (a selected entry's slot is never behind its position, so a slot >= kept
  // is written here alone)
  for (int p = kept + tid; p < n; p += VW_THREADS) {
    out_a[p] = a[p];
    out_b[p] = b[p];
    pos[p] = -1;  // the row mover copies nothing for it
  }
  return kept;
}

// Capacities (the host allocates them): marg_ii, marg_jj, marg_pos [n_cur]; act_ii, act_jj, act_pos [n]; res
// [DBA_VW_RES_WORDS].  n_cur == 0: the marginalisation branch is not entered.
__global__ __launch_bounds__(VW_THREADS) void vio_window_plan_kernel(
    const int64_t *__restrict__ cur_ii, const int64_t *__restrict__ cur_jj, int n_cur, int64_t last_t0, int64_t lo,
    int64_t last_t1, const int64_t *__restrict__ ii, const int64_t *__restrict__ jj, int n, int64_t t0,
    int64_t *__restrict__ marg_ii, int64_t *__restrict__ marg_jj, int *__restrict__ marg_pos,
    int64_t *__restrict__ act_ii, int64_t *__restrict__ act_jj, int *__restrict__ act_pos, int *__restrict__ res) {
  __shared__ int wcount[VW_WAVES];
  __shared__ int red[VW_WAVES];
  int hi_mj = -VW_INDEX_CLAMP, lo_i = VW_INDEX_CLAMP, unused_lo = VW_INDEX_CLAMP, unused_hi = -VW_INDEX_CLAMP;
  // :360-367
  const int64_t newest = last_t1 - 2;
  const int n_marg = vw_select(
      cur_ii, cur_jj, n_cur, [=](int64_t i, int64_t j) { return i >= last_t0 && i < lo && i < newest && j < newest; },
      marg_ii, marg_jj, marg_pos, wcount, &hi_mj, &unused_lo);
  // :470-472, and ii.min() of :475 over the whole list
  const int n_active = vw_select(
      ii, jj, n, [=](int64_t i, int64_t j) { return i >= t0 && j >= t0; }, act_ii, act_jj, act_pos, wcount, &unused_hi,
      &lo_i);
  hi_mj = vw_block_minmax<false>(hi_mj, red);
  lo_i = vw_block_minmax<true>(lo_i, red);
  if (threadIdx.x == 0) {
    res[0] = n_marg;
    res[1] = hi_mj;  // -2^30 when nothing is selected
    res[2] = n_active;
    res[3] = lo_i;
  }
}

struct VwGuard {
  const int *res;
  int *status;  // pinned host words
  int exp[4];   // what the outputs were sized for: n_marg, max(marg_jj), n_active, min(ii)
  unsigned wgs;  // workgroups of the table
};

__global__ __launch_bounds__(MOVE_THREADS) void vio_window_payload_kernel(RowTable<DBA_VW_MAX_JOBS> t, VwGuard g) {
  const int r0 = g.res[0], r1 = g.res[1], r2 = g.res[2], r3 = g.res[3];
  const bool ok = r0 == g.exp[0] && r1 == g.exp[1] && r2 == g.exp[2] && r3 == g.exp[3];
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) guard_report<4>(g.status, {r0, r1, r2, r3}, g.exp);
  if (blockIdx.x >= g.wgs) return;  // (a call that moves no row still runs the comparison, in one workgroup)
  RowTable<DBA_VW_MAX_JOBS> u = t;
#pragma unroll
  for (int q = 0; q < DBA_VW_MAX_JOBS; q++) u.j[q].src = ok ? t.j[q].src : nullptr;  // the guard: the rows are zeroed
  run_row_jobs<DBA_VW_MAX_JOBS, true>(u);
}

// a mismatch is reported through its words (size_guard.h): [1..4] the plan's result block, [5..8] the words the outputs
// were sized for
static SizeGuard vw_guard;

}  // namespace dba

using namespace dba;

extern "C" {

int dba_vio_window_plan(const int64_t *cur_ii, const int64_t *cur_jj, int n_cur, int64_t last_t0, int64_t lo,
                        int64_t last_t1, const int64_t *ii, const int64_t *jj, int n, int64_t t0, int64_t *marg_ii,
                        int64_t *marg_jj, int *marg_pos, int64_t *act_ii, int64_t *act_jj, int *act_pos, int *res,
                        dba_stream_t stream) {
  if (n_cur < 0 || n <= 0 || !ii || !jj || !act_ii || !act_jj || !act_pos || !res) return DBA_ERR_ARG;
  if (n_cur > 0 && (!cur_ii || !cur_jj || !marg_ii || !marg_jj || !marg_pos)) return DBA_ERR_ARG;
  if (n_cur > DBA_SEL_MAX_EDGES || n > DBA_SEL_MAX_EDGES) return DBA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(vio_window_plan_kernel, dim3(1), dim3(VW_THREADS), 0, (hipStream_t)stream, cur_ii, cur_jj, n_cur,
                     last_t0, lo, last_t1, ii, jj, n, t0, marg_ii, marg_jj, marg_pos, act_ii, act_jj, act_pos, res);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_vio_window_payload(const dba_row_job *jobs, int n_jobs, const int *res, const int *expect4, dba_stream_t stream) {
  if (n_jobs < 0 || n_jobs > DBA_VW_MAX_JOBS || (n_jobs > 0 && !jobs) || !res || !expect4) return DBA_ERR_ARG;
  RowTable<DBA_VW_MAX_JOBS> t{};
  uint64_t wgs = 0;
  for (int k = 0; k < n_jobs; k++) {
    const dba_row_job &j = jobs[k];
    const int live = check_row_job(j, true, POS_REQUIRED);
    if (live < 0) return live;
    if (!live) continue;
    if (!push_job(t, wgs, (const char *)j.src, (char *)j.dst, j.pos, j.row_bytes, j.count, j.dst_row0, j.src_rows))
      return DBA_ERR_UNSUPPORTED;
  }
  VwGuard g{};
  if (const int rc = vw_guard.words(&g.status)) return rc;
  g.res = res;
  for (int k = 0; k < 4; k++) g.exp[k] = expect4[k];
  g.wgs = (unsigned)wgs;
  hipLaunchKernelGGL(vio_window_payload_kernel, dim3(wgs ? (unsigned)wgs : 1u), dim3(MOVE_THREADS), 0,
                     (hipStream_t)stream, t, g);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_vio_window_poll(int *words8) { return vw_guard.poll(words8, 8); }

}  // extern "C"
