// The BA cost report (dba_ba_cost, include/dba_hip.h): per edge of a window the weighted reprojection cost the linearisation
// minimises, the sum of its weights, the number of pixels that carry it and the largest squared residual; one more row for the
// window.  The per-pixel chain is the linearisation's own (ba_cost_pixel.h); from (r, w) on everything is float64.
//
// Two launches, no atomics, nothing waits on the host, no BA workspace:
//   1. ba_cost_partial_kernel, grid N x S with S = ceil(HW / 1024) (a function of the map size alone: the bytes do not depend on
//      the device), 256 threads, four pixels per lane (pixel = 1024 s + 256 q + thread: every q is a coalesced segment).  Thread 0
//      forms the edge's relative pose in float64 and rounds it once; every lane adds its pixels into four float64 accumulators;
//      a xor butterfly over the wave (the same bits in every lane), then the four waves' sums in wave order; one entry of four
//      doubles per (edge, slice) into the caller's scratch.
//   2. ba_cost_finish_kernel, ONE workgroup: a thread per edge adds its slices in slice order into row n, keeps a running sum
//      of its edges (n = thread, thread + 256, ...), and a fixed tree over the 256 threads forms row N.
// Every sum therefore has one order: the same bytes from run to run.  A maximum carries a NaN (nan_max), so a NaN residual of a
// used pixel shows in its edge's cost and r2max and in the total's, and in no other row.
// An edge whose ii or jj is not a frame of the buffer is refused per edge: no lane reads through the index, the row is
// (NaN, NaN, -1, NaN), and the total -- the sum of the rows as they are stored -- says so too.
#include "ba_cost_pixel.h"

#include <limits.h>

namespace dba {
namespace {

constexpr int COST_THREADS = 256;
constexpr int COST_PPL = 4;                               // pixels per lane
constexpr int COST_SLICE = COST_THREADS * COST_PPL;       // pixels of a workgroup

inline long long cost_slices(long long HW) { return (HW + COST_SLICE - 1) / COST_SLICE; }

__device__ __forceinline__ double nan_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

struct CostSums {
  double cost, wsum, used, r2max;
};

__device__ __forceinline__ void cost_join(CostSums &a, const CostSums &b) {
  a.cost += b.cost;
  a.wsum += b.wsum;
  a.used += b.used;
  a.r2max = nan_max(a.r2max, b.r2max);
}

__global__ __launch_bounds__(COST_THREADS) void ba_cost_partial_kernel(
    const float *__restrict__ poses, const float *__restrict__ disps, const float *__restrict__ intrinsics,
    const float *__restrict__ targets, const float *__restrict__ weights, const int64_t *__restrict__ ii,
    const int64_t *__restrict__ jj, int B, int HW, int wd, int S, double *__restrict__ scratch) {
  __shared__ float s_pose[12];              // tij[3], R[9]
  __shared__ double s_red[COST_THREADS / 64][4];
  const int n = blockIdx.x / S, s = blockIdx.x - n * S;
  const int64_t i64 = ii[n], j64 = jj[n];
  if (i64 < 0 || i64 >= B || j64 < 0 || j64 >= B) return;   // (the whole workgroup: the finish kernel writes the row)
  const int ix = (int)i64, jx = (int)j64;
  const int tid = threadIdx.x;
  if (tid == 0) {
    float t[3];
    Rot3 R0;
    cost_edge_pose(poses, ix, jx, t, R0);
#pragma unroll
    for (int c = 0; c < 3; c++) s_pose[c] = t[c];
#pragma unroll
    for (int c = 0; c < 9; c++) s_pose[3 + c] = R0.r[c];
  }

  // the loads of all four pixels are in flight before the pose is needed
  const float intr[4] = {intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3]};
  const float *dp = disps + (size_t)ix * HW;
  const float *tp = targets + (size_t)n * 2 * HW, *wp = weights + (size_t)n * 2 * HW;
  bool active[COST_PPL];
  float disp[COST_PPL], tu[COST_PPL], tv[COST_PPL], gu[COST_PPL], gv[COST_PPL];
  int kk[COST_PPL];
#pragma unroll
  for (int q = 0; q < COST_PPL; q++) {
    const long long k = (long long)s * COST_SLICE + q * COST_THREADS + tid;
    active[q] = k < HW;
    kk[q] = active[q] ? (int)k : 0;
    disp[q] = tu[q] = tv[q] = gu[q] = gv[q] = 0.f;
    if (active[q]) {
      disp[q] = dp[kk[q]];
      tu[q] = tp[kk[q]];
      tv[q] = tp[(size_t)HW + kk[q]];
      gu[q] = wp[kk[q]];
      gv[q] = wp[(size_t)HW + kk[q]];
    }
  }
  __syncthreads();
  float tij[3];
  Rot3 R;
#pragma unroll
  for (int c = 0; c < 3; c++) tij[c] = s_pose[c];
#pragma unroll
  for (int c = 0; c < 9; c++) R.r[c] = s_pose[3 + c];

  CostSums a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < COST_PPL; q++) {
    if (!active[q]) continue;
    const int v = kk[q] / wd, u = kk[q] - v * wd;
    PixelResidual p;
    if (!residual_pixel((float)u, (float)v, disp[q], tu[q], tv[q], gu[q], gv[q], intr, tij, R, p)) continue;
    const double wu = p.wu, wv = p.wv, ru = p.ru, rv = p.rv;
    if (!(wu + wv != 0.0)) continue;         // (a NaN weight counts as used and shows in the sums)
    const double ru2 = ru * ru, rv2 = rv * rv;
    a.cost += wu * ru2 + wv * rv2;
    a.wsum += wu + wv;
    a.used += 1.0;
    a.r2max = nan_max(a.r2max, ru2 + rv2);
  }

#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    CostSums o;
    o.cost = __shfl_xor(a.cost, m, 64);
    o.wsum = __shfl_xor(a.wsum, m, 64);
    o.used = __shfl_xor(a.used, m, 64);
    o.r2max = __shfl_xor(a.r2max, m, 64);
    cost_join(a, o);
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
    s_red[wave][0] = a.cost;
    s_red[wave][1] = a.wsum;
    s_red[wave][2] = a.used;
    s_red[wave][3] = a.r2max;
  }
  __syncthreads();
  if (tid == 0) {
    CostSums t = {s_red[0][0], s_red[0][1], s_red[0][2], s_red[0][3]};
#pragma unroll
    for (int w = 1; w < COST_THREADS / 64; w++) {
      const CostSums o = {s_red[w][0], s_red[w][1], s_red[w][2], s_red[w][3]};
      cost_join(t, o);
    }
    double2 *dst = reinterpret_cast<double2 *>(scratch + 4 * (size_t)blockIdx.x);
    dst[0] = make_double2(t.cost, t.wsum);
    dst[1] = make_double2(t.used, t.r2max);
  }
}

__global__ __launch_bounds__(COST_THREADS) void ba_cost_finish_kernel(const double *__restrict__ scratch,
                                                                      const int64_t *__restrict__ ii,
                                                                      const int64_t *__restrict__ jj, int N, int B, int S,
                                                                      double *__restrict__ out) {
  __shared__ double s_tree[COST_THREADS][4];
  const int tid = threadIdx.x;
  CostSums mine = {0.0, 0.0, 0.0, 0.0};
  for (int n = tid; n < N; n += COST_THREADS) {
    const int64_t i64 = ii[n], j64 = jj[n];
    CostSums row;
    if (i64 < 0 || i64 >= B || j64 < 0 || j64 >= B) {
      const double nan = __builtin_nan("");
      row = {nan, nan, -1.0, nan};
    } else {
      const double2 *src = reinterpret_cast<const double2 *>(scratch + 4 * (size_t)n * S);
      row = {0.0, 0.0, 0.0, 0.0};
      for (int s = 0; s < S; s++) {
        const double2 lo = src[2 * s], hi = src[2 * s + 1];
        const CostSums o = {lo.x, lo.y, hi.x, hi.y};
        cost_join(row, o);
      }
    }
    double *dst = out + 4 * (size_t)n;
    dst[0] = row.cost;
    dst[1] = row.wsum;
    dst[2] = row.used;
    dst[3] = row.r2max;
    cost_join(mine, row);
  }
  s_tree[tid][0] = mine.cost;
  s_tree[tid][1] = mine.wsum;
  s_tree[tid][2] = mine.used;
  s_tree[tid][3] = mine.r2max;
  __syncthreads();
  for (int half = COST_THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
      CostSums x = {s_tree[tid][0], s_tree[tid][1], s_tree[tid][2], s_tree[tid][3]};
      const CostSums y = {s_tree[tid + half][0], s_tree[tid + half][1], s_tree[tid + half][2], s_tree[tid + half][3]};
      cost_join(x, y);
      s_tree[tid][0] = x.cost;
      s_tree[tid][1] = x.wsum;
      s_tree[tid][2] = x.used;
      s_tree[tid][3] = x.r2max;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double *dst = out + 4 * (size_t)N;
#pragma unroll
    for (int c = 0; c < 4; c++) dst[c] = s_tree[0][c];
  }
}

inline bool misaligned(const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace
}  // namespace dba

using namespace dba;

extern "C" {

size_t dba_ba_cost_scratch_bytes(int N, int ht, int wd) {
  if (N < 0 || ht < 1 || wd < 1) return 0;
  const long long S = cost_slices((long long)ht * wd);
  return (size_t)N * (size_t)S * 4 * sizeof(double);
}

int dba_ba_cost(const float *poses, const float *disps, const float *intrinsics4, const float *targets, const float *weights,
                const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, double *out, int out_rows, void *scratch,
                size_t scratch_bytes, dba_stream_t stream) {
  // every refusal comes before the first runtime call
  if (N < 0 || B < 1 || ht < 1 || wd < 1 || out_rows < 0 || out_rows - 1 < N) return DBA_ERR_ARG;
  if (!out || misaligned(out, sizeof(double))) return DBA_ERR_ARG;
  const long long HW = (long long)ht * wd, S = cost_slices(HW);
  if (N > 0) {
    if (!poses || !disps || !intrinsics4 || !targets || !weights || !ii || !jj || !scratch) return DBA_ERR_ARG;
    if (misaligned(poses, sizeof(float)) || misaligned(disps, sizeof(float)) || misaligned(intrinsics4, sizeof(float)) ||
        misaligned(targets, sizeof(float)) || misaligned(weights, sizeof(float)) || misaligned(ii, sizeof(int64_t)) ||
        misaligned(jj, sizeof(int64_t)) || misaligned(scratch, 2 * sizeof(double)))
      return DBA_ERR_ARG;
    if (HW > INT_MAX || (long long)N * S > INT_MAX) return DBA_ERR_UNSUPPORTED;
    if (scratch_bytes < (size_t)N * (size_t)S * 4 * sizeof(double)) return DBA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N > 0) {
    hipLaunchKernelGGL(ba_cost_partial_kernel, dim3((unsigned)(N * S)), dim3(COST_THREADS), 0, st, poses, disps, intrinsics4,
                       targets, weights, ii, jj, B, (int)HW, wd, (int)S, static_cast<double *>(scratch));
    DBA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ba_cost_finish_kernel, dim3(1), dim3(COST_THREADS), 0, st, static_cast<const double *>(scratch), ii, jj, N, B,
                     (int)S, out);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
