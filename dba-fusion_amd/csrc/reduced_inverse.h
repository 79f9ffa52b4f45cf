// What depth_variance.hip and pose_covariance.hip share: the factorisation of the damped reduced camera system
//   Sd = H + diag(ep + lm diag(H)) = L L^T          (dv_factor_kernel, ONE workgroup)
// and one column of M = Sd^-1 by two substitutions     (dv_solve_column, one WAVE),
// with the layout of the scratch both stages work in:
//   [0, n^2) doubles           L as a full square (L below, L^T above the diagonal): both substitutions read rows
//   [n^2, 2 n^2) doubles       M, row c = the solve of column c (written by dv_inverse_kernel only)
//   then DV_STATUS_BYTES       word 0: 1 when a pivot was not positive (written by every factor launch)
// Everything here sits in an unnamed namespace: each of the two files keeps a factor kernel of its own, launched through
// dv_launch_factor, and the arithmetic -- every fma, every summation order -- is one text.
#pragma once
#include "ba_kernels.h"

namespace dba {
namespace {

constexpr int DV_MAX_P = 64;
constexpr int DV_THREADS = 256;
constexpr int DV_NB = 32;              // columns of a Cholesky panel
constexpr int DV_RESIDENT_MAX = 128;   // unknowns up to which the whole triangle lives in LDS

constexpr size_t DV_STATUS_BYTES = 256;

__host__ __device__ inline int dv_ld(int n) { return n | 1; }   // odd row length of the resident triangle: no bank column
inline size_t dv_scratch_bytes(int n) { return 2 * sizeof(double) * (size_t)n * n + DV_STATUS_BYTES; }
inline size_t dv_factor_lds(int n) {
  const size_t doubles = n <= DV_RESIDENT_MAX ? (size_t)n * dv_ld(n) : (size_t)n * (DV_NB + 1);
  return sizeof(double) * doubles + 16;
}

struct DvScratch {   // the three parts of a scratch of dv_scratch_bytes(n) bytes
  double *Lg, *Mg;
  int *status;
  DvScratch(void *scratch, int n)
      : Lg(static_cast<double *>(scratch)), Mg(Lg + (size_t)n * n), status(reinterpret_cast<int *>(Mg + (size_t)n * n)) {}
};

__device__ __forceinline__ double dv_wave_sum(double s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

__global__ __launch_bounds__(DV_THREADS) void dv_factor_kernel(const double *__restrict__ H, int n, double lm, double ep,
                                                               double *__restrict__ Lg, int *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double dv_sm[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const bool resident = n <= DV_RESIDENT_MAX;
  const int ld = resident ? dv_ld(n) : n;          // row length of the finished factor: in LDS, or in the scratch
  double *Lf = resident ? dv_sm : Lg;
  int *bad = reinterpret_cast<int *>(dv_sm + (resident ? (size_t)n * dv_ld(n) : (size_t)n * (DV_NB + 1)));
  auto damped = [&](int i, int j) {                // j <= i: the lower triangle of H is all that is read
    double v = H[(size_t)i * n + j];
    if (i == j) v += ep + lm * v;
    return v;
  };
  if (tid == 0) *bad = 0;
  if (resident) {
    for (int e = tid; e < n * n; e += nt) {
      const int i = e / n, j = e - i * n;
      if (j <= i) Lf[i * ld + j] = damped(i, j);
    }
  }
  __syncthreads();

  for (int k0 = 0; k0 < n; k0 += DV_NB) {
    const int kb = min(DV_NB, n - k0), rows = n - k0;
    double *Pn = resident ? dv_sm + (size_t)k0 * ld + k0 : dv_sm;   // entry (r, j) of the panel: row k0 + r, column k0 + j
    const int ldp = resident ? ld : DV_NB + 1;
    // the panel minus what the finished columns contribute
    for (int e = tid; e < rows * kb; e += nt) {
      const int r = e / kb, j = e - r * kb;
      if (j > r) continue;
      double a = resident ? Pn[r * ldp + j] : damped(k0 + r, k0 + j);
      const double *x = Lf + (size_t)(k0 + r) * ld, *y = Lf + (size_t)(k0 + j) * ld;
      for (int t = 0; t < k0; t++) a = fma(-x[t], y[t], a);
      Pn[r * ldp + j] = a;
    }
    __syncthreads();
    // its columns, one by one: scale, then take the column out of the ones to its right
    for (int j = 0; j < kb; j++) {
      const double d = Pn[j * ldp + j];
      const bool ok = d > 0.0;                     // (false for a NaN too)
      if (!ok && tid == 0) *bad = 1;
      const double piv = sqrt(ok ? d : 1.0);
      for (int r = j + 1 + tid; r < rows; r += nt) Pn[r * ldp + j] /= piv;
      __syncthreads();                             // every thread has read d
      if (tid == 0) Pn[j * ldp + j] = piv;
      const int nc = kb - 1 - j;
      for (int e = tid; e < (rows - j - 1) * nc; e += nt) {
        const int r = j + 1 + e / nc, c = j + 1 + e % nc;
        if (c <= r) Pn[r * ldp + c] = fma(-Pn[r * ldp + j], Pn[c * ldp + j], Pn[r * ldp + c]);
      }
      __syncthreads();
    }
    if (!resident) {
      for (int e = tid; e < rows * kb; e += nt) {
        const int r = e / kb, j = e - r * kb;
        if (j > r) continue;
        const double v = Pn[r * ldp + j];
        Lg[(size_t)(k0 + r) * n + k0 + j] = v;
        Lg[(size_t)(k0 + j) * n + k0 + r] = v;
      }
      __syncthreads();
    }
  }
  if (resident) {
    for (int e = tid; e < n * n; e += nt) {
      const int i = e / n, j = e - i * n;
      if (j > i) continue;
      const double v = Lf[i * ld + j];
      Lg[(size_t)i * n + j] = v;
      Lg[(size_t)j * n + i] = v;
    }
  }
  if (tid == 0) status[0] = *bad;
}

// Sd^-1 rhs into y[0, n), by ONE wave: L y = rhs forwards (from row c on: the entries of rhs before row c are zero, rhs(i) is
// asked for i >= c only), L^T x = y backwards; the 64 lanes share each row's dot product (lane t & 63 owns y[t]: no lane reads
// what another wrote) and add their parts in a xor butterfly, which leaves the same bits in every lane.  y: n doubles of LDS
// that belong to this wave.  No workgroup barrier.  dv_solve_column: rhs = e_c, column c of M (the stages of this header);
// inertial.hip solves its one right-hand side with c = 0.
// The forward half alone: L y = rhs from row c on.  inertial.hip runs it per column of its marginal system (c = 0).
template <class Rhs>
__device__ __forceinline__ void dv_forward_rhs(const double *__restrict__ Lg, int n, int c, Rhs rhs, double *y, int lane) {
  for (int t = lane; t < n; t += 64) y[t] = 0.0;
  const int tb = c & ~63;
  for (int i = c; i < n; i++) {
    const double *row = Lg + (size_t)i * n;
    double s = 0.0;
    for (int t = tb + lane; t < i; t += 64) s = fma(row[t], y[t], s);
    s = dv_wave_sum(s);
    if ((i & 63) == lane) y[i] = (rhs(i) - s) / row[i];
  }
}
template <class Rhs>
__device__ __forceinline__ void dv_solve_rhs(const double *__restrict__ Lg, int n, int c, Rhs rhs, double *y, int lane) {
  dv_forward_rhs(Lg, n, c, rhs, y, lane);
  for (int i = n - 1; i >= 0; i--) {
    const double *row = Lg + (size_t)i * n;        // above the diagonal: L^T
    double s = 0.0;
    for (int t = i + 1 + ((lane - (i + 1)) & 63); t < n; t += 64) s = fma(row[t], y[t], s);
    s = dv_wave_sum(s);
    if ((i & 63) == lane) y[i] = (y[i] - s) / row[i];
  }
}
__device__ __forceinline__ void dv_solve_column(const double *__restrict__ Lg, int n, int c, double *y, int lane) {
  dv_solve_rhs(Lg, n, c, [c](int i) { return i == c ? 1.0 : 0.0; }, y, lane);
}

// launch 1 of both stages: the factor of the n x n system in the workspace's H into the scratch
inline int dv_launch_factor(const double *H, int n, float lm, float ep, const DvScratch &sc, hipStream_t s) {
  static DeviceOnce once;
  if (once.needed()) {
    DBA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&dv_factor_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)dv_factor_lds(DV_RESIDENT_MAX)));
    once.done();
  }
  hipLaunchKernelGGL(dv_factor_kernel, dim3(1), dim3(DV_THREADS), dv_factor_lds(n), s, H, n, (double)lm, (double)ep, sc.Lg,
                     sc.status);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace
}  // namespace dba
