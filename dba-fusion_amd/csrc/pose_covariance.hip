// 6 x 6 covariances of the poses of a BA window (dba_ba_pose_covariance, include/dba_hip.h): a stage on the workspace as stages
// 1 and 2 leave it -- the reduced camera system H (float64, LOWER triangle) -- that changes nothing in it.
//
//   Sd = H + diag(ep + lm diag(H)),   M = Sd^-1      as in depth_variance.hip: the same factor kernel, the same column solve
//   marginal job (b):     S_bb = M[6p:6p+6, 6p:6p+6], p = b - t0: the covariance of pose b's tangent given the gauge (the fixed
//                         poses outside [t0, t1)), the depths marginalised out, under the damping of the step.
//                         With a frame map Ainv (6 x 6):  S_g = Ainv S_bb Ainv^T.
//   relative job (a, b):  S_rel = S_bb + Ad S_aa Ad^T - Ad S_ab - S_ba Ad^T = J S J^T,  J = [-Ad | I],  S = [[S_aa, S_ab], [S_ba, S_bb]],
//                         Ad = Ad(G), G = T_b T_a^-1: the first-order covariance of xi_rel in G' = Exp(xi_rel) G, xi_rel = xi_b - Ad xi_a.
//                         Always in camera tangents.  A frame outside [t0, t1) is a fixed pose: its blocks of S are zero.
// Tangents are (tau, phi), perturbations act on the left (T' = Exp(xi) T, T world -> camera), so for G = (R, t)
//   Ad(G) = [[R, [t]x R], [0, R]],   R = R_b R_a^T,  t = t_b - R t_a,
// formed in float64 from the poses (t, q_xyzw float32, q normalised in float64) as they are stored when the kernel runs.
//
// Two launches:
//   1. dv_factor_kernel (reduced_inverse.h), exactly as in dba_ba_depth_variance.
//   2. pc_jobs_kernel, one workgroup per job; the job lists travel in the kernel's argument block (no copy, no host
//      synchronisation, recordable).  Wave w of a group of six solves column 6 p + w of M with dv_solve_column -- the arithmetic
//      and the summation order of dv_inverse_kernel, so the entries are the bits that kernel writes.  A marginal job has one
//      group (six waves); a launch with relative jobs has two (twelve waves: the columns of a and of b side by side -- the
//      kernel is bound by the latency of one column's 2 n dependent rows, so a second pass would double a job's time).
//      S is then read from the waves' columns in LDS: entry (i, j), i >= j, is wave i's solve at row j (the LOWER triangle of M
//      as dv_inverse_kernel stores it), mirrored; J S J^T is summed by 21 threads, one per entry of the lower triangle, in one
//      fixed order, and mirrored: every block is symmetric to the bit.
// All arithmetic is float64, there are no atomics.  A pivot that is not positive (the status word) makes every block NaN.
#include "reduced_inverse.h"

namespace dba {
namespace {

constexpr int PC_MAX_JOBS = 64;
constexpr int PC_GROUP = 6 * 64;       // threads that solve one pose's six columns

struct PcJobs {                        // the kernel's job table: frame indices, validated by the host
  int n_marg, n_pairs, mapped, pad;
  int marg[PC_MAX_JOBS];
  int pa[PC_MAX_JOBS], pb[PC_MAX_JOBS];
  double Ainv[36];
};
static_assert(sizeof(PcJobs) <= 2048, "the job table travels as a kernel argument");

inline size_t pc_lds(int n, int groups) { return sizeof(double) * ((size_t)6 * groups * n + 144 + 72); }

// R (row-major) of a stored pose's quaternion, normalised in float64
__device__ inline void pc_rotation(const float *__restrict__ p, double (&R)[9]) {
  double x = p[3], y = p[4], z = p[5], w = p[6];
  const double s = 1.0 / sqrt(x * x + y * y + z * z + w * w);
  x *= s, y *= s, z *= s, w *= s;
  R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - w * z), R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y), R[7] = 2 * (y * z + w * x), R[8] = 1 - 2 * (x * x + y * y);
}

// J [6][12] = [-Ad(T_b T_a^-1) | I]
__device__ inline void pc_relative_map(const float *__restrict__ Ta, const float *__restrict__ Tb, double *J) {
  double Ra[9], Rb[9], R[9], t[3];
  pc_rotation(Ta, Ra);
  pc_rotation(Tb, Rb);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
  for (int i = 0; i < 3; i++)
    t[i] = (double)Tb[i] - (R[3 * i] * (double)Ta[0] + R[3 * i + 1] * (double)Ta[1] + R[3 * i + 2] * (double)Ta[2]);
  const double tx[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double txR = tx[3 * i] * R[j] + tx[3 * i + 1] * R[3 + j] + tx[3 * i + 2] * R[6 + j];
      J[12 * i + j] = -R[3 * i + j];
      J[12 * i + 3 + j] = -txR;
      J[12 * (3 + i) + j] = 0.0;
      J[12 * (3 + i) + 3 + j] = -R[3 * i + j];
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) J[12 * i + 6 + j] = i == j ? 1.0 : 0.0;
}

__global__ __launch_bounds__(2 * PC_GROUP) void pc_jobs_kernel(const double *__restrict__ Lg, const int *__restrict__ status, int n,
                                                               int t0, int P, const float *__restrict__ poses, PcJobs jobs,
                                                               double *__restrict__ out_marg, double *__restrict__ out_pairs) {
  extern __shared__ __attribute__((aligned(16))) double dv_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, groups = blockDim.x / PC_GROUP;
  double *S = dv_sm + (size_t)6 * groups * n;      // [12][12]
  double *J = S + 144;                             // [6][12]
  const int job = blockIdx.x;
  const bool rel = job >= jobs.n_marg;
  // group 0 solves the columns of fr[0], group 1 those of fr[1]; a marginal job has fr[0] alone
  int fr[2];
  double *out;
  if (!rel) {
    fr[0] = jobs.marg[job], fr[1] = -1;
    out = out_marg + (size_t)36 * job;
  } else {
    fr[0] = jobs.pa[job - jobs.n_marg], fr[1] = jobs.pb[job - jobs.n_marg];
    out = out_pairs + (size_t)36 * (job - jobs.n_marg);
  }
  if (rel && groups < 2) return;                   // (the host launches two groups whenever there is a pair)
  if (status[0]) {                                 // a pivot was not positive: the inverse does not exist
    if (tid < 36) out[tid] = __builtin_nan("");
    return;
  }
  int win[2];                                      // the pose's place in the window, or -1: a fixed pose
  for (int g = 0; g < 2; g++) win[g] = (fr[g] >= t0 && fr[g] - t0 < P) ? fr[g] - t0 : -1;

  const int g = wave / 6;
  if (g < 2 && win[g] >= 0) dv_solve_column(Lg, n, 6 * win[g] + wave % 6, dv_sm + (size_t)wave * n, lane);
  const bool mapped = rel || jobs.mapped;
  if (tid == blockDim.x - 1 && mapped) {
    if (rel) {
      pc_relative_map(poses + (size_t)7 * fr[0], poses + (size_t)7 * fr[1], J);
    } else {
      for (int e = 0; e < 72; e++) J[e] = (e % 12) < 6 ? jobs.Ainv[6 * (e / 12) + e % 12] : 0.0;
    }
  }
  __syncthreads();
  if (tid < 144) {
    const int i = tid / 12, j = tid % 12, hi = max(i, j), lo = min(i, j);
    const int gh = hi / 6, gl = lo / 6;
    double v = 0.0;
    if (gh < groups && win[gh] >= 0 && win[gl] >= 0) v = dv_sm[(size_t)hi * n + 6 * win[gl] + lo % 6];
    S[tid] = v;
  }
  __syncthreads();
  if (tid < 36) {
    const int r = tid / 6, k = tid % 6, hi = max(r, k), lo = min(r, k);
    double acc;
    if (!mapped) {
      acc = S[12 * hi + lo];
    } else {
      acc = 0.0;
      for (int i = 0; i < 12; i++) {
        double row = 0.0;
        for (int j = 0; j < 12; j++) row = fma(S[12 * i + j], J[12 * lo + j], row);
        acc = fma(J[12 * hi + i], row, acc);
      }
    }
    out[tid] = acc;                                // (entry (r, k) and entry (k, r) are the same sum: the mirror)
  }
}

}  // namespace
}  // namespace dba

using namespace dba;

extern "C" {

int dba_ba_pose_covariance(const float *poses, int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, const int *marg,
                           int n_marg, const int *pairs, int n_pairs, const double *Ainv, double *out_marg, int out_marg_rows,
                           double *out_pairs, int out_pair_rows, void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes,
                           dba_stream_t stream) {
  // every refusal comes before the first runtime call: a launch sized by arguments that do not describe the buffers is
  // how an entry gets to write beyond them
  if (!scratch || !ws) return DBA_ERR_ARG;
  if (n_marg < 0 || n_pairs < 0 || n_marg + n_pairs < 1) return DBA_ERR_ARG;
  if (n_marg > PC_MAX_JOBS || n_pairs > PC_MAX_JOBS) return DBA_ERR_ARG;
  if (n_marg && (!marg || !out_marg || out_marg_rows < n_marg)) return DBA_ERR_ARG;
  if (n_pairs && (!pairs || !out_pairs || !poses || out_pair_rows < n_pairs)) return DBA_ERR_ARG;
  DBA_PLAN_OR_RETURN(plan);
  if (plan.P < 1) return DBA_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(scratch) % sizeof(double) || reinterpret_cast<uintptr_t>(out_marg) % sizeof(double) ||
      reinterpret_cast<uintptr_t>(out_pairs) % sizeof(double) || reinterpret_cast<uintptr_t>(poses) % sizeof(float))
    return DBA_ERR_ARG;
  PcJobs jobs = {};
  jobs.n_marg = n_marg, jobs.n_pairs = n_pairs, jobs.mapped = Ainv ? 1 : 0;
  for (int k = 0; k < n_marg; k++) {
    if (marg[k] < 0 || marg[k] >= B || marg[k] < t0 || marg[k] >= t1) return DBA_ERR_ARG;
    jobs.marg[k] = marg[k];
  }
  for (int k = 0; k < n_pairs; k++) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || a >= B || b < 0 || b >= B || a == b) return DBA_ERR_ARG;
    jobs.pa[k] = a, jobs.pb[k] = b;
  }
  for (int e = 0; e < 36 && Ainv; e++) jobs.Ainv[e] = Ainv[e];
  if (plan.P > DV_MAX_P) return DBA_ERR_UNSUPPORTED;
  const int n = 6 * plan.P;
  if (scratch_bytes < dv_scratch_bytes(n)) return DBA_ERR_WORKSPACE;

  const DvScratch sc(scratch, n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rc = dv_launch_factor(plan.W.H, n, lm, ep, sc, s)) return rc;
  const int groups = n_pairs ? 2 : 1;
  hipLaunchKernelGGL(pc_jobs_kernel, dim3(n_marg + n_pairs), dim3(groups * PC_GROUP), pc_lds(n, groups), s, sc.Lg, sc.status, n, t0,
                     plan.P, poses, jobs, out_marg, out_pairs);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
