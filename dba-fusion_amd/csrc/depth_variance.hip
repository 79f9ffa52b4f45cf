// Marginal variances of the inverse depths of a BA window (dba_ba_depth_variance, include/dba_hip.h): a stage on the workspace
// as stages 1 and 2 leave it -- the coupling rows E, Q = 1 / C (float32) and the reduced camera system H (float64, LOWER
// triangle) -- that changes nothing in it.
//
//   Sd = H + diag(ep + lm diag(H))                 the matrix the solvers factorise (they add the damping while loading)
//   M  = Sd^-1
//   var[f, k] = Q[m, k] + Q[m, k]^2  sum over rows r, s of frame f = kx[m]  of  E[r, :, k]^T M[tgt_r, tgt_s] E[s, :, k]
//
// the k-th diagonal entry of the depth block of the inverse of [[Sd + E Q E^T, E], [E^T, C]].  The rows of a frame are its own
// pose row (f inside the window) and the rows P + n of its out-edges whose target pose lies inside the window: read from the
// tables of stage 0 (kx, eoff, einfo), so the call needs no edge list.  All arithmetic is float64, nothing is accumulated with
// atomics (every sum has one fixed order: the same bits from run to run), nothing waits on the host.
//
// AFTER A SOLVE?  Yes.  Every solver of stage 3 (ba_solve*.hip, ba_solve_general.inc) takes H as `const double *`, adds the
// damping to the diagonal while it loads a copy into LDS / registers / its own scratch and never writes H back; they write dx
// and meta only.  E and Q are written by the linearisation alone.  So the stage gives the same result before and after
// dba_ba_solve, dba_ba_update and BACore.retract, until the next linearisation on the workspace.  It leaves meta[1] alone.
//
// Three launches (the first and the column solve of the second live in reduced_inverse.h, which pose_covariance.hip shares):
//   1. dv_factor_kernel, ONE workgroup: Sd = L L^T, left-looking by panels of DV_NB columns.  n <= DV_RESIDENT_MAX: the
//      triangle stays in LDS for the whole factorisation.  Beyond: one panel [n - k0][DV_NB] in LDS at a time, the finished
//      panels are read back from the scratch (L2).  L leaves as a full square (L below, L^T above the diagonal), so that both
//      substitutions of launch 2 read rows.  A pivot that is not positive raises a word in the scratch; nothing else.
//   2. dv_inverse_kernel, one WAVE per column c of M: L y = e_c forwards (from row c on), L^T x = y backwards, the 64 lanes
//      share each row's dot product (lane t & 63 owns y[t]: no lane reads what another wrote) and add their parts in a xor
//      butterfly, which leaves the same bits in every lane.  Row c of M = the column (M is symmetric).
//   3. dv_quadform_kernel, grid (tiles of 64 pixels, slots of kx), four waves: the frame's rows of E for the tile are read
//      once into LDS (up to DV_RCAP rows; a frame with more rows reads E from memory as it goes), the 6 x 6 blocks of M come in
//      tiles of DV_RT x DV_RT row pairs, the waves share a tile's pairs (r <= s; an off-diagonal pair counts twice) and their
//      four partial sums are added in wave order.  One float store per pixel into var_out[kx[m]].
// The general solver (ba_solve_general.inc) is not reused: it keeps a packed triangle with the right-hand side as an extra row,
// in LDS or in the workspace's own scratch, and hands out dx -- the inverse needs L itself, as rows AND as columns.
#include "reduced_inverse.h"   // the factor kernel, one column of the inverse, the scratch: shared with pose_covariance.hip

namespace dba {
namespace {

constexpr int DV_TP = 64;              // pixels of a quadratic-form workgroup: one per lane
constexpr int DV_RT = 8;               // rows of a tile of staged blocks of M
constexpr int DV_RCAP = 24;            // rows of E a workgroup stages in LDS
constexpr int DV_RLIST = 1024;         // rows of one frame at the most (its own + N out-edges)

constexpr size_t DV_QUAD_LDS = sizeof(double) * (DV_RT * DV_RT * 36 + 4 * DV_TP) + sizeof(float) * DV_RCAP * 6 * DV_TP +
                               sizeof(int) * DV_RLIST + 16;
static_assert(DV_QUAD_LDS <= 64 * 1024, "the quadratic form stays inside the default dynamic LDS limit");

__global__ __launch_bounds__(DV_THREADS) void dv_inverse_kernel(const double *__restrict__ Lg, int n,
                                                                double *__restrict__ Mg, const int *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double dv_sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * (DV_THREADS / 64) + wave;
  if (c >= n || status[0]) return;                 // (no workgroup barrier below)
  double *y = dv_sm + (size_t)wave * n;            // lane t & 63 owns y[t]
  dv_solve_column(Lg, n, c, y, lane);
  for (int t = lane; t < n; t += 64) Mg[(size_t)c * n + t] = y[t];
}

__global__ __launch_bounds__(DV_THREADS) void dv_quadform_kernel(const double *__restrict__ Mg, const int *__restrict__ status,
                                                                 int n, int HW, int t0, int P, int N,
                                                                 float *__restrict__ var_out, int out_rows, BaTables T,
                                                                 BaBuffers W) {
  extern __shared__ __attribute__((aligned(16))) double dv_sm[];
  double *sM = dv_sm;                                        // [DV_RT * DV_RT][36]
  double *sred = sM + DV_RT * DV_RT * 36;                    // [4][DV_TP]
  float *sE = reinterpret_cast<float *>(sred + 4 * DV_TP);   // [DV_RCAP][6][DV_TP]
  unsigned *slist = reinterpret_cast<unsigned *>(sE + DV_RCAP * 6 * DV_TP);   // [DV_RLIST]  row of E | pose << 24
  int *sR = reinterpret_cast<int *>(slist + DV_RLIST);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.y;
  if (m >= T.meta[0]) return;
  const int f = T.kx[m];
  if (f < 0 || f >= out_rows) return;
  const int k = blockIdx.x * DV_TP + lane;
  const bool live = k < HW;

  if (wave == 0) {   // the rows of E that count for this frame: its own pose row, its out-edges with a target inside the window
    int cnt = 0;
    const int pp = f - t0;
    if (pp >= 0 && pp < P) {
      if (lane == 0) slist[0] = (unsigned)pp | ((unsigned)pp << 24);
      cnt = 1;
    }
    const int e0 = max(T.eoff[m], 0), e1 = min(T.eoff[m + 1], N);   // (tables nobody prepared must not steer a read)
    for (int base = e0; base < e1; base += 64) {
      const int pos = base + lane;
      int edge = 0, tg = -1;
      if (pos < e1) edge = T.einfo[2 * pos], tg = T.einfo[2 * pos + 1] - t0;
      const bool ok = tg >= 0 && tg < P && edge >= 0 && edge < N;
      const unsigned long long mask = __ballot(ok);
      const int at = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (ok && at < DV_RLIST) slist[at] = (unsigned)(P + edge) | ((unsigned)tg << 24);
      cnt += __popcll(mask);
    }
    if (lane == 0) *sR = min(cnt, DV_RLIST);
  }
  __syncthreads();
  const int R = *sR;
  const bool staged = R <= DV_RCAP;
  if (staged) {
    for (int e = tid; e < R * 6 * DV_TP; e += DV_THREADS) {
      const int rc = e >> 6, l = e & 63, kk = blockIdx.x * DV_TP + l;
      const int r = rc / 6, c = rc - 6 * r;
      const size_t row = slist[r] & 0xffffffu;
      sE[e] = kk < HW ? W.E[(row * 6 + c) * HW + kk] : 0.f;
    }
  }
  auto coupling = [&](int r, double (&e)[6]) {
    if (staged) {
#pragma unroll
      for (int c = 0; c < 6; c++) e[c] = (double)sE[((r * 6 + c) << 6) + lane];
    } else {
      const size_t row = slist[r] & 0xffffffu;
#pragma unroll
      for (int c = 0; c < 6; c++) e[c] = (double)W.E[(row * 6 + c) * HW + k];
    }
  };

  double acc = 0.0;
  for (int r0 = 0; r0 < R; r0 += DV_RT) {
    for (int s0 = r0; s0 < R; s0 += DV_RT) {
      const int nr = min(DV_RT, R - r0), ns = min(DV_RT, R - s0);
      __syncthreads();   // (the first time: sE is complete; later: the tile before has been read)
      for (int e = tid; e < nr * ns * 36; e += DV_THREADS) {
        const int blk = e / 36, ab = e - 36 * blk;
        const int dr = blk / ns, ds = blk - dr * ns, a = ab / 6, b = ab - 6 * a;
        const int tr = slist[r0 + dr] >> 24, ts = slist[s0 + ds] >> 24;
        sM[e] = Mg[(size_t)(6 * tr + a) * n + 6 * ts + b];
      }
      __syncthreads();
      if (!live) continue;
      for (int blk = wave; blk < nr * ns; blk += DV_THREADS / 64) {
        const int dr = blk / ns, ds = blk - dr * ns;
        const int r = r0 + dr, s = s0 + ds;
        if (s < r) continue;
        double er[6], es[6];
        coupling(r, er);
        coupling(s, es);
        const double *Mb = sM + blk * 36;
        double q = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          double t = 0.0;
#pragma unroll
          for (int b = 0; b < 6; b++) t = fma(Mb[a * 6 + b], es[b], t);
          q = fma(er[a], t, q);
        }
        acc += (s == r) ? q : 2.0 * q;
      }
    }
  }
  sred[wave * DV_TP + lane] = acc;
  __syncthreads();
  if (wave == 0 && live) {
    const double q = ((sred[lane] + sred[DV_TP + lane]) + sred[2 * DV_TP + lane]) + sred[3 * DV_TP + lane];
    const double Qv = (double)W.Q[(size_t)m * HW + k];
    double var = fma(Qv * Qv, q, Qv);
    if (status[0]) var = __builtin_nan("");   // a pivot was not positive: the inverse does not exist
    var_out[(size_t)f * HW + k] = (float)var;
  }
}

}  // namespace
}  // namespace dba

using namespace dba;

extern "C" {

size_t dba_ba_depth_variance_scratch_bytes(int P) {
  if (P < 1 || P > DV_MAX_P) return 0;
  return dv_scratch_bytes(6 * P);
}

int dba_ba_depth_variance_parts(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, float *var_out, int out_rows,
                                void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes, dba_stream_t stream, int parts) {
  // every refusal comes before the first runtime call: a launch sized by arguments that do not describe the buffers is
  // how an entry gets to write beyond them
  if (!var_out || !scratch || !ws) return DBA_ERR_ARG;
  DBA_PLAN_OR_RETURN(plan);
  if (plan.P < 1 || out_rows < B || parts < 1 || parts > 3) return DBA_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(scratch) % sizeof(double) || reinterpret_cast<uintptr_t>(var_out) % sizeof(float))
    return DBA_ERR_ARG;
  if (plan.P > DV_MAX_P || N + 1 > DV_RLIST) return DBA_ERR_UNSUPPORTED;
  const int n = 6 * plan.P;
  if (scratch_bytes < dv_scratch_bytes(n)) return DBA_ERR_WORKSPACE;

  const DvScratch sc(scratch, n);
  double *Lg = sc.Lg, *Mg = sc.Mg;
  int *status = sc.status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (parts & 1) {
    if (const int rc = dv_launch_factor(plan.W.H, n, lm, ep, sc, s)) return rc;
    constexpr int per = DV_THREADS / 64;
    hipLaunchKernelGGL(dv_inverse_kernel, dim3((n + per - 1) / per), dim3(DV_THREADS), sizeof(double) * per * n, s, Lg, n, Mg,
                       status);
    DBA_LAUNCH_CHECK();
  }
  if (!(parts & 2)) return DBA_OK;
  hipLaunchKernelGGL(dv_quadform_kernel, dim3((plan.HW + DV_TP - 1) / DV_TP, plan.T.Mmax), dim3(DV_THREADS), DV_QUAD_LDS, s, Mg,
                     status, n, plan.HW, t0, plan.P, N, var_out, out_rows, plan.T, plan.W);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_ba_depth_variance(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, float *var_out, int out_rows,
                          void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes, dba_stream_t stream) {
  return dba_ba_depth_variance_parts(N, B, ht, wd, t0, t1, lm, ep, var_out, out_rows, scratch, scratch_bytes, ws, ws_bytes, stream, 3);
}

}  // extern "C"
