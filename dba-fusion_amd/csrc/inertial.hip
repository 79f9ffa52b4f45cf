// Inertial factors in the window solve (dba_inertial_linearize, dba_inertial_step, include/dba_hip.h; dbaf_amd/inertial.py
// states the residual).  One visual-inertial Gauss-Newton step without a host read:
//
//   (a) in_linearize_kernel   one workgroup per state k: interval k -> k + 1 (k < P - 1) and the prior of state k.  One lane
//                             forms r (15) and the analytic J (15 x 30) -- a few hundred dependent float64 operations, most of
//                             them zero blocks away from the others --, the workgroup forms L J, J^T (L J) and J^T (L r) from
//                             LDS: every entry one lane, one fixed order, the lower triangle mirrored.
//   (b) in_assemble_kernel    the 15 P x 15 P system, every entry owned by one lane which adds, in this order: the visual
//                             system of the BA workspace (stabiliser on the first six diagonal entries, congruence by the 6 x 6
//                             tangent block -- the arithmetic of ba_export_kernel's layout 1), the interval before the state,
//                             the interval after it, the prior.  rhs = vg - sum J^T L r: the step solves M dx = rhs.
//   (c) dv_factor_kernel      reduced_inverse.h: M + diag(ep + lm diag(M)) = L L^T, one workgroup, the status word.
//   (d) in_solve_retract_kernel   one workgroup: wave 0 runs the two substitutions (dv_solve_rhs), then lane k retracts state k
//                             and forms dx_ba = A dx_g of its pose; a status word that is set makes dx NaN and moves nothing.
//   then ba_retract_device (ba_host.hip): dx_ba rounded to float32, the BA's own back-substitution + retraction launch.
//
// The scratch, in doubles (in_layout): Hf [P-1][900] | gf [P-1][30] | rf [P-1][15] | Hp [P][225] | gp [P][15] | M [n][n] |
// rhs [n] | dx_ba [6P] | then the scratch of reduced_inverse.h for n = 15 P (L, its unused M, the status word).
// All arithmetic is float64; there are no atomics; no kernel indexes beyond what P states.
//
// The dense prior (dba_inertial_state.dense_*): H [15K][15K], b [15K] at a linearisation point x0 of the first K states.
// (a) forms delta_k = local(x0_k, x_k) by lane 0 of state k < K; (b) adds H to M and b - H delta to rhs, the row of H delta
// summed with t ascending by the owner lane of the entry.  No dense prior: the term is skipped.  delta lives in the first
// 15 P doubles of the reduced_inverse scratch's unused M.
//
// Marginalisation (dba_inertial_marginalize): the Schur complement over the m oldest states, four launches behind (a):
//   (e) in_marg_assemble_kernel   the system over S states, the terms of (b) restricted to what touches the departing states
//                             (in_entry: one text for both assemblies), written as M_mm [15m][15m] | M_km | M_kk and rhs [15S]
//   (f) dv_factor_kernel      M_mm = L L^T, no damping
//   (g) in_marg_forward_kernel    W = L^-1 [M_mk | rhs_m]: one wave and one workgroup per column, dv_forward_rhs
//   (h) in_marg_schur_kernel  H_new = M_kk - W W^T (lower triangle, mirrored), b_new = rhs_k - W w, the linearisation point;
//                             a status word that is set makes H_new and b_new NaN and writes nothing else.
// The three parts of the marginal system share the scratch's M (15m x 15m + 15(S-m) x 15m + (15(S-m))^2 <= (15S)^2), W follows
// delta in the reduced_inverse scratch's unused M.
#include "reduced_inverse.h"

namespace dba {
namespace {

constexpr int IN_K = DBA_INERTIAL_K;
constexpr int IN_MAX_P = DBA_INERTIAL_MAX_P;
constexpr int IN_THREADS = 256;
static_assert(15 * IN_MAX_P <= 6 * DV_MAX_P, "the factor kernel's largest system");

// offsets into a packed interval row
constexpr int PK_DR = 0, PK_DV = 9, PK_DP = 12, PK_DT = 15, PK_JRG = 16, PK_JVA = 25, PK_JVG = 34, PK_JPA = 43, PK_JPG = 52,
              PK_BIAS = 61, PK_L9 = 67, PK_L6 = 148;
static_assert(PK_L6 + 36 == IN_K, "the packed row");

struct InLayout {   // the parts of a scratch of in_scratch_bytes(P) bytes
  double *Hf, *gf, *rf, *Hp, *gp, *M, *rhs, *dxba;
  void *dv;
  double *delta() const { return static_cast<double *>(dv) + (size_t)225 * P * P; }   // [15 P], in the unused M of dv
  double *W() const { return delta() + (size_t)15 * P; }                             // the marginalisation's [15 (S - m) + 1][15 m]
  int P;
  InLayout(void *scratch, int P_) : P(P_) {
    const size_t n = (size_t)15 * P;
    Hf = static_cast<double *>(scratch);
    gf = Hf + (size_t)900 * (P - 1);
    rf = gf + (size_t)30 * (P - 1);
    Hp = rf + (size_t)15 * (P - 1);
    gp = Hp + (size_t)225 * P;
    M = gp + (size_t)15 * P;
    rhs = M + n * n;
    dxba = rhs + n;
    dv = dxba + (size_t)6 * P;
  }
};
inline size_t in_scratch_bytes(int P) {
  const size_t n = (size_t)15 * P;
  return sizeof(double) * ((size_t)945 * (P - 1) + (size_t)240 * P + n * n + n + (size_t)6 * P) + dv_scratch_bytes((int)n);
}

struct InState {   // dba_inertial_state as the kernels take it
  double *R, *p, *vel, *bias;
  const double *pR, *pp, *pv, *pb, *pw;
  double g[3];
  const double *dR, *dp, *dvel, *dbias, *dH, *db;   // the dense prior over the first dK states; dH null: none
  int dK;
};

// ---- 3 x 3, row-major -------------------------------------------------------------------------------------------------------
__device__ inline void m3_mul(const double *A, const double *B, double *C) {     // C = A B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ inline void m3_tmul(const double *A, const double *B, double *C) {    // C = A^T B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ inline void m3_vec(const double *A, const double *x, double *y) {     // y = A x
  for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
__device__ inline void m3_tvec(const double *A, const double *x, double *y) {    // y = A^T x
  for (int i = 0; i < 3; i++) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}
__device__ inline void m3_hat(const double *v, double *W) {
  W[0] = 0.0, W[1] = -v[2], W[2] = v[1], W[3] = v[2], W[4] = 0.0, W[5] = -v[0], W[6] = -v[1], W[7] = v[0], W[8] = 0.0;
}
// I + a W + b W^2, W = hat(phi)
__device__ inline void so3_poly(const double *phi, double a, double b, double *R) {
  double W[9], W2[9];
  m3_hat(phi, W);
  m3_mul(W, W, W2);
  for (int e = 0; e < 9; e++) R[e] = ((e % 4 == 0) ? 1.0 : 0.0) + a * W[e] + b * W2[e];
}
// sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3
__device__ inline void so3_coeffs(double th2, double &a, double &b, double &c) {
  const double th = sqrt(th2);
  if (th < 1e-4) {
    a = 1.0 - th2 / 6.0, b = 0.5 - th2 / 24.0, c = 1.0 / 6.0 - th2 / 120.0;
  } else {
    a = sin(th) / th, b = (1.0 - cos(th)) / th2, c = (th - sin(th)) / (th2 * th);
  }
}
__device__ inline double dot3(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
__device__ inline void so3_exp(const double *phi, double *R) {
  double a, b, c;
  so3_coeffs(dot3(phi, phi), a, b, c);
  so3_poly(phi, a, b, R);
}
__device__ inline void so3_log(const double *R, double *phi) {   // (rotations close to pi are outside the interface)
  const double w[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double s = sqrt(dot3(w, w)), c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double k = s < 1e-4 ? 1.0 + s * s / 6.0 : atan2(s, c) / s;
  for (int i = 0; i < 3; i++) phi[i] = k * w[i];
}
__device__ inline void so3_jr(const double *phi, double *J) {
  double a, b, c;
  so3_coeffs(dot3(phi, phi), a, b, c);
  so3_poly(phi, -b, c, J);
}
__device__ inline void so3_jr_inv(const double *phi, double *J) {
  const double th2 = dot3(phi, phi), th = sqrt(th2);
  const double k = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  so3_poly(phi, 0.5, k, J);
}
__device__ inline void put3(double *J, int ld, int r0, int c0, const double *B, double s) {   // block (r0, c0) of J = s B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) J[(r0 + i) * ld + c0 + j] = s * B[3 * i + j];
}

// r [15] and J [15][30] (zeroed by the caller) of interval k, by one lane
__device__ void in_interval(const InState &st, int k, const double *pk, double *r, double *J) {
  const double *Ri = st.R + 9 * k, *Rj = st.R + 9 * (k + 1), *pi = st.p + 3 * k, *pj = st.p + 3 * (k + 1);
  const double *vi = st.vel + 3 * k, *vj = st.vel + 3 * (k + 1), *bi = st.bias + 6 * k, *bj = st.bias + 6 * (k + 1);
  const double dt = pk[PK_DT];
  double dba[3], dbg[3];
  for (int i = 0; i < 3; i++) dba[i] = bi[i] - pk[PK_BIAS + i], dbg[i] = bi[3 + i] - pk[PK_BIAS + 3 + i];
  // r_R = Log((dR Exp(JRg dbg))^T R_i^T R_j)
  double c[3], Ec[9], dRc[9], Rij[9], Er[9], rR[3], Ji[9], T1[9], T2[9];
  m3_vec(pk + PK_JRG, dbg, c);
  so3_exp(c, Ec);
  m3_mul(pk + PK_DR, Ec, dRc);
  m3_tmul(Ri, Rj, Rij);
  m3_tmul(dRc, Rij, Er);
  so3_log(Er, rR);
  so3_jr_inv(rR, Ji);
  // r_v, r_p
  double a[3], x[3], y[3], sv[3], sp[3];
  for (int i = 0; i < 3; i++) x[i] = vj[i] - vi[i] - st.g[i] * dt;
  m3_tvec(Ri, x, sv);
  for (int i = 0; i < 3; i++) x[i] = pj[i] - pi[i] - vi[i] * dt - 0.5 * st.g[i] * dt * dt;
  m3_tvec(Ri, x, sp);
  m3_vec(pk + PK_JVA, dba, a);
  m3_vec(pk + PK_JVG, dbg, y);
  for (int i = 0; i < 3; i++) r[i] = rR[i], r[3 + i] = sv[i] - (pk[PK_DV + i] + a[i] + y[i]);
  m3_vec(pk + PK_JPA, dba, a);
  m3_vec(pk + PK_JPG, dbg, y);
  for (int i = 0; i < 3; i++) r[6 + i] = sp[i] - (pk[PK_DP + i] + a[i] + y[i]);
  for (int i = 0; i < 6; i++) r[9 + i] = bj[i] - bi[i];
  // the rotation row
  double Rji[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rji[3 * i + j] = Rij[3 * j + i];
  m3_mul(Ji, Rji, T1);
  put3(J, 30, 0, 0, T1, -1.0);
  so3_jr(c, T1);
  m3_mul(T1, pk + PK_JRG, T2);       // Jr(c) JRg
  m3_tmul(Er, T2, T1);               // Exp(r_R)^T ..
  m3_mul(Ji, T1, T2);
  put3(J, 30, 0, 12, T2, -1.0);
  put3(J, 30, 0, 15, Ji, 1.0);
  // the velocity row
  double RiT[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) RiT[3 * i + j] = Ri[3 * j + i];
  m3_hat(sv, T1);
  put3(J, 30, 3, 0, T1, 1.0);
  put3(J, 30, 3, 6, RiT, -1.0);
  put3(J, 30, 3, 9, pk + PK_JVA, -1.0);
  put3(J, 30, 3, 12, pk + PK_JVG, -1.0);
  put3(J, 30, 3, 21, RiT, 1.0);
  // the position row
  m3_hat(sp, T1);
  put3(J, 30, 6, 0, T1, 1.0);
  for (int i = 0; i < 3; i++) J[(6 + i) * 30 + 3 + i] = -1.0;
  put3(J, 30, 6, 6, RiT, -dt);
  put3(J, 30, 6, 9, pk + PK_JPA, -1.0);
  put3(J, 30, 6, 12, pk + PK_JPG, -1.0);
  put3(J, 30, 6, 18, Rij, 1.0);
  // the bias row
  for (int i = 0; i < 6; i++) J[(9 + i) * 30 + 9 + i] = -1.0, J[(9 + i) * 30 + 24 + i] = 1.0;
}

// r [15] = the tangent at the anchor that leads to state k, J [15][15] (zeroed by the caller) = blockdiag(Jr^-1(r_phi), R_a^T R, I)
__device__ void in_prior(const InState &st, int k, double *r, double *J) {
  double Rar[9], T[9];
  m3_tmul(st.pR + 9 * k, st.R + 9 * k, Rar);
  so3_log(Rar, r);
  double x[3];
  for (int i = 0; i < 3; i++) x[i] = st.p[3 * k + i] - st.pp[3 * k + i];
  m3_tvec(st.pR + 9 * k, x, r + 3);
  for (int i = 0; i < 3; i++) r[6 + i] = st.vel[3 * k + i] - st.pv[3 * k + i];
  for (int i = 0; i < 6; i++) r[9 + i] = st.bias[6 * k + i] - st.pb[6 * k + i];
  so3_jr_inv(r, T);
  put3(J, 15, 0, 0, T, 1.0);
  put3(J, 15, 3, 3, Rar, 1.0);
  for (int i = 6; i < 15; i++) J[i * 15 + i] = 1.0;
}

// d [15] = local(x0_k, x_k) of the dense prior: (Log(R0^T R), R0^T (p - p0), v - v0, bias - bias0), by one lane
__device__ void in_local(const InState &st, int k, double *d) {
  double Rr[9], x[3];
  m3_tmul(st.dR + 9 * k, st.R + 9 * k, Rr);
  so3_log(Rr, d);
  for (int i = 0; i < 3; i++) x[i] = st.p[3 * k + i] - st.dp[3 * k + i];
  m3_tvec(st.dR + 9 * k, x, d + 3);
  for (int i = 0; i < 3; i++) d[6 + i] = st.vel[3 * k + i] - st.dvel[3 * k + i];
  for (int i = 0; i < 6; i++) d[9 + i] = st.bias[6 * k + i] - st.dbias[6 * k + i];
}

__global__ __launch_bounds__(IN_THREADS) void in_linearize_kernel(InState st, int P, const double *__restrict__ preint,
                                                                  double *__restrict__ r_out, double *__restrict__ H_out,
                                                                  double *__restrict__ g_out, double *__restrict__ Hp,
                                                                  double *__restrict__ gp, double *__restrict__ delta) {
  __shared__ double pk[IN_K], J[450], LJ[450], r[15], Lr[15];
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= P) return;
  if (st.dH && k < st.dK && tid == 0) in_local(st, k, delta + 15 * k);   // (read by the assembly launch alone)
  if (k < P - 1) {   // (uniform over the workgroup: every barrier below is reached by all of it)
    for (int e = tid; e < IN_K; e += IN_THREADS) pk[e] = preint[(size_t)IN_K * k + e];
    for (int e = tid; e < 450; e += IN_THREADS) J[e] = 0.0;
    __syncthreads();
    if (tid == 0) in_interval(st, k, pk, r, J);
    __syncthreads();
    // L J and L r, L = blockdiag(L9, L6)
    for (int e = tid; e < 465; e += IN_THREADS) {
      const int row = e < 450 ? e / 30 : e - 450, col = e < 450 ? e - 30 * row : -1;
      const int b0 = row < 9 ? 0 : 9, bn = row < 9 ? 9 : 6;
      const double *L = row < 9 ? pk + PK_L9 + 9 * row : pk + PK_L6 + 6 * (row - 9);
      double s = 0.0;
      for (int l = 0; l < bn; l++) s = fma(L[l], col >= 0 ? J[(b0 + l) * 30 + col] : r[b0 + l], s);
      if (col >= 0) LJ[e] = s;
      else Lr[row] = s;
    }
    __syncthreads();
    // J^T (L J): the lower triangle's sum for both mirror entries; J^T (L r); r
    for (int e = tid; e < 945; e += IN_THREADS) {
      if (e < 900) {
        const int a = e / 30, c = e - 30 * a, hi = max(a, c), lo = min(a, c);
        double s = 0.0;
        for (int l = 0; l < 15; l++) s = fma(J[l * 30 + hi], LJ[l * 30 + lo], s);
        H_out[(size_t)900 * k + e] = s;
      } else if (e < 930) {
        const int a = e - 900;
        double s = 0.0;
        for (int l = 0; l < 15; l++) s = fma(J[l * 30 + a], Lr[l], s);
        g_out[(size_t)30 * k + a] = s;
      } else {
        r_out[(size_t)15 * k + e - 930] = r[e - 930];
      }
    }
    __syncthreads();
  }
  // the prior of state k: J^T W J [15][15], J^T W r [15]; zeros without one
  if (!st.pw) {
    for (int e = tid; e < 240; e += IN_THREADS) {
      if (e < 225) Hp[(size_t)225 * k + e] = 0.0;
      else gp[(size_t)15 * k + e - 225] = 0.0;
    }
    return;
  }
  for (int e = tid; e < 225; e += IN_THREADS) J[e] = 0.0;
  __syncthreads();
  if (tid == 0) in_prior(st, k, r, J);
  __syncthreads();
  for (int e = tid; e < 240; e += IN_THREADS) {
    const double *w = st.pw + (size_t)15 * k;
    double s = 0.0;
    if (e < 225) {
      const int a = e / 15, c = e - 15 * a, hi = max(a, c), lo = min(a, c);
      for (int l = 0; l < 15; l++) s = fma(J[l * 15 + hi] * w[l], J[l * 15 + lo], s);
      Hp[(size_t)225 * k + e] = s;
    } else {
      const int a = e - 225;
      for (int l = 0; l < 15; l++) s = fma(J[l * 15 + a] * w[l], r[l], s);
      gp[(size_t)15 * k + a] = s;
    }
  }
}

// The terms an entry of a system over the states' tangents takes, in the order they are added: the visual system (H6, b6: a BA
// workspace's reduced camera system over Pv poses, LOWER triangle; states < Pv), the intervals k < nI (before the state, then
// after it), the diagonal priors of the states < nP, the dense prior over the first nd unknowns (dH null: skipped).
struct InTerms {
  const double *H6, *b6;
  int Pv;
  const double *Hf, *gf;
  int nI;
  const double *Hp, *gp;
  int nP;
  const double *dH, *db, *delta;
  int nd;
};

// entry (hi, lo), hi >= lo, of the system's matrix
__device__ inline double in_entry(const InTerms &T, const ExportArg &arg, double stab, int hi, int lo) {
  const int si = hi / 15, a = hi - 15 * si, sj = lo / 15, c = lo - 15 * sj, n6 = 6 * T.Pv;
  double v = 0.0;
  if (a < 6 && c < 6 && si < T.Pv) {   // (A^T (H + stabiliser) A)[6 si + a][6 sj + c], as ba_export_kernel forms it
    auto h = [&](int r, int q) {
      const double x = T.H6[(size_t)max(r, q) * n6 + min(r, q)];
      return (r == q && r < 6) ? x + stab : x;
    };
#pragma unroll
    for (int k = 0; k < 6; k++) {
      double t = 0.0;
#pragma unroll
      for (int l = 0; l < 6; l++) t = fma(h(6 * si + k, 6 * sj + l), arg.A[6 * l + c], t);
      v = fma(arg.A[6 * k + a], t, v);
    }
  }
  if (si >= 1 && si - 1 < T.nI && sj == si) v += T.Hf[(size_t)900 * (si - 1) + 30 * (15 + a) + 15 + c];
  if (si >= 1 && si - 1 < T.nI && sj == si - 1) v += T.Hf[(size_t)900 * (si - 1) + 30 * (15 + a) + c];
  if (si < T.nI && sj == si) v += T.Hf[(size_t)900 * si + 30 * a + c];
  if (si < T.nP && sj == si) v += T.Hp[(size_t)225 * si + 15 * a + c];
  if (T.dH && hi < T.nd) v += T.dH[(size_t)hi * T.nd + lo];
  return v;
}

// entry i of the system's right-hand side
__device__ inline double in_rhs_entry(const InTerms &T, const ExportArg &arg, int i) {
  const int s = i / 15, a = i - 15 * s;
  double v = 0.0;
  if (a < 6 && s < T.Pv) {   // vg = sum_k A[k][a] v[6 s + k]
#pragma unroll
    for (int k = 0; k < 6; k++) v = fma(arg.A[6 * k + a], T.b6[6 * s + k], v);
  }
  if (s >= 1 && s - 1 < T.nI) v -= T.gf[(size_t)30 * (s - 1) + 15 + a];
  if (s < T.nI) v -= T.gf[(size_t)30 * s + a];
  if (s < T.nP) v -= T.gp[(size_t)15 * s + a];
  if (T.dH && i < T.nd) {    // b - H delta, the row's sum with t ascending
    const double *row = T.dH + (size_t)i * T.nd;
    double hd = 0.0;
    for (int t = 0; t < T.nd; t++) hd = fma(row[t], T.delta[t], hd);
    v += T.db[i] - hd;
  }
  return v;
}

// M [n][n] full, rhs [n], n = 15 P: the step's system (T.Pv = T.nP = P, T.nI = P - 1)
__global__ __launch_bounds__(IN_THREADS) void in_assemble_kernel(InTerms T, int P, ExportArg arg, double stab, double *__restrict__ M,
                                                                 double *__restrict__ rhs) {
  const int n = 15 * P;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n + n) return;
  if (idx >= n * n) {
    rhs[idx - n * n] = in_rhs_entry(T, arg, idx - n * n);
    return;
  }
  const int i = idx / n, j = idx - i * n;
  M[idx] = in_entry(T, arg, stab, max(i, j), min(i, j));
}

// The marginal system over S states, nm = 15 m departing unknowns first: Mmm [nm][nm] (the row length dv_factor_kernel takes),
// Mkm [nk][nm], Mkk [nk][nk], nk = 15 (S - m), and rhs [15 S].  One owner lane per entry; M_mk is M_km transposed and is not stored.
__global__ __launch_bounds__(IN_THREADS) void in_marg_assemble_kernel(InTerms T, int S, int m, ExportArg arg, double stab,
                                                                      double *__restrict__ Mmm, double *__restrict__ Mkm,
                                                                      double *__restrict__ Mkk, double *__restrict__ rhs) {
  const int n = 15 * S, nm = 15 * m, nk = n - nm;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n + n) return;
  if (idx >= n * n) {
    rhs[idx - n * n] = in_rhs_entry(T, arg, idx - n * n);
    return;
  }
  const int i = idx / n, j = idx - i * n;
  if (i < nm && j >= nm) return;
  const double v = in_entry(T, arg, stab, max(i, j), min(i, j));
  if (i < nm) Mmm[(size_t)i * nm + j] = v;
  else if (j < nm) Mkm[(size_t)(i - nm) * nm + j] = v;
  else Mkk[(size_t)(i - nm) * nk + j - nm] = v;
}

// W [nk + 1][nm]: row c < nk = L^-1 (column c of M_mk = row c of Mkm), row nk = L^-1 rhs_m.  One wave per workgroup and column.
__global__ __launch_bounds__(64) void in_marg_forward_kernel(const double *__restrict__ Lg, const int *__restrict__ status, int nm,
                                                             int nk, const double *__restrict__ Mkm, const double *__restrict__ rhs,
                                                             double *__restrict__ W) {
  __shared__ double y[15 * (IN_MAX_P - 1)];
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c > nk || status[0]) return;   // (no factor: the Schur launch writes NaN and reads nothing of W)
  const double *src = c < nk ? Mkm + (size_t)c * nm : rhs;
  dv_forward_rhs(Lg, nm, 0, [src](int i) { return src[i]; }, y, lane);
  for (int t = lane; t < nm; t += 64) W[(size_t)c * nm + t] = y[t];   // (lane t & 63 owns y[t])
}

// H_new [nk][nk] = Mkk - W W^T: one lane per entry of the lower triangle, the sum with t ascending, mirrored; b_new [nk]; the
// linearisation point = the states m .. S - 1 (21 doubles each).  status set: H_new, b_new NaN, nothing else written.
__global__ __launch_bounds__(IN_THREADS) void in_marg_schur_kernel(const int *__restrict__ status, int nm, int nk, int m,
                                                                   const double *__restrict__ Mkk, const double *__restrict__ rhs,
                                                                   const double *__restrict__ W, InState st, double *__restrict__ H_new,
                                                                   double *__restrict__ b_new, double *__restrict__ R0,
                                                                   double *__restrict__ p0, double *__restrict__ vel0,
                                                                   double *__restrict__ bias0, int *__restrict__ status_out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, K = nk / 15;
  const bool bad = status[0] != 0;
  if (idx == 0 && status_out) status_out[0] = bad ? 1 : 0;
  if (idx < nk * nk) {
    const int i = idx / nk, j = idx - i * nk;
    if (j > i) return;
    double v = __builtin_nan("");
    if (!bad) {
      const double *wi = W + (size_t)i * nm, *wj = W + (size_t)j * nm;
      double s = 0.0;
      for (int t = 0; t < nm; t++) s = fma(wi[t], wj[t], s);
      v = Mkk[idx] - s;
    }
    H_new[(size_t)i * nk + j] = v;
    H_new[(size_t)j * nk + i] = v;
  } else if (idx < nk * nk + nk) {
    const int i = idx - nk * nk;
    double v = __builtin_nan("");
    if (!bad) {
      const double *wi = W + (size_t)i * nm, *wr = W + (size_t)nk * nm;
      double s = 0.0;
      for (int t = 0; t < nm; t++) s = fma(wi[t], wr[t], s);
      v = rhs[nm + i] - s;
    }
    b_new[i] = v;
  } else if (idx < nk * nk + nk + 21 * K && !bad) {
    const int e = idx - nk * nk - nk;
    if (e < 9 * K) R0[e] = st.R[9 * m + e];
    else if (e < 12 * K) p0[e - 9 * K] = st.p[3 * m + e - 9 * K];
    else if (e < 15 * K) vel0[e - 12 * K] = st.vel[3 * m + e - 12 * K];
    else bias0[e - 15 * K] = st.bias[6 * m + e - 15 * K];
  }
}

__global__ __launch_bounds__(IN_THREADS) void in_solve_retract_kernel(const double *__restrict__ Lg, const int *__restrict__ status,
                                                                      int P, const double *__restrict__ rhs, InState st,
                                                                      ExportArg arg, double *__restrict__ dx_out,
                                                                      double *__restrict__ dxba, int *__restrict__ status_out) {
  __shared__ double y[15 * IN_MAX_P];
  const int n = 15 * P, tid = threadIdx.x;
  if (status[0]) {   // a pivot was not positive: no step exists
    for (int e = tid; e < n; e += IN_THREADS) dx_out[e] = __builtin_nan("");
    for (int e = tid; e < 6 * P; e += IN_THREADS) dxba[e] = 0.0;   // (what the skipped retraction's copy puts into the workspace)
    if (tid == 0 && status_out) status_out[0] = 1;
    return;
  }
  if (tid < 64) dv_solve_rhs(Lg, n, 0, [rhs](int i) { return rhs[i]; }, y, tid);
  __syncthreads();
  for (int e = tid; e < n; e += IN_THREADS) dx_out[e] = y[e];
  if (tid == 0 && status_out) status_out[0] = 0;
  if (tid >= P) return;
  const int k = tid;
  const double *d = y + 15 * k;
  double E[9], Rn[9], x[3];
  double *R = st.R + 9 * k;
  m3_vec(R, d + 3, x);                       // p <- p + R dp with R as it was
  for (int i = 0; i < 3; i++) st.p[3 * k + i] += x[i];
  so3_exp(d, E);
  m3_mul(R, E, Rn);
  for (int e = 0; e < 9; e++) R[e] = Rn[e];
  for (int i = 0; i < 3; i++) st.vel[3 * k + i] += d[6 + i];
  for (int i = 0; i < 6; i++) st.bias[6 * k + i] += d[9 + i];
  for (int r = 0; r < 6; r++) {              // dx_ba = A dx_g
    double s = 0.0;
    for (int q = 0; q < 6; q++) s = fma(arg.A[6 * r + q], d[q], s);
    dxba[6 * k + r] = s;
  }
}

inline bool misaligned(const void *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(double) != 0; }

// every refusal of both entries that needs no plan, before the first runtime call
int in_check(const dba_inertial_state *st, int P, const double *preint, int preint_rows, const void *scratch, size_t scratch_bytes,
             InState *out) {
  if (!st || !st->R || !st->p || !st->vel || !st->bias || !preint || !scratch) return DBA_ERR_ARG;
  const int given = (st->prior_R != nullptr) + (st->prior_p != nullptr) + (st->prior_vel != nullptr) + (st->prior_bias != nullptr) +
                    (st->prior_w != nullptr);
  if (given != 0 && given != 5) return DBA_ERR_ARG;
  const int dense = (st->dense_R != nullptr) + (st->dense_p != nullptr) + (st->dense_vel != nullptr) + (st->dense_bias != nullptr) +
                    (st->dense_H != nullptr) + (st->dense_b != nullptr);
  if ((dense != 0 && dense != 6) || (dense == 0 && st->dense_K != 0)) return DBA_ERR_ARG;
  const void *ptrs[] = {st->R, st->p, st->vel, st->bias, st->prior_R, st->prior_p, st->prior_vel, st->prior_bias, st->prior_w,
                        st->dense_R, st->dense_p, st->dense_vel, st->dense_bias, st->dense_H, st->dense_b, preint, scratch};
  for (const void *q : ptrs)
    if (misaligned(q)) return DBA_ERR_ARG;
  if (P < 2 || preint_rows < P - 1) return DBA_ERR_ARG;
  if (dense == 6 && (st->dense_K < 1 || st->dense_K > P)) return DBA_ERR_ARG;
  if (P > IN_MAX_P) return DBA_ERR_UNSUPPORTED;
  if (scratch_bytes < in_scratch_bytes(P)) return DBA_ERR_WORKSPACE;
  out->R = st->R, out->p = st->p, out->vel = st->vel, out->bias = st->bias;
  out->pR = st->prior_R, out->pp = st->prior_p, out->pv = st->prior_vel, out->pb = st->prior_bias, out->pw = st->prior_w;
  for (int i = 0; i < 3; i++) out->g[i] = st->gravity[i];
  out->dR = st->dense_R, out->dp = st->dense_p, out->dvel = st->dense_vel, out->dbias = st->dense_bias;
  out->dH = st->dense_H, out->db = st->dense_b, out->dK = st->dense_K;
  return DBA_OK;
}

int in_launch_linearize(const InState &s, int P, const double *preint, double *r_out, double *H_out, double *g_out,
                        const InLayout &lay, hipStream_t stream) {
  hipLaunchKernelGGL(in_linearize_kernel, dim3(P), dim3(IN_THREADS), 0, stream, s, P, preint, r_out ? r_out : lay.rf,
                     H_out ? H_out : lay.Hf, g_out ? g_out : lay.gf, lay.Hp, lay.gp, lay.delta());
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace
}  // namespace dba

using namespace dba;

extern "C" {

size_t dba_inertial_scratch_bytes(int P) { return (P < 2 || P > IN_MAX_P) ? 0 : in_scratch_bytes(P); }
size_t dba_inertial_marg_scratch_bytes(int P) { return dba_inertial_scratch_bytes(P); }   // (one scratch serves both entries)

int dba_inertial_linearize(const dba_inertial_state *st, int P, const double *preint, int preint_rows, double *r_out,
                           double *H_out, double *g_out, void *scratch, size_t scratch_bytes, dba_stream_t stream) {
  InState s;
  if (const int rc = in_check(st, P, preint, preint_rows, scratch, scratch_bytes, &s)) return rc;
  if (misaligned(r_out) || misaligned(H_out) || misaligned(g_out)) return DBA_ERR_ARG;
  return in_launch_linearize(s, P, preint, r_out, H_out, g_out, InLayout(scratch, P), static_cast<hipStream_t>(stream));
}

int dba_inertial_step(const dba_inertial_state *st, int P, const double *preint, int preint_rows, const double *A36,
                      double stabilizer, float lm, float ep, float *poses, float *disps, const int64_t *ii, const int64_t *jj, int N,
                      int B, int ht, int wd, int t0, int t1, double *dx_out, int *status_out, void *scratch, size_t scratch_bytes,
                      void *ws, size_t ws_bytes, dba_stream_t stream) {
  (void)ii;
  InState s;
  if (const int rc = in_check(st, P, preint, preint_rows, scratch, scratch_bytes, &s)) return rc;
  if (!A36 || !dx_out || !poses || !disps || !jj || misaligned(dx_out)) return DBA_ERR_ARG;
  DBA_PLAN_OR_RETURN(plan);
  if (plan.P != P) return DBA_ERR_ARG;

  const InLayout lay(scratch, P);
  const int n = 15 * P;
  const DvScratch sc(lay.dv, n);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  ExportArg arg;
  for (int e = 0; e < 36; e++) arg.A[e] = A36[e];
  if (const int rc = in_launch_linearize(s, P, preint, nullptr, nullptr, nullptr, lay, hs)) return rc;
  const InTerms terms = {plan.W.H, plan.W.b, P, lay.Hf, lay.gf, P - 1, lay.Hp, lay.gp, P, s.dH, s.db, lay.delta(), 15 * s.dK};
  hipLaunchKernelGGL(in_assemble_kernel, dim3((n * n + n + IN_THREADS - 1) / IN_THREADS), dim3(IN_THREADS), 0, hs, terms, P, arg,
                     stabilizer, lay.M, lay.rhs);
  DBA_LAUNCH_CHECK();
  if (const int rc = dv_launch_factor(lay.M, n, lm, ep, sc, hs)) return rc;
  hipLaunchKernelGGL(in_solve_retract_kernel, dim3(1), dim3(IN_THREADS), 0, hs, sc.Lg, sc.status, P, lay.rhs, s, arg, dx_out, lay.dxba,
                     status_out);
  DBA_LAUNCH_CHECK();
  return ba_retract_device(plan, poses, disps, jj, lay.dxba, sc.status, nullptr, nullptr, hs);
}

int dba_inertial_marginalize(const dba_inertial_state *st, int P, const double *preint, int preint_rows, const double *A36,
                             double stabilizer, int m, int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes,
                             double *H_new, int h_rows, double *b_new, int b_rows, double *R0, double *p0, double *vel0,
                             double *bias0, int x0_rows, int *status_out, void *scratch, size_t scratch_bytes, dba_stream_t stream) {
  InState s;
  if (const int rc = in_check(st, P, preint, preint_rows, scratch, scratch_bytes, &s)) return rc;
  if (!A36 || !H_new || !b_new || !R0 || !p0 || !vel0 || !bias0) return DBA_ERR_ARG;
  for (const void *q : {(const void *)H_new, (const void *)b_new, (const void *)R0, (const void *)p0, (const void *)vel0,
                        (const void *)bias0})
    if (misaligned(q)) return DBA_ERR_ARG;
  if (m < 1 || m >= P) return DBA_ERR_ARG;
  BaPlan plan;
  int Pm = 0;
  if (ws) {   // (no workspace: nothing visual was selected)
    if (const int rc = ba_plan(N, B, ht, wd, t0, t1, ws, ws_bytes, &plan)) return rc;
    Pm = plan.P;
  }
  if (Pm > P) return DBA_ERR_ARG;
  const int S = std::max(std::max(Pm, m + 1), s.dH ? s.dK : 0), K = S - m;   // (dK <= P: in_check)
  if (h_rows < 15 * K || b_rows < 15 * K || x0_rows < K) return DBA_ERR_ARG;

  const InLayout lay(scratch, P);
  const int n = 15 * S, nm = 15 * m, nk = 15 * K;
  const DvScratch sc(lay.dv, 15 * P);   // (the factor of nm unknowns fills the head of L; the status word stays where the step's is)
  hipStream_t hs = static_cast<hipStream_t>(stream);
  ExportArg arg;
  for (int e = 0; e < 36; e++) arg.A[e] = A36[e];
  double *Mmm = lay.M, *Mkm = Mmm + (size_t)nm * nm, *Mkk = Mkm + (size_t)nk * nm;
  if (const int rc = in_launch_linearize(s, P, preint, nullptr, nullptr, nullptr, lay, hs)) return rc;
  const InTerms terms = {Pm ? plan.W.H : nullptr, Pm ? plan.W.b : nullptr, Pm, lay.Hf, lay.gf, m, lay.Hp, lay.gp, m, s.dH, s.db,
                         lay.delta(), 15 * s.dK};
  hipLaunchKernelGGL(in_marg_assemble_kernel, dim3((n * n + n + IN_THREADS - 1) / IN_THREADS), dim3(IN_THREADS), 0, hs, terms, S, m,
                     arg, stabilizer, Mmm, Mkm, Mkk, lay.rhs);
  DBA_LAUNCH_CHECK();
  if (const int rc = dv_launch_factor(Mmm, nm, 0.0f, 0.0f, sc, hs)) return rc;
  hipLaunchKernelGGL(in_marg_forward_kernel, dim3(nk + 1), dim3(64), 0, hs, sc.Lg, sc.status, nm, nk, Mkm, lay.rhs, lay.W());
  DBA_LAUNCH_CHECK();
  const int lanes = nk * nk + nk + 21 * K;
  hipLaunchKernelGGL(in_marg_schur_kernel, dim3((lanes + IN_THREADS - 1) / IN_THREADS), dim3(IN_THREADS), 0, hs, sc.status, nm, nk, m,
                     Mkk, lay.rhs, lay.W(), s, H_new, b_new, R0, p0, vel0, bias0, status_out);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
