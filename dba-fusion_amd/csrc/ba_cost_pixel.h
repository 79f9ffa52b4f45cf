// The residual of one pixel on one edge as the BA linearisation sees it, without its Jacobians (csrc/ba_cost.hip).
// Both functions restate expressions of ba_kernels.hip -- edge_pose64 with no pending update, and the head of linearize_pixel up
// to (r, w) -- operation by operation, so that the cost report measures the objective the linearisation minimises: the same
// float64 relative pose rounded once, the same fmaf chains, the same z < 0.25 cut, the same 0.001 weight scale.  They are kept
// apart from those two on purpose: the linearisation kernel's code generation does not depend on this header.
#pragma once
#include "common.h"

namespace dba {

// Gij = Tj Ti^-1 of an edge as t[3], R[9] (row-major): formed in float64 from the float poses, rounded to float once.
// ix == jx is the fixed stereo baseline.  The caller has checked 0 <= ix, jx < B.
__device__ __forceinline__ void cost_edge_pose(const float *__restrict__ poses, int ix, int jx, float *tij, Rot3 &R) {
  double q[4], t[3];
  if (ix == jx) {
    t[0] = -0.1; t[1] = 0.0; t[2] = 0.0;
    q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; q[3] = 1.0;
  } else {
    const float *Pi = poses + 7 * (size_t)ix, *Pj = poses + 7 * (size_t)jx;
    const double ti[3] = {Pi[0], Pi[1], Pi[2]}, qi[4] = {Pi[3], Pi[4], Pi[5], Pi[6]};
    const double tj[3] = {Pj[0], Pj[1], Pj[2]}, qj[4] = {Pj[3], Pj[4], Pj[5], Pj[6]};
    q[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];   // qj * conj(qi)
    q[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
    q[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
    q[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
    const double uv0 = 2.0 * (q[1] * ti[2] - q[2] * ti[1]);
    const double uv1 = 2.0 * (q[2] * ti[0] - q[0] * ti[2]);
    const double uv2 = 2.0 * (q[0] * ti[1] - q[1] * ti[0]);
    t[0] = tj[0] - (ti[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1));
    t[1] = tj[1] - (ti[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2));
    t[2] = tj[2] - (ti[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0));
  }
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  tij[0] = (float)t[0];
  tij[1] = (float)t[1];
  tij[2] = (float)t[2];
  R.r[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  R.r[1] = (float)(2.0 * (x * y - w * z));
  R.r[2] = (float)(2.0 * (x * z + w * y));
  R.r[3] = (float)(2.0 * (x * y + w * z));
  R.r[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  R.r[5] = (float)(2.0 * (y * z - w * x));
  R.r[6] = (float)(2.0 * (x * z - w * y));
  R.r[7] = (float)(2.0 * (y * z + w * x));
  R.r[8] = (float)(1.0 - 2.0 * (x * x + y * y));
}

struct PixelResidual {
  float ru, rv, wu, wv;
};

// false: the pixel is cut (z < 0.25) and out is not written.  A stereo edge keeps its real weights: this is the residual its
// depth block sees.
__device__ __forceinline__ bool residual_pixel(float u, float v, float disp, float tu, float tv, float wgt_u, float wgt_v,
                                               const float *intr, const float *tij, const Rot3 &R, PixelResidual &out) {
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float X0 = (u - cx) / fx, X1 = (v - cy) / fy;
  const float x = fmaf(disp, tij[0], fmaf(R.r[0], X0, fmaf(R.r[1], X1, R.r[2])));
  const float y = fmaf(disp, tij[1], fmaf(R.r[3], X0, fmaf(R.r[4], X1, R.r[5])));
  const float z = fmaf(disp, tij[2], fmaf(R.r[6], X0, fmaf(R.r[7], X1, R.r[8])));
  if (z < 0.25f) return false;
  const float d = 1.f / z;
  out.wu = 0.001f * wgt_u;
  out.wv = 0.001f * wgt_v;
  out.ru = tu - fmaf(fx * d, x, cx);
  out.rv = tv - fmaf(fy * d, y, cy);
  return true;
}

}  // namespace dba
