// The lietorch shim's SE3.inv on a (t, q_xyzw) row (lietorch/__init__.py: _qinv, _qrot, SE3.inv), in its order of
// operations.  Shared by keyframe_check_kernel (keyframe.hip), the map export's plan launch (map_export.hip) and
// world_poses_kernel (frames.hip).  Callers that need the same BITS for the same pose call kf_inv_matrix below.
#pragma once
#include "common.h"

namespace dba {

// ---- the shim's float statements, unfused ---------------------------------------------------------------------------
__device__ __forceinline__ void kf_cross(const float *a, const float *b, float *c) {
  c[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
  c[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
  c[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
}

// _qrot: uv = 2 * cross(qv, v); v + w * uv + cross(qv, uv)
__device__ __forceinline__ void kf_qrot(const float *q, const float *v, float *out) {
  float uv[3], c[3];
  kf_cross(q, v, uv);
#pragma unroll
  for (int k = 0; k < 3; k++) uv[k] = __fmul_rn(2.0f, uv[k]);
  kf_cross(q, uv, c);
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = __fadd_rn(__fadd_rn(v[k], __fmul_rn(q[3], uv[k])), c[k]);
}

// SE3.inv: qi = q * (-1, -1, -1, 1), ti = -_qrot(qi, t)
__device__ __forceinline__ void kf_inv(const float *P, float *ti, float *qi) {
  qi[0] = -P[3]; qi[1] = -P[4]; qi[2] = -P[5]; qi[3] = P[6];
  float r[3];
  kf_qrot(qi, P, r);
  ti[0] = -r[0]; ti[1] = -r[1]; ti[2] = -r[2];
}

// poses[r].inv().matrix(), its first three rows (row-major 3 x 4): the columns of R are _qrot(qi, e_k), the fourth column is
// ti.  NOT inlined.  To hipcc the intrinsics above are plain operators, and its backend fuses a product into a sum where it
// finds one; which ones it finds depends on the code around an inlined copy (keyframe_check_kernel and a second kernel with
// the same statements inlined differed in the last bits of ti).  A call is compiled once per translation unit from this text
// alone, so keyframe_check_kernel (keyframe.hip) and world_poses_kernel (frames.hip), built with the same flags, give the
// same bits for the same pose.
struct KfMat34 {
  float m[12];
};
static __device__ __noinline__ KfMat34 kf_inv_matrix(float tx, float ty, float tz, float qx, float qy, float qz, float qw) {
  const float P[7] = {tx, ty, tz, qx, qy, qz, qw};
  float ti[3], qi[4];
  kf_inv(P, ti, qi);
  KfMat34 M;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float e[3] = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f};
    float col[3];
    kf_qrot(qi, e, col);
    M.m[0 + k] = col[0]; M.m[4 + k] = col[1]; M.m[8 + k] = col[2];
  }
  M.m[3] = ti[0]; M.m[7] = ti[1]; M.m[11] = ti[2];
  return M;
}

}  // namespace dba
