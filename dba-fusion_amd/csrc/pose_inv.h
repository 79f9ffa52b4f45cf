// The lietorch shim's SE3.inv on a (t, q_xyzw) row (lietorch/__init__.py: _qinv, _qrot, SE3.inv), in its order of
// operations, each spelled with an intrinsic the compiler does not fuse: the same bits in every translation unit.
// Shared by keyframe_check_kernel (keyframe.hip) and the map export's plan launch (map_export.hip).
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

}  // namespace dba
