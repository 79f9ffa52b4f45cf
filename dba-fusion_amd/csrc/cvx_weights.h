// The per-output arithmetic of convex upsampling (dbaf/droid_net.py:17-31), shared by cvx_upsample_kernel (upsample.hip)
// and upmask_upsample_kernel (upmask.hip): ONE routine, so that the two launches agree to the last bit on the same mask
// values (inlined copies of such arithmetic have differed in their last bits before: DESIGN.md 4.19).
#pragma once
#include <hip/hip_runtime.h>

namespace dba {

// The zero-padded 3x3 neighbourhood of pixel (y, x) of one [ht, wd] disparity map, tap k = ky*3 + kx.
__device__ __forceinline__ void cvx_taps(const float *__restrict__ d, int y, int x, int ht, int wd, float (&dk)[9]) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = y + ky - 1;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = x + kx - 1;
      const bool in = yy >= 0 && yy < ht && xx >= 0 && xx < wd;
      dk[ky * 3 + kx] = in ? d[yy * wd + xx] : 0.f;
    }
  }
}

// sum_k softmax_k(e) * dk.  exp(t) is the hardware exp2 of t*log2 e on t = e - max <= 0; the nine weights share one
// reciprocal of their sum; HALF: each weight is rounded to half before its product (torch.softmax keeps a half mask's
// dtype, the product with the float disparity promotes).  The products are summed in tap order, in float.
template <bool HALF>
__device__ __forceinline__ float cvx_combine(const float (&e)[9], const float (&dk)[9]) {
  float mx = e[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) mx = fmaxf(mx, e[k]);
  float ex[9];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    ex[k] = __builtin_amdgcn_exp2f((e[k] - mx) * 1.4426950408889634f);
    s += ex[k];
  }
  const float inv = 1.f / s;
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float w = ex[k] * inv;
    if (HALF) w = (float)(_Float16)w;
    r += w * dk[k];
  }
  return r;
}

}  // namespace dba
