// The per-pair body of frame_distance_kernel (src/droid_kernels.cu:562-702), shared by csrc/geom.hip
// (dba_frame_distance) and csrc/proximity.hip (dba_frame_distance_bidir, dba_proximity_edges) so that every route
// computes the same float operations in the same order: the same pixel stride over 256 lanes, the same wave_sum
// and the same order of the four per-wave partials.  Both files are built with the same flags.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "reproj.h"

namespace dba {

__device__ __forceinline__ void act_point(const Rot3 &R, const float *t, float X0, float X1, float d,
                                          float &x, float &y, float &z) {
  x = fmaf(d, t[0], fmaf(R.r[0], X0, fmaf(R.r[1], X1, R.r[2])));
  y = fmaf(d, t[1], fmaf(R.r[3], X0, fmaf(R.r[4], X1, R.r[5])));
  z = fmaf(d, t[2], fmaf(R.r[6], X0, fmaf(R.r[7], X1, R.r[8])));
}

// Lane `tid` of a 256-lane group (4 waves, stride 256) accumulates pixels tid, tid+256, ... of frame ix seen from jx, reduces
// its wave and leaves the wave's three partials in red[0..2][tid >> 6].  The caller synchronises the workgroup and
// calls frame_distance_finish(red) in one lane.
__device__ __forceinline__ void frame_distance_partials(const float *__restrict__ poses, const float *__restrict__ disps,
                                                        const float *__restrict__ intr, int ix, int jx, int HW,
                                                        int wd, float beta, int tid, int stride,
                                                        float (*red)[4]) {
  float tij[3], qij[4];
  rel_pose(poses + 7 * ix, poses + 7 * jx, tij, qij);
  const Rot3 R = quat_to_rot(qij);
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  float accum = 0.f, valid = 0.f, total = 0.f;
  for (int k = tid; k < HW; k += stride) {
    const float u = (float)(k % wd), v = (float)(k / wd);
    const float X0 = (u - cx) / fx, X1 = (v - cy) / fy;
    const float d = disps[(size_t)ix * HW + k];
    float x, y, z;
    act_point(R, tij, X0, X1, d, x, y, z);
    float du = fx * (x / z) + cx - u, dv = fy * (y / z) + cy - v;
    float r = sqrtf(du * du + dv * dv);
    total += beta;
    if (z > 0.25f) { accum += beta * r; valid += beta; }
    // translation-only flow (:662-680)
    x = X0 + d * tij[0];
    y = X1 + d * tij[1];
    z = 1.0f + d * tij[2];
    du = fx * (x / z) + cx - u;
    dv = fy * (y / z) + cy - v;
    r = sqrtf(du * du + dv * dv);
    total += (1.f - beta);
    if (z > 0.25f) { accum += (1.f - beta) * r; valid += (1.f - beta); }
  }
  const int lane = tid & 63, wv = tid >> 6;
  const float a = wave_sum(accum), vv = wave_sum(valid), tt = wave_sum(total);
  if (lane == 0) { red[0][wv] = a; red[1][wv] = vv; red[2][wv] = tt; }
}

__device__ __forceinline__ float frame_distance_finish(const float (*red)[4]) {
  const float A = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const float V = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const float T = red[2][0] + red[2][1] + red[2][2] + red[2][3];
  return ((double)V / ((double)T + 1e-8) < 0.75) ? 1000.0f : A / V;  // :700
}

}  // namespace dba
