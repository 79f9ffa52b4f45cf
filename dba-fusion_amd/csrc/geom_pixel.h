// The per-pixel bodies of iproj_kernel and depth_filter_kernel (geom.hip), shared with the map export's launches
// (map_export.hip), which must give the same bits.  Both files are built with the same flags, and each body is one
// function from the pixel index to its result, so the compiler sees the same expressions in either place.
//   iproj_pixel         <- iproj_kernel        (src/droid_kernels.cu:824-895)
//   depth_filter_pixel  <- depth_filter_kernel (src/droid_kernels.cu:706-820)
#pragma once
#include "common.h"
#include "frame_distance.h"

namespace dba {

// the point of pixel k of frame b: (R X + d t) / d with the frame's own (t, q) row
__device__ __forceinline__ void iproj_pixel(const float *__restrict__ poses, const float *__restrict__ disps,
                                            const float *__restrict__ intr, int b, int k, int HW, int wd, float &px,
                                            float &py, float &pz) {
  const float *t = poses + 7 * b;
  const Rot3 R = quat_to_rot(poses + 7 * b + 3);
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float u = (float)(k % wd), v = (float)(k / wd);
  const float d = disps[(size_t)b * HW + k];
  float x, y, z;
  act_point(R, t, (u - cx) / fx, (v - cy) / fy, d, x, y, z);
  px = x / d;
  py = y / d;
  pz = z / d;
}

// the number of neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 inside [0, nbuf) that confirm the depth of pixel k of
// frame ix within t; the six neighbours are visited in order so no atomics are needed
__device__ __forceinline__ float depth_filter_pixel(const float *__restrict__ poses, const float *__restrict__ disps,
                                                    const float *__restrict__ intr, int ix, float t, int nbuf, int ht,
                                                    int wd, int k) {
  const int HW = ht * wd;
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float u = (float)(k % wd), v = (float)(k / wd);
  const float X0 = (u - cx) / fx, X1 = (v - cy) / fy;
  const float di = disps[(size_t)ix * HW + k];
  float count = 0.f;
  for (int neigh = 0; neigh < 6; neigh++) {
    const int jx = (neigh < 3) ? ix - neigh - 1 : ix + neigh;  // :740
    if (jx < 0 || jx >= nbuf) continue;
    float tij[3], qij[4];
    rel_pose(poses + 7 * ix, poses + 7 * jx, tij, qij);
    const Rot3 R = quat_to_rot(qij);
    float x, y, z;
    act_point(R, tij, X0, X1, di, x, y, z);
    const float uj = fx * (x / z) + cx, vj = fy * (y / z) + cy;
    const float dj = di / z;
    const int u0 = (int)floorf(uj), v0 = (int)floorf(vj);
    if (u0 >= 0 && v0 >= 0 && u0 < wd - 1 && v0 < ht - 1) {
      const float *dp = disps + (size_t)jx * HW + (size_t)v0 * wd + u0;
      const double idj = 1.0 / (double)dj;  // abs(1.0/dj - 1.0/d00) is double arithmetic (:813-817)
      const double tt = (double)t;
      if (fabs(idj - 1.0 / (double)dp[0]) < tt) count += 1.f;
      else if (fabs(idj - 1.0 / (double)dp[1]) < tt) count += 1.f;
      else if (fabs(idj - 1.0 / (double)dp[wd]) < tt) count += 1.f;
      else if (fabs(idj - 1.0 / (double)dp[wd + 1]) < tt) count += 1.f;
    }
  }
  return count;
}

}  // namespace dba
