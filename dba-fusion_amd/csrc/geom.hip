// Geometry kernels of the hot path's neighbours, gfx950:
//   dba_reproject       <- pops.projective_transform (dbaf/geom/projective_ops.py:96-125), the ~15 small
//                          torch/lietorch kernels issued by DepthVideo.reproject on every update
//   dba_frame_distance  <- frame_distance_kernel (src/droid_kernels.cu:562-702)
//   dba_projmap         <- projmap_kernel        (src/droid_kernels.cu:471-560)
//   dba_iproj           <- iproj_kernel          (src/droid_kernels.cu:824-895)
//   dba_depth_filter    <- depth_filter_kernel   (src/droid_kernels.cu:706-820)
// All are one pass over [N or B, ht*wd] with 4-20 bytes per pixel: HBM/latency trivial, so the only
// design rule is "one launch, coalesced, enough workgroups" (grid = pixels x edges).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "frame_distance.h"
#include "geom_pixel.h"
#include "reproj.h"

namespace dba {

__global__ __launch_bounds__(256) void reproject_kernel(const float *__restrict__ poses,
                                                        const float *__restrict__ disps,
                                                        const float *__restrict__ intr_b4,
                                                        const int64_t *__restrict__ ii,
                                                        const int64_t *__restrict__ jj, int HW, int wd,
                                                        float2 *__restrict__ coords, float *__restrict__ valid) {
  const int n = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= HW) return;
  const int ix = (int)ii[n], jx = (int)jj[n];
  // (reproj.h: the arithmetic the lookup kernels repeat in their prologue when they take the reprojection along --
  // dba_corr_lookup_reproject_sheared -- so that the fused call equals this kernel + the lookup bit for bit)
  const EdgeGeom G = edge_geom(poses, intr_b4, ix, jx);  // stereo edges: (-0.1,0,0), identity (projective_ops.py:105)
  const float u = (float)(k % wd), v = (float)(k / wd);
  float ok;
  coords[(size_t)n * HW + k] = reproject_pixel(G, u, v, disps[(size_t)ix * HW + k], ok);
  valid[(size_t)n * HW + k] = ok;  // X0.z == 1 > MIN_DEPTH always (:112)
}

__global__ __launch_bounds__(256) void frame_distance_kernel(const float *__restrict__ poses,
                                                             const float *__restrict__ disps,
                                                             const float *__restrict__ intr,
                                                             const int64_t *__restrict__ ii,
                                                             const int64_t *__restrict__ jj, int HW, int wd,
                                                             float beta, float *__restrict__ dist) {
  __shared__ float red[3][4];
  const int n = blockIdx.x;
  frame_distance_partials(poses, disps, intr, (int)ii[n], (int)jj[n], HW, wd, beta, threadIdx.x, blockDim.x, red);
  __syncthreads();
  if (threadIdx.x == 0) dist[n] = frame_distance_finish(red);
}

__global__ __launch_bounds__(256) void projmap_kernel(const float *__restrict__ poses,
                                                      const float *__restrict__ disps,
                                                      const float *__restrict__ intr,
                                                      const int64_t *__restrict__ ii,
                                                      const int64_t *__restrict__ jj, int HW, int wd,
                                                      float *__restrict__ coords, float *__restrict__ valid) {
  const int n = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= HW) return;
  const int ix = (int)ii[n], jx = (int)jj[n];
  float tij[3], qij[4];
  rel_pose(poses + 7 * ix, poses + 7 * jx, tij, qij);
  const Rot3 R = quat_to_rot(qij);
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float u = (float)(k % wd), v = (float)(k / wd);
  float x, y, z;
  act_point(R, tij, (u - cx) / fx, (v - cy) / fy, disps[(size_t)ix * HW + k], x, y, z);
  float *c = coords + ((size_t)n * HW + k) * 3;
  float ou = u, ov = v;
  if (z > 0.01f) { ou = fx * (x / z) + cx; ov = fy * (y / z) + cy; }
  c[0] = ou;
  c[1] = ov;
  c[2] = 0.f;  // the reference allocates 3 channels and writes 2 (:549-554, :1718)
  valid[(size_t)n * HW + k] = (z > 0.25f) ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void iproj_kernel(const float *__restrict__ poses,
                                                    const float *__restrict__ disps,
                                                    const float *__restrict__ intr, int HW, int wd,
                                                    float *__restrict__ points) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= HW) return;
  float x, y, z;
  iproj_pixel(poses, disps, intr, b, k, HW, wd, x, y, z);
  float *p = points + ((size_t)b * HW + k) * 3;
  p[0] = x;
  p[1] = y;
  p[2] = z;
}

__global__ __launch_bounds__(256) void depth_filter_kernel(const float *__restrict__ poses,
                                                           const float *__restrict__ disps,
                                                           const float *__restrict__ intr,
                                                           const int64_t *__restrict__ inds,
                                                           const float *__restrict__ thresh, int nbuf, int ht,
                                                           int wd, float *__restrict__ counter) {
  // one lane per (keyframe, pixel)
  const int b = blockIdx.y;
  const int HW = ht * wd;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= HW) return;
  const float count = depth_filter_pixel(poses, disps, intr, (int)inds[b], thresh[b], nbuf, ht, wd, k);
  counter[(size_t)b * HW + k] += count;
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_reproject(const float *poses, const float *disps, const float *intrinsics_b4, const int64_t *ii,
                  const int64_t *jj, int N, int ht, int wd, float *coords, float *valid, dba_stream_t stream) {
  if (N < 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (N == 0) return DBA_OK;
  const int HW = ht * wd;
  hipLaunchKernelGGL(reproject_kernel, dim3((HW + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, poses, disps,
                     intrinsics_b4, ii, jj, HW, wd, reinterpret_cast<float2 *>(coords), valid);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_frame_distance(const float *poses, const float *disps, const float *intrinsics, const int64_t *ii,
                       const int64_t *jj, int N, int ht, int wd, float beta, float *dist, dba_stream_t stream) {
  if (N < 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (N == 0) return DBA_OK;
  hipLaunchKernelGGL(frame_distance_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, poses, disps, intrinsics,
                     ii, jj, ht * wd, wd, beta, dist);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_projmap(const float *poses, const float *disps, const float *intrinsics, const int64_t *ii,
                const int64_t *jj, int N, int ht, int wd, float *coords, float *valid, dba_stream_t stream) {
  if (N < 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (N == 0) return DBA_OK;
  const int HW = ht * wd;
  hipLaunchKernelGGL(projmap_kernel, dim3((HW + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, poses, disps,
                     intrinsics, ii, jj, HW, wd, coords, valid);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_iproj(const float *poses, const float *disps, const float *intrinsics, int nm, int ht, int wd,
              float *points, dba_stream_t stream) {
  if (nm < 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (nm == 0) return DBA_OK;
  const int HW = ht * wd;
  hipLaunchKernelGGL(iproj_kernel, dim3((HW + 255) / 256, nm), dim3(256), 0, (hipStream_t)stream, poses, disps,
                     intrinsics, HW, wd, points);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_depth_filter(const float *poses, const float *disps, const float *intrinsics, const int64_t *inds,
                     const float *thresh, int num, int nbuf, int ht, int wd, float *counter,
                     dba_stream_t stream) {
  if (num < 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (num == 0) return DBA_OK;
  const int HW = ht * wd;
  hipLaunchKernelGGL(depth_filter_kernel, dim3((HW + 255) / 256, num), dim3(256), 0, (hipStream_t)stream, poses,
                     disps, intrinsics, inds, thresh, nbuf, ht, wd, counter);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
