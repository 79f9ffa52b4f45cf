// The map export (include/dba_hip.h "map export"), gfx950:
//
//   dba_archive_frames  <- the five or six statements that archive a marginalised keyframe (dbaf/depth_video.py:337-343,
//                          :379-385), for frames [i0, i1) in ONE launch
//   dba_map_plan        <- the per-frame statements of save_vis_easy (dbaf/dbaf.py:71-89, :114-126): disps.mean(dim=[1,2]),
//                          SE3(poses).inv() as data and as matrix, torch.median, thresh, depth_filter and the mask
//   dba_map_payload     <- iproj on the inverse poses and the boolean-mask indexing of points and colours (:96-97), for
//                          the surviving pixels only
//
// A workgroup is 256 lanes and owns ONE archived frame; it walks the frame's pixels in chunks of 256, in row-major order.
//   mean       lane l adds pixels l, l + 256, ... in that order; wave_sum (common.h) folds the 64 lanes of each wave, the
//              four wave totals are added in wave order, the sum is divided by HW (IEEE).  One fixed order: the same bits
//              in every run.
//   median     the LAST workgroup of the frames launch to finish (an integer ticket) selects sorted[(count - 1) / 2] by a
//              32-step radix selection over order-preserving integer keys: the value torch.median returns, ties and even
//              counts included.  A NaN among the means gives NaN, as torch does.
//   mask       (count >= min_count) & (disp > 0.5f * mean); survivors are counted with ballots, one integer per frame.
//   scan       the last workgroup of the launch that wrote the frame counts turns them into offsets[count + 1] (int64).
//              A frame is a workgroup, so offsets are the per-workgroup bases too.
//   payload    a workgroup re-reads its frame's mask; a survivor's place is its frame's offset + the survivors of the
//              chunks and waves before it + the survivors of lower lanes of its wave (ballot and popcount): frame-major,
//              row-major within a frame, the same in every run.  No atomics on floats anywhere; the only atomics are the
//              two integer tickets.
// filtered: frames launch (+ median), mask launch (+ scan), payload.  raw: the frames launch takes the mask and the scan
// along (the mask needs only the frame's own mean) and NO depth-filter code runs; then the payload.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "geom_pixel.h"
#include "pose_inv.h"

namespace dba {

constexpr int MX_THREADS = 256;
constexpr int MX_WAVES = MX_THREADS / WAVE;
// torch's division of a device tensor by a host scalar multiplies by the scalar's float32 reciprocal
constexpr float MX_INV255 = 1.0f / 255.0f;

struct ArchiveArgs {
  const double *tstamp;
  const float *disps, *poses, *disps_up;
  const uint8_t *images;
  double *tstamp_save;
  float *disps_save, *poses_save, *disps_up_save, *images_save;
  int i0, row, ht, wd, H, W;
  long long up_elems;
};

// grid (ceil(max(HW, 7, up_elems) / 256), i1 - i0): lane e of frame f copies element e of every row that has one
__global__ __launch_bounds__(MX_THREADS) void archive_frames_kernel(ArchiveArgs a) {
  const size_t src = (size_t)a.i0 + blockIdx.y, dst = (size_t)a.row + blockIdx.y;
  const long long e = (long long)blockIdx.x * MX_THREADS + threadIdx.x;
  const int HW = a.ht * a.wd;
  if (e == 0) a.tstamp_save[dst] = a.tstamp[src];
  if (e < 7) a.poses_save[dst * 7 + e] = a.poses[src * 7 + e];
  if (e < HW) {
    a.disps_save[dst * HW + e] = a.disps[src * HW + e];
    // images[i, [2,1,0], ::8, ::8].permute(1,2,0) / 255.0
    const int y = (int)e / a.wd, x = (int)e - y * a.wd;
    const size_t plane = (size_t)a.H * a.W;
    const uint8_t *px = a.images + src * 3 * plane + (size_t)(8 * y) * a.W + 8 * x;
    float *o = a.images_save + (dst * HW + e) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = __fmul_rn((float)px[(size_t)(2 - c) * plane], MX_INV255);
  }
  if (a.disps_up && e < a.up_elems) a.disps_up_save[dst * a.up_elems + e] = a.disps_up[src * a.up_elems + e];
}

struct PlanArgs {
  const float *poses, *disps, *intr;  // the save buffers [rows, ...] and the intrinsics [4]
  int count, rows, ht, wd;
  float min_count;                    // <= 0: raw
  float *means, *inv_poses, *cameras; // [count], [count, 7], [count, 16]
  float *scalars;                     // [0] median, [1] thresh
  float *counts;                      // [count, HW], filtered only
  uint8_t *mask;                      // [count, HW]
  int *frame_counts;                  // [count]
  long long *offsets;                 // [count + 1]
  int *tickets;                       // [2], zero on entry
};

// true in every lane of the workgroup that takes the last of `nblocks` tickets; what the other workgroups wrote before
// their tickets is visible to it
__device__ __forceinline__ bool mx_last_block(int *ticket, int nblocks) {
  __shared__ int s_last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1;
  __syncthreads();
  const bool last = s_last != 0;
  if (last) __threadfence();
  return last;
}

__device__ __forceinline__ unsigned mx_key(float x) {  // unsigned order == float order
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mx_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// sorted(m)[(n - 1) / 2] in every lane; n >= 1; one workgroup
__device__ float mx_lower_median(const float *m, int n) {
  __shared__ int s_c0, s_nan;
  const int tid = threadIdx.x;
  if (tid == 0) s_nan = 0;
  __syncthreads();
  unsigned prefix = 0;
  int k = (n - 1) / 2;
  for (int bit = 31; bit >= 0; bit--) {
    if (tid == 0) s_c0 = 0;
    __syncthreads();
    const unsigned himask = bit == 31 ? 0u : ~0u << (bit + 1);
    int c = 0;
    bool nan = false;
    for (int i = tid; i < n; i += MX_THREADS) {
      const float x = m[i];
      const unsigned key = mx_key(x);
      nan = nan || x != x;
      if ((key & himask) == prefix && !((key >> bit) & 1u)) c++;
    }
    if (c) atomicAdd(&s_c0, c);
    if (nan) s_nan = 1;
    __syncthreads();
    const int c0 = s_c0;
    if (k >= c0) {
      k -= c0;
      prefix |= 1u << bit;
    }
    __syncthreads();
  }
  return s_nan ? __uint_as_float(0x7fc00000u) : mx_unkey(prefix);
}

// offsets[i] = fc[0] + ... + fc[i-1] for i in [0, n]; one workgroup, lane l owns the l-th run of ceil(n / 256) frames
__device__ void mx_scan(const int *fc, int n, long long *offsets) {
  __shared__ long long s_part[MX_THREADS];
  const int tid = threadIdx.x;
  const int seg = (n + MX_THREADS - 1) / MX_THREADS;
  const int lo = min(n, tid * seg), hi = min(n, lo + seg);
  long long s = 0;
  for (int i = lo; i < hi; i++) s += fc[i];
  s_part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < MX_THREADS; t++) {
      const long long v = s_part[t];
      s_part[t] = run;
      run += v;
    }
    offsets[n] = run;
  }
  __syncthreads();
  long long run = s_part[tid];
  for (int i = lo; i < hi; i++) {
    offsets[i] = run;
    run += fc[i];
  }
}

// the mask of frame b and its survivor count (frame_counts[b]); FILTER: the depth-filter count of every pixel first
template <bool FILTER>
__device__ __forceinline__ void mx_mask_frame(const PlanArgs &a, int b, float mean, float thresh) {
  __shared__ int s_cnt[MX_WAVES];
  const int tid = threadIdx.x, HW = a.ht * a.wd;
  const float half = __fmul_rn(0.5f, mean);
  int wave_cnt = 0;
  for (int k0 = 0; k0 < HW; k0 += MX_THREADS) {
    const int k = k0 + tid;
    bool m = false;
    if (k < HW) {
      const size_t at = (size_t)b * HW + k;
      bool ok = true;
      if (FILTER) {
        const float c = depth_filter_pixel(a.poses, a.disps, a.intr, b, thresh, a.rows, a.ht, a.wd, k);
        a.counts[at] = c;
        ok = c >= a.min_count;
      }
      m = ok && a.disps[at] > half;
      a.mask[at] = m ? 1 : 0;
    }
    wave_cnt += __popcll(__ballot(m));
  }
  if ((tid & (WAVE - 1)) == 0) s_cnt[tid >> 6] = wave_cnt;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < MX_WAVES; w++) s += s_cnt[w];
    a.frame_counts[b] = s;
  }
}

// grid (count): mean, inverse pose and camera matrix of frame b; RAW: its mask too.  Last workgroup: median and thresh;
// RAW: the scan.
template <bool RAW>
__global__ __launch_bounds__(MX_THREADS) void map_frames_kernel(PlanArgs a) {
  __shared__ float s_part[MX_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, HW = a.ht * a.wd;
  const float *d = a.disps + (size_t)b * HW;
  float acc = 0.f;
  for (int k = tid; k < HW; k += MX_THREADS) acc = __fadd_rn(acc, d[k]);
  const float w = wave_sum(acc);
  if ((tid & (WAVE - 1)) == 0) s_part[tid >> 6] = w;
  __syncthreads();
  float s = s_part[0];
#pragma unroll
  for (int q = 1; q < MX_WAVES; q++) s = __fadd_rn(s, s_part[q]);
  const float mean = __fdiv_rn(s, (float)HW);
  if (tid == 0) {
    a.means[b] = mean;
    // SE3(pose).inv() and its matrix: the columns of R are _qrot(qi, e_k), the fourth column is ti (keyframe.hip)
    float ti[3], qi[4];
    kf_inv(a.poses + 7 * (size_t)b, ti, qi);
    float *P = a.inv_poses + 7 * (size_t)b, *M = a.cameras + 16 * (size_t)b;
    P[0] = ti[0]; P[1] = ti[1]; P[2] = ti[2];
    P[3] = qi[0]; P[4] = qi[1]; P[5] = qi[2]; P[6] = qi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float e[3] = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f};
      float col[3];
      kf_qrot(qi, e, col);
      M[0 + k] = col[0]; M[4 + k] = col[1]; M[8 + k] = col[2];
    }
    M[3] = ti[0]; M[7] = ti[1]; M[11] = ti[2];
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
  }
  if (RAW) mx_mask_frame<false>(a, b, mean, 0.f);
  if (!mx_last_block(a.tickets + 0, a.count)) return;
  const float med = mx_lower_median(a.means, a.count);
  if (tid == 0) {
    a.scalars[0] = med;
    // 0.4 * ones / 4.0 * (1.0 / median) (dbaf.py:77); raw: 0.4 * ones (:120), which no mask depends on
    a.scalars[1] = RAW ? 0.4f : __fmul_rn(__fdiv_rn(__fmul_rn(0.4f, 1.0f), 4.0f), __fdiv_rn(1.0f, med));
  }
  if (RAW) mx_scan(a.frame_counts, a.count, a.offsets);
}

// grid (count), filtered only: depth-filter counts and mask of frame b.  Last workgroup: the scan.
__global__ __launch_bounds__(MX_THREADS) void map_mask_kernel(PlanArgs a) {
  const int b = blockIdx.x;
  mx_mask_frame<true>(a, b, a.means[b], a.scalars[1]);
  if (!mx_last_block(a.tickets + 1, a.count)) return;
  mx_scan(a.frame_counts, a.count, a.offsets);
}

struct PayloadArgs {
  const float *inv_poses, *disps, *intr, *images;
  const uint8_t *mask;
  const long long *offsets;
  int count, ht, wd;
  long long total;
  float *pts, *clr;
};

// grid (count): the survivors of frame b, in pixel order, to rows offsets[b] ... of pts and clr
__global__ __launch_bounds__(MX_THREADS) void map_payload_kernel(PayloadArgs a) {
  __shared__ int s_wave[MX_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, HW = a.ht * a.wd;
  const int lane = tid & (WAVE - 1), w = tid >> 6;
  long long base = a.offsets[b];
  for (int k0 = 0; k0 < HW; k0 += MX_THREADS) {
    const int k = k0 + tid;
    const size_t at = (size_t)b * HW + (k < HW ? k : 0);
    const bool m = k < HW && a.mask[at] != 0;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) s_wave[w] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < MX_WAVES; q++) {
      const int c = s_wave[q];
      before += q < w ? c : 0;
      all += c;
    }
    if (m) {
      const long long row = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (row < a.total) {  // (always, when mask and offsets are one plan's)
        float x, y, z;
        iproj_pixel(a.inv_poses, a.disps, a.intr, b, k, HW, a.wd, x, y, z);
        float *p = a.pts + row * 3, *c = a.clr + row * 3;
        const float *rgb = a.images + at * 3;
        p[0] = x; p[1] = y; p[2] = z;
        c[0] = rgb[0]; c[1] = rgb[1]; c[2] = rgb[2];
      }
    }
    base += all;
    __syncthreads();
  }
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_archive_frames(const double *tstamp, const float *disps, const float *poses, const float *disps_up,
                       const uint8_t *images, double *tstamp_save, float *disps_save, float *poses_save,
                       float *disps_up_save, float *images_save, int n_src, int n_dst, int i0, int i1, int row, int ht,
                       int wd, int img_h, int img_w, int64_t up_elems, dba_stream_t stream) {
  if (n_src < 0 || n_dst < 0 || i0 < 0 || i1 > n_src || row < 0) return DBA_ERR_ARG;
  if (ht < 1 || wd < 1 || img_h < 1 || img_w < 1 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if ((img_h + 7) / 8 != ht || (img_w + 7) / 8 != wd) return DBA_ERR_ARG;  // the shape of [::8, ::8]
  if ((disps_up == nullptr) != (disps_up_save == nullptr) || (disps_up && up_elems < 1) || up_elems < 0) return DBA_ERR_ARG;
  if (i1 <= i0) return DBA_OK;
  const int n = i1 - i0;
  if (n > 65535 || (int64_t)row + n > n_dst) return DBA_ERR_ARG;
  if (!tstamp || !disps || !poses || !images || !tstamp_save || !disps_save || !poses_save || !images_save) return DBA_ERR_ARG;
  int64_t elems = (int64_t)ht * wd;
  if (elems < 7) elems = 7;
  if (disps_up && up_elems > elems) elems = up_elems;
  const int64_t wgs = (elems + MX_THREADS - 1) / MX_THREADS;
  if (wgs > INT32_MAX) return DBA_ERR_ARG;
  ArchiveArgs a{tstamp, disps, poses, disps_up, images, tstamp_save, disps_save, poses_save, disps_up_save, images_save,
                i0, row, ht, wd, img_h, img_w, disps_up ? up_elems : 0};
  hipLaunchKernelGGL(archive_frames_kernel, dim3((unsigned)wgs, (unsigned)n), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_map_plan(const float *poses_save, const float *disps_save, const float *intrinsics, int count, int rows, int ht,
                 int wd, int min_count, float *means, float *inv_poses, float *cameras, float *scalars, float *counts,
                 uint8_t *mask, int *frame_counts, int64_t *offsets, int *tickets, int *launches, dba_stream_t stream) {
  if (launches) *launches = 0;
  if (count < 0 || rows < 0 || count > rows || ht < 1 || wd < 1 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if (count == 0) return DBA_OK;
  const bool raw = min_count <= 0;
  if (!poses_save || !disps_save || !intrinsics || !means || !inv_poses || !cameras || !scalars || !mask || !frame_counts ||
      !offsets || !tickets || (!raw && !counts))
    return DBA_ERR_ARG;
  PlanArgs a{poses_save, disps_save, intrinsics, count, rows, ht, wd, (float)min_count, means, inv_poses, cameras, scalars,
             counts, mask, frame_counts, reinterpret_cast<long long *>(offsets), tickets};
  if (raw) {
    hipLaunchKernelGGL(map_frames_kernel<true>, dim3(count), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
    DBA_LAUNCH_CHECK();
    if (launches) *launches = 1;
    return DBA_OK;
  }
  hipLaunchKernelGGL(map_frames_kernel<false>, dim3(count), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  if (launches) *launches = 1;
  hipLaunchKernelGGL(map_mask_kernel, dim3(count), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  if (launches) *launches = 2;
  return DBA_OK;
}

int dba_map_payload(const float *inv_poses, const float *disps_save, const float *intrinsics, const float *images_save,
                    const uint8_t *mask, const int64_t *offsets, int count, int rows, int ht, int wd, int64_t total,
                    float *pts, float *clr, dba_stream_t stream) {
  if (count < 0 || rows < 0 || count > rows || ht < 1 || wd < 1 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if (total < 0 || total > (int64_t)count * ht * wd) return DBA_ERR_ARG;
  if (count == 0 || total == 0) return DBA_OK;
  if (!inv_poses || !disps_save || !intrinsics || !images_save || !mask || !offsets || !pts || !clr) return DBA_ERR_ARG;
  PayloadArgs a{inv_poses, disps_save, intrinsics, images_save, mask, reinterpret_cast<const long long *>(offsets),
                count, ht, wd, total, pts, clr};
  hipLaunchKernelGGL(map_payload_kernel, dim3(count), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
