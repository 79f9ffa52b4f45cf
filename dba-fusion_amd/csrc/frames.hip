// How a frame enters and leaves the window (include/dba_hip.h "frame admission"), gfx950:
//
//   dba_frame_append     <- DepthVideo.append / __item_setter (dbaf/depth_video.py:129-159, :183-185) with the sensor-depth
//                           statements of :146-147, and optionally the seed of dbaf/dbaf_frontend.py:247-248
//   dba_frame_seed_next  <- poses[t1] = poses[t1-1], disps[t1] = disps[t1-k:t1].mean(), dirty[ii.min():t1] = True
//                           (dbaf_frontend.py:372-375, :841-849)
//   dba_world_poses      <- SE3(poses[:n]).inv().matrix().cpu() (:554, :608)
//   dba_set_world_poses  <- the write-back loops of :224-228, :424-432, :565-570, :809-814
//
// frame_append_kernel: the grid is the row mover's job table (row_jobs.h: image, fmap, net, inp; pure streaming, the
// widest vector width each row's base and size allow, four loads in flight per lane, no LDS), then the workgroups of the
// maps (a lane owns one pixel of disps_sens[row] and disps[row]: the depth gather, the reciprocal, the disparity and the
// seed are all decided by the one lane that writes the pixel, so nothing orders two workgroups), then one workgroup for the
// scalars (tstamp, pose, intrinsics; host values travel in the kernel's arguments).
//
// seed_next_kernel: one workgroup of 1024 lanes.  THE ORDER OF THE MEAN over the n = mean_rows * ht * wd entries
// x[0 .. n) of disps[t1 - mean_rows : t1]:
//   1. lane l holds x[l], x[l + 1024], ...: c = ceil(n / 1024) values, those past n being +0.  It adds them pairwise as a
//      binary counter does: value i goes to level 0; two values of one level are added (the older on the left) and move
//      up.  The levels that remain (the set bits of c) are then added from the lowest up, the higher level on the left.
//   2. the 64 lanes of a wave: wave_sum (common.h), six steps.
//   3. n > 64 only: the 16 wave totals as a balanced tree, ((w0 + w1) + (w2 + w3)) + ..., four steps.  n <= 64: the total
//      is wave 0's.
//   4. one IEEE division by float(n).
// The longest chain of additions is depth(c) + 6 (+ 4), depth(c) <= ceil(log2 c) + 1 (tests/frames_model.py computes it).
// No atomics: the same bits on every run.
//
// world_poses_kernel / set_world_poses_kernel: one pinned, host-coherent block per (device, stream), never freed, holds
// the matrices going out, the matrices coming in and one completion word for each direction.  The lanes that touched the
// block fence, the workgroup meets, lane 0 releases the word at system scope (the hand-over of keyframe.hip).
// dba_world_poses waits for its word; dba_set_world_poses waits, before it overwrites the staging area, for the word of
// the launch that last read it.
// Built with the flags of keyframe.hip: world_poses calls the routine of pose_inv.h that dba_keyframe_check calls (not
// inlined, compiled from the same text with the same flags in both files), which gives row t1 - 1 the bits of that call's
// matrix.  Nothing else here depends on them: the append's division and selects, the mean's additions and the
// scaling's multiplication have no product feeding a sum, and set_world_poses' float64 statements (tests/frames_model.py
// says them again) are rounded to float32 at the end.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>

#include "common.h"
#include "pose_inv.h"
#include "row_jobs.h"

namespace dba {

constexpr int FR_JOBS = 4;  // image, fmap, net, inp
constexpr int FR_THREADS = MOVE_THREADS;
constexpr int SN_THREADS = 1024, SN_WAVES = SN_THREADS / 64, SN_LEVELS = 16, SN_LOADS = 4;
constexpr long long SN_MAX_ELEMS = 1ll << 24;  // float(n) exact; c <= 16384 < 2^SN_LEVELS - 1
constexpr int WP_THREADS = 256;
constexpr int SC_PER_WG = 1024;  // disps entries per scaling workgroup of set_world_poses

struct FrameAppendDev {
  RowTable<FR_JOBS> t;
  unsigned map_wg0, scalar_wg;  // the first workgroup of the maps; the workgroup of the scalars
  double *tstamp_dst;
  double tstamp;
  float *pose_dst, *intr_dst, *disp_dst, *sens_dst;
  const float *pose_src, *intr_src, *disp_src, *depth;
  int pose_mode, intr_mode, disp_mode, seed;
  int ht, wd;
  float pose[7], intr[4], disp_fill;
};

__global__ __launch_bounds__(FR_THREADS) void frame_append_kernel(FrameAppendDev a) {
  const unsigned bid = blockIdx.x;
  const int tid = threadIdx.x;
  if (bid < a.map_wg0) {
    run_row_jobs<FR_JOBS>(a.t);
    return;
  }
  if (bid == a.scalar_wg) {  // wave 0: the pose, wave 1: the intrinsics, wave 2: the timestamp
    if (tid < 7 && a.pose_mode != DBA_FR_SKIP) {
      float v;
      if (a.pose_mode == DBA_FR_DEVICE) {
        v = a.pose_src[tid];
      } else {
        v = a.pose[0];
#pragma unroll
        for (int k = 1; k < 7; k++)
          if (tid == k) v = a.pose[k];
      }
      a.pose_dst[tid] = v;
    } else if (tid >= 64 && tid < 68 && a.intr_mode != DBA_FR_SKIP) {
      const int e = tid - 64;
      float v;
      if (a.intr_mode == DBA_FR_DEVICE) {
        v = a.intr_src[e];
      } else {
        v = a.intr[0];
#pragma unroll
        for (int k = 1; k < 4; k++)
          if (e == k) v = a.intr[k];
      }
      a.intr_dst[e] = v;
    } else if (tid == 128) {
      *a.tstamp_dst = a.tstamp;
    }
    return;
  }
  // one pixel of the two maps
  const int p = (int)(bid - a.map_wg0) * FR_THREADS + tid;
  if (p >= a.ht * a.wd) return;
  float s = 0.f;
  if (a.depth) {
    const int y = p / a.wd, x = p - y * a.wd;
    const float d = a.depth[(long long)(8 * y + 3) * (8 * a.wd) + (8 * x + 3)];  // depth[3::8, 3::8]
    s = d > 0.f ? __fdiv_rn(1.0f, d) : d;                                         // torch.where(depth > 0, 1.0 / depth, depth)
    a.sens_dst[p] = s;
  } else if (a.seed) {
    s = a.sens_dst[p];
  }
  if (a.disp_mode != DBA_FR_SKIP || a.seed) {
    float v = a.disp_mode == DBA_FR_HOST ? a.disp_fill : a.disp_mode == DBA_FR_DEVICE ? a.disp_src[p] : a.disp_dst[p];
    if (a.seed && s > 0.f) v = s;  // torch.where(disps_sens[row] > 0, disps_sens[row], disps[row])
    a.disp_dst[p] = v;
  }
}

// step 1 of the mean's order: value number i of a lane enters the binary counter
__device__ __forceinline__ void sn_push(float (&lv)[SN_LEVELS], float v, int i) {
  bool carry = true;
#pragma unroll
  for (int j = 0; j < SN_LEVELS; j++) {
    if (carry) {
      if ((i >> j) & 1) {
        v = __fadd_rn(lv[j], v);
      } else {
        lv[j] = v;
        carry = false;
      }
    }
  }
}

__global__ __launch_bounds__(SN_THREADS) void seed_next_kernel(float *poses, float *disps, unsigned char *dirty, int HW,
                                                               int t1, int mean_rows, const long long *ii, long long n_ii) {
  __shared__ float part[SN_WAVES];
  __shared__ int lo_part[SN_WAVES];
  __shared__ float s_mean;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int n = mean_rows * HW;
  const float *src = disps + (long long)(t1 - mean_rows) * HW;
  const int c = (n + SN_THREADS - 1) / SN_THREADS;
  float lv[SN_LEVELS];
#pragma unroll
  for (int j = 0; j < SN_LEVELS; j++) lv[j] = 0.f;
  for (int i0 = 0; i0 < c; i0 += SN_LOADS) {
    float x[SN_LOADS];
#pragma unroll
    for (int u = 0; u < SN_LOADS; u++) {
      const int e = (i0 + u) * SN_THREADS + tid;
      x[u] = e < n ? src[e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SN_LOADS; u++)
      if (i0 + u < c) sn_push(lv, x[u], i0 + u);
  }
  float acc = 0.f;
  bool have = false;
#pragma unroll
  for (int j = 0; j < SN_LEVELS; j++)
    if ((c >> j) & 1) {
      acc = have ? __fadd_rn(lv[j], acc) : lv[j];
      have = true;
    }
  const float wsum = wave_sum(acc);
  // lo = min(ii) clamped to [0, t1]; clamping each entry first gives the same minimum
  int lo = ii ? t1 : 0;
  for (long long k = tid; k < n_ii; k += SN_THREADS) {
    const long long v = ii[k];
    const int cl = v < 0 ? 0 : (v > t1 ? t1 : (int)v);
    lo = min(lo, cl);
  }
  lo = wave_minmax<true>(lo);
  if ((tid & 63) == 0) {
    part[wave] = wsum;
    lo_part[wave] = lo;
  }
  __syncthreads();
  if (tid == 0) {
    float tot = part[0];
    if (n > 64) {
      float p[SN_WAVES];
#pragma unroll
      for (int w = 0; w < SN_WAVES; w++) p[w] = part[w];
#pragma unroll
      for (int st = 1; st < SN_WAVES; st *= 2)
#pragma unroll
        for (int q = 0; q < SN_WAVES; q += 2 * st) p[q] = __fadd_rn(p[q], p[q + st]);
      tot = p[0];
    }
    s_mean = __fdiv_rn(tot, (float)n);
  }
#pragma unroll
  for (int w = 0; w < SN_WAVES; w++) lo = min(lo, lo_part[w]);
  __syncthreads();
  const float m = s_mean;
  float *dst = disps + (long long)t1 * HW;
  for (int e = tid; e < HW; e += SN_THREADS) dst[e] = m;
  for (int r = lo + tid; r < t1; r += SN_THREADS) dirty[r] = 1;
  if (tid < 7) poses[7 * t1 + tid] = poses[7 * (t1 - 1) + tid];
}

// the completion of a launch that read or wrote the pinned block: every lane fences what it did, the workgroup meets,
// lane 0 releases the word to the host
__device__ __forceinline__ void fr_complete(int *flag, int seq) {
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(WP_THREADS) void world_poses_kernel(const float *__restrict__ poses, int n, float *out,
                                                                  int *flag, int seq) {
  for (int r = threadIdx.x; r < n; r += WP_THREADS) {
    // poses[r].inv().matrix() by the call keyframe_check_kernel makes (pose_inv.h: not inlined, so the same bits)
    const float *P = poses + 7 * r;
    const KfMat34 M = kf_inv_matrix(P[0], P[1], P[2], P[3], P[4], P[5], P[6]);
    float4 *o = reinterpret_cast<float4 *>(out + 16 * r);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = make_float4(M.m[4 * k], M.m[4 * k + 1], M.m[4 * k + 2], M.m[4 * k + 3]);
    o[3] = make_float4(0.f, 0.f, 0.f, 1.f);
  }
  fr_complete(flag, seq);
}

// workgroup 0: the poses, then the staging block's completion word; workgroups 1..: disps[i0 : i0 + n] *= inv_scale
__global__ __launch_bounds__(WP_THREADS) void set_world_poses_kernel(float *poses, float *disps, long long scaled, int i0,
                                                                      int n, const double *stage, float inv_scale,
                                                                      int *flag, int seq) {
  if (blockIdx.x > 0) {
    const long long e0 = (long long)(blockIdx.x - 1) * SC_PER_WG + threadIdx.x;
    float v[SC_PER_WG / WP_THREADS];
#pragma unroll
    for (int u = 0; u < SC_PER_WG / WP_THREADS; u++)
      if (e0 + u * WP_THREADS < scaled) v[u] = disps[e0 + u * WP_THREADS];
#pragma unroll
    for (int u = 0; u < SC_PER_WG / WP_THREADS; u++)
      if (e0 + u * WP_THREADS < scaled) disps[e0 + u * WP_THREADS] = __fmul_rn(v[u], inv_scale);
    return;
  }
  for (int r = threadIdx.x; r < n; r += WP_THREADS) {
    const double *T = stage + 16 * r;
    const double r00 = T[0], r01 = T[1], r02 = T[2], tx = T[3];
    const double r10 = T[4], r11 = T[5], r12 = T[6], ty = T[7];
    const double r20 = T[8], r21 = T[9], r22 = T[10], tz = T[11];
    // world-to-camera: M = R^T, ti = -(R^T t)
    const double m00 = r00, m01 = r10, m02 = r20, m10 = r01, m11 = r11, m12 = r21, m20 = r02, m21 = r12, m22 = r22;
    const double t0 = -((m00 * tx + m01 * ty) + m02 * tz);
    const double t1 = -((m10 * tx + m11 * ty) + m12 * tz);
    const double t2 = -((m20 * tx + m21 * ty) + m22 * tz);
    // the four-branch rule: the largest of (m00, m11, m22, trace), the first on a tie
    const double tr = (m00 + m11) + m22;
    int c = 0;
    double best = m00;
    if (m11 > best) { best = m11; c = 1; }
    if (m22 > best) { best = m22; c = 2; }
    if (tr > best) c = 3;
    double qx, qy, qz, qw;
    if (c == 0) {
      qx = (1.0 - tr) + 2.0 * m00; qy = m10 + m01; qz = m20 + m02; qw = m21 - m12;
    } else if (c == 1) {
      qy = (1.0 - tr) + 2.0 * m11; qz = m21 + m12; qx = m01 + m10; qw = m02 - m20;
    } else if (c == 2) {
      qz = (1.0 - tr) + 2.0 * m22; qx = m02 + m20; qy = m12 + m21; qw = m10 - m01;
    } else {
      qx = m21 - m12; qy = m02 - m20; qz = m10 - m01; qw = 1.0 + tr;
    }
    const double nrm = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
    float *P = poses + 7 * (long long)(i0 + r);
    P[0] = (float)t0; P[1] = (float)t1; P[2] = (float)t2;
    P[3] = (float)(qx / nrm); P[4] = (float)(qy / nrm); P[5] = (float)(qz / nrm); P[6] = (float)(qw / nrm);
  }
  fr_complete(flag, seq);
}

// ---- the pinned blocks: one per (device, stream), never freed -------------------------------------------------------------
namespace {
constexpr size_t FR_HEAD_BYTES = 128;  // [0] the completion word of world_poses, [1] of set_world_poses
constexpr size_t FR_OUT_BYTES = sizeof(float) * 16 * DBA_FR_MAX_ROWS;
constexpr size_t FR_STAGE_BYTES = sizeof(double) * 16 * DBA_FR_MAX_ROWS;

struct FrBlock {
  std::mutex mu;  // one call at a time
  int *words = nullptr;
  float *out = nullptr;
  double *stage = nullptr;
  hipStream_t stream = nullptr;
  int out_seq = 0, stage_seq = 0;  // the last sequence numbers handed out; 0: none yet
};
std::mutex g_fr_mu;
typedef std::map<std::pair<int, hipStream_t>, FrBlock *> FrStreamMap;
FrStreamMap &fr_blocks() {
  static FrStreamMap *m = new FrStreamMap;  // (never destroyed: calls may still arrive at exit)
  return *m;
}

int fr_block_for(hipStream_t stream, FrBlock **out) {
  int dev = 0;
  DBA_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_fr_mu);
  FrBlock *&b = fr_blocks()[std::make_pair(dev, stream)];
  if (!b) {
    void *p = nullptr;
    const size_t bytes = FR_HEAD_BYTES + FR_OUT_BYTES + FR_STAGE_BYTES;
    DBA_HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
    memset(p, 0, bytes);
    b = new FrBlock;
    b->words = static_cast<int *>(p);
    b->out = reinterpret_cast<float *>(static_cast<char *>(p) + FR_HEAD_BYTES);
    b->stage = reinterpret_cast<double *>(static_cast<char *>(p) + FR_HEAD_BYTES + FR_OUT_BYTES);
    b->stream = stream;
  }
  *out = b;
  return DBA_OK;
}

int fr_next_seq(int seq) { return seq + 1 <= 0 ? 1 : seq + 1; }  // never 0, the word of a fresh block

// spins until *flag shows seq (dba_keyframe_wait's loop); *spun: whether the first look missed
int fr_wait(const int *flag, int seq, hipStream_t stream, int *spun) {
  if (spun) *spun = 0;
  for (unsigned long spins = 1;; spins++) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return DBA_OK;
    if (spun) *spun = 1;
    if ((spins & 0x3fff) == 0) {
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return DBA_OK;
        set_last_error("frames: the stream drained without the completion word", hipErrorUnknown);
        return DBA_ERR_HIP;
      }
      if (q != hipErrorNotReady) {
        set_last_error("hipStreamQuery", q);
        return DBA_ERR_HIP;
      }
    }
    __builtin_ia32_pause();
  }
}
}  // namespace

}  // namespace dba

using namespace dba;

extern "C" {

int dba_frame_append(const dba_frame_item *it, dba_stream_t stream) {
  if (!it || it->rows <= 0 || it->row < 0 || it->row >= it->rows || it->ht <= 0 || it->wd <= 0) return DBA_ERR_ARG;
  if ((int64_t)it->ht * it->wd > INT32_MAX / 64) return DBA_ERR_ARG;
  if (!it->tstamp) return DBA_ERR_ARG;
  const int modes[3] = {it->pose_mode, it->intr_mode, it->disp_mode};
  for (int k = 0; k < 3; k++)
    if (modes[k] != DBA_FR_SKIP && modes[k] != DBA_FR_HOST && modes[k] != DBA_FR_DEVICE) return DBA_ERR_ARG;
  if (it->pose_mode != DBA_FR_SKIP && (!it->poses || (it->pose_mode == DBA_FR_DEVICE && !it->pose_dev))) return DBA_ERR_ARG;
  if (it->intr_mode != DBA_FR_SKIP && (!it->intrinsics || (it->intr_mode == DBA_FR_DEVICE && !it->intr_dev)))
    return DBA_ERR_ARG;
  if (it->disp_mode != DBA_FR_SKIP && (!it->disps || (it->disp_mode == DBA_FR_DEVICE && !it->disp_dev))) return DBA_ERR_ARG;
  if (it->depth && !it->disps_sens) return DBA_ERR_ARG;
  if (it->seed_disps && (!it->disps || !it->disps_sens)) return DBA_ERR_ARG;
  const int HW = it->ht * it->wd;
  FrameAppendDev a{};
  uint64_t wgs = 0;
  const struct { const void *src; void *dst; int64_t row_bytes; } dense[FR_JOBS] = {
      {it->image, it->images, (int64_t)3 * 64 * HW}, {it->fmap, it->fmaps, it->fmap_row_bytes},
      {it->net, it->nets, it->net_row_bytes}, {it->inp, it->inps, it->inp_row_bytes}};
  for (int k = 0; k < FR_JOBS; k++) {
    if (!dense[k].src) continue;
    dba_row_job j{};
    j.src = dense[k].src; j.dst = dense[k].dst; j.pos = nullptr; j.row_bytes = dense[k].row_bytes;
    j.count = 1; j.dst_row0 = it->row; j.src_rows = 1; j.dst_rows = it->rows;
    const int rc = check_row_job(j, true, POS_FORBIDDEN);
    if (rc < 0) return rc;
    if (rc == 0) continue;
    if (!push_job(a.t, wgs, (const char *)j.src, (char *)j.dst, nullptr, j.row_bytes, 1, j.dst_row0, 1)) return DBA_ERR_ARG;
  }
  a.map_wg0 = (unsigned)wgs;
  if (it->depth || it->seed_disps || it->disp_mode != DBA_FR_SKIP) wgs += (uint64_t)((HW + FR_THREADS - 1) / FR_THREADS);
  a.scalar_wg = (unsigned)wgs++;
  a.tstamp_dst = static_cast<double *>(it->tstamp) + it->row;
  a.tstamp = it->tstamp_value;
  a.pose_dst = it->poses ? static_cast<float *>(it->poses) + 7 * (int64_t)it->row : nullptr;
  a.intr_dst = it->intrinsics ? static_cast<float *>(it->intrinsics) + 4 * (int64_t)it->row : nullptr;
  a.disp_dst = it->disps ? static_cast<float *>(it->disps) + (int64_t)HW * it->row : nullptr;
  a.sens_dst = it->disps_sens ? static_cast<float *>(it->disps_sens) + (int64_t)HW * it->row : nullptr;
  a.pose_src = it->pose_dev; a.intr_src = it->intr_dev; a.disp_src = it->disp_dev; a.depth = it->depth;
  a.pose_mode = it->pose_mode; a.intr_mode = it->intr_mode; a.disp_mode = it->disp_mode; a.seed = it->seed_disps ? 1 : 0;
  a.ht = it->ht; a.wd = it->wd;
  memcpy(a.pose, it->pose, sizeof(a.pose));
  memcpy(a.intr, it->intr, sizeof(a.intr));
  a.disp_fill = it->disp_fill;
  hipLaunchKernelGGL(frame_append_kernel, dim3((unsigned)wgs), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_frame_seed_next(float *poses, float *disps, uint8_t *dirty, int rows, int dirty_rows, int ht, int wd, int t1,
                        int mean_rows, const int64_t *ii, int64_t n_ii, dba_stream_t stream) {
  if (!poses || !disps || !dirty || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if (mean_rows < 1 || mean_rows > t1 || t1 >= rows || t1 > dirty_rows) return DBA_ERR_ARG;
  if ((int64_t)ht * wd * mean_rows > SN_MAX_ELEMS) return DBA_ERR_ARG;
  if (ii ? n_ii < 1 : n_ii != 0) return DBA_ERR_ARG;
  hipLaunchKernelGGL(seed_next_kernel, dim3(1), dim3(SN_THREADS), 0, (hipStream_t)stream, poses, disps, dirty, ht * wd, t1,
                     mean_rows, reinterpret_cast<const long long *>(ii), (long long)n_ii);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_world_poses(const float *poses, int rows, int n, float *out_host, dba_stream_t stream) {
  if (!poses || !out_host || n < 1 || n > rows || n > DBA_FR_MAX_ROWS) return DBA_ERR_ARG;
  FrBlock *b = nullptr;
  const int rc = fr_block_for((hipStream_t)stream, &b);
  if (rc != DBA_OK) return rc;
  std::lock_guard<std::mutex> lock(b->mu);
  const int seq = b->out_seq = fr_next_seq(b->out_seq);
  hipLaunchKernelGGL(world_poses_kernel, dim3(1), dim3(WP_THREADS), 0, (hipStream_t)stream, poses, n, b->out, b->words + 0,
                     seq);
  DBA_LAUNCH_CHECK();
  const int wrc = fr_wait(b->words + 0, seq, b->stream, nullptr);
  if (wrc != DBA_OK) return wrc;
  memcpy(out_host, b->out, sizeof(float) * 16 * (size_t)n);
  return DBA_OK;
}

int dba_set_world_poses(float *poses, float *disps, int rows, int disps_rows, int64_t map_elems, int i0, int n,
                        const double *wTc_host, float inv_scale, int *waited, dba_stream_t stream) {
  if (waited) *waited = 0;
  if (!poses || !wTc_host || n < 1 || n > DBA_FR_MAX_ROWS || i0 < 0 || (int64_t)i0 + n > rows) return DBA_ERR_ARG;
  const bool scales = inv_scale != 0.f;
  if (scales && (!disps || map_elems <= 0 || (int64_t)i0 + n > disps_rows || !(inv_scale > 0.f))) return DBA_ERR_ARG;
  const int64_t scaled = scales ? map_elems * n : 0;
  const int64_t wgs = 1 + (scaled + SC_PER_WG - 1) / SC_PER_WG;
  if (wgs > INT32_MAX) return DBA_ERR_ARG;
  FrBlock *b = nullptr;
  const int rc = fr_block_for((hipStream_t)stream, &b);
  if (rc != DBA_OK) return rc;
  std::lock_guard<std::mutex> lock(b->mu);
  if (b->stage_seq != 0) {  // the launch that last read the staging area must have finished with it
    const int wrc = fr_wait(b->words + 1, b->stage_seq, b->stream, waited);
    if (wrc != DBA_OK) return wrc;
  }
  memcpy(b->stage, wTc_host, sizeof(double) * 16 * (size_t)n);
  const int prev = b->stage_seq, seq = fr_next_seq(prev);
  hipLaunchKernelGGL(set_world_poses_kernel, dim3((unsigned)wgs), dim3(WP_THREADS), 0, (hipStream_t)stream, poses,
                     scales ? disps + map_elems * i0 : nullptr, (long long)scaled, i0, n, b->stage, inv_scale, b->words + 1,
                     seq);
  DBA_LAUNCH_CHECK();  // (a launch that failed leaves stage_seq at the word the block still shows)
  b->stage_seq = seq;
  return DBA_OK;
}

}  // extern "C"
