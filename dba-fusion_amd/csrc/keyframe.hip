// The two per-frame decisions the host takes from device data (dbaf/dbaf_frontend.py:262-264, :319-324 and
// dbaf/motion_filter.py:87), gfx950.  Each is ONE launch of one workgroup that writes a small report into pinned,
// host-coherent words and then a completion word; the host spins on that word (the hand-over of BACore.hessian,
// ba_host.hip).  Nothing synchronises the stream.
//   dba_keyframe_check           <- d = video.distance([t1-3], [t1-2], beta, bidirectional=True) (:263),
//                                   poses[t1-1].inv().matrix() (:264) and cam_translation (:320-323)
//   dba_keyframe_flow_magnitude  <- delta.norm(dim=-1).mean() (motion_filter.py:87)
// keyframe_check_kernel: 512 lanes.  Lanes 0-255 and 256-511 run the per-pair body of frame_distance_kernel
// (frame_distance.h) for (t1-3, t1-2) and (t1-2, t1-3) exactly as frame_distance_bidir_kernel (proximity.hip) does, so d
// is bit-identical to dba_frame_distance_bidir on that pair (this file is built with the same flags).  Lanes 0-7 of wave
// 0 then compute the pose statements with the operations of the lietorch shim (lietorch/__init__.py: _qinv, _qrot,
// SE3.inv, SE3.mul, SE3.matrix) in its order, each spelled with an intrinsic the compiler does not fuse.  After the
// barrier lane 0 writes the report.
// flow_magnitude_kernel: 1024 lanes, pixels lane-strided, wave_sum, the 16 partials in wave order: one fixed order of
// additions, bit-identical run to run.  No atomics anywhere.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>

#include "common.h"
#include "frame_distance.h"
#include "pose_inv.h"

namespace dba {

// the report, 32-bit words: [0] d or the flow magnitude (float)  [1] the window length, 7 or 3 (int)
// [2..9) cam_translation (float)  [9..25) the 4x4 matrix, row-major (float)  [25] the completion word (int)
constexpr int KF_D = DBA_KF_D, KF_WIN = DBA_KF_WIN, KF_CAM = DBA_KF_CAM, KF_MAT = DBA_KF_MAT, KF_SEQ = DBA_KF_SEQ;
constexpr int KF_WORDS = DBA_KF_WORDS;
constexpr int KF_MAX_WIN = 7;
static_assert(KF_CAM + KF_MAX_WIN == KF_MAT && KF_MAT + 16 == KF_SEQ && KF_SEQ + 1 == KF_WORDS, "report layout");
constexpr int KF_BLOCK_WORDS = 32;   // one block per 128-byte line
constexpr int KF_SLAB_BLOCKS = 32;
constexpr int KF_FLOW_THREADS = 1024;

__global__ __launch_bounds__(512) void keyframe_check_kernel(const float *__restrict__ poses,
                                                             const float *__restrict__ disps,
                                                             const float *__restrict__ intr, int t1, int HW, int wd,
                                                             float beta, float *report, int seq) {
  __shared__ float red[2][3][4];
  __shared__ float s_cam[KF_MAX_WIN + 1];
  __shared__ float s_mat[16];
  const int dir = threadIdx.x >> 8, tid = threadIdx.x & 255;
  const int i = t1 - 3, j = t1 - 2;
  frame_distance_partials(poses, disps, intr, dir ? j : i, dir ? i : j, HW, wd, beta, tid, 256, red[dir]);
  const int win = t1 > 10 ? KF_MAX_WIN : 3, k0 = t1 - 3 - win;   // :320-323: rows [t1-10, t1-3) or [t1-6, t1-3)
  if (threadIdx.x < KF_MAX_WIN) {
    float c = 0.f;
    if ((int)threadIdx.x < win) {
      // (poses[k] * poses[t1-2].inv()).translation(): _qrot(q_k, t_inv) + t_k, then torch.norm over its three entries
      float ti[3], qi[4], r[3];
      kf_inv(poses + 7 * j, ti, qi);
      const float *Pk = poses + 7 * (k0 + (int)threadIdx.x);
      kf_qrot(Pk + 3, ti, r);
      const float x = __fadd_rn(r[0], Pk[0]), y = __fadd_rn(r[1], Pk[1]), z = __fadd_rn(r[2], Pk[2]);
      c = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    }
    s_cam[threadIdx.x] = c;
  } else if (threadIdx.x == KF_MAX_WIN) {
    // poses[t1-1].inv().matrix(), by the call that dba_world_poses (frames.hip) makes for every row: the same bits
    const float *P = poses + 7 * (t1 - 1);
    const KfMat34 M = kf_inv_matrix(P[0], P[1], P[2], P[3], P[4], P[5], P[6]);
#pragma unroll
    for (int k = 0; k < 12; k++) s_mat[k] = M.m[k];
    s_mat[12] = 0.f; s_mat[13] = 0.f; s_mat[14] = 0.f; s_mat[15] = 1.f;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float d1 = frame_distance_finish(red[0]), d2 = frame_distance_finish(red[1]);
  report[KF_D] = 0.5f * (d1 + d2);  // depth_video.py:261, float32
  reinterpret_cast<int *>(report)[KF_WIN] = win;
#pragma unroll
  for (int k = 0; k < KF_MAX_WIN; k++) report[KF_CAM + k] = s_cam[k];
#pragma unroll
  for (int k = 0; k < 16; k++) report[KF_MAT + k] = s_mat[k];
  __threadfence_system();
  __hip_atomic_store(reinterpret_cast<int *>(report) + KF_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void kf_load_pair(const float *p, int k, float &x, float &y) {
  const float2 v = reinterpret_cast<const float2 *>(p)[k];
  x = v.x; y = v.y;
}
__device__ __forceinline__ void kf_load_pair(const __half *p, int k, float &x, float &y) {
  const __half2 v = reinterpret_cast<const __half2 *>(p)[k];
  x = __low2float(v); y = __high2float(v);
}

// mean over pixels of sqrt(dx^2 + dy^2).  HALF: torch's semantics for a half tensor -- each norm is computed in float
// (x * x is exact there, the sum is rounded once) and rounded to half, the halves are summed in float, the mean is
// rounded to half.
template <typename T, bool HALF>
__global__ __launch_bounds__(KF_FLOW_THREADS) void flow_magnitude_kernel(const T *__restrict__ delta, int n,
                                                                         float *report, int seq) {
  __shared__ float part[KF_FLOW_THREADS / 64];
  float acc = 0.f;
  for (int k = threadIdx.x; k < n; k += KF_FLOW_THREADS) {
    float x, y;
    kf_load_pair(delta, k, x, y);
    float r = sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
    if (HALF) r = __half2float(__float2half_rn(r));
    acc = __fadd_rn(acc, r);
  }
  const float a = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float s = part[0];
#pragma unroll
  for (int w = 1; w < KF_FLOW_THREADS / 64; w++) s = __fadd_rn(s, part[w]);
  float m = __fdiv_rn(s, (float)n);
  if (HALF) m = __half2float(__float2half_rn(m));
  report[KF_D] = m;
  __threadfence_system();
  __hip_atomic_store(reinterpret_cast<int *>(report) + KF_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the pinned report blocks: one per (device, stream), carved from slabs that are never freed (a view of a block that
// outlives its call must not dangle) ----------------------------------------------------------------------
namespace {
struct KfBlock {
  float *words = nullptr;
  hipStream_t stream = nullptr;
  int seq = 0;
};
std::mutex g_kf_mu;
typedef std::map<std::pair<int, hipStream_t>, KfBlock *> KfStreamMap;
typedef std::map<const void *, KfBlock *> KfAddressMap;
struct KfState {   // (never destroyed: calls may still arrive at exit)
  KfStreamMap by_stream;
  KfAddressMap by_address;
  float *slab = nullptr;
  int used = KF_SLAB_BLOCKS;
};
KfState &kf_state() {
  static KfState *s = new KfState;
  return *s;
}

// the block behind a report pointer this library handed out, or null
KfBlock *kf_block_of(const void *report) {
  std::lock_guard<std::mutex> lock(g_kf_mu);
  KfState &S = kf_state();
  const KfAddressMap::iterator it = S.by_address.find(report);
  return it == S.by_address.end() ? nullptr : it->second;
}

int kf_block_for(hipStream_t stream, KfBlock **out) {
  int dev = 0;
  DBA_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_kf_mu);
  KfState &S = kf_state();
  KfBlock *&b = S.by_stream[std::make_pair(dev, stream)];
  if (!b) {
    if (S.used == KF_SLAB_BLOCKS) {
      void *p = nullptr;
      const size_t bytes = sizeof(float) * KF_BLOCK_WORDS * KF_SLAB_BLOCKS;
      DBA_HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
      memset(p, 0, bytes);
      S.slab = static_cast<float *>(p), S.used = 0;
    }
    b = new KfBlock;
    b->words = S.slab + (size_t)KF_BLOCK_WORDS * S.used++;
    b->stream = stream;
    S.by_address[b->words] = b;
  }
  *out = b;
  return DBA_OK;
}
}  // namespace

}  // namespace dba

using namespace dba;

extern "C" {

int dba_keyframe_report_words(void) { return KF_WORDS; }

int dba_keyframe_report(dba_stream_t stream, void **report, int *seq) {
  if (!report || !seq) return DBA_ERR_ARG;
  KfBlock *b = nullptr;
  const int rc = kf_block_for((hipStream_t)stream, &b);
  if (rc != DBA_OK) return rc;
  std::lock_guard<std::mutex> lock(g_kf_mu);
  if (++b->seq <= 0) b->seq = 1;   // never 0, the word of a fresh block
  *report = b->words;
  *seq = b->seq;
  return DBA_OK;
}

int dba_keyframe_check(const float *poses, const float *disps, const float *intrinsics, int n_frames, int ht, int wd,
                       int t1, float beta, void *report, int seq, dba_stream_t stream) {
  if (t1 < 6 || (int64_t)t1 - 1 >= n_frames || ht <= 0 || wd <= 0 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if (!poses || !disps || !intrinsics || !report) return DBA_ERR_ARG;
  const KfBlock *b = kf_block_of(report);
  if (!b || b->stream != (hipStream_t)stream) return DBA_ERR_ARG;
  hipLaunchKernelGGL(keyframe_check_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, poses, disps, intrinsics, t1,
                     ht * wd, wd, beta, static_cast<float *>(report), seq);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_keyframe_flow_magnitude(const void *delta, int dtype, int n_pixels, void *report, int seq, dba_stream_t stream) {
  if (n_pixels <= 0 || !delta || !report) return DBA_ERR_ARG;
  if (dtype != DBA_F32 && dtype != DBA_F16) return DBA_ERR_UNSUPPORTED;
  const KfBlock *b = kf_block_of(report);
  if (!b || b->stream != (hipStream_t)stream) return DBA_ERR_ARG;
  float *rep = static_cast<float *>(report);
  if (dtype == DBA_F16)
    hipLaunchKernelGGL((flow_magnitude_kernel<__half, true>), dim3(1), dim3(KF_FLOW_THREADS), 0, (hipStream_t)stream,
                       static_cast<const __half *>(delta), n_pixels, rep, seq);
  else
    hipLaunchKernelGGL((flow_magnitude_kernel<float, false>), dim3(1), dim3(KF_FLOW_THREADS), 0, (hipStream_t)stream,
                       static_cast<const float *>(delta), n_pixels, rep, seq);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

// spins until the block's completion word shows `seq`; every few thousand looks asks the runtime whether the stream has
// drained (a launch that failed never sets the word)
int dba_keyframe_wait(const void *report, int seq) {
  const KfBlock *b = kf_block_of(report);
  if (!b) return DBA_ERR_ARG;
  const int *flag = reinterpret_cast<const int *>(b->words) + KF_SEQ;
  for (unsigned long spins = 1;; spins++) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return DBA_OK;
    if ((spins & 0x3fff) == 0) {
      const hipError_t q = hipStreamQuery(b->stream);
      if (q == hipSuccess) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return DBA_OK;
        set_last_error("keyframe: the stream drained without the report's completion word", hipErrorUnknown);
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

}  // extern "C"
