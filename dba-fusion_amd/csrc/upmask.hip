// Upsample mode without the 576-channel mask in HBM, and without torch.unique (dbaf/droid_net.py:17-31, :55-72;
// dbaf/depth_video.py:205-209):
//   dba_upmask_upsample_disp  <- GraphAgg's `upmask = Conv2d(128, 576, 1)(net)` (droid_net.py:70) and DepthVideo.upsample
//                                (depth_video.py:205-209) in ONE launch: disps_up[dst[f]] = cvx_upsample(disps[src[f]], W x[f] + b)
//   dba_frame_plan            <- `_, ix = torch.unique(ii, return_inverse=True)` (droid_net.py:57) and the caller's
//                                torch.unique(self.ii) (covisible_graph.py:240, :340), one small launch
//
// upmask_upsample_kernel.  One workgroup = 128 consecutive pixels of the flat [B * ht * wd] pixel axis (a tile may straddle
// two frames) x all 576 channels; four waves, wave g owns the channels k*64 + g*16 + 0..15 of the nine taps k, i.e. the
// sub-rows a = 2g, 2g + 1 of every pixel.
//   - the wave keeps ITS slice of W in registers for the workgroup's life: nine taps x four K-steps of mfma_f32_16x16x32_f16
//     fragments, each lane's fragment 16 contiguous bytes of a row of W (144 VGPRs).  W is read once per workgroup, from L2;
//   - the workgroup's x (128 pixels x 128 channels, channel-major in HBM) is staged once, transposed, into LDS rows of
//     128 + 8 halves: a fragment of x is then one 16-byte LDS read, and the 272-byte row pitch spreads the 16 pixels of a
//     read over all banks;
//   - per 16 pixels: 36 MFMAs into nine accumulator tiles.  W's rows are the A operand and the pixels the B operand, so
//     a lane holds, for ONE pixel (column l & 15), the channels 4 (l >> 4) + 0..3 of each tap: the nine taps of a sub-pixel
//     sit in the same register of the nine tiles (the softmax needs no cross-lane traffic), and the four registers of a tile
//     are four consecutive sub-columns b: the lane's outputs leave as one 16-byte store, and the 16 pixels x 2 lanes of a
//     sub-row write 512 contiguous bytes;
//   - epilogue per accumulator: + bias in float, ONE rounding to half (what the stock convolution stores; mask_out
//     receives it when asked), then cvx_combine of cvx_weights.h, the routine cvx_upsample_kernel calls.
// No atomics, no host synchronisation, caller's memory only.
//
// frame_plan_kernel.  One workgroup: a presence flag per buffer row in LDS, a scan over the rows, then uniq (ascending) and
// inverse.  Words of `res`: [0] n_uniq, [1] entries outside [0, buffer), [2] the first such entry's position.  A later
// call on a remembered edge set passes the n_uniq its outputs were sized for; a mismatch or an index out of range is
// reported through the pinned words of size_guard.h, which the next call polls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "cvx_weights.h"
#include "size_guard.h"

namespace dba {

typedef _Float16 half_t;
typedef half_t half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int UM_PT = 128;         // pixels per workgroup
constexpr int UM_C = 128;          // channels of x: K
constexpr int UM_XS = UM_C + 8;    // LDS row pitch in halves (272 bytes)
constexpr int UM_CH = 576;         // 9 taps x 8 x 8 sub-pixels

__global__ __launch_bounds__(256) void upmask_upsample_kernel(const half_t *__restrict__ x, const half_t *__restrict__ W,
                                                              const half_t *__restrict__ bias,
                                                              const float *__restrict__ disps, int n_disps,
                                                              const int64_t *__restrict__ src_rows, int B, int ht, int wd,
                                                              float *__restrict__ out, int n_out,
                                                              const int64_t *__restrict__ dst_rows,
                                                              half_t *__restrict__ mask_out) {
  __shared__ __attribute__((aligned(16))) half_t xs[UM_PT * UM_XS];
  __shared__ __attribute__((aligned(16))) float bl[UM_CH];
  const int HW = ht * wd;
  const int64_t total = (int64_t)B * HW;
  const int64_t tile0 = (int64_t)blockIdx.x * UM_PT;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;

  for (int c = threadIdx.x; c < UM_CH; c += 256) bl[c] = bias ? (float)bias[c] : 0.f;

  {  // x -> LDS, transposed: a thread takes one pixel and 64 channels, 8 channels per 16-byte LDS write
    const int p = threadIdx.x & (UM_PT - 1), c0 = (threadIdx.x >> 7) * 64;
    const int64_t gp = tile0 + p;
    const bool ok = gp < total;
    const int f = ok ? (int)(gp / HW) : 0;
    const int pp = ok ? (int)(gp - (int64_t)f * HW) : 0;
    const half_t *src = x + ((size_t)f * UM_C + c0) * HW + pp;
#pragma unroll 4
    for (int c8 = 0; c8 < 8; ++c8) {
      half8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ok ? src[(size_t)(c8 * 8 + j) * HW] : (half_t)0.f;
      *reinterpret_cast<half8 *>(&xs[p * UM_XS + c0 + c8 * 8]) = v;
    }
  }
  // this wave's slice of W (read behind the staging, whose loads need the registers first): tap k, K-step s -> rows k*64 + g*16 + r, halves s*32 + q*8 .. +8
  half8 wa[9][4];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      wa[k][s] = *reinterpret_cast<const half8 *>(W + (size_t)(k * 64 + g * 16 + r) * UM_C + s * 32 + q * 8);

  __syncthreads();

  const int a = 2 * g + (q >> 1), b0 = 4 * (q & 1);
#pragma unroll 1
  for (int t = 0; t < UM_PT / 16; ++t) {
    const int pl = t * 16 + r;
    if (tile0 + t * 16 >= total) break;   // uniform: the whole 16-pixel group lies past the end
    half8 xb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) xb[s] = *reinterpret_cast<const half8 *>(&xs[pl * UM_XS + s * 32 + q * 8]);
    float4v acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[k][s], xb[s], acc[k], 0, 0, 0);

    const int64_t gp = tile0 + pl;
    if (gp >= total) continue;
    const int f = (int)(gp / HW);
    const int pp = (int)(gp - (int64_t)f * HW);
    const int y = pp / wd, xx = pp - y * wd;
    const int64_t sr = src_rows ? src_rows[f] : f;
    const int64_t dr = dst_rows ? dst_rows[f] : f;
    const bool rows_ok = sr >= 0 && sr < n_disps && dr >= 0 && dr < n_out;   // bad row maps are skipped, never dereferenced
    if (!rows_ok && !mask_out) continue;
    float dk[9];
    if (rows_ok) {
      cvx_taps(disps + (size_t)sr * HW, y, xx, ht, wd, dk);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) dk[k] = 0.f;
    }
    float res[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float e[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int ch = k * 64 + g * 16 + 4 * q + i;
        const half_t h = (half_t)(acc[k][i] + bl[ch]);
        if (mask_out) mask_out[((size_t)f * UM_CH + ch) * HW + pp] = h;
        e[k] = (float)h;
      }
      res[i] = cvx_combine<true>(e, dk);
    }
    if (rows_ok) {
      float *o = out + (size_t)dr * 64 * HW + (size_t)(8 * y + a) * (8 * wd) + 8 * xx + b0;
      *reinterpret_cast<float4 *>(o) = make_float4(res[0], res[1], res[2], res[3]);
    }
  }
}

// ---- frame plan ------------------------------------------------------------------------------------------------------
constexpr int FP_MAX_ROWS = 4096;
static SizeGuard g_plan_guard;

__global__ __launch_bounds__(256) void frame_plan_kernel(const int64_t *__restrict__ ii, int n, int buffer, int cap,
                                                         int64_t *__restrict__ uniq, int64_t *__restrict__ inverse,
                                                         int *__restrict__ res, int expect, int *status) {
  __shared__ unsigned char present[FP_MAX_ROWS];
  __shared__ unsigned short rank[FP_MAX_ROWS];
  __shared__ int scan[256];
  __shared__ int bad_count[256];
  __shared__ int bad_first[256];
  const int t = threadIdx.x;
  for (int row = t; row < buffer; row += 256) present[row] = 0;
  __syncthreads();
  int nbad = 0, first = n;
  for (int e = t; e < n; e += 256) {
    const int64_t v = ii[e];
    if (v < 0 || v >= buffer) {
      if (!nbad) first = e;
      ++nbad;
    } else {
      present[v] = 1;   // every writer stores the same value
    }
  }
  bad_count[t] = nbad;
  bad_first[t] = first;
  __syncthreads();
  // each thread owns `per` consecutive rows; an inclusive scan of the 256 counts through LDS
  const int per = (buffer + 255) / 256;
  const int r0 = t * per, r1 = min(buffer, r0 + per);
  int cnt = 0;
  for (int row = r0; row < r1; ++row) cnt += present[row];
  scan[t] = cnt;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? scan[t - d] : 0;
    const int bc = t >= d ? bad_count[t - d] : 0;
    const int bf = t >= d ? bad_first[t - d] : n;
    __syncthreads();
    scan[t] += add;
    bad_count[t] += bc;
    bad_first[t] = min(bad_first[t], bf);
    __syncthreads();
  }
  const int total = scan[255];
  int off = scan[t] - cnt;
  for (int row = r0; row < r1; ++row)
    if (present[row]) {
      rank[row] = (unsigned short)off;
      if (off < cap) uniq[off] = row;
      ++off;
    }
  for (int j = total + t; j < cap; j += 256) uniq[j] = -1;   // what a call sized for more rows must not read as a row
  __syncthreads();
  for (int e = t; e < n; e += 256) {
    const int64_t v = ii[e];
    inverse[e] = (v < 0 || v >= buffer) ? -1 : (int64_t)rank[v];
  }
  if (t == 255) {
    const int bad = bad_count[255], bfirst = bad ? bad_first[255] : -1;
    res[0] = total;
    res[1] = bad;
    res[2] = bfirst;
    res[3] = 0;
    if (expect >= 0 && (total != expect || bad)) {
      const int got[3] = {total, bad, bfirst}, exp[3] = {expect, 0, -1};
      guard_report<3>(status, got, exp);
    }
  }
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_upmask_upsample_disp(const void *x, const void *weight, const void *bias, const float *disps, int n_disps,
                             const int64_t *src_rows, int B, int ht, int wd, float *out, int n_out,
                             const int64_t *dst_rows, void *mask_out, dba_stream_t stream) {
  if (B < 0 || ht <= 0 || wd <= 0 || n_disps < 0 || n_out < 0) return DBA_ERR_ARG;
  if ((int64_t)ht * wd * 64 > INT32_MAX) return DBA_ERR_ARG;
  const int64_t tiles = ((int64_t)B * ht * wd + UM_PT - 1) / UM_PT;
  if (tiles > INT32_MAX) return DBA_ERR_ARG;
  if (B == 0) return DBA_OK;
  if (!x || !weight || !disps || !out) return DBA_ERR_ARG;
  if (((uintptr_t)out & 15) || ((uintptr_t)weight & 15) || ((uintptr_t)x & 1) || ((uintptr_t)mask_out & 1) ||
      ((uintptr_t)bias & 1))
    return DBA_ERR_ARG;
  hipLaunchKernelGGL(upmask_upsample_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const half_t *)x,
                     (const half_t *)weight, (const half_t *)bias, disps, n_disps, src_rows, B, ht, wd, out, n_out,
                     dst_rows, (half_t *)mask_out);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_frame_plan_max_rows(void) { return FP_MAX_ROWS; }

int dba_frame_plan(const int64_t *ii, int n, int buffer, int cap, int64_t *uniq, int64_t *inverse, int *res, int expect,
                   dba_stream_t stream) {
  if (n < 0 || buffer <= 0 || buffer > FP_MAX_ROWS || cap < 0) return DBA_ERR_ARG;
  if (!res || (n > 0 && (!ii || !inverse)) || (cap > 0 && !uniq)) return DBA_ERR_ARG;
  if (cap < (n < buffer ? n : buffer)) return DBA_ERR_ARG;   // uniq must hold min(n, buffer) rows
  int *status = nullptr;
  const int rc = g_plan_guard.words(&status);
  if (rc != DBA_OK) return rc;
  hipLaunchKernelGGL(frame_plan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ii, n, buffer, cap, uniq, inverse, res,
                     expect, status);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_frame_plan_poll(int *out6) { return g_plan_guard.poll(out6, 6); }

}  // extern "C"
