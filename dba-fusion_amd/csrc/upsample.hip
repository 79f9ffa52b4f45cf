// The `--upsample` path of the reference (dbaf/droid_net.py, dbaf/depth_video.py:205-209):
//   dba_cvx_upsample_disp  <- cvx_upsample with dim == 1        (droid_net.py:17-31), optionally fused with the
//                             gather / index_put of DepthVideo.upsample (depth_video.py:205-209)
//   dba_segment_reduce     <- torch_scatter.scatter_sum / scatter_mean (droid_net.py:14,65 GraphAgg; geom/ba.py:7)
// Both are streaming kernels bound by one read of their large operand (the 576-channel mask, the hidden state):
//   - convex upsampling: one lane = V consecutive coarse pixels (flat index inside the frame) x one sub-row a.  For each
//     sub-column b the lane reads the 9 taps of its V pixels as 9 vector loads (every (k,a,b) plane is contiguous in
//     the pixel index, so a wave reads 64*V consecutive elements per load), keeps the 3x3 disparity neighbourhoods in
//     registers (read through L1: neighbouring lanes and the other seven sub-rows share them) and writes the 8 outputs
//     of a pixel's sub-row as two 16-byte stores;
//   - segmented sum / mean: one workgroup = one output slot x 256*VEC elements of `inner`.  The workgroup collects the
//     slot's members in ascending order into LDS (ballot + per-wave counts, 256 index entries at a time), then every
//     thread sums its VEC elements over them in float and rounds once.  No atomics: results are bit-identical run to
//     run, and nothing synchronises the host (graph-capturable).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "cvx_weights.h"

namespace dba {

typedef _Float16 half_t;

// V consecutive elements of T as floats, one load (the caller guarantees V*sizeof(T) alignment)
template <typename T, int V> struct VecLoad;
template <> struct VecLoad<float, 1> {
  static __device__ __forceinline__ void run(const float *p, float *o) { o[0] = *p; }
};
template <> struct VecLoad<float, 2> {
  static __device__ __forceinline__ void run(const float *p, float *o) {
    const float2 v = *reinterpret_cast<const float2 *>(p);
    o[0] = v.x; o[1] = v.y;
  }
};
template <int V> struct VecLoad<half_t, V> {
  // hipcc does not widen 16-bit scalar loads: read V halves as one word
  typedef half_t vec_t __attribute__((ext_vector_type(V)));
  static __device__ __forceinline__ void run(const half_t *p, float *o) {
    const vec_t v = *reinterpret_cast<const vec_t *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (float)v[j];
  }
};
template <> struct VecLoad<half_t, 1> {
  static __device__ __forceinline__ void run(const half_t *p, float *o) { o[0] = (float)*p; }
};

// ---- convex upsampling ---------------------------------------------------------------------------------------------
// out[dst, 8y+a, 8x+b] = sum_k w_k d[src, y+ky-1, x+kx-1] (zero outside the map), w = softmax_k(mask[f, k*64+a*8+b, y, x]),
// k = ky*3+kx.  exp(t) is evaluated as the hardware exp2 of t*log2 e on t = m - max <= 0: the rounding of the scaled
// argument costs at most |t| e^t * 2^-24 <= 2^-24/e of a weight, and a weight below 2^-126 (flushed to 0) is below the
// float rounding of the sum.  The nine weights share one reciprocal of their sum.  With a half mask each weight is
// rounded to half before the product, as torch.softmax returns the mask's dtype and the product with the float
// disparity promotes.
template <typename T, int V>
__global__ __launch_bounds__(256) void cvx_upsample_kernel(const float *__restrict__ disps, int n_disps,
                                                           const int64_t *__restrict__ src_rows,
                                                           const T *__restrict__ mask, int ht, int wd,
                                                           float *__restrict__ out, int n_out,
                                                           const int64_t *__restrict__ dst_rows) {
  const int f = blockIdx.z;
  const int a = blockIdx.y;
  const int HW = ht * wd;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g * V >= HW) return;
  const int64_t sr = src_rows ? src_rows[f] : f;
  const int64_t dr = dst_rows ? dst_rows[f] : f;
  if (sr < 0 || sr >= n_disps || dr < 0 || dr >= n_out) return;  // bad row maps are skipped, never dereferenced

  const int p0 = g * V;
  const float *d = disps + (size_t)sr * HW;
  float dk[V][9];
  int py[V], px[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int p = p0 + v;
    const int y = p / wd, x = p - y * wd;
    py[v] = y;
    px[v] = x;
    cvx_taps(d, y, x, ht, wd, dk[v]);
  }

  const T *m = mask + ((size_t)f * 576 + (size_t)a * 8) * HW + p0;
  float res[V][8];
#pragma unroll 2
  for (int b = 0; b < 8; ++b) {
    float e[9][V];
#pragma unroll
    for (int k = 0; k < 9; ++k) VecLoad<T, V>::run(m + (size_t)(k * 64 + b) * HW, e[k]);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float ev[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) ev[k] = e[k][v];
      res[v][b] = cvx_combine<sizeof(T) == 2>(ev, dk[v]);
    }
  }

  const int W8 = 8 * wd;
  float *o = out + (size_t)dr * 64 * HW;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float4 *q = reinterpret_cast<float4 *>(o + (size_t)(8 * py[v] + a) * W8 + 8 * px[v]);
    q[0] = make_float4(res[v][0], res[v][1], res[v][2], res[v][3]);
    q[1] = make_float4(res[v][4], res[v][5], res[v][6], res[v][7]);
  }
}

template <typename T, int V>
static int launch_cvx(const float *disps, int n_disps, const int64_t *src_rows, const void *mask, int B, int ht,
                      int wd, float *out, int n_out, const int64_t *dst_rows, hipStream_t stream) {
  const int G = ht * wd / V;
  hipLaunchKernelGGL((cvx_upsample_kernel<T, V>), dim3((G + 255) / 256, 8, B), dim3(256), 0, stream, disps, n_disps,
                     src_rows, (const T *)mask, ht, wd, out, n_out, dst_rows);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

// ---- segmented sum / mean ------------------------------------------------------------------------------------------
template <typename T, int VEC> struct SegIO;
template <> struct SegIO<float, 8> {
  static __device__ __forceinline__ void load(const float *p, float *o) {
    const float4 u = reinterpret_cast<const float4 *>(p)[0], v = reinterpret_cast<const float4 *>(p)[1];
    o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w; o[4] = v.x; o[5] = v.y; o[6] = v.z; o[7] = v.w;
  }
  static __device__ __forceinline__ void store(float *p, const float *o) {
    reinterpret_cast<float4 *>(p)[0] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<float4 *>(p)[1] = make_float4(o[4], o[5], o[6], o[7]);
  }
};
template <> struct SegIO<half_t, 8> {
  typedef half_t vec_t __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ void load(const half_t *p, float *o) {
    const vec_t v = *reinterpret_cast<const vec_t *>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)v[j];
  }
  static __device__ __forceinline__ void store(half_t *p, const float *o) {
    vec_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (half_t)o[j];
    *reinterpret_cast<vec_t *>(p) = v;
  }
};
template <typename T> struct SegIO<T, 1> {
  static __device__ __forceinline__ void load(const T *p, float *o) { o[0] = (float)*p; }
  static __device__ __forceinline__ void store(T *p, const float *o) { *p = (T)o[0]; }
};

template <typename T, int VEC>
__global__ __launch_bounds__(256) void segment_reduce_kernel(const T *__restrict__ src,
                                                             const int64_t *__restrict__ index, int n,
                                                             int64_t inner, int dim_size, int nchunks, int mean,
                                                             T *__restrict__ out) {
  __shared__ int members[256];
  __shared__ int wave_count[4];
  const int64_t bid = blockIdx.x;
  const int chunk = (int)(bid % nchunks);
  const int64_t rest = bid / nchunks;
  const int slot = (int)(rest % dim_size);
  const int64_t o = rest / dim_size;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)chunk * 256 + threadIdx.x) * VEC;
  const bool active = i0 < inner;
  const T *s0 = src + (size_t)o * n * inner + i0;

  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  int count = 0;
  for (int base = 0; base < n; base += 256) {
    // this slot's members among index[base, base+256), in ascending order (entries outside [0, dim_size) match no slot)
    const int e = base + threadIdx.x;
    const bool hit = e < n && index[e] == (int64_t)slot;
    const unsigned long long ball = __ballot(hit);
    if (lane == 0) wave_count[wv] = __popcll(ball);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wave_count[w];
      off += w < wv ? c : 0;
      tot += c;
    }
    if (hit) members[off + __popcll(ball & ((1ull << lane) - 1ull))] = e;
    __syncthreads();
    if (active) {
      int j = 0;
      for (; j + 4 <= tot; j += 4) {  // four rows in flight, added in member order
        float v[4][VEC];
#pragma unroll
        for (int q = 0; q < 4; ++q) SegIO<T, VEC>::load(s0 + (size_t)members[j + q] * inner, v[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < VEC; ++t) acc[t] += v[q][t];
      }
      for (; j < tot; ++j) {
        float v[VEC];
        SegIO<T, VEC>::load(s0 + (size_t)members[j] * inner, v);
#pragma unroll
        for (int t = 0; t < VEC; ++t) acc[t] += v[t];
      }
    }
    count += tot;
    __syncthreads();  // members[] is rewritten by the next 256 entries
  }
  if (!active) return;
  if (mean) {
    const float c = (float)(count > 0 ? count : 1);
#pragma unroll
    for (int t = 0; t < VEC; ++t) acc[t] = acc[t] / c;
  }
  SegIO<T, VEC>::store(out + ((size_t)o * dim_size + slot) * inner + i0, acc);
}

template <typename T, int VEC>
static int launch_segment(const void *src, const int64_t *index, int n, int64_t outer, int64_t inner, int dim_size,
                          int mean, void *out, hipStream_t stream) {
  const int64_t nchunks = (inner + 256 * VEC - 1) / (256 * VEC);
  const int64_t blocks = outer * dim_size * nchunks;
  if (nchunks > INT32_MAX || blocks > INT32_MAX) return DBA_ERR_ARG;
  hipLaunchKernelGGL((segment_reduce_kernel<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, stream, (const T *)src,
                     index, n, inner, dim_size, (int)nchunks, mean, (T *)out);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_cvx_upsample_disp(const float *disps, int n_disps, const int64_t *src_rows, const void *mask, int mask_dtype,
                          int B, int ht, int wd, float *out, int n_out, const int64_t *dst_rows, dba_stream_t stream) {
  if (B < 0 || ht <= 0 || wd <= 0 || n_disps < 0 || n_out < 0 || B > 65535) return DBA_ERR_ARG;
  if (mask_dtype != DBA_F32 && mask_dtype != DBA_F16) return DBA_ERR_UNSUPPORTED;
  if ((int64_t)ht * wd * 64 > INT32_MAX) return DBA_ERR_ARG;
  if (B == 0) return DBA_OK;
  if (!disps || !mask || !out || ((uintptr_t)out & 15)) return DBA_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int HW = ht * wd;
  const size_t esz = mask_dtype == DBA_F16 ? 2 : 4;
  auto fits = [&](int v) { return HW % v == 0 && ((uintptr_t)mask % (v * esz)) == 0; };
  // two pixels per lane when the plane stride and the base allow it (every (k,a,b) plane starts at a multiple of HW):
  // ~70 VGPRs, room for 7 waves per SIMD.  Four half pixels per lane (8-byte loads, ~128 VGPRs) measured 48 us against
  // 34 us for two at the 25-frame 64x64 window: the waves, not the load width, cover the HBM latency there.
  if (mask_dtype == DBA_F16) {
    if (fits(2)) return launch_cvx<half_t, 2>(disps, n_disps, src_rows, mask, B, ht, wd, out, n_out, dst_rows, s);
    return launch_cvx<half_t, 1>(disps, n_disps, src_rows, mask, B, ht, wd, out, n_out, dst_rows, s);
  }
  if (fits(2)) return launch_cvx<float, 2>(disps, n_disps, src_rows, mask, B, ht, wd, out, n_out, dst_rows, s);
  return launch_cvx<float, 1>(disps, n_disps, src_rows, mask, B, ht, wd, out, n_out, dst_rows, s);
}

int dba_segment_reduce(const void *src, int dtype, const int64_t *index, int n, int64_t outer, int64_t inner,
                       int dim_size, int mean, void *out, dba_stream_t stream) {
  if (n < 0 || outer < 0 || inner < 0 || dim_size < 0) return DBA_ERR_ARG;
  if (dtype != DBA_F32 && dtype != DBA_F16) return DBA_ERR_UNSUPPORTED;
  if (outer == 0 || inner == 0 || dim_size == 0) return DBA_OK;
  if (!out || (n > 0 && (!src || !index))) return DBA_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const size_t esz = dtype == DBA_F16 ? 2 : 4;
  // 8 elements per thread when every row of `inner` starts on a 8-element boundary of an aligned base
  const bool wide = inner % 8 == 0 && ((uintptr_t)src % (8 * esz)) == 0 && ((uintptr_t)out % (8 * esz)) == 0;
  if (dtype == DBA_F16)
    return wide ? launch_segment<half_t, 8>(src, index, n, outer, inner, dim_size, mean, out, s)
                : launch_segment<half_t, 1>(src, index, n, outer, inner, dim_size, mean, out, s);
  return wide ? launch_segment<float, 8>(src, index, n, outer, inner, dim_size, mean, out, s)
              : launch_segment<float, 1>(src, index, n, outer, inner, dim_size, mean, out, s);
}

}  // extern "C"
