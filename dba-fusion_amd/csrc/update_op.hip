// The heads of the update operator (include/dba_hip.h "Update operator heads"): 3x3 convolutions with ONE or TWO output
// channels, with what the reference runs around them, every head of a call in one launch
// (dbaf/droid_net.py:47-50, :68, :71, :91-102, :124-128):
//
//   dba_upd_heads  <- [ReLU,] Conv2d(c, k, 3, padding=1), GradientClip (identity in forward), then nothing / Sigmoid /
//                     Softplus and `.01 *`, and the permute(..)[..., :k].contiguous() that makes [n, ht, wd, k] of it
//
// A c -> 2 convolution is a 9 c term dot product per pixel and output, bound by reading x once; it is no GEMM.  This file
// is built with -ffp-contract=off: a product and the addition that takes it round separately.
//
// Tile.  A workgroup of 256 lanes owns UPD_TR x UPD_TC = 16 x 64 pixels of one edge of one head, all c channels; lane t
// owns the four pixels (row t / 16, columns 4 (t % 16) .. + 3).  The channels go by in chunks of UPD_CC = 4: the chunk's
// slab of x (the tile and its halo of one pixel, as float32, ReLU applied where relu_in) and its 4 * 9 * k weights are
// staged in LDS, 21 KB in all; the next chunk's loads are issued into registers before the current chunk's arithmetic, so a
// chunk's latency hides behind the one before it.  Positions of the slab outside the map are written once, as zeros, and
// never again: that is the padding.  Every byte of x is requested once, apart from the halo rows between two tiles (2 in
// 18) and, on maps wider than 64, the halo columns (2 in 66); a halo is read a second time while the neighbouring tile's
// workgroup runs, out of L2.
// Staging routes, the same arithmetic and the same bits behind both:
//   vectors   hw * itemsize a multiple of 16, every x base on a 16-byte boundary and wd <= 64 (one tile across): the slab of
//             a channel is one contiguous run of the plane, read in 16-byte vectors from the vector boundary at or below
//             its first element; a lane works out once where its vector's elements land in the LDS rows;
//   elements  everything else (5 x 7, 55 x 55, 28 x 107): element loads, consecutive lanes on consecutive columns.
// Arithmetic, in two levels.  Per pixel and output, every chunk of four channels (channels 4 j .. 4 j + 3; the last chunk may
// be short) has its own sum, from +0, p = (..((0 + x w)_{c,ky=0,kx=0} + x w)_{c,0,1} ..): c ascending within the chunk, then
// ky, then kx, padded taps included as +0 * w; the chunk sums are then added one by one, chunk 0 first, to the accumulator,
// which starts at +0: s = (..((0 + p_0) + p_1) ..).  (One chain over all 9 c terms measured 1.3 x the error of MIOpen's
// float32 convolution on the delta head; with chunk sums the rounding of 36 terms no longer rides on the whole sum.)  One
// order on both routes, no atomics, no cross-lane sum: the same bits run to run.  The weights come from LDS at one address
// for all lanes (a broadcast); with two outputs a pixel's two accumulators form one packed float32 pair.  expf, log1pf and
// the division are the accurate library forms (csrc/gru.hip says why).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"

namespace dba {

constexpr int UPD_THREADS = 256;
constexpr int UPD_TR = 16, UPD_TC = 64;   // the tile: rows x columns (dba_upd_heads_tile)
constexpr int UPD_PX = 4;                 // pixels of a row per lane
constexpr int UPD_CC = 4;                 // channels per staged chunk
constexpr int UPD_ROWS = UPD_TR + 2;      // slab rows
constexpr int UPD_STR = UPD_TC + 8;       // floats per slab row in LDS: column x of the tile at index x + 4, so a lane's four
                                          // pixels are one aligned float4 and the halo columns sit at 3 and TC + 4
constexpr int UPD_CH = UPD_ROWS * UPD_STR;
constexpr int UPD_WS = 12;                // floats per (channel, output) in LDS: 9 taps, padded to three float4
constexpr int UPD_NE = (UPD_ROWS * (UPD_TC + 2) + UPD_THREADS - 1) / UPD_THREADS;   // slab elements per lane and channel
static_assert(UPD_THREADS == UPD_TR * (UPD_TC / UPD_PX), "one lane per four pixels of the tile");

struct UpdHead {
  const void *x, *w, *b;
  void *out;
  float *sum;
  int k, relu_in, act;
  float scale;
  int out_f32;   // out is float32 whatever T: the activation's float32 value, not rounded
};

struct UpdHeads {
  UpdHead h[2];
  int n_heads;
};

template <typename T, int W>
struct alignas(sizeof(T) * W) UpdVec {
  T e[W];
};

typedef float upd_f2 __attribute__((ext_vector_type(2)));
typedef float upd_f4 __attribute__((ext_vector_type(4)));

// the extractor's ReLU: NaN goes through, -0 becomes +0
__device__ __forceinline__ float upd_relu(float x) { return x > 0.0f ? x : (x != x ? x : 0.0f); }

// a float32 result that is rounded to half next keeps its float32 rounding (csrc/extractor.hip: enc_f32)
__device__ __forceinline__ float upd_f32(float x) {
  asm("" : "+v"(x));
  return x;
}

template <typename T>
__device__ __forceinline__ float upd_rnd(float x) { return (float)(T)x; }

template <typename T>
__device__ __forceinline__ float upd_epilogue(float v, int act, float scale) {
  if (act == DBA_UPD_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
  if (act == DBA_UPD_ACT_SOFTPLUS) {
    const float sp = upd_rnd<T>(v > 20.0f ? v : log1pf(expf(v)));   // torch's softplus, beta 1, threshold 20
    return upd_f32(scale * sp);
  }
  return v;
}

// the head's value for a float32 `out` (autocast's softplus on a half convolution): v is already h(s + b); the activation and
// the scale stay in float32, nothing rounds behind them
__device__ __forceinline__ float upd_epilogue_f32(float v, int act, float scale) {
  if (act == DBA_UPD_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
  if (act == DBA_UPD_ACT_SOFTPLUS) return upd_f32(scale * upd_f32(v > 20.0f ? v : log1pf(expf(v))));
  return v;
}

template <typename T, int K, bool VEC>
__global__ __launch_bounds__(UPD_THREADS) void upd_heads_kernel(UpdHeads hs, int n, int c, int ht, int wd, unsigned tiles_x,
                                                                unsigned tiles) {
  constexpr int W = 16 / sizeof(T);
  constexpr int NV = ((UPD_ROWS * UPD_TC + W - 1) / W + 1 + UPD_THREADS - 1) / UPD_THREADS;   // slab vectors per lane and channel
  using VT = UpdVec<T, W>;
  __shared__ __attribute__((aligned(16))) float xs[UPD_CC * UPD_CH];
  __shared__ __attribute__((aligned(16))) float wl[UPD_CC * 2 * UPD_WS];

  // the workgroup's head, edge and tile; the head by selects on constant indices, so it stays in scalar registers
  const unsigned per_head = (unsigned)n * tiles;
  const bool second = hs.n_heads > 1 && blockIdx.x >= per_head;
  const unsigned local = blockIdx.x - (second ? per_head : 0u);
  const T *x = (const T *)(second ? hs.h[1].x : hs.h[0].x);
  const T *wt = (const T *)(second ? hs.h[1].w : hs.h[0].w);
  const T *bias = (const T *)(second ? hs.h[1].b : hs.h[0].b);
  T *out = (T *)(second ? hs.h[1].out : hs.h[0].out);
  float *sum = second ? hs.h[1].sum : hs.h[0].sum;
  const int k = second ? hs.h[1].k : hs.h[0].k;
  const int relu_in = second ? hs.h[1].relu_in : hs.h[0].relu_in;
  const int act = second ? hs.h[1].act : hs.h[0].act;
  const float scale = second ? hs.h[1].scale : hs.h[0].scale;
  const int out_f32 = second ? hs.h[1].out_f32 : hs.h[0].out_f32;

  const unsigned e = local / tiles, tile = local - e * tiles;
  const int ty = (int)(tile / tiles_x), tx = (int)(tile - (unsigned)ty * tiles_x);
  const int r0 = ty * UPD_TR, c0 = tx * UPD_TC;
  const int hw = ht * wd;
  const T *xe = x + (long long)e * c * hw;   // n * c * hw < 2^31 (host)
  const int tid = threadIdx.x;

  for (int i = tid; i < UPD_CC * UPD_CH; i += UPD_THREADS) xs[i] = 0.0f;
  if (tid < UPD_CC * 2 * UPD_WS) wl[tid] = 0.0f;

  // ---- where this lane's share of a channel's slab comes from and where it lands: worked out once ----
  int goff[VEC ? 1 : UPD_NE];    // elements: offset in the plane, -1 outside the map
  int eoff[VEC ? 1 : UPD_NE];    //           index in the channel's LDS slab
  int voff[VEC ? NV : 1];        // vectors: offset of the vector in the plane, -1 when the lane has none
  int loff[VEC ? NV * W : 1];    //          index of each element in the LDS slab, -1 when it is not part of the slab
  if constexpr (VEC) {
    const int y_lo = r0 - 1 < 0 ? 0 : r0 - 1, y_hi = r0 + UPD_TR + 1 > ht ? ht : r0 + UPD_TR + 1;
    const int f0 = y_lo * wd, f1 = y_hi * wd, a0 = f0 & ~(W - 1);
    const int n_vec = (f1 - a0 + W - 1) / W;   // the last vector ends inside the plane: hw is a multiple of W
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int v = tid + u * UPD_THREADS;
      const int g = a0 + v * W;
      voff[u] = v < n_vec ? g : -1;
      int row = g / wd, col = g - row * wd;
#pragma unroll
      for (int j = 0; j < W; j++) {
        const int f = g + j;
        loff[u * W + j] = (v < n_vec && f >= f0 && f < f1) ? (row - (r0 - 1)) * UPD_STR + col + 4 : -1;
        if (++col == wd) {
          col = 0;
          row++;
        }
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < UPD_NE; u++) {
      const int i = tid + u * UPD_THREADS;
      const int r = i / (UPD_TC + 2), cc = i - r * (UPD_TC + 2);
      const int gy = r0 - 1 + r, gx = c0 - 1 + cc;
      const bool ok = i < UPD_ROWS * (UPD_TC + 2) && gy >= 0 && gy < ht && gx >= 0 && gx < wd;
      goff[u] = ok ? gy * wd + gx : -1;
      eoff[u] = r * UPD_STR + cc + 3;
    }
  }
  // the lane's weight of a chunk: (channel of the chunk, output, tap)
  const int w_ch = tid / (K * 9), w_ko = (tid - w_ch * (K * 9)) / 9, w_tap = tid - w_ch * (K * 9) - w_ko * 9;
  const bool w_lane = tid < UPD_CC * K * 9 && w_ko < k;

  T ev[VEC ? 1 : UPD_CC][VEC ? 1 : UPD_NE];
  VT vv[VEC ? UPD_CC : 1][VEC ? NV : 1];
  float wreg = 0.0f;

  auto load_chunk = [&](int cb) {
#pragma unroll
    for (int ch = 0; ch < UPD_CC; ch++) {
      if (cb + ch >= c) break;
      const T *plane = xe + (long long)(cb + ch) * hw;
      if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < NV; u++)
          if (voff[u] >= 0) vv[ch][u] = *(const VT *)(plane + voff[u]);
      } else {
#pragma unroll
        for (int u = 0; u < UPD_NE; u++)
          if (goff[u] >= 0) ev[ch][u] = plane[goff[u]];
      }
    }
    wreg = (w_lane && cb + w_ch < c) ? (float)wt[((long long)w_ko * c + cb + w_ch) * 9 + w_tap] : 0.0f;
  };

  auto store_chunk = [&](int cb) {
#pragma unroll
    for (int ch = 0; ch < UPD_CC; ch++) {
      if (cb + ch >= c) break;
      float *slab = xs + ch * UPD_CH;
      if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < NV; u++)
          if (voff[u] >= 0) {
#pragma unroll
            for (int j = 0; j < W; j++)
              if (loff[u * W + j] >= 0) {
                const float f = (float)vv[ch][u].e[j];
                slab[loff[u * W + j]] = relu_in ? upd_relu(f) : f;
              }
          }
      } else {
#pragma unroll
        for (int u = 0; u < UPD_NE; u++)
          if (goff[u] >= 0) {
            const float f = (float)ev[ch][u];
            slab[eoff[u]] = relu_in ? upd_relu(f) : f;
          }
      }
    }
    if (tid < UPD_CC * K * 9) wl[(w_ch * 2 + w_ko) * UPD_WS + w_tap] = wreg;
  };

  const int lr = tid / (UPD_TC / UPD_PX), lj = tid - lr * (UPD_TC / UPD_PX);
  const float *mine = xs + lr * UPD_STR + UPD_PX * lj + 3;   // column 4 lj - 1 of the lane's row - 1
  constexpr int N_ACC = K == 2 ? UPD_PX : UPD_PX / 2;
  upd_f2 acc[N_ACC];                                         // K == 2: (output 0, output 1) of a pixel; K == 1: two pixels
#pragma unroll
  for (int p = 0; p < N_ACC; p++) acc[p] = (upd_f2){0.0f, 0.0f};

  load_chunk(0);
  for (int cb = 0; cb < c; cb += UPD_CC) {
    __syncthreads();   // the zeros, or the chunk before, have been read
    store_chunk(cb);
    __syncthreads();
    if (cb + UPD_CC < c) load_chunk(cb + UPD_CC);
    upd_f2 part[N_ACC];   // the chunk's own sum, from +0
#pragma unroll
    for (int p = 0; p < N_ACC; p++) part[p] = (upd_f2){0.0f, 0.0f};
#pragma unroll
    for (int ch = 0; ch < UPD_CC; ch++) {
      if (cb + ch >= c) break;
      float wv[K][UPD_WS];
#pragma unroll
      for (int ko = 0; ko < K; ko++) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const upd_f4 t = *(const upd_f4 *)(wl + (ch * 2 + ko) * UPD_WS + 4 * q);
          wv[ko][4 * q] = t.x;
          wv[ko][4 * q + 1] = t.y;
          wv[ko][4 * q + 2] = t.z;
          wv[ko][4 * q + 3] = t.w;
        }
      }
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const float *row = mine + ch * UPD_CH + ky * UPD_STR;
        const upd_f4 m = *(const upd_f4 *)(row + 1);
        const float xv[UPD_PX + 2] = {row[0], m.x, m.y, m.z, m.w, row[UPD_PX + 1]};
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          if constexpr (K == 2) {
            const upd_f2 w2 = {wv[0][ky * 3 + kx], wv[1][ky * 3 + kx]};
#pragma unroll
            for (int p = 0; p < UPD_PX; p++) part[p] = part[p] + (upd_f2){xv[p + kx], xv[p + kx]} * w2;
          } else {
            const float w1 = wv[0][ky * 3 + kx];
#pragma unroll
            for (int p = 0; p < UPD_PX / 2; p++)
              part[p] = part[p] + (upd_f2){xv[2 * p + kx], xv[2 * p + 1 + kx]} * (upd_f2){w1, w1};
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < N_ACC; p++) acc[p] = acc[p] + part[p];
  }

  // ---- v = h(s + b), the head's own epilogue, the k outputs of a pixel side by side ----
  const int gy = r0 + lr;
  if (gy >= ht) return;
  const float b0 = bias ? (float)bias[0] : 0.0f, b1 = (bias && k == 2) ? (float)bias[1] : 0.0f;
  const bool pairs = k == 2 && ((uintptr_t)out % (2 * sizeof(T))) == 0;
#pragma unroll
  for (int p = 0; p < UPD_PX; p++) {
    const int gx = c0 + UPD_PX * lj + p;
    if (gx >= wd) continue;
    const long long pix = ((long long)e * ht + gy) * wd + gx;
    float s0, s1 = 0.0f;
    if constexpr (K == 2) {
      s0 = acc[p].x;
      s1 = acc[p].y;
    } else {
      s0 = (p & 1) ? acc[p / 2].y : acc[p / 2].x;
    }
    s0 = upd_f32(s0 + b0);
    s1 = upd_f32(s1 + b1);
    if (out_f32) {   // uniform over the workgroup
      float *of = (float *)out;
      of[(long long)k * pix] = upd_epilogue_f32(upd_rnd<T>(s0), act, scale);
      if (k == 2) of[2 * pix + 1] = upd_epilogue_f32(upd_rnd<T>(s1), act, scale);
      if (sum) {
        sum[(long long)k * pix] = s0;
        if (k == 2) sum[2 * pix + 1] = s1;
      }
      continue;
    }
    const T o0 = (T)upd_epilogue<T>(upd_rnd<T>(s0), act, scale);
    if (k == 2) {
      const T o1 = (T)upd_epilogue<T>(upd_rnd<T>(s1), act, scale);
      if (pairs) {
        UpdVec<T, 2> o;
        o.e[0] = o0;
        o.e[1] = o1;
        *(UpdVec<T, 2> *)(out + 2 * pix) = o;
      } else {
        out[2 * pix] = o0;
        out[2 * pix + 1] = o1;
      }
      if (sum) {
        sum[2 * pix] = s0;
        sum[2 * pix + 1] = s1;
      }
    } else {
      out[pix] = o0;
      if (sum) sum[pix] = s0;
    }
  }
}

}  // namespace dba

using namespace dba;

namespace {

template <typename T, int K>
int launch_heads(const UpdHeads &hs, bool vec, int n, int c, int ht, int wd, unsigned tiles_x, unsigned tiles, unsigned grid,
                 hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((upd_heads_kernel<T, K, true>), dim3(grid), dim3(UPD_THREADS), 0, s, hs, n, c, ht, wd, tiles_x, tiles);
  else
    hipLaunchKernelGGL((upd_heads_kernel<T, K, false>), dim3(grid), dim3(UPD_THREADS), 0, s, hs, n, c, ht, wd, tiles_x, tiles);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace

extern "C" {

int dba_upd_heads_tile(int *rows, int *cols) {
  if (!rows || !cols) return DBA_ERR_ARG;
  *rows = UPD_TR;
  *cols = UPD_TC;
  return DBA_OK;
}

int dba_upd_heads(const dba_upd_head_t *heads, int n_heads, int n, int c, int ht, int wd, int dtype, dba_stream_t stream) {
  const int isz = dtype == DBA_F16 ? 2 : dtype == DBA_F32 ? 4 : 0;
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!heads || n_heads < 1 || n_heads > 2 || n <= 0 || c <= 0 || ht <= 0 || wd <= 0) return DBA_ERR_ARG;
  if ((long long)ht * wd > (long long)INT32_MAX || (long long)n * c > (long long)INT32_MAX / ((long long)ht * wd))
    return DBA_ERR_ARG;   // n * c * ht * wd beyond 2^31 - 1
  const long long tiles_x = (wd + UPD_TC - 1) / UPD_TC, tiles = tiles_x * ((ht + UPD_TR - 1) / UPD_TR);
  if (tiles * n * n_heads > (long long)INT32_MAX) return DBA_ERR_ARG;
  const long long hw = (long long)ht * wd, xbytes = (long long)n * c * hw * isz;
  UpdHeads hs{};
  hs.n_heads = n_heads;
  bool vec = wd <= UPD_TC && (hw * isz) % 16 == 0;
  int kmax = 1;
  for (int i = 0; i < n_heads; i++) {
    const dba_upd_head_t &h = heads[i];
    if (!h.x || !h.weight || !h.out || (h.k != 1 && h.k != 2)) return DBA_ERR_ARG;
    if (h.act != DBA_UPD_ACT_NONE && h.act != DBA_UPD_ACT_SIGMOID && h.act != DBA_UPD_ACT_SOFTPLUS) return DBA_ERR_ARG;
    if (((uintptr_t)h.x | (uintptr_t)h.weight | (uintptr_t)h.bias) % isz || (uintptr_t)h.out % (h.out_f32 ? 4 : isz) ||
        (uintptr_t)h.sum % 4)
      return DBA_ERR_ARG;
    hs.h[i] = UpdHead{h.x, h.weight, h.bias, h.out, h.sum, h.k, h.relu_in != 0, h.act, h.scale, h.out_f32 != 0};
    vec = vec && ((uintptr_t)h.x & 15) == 0;
    kmax = h.k > kmax ? h.k : kmax;
  }
  // what a head writes shares no byte with anything the call reads, nor with what else it writes
  for (int i = 0; i < n_heads; i++) {
    const dba_upd_head_t &h = heads[i];
    const long long obytes = (long long)n * hw * h.k * (h.out_f32 ? 4 : isz), sbytes = (long long)n * hw * h.k * 4;
    if (ranges_overlap(h.out, obytes, h.sum, sbytes)) return DBA_ERR_ARG;
    for (int j = 0; j < n_heads; j++) {
      const dba_upd_head_t &g = heads[j];
      const long long wbytes = (long long)g.k * c * 9 * isz, bbytes = (long long)g.k * isz;
      for (int o = 0; o < 2; o++) {
        const void *p = o ? (const void *)h.sum : (const void *)h.out;
        const long long pbytes = o ? sbytes : obytes;
        if (ranges_overlap(p, pbytes, g.x, xbytes) || ranges_overlap(p, pbytes, g.weight, wbytes) ||
            ranges_overlap(p, pbytes, g.bias, bbytes))
          return DBA_ERR_ARG;
        if (j != i && (ranges_overlap(p, pbytes, g.out, (long long)n * hw * g.k * (g.out_f32 ? 4 : isz)) ||
                       ranges_overlap(p, pbytes, g.sum, (long long)n * hw * g.k * 4)))
          return DBA_ERR_ARG;
      }
    }
  }
  const unsigned grid = (unsigned)(tiles * n * n_heads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DBA_F16)
    return kmax == 2 ? launch_heads<_Float16, 2>(hs, vec, n, c, ht, wd, (unsigned)tiles_x, (unsigned)tiles, grid, s)
                     : launch_heads<_Float16, 1>(hs, vec, n, c, ht, wd, (unsigned)tiles_x, (unsigned)tiles, grid, s);
  return kmax == 2 ? launch_heads<float, 2>(hs, vec, n, c, ht, wd, (unsigned)tiles_x, (unsigned)tiles, grid, s)
                   : launch_heads<float, 1>(hs, vec, n, c, ht, wd, (unsigned)tiles_x, (unsigned)tiles, grid, s);
}

}  // extern "C"
