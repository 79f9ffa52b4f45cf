// The encoders' convolutions (dbaf/modules/extractor.py) on the matrix cores, half tensors in the modules' NCHW layout
// (include/dba_hip.h "The encoders' convolutions"):
//   dba_conv3x3s_f16       <- nn.Conv2d(C_in, C_out, 3, stride=s, padding=1)(x), s = 1 or 2, optionally torch.relu behind it
//   dba_conv3x3s_down_f16  <- a stride-2 block's conv1(x) (optionally through torch.relu) AND its downsample[0](x) =
//                             nn.Conv2d(C_in, C_out, 1, stride=2)(x), one launch, x read once
//   dba_conv7x7s2_f16      <- the stem nn.Conv2d(3, C_out, 7, stride=2, padding=3)(x.half()), optionally torch.relu behind it
//
// conv3x3s_kernel<S, SPLIT, DOWN>: conv_mfma.h's GEMM with N = 16 consecutive OUTPUT pixels of a row and K = 32 input
// channels of one tap.  C_in % 32 == 0, C_out % 32 == 0.
//   - tile: 16 output columns x TR output rows, TR = 16 at stride 1 and 8 at stride 2.  With its halo a tile reads
//     ((TR - 1) S + 3) x (15 S + 3) input pixels: 18 x 18 (25.9 KB of LDS a chunk) at stride 1, 17 x 33 (44.9 KB) at stride 2
//     -- a 16 x 16 tile at stride 2 would need 33 x 33 pixels, 87 KB, and one workgroup per CU; at 8 rows two workgroups
//     share a CU's 160 KB as in conv3x3.hip (amdgpu_waves_per_eu(2, 2)) and one stages while the other multiplies;
//   - a workgroup's channels: 64 (wave g: channels 16 g .., all TR rows) where C_out % 64 == 0; else SPLIT: 32 channels, the
//     four waves as two channel groups of 16 x two halves of the tile's rows.  A wave always walks ITS rows with the same
//     loops, so an output element's accumulation order does not depend on the split;
//   - staging: conv3x3.hip's.  A chunk of 32 channels goes through LDS transposed at the 80-byte pitch, a thread takes one
//     pixel and 8 channels; positions outside the image are zeros and are never dereferenced;
//   - fragments: B for output row o, tap (ky, kx) is the fragment of halo row S o + ky at pixel S r + kx for lane r: with
//     stride 2 lane r reads pixel 2 r + kx.  A (halo row, kx) fragment is read ONCE and feeds the taps ky that use it;
//   - accumulation order of an output element, fixed: chunks ascending; inside a chunk kx = 0, 1, 2; inside kx ky = 0, 1, 2;
//     inside an MFMA the hardware's order over its 32 channels.  float32 throughout, no atomics;
//   - DOWN (stride 2): downsample[0] reads input pixel (2 y, 2 x), which is conv1's centre tap (ky = kx = 1) at stride 2
//     with padding 1, and both outputs have floor((H - 1) / 2) + 1 rows.  The centre-tap fragments feed a second set of
//     accumulators with the TENTH weight slice; order of an out2 element: chunks ascending.  out2 never takes the ReLU;
//   - epilogue: c = mf_round(acc, bias), out = mf_relu(c).
//
// conv7x7s2_kernel<T>: conv7x7.hip's scheme at stride 2 for THREE input channels.  K = one kernel row: 8 tap slots x 4
// channel slots; the fourth channel slot and the eighth tap slot are zero in the packed weights AND in the fragment (the
// fourth channel is staged as zero; the eighth tap would be pixel 2 x + 4, real data right of the footprint, and the lane
// replaces it with zeros: NaN * 0 and inf * 0 are NaN).  C_out % 32 == 0.  T is the input's element type, half_t or float.
//   - tile: 16 x 16 output pixels, 32 channels a workgroup, the waves split 2 x 2 as above (8 rows each);
//   - staging: the tile's 37 x 37 input pixels ONCE as [row][pixel][4], 8 bytes a pixel, 10.7 KB, and one zero pixel behind
//     them (slot 7 of the last row's lane r = 15 reads there).  float32 is rounded to nearest even as it arrives (beyond
//     65504 to infinity: the bytes of .to(torch.float16)).  Positions outside the image are zeros, never dereferenced;
//   - fragments: lane (r, q) of output row y, kernel row ky: halo row 2 y + ky, pixels 2 r + 2 q and 2 r + 2 q + 1, 16
//     contiguous bytes, 8-byte aligned (two 8-byte reads).  A halo row's fragment is read once and feeds every ky using it;
//   - accumulation order of an output element, fixed: ky = 0 .. 6 ascending; inside an MFMA the hardware's order.
// Built with -ffp-contract=off as the other matrix-core convolutions.  Resources: profiles/conv_enc_resources.txt.
#include "conv_mfma.h"

namespace dba {

typedef half_t half4 __attribute__((ext_vector_type(4)));

constexpr int EN_TC = 16;                 // a tile's output columns: N of one MFMA

template <int S>
struct EnTile {
  static constexpr int TR = S == 1 ? 16 : 8;                              // output rows
  static constexpr int HR = (TR - 1) * S + 3;                             // input rows with the halo
  static constexpr int HC = (EN_TC - 1) * S + 3;                          // input columns with the halo
  static constexpr int HP = HR * HC;                                      // staged pixels: 324, 561
  static constexpr int ITEMS = HP * (MF_KC / 8);                          // (pixel, 8 channels) items of a chunk
  static constexpr int STAGE = (ITEMS + MF_THREADS - 1) / MF_THREADS;     // per thread: 6, 9
};

struct EncArgs {
  const half_t *x;                 // [n, c_in, h, w]
  const half_t *w, *bias, *bias2;  // [9 or 10][c_out][c_in]; [c_out] or null each
  int c_in, c_out, n, h, wd, oh, ow, tiles_x, tiles;
  half_t *out, *out2;              // [n, c_out, oh, ow]
  int relu;
};

template <int S, bool SPLIT, bool DOWN>
__global__ __launch_bounds__(MF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3s_kernel(const EncArgs a) {
  using T = EnTile<S>;
  constexpr int WR = SPLIT ? T::TR / 2 : T::TR;   // output rows of a wave
  constexpr int WH = (WR - 1) * S + 3;            // halo rows a wave reads
  __shared__ __attribute__((aligned(16))) half_t xs[T::HP * MF_XS];
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty0 = (tile / a.tiles_x) * T::TR, tx0 = (tile - (tile / a.tiles_x) * a.tiles_x) * EN_TC;
  const int HW = a.h * a.wd, OHW = a.oh * a.ow;
  const int co0 = SPLIT ? blockIdx.y * 32 + (g & 1) * 16 : blockIdx.y * 64 + g * 16;   // the wave's first output channel
  const int row0 = SPLIT ? (g >> 1) * WR : 0;                                          // and its first output row in the tile
  const int rows = min(WR, a.oh - ty0 - row0);              // the wave's output rows inside the image (uniform, may be <= 0)
  const int live = rows > 0 ? (rows - 1) * S + 3 : 0;       // the halo rows that feed them

  // where this thread's staging items lie: fixed over the chunks
  int s_lds[T::STAGE], s_off[T::STAGE];   // LDS half index; offset inside the chunk's planes, -1: zero
#pragma unroll
  for (int k = 0; k < T::STAGE; ++k) {
    const int it = threadIdx.x + k * MF_THREADS;
    const int cg = it / T::HP, p = it - cg * T::HP;
    const int iy = p / T::HC, ix = p - iy * T::HC;
    const int gy = ty0 * S - 1 + iy, gx = tx0 * S - 1 + ix;
    const bool ok = it < T::ITEMS && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
    s_lds[k] = it < T::ITEMS ? p * MF_XS + cg * 8 : -1;
    s_off[k] = ok ? cg * 8 * HW + gy * a.wd + gx : -1;
  }

  float4v acc[WR], acc2[DOWN ? WR : 1];
#pragma unroll
  for (int o = 0; o < WR; ++o) acc[o] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < (DOWN ? WR : 1); ++o) acc2[o] = float4v{0.f, 0.f, 0.f, 0.f};

  const half_t *wrow = a.w + (size_t)(co0 + r) * a.c_in + q * 8;   // + tap * c_out * c_in + chunk * 32
  const size_t tap_stride = (size_t)a.c_out * a.c_in;
  const half_t *xw = xs + row0 * S * T::HC * MF_XS;                // the wave's first halo row

#pragma unroll 1
  for (int ch0 = 0; ch0 < a.c_in; ch0 += MF_KC) {
    const half_t *planes = a.x + ((size_t)img * a.c_in + ch0) * HW;
    half8 v[T::STAGE];
#pragma unroll
    for (int k = 0; k < T::STAGE; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = s_off[k] >= 0 ? planes[(size_t)s_off[k] + (size_t)j * HW] : (half_t)0.f;
    }
    __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
    for (int k = 0; k < T::STAGE; ++k)
      if (s_lds[k] >= 0) *reinterpret_cast<half8 *>(&xs[s_lds[k]]) = v[k];
    __syncthreads();

#pragma unroll 1
    for (int kx = 0; kx < 3; ++kx) {
      half8 wa[3], wc{};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) wa[ky] = *reinterpret_cast<const half8 *>(wrow + (size_t)(ky * 3 + kx) * tap_stride + ch0);
      if (DOWN && kx == 1) wc = *reinterpret_cast<const half8 *>(wrow + (size_t)9 * tap_stride + ch0);
#pragma unroll
      for (int ir = 0; ir < WH; ++ir) {
        if (ir >= live) continue;   // uniform: halo rows that only feed output rows outside the image
        const half8 xb = mf_fragment(xw, ir * T::HC + S * r + kx, q);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          if (ir < ky || (ir - ky) % S || (ir - ky) / S >= WR) continue;   // compile time
          const int o = (ir - ky) / S;
          acc[o] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ky], xb, acc[o], 0, 0, 0);
          if (DOWN && kx == 1 && ky == 1) acc2[o] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc, xb, acc2[o], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: lane = output column r, channels co0 + 4q + i
  const int x = tx0 + r;
  if (x >= a.ow) return;
  float bf[4], bf2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bf[i] = mf_bias(a.bias, co0 + 4 * q + i);
    bf2[i] = DOWN ? mf_bias(a.bias2, co0 + 4 * q + i) : 0.f;
  }
  const size_t first = ((size_t)img * a.c_out + co0 + 4 * q) * OHW + x;
#pragma unroll
  for (int o = 0; o < WR; ++o) {
    if (o >= rows) continue;   // uniform
    const int pix = (ty0 + row0 + o) * a.ow;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a.out[first + (size_t)i * OHW + pix] = mf_relu(mf_round(acc[o][i], bf[i]), a.relu);
      if (DOWN) a.out2[first + (size_t)i * OHW + pix] = mf_round(acc2[o][i], bf2[i]);
    }
  }
}

// ---- the stem

constexpr int ES_T = 16;                          // the tile's output rows and columns
constexpr int ES_K = 7;                           // kernel rows and taps
constexpr int ES_H = (ES_T - 1) * 2 + ES_K;       // input rows and columns with the halo: 37
constexpr int ES_HP = ES_H * ES_H;                // staged pixels: 1369
constexpr int ES_PIX = ES_HP + 1;                 // and the zero pixel behind them
constexpr int ES_STAGE = (ES_PIX + MF_THREADS - 1) / MF_THREADS;   // pixels per thread: 6
constexpr int ES_C = 3;                           // input channels, and nothing else
constexpr int ES_WR = ES_T / 2;                   // output rows of a wave
constexpr int ES_WH = (ES_WR - 1) * 2 + ES_K;     // halo rows a wave reads: 21

struct EncStemArgs {
  const void *x;               // [n, 3, h, w] half or float32
  const half_t *w, *bias;      // [7][c_out][32]; [c_out] or null
  int c_out, n, h, wd, oh, ow, tiles_x, tiles;
  half_t *out;                 // [n, c_out, oh, ow]
  int relu;
};

template <class T>
__global__ __launch_bounds__(MF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv7x7s2_kernel(const EncStemArgs a) {
  __shared__ __attribute__((aligned(16))) half_t xs[ES_PIX * 4];
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty0 = (tile / a.tiles_x) * ES_T, tx0 = (tile - (tile / a.tiles_x) * a.tiles_x) * ES_T;
  const int HW = a.h * a.wd, OHW = a.oh * a.ow;
  const int co0 = blockIdx.y * 32 + (g & 1) * 16, row0 = (g >> 1) * ES_WR;
  const int rows = min(ES_WR, a.oh - ty0 - row0);           // uniform, may be <= 0
  const int live = rows > 0 ? (rows - 1) * 2 + ES_K : 0;

  // ---- staging: one pixel, three channels and a zero, one 8-byte LDS vector
  const T *image = static_cast<const T *>(a.x) + (size_t)img * ES_C * HW;
#pragma unroll
  for (int k = 0; k < ES_STAGE; ++k) {
    const int p = threadIdx.x + k * MF_THREADS;
    if (p >= ES_PIX) continue;
    const int iy = p / ES_H, ix = p - iy * ES_H;
    const int gy = ty0 * 2 - 3 + iy, gx = tx0 * 2 - 3 + ix;
    const bool ok = p < ES_HP && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
    half4 v;
#pragma unroll
    for (int j = 0; j < ES_C; ++j) v[j] = ok ? (half_t)image[(size_t)j * HW + (gy * a.wd + gx)] : (half_t)0.f;
    v[3] = (half_t)0.f;
    *reinterpret_cast<half4 *>(&xs[p * 4]) = v;
  }

  // ---- A: the wave's weights of every kernel row
  half8 wa[ES_K];
  const half_t *wrow = a.w + (size_t)(co0 + r) * MF_KC + q * 8;   // + ky * c_out * 32
#pragma unroll
  for (int ky = 0; ky < ES_K; ++ky) wa[ky] = *reinterpret_cast<const half8 *>(wrow + (size_t)ky * a.c_out * MF_KC);

  float4v acc[ES_WR];
#pragma unroll
  for (int o = 0; o < ES_WR; ++o) acc[o] = float4v{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  const half4 zero4 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
  const half_t *frag = xs + (row0 * 2 * ES_H + 2 * r + 2 * q) * 4;
#pragma unroll
  for (int ir = 0; ir < ES_WH; ++ir) {
    if (ir >= live) continue;   // uniform
    const half4 lo = *reinterpret_cast<const half4 *>(frag + ir * ES_H * 4);
    half4 hi = *reinterpret_cast<const half4 *>(frag + ir * ES_H * 4 + 4);
    hi = q == 3 ? zero4 : hi;   // slot 7: pixel 2 x + 4 is not in the footprint
    const half8 xb = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int ky = 0; ky < ES_K; ++ky) {
      if (ir < ky || (ir - ky) % 2 || (ir - ky) / 2 >= ES_WR) continue;   // compile time
      const int o = (ir - ky) / 2;
      acc[o] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ky], xb, acc[o], 0, 0, 0);
    }
  }

  // ---- epilogue: lane = output column r, channels co0 + 4q + i
  const int x = tx0 + r;
  if (x >= a.ow) return;
  float bf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bf[i] = mf_bias(a.bias, co0 + 4 * q + i);
  half_t *dst = a.out + ((size_t)img * a.c_out + co0 + 4 * q) * OHW + x;
#pragma unroll
  for (int o = 0; o < ES_WR; ++o) {
    if (o >= rows) continue;   // uniform
    const int pix = (ty0 + row0 + o) * a.ow;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(size_t)i * OHW + pix] = mf_relu(mf_round(acc[o][i], bf[i]), a.relu);
  }
}

}  // namespace dba

using namespace dba;

namespace {

inline int en_out(int extent, int stride) { return (extent - 1) / stride + 1; }   // kernel 2 pad + 1: floor((e - 1) / s) + 1

// the checks the two 3x3 entry points share
int en_input(EncArgs &a, const void *x, const void *w, const void *bias, int c_in, int c_out, int n, int h, int wd, int stride) {
  if (n <= 0 || h <= 0 || wd <= 0 || c_in <= 0 || c_out <= 0) return DBA_ERR_ARG;
  if (stride != 1 && stride != 2) return DBA_ERR_ARG;
  if (c_in % 32 || c_out % 32) return DBA_ERR_ARG;
  if (!x || !w) return DBA_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)bias) & 1) return DBA_ERR_ARG;
  if ((uintptr_t)w & 15) return DBA_ERR_ARG;
  const long long hw = (long long)h * wd;
  if (hw * (c_in > c_out ? c_in : c_out) > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const int oh = en_out(h, stride), ow = en_out(wd, stride), tr = stride == 1 ? EnTile<1>::TR : EnTile<2>::TR;
  const long long tiles_x = (ow + EN_TC - 1) / EN_TC, tiles = tiles_x * ((oh + tr - 1) / tr);
  if (!mf_grid_ok(tiles, n, c_out) || c_out / 32 > 65535) return DBA_ERR_ARG;
  a.x = (const half_t *)x;
  a.w = (const half_t *)w;
  a.bias = (const half_t *)bias;
  a.c_in = c_in;
  a.c_out = c_out;
  a.n = n;
  a.h = h;
  a.wd = wd;
  a.oh = oh;
  a.ow = ow;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  return DBA_OK;
}

// a written tensor [n, c_out, oh, ow] must not share a byte with anything the launch reads
bool en_clobbers(const EncArgs &a, const void *dst, int taps) {
  const size_t bytes = (size_t)a.n * a.c_out * a.oh * a.ow * 2;
  return ranges_overlap(dst, bytes, a.x, (size_t)a.n * a.c_in * a.h * a.wd * 2) ||
         ranges_overlap(dst, bytes, a.w, (size_t)taps * a.c_out * a.c_in * 2) ||
         ranges_overlap(dst, bytes, a.bias, (size_t)a.c_out * 2) || ranges_overlap(dst, bytes, a.bias2, (size_t)a.c_out * 2);
}

template <auto Wide, auto Split>
int en_launch(const EncArgs &a, hipStream_t s) {
  const bool wide = a.c_out % 64 == 0;
  const dim3 grid((unsigned)((long long)a.tiles * a.n), (unsigned)(a.c_out / (wide ? 64 : 32)));
  if (wide)
    hipLaunchKernelGGL(Wide, grid, dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(Split, grid, dim3(MF_THREADS), 0, s, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace

extern "C" {

int dba_conv3x3s_tile_rows(int stride) { return stride == 1 ? EnTile<1>::TR : stride == 2 ? EnTile<2>::TR : 0; }
int dba_conv3x3s_tile_cols(void) { return EN_TC; }
int dba_conv7x7s2_tile(void) { return ES_T; }

int dba_conv3x3s_f16(const void *x, const void *weight, const void *bias, int c_in, int c_out, int n, int h, int w, int stride,
                     int relu, void *out, dba_stream_t stream) {
  EncArgs a{};
  const int rc = en_input(a, x, weight, bias, c_in, c_out, n, h, w, stride);
  if (rc != DBA_OK) return rc;
  if (!out || ((uintptr_t)out & 1) || en_clobbers(a, out, 9)) return DBA_ERR_ARG;
  a.out = (half_t *)out;
  a.relu = relu != 0;
  if (stride == 1) return en_launch<conv3x3s_kernel<1, false, false>, conv3x3s_kernel<1, true, false>>(a, (hipStream_t)stream);
  return en_launch<conv3x3s_kernel<2, false, false>, conv3x3s_kernel<2, true, false>>(a, (hipStream_t)stream);
}

int dba_conv3x3s_down_f16(const void *x, const void *weight, const void *bias, const void *bias_down, int c_in, int c_out, int n,
                          int h, int w, int relu, void *out, void *out_down, dba_stream_t stream) {
  EncArgs a{};
  const int rc = en_input(a, x, weight, bias, c_in, c_out, n, h, w, 2);
  if (rc != DBA_OK) return rc;
  if (!out || !out_down || (((uintptr_t)out | (uintptr_t)out_down | (uintptr_t)bias_down) & 1)) return DBA_ERR_ARG;
  a.bias2 = (const half_t *)bias_down;
  const size_t bytes = (size_t)n * c_out * a.oh * a.ow * 2;
  if (en_clobbers(a, out, 10) || en_clobbers(a, out_down, 10) || ranges_overlap(out, bytes, out_down, bytes)) return DBA_ERR_ARG;
  a.out = (half_t *)out;
  a.out2 = (half_t *)out_down;
  a.relu = relu != 0;
  return en_launch<conv3x3s_kernel<2, false, true>, conv3x3s_kernel<2, true, true>>(a, (hipStream_t)stream);
}

int dba_conv7x7s2_f16(const void *x, int dtype, const void *weight, const void *bias, int c_out, int n, int h, int w, int relu,
                      void *out, dba_stream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c_out <= 0 || c_out % 32) return DBA_ERR_ARG;
  if (dtype != DBA_F16 && dtype != DBA_F32) return DBA_ERR_ARG;
  if (!x || !weight || !out) return DBA_ERR_ARG;
  const size_t esz = dtype == DBA_F32 ? 4 : 2;
  if (((uintptr_t)x & (esz - 1)) || (((uintptr_t)bias | (uintptr_t)out) & 1) || ((uintptr_t)weight & 15)) return DBA_ERR_ARG;
  const long long hw = (long long)h * w;
  if (hw * (c_out > ES_C ? c_out : ES_C) > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const int oh = en_out(h, 2), ow = en_out(w, 2);
  const long long tiles_x = (ow + ES_T - 1) / ES_T, tiles = tiles_x * ((oh + ES_T - 1) / ES_T);
  if (!mf_grid_ok(tiles, n, c_out) || c_out / 32 > 65535) return DBA_ERR_ARG;
  const size_t obytes = (size_t)n * c_out * oh * ow * 2;
  if (ranges_overlap(out, obytes, x, (size_t)n * ES_C * hw * esz) ||
      ranges_overlap(out, obytes, weight, (size_t)ES_K * c_out * MF_KC * 2) || ranges_overlap(out, obytes, bias, (size_t)c_out * 2))
    return DBA_ERR_ARG;
  EncStemArgs a{};
  a.x = x;
  a.w = (const half_t *)weight;
  a.bias = (const half_t *)bias;
  a.c_out = c_out;
  a.n = n;
  a.h = h;
  a.wd = w;
  a.oh = oh;
  a.ow = ow;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  a.out = (half_t *)out;
  a.relu = relu != 0;
  const dim3 grid((unsigned)(tiles * n), (unsigned)(c_out / 32));
  if (dtype == DBA_F32)
    hipLaunchKernelGGL(conv7x7s2_kernel<float>, grid, dim3(MF_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv7x7s2_kernel<half_t>, grid, dim3(MF_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
