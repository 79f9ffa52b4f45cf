// The 7x7 flow stem (stride 1, zero padding 3) of a FOUR-channel map in the modules' NCHW layout on the matrix cores
// (include/dba_hip.h "7x7 convolution of four channels"):
//   dba_conv7x7_f16  <- nn.Conv2d(4, C_out, 7, padding=3)(x.half()), optionally torch.relu behind it
//
// conv7x7_kernel<MT, T>: conv_mfma.h's GEMM with N = 16 consecutive pixels of a map row and K = one KERNEL ROW: 7 taps and
// one zero slot, 4 channels each.  T is the input's element type, half_t or float.
//   - tile: 16 x 16 output pixels; a wave holds 16 x MT accumulator tiles of 4 floats (128 registers at MT = 2);
//   - staging: the tile's 22 x 22 input pixels (the tile and its halo of 3), ONCE, as [row][pixel][4 channels]: 8 bytes a
//     pixel, 3.9 KB.  A thread takes a pixel: 4 guarded element loads (plane bases are aligned to an element only), each
//     rounded to half as it arrives (float32: round to nearest even, beyond 65504 to infinity -- the bytes of the
//     .to(torch.float16) it replaces), one 8-byte LDS store.  Positions outside the image are zeros and are never
//     dereferenced.  Two pixels behind the last row are zeros as well: slot 7 of the last row's lane r = 15 reads there;
//   - fragments: B for kernel row ky, output row y and lane (r, q) is the 16 bytes at halo row y + ky, pixels r + 2q and
//     r + 2q + 1: taps kx = 2q, 2q + 1.  The address is 8-byte aligned, so it is read as two 8-byte halves.  The second
//     pixel of q = 3 would be tap 7: it is pixel x + 4, REAL data next to the footprint, and the lane replaces it with
//     zeros before the MFMA (the weight's zero would not do: NaN * 0 and inf * 0 are NaN).  A halo row's fragment is read
//     ONCE and feeds the seven kernel rows (output rows ir, ir - 1, .. ir - 6): 22 LDS reads per wave for 112 * MT MFMAs.
//     A for kernel row ky is 16 bytes of the packed weights [7][C_out][32] at [ky][channel l & 15][8 (l >> 4)], entry
//     [4 kx + i] = w[o, i, ky, kx] and zero for kx = 7; the 7 * MT fragments are read once per wave and stay in registers;
//   - accumulation order of an output element, fixed: ky = 0 .. 6 ascending; inside an MFMA the hardware's order over its
//     32 slots.  float32 throughout, no atomics: the same inputs give the same bits on every run;
//   - epilogue: c = mf_round(acc, bias), out = mf_relu(c).  A lane holds 4 consecutive channels of one pixel; a store
//     instruction writes 4 channel planes x 16 consecutive pixels.
// Built with -ffp-contract=off as the other matrix-core convolutions.  Resources: profiles/conv7x7_resources.txt.
#include "conv_mfma.h"

namespace dba {

typedef half_t half4 __attribute__((ext_vector_type(4)));

constexpr int S7_T = 16;                  // the tile's rows and columns
constexpr int S7_R = 3;                   // the halo
constexpr int S7_K = 2 * S7_R + 1;        // kernel rows and taps
constexpr int S7_H = S7_T + 2 * S7_R;     // with the halo: 22
constexpr int S7_HP = S7_H * S7_H;        // halo pixels: 484
constexpr int S7_PIX = S7_HP + 2;         // and the two zero pixels behind them
constexpr int S7_STAGE = (S7_PIX + MF_THREADS - 1) / MF_THREADS;   // pixels per thread: 2
constexpr int S7_C = 4;                   // input channels, and nothing else

struct StemArgs {
  const void *x;               // [n, 4, h, w] half or float32
  const half_t *w, *bias;      // [7][c_out][32]; [c_out] or null
  int c_out, n, h, wd, tiles_x, tiles;
  half_t *out;                 // [n, c_out, h, w]
  int relu;
};

template <int MT, class T>
__global__ __launch_bounds__(MF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv7x7_kernel(const StemArgs a) {
  __shared__ __attribute__((aligned(16))) half_t xs[S7_PIX * S7_C];
  const MfWave wv;
  const int r = wv.r, q = wv.q;
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty0 = (tile / a.tiles_x) * S7_T, tx0 = (tile - (tile / a.tiles_x) * a.tiles_x) * S7_T;
  const int HW = a.h * a.wd;
  const int co0 = wv.co0(MT);
  const int rows = min(S7_T, a.h - ty0);                    // output rows of the tile inside the image (uniform)

  // ---- staging: one pixel, four channels, one 8-byte LDS vector
  const T *image = static_cast<const T *>(a.x) + (size_t)img * S7_C * HW;
#pragma unroll
  for (int k = 0; k < S7_STAGE; ++k) {
    const int p = threadIdx.x + k * MF_THREADS;
    if (p >= S7_PIX) continue;
    const int iy = p / S7_H, ix = p - iy * S7_H;
    const int gy = ty0 - S7_R + iy, gx = tx0 - S7_R + ix;
    const bool ok = p < S7_HP && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
    half4 v;
#pragma unroll
    for (int j = 0; j < S7_C; ++j) v[j] = ok ? (half_t)image[(size_t)j * HW + (gy * a.wd + gx)] : (half_t)0.f;
    *reinterpret_cast<half4 *>(&xs[p * S7_C]) = v;
  }

  // ---- A: the wave's weights of every kernel row
  half8 wa[S7_K][MT];
  const half_t *wrow = a.w + (size_t)(co0 + r) * MF_KC + q * 8;   // + (ky * c_out + m * 16) * 32
#pragma unroll
  for (int ky = 0; ky < S7_K; ++ky)
#pragma unroll
    for (int m = 0; m < MT; ++m)
      wa[ky][m] = *reinterpret_cast<const half8 *>(wrow + ((size_t)ky * a.c_out + m * 16) * MF_KC);

  float4v acc[S7_T][MT];
#pragma unroll
  for (int o = 0; o < S7_T; ++o) mf_zero(acc[o]);
  __syncthreads();

  const half4 zero4 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
  const half_t *frag = xs + (r + 2 * q) * S7_C;
#pragma unroll
  for (int ir = 0; ir < S7_H; ++ir) {
    if (ir >= rows + 2 * S7_R) continue;   // uniform: halo rows that only feed output rows outside the image
    const half4 lo = *reinterpret_cast<const half4 *>(frag + ir * S7_H * S7_C);
    half4 hi = *reinterpret_cast<const half4 *>(frag + ir * S7_H * S7_C + S7_C);
    hi = q == 3 ? zero4 : hi;              // slot 7: pixel x + 4 is not in the footprint
    const half8 xb = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int ky = 0; ky < S7_K; ++ky) {
      const int o = ir - ky;
      if (o < 0 || o >= S7_T) continue;    // compile time
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ky][m], xb, acc[o][m], 0, 0, 0);
    }
  }

  // ---- epilogue: lane = pixel column r, channels co0 + m * 16 + 4q + i
  const int x = tx0 + r;
  if (x >= a.wd) return;
  float bf[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[m][i] = mf_bias(a.bias, co0 + m * 16 + 4 * q + i);
  half_t *dst = a.out + ((size_t)img * a.c_out + co0 + 4 * q) * HW + x;
#pragma unroll
  for (int o = 0; o < S7_T; ++o) {
    if (o >= rows) continue;   // uniform
    const int pix = (ty0 + o) * a.wd;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        dst[(size_t)(m * 16 + i) * HW + pix] = mf_relu(mf_round(acc[o][m][i], bf[m][i]), a.relu);
  }
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_conv7x7_tile(void) { return S7_T; }

int dba_conv7x7_f16(const void *x, int dtype, const void *weight, const void *bias, int c_out, int n, int h, int w, int relu,
                    void *out, dba_stream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c_out <= 0 || c_out % 64) return DBA_ERR_ARG;
  if (dtype != DBA_F16 && dtype != DBA_F32) return DBA_ERR_ARG;
  if (!x || !weight || !out) return DBA_ERR_ARG;
  const size_t esz = dtype == DBA_F32 ? 4 : 2;
  if (((uintptr_t)x & (esz - 1)) || (((uintptr_t)bias | (uintptr_t)out) & 1) || ((uintptr_t)weight & 15)) return DBA_ERR_ARG;
  const long long hw = (long long)h * w;
  if (hw * (c_out > S7_C ? c_out : S7_C) > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const long long tiles_x = (w + S7_T - 1) / S7_T, tiles = tiles_x * ((h + S7_T - 1) / S7_T);
  if (!mf_grid_ok(tiles, n, c_out)) return DBA_ERR_ARG;
  const size_t obytes = (size_t)n * c_out * hw * 2;
  if (ranges_overlap(out, obytes, x, (size_t)n * S7_C * hw * esz) ||
      ranges_overlap(out, obytes, weight, (size_t)S7_K * c_out * MF_KC * 2) || ranges_overlap(out, obytes, bias, (size_t)c_out * 2))
    return DBA_ERR_ARG;
  StemArgs a{};
  a.x = x;
  a.w = (const half_t *)weight;
  a.bias = (const half_t *)bias;
  a.c_out = c_out;
  a.n = n;
  a.h = h;
  a.wd = w;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  a.out = (half_t *)out;
  a.relu = relu != 0;
  if (dtype == DBA_F32) return mf_launch<conv7x7_kernel<2, float>, conv7x7_kernel<1, float>>(a, (hipStream_t)stream);
  return mf_launch<conv7x7_kernel<2, half_t>, conv7x7_kernel<1, half_t>>(a, (hipStream_t)stream);
}

}  // extern "C"
