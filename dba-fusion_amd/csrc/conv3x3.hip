// 3x3 convolutions (stride 1, zero padding 1) of half tensors in the modules' NCHW layout on the matrix cores, with the
// ConvGRU's gate arithmetic in the epilogue (include/dba_hip.h "3x3 convolutions"):
//   dba_conv3x3_f16        <- nn.Conv2d(C_in, C_out, 3, padding=1)(x), optionally torch.relu behind it
//   dba_conv3x3_pair_f16   <- two such convolutions of one input, each into a tensor of its own (the heads' delta[0], weight[0])
//   dba_conv3x3_gates_f16  <- z = sigmoid(convz(x) + gz); r = sigmoid(convr(x) + gr); r * net       (dbaf/modules/gru.py:27-29)
//   dba_conv3x3_blend_f16  <- q = tanh(convq(cat([r*net, inp])) + gq); (1 - z) * net + z * q          (gru.py:29-31)
//
// conv3x3_kernel<MT, EPI>: conv_mfma.h's GEMM with N = 16 consecutive pixels of a map row and K = 32 input channels of one tap.
//   - tile: 16 x 16 output pixels; a wave holds 16 x MT accumulator tiles of 4 floats (128 registers at MT = 2);
//   - staging: c0 and c1 are multiples of 32, so a chunk lies in ONE of the two sources.  The workgroup stages the chunk's
//     18 x 18 pixels (the tile and its one-pixel halo) once.  Positions outside the image are zeros: the map's borders, the
//     tail of a row and the tail of the last image.  One buffer, two barriers per chunk, no double buffering: the kernel is
//     held to two waves per SIMD (amdgpu_waves_per_eu(2, 2): 243 VGPRs at MT = 2, no scratch), so two workgroups share a CU
//     (26 KB of LDS each) and one stages while the other multiplies;
//   - fragments: B for output row o, tap (ky, kx) is the fragment of halo row o + ky at pixel offset kx.  A halo row's
//     fragment at a given kx is read ONCE and feeds the three taps ky (output rows ir, ir - 1, ir - 2): 54 LDS reads per chunk
//     and wave for up to 144 * MT MFMAs.  A for tap t is 16 bytes of the packed weights [9][C_out][C_in] at [t][channel l & 15]
//     [chunk * 32 + 8 (l >> 4)], read from L2 once per (workgroup, chunk, tap) and used for 16 pixel groups;
//   - accumulation order of an output element, fixed: chunks ascending; inside a chunk kx = 0, 1, 2; inside kx the halo rows
//     ascending (ky = 0, 1, 2); inside an MFMA the hardware's order over its 32 channels.  float32 throughout, no atomics:
//     the same inputs give the same bits on every run;
//   - epilogue: c = mf_round(acc, bias), then per variant
//       BIAS   out = mf_relu(c)
//       PAIR   BIAS with C_out = 2c written as two tensors [n, c, h, w]: channels < c -> out, channels >= c -> out2
//       GATES  channels < c: z = gru_gate(c, gz) -> z_out; channels >= c: gru_reset_value(c, gr, net) -> rnet_out
//       BLEND  out = gru_blend_value(z, c, gq, net); out may be net (a lane reads its own element before it writes it)
//     with the statements of gru_gates.h, the ones gru.hip's kernels evaluate.  A lane holds 4 consecutive channels of one
//     pixel; a store instruction writes 4 channel planes x 16 consecutive pixels.
// Built with -ffp-contract=off (the gate statements).  Resources from the cross-compile: profiles/conv3x3_resources.txt.
#include "conv_mfma.h"
#include "gru_gates.h"

namespace dba {

constexpr int CV_T = 16;                  // the tile's rows and columns
constexpr int CV_H = CV_T + 2;            // with the halo
constexpr int CV_HP = CV_H * CV_H;        // halo pixels: 324
constexpr int CV_ITEMS = CV_HP * (MF_KC / 8);                            // (pixel, 8 channels) items of a chunk
constexpr int CV_STAGE = (CV_ITEMS + MF_THREADS - 1) / MF_THREADS;       // per thread: 6

enum { CV_BIAS = 0, CV_GATES = 1, CV_BLEND = 2, CV_PAIR = 3 };

struct ConvArgs {
  const half_t *src0, *src1;   // [n, c0, h, w]; [n, c1_total, h, w], channels src1_first .. + c1
  int c0, c1, c1_total, src1_first;
  const half_t *w, *bias;      // [9][c_out][c0 + c1]; [c_out] or null
  int c_out, n, h, wd, tiles_x, tiles;
  half_t *out, *out2;          // BIAS, BLEND: out; GATES: z_out, rnet_out; PAIR: the two halves of c_out
  const half_t *g0, *g1;       // GATES: gz, gr [n, c]; BLEND: gq [n, c_out]
  const half_t *z, *net;       // BLEND: z; GATES, BLEND: net
  int c, relu;                 // GATES, PAIR: the channels of one output (c_out = 2c); BIAS, PAIR: relu
};

template <int MT, int EPI>
__global__ __launch_bounds__(MF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_kernel(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) half_t xs[CV_HP * MF_XS];
  const MfWave wv;
  const int r = wv.r, q = wv.q;
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty0 = (tile / a.tiles_x) * CV_T, tx0 = (tile - (tile / a.tiles_x) * a.tiles_x) * CV_T;
  const int HW = a.h * a.wd, c_in = a.c0 + a.c1;
  const int co0 = wv.co0(MT);
  const int rows = min(CV_T, a.h - ty0);                    // output rows of the tile inside the image (uniform)

  // where this thread's staging items lie: fixed over the chunks
  int s_lds[CV_STAGE], s_off[CV_STAGE];   // LDS half index; offset inside the chunk's planes, -1: zero
#pragma unroll
  for (int k = 0; k < CV_STAGE; ++k) {
    const int it = threadIdx.x + k * MF_THREADS;
    const int cg = it / CV_HP, p = it - cg * CV_HP;
    const int iy = p / CV_H, ix = p - iy * CV_H;
    const int gy = ty0 - 1 + iy, gx = tx0 - 1 + ix;
    const bool ok = it < CV_ITEMS && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
    s_lds[k] = it < CV_ITEMS ? p * MF_XS + cg * 8 : -1;
    s_off[k] = ok ? cg * 8 * HW + gy * a.wd + gx : -1;
  }

  float4v acc[CV_T][MT];
#pragma unroll
  for (int o = 0; o < CV_T; ++o) mf_zero(acc[o]);

  const half_t *wrow = a.w + (size_t)(co0 + r) * c_in + q * 8;   // + (tap * c_out + m * 16) * c_in + chunk * 32
  const size_t tap_stride = (size_t)a.c_out * c_in;

#pragma unroll 1
  for (int ch0 = 0; ch0 < c_in; ch0 += MF_KC) {
    const half_t *planes = ch0 < a.c0 ? a.src0 + ((size_t)img * a.c0 + ch0) * HW
                                      : a.src1 + ((size_t)img * a.c1_total + a.src1_first + (ch0 - a.c0)) * HW;
    half8 v[CV_STAGE];
#pragma unroll
    for (int k = 0; k < CV_STAGE; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = s_off[k] >= 0 ? planes[(size_t)s_off[k] + (size_t)j * HW] : (half_t)0.f;
    }
    __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
    for (int k = 0; k < CV_STAGE; ++k)
      if (s_lds[k] >= 0) *reinterpret_cast<half8 *>(&xs[s_lds[k]]) = v[k];
    __syncthreads();

#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      half8 wa[3][MT];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          wa[ky][m] = *reinterpret_cast<const half8 *>(wrow + (size_t)(ky * 3 + kx) * tap_stride + (size_t)(m * 16) * c_in + ch0);
#pragma unroll
      for (int ir = 0; ir < CV_H; ++ir) {
        if (ir >= rows + 2) continue;   // uniform: halo rows that only feed output rows outside the image
        const half8 xb = mf_fragment(xs, ir * CV_H + kx + r, q);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int o = ir - ky;
          if (o < 0 || o >= CV_T) continue;   // compile time
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ky][m], xb, acc[o][m], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: lane = pixel column r, channels co0 + m * 16 + 4q + i
  const int x = tx0 + r;
  if (x >= a.wd) return;
  float bf[MT][4], gt[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + m * 16 + 4 * q + i;
      bf[m][i] = mf_bias(a.bias, co);
      if (EPI == CV_GATES)
        gt[m][i] = co < a.c ? (float)a.g0[(size_t)img * a.c + co] : (float)a.g1[(size_t)img * a.c + (co - a.c)];
      else if (EPI == CV_BLEND)
        gt[m][i] = (float)a.g0[(size_t)img * a.c_out + co];
      else
        gt[m][i] = 0.f;
    }
#pragma unroll
  for (int o = 0; o < CV_T; ++o) {
    if (o >= rows) continue;   // uniform
    const int pix = (ty0 + o) * a.wd + x;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = co0 + m * 16 + 4 * q + i;
        const half_t c = mf_round(acc[o][m][i], bf[m][i]);
        if (EPI == CV_BIAS) {
          a.out[((size_t)img * a.c_out + co) * HW + pix] = mf_relu(c, a.relu);
        } else if (EPI == CV_PAIR) {
          half_t *dst = co < a.c ? a.out + ((size_t)img * a.c + co) * HW : a.out2 + ((size_t)img * a.c + (co - a.c)) * HW;
          dst[pix] = mf_relu(c, a.relu);
        } else if (EPI == CV_GATES) {
          if (co < a.c) {
            a.out[((size_t)img * a.c + co) * HW + pix] = (half_t)gru_gate<half_t>((float)c, gt[m][i]);
          } else {
            const size_t e = ((size_t)img * a.c + (co - a.c)) * HW + pix;
            a.out2[e] = gru_reset_value<half_t>((float)c, gt[m][i], (float)a.net[e]);
          }
        } else {
          const size_t e = ((size_t)img * a.c_out + co) * HW + pix;
          const float zz = (float)a.z[e], nn = (float)a.net[e];
          a.out[e] = gru_blend_value<half_t>(zz, (float)c, gt[m][i], nn);
        }
      }
  }
}

}  // namespace dba

using namespace dba;

namespace {

// the checks the three entry points share; fills the input half of the arguments
int cv_input(ConvArgs &a, const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first, const void *w,
             const void *bias, int c_out, int n, int h, int wd) {
  if (n <= 0 || h <= 0 || wd <= 0 || c0 <= 0 || c1 < 0 || c_out <= 0) return DBA_ERR_ARG;
  if (c0 % 32 || c1 % 32 || c_out % 64) return DBA_ERR_ARG;
  if (!src0 || !w) return DBA_ERR_ARG;
  if (c1 > 0 && (!src1 || src1_first < 0 || c1_total < c1 || src1_first > c1_total - c1)) return DBA_ERR_ARG;
  if (((uintptr_t)src0 | (uintptr_t)src1 | (uintptr_t)bias) & 1) return DBA_ERR_ARG;
  if ((uintptr_t)w & 15) return DBA_ERR_ARG;
  const long long hw = (long long)h * wd;
  const long long cmax = (long long)c0 + c1 > c_out ? (long long)c0 + c1 : c_out;
  if (hw * (cmax > c1_total ? cmax : c1_total) > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const long long tiles_x = (wd + CV_T - 1) / CV_T, tiles = tiles_x * ((h + CV_T - 1) / CV_T);
  if (!mf_grid_ok(tiles, n, c_out)) return DBA_ERR_ARG;
  a.src0 = (const half_t *)src0;
  a.src1 = (const half_t *)(c1 > 0 ? src1 : src0);
  a.c0 = c0;
  a.c1 = c1;
  a.c1_total = c1 > 0 ? c1_total : 0;
  a.src1_first = c1 > 0 ? src1_first : 0;
  a.w = (const half_t *)w;
  a.bias = (const half_t *)bias;
  a.c_out = c_out;
  a.n = n;
  a.h = h;
  a.wd = wd;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  return DBA_OK;
}

// a written tensor [n, c, h, w] must not share a byte with anything the launch reads through the halo
bool cv_clobbers(const ConvArgs &a, const void *dst, int c) {
  const size_t hw = (size_t)a.h * a.wd, bytes = (size_t)a.n * c * hw * 2;
  return ranges_overlap(dst, bytes, a.src0, (size_t)a.n * a.c0 * hw * 2) ||
         (a.c1 > 0 && ranges_overlap(dst, bytes, a.src1, (size_t)a.n * a.c1_total * hw * 2)) ||
         ranges_overlap(dst, bytes, a.w, (size_t)9 * a.c_out * (a.c0 + a.c1) * 2) ||
         ranges_overlap(dst, bytes, a.bias, (size_t)a.c_out * 2);
}

}  // namespace

extern "C" {

int dba_conv3x3_tile(void) { return CV_T; }

int dba_conv3x3_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first, const void *weight,
                    const void *bias, int c_out, int n, int h, int w, int relu, void *out, dba_stream_t stream) {
  ConvArgs a{};
  const int rc = cv_input(a, src0, c0, src1, c1, c1_total, src1_first, weight, bias, c_out, n, h, w);
  if (rc != DBA_OK) return rc;
  if (!out || ((uintptr_t)out & 1) || cv_clobbers(a, out, c_out)) return DBA_ERR_ARG;
  a.out = (half_t *)out;
  a.relu = relu != 0;
  return mf_launch<conv3x3_kernel<2, CV_BIAS>, conv3x3_kernel<1, CV_BIAS>>(a, (hipStream_t)stream);
}

int dba_conv3x3_pair_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first, const void *weight,
                         const void *bias, int c, int n, int h, int w, int relu, void *out0, void *out1, dba_stream_t stream) {
  if (c <= 0 || c > INT32_MAX / 2) return DBA_ERR_ARG;
  ConvArgs a{};
  const int rc = cv_input(a, src0, c0, src1, c1, c1_total, src1_first, weight, bias, 2 * c, n, h, w);
  if (rc != DBA_OK) return rc;
  if (!out0 || !out1 || (((uintptr_t)out0 | (uintptr_t)out1) & 1)) return DBA_ERR_ARG;
  const size_t bytes = (size_t)n * c * h * w * 2;
  if (cv_clobbers(a, out0, c) || cv_clobbers(a, out1, c) || ranges_overlap(out0, bytes, out1, bytes)) return DBA_ERR_ARG;
  a.out = (half_t *)out0;
  a.out2 = (half_t *)out1;
  a.c = c;
  a.relu = relu != 0;
  return mf_launch<conv3x3_kernel<2, CV_PAIR>, conv3x3_kernel<1, CV_PAIR>>(a, (hipStream_t)stream);
}

int dba_conv3x3_gates_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first,
                          const void *weight, const void *bias, const void *gz, const void *gr, const void *net, int c, int n,
                          int h, int w, void *z_out, void *rnet_out, dba_stream_t stream) {
  if (c <= 0 || c > INT32_MAX / 2) return DBA_ERR_ARG;
  ConvArgs a{};
  const int rc = cv_input(a, src0, c0, src1, c1, c1_total, src1_first, weight, bias, 2 * c, n, h, w);
  if (rc != DBA_OK) return rc;
  if (!gz || !gr || !net || !z_out || !rnet_out) return DBA_ERR_ARG;
  if (((uintptr_t)gz | (uintptr_t)gr | (uintptr_t)net | (uintptr_t)z_out | (uintptr_t)rnet_out) & 1) return DBA_ERR_ARG;
  const size_t bytes = (size_t)n * c * h * w * 2, gbytes = (size_t)n * c * 2;
  void *const outs[2] = {z_out, rnet_out};
  for (void *o : outs)
    if (cv_clobbers(a, o, c) || ranges_overlap(o, bytes, gz, gbytes) || ranges_overlap(o, bytes, gr, gbytes) ||
        ranges_overlap(o, bytes, net, bytes))
      return DBA_ERR_ARG;
  if (ranges_overlap(z_out, bytes, rnet_out, bytes)) return DBA_ERR_ARG;
  a.out = (half_t *)z_out;
  a.out2 = (half_t *)rnet_out;
  a.g0 = (const half_t *)gz;
  a.g1 = (const half_t *)gr;
  a.net = (const half_t *)net;
  a.c = c;
  return mf_launch<conv3x3_kernel<2, CV_GATES>, conv3x3_kernel<1, CV_GATES>>(a, (hipStream_t)stream);
}

int dba_conv3x3_blend_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first,
                          const void *weight, const void *bias, const void *gq, const void *z, const void *net, int c, int n,
                          int h, int w, void *out, dba_stream_t stream) {
  ConvArgs a{};
  const int rc = cv_input(a, src0, c0, src1, c1, c1_total, src1_first, weight, bias, c, n, h, w);
  if (rc != DBA_OK) return rc;
  if (!gq || !z || !net || !out) return DBA_ERR_ARG;
  if (((uintptr_t)gq | (uintptr_t)z | (uintptr_t)net | (uintptr_t)out) & 1) return DBA_ERR_ARG;
  const size_t bytes = (size_t)n * c * h * w * 2, gbytes = (size_t)n * c * 2;
  if (cv_clobbers(a, out, c) || ranges_overlap(out, bytes, gq, gbytes) || ranges_overlap(out, bytes, z, bytes)) return DBA_ERR_ARG;
  if (out != net && ranges_overlap(out, bytes, net, bytes)) return DBA_ERR_ARG;
  a.out = (half_t *)out;
  a.g0 = (const half_t *)gq;
  a.z = (const half_t *)z;
  a.net = (const half_t *)net;
  return mf_launch<conv3x3_kernel<2, CV_BLEND>, conv3x3_kernel<1, CV_BLEND>>(a, (hipStream_t)stream);
}

}  // extern "C"
