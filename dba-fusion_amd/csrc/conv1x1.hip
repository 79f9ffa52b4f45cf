// 1x1 (pointwise) convolutions of half tensors in the modules' NCHW layout as a GEMM on the matrix cores, and the ConvGRU's
// context chain behind one of them (include/dba_hip.h "1x1 convolutions"):
//   dba_conv1x1_f16          <- nn.Conv2d(C_in, C_out, 1)(x), optionally torch.relu behind it
//   dba_conv1x1_context_f16  <- glo = (sigmoid(w(net)) * net).view(b, c, h*w).mean(-1); convz_glo(glo), convr_glo(glo),
//                               convq_glo(glo)                                                (dbaf/modules/gru.py:24-29)
//
// conv1x1_kernel<MT, EPI>: conv_mfma.h's GEMM with N = 16 consecutive pixels of the flattened plane.
//   - tile: PW_P = 128 consecutive pixels of one image's plane; a wave holds 8 x MT accumulator tiles of 4 floats;
//   - staging: a chunk's 128 pixels.  Pixels at or beyond hw and channels at or beyond C_in (the last chunk of a C_in that is
//     no multiple of 32: 196) are zeros.  One buffer (10 KB), two barriers per chunk;
//   - fragments: B for pixel group o is the fragment of pixel 16 o + (l & 15); A is 16 bytes of the packed weights [C_out][Kp]
//     (Kp = C_in rounded up to 32, the tail zero) at [channel l & 15][chunk * 32 + 8 (l >> 4)], read from L2 once per (wave,
//     chunk) and used for the 8 pixel groups.  Both operands are zero in the tail of the last chunk, so a NaN or an infinity
//     there cannot arise;
//   - accumulation order of an output element, fixed: chunks ascending; inside an MFMA the hardware's order over its 32
//     channels.  float32 throughout, no atomics: the same inputs give the same bits on every run;
//   - epilogue: c = mf_round(acc, bias), then
//       BIAS     out = mf_relu(c)
//       CONTEXT  c is a = w(net) and is never stored.  p = h(h(sigmoid(a)) * net) per pixel, gru_gates.h's statements as
//                gru.hip's context kernel evaluates them.  A lane adds its p over the tile's pixel groups ascending (pixels
//                r, r + 16, ..), the 16 lanes of a row (one channel each row and register) fold on the DPP network (row_shr
//                1, 2, 4, 8 into lane 15), and lane 15 writes the float32 partial[image][tile][channel].
// conv1x1_context_tail_kernel: the second stage, one workgroup per image.  A thread owns a channel: s = the partials of the
//   image's tiles added in tile order; glo = half(s * float32(1 / hw)).  Then a thread owns one of the 3c outputs of the
//   concatenated *_glo weights [3c][c]: a float32 sum over the channels ascending (the products of two halves are exact in
//   float32), plus the bias, ONE rounding to half.
//   Why two launches and not one workgroup per image: an image's 128 channels x hw sigmoids on the four waves of one
//   workgroup are bound by the transcendental rate of a single CU, and 48-122 images leave more than half of the 256 CUs idle;
//   the split fills the chip with n * ceil(hw / 128) workgroups and costs one small launch.  The one-launch form was not
//   built, so the choice rests on this count, not on a measurement against it.
// Built with -ffp-contract=off (the gate statements).  Resources from the cross-compile: profiles/conv1x1_resources.txt.
#include "conv_mfma.h"
#include "gru_gates.h"

namespace dba {

constexpr int PW_P = 128;                 // pixels of a workgroup's tile
constexpr int PW_G = PW_P / 16;           // pixel groups of 16: N of one MFMA
constexpr int PW_STAGE = PW_P * (MF_KC / 8) / MF_THREADS;   // (pixel, 8 channels) items per thread: 2
constexpr int PW_CMAX = 1024;             // the context tail keeps glo of one image in LDS

enum { PW_BIAS = 0, PW_CONTEXT = 1 };

struct PwArgs {
  const half_t *x;             // [n, c_in, hw]
  const half_t *w, *bias;      // [c_out][kp], kp = ceil32(c_in), zero tail; [c_out] or null
  int c_in, kp, c_out, n, hw, tiles;
  half_t *out;                 // BIAS: [n, c_out, hw]
  float *partial;              // CONTEXT: [n, tiles, c_out]
  int relu;
};

template <int MT, int EPI>
__global__ __launch_bounds__(MF_THREADS) void conv1x1_kernel(const PwArgs a) {
  __shared__ __attribute__((aligned(16))) half_t xs[PW_P * MF_XS];
  const MfWave wv;
  const int r = wv.r, q = wv.q;
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int p0 = tile * PW_P;
  const int co0 = wv.co0(MT);

  // where this thread's staging items lie: fixed over the chunks
  int s_lds[PW_STAGE], s_cg[PW_STAGE], s_off[PW_STAGE];   // LDS half index; first channel inside the chunk; plane offset, -1: zero
#pragma unroll
  for (int k = 0; k < PW_STAGE; ++k) {
    const int it = threadIdx.x + k * MF_THREADS;
    const int cg = it / PW_P, p = it - cg * PW_P;
    s_lds[k] = p * MF_XS + cg * 8;
    s_cg[k] = cg * 8;
    s_off[k] = p0 + p < a.hw ? p0 + p : -1;
  }

  float4v acc[PW_G][MT];
#pragma unroll
  for (int o = 0; o < PW_G; ++o) mf_zero(acc[o]);

  const half_t *wrow = a.w + (size_t)(co0 + r) * a.kp + q * 8;   // + m * 16 * kp + chunk * 32
  const half_t *image = a.x + (size_t)img * a.c_in * a.hw;

#pragma unroll 1
  for (int ch0 = 0; ch0 < a.c_in; ch0 += MF_KC) {
    half8 v[PW_STAGE];
#pragma unroll
    for (int k = 0; k < PW_STAGE; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = ch0 + s_cg[k] + j;
        v[k][j] = (s_off[k] >= 0 && ch < a.c_in) ? image[(size_t)ch * a.hw + s_off[k]] : (half_t)0.f;
      }
    }
    half8 wa[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) wa[m] = *reinterpret_cast<const half8 *>(wrow + (size_t)(m * 16) * a.kp + ch0);
    __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
    for (int k = 0; k < PW_STAGE; ++k) *reinterpret_cast<half8 *>(&xs[s_lds[k]]) = v[k];
    __syncthreads();
#pragma unroll
    for (int o = 0; o < PW_G; ++o) {
      const half8 xb = mf_fragment(xs, o * 16 + r, q);
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[o][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[m], xb, acc[o][m], 0, 0, 0);
    }
  }

  // ---- epilogue: lane = pixel r of every group, channels co0 + m * 16 + 4q + i
  float bf[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[m][i] = mf_bias(a.bias, co0 + m * 16 + 4 * q + i);

  if (EPI == PW_BIAS) {
#pragma unroll
    for (int o = 0; o < PW_G; ++o) {
      const int pix = p0 + o * 16 + r;
      if (pix >= a.hw) continue;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = co0 + m * 16 + 4 * q + i;
          a.out[((size_t)img * a.c_out + co) * a.hw + pix] = mf_relu(mf_round(acc[o][m][i], bf[m][i]), a.relu);
        }
    }
  } else {
    float s[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) s[m][i] = 0.f;
#pragma unroll
    for (int o = 0; o < PW_G; ++o) {
      const int pix = p0 + o * 16 + r;
      if (pix >= a.hw) continue;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = co0 + m * 16 + 4 * q + i;   // c_out == c_in: the state's own channel
          const float av = (float)mf_round(acc[o][m][i], bf[m][i]);
          const float nn = (float)image[(size_t)co * a.hw + pix];
          s[m][i] += rnd<half_t>(rnd<half_t>(sigmoid_f32(av)) * nn);
        }
    }
    // every lane is back here: fold the 16 pixels of a row into its lane 15
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = s[m][i];
        t = dpp_add<0x111, 0xf>(t);  // row_shr:1
        t = dpp_add<0x112, 0xf>(t);  // row_shr:2
        t = dpp_add<0x114, 0xf>(t);  // row_shr:4
        t = dpp_add<0x118, 0xf>(t);  // row_shr:8
        if (r == 15) a.partial[((size_t)img * a.tiles + tile) * a.c_out + co0 + m * 16 + 4 * q + i] = t;
      }
  }
}

// partial [n, tiles, c] -> glo [n, c]; wg [3c][c], bg [3c] or null -> gz, gr, gq [n, c]
__global__ __launch_bounds__(MF_THREADS) void conv1x1_context_tail_kernel(const float *__restrict__ partial, int tiles, int c,
                                                                          float inv_hw, const half_t *__restrict__ wg,
                                                                          const half_t *__restrict__ bg, half_t *__restrict__ glo,
                                                                          half_t *__restrict__ gz, half_t *__restrict__ gr,
                                                                          half_t *__restrict__ gq) {
  __shared__ float gs[PW_CMAX];
  const int img = blockIdx.x;
  for (int ch = threadIdx.x; ch < c; ch += MF_THREADS) {
    const float *p = partial + (size_t)img * tiles * c + ch;
    float s = 0.0f;
    for (int t = 0; t < tiles; ++t) s += p[(size_t)t * c];
    const half_t h = (half_t)(s * inv_hw);
    glo[(size_t)img * c + ch] = h;
    gs[ch] = (float)h;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 3 * c; o += MF_THREADS) {
    const half8 *row = reinterpret_cast<const half8 *>(wg + (size_t)o * c);
    float acc = 0.0f;
    for (int k = 0; k < c / 8; ++k) {
      const half8 w8 = row[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += (float)w8[j] * gs[8 * k + j];
    }
    const half_t v = (half_t)(acc + (bg ? (float)bg[o] : 0.f));
    const int which = o / c, ch = o - which * c;
    half_t *dst = which == 0 ? gz : (which == 1 ? gr : gq);
    dst[(size_t)img * c + ch] = v;
  }
}

}  // namespace dba

using namespace dba;

namespace {

// the checks the two entry points share; fills the input half of the arguments
int pw_input(PwArgs &a, const void *x, int c_in, const void *w, const void *bias, int c_out, int n, int hw) {
  if (n <= 0 || hw <= 0 || c_in <= 0 || c_out <= 0 || c_out % 64) return DBA_ERR_ARG;
  if (!x || !w) return DBA_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)bias) & 1) return DBA_ERR_ARG;
  if ((uintptr_t)w & 15) return DBA_ERR_ARG;
  if (c_in > INT32_MAX - 31) return DBA_ERR_ARG;
  const long long cmax = c_in > c_out ? c_in : c_out;
  if ((long long)hw * cmax > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const long long tiles = ((long long)hw + PW_P - 1) / PW_P;
  if (!mf_grid_ok(tiles, n, c_out)) return DBA_ERR_ARG;
  a.x = (const half_t *)x;
  a.w = (const half_t *)w;
  a.bias = (const half_t *)bias;
  a.c_in = c_in;
  a.kp = (c_in + 31) / 32 * 32;
  a.c_out = c_out;
  a.n = n;
  a.hw = hw;
  a.tiles = (int)tiles;
  return DBA_OK;
}

// a written range must not share a byte with anything the launch reads
bool pw_clobbers(const PwArgs &a, const void *dst, size_t bytes) {
  return ranges_overlap(dst, bytes, a.x, (size_t)a.n * a.c_in * a.hw * 2) ||
         ranges_overlap(dst, bytes, a.w, (size_t)a.c_out * a.kp * 2) || ranges_overlap(dst, bytes, a.bias, (size_t)a.c_out * 2);
}

}  // namespace

extern "C" {

int dba_conv1x1_tile(void) { return PW_P; }

int dba_conv1x1_f16(const void *x, int c_in, const void *weight, const void *bias, int c_out, int n, int hw, int relu, void *out,
                    dba_stream_t stream) {
  PwArgs a{};
  const int rc = pw_input(a, x, c_in, weight, bias, c_out, n, hw);
  if (rc != DBA_OK) return rc;
  if (!out || ((uintptr_t)out & 1) || pw_clobbers(a, out, (size_t)n * c_out * hw * 2)) return DBA_ERR_ARG;
  a.out = (half_t *)out;
  a.relu = relu != 0;
  return mf_launch<conv1x1_kernel<2, PW_BIAS>, conv1x1_kernel<1, PW_BIAS>>(a, (hipStream_t)stream);
}

size_t dba_conv1x1_context_workspace_bytes(int n, int c, int hw) {
  if (n <= 0 || c <= 0 || hw <= 0) return 0;
  return (size_t)n * (size_t)((hw + PW_P - 1) / PW_P) * (size_t)c * sizeof(float);
}

int dba_conv1x1_context_f16(const void *net, const void *weight, const void *bias, const void *glo_weight, const void *glo_bias,
                            int c, int n, int hw, void *workspace, size_t workspace_bytes, void *glo, void *gz, void *gr,
                            void *gq, dba_stream_t stream) {
  if (c > PW_CMAX) return DBA_ERR_ARG;
  PwArgs a{};
  const int rc = pw_input(a, net, c, weight, bias, c, n, hw);
  if (rc != DBA_OK) return rc;
  if (!glo_weight || ((uintptr_t)glo_weight & 15) || ((uintptr_t)glo_bias & 1)) return DBA_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 3)) return DBA_ERR_ARG;
  if (workspace_bytes < dba_conv1x1_context_workspace_bytes(n, c, hw)) return DBA_ERR_WORKSPACE;
  void *const outs[4] = {glo, gz, gr, gq};
  const size_t gbytes = (size_t)n * c * 2, wsbytes = dba_conv1x1_context_workspace_bytes(n, c, hw);
  for (int i = 0; i < 4; ++i) {
    void *o = outs[i];
    if (!o || ((uintptr_t)o & 1) || pw_clobbers(a, o, gbytes) || ranges_overlap(o, gbytes, glo_weight, (size_t)3 * c * c * 2) ||
        ranges_overlap(o, gbytes, glo_bias, (size_t)3 * c * 2) || ranges_overlap(o, gbytes, workspace, wsbytes))
      return DBA_ERR_ARG;
    for (int j = i + 1; j < 4; ++j)
      if (ranges_overlap(o, gbytes, outs[j], gbytes)) return DBA_ERR_ARG;
  }
  if (pw_clobbers(a, workspace, wsbytes) || ranges_overlap(workspace, wsbytes, glo_weight, (size_t)3 * c * c * 2) ||
      ranges_overlap(workspace, wsbytes, glo_bias, (size_t)3 * c * 2))
    return DBA_ERR_ARG;
  a.partial = (float *)workspace;
  const int rl = mf_launch<conv1x1_kernel<2, PW_CONTEXT>, conv1x1_kernel<1, PW_CONTEXT>>(a, (hipStream_t)stream);
  if (rl != DBA_OK) return rl;
  hipLaunchKernelGGL(conv1x1_context_tail_kernel, dim3((unsigned)n), dim3(MF_THREADS), 0, (hipStream_t)stream,
                     (const float *)workspace, a.tiles, c, 1.0f / (float)hw, (const half_t *)glo_weight, (const half_t *)glo_bias,
                     (half_t *)glo, (half_t *)gz, (half_t *)gr, (half_t *)gq);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
