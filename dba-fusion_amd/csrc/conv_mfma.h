// What the matrix-core convolutions share (conv3x3.hip, conv1x1.hip): an implicit GEMM on mfma_f32_16x16x32_f16 with M = output
// channels (A = the packed weights), N = 16 pixels (B = the staged input), K = 32 input channels.  A workgroup of 4 waves owns
// a pixel tile of one image and 64 * MT output channels (MT = 2 when C_out is a multiple of 128, else 1); blockIdx.x = image *
// tiles + tile, blockIdx.y = the channel block.  The planes are pixel-contiguous and the MFMA wants 8 consecutive channels per
// lane, so the input is walked in chunks of 32 channels and a chunk's pixels go through LDS transposed: a thread takes one
// pixel and 8 channels (8 guarded 2-byte loads, neighbouring threads neighbouring pixels) and writes one 16-byte LDS vector;
// what the kernel's guard refuses is written as zero and never dereferenced.  That gather stays spelled out in each kernel:
// 3x3 guards on a precomputed offset, 1x1 on pixel and channel, and every shared form of it tried moved the register
// allocation of both.  The kernels also keep their own tiles, staging maps, loops and epilogue bodies; every result they store
// is rounded by mf_round and nowhere else.  conv7x7.hip (four input channels) uses the wave's place, the accumulators, the
// epilogue's statements and the launch; its K is a kernel row of 8 tap slots x 4 channels and its LDS image is its own.
// conv_enc.hip (the encoders: stride 1 or 2, C_out % 32 == 0, a 7x7 stem of three channels) uses the fragment, the epilogue's
// statements and the grid limits; its tiles, its division of a workgroup's waves and its launches are its own.
#pragma once
#include "common.h"

namespace dba {

typedef _Float16 half_t;
typedef half_t half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int MF_KC = 32;                 // channels per chunk: K of one MFMA
constexpr int MF_XS = MF_KC + 8;          // LDS row pitch in halves (80 bytes): two-way conflicts inside a ds_read_b128 lane group
constexpr int MF_THREADS = 256;

// a wave's place: wave g owns the channels co0 .. + 16 * MT of the workgroup's block for all the tile's pixels; in a fragment
// lane = 16 q + r holds pixel r, input channels 8q .. 8q + 7 (A, B) and output channels 4q .. 4q + 3 (the accumulator)
struct MfWave {
  int lane, g, r, q;
  __device__ __forceinline__ MfWave() : lane(threadIdx.x & 63), g(threadIdx.x >> 6), r(lane & 15), q(lane >> 4) {}
  __device__ __forceinline__ int co0(int mt) const { return blockIdx.y * (64 * mt) + g * (16 * mt); }   // the wave's first output channel
};

// the MT accumulator tiles of one pixel group
template <int MT>
__device__ __forceinline__ void mf_zero(float4v (&acc)[MT]) {
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = float4v{0.f, 0.f, 0.f, 0.f};
}

// B of one MFMA: the 16 bytes [pixel][channels 8q ..] of the staged chunk, one aligned ds_read_b128
__device__ __forceinline__ half8 mf_fragment(const half_t *xs, int pixel, int q) {
  return *reinterpret_cast<const half8 *>(&xs[pixel * MF_XS + q * 8]);
}

// the bias of output channel co in float32; no bias: zero
__device__ __forceinline__ float mf_bias(const half_t *bias, int co) { return bias ? (float)bias[co] : 0.f; }

// the convolution's value: float32 sum plus float32 bias, ONE rounding (what a stock half convolution stores)
__device__ __forceinline__ half_t mf_round(float acc, float b) { return (half_t)(acc + b); }

// torch.relu on the bits' meaning: NaN stays, -0 -> +0
__device__ __forceinline__ half_t mf_relu(half_t c, int relu) {
  const float cf = (float)c;
  return (relu && cf <= 0.f) ? (half_t)0.f : c;
}

// the launch grid's limits: x = tiles * n, y = c_out / 64 at most.  Beyond them a launch could never start
inline bool mf_grid_ok(long long tiles, int n, int c_out) { return tiles * n <= (long long)INT32_MAX && c_out / 64 <= 65535; }

// Wide (MT = 2) where c_out is a multiple of 128, else Narrow (MT = 1); the arguments carry tiles, n and c_out
template <auto Wide, auto Narrow, class Args>
int mf_launch(const Args &a, hipStream_t s) {
  const bool wide = a.c_out % 128 == 0;
  const dim3 grid((unsigned)(a.tiles * a.n), (unsigned)(a.c_out / (wide ? 128 : 64)));
  if (wide)
    hipLaunchKernelGGL(Wide, grid, dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(Narrow, grid, dim3(MF_THREADS), 0, s, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // namespace dba
