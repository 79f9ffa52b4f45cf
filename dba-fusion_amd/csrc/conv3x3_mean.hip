// GraphAgg's conv1 + ReLU + the mean over each frame's edges in ONE launch (include/dba_hip.h "3x3 convolution with the frame
// mean"; dbaf/droid_net.py:57-65):
//   dba_frame_members      <- the edges of every frame slot, ascending, from dba_frame_plan's inverse: one small launch
//   dba_conv3x3_mean_f16   <- scatter_mean(relu(conv1(x)), inverse, dim_size=F): the [n, C_out, h, w] tensor between
//                             dba_conv3x3_f16(relu) and dba_segment_reduce(mean) is never written
//
// conv3x3_mean_kernel: conv3x3.hip's kernel at MT = 1 with a second accumulator set.  One workgroup per (frame slot, 16 x 16
// tile, 64 output channels); blockIdx.x = slot * tiles + tile, blockIdx.y = the channel block.  For each member of its slot,
// ascending, the workgroup runs conv3x3_kernel's chunk loop in that kernel's accumulation order (chunks ascending; kx = 0, 1,
// 2; halo rows ascending; the hardware's order inside an MFMA), then the BIAS epilogue mf_relu(mf_round(acc, bias)): the half
// dba_conv3x3_f16 would store.  That half, as a float, is added to a float32 sum that starts at 0; after the last member
// sum / (float)max(count, 1), an IEEE division, is rounded once to half and stored to out[slot]: segment_reduce_kernel's
// arithmetic (csrc/upsample.hip) behind conv3x3's, so the bytes are those of the two launches.  No atomics, no scratch
// (profiles/conv3x3_mean_resources.txt); an empty slot writes zeros.
// What the kernel holds itself to, whatever the tables say: a workgroup whose slot is >= F returns; a slot's bounds are
// clamped to [0, n]; a member outside [0, n) is skipped.  So it reads seg_start[0 .. F], members[0 .. n), rows [0, n) of src
// and writes rows [0, F) of out, nothing else; the host refuses F > out_rows before any launch.
//
// frame_members_kernel: a stable counting sort by slot in one workgroup, without atomics.  The edges go by in rounds of 256,
// ascending; a thread's place inside its round is the number of earlier threads of the round with its slot, and the last
// thread of a slot in a round moves that slot's cursor.  The first pass counts, a scan makes seg_start, the second pass places.  Entries of
// inverse outside [0, F) belong to no slot (dba_segment_reduce ignores them in the same way); the tail of members behind
// seg_start[F] is -1.
// Built with -ffp-contract=off, as conv3x3.hip is.
#include "conv_mfma.h"

namespace dba {

constexpr int CM_T = 16;                  // conv3x3.hip's tile, halo and staging map
constexpr int CM_H = CM_T + 2;
constexpr int CM_HP = CM_H * CM_H;
constexpr int CM_ITEMS = CM_HP * (MF_KC / 8);
constexpr int CM_STAGE = (CM_ITEMS + MF_THREADS - 1) / MF_THREADS;
constexpr unsigned CM_ZERO = 0xffffffffu;   // a staging item outside the image
constexpr int FM_MAX_SLOTS = 4096;        // dba_frame_plan_max_rows(): a plan has no more frames

struct MeanArgs {
  const half_t *src;           // [n, c_in, h, w]
  const half_t *w, *bias;      // [9][c_out][c_in]; [c_out] or null
  int c_in, c_out, n, h, wd, tiles_x, tiles;
  const int *seg_start;        // [F + 1]
  const int *members;          // [n]
  int F;
  half_t *out;                 // [out_rows >= F, c_out, h, w]
};

__global__ __launch_bounds__(MF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_mean_kernel(const MeanArgs a) {
  __shared__ __attribute__((aligned(16))) half_t xs[CM_HP * MF_XS];
  const MfWave wv;
  const int r = wv.r, q = wv.q;
  const int slot = blockIdx.x / a.tiles, tile = blockIdx.x - slot * a.tiles;
  if (slot >= a.F) return;   // uniform
  const int ty0 = (tile / a.tiles_x) * CM_T, tx0 = (tile - (tile / a.tiles_x) * a.tiles_x) * CM_T;
  const int HW = a.h * a.wd, c_in = a.c_in;
  const int co0 = wv.co0(1);
  const int rows = min(CM_T, a.h - ty0);                    // output rows of the tile inside the image (uniform)
  const int j0 = min(max(a.seg_start[slot], 0), a.n), j1 = min(max(a.seg_start[slot + 1], 0), a.n);

  // LDS half index; BYTE offset inside the chunk's planes (below 2^32: the host holds c_in * h * w to 2^31 - 1), CM_ZERO: zero.
  // The plane of channel t is a uniform base, so a load is that base plus one 32-bit lane offset
  int s_lds[CM_STAGE];
  unsigned s_off[CM_STAGE];
#pragma unroll
  for (int k = 0; k < CM_STAGE; ++k) {
    const int it = threadIdx.x + k * MF_THREADS;
    const int cg = it / CM_HP, p = it - cg * CM_HP;
    const int iy = p / CM_H, ix = p - iy * CM_H;
    const int gy = ty0 - 1 + iy, gx = tx0 - 1 + ix;
    const bool ok = it < CM_ITEMS && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
    s_lds[k] = it < CM_ITEMS ? p * MF_XS + cg * 8 : -1;
    s_off[k] = ok ? 2u * (unsigned)(cg * 8 * HW + gy * a.wd + gx) : CM_ZERO;
  }

  float bf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bf[i] = mf_bias(a.bias, co0 + 4 * q + i);

  float4v sum[CM_T];
#pragma unroll
  for (int o = 0; o < CM_T; ++o) sum[o] = float4v{0.f, 0.f, 0.f, 0.f};
  int count = 0;

  const half_t *wrow = a.w + (size_t)(co0 + r) * c_in + q * 8;   // + tap * c_out * c_in + chunk * 32
  const size_t tap_stride = (size_t)a.c_out * c_in;

#pragma unroll 1
  for (int j = j0; j < j1; ++j) {
    const int img = a.members[j];
    if (img < 0 || img >= a.n) continue;   // uniform
    ++count;
    float4v acc[CM_T][1];
#pragma unroll
    for (int o = 0; o < CM_T; ++o) mf_zero(acc[o]);

#pragma unroll 1
    for (int ch0 = 0; ch0 < c_in; ch0 += MF_KC) {
      const half_t *planes = a.src + ((size_t)img * c_in + ch0) * HW;
      half8 v[CM_STAGE];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const char *plane = reinterpret_cast<const char *>(planes + (size_t)t * HW);   // uniform
#pragma unroll
        for (int k = 0; k < CM_STAGE; ++k)
          v[k][t] = s_off[k] != CM_ZERO ? *reinterpret_cast<const half_t *>(plane + s_off[k]) : (half_t)0.f;
      }
      __syncthreads();   // every wave is done with the previous chunk (of this member or of the one before)
#pragma unroll
      for (int k = 0; k < CM_STAGE; ++k)
        if (s_lds[k] >= 0) *reinterpret_cast<half8 *>(&xs[s_lds[k]]) = v[k];
      __syncthreads();

#pragma unroll 1   // rolled: unrolled over kx the schedule keeps more fragments in flight than fit beside two accumulator sets
      for (int kx = 0; kx < 3; ++kx) {
        half8 wa[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
          wa[ky] = *reinterpret_cast<const half8 *>(wrow + (size_t)(ky * 3 + kx) * tap_stride + ch0);
#pragma unroll
        for (int ir = 0; ir < CM_H; ++ir) {
          if (ir >= rows + 2) continue;   // uniform: halo rows that only feed output rows outside the image
          const half8 xb = mf_fragment(xs, ir * CM_H + kx + r, q);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int o = ir - ky;
            if (o < 0 || o >= CM_T) continue;   // compile time
            acc[o][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ky], xb, acc[o][0], 0, 0, 0);
          }
        }
      }
    }

    // the BIAS epilogue's half, added as a float in member order
#pragma unroll
    for (int o = 0; o < CM_T; ++o)
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[o][i] += (float)mf_relu(mf_round(acc[o][0][i], bf[i]), 1);
  }

  // ---- lane = pixel column r, channels co0 + 4q + i
  const int x = tx0 + r;
  if (x >= a.wd) return;
  const float cnt = (float)(count > 0 ? count : 1);
#pragma unroll
  for (int o = 0; o < CM_T; ++o) {
    if (o >= rows) continue;   // uniform
    const int pix = (ty0 + o) * a.wd + x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + 4 * q + i;
      a.out[((size_t)slot * a.c_out + co) * HW + pix] = (half_t)(sum[o][i] / cnt);
    }
  }
}

__global__ __launch_bounds__(256) void frame_members_kernel(const int64_t *__restrict__ inverse, int n, int F,
                                                            int *__restrict__ seg_start, int *__restrict__ members) {
  __shared__ int cursor[FM_MAX_SLOTS];   // pass 1: the slot's count; pass 2: where its next member goes
  __shared__ int round_slot[256];
  __shared__ int scan[256];
  const int t = threadIdx.x;
  for (int s = t; s < F; s += 256) cursor[s] = 0;
  __syncthreads();
  const int per = (F + 255) / 256;       // the scan: each thread owns `per` consecutive slots
  const int s0 = min(F, t * per), s1 = min(F, s0 + per);
  for (int pass = 0; pass < 2; ++pass) {
    for (int base = 0; base < n; base += 256) {
      const int e = base + t;
      const int64_t v = e < n ? inverse[e] : -1;
      const int s = (v >= 0 && v < F) ? (int)v : -1;
      round_slot[t] = s;
      __syncthreads();
      int before = 0, after = 0;
      if (s >= 0)
        for (int k = 0; k < 256; ++k) {
          const bool same = round_slot[k] == s;
          before += (same && k < t) ? 1 : 0;
          after += (same && k > t) ? 1 : 0;
        }
      const int at = s >= 0 ? cursor[s] + before : 0;
      __syncthreads();                          // every thread of the round has read its slot's cursor
      if (s >= 0) {
        if (pass == 1 && at < n) members[at] = e;   // at < seg_start[s + 1] <= n by the counts of pass 0; held anyway
        if (after == 0) cursor[s] = at + 1;     // one writer per slot and round: the slot's last thread
      }
      __syncthreads();
    }
    if (pass == 0) {
      int cnt = 0;
      for (int s = s0; s < s1; ++s) cnt += cursor[s];
      scan[t] = cnt;
      __syncthreads();
      for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
      }
      int off = scan[t] - cnt;
      for (int s = s0; s < s1; ++s) {
        const int c = cursor[s];
        seg_start[s] = off;
        cursor[s] = off;
        off += c;
      }
      const int total = scan[255];
      if (t == 0) seg_start[F] = total;
      for (int k = total + t; k < n; k += 256) members[k] = -1;   // behind the last slot: edges that belong to none
      __syncthreads();
    }
  }
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_frame_members_max_slots(void) { return FM_MAX_SLOTS; }

int dba_frame_members(const int64_t *inverse, int n, int F, int *seg_start, int *members, dba_stream_t stream) {
  if (n < 1 || F < 1 || F > FM_MAX_SLOTS) return DBA_ERR_ARG;
  if (!inverse || !seg_start || !members) return DBA_ERR_ARG;
  if (((uintptr_t)inverse & 7) || (((uintptr_t)seg_start | (uintptr_t)members) & 3)) return DBA_ERR_ARG;
  hipLaunchKernelGGL(frame_members_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, inverse, n, F, seg_start, members);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_conv3x3_mean_f16(const void *src, int c_in, const void *weight, const void *bias, int c_out, int n, int h, int w,
                         const int *seg_start, const int *members, int F, void *out, int out_rows, dba_stream_t stream) {
  // everything is decided here, on the arguments alone, before any call into the HIP runtime
  if (F < 1 || F > out_rows || n < 1) return DBA_ERR_ARG;
  if (!src || !weight || !seg_start || !members || !out) return DBA_ERR_ARG;
  if (h <= 0 || w <= 0 || c_in <= 0 || c_out <= 0 || c_in % 32 || c_out % 64) return DBA_ERR_ARG;
  if ((uintptr_t)weight & 15) return DBA_ERR_ARG;
  if (((uintptr_t)src | (uintptr_t)bias | (uintptr_t)out) & 1) return DBA_ERR_ARG;
  if (((uintptr_t)seg_start | (uintptr_t)members) & 3) return DBA_ERR_ARG;
  const long long hw = (long long)h * w;
  if (hw * (c_in > c_out ? c_in : c_out) > (long long)INT32_MAX) return DBA_ERR_ARG;   // an image's planes: int offsets
  const long long tiles_x = (w + CM_T - 1) / CM_T, tiles = tiles_x * ((h + CM_T - 1) / CM_T);
  if (!mf_grid_ok(tiles, F, c_out)) return DBA_ERR_ARG;
  const size_t out_bytes = (size_t)F * c_out * hw * 2;
  if (ranges_overlap(out, out_bytes, src, (size_t)n * c_in * hw * 2) ||
      ranges_overlap(out, out_bytes, weight, (size_t)9 * c_out * c_in * 2) ||
      ranges_overlap(out, out_bytes, bias, (size_t)c_out * 2) ||
      ranges_overlap(out, out_bytes, seg_start, ((size_t)F + 1) * 4) || ranges_overlap(out, out_bytes, members, (size_t)n * 4))
    return DBA_ERR_ARG;
  MeanArgs a{};
  a.src = (const half_t *)src;
  a.w = (const half_t *)weight;
  a.bias = (const half_t *)bias;
  a.c_in = c_in;
  a.c_out = c_out;
  a.n = n;
  a.h = h;
  a.wd = w;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  a.seg_start = seg_start;
  a.members = members;
  a.F = F;
  a.out = (half_t *)out;
  const dim3 grid((unsigned)(tiles * F), (unsigned)(c_out / 64));
  hipLaunchKernelGGL(conv3x3_mean_kernel, grid, dim3(MF_THREADS), 0, (hipStream_t)stream, a);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
